#!/usr/bin/env python3
"""Writes the patch database train.py --db_path reads (data.bin + meta_info.txt, the reference's LMDB records in a flat file) from a
directory of cubes: the scene pyramid is built once on the GPU (mp-hsir_amd/scene_store.py), every grid record is cut out and min-max
normalised by ops.patch_sample in batches, and data.write_patch_db stores them in the reference's order.

    python tools/make_patch_db.py --scene_dir DIR --db_path OUT --data_type natural_scene [--patch_size 64] [--drop_degenerate 1]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401

from mp_hsir_amd.data import write_patch_db  # noqa: E402
from mp_hsir_amd.scene_store import SceneStore, scene_files  # noqa: E402


def export_patch_db(store, db_path, batch=256):
    """every record of `store`, in order, as one record of the patch database at db_path; -> the number of records written"""
    def patches():
        for p in store.patches(batch):
            yield from p.cpu().numpy()
    write_patch_db(db_path, patches(), store.names)
    return len(store)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene_dir", required=True)
    ap.add_argument("--db_path", required=True)
    ap.add_argument("--data_type", default="natural_scene", choices=["natural_scene", "remote_sensing"])
    ap.add_argument("--patch_size", type=int, default=64)
    ap.add_argument("--drop_degenerate", type=int, default=0)
    o = ap.parse_args()
    P = o.patch_size
    store = SceneStore(scene_files(o.scene_dir), o.data_type, "cuda", patch=P, strides=(P, P // 2, P // 2), drop_degenerate=bool(o.drop_degenerate))
    n = export_patch_db(store, o.db_path)
    print("%d records of %d x %d x %d written to %s (%d degenerate %s)" % (n, store.C, P, P, o.db_path, store.degenerate,
                                                                          "dropped" if o.drop_degenerate else "kept as NaN patches, as the reference does"))


if __name__ == "__main__":
    main()
