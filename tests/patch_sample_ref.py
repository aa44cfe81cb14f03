"""Checks of mphsir_patch_sample (mp-hsir_amd/csrc/patch_sample.hip), scene_store.SceneStore and data.SceneStoreSource, written once and run
on the CPU emulator (tests/test_patch_sample_emu.py) and on the GPU (tests/test_patch_sample_gpu.py): `device` is "cpu" or "cuda".

The reference is the numpy restatement `numpy_patches`: (p - p.min()) / (p.max() - p.min()) on the float32 window, as the reference's
Data2Volume computes it (utils/image_utils.py:437-439).  The kernel must give the same FLOATS: equal where finite or infinite (== , so a
zero of either sign is a zero), NaN where numpy has NaN."""
import ctypes
import os
import sys

import numpy as np
import torch

from util import same_floats  # noqa: F401  (the tests reach it through this module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def numpy_patches(arena, levels, triples, C, P):
    """arena float32 (n,), levels [(offset, H, W)], triples [(level, y, x)] -> (B,C,P,P) float32"""
    out = []
    with np.errstate(all="ignore"):
        for l, y, x in triples:
            off, H, W = (int(v) for v in levels[l])
            p = arena[off:off + C * H * W].reshape(C, H, W)[:, y:y + P, x:x + P]
            assert p.shape == (C, P, P) and p.dtype == np.float32
            out.append((p - p.min()) / (p.max() - p.min()))
    return np.stack(out)


class Tables:
    """levels: list of (C,H,W) float32 arrays -> one arena (level starts padded to 4 elements; `shift` elements of slack in front, so that
    shift = 1 puts an aligned-width level on addresses that are not 16-byte aligned) and the level table, on `device`"""

    def __init__(self, levels, device, shift=0):
        self.C = levels[0].shape[0]
        offs, total = [], 0
        for lv in levels:
            assert lv.dtype == np.float32 and lv.shape[0] == self.C
            offs.append(total)
            total += (lv.size + 3) // 4 * 4
        self.host = np.full(total, np.float32(-9.0))
        for o, lv in zip(offs, levels):
            self.host[o:o + lv.size] = lv.reshape(-1)
        self.level_list = [(o, lv.shape[1], lv.shape[2]) for o, lv in zip(offs, levels)]
        self.levels_host = torch.tensor(self.level_list, dtype=torch.int64).reshape(-1, 3)
        assert self.levels_host.dtype == torch.int64                # the offsets are 64-bit by type, on the host and on the device
        whole = torch.full((total + shift,), -9.0, dtype=torch.float32, device=device)
        whole[shift:] = torch.from_numpy(self.host).to(device)
        self.arena = whole[shift:]
        assert self.arena.data_ptr() % 16 == (4 * shift) % 16
        self.levels = self.levels_host.to(device)
        self.device = device

    def run(self, triples, P, index=None):
        from mp_hsir_amd import ops
        rec = torch.tensor(triples, dtype=torch.int32, device=self.device).reshape(-1, 3)
        idx = None if index is None else torch.tensor(index, dtype=torch.int64, device=self.device)
        return ops.patch_sample(self.arena, self.levels, self.levels_host, rec, idx, self.C, P).cpu().numpy()

    def check(self, triples, P, index=None, label=""):
        got = self.run(triples, P, index)
        want = numpy_patches(self.host, self.level_list, triples if index is None else [triples[i] for i in index], self.C, P)
        assert same_floats(got, want), "%s: kernel differs from numpy at %d of %d elements" % (
            label, int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()), want.size)
        return got


def pyramid(cubes, scales=(1, .5, .25)):
    """the float32 levels of float64 cubes, scene then scale, built by scene_store.zoom_level"""
    from mp_hsir_amd import scene_store as S
    out = []
    for x in cubes:
        for s in scales:
            lv = torch.from_numpy(x) if s == 1 else S.zoom_level(torch.from_numpy(x), s)
            out.append(lv.numpy().astype(np.float32))
    return out


def grid(levels, P, stride):
    """every grid origin of every level, the last row and column of origins included; plus the window in the level's far corner"""
    out = []
    for l, lv in enumerate(levels):
        H, W = lv.shape[1:]
        out += [(l, y, x) for y in range(0, H - P + 1, stride) for x in range(0, W - P + 1, stride)]
        out.append((l, H - P, W - P))
    return out


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
def check_shapes(device, C):
    """P = 16; two scenes of different extent (C x 64 x 96 and C x 48 x 80) with their three levels each: six levels, six offsets; all grid
    records, the last row and column and the far corner of every level; B = 1 and B = 5 with repeated indices; a level that IS the window"""
    rs = np.random.RandomState(C)
    levels = pyramid([rs.rand(C, 64, 96), rs.rand(C, 48, 80)]) + [rs.rand(C, 16, 16).astype(np.float32)]
    assert [lv.shape[1:] for lv in levels] == [(64, 96), (32, 48), (16, 24), (48, 80), (24, 40), (12, 20), (16, 16)]
    levels = [lv for lv in levels if min(lv.shape[1:]) >= 16]
    t = Tables(levels, device)
    recs = grid(levels, 16, 16)
    assert (len(levels) - 1, 0, 0) in recs and len(recs) > 40
    for i in (0, len(recs) - 1, len(recs) // 2):
        t.check(recs, 16, index=[i], label="B = 1, record %d" % i)
    order = rs.permutation(len(recs)).tolist()
    for i in range(0, len(order) - 4, 5):
        idx = order[i:i + 5]
        idx[3] = idx[0]                                          # a repeated index
        t.check(recs, 16, index=idx, label="B = 5 at %d" % i)
    t.check(recs[:5], 16, label="per-sample triples")


def check_alignment(device):
    """a level of width 41 (no row but the first is 16-byte aligned) with origins at x = 0, 1, 2, 3, 25: the element-wise path; a level of
    width 48 at aligned origins: the 16-byte path; the same level with the whole arena moved by one element: element-wise again"""
    rs = np.random.RandomState(41)
    odd, even = rs.rand(3, 20, 41).astype(np.float32), rs.rand(3, 32, 48).astype(np.float32)
    for shift in (0, 1):
        t = Tables([odd, even], device, shift=shift)
        t.check([(0, y, x) for x in (0, 1, 2, 3, 25) for y in (0, 3, 4)], 16, label="width 41, shift %d" % shift)
        t.check([(1, y, x) for x in (0, 4, 16, 32) for y in (0, 5, 16)], 16, label="width 48 aligned origins, shift %d" % shift)
        t.check([(1, 2, x) for x in (1, 2, 3, 31)], 16, label="width 48 odd origins, shift %d" % shift)


def check_extremes(device):
    """the minimum and the maximum in different bands, each at the first and at the last element of the window (and of the last lane's
    last quad): a reduction that drops a lane, a band or the tail misses one of them"""
    rs = np.random.RandomState(7)
    C, P, y0, x0 = 5, 16, 2, 4
    for cmin, cmax in ((0, 4), (4, 0), (2, 3)):
        for first_is_min in (True, False):
            lv = (0.3 + 0.4 * rs.rand(C, 20, 24)).astype(np.float32)
            lv[:, :y0] = 5.0                                      # outside the window: must not enter the reduction
            lv[:, :, :x0] = -5.0
            a, b = (cmin, y0, x0), (cmax, y0 + P - 1, x0 + P - 1)
            if not first_is_min:
                a, b = (cmin, y0 + P - 1, x0 + P - 1), (cmax, y0, x0)
            lv[a], lv[b] = 0.125, 0.875
            for shift in (0, 1):
                got = Tables([lv], device, shift=shift).check([(0, y0, x0)], P, label="extremes %s" % ((cmin, cmax, first_is_min),))[0]
                assert got[a[0], a[1] - y0, a[2] - x0] == 0.0 and got[b[0], b[1] - y0, b[2] - x0] == 1.0
                assert got.min() == 0.0 and got.max() == 1.0


def check_nan_and_inf(device):
    rs = np.random.RandomState(9)
    C, P = 3, 16
    base = rs.rand(C, 16, 48).astype(np.float32)                  # three windows side by side: samples 0, 1, 2
    recs = [(0, 0, 0), (0, 0, 16), (0, 0, 32)]
    clean = Tables([base], device).check(recs, P, label="clean")
    for where in ((0, 3, 16 + 5), (C - 1, 15, 31)):               # band 0; the last element of the last band -- of sample 1
        lv = base.copy()
        lv[where] = np.nan
        got = Tables([lv], device).check(recs, P, label="NaN at %s" % (where,))
        assert np.isnan(got[1]).all(), "a NaN anywhere in the window makes the whole patch NaN"
        assert np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2]), "and only that sample's"
    lv = base.copy()
    lv[:, :, 16:32] = 0.25
    got = Tables([lv], device).check(recs, P, label="constant window")
    assert np.isnan(got[1]).all() and np.isfinite(got[0]).all()
    for v in (np.inf, -np.inf):
        lv = base.copy()
        lv[1, 7, 20] = v
        got = Tables([lv], device).check(recs, P, label="%s in the window" % v)
        assert np.isnan(got[1]).any() and np.isfinite(got[2]).all()
    lv = base.copy()
    lv[0, 0, 16], lv[2, 15, 31] = np.inf, -np.inf
    Tables([lv], device).check(recs, P, label="both infinities")


def check_reproducible(device):
    rs = np.random.RandomState(11)
    levels = pyramid([rs.rand(3, 64, 96)], scales=(1, .5))
    t = Tables(levels, device)
    recs = grid(levels, 16, 8)
    idx = rs.randint(0, len(recs), 5).tolist()
    one, two = t.run(recs, 16, idx), t.run(recs, 16, idx)
    assert one.tobytes() == two.tobytes()


def check_refusals(device):
    """wrong struct_size, P not a multiple of 4, P larger than a level, workspace too small: MPHSIR_EINVAL and nothing launched (out and
    the workspace keep their fill)"""
    import mp_hsir_amd._lib as L
    lib = L.load()
    rs = np.random.RandomState(13)
    t = Tables([rs.rand(3, 32, 48).astype(np.float32), rs.rand(3, 12, 40).astype(np.float32)], device)
    B, C, P = 2, 3, 8
    need = lib.mphsir_patch_sample_workspace_bytes(B, C)
    assert need == 8 * B * C and lib.mphsir_patch_sample_workspace_bytes(0, C) < 0 and lib.mphsir_patch_sample_workspace_bytes(B, 65536) < 0
    rec = torch.tensor([(0, 0, 0), (1, 4, 4)], dtype=torch.int32, device=device)
    out = torch.full((B, C, 16, 16), -7.0, device=device)
    ws = torch.full((need // 4,), -7.0, device=device)

    def args(**kw):
        a = L.PatchSampleArgs(arena=t.arena.data_ptr(), levels=t.levels.data_ptr(), levels_host=t.levels_host.data_ptr(), records=rec.data_ptr(),
                              index=None, out=out.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=need, arena_elems=t.arena.numel(),
                              n_levels=2, n_records=2, B=B, C=C, P=P)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, text):
        assert lib.mphsir_patch_sample(ctypes.byref(a), None) == -1
        assert text in lib.mphsir_last_error().decode(), lib.mphsir_last_error()
        if device == "cuda":
            torch.cuda.synchronize()
        assert float(out.min()) == -7.0 == float(out.max()) and float(ws.min()) == -7.0 == float(ws.max()), "something was launched"

    refused(args(struct_size=ctypes.sizeof(L.PatchSampleArgs) - 8), "struct_size")
    refused(args(P=6), "multiple of 4")
    refused(args(P=0), "multiple of 4")
    refused(args(P=16), "leaves level 1")                        # 16 > H = 12 of the second level
    refused(args(workspace_bytes=need - 1), "workspace")
    refused(args(arena_elems=t.arena.numel() - 1), "leaves the arena")
    refused(args(out=None), "null pointer")
    refused(args(levels_host=None), "null pointer")
    refused(args(B=65536), "bad sizes")
    refused(args(B=3), "records")                                # three samples, two per-sample records, no index
    assert lib.mphsir_patch_sample(ctypes.byref(args()), None) == 0
    if device == "cuda":
        torch.cuda.synchronize()
    got = out.reshape(-1)[:B * C * P * P].reshape(B, C, P, P).cpu().numpy()
    assert same_floats(got, numpy_patches(t.host, t.level_list, [(0, 0, 0), (1, 4, 4)], C, P))
    assert lib.mphsir_kernel_name(35) == b"patch_sample" and lib.mphsir_kernel_name(36) == b"patch_normalise"


def check_device_values_are_clamped(device):
    """index, level and origins come from device memory: out-of-range values are clamped into the tables, so the launch reads inside the
    arena and returns the clamped record's patch"""
    rs = np.random.RandomState(17)
    t = Tables([rs.rand(3, 20, 24).astype(np.float32), rs.rand(3, 16, 32).astype(np.float32)], device)
    got = t.run([(0, -5, 3), (0, 9, 100), (7, 0, 0), (-1, 2, 2)], 16)
    want = numpy_patches(t.host, t.level_list, [(0, 0, 3), (0, 4, 8), (1, 0, 0), (0, 2, 2)], 3, 16)
    assert same_floats(got, want)
    got = t.run([(0, 0, 0), (1, 0, 16)], 16, index=[-3, 99, 1])
    assert same_floats(got, numpy_patches(t.host, t.level_list, [(0, 0, 0), (1, 0, 16), (1, 0, 16)], 3, 16))


# ---- the store and the source -----------------------------------------------------------------------------------------------------------
TYPES = ["gaussianN", "inpaint", "bandmiss"]


def small_store(device, with_mask=True, patch=8, **kw):
    from mp_hsir_amd.scene_store import SceneStore
    rs = np.random.RandomState(23)
    a, b = rs.rand(31, 32, 48), rs.rand(31, 32, 32)
    mask = np.zeros((32, 48), dtype=bool)
    if with_mask:
        mask[10:14, 20:26] = True
    return SceneStore([(a, mask), b], "natural_scene", device, patch=patch, strides=(patch, patch // 2, patch // 2), crop_multiple=16,
                      sources=["ICVL_a.mat", "ARAD_b.mat"], **kw)


def check_store_against_numpy(device):
    """every record of a two-scene store through store.sample against numpy on the store's own arena; the record order is scene, scale, y, x"""
    st = small_store(device)
    rec = st.records_host
    assert rec.shape[1] == 3 and len(st) == len(st.names) and st.degenerate == 0
    key = [(int(l), int(y), int(x)) for l, y, x in rec]
    assert key == sorted(key) and set(st.names[:5]) == {"ICVL_a.mat"} and st.names[-1] == "ARAD_b.mat"
    assert 0 < len(st) < 24 + 15 + 2 + 16 + 9 + 1, "the mask removes some records"
    got = torch.cat(list(st.patches(batch=7))).cpu().numpy()
    want = numpy_patches(st.arena.cpu().numpy(), st.levels_host.tolist(), key, 31, 8)
    assert same_floats(got, want)


def check_source_equals_patch_db_source(device, tmp_path):
    """the store exported by tools/make_patch_db.export_patch_db and read back through PatchDBSource against SceneStoreSource, same seed, two
    epochs, world 1 and rank 1 of world 2: names, clean batches, prompts -- and with the tensor synthesiser the degraded batches -- equal"""
    from make_patch_db import export_patch_db
    from mp_hsir_amd.data import PatchDB, PatchDBSource, SceneStoreSource
    st = small_store(device)
    db_path = os.path.join(str(tmp_path), "db")
    assert export_patch_db(st, db_path, batch=16) == len(st)
    db = PatchDB(db_path, dataset_names=None)
    assert len(db) == len(st)
    for rank, world, fused in ((0, 1, False), (1, 2, False), (0, 1, True)):
        a = PatchDBSource(db, 4, TYPES, "natural_scene", device, seed=5, rank=rank, world=world, fused_degrade=fused)
        b = SceneStoreSource(st, 4, TYPES, "natural_scene", device, seed=5, rank=rank, world=world, fused_degrade=fused)
        assert a.steps_per_epoch() == b.steps_per_epoch() == len(st) // (4 * world)
        steps = 2 * a.steps_per_epoch() if not fused else 3
        for it in range(steps):
            (na, pa), da, ca, qa = a.next()
            (nb, pb), db_, cb, qb = b.next()
            assert na == nb, (rank, world, it)
            assert torch.equal(ca, cb) and torch.equal(qa, qb) and torch.equal(pa, pb), (rank, world, it)
            assert torch.equal(da, db_), (rank, world, it, fused)
            assert cb.shape == (4, 31, 8, 8) and float(cb.min()) == 0.0 and float(cb.max()) == 1.0


def check_jitter(device):
    """every jittered window lies inside its level and touches no mask pixel (recomputed on the host from the origins the source exposes);
    without a mask and with stride > 1 some origin leaves the grid; a window that would touch the mask keeps the record's origin"""
    from mp_hsir_amd.data import SceneStoreSource
    for with_mask in (True, False):
        st = small_store(device, with_mask=with_mask)
        src = SceneStoreSource(st, 8, TYPES, "natural_scene", device, seed=3, jitter=True)
        grid_rec = {tuple(int(v) for v in r) for r in st.records_host}
        levels = st.levels_host.tolist()
        moved = 0
        for _ in range(src.steps_per_epoch() + 1):
            _, deg, clean, prompt = src.next()
            org = src.last_origins.cpu().numpy()
            assert org.shape == (8, 3) and org.dtype == np.int32 and clean.shape == (8, 31, 8, 8)
            for l, y, x in org:
                _, H, W = levels[l]
                assert 0 <= y <= H - 8 and 0 <= x <= W - 8
                assert not st.masks[l][y:y + 8, x:x + 8].any()
                moved += (int(l), int(y), int(x)) not in grid_rec
            assert bool(torch.isfinite(clean).all())
        assert moved > 0
