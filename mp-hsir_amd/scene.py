"""Whole-scene restoration: a scene of any extent goes through the network as overlapping tiles and comes back whole.

The reference evaluates one forward over a cube centre-cropped to multiples of 64 (test.py / utils/image_utils.py:58-70) and has no
tiled path.  Here the scene stays as it is: `plan_tiles` lays tiles over it (host, pure Python), `mphsir_scene_gather` cuts a batch
of them on the device (mirror padding where a scene is smaller than one tile), the network restores the batch, and one
`mphsir_scene_blend` launch folds all restored tiles back with linear ramps across the overlaps (mp-hsir_amd/csrc/scene.hip).

Tile plan, per axis of extent H with requested tile T and nominal overlap ov:
    th = min(T, round_up(H, grain))
    H <= th: one tile at origin 0; its rows H..th-1 are mirror padding (source row 2(H-1) - y, at most grain - 1 < H of them)
    else:    n = ceil((H - ov) / (th - ov)) tiles at origins (i * (H - th)) // (n - 1): evenly spread, first at 0, last ending at H,
             neighbours overlapping by at least ov, nothing padded, at most 3 tiles over any pixel
The tiles of a scene are the outer product of the two axes, numbered iy * nx + ix.

Batching tiles is exact for this model, for a reason of its own: TVSP samples row floor(i * B / ps) of the (B,512) CLIP prompt, so
a sample's prompt map depends on the batch around it -- but when every sample of the batch carries the SAME task id all
B rows are equal and the map is the one a batch of 1 gets.  Every other operation of the network is per sample.  So one scene is one
task id, and a batch of mixed ids is refused.

Self-ensemble (`ensemble` = 4 or 8): every tile is restored under G flip / rotation transforms, each restoration is mapped back and
the G of them are averaged before the blend.  The transforms carry the numbers of the training augmentation -- degrade.augment, the
reference's data_augmentation: mode m = rot90 counter-clockwise m // 2 times, then an up-down flip when m is odd -- because those
are the eight views the weights were trained on, and the C ABI and the tests speak of the same numbers.  The network is not
equivariant under them (shifted windows, the depthwise 3x3 taps, the prompt stretch), which is why the mean differs from one
forward.  Work is the flat list of items j = g * n_tiles + t (pass g, tile t), walked in batches of `tile_batch` ACROSS passes:
`mphsir_scene_gather_d4` cuts and transforms a batch in one launch, the network restores it (one task id: as exact as a batch of
different tiles), `mphsir_scene_fold_d4` maps it back and accumulates the mean in the tile store itself (mp-hsir_amd/csrc/scene_d4.hip);
then the same one blend.  n_tiles * G items take ceil(n_tiles * G / tile_batch) forwards; nothing cube-sized is allocated per pass.

Spectral windows (`bands`): a band-limited model restores a scene of another band count through windows along the spectral axis, the
same mechanism with one more axis (include/mphsir_bands.h; resampling the cube to the model's bands would lose the sensor's own).
C is the model's band count, Cs the scene's, ovb the nominal band overlap, 0 <= ovb <= C // 2.
    Band plan (`plan_bands`): the multi-tile branch of `plan_axis` with grain 1.
        Cs <= C: one window at band origin 0; its bands Cs..C-1 are mirror padding, source band mirror(c, Cs)
        Cs >  C: n = ceil((Cs - ovb) / (C - ovb)) windows at origins (i * (Cs - C)) // (n - 1): first at 0, last ending at Cs, strictly
                 ascending, neighbours sharing at least ovb bands, at most 3 windows over any band
    Items: a scene has N = nb * ny * nx items; item s = (ib * ny + iy) * nx + ix sits at (ob[ib], oy[iy], ox[ix]).  With ensemble passes
        the work list is j = g * N + s, pass-major: what `mphsir_scene_fold_d4` already numbers, with n_tiles = N.  The store is
        [N][C][th][tw]; the fold and the ensemble-1 copy into it are the ones above.
    Gather (`mphsir_scene_gather_bands`): tiles[z][c][u][v] = mode_g(scene[mirror(ob + c, Cs)][mirror(oy + u', H)][mirror(ox + v', W)]).
    Blend (`mphsir_scene_blend_bands`): scene[c][y][x] = sum(w * tile) / sum(w) over the covering items in ascending s, with
        w = wb(c - ob) * wy * wx and wb the same ramp on the band axis (ovb + 1 in place of ov + 1); mirror-padded bands are never read.
One scene is still one task id, so a batch of items sees the prompt map a batch of one would see.  A window sees the WINDOW's spectral
attention, as a tile sees the tile's: a second instance of the same caveat.  A scene with Cs == C takes none of this: it issues exactly
the launches described above.
"""
import torch

from . import ops

ENSEMBLE_MODES = {1: (0,), 4: (0, 1, 4, 5), 8: (0, 1, 2, 3, 4, 5, 6, 7)}      # 4: the flips and the half turn, any tile shape; 8: needs th == tw
GRAINS = (32, 64)       # 64: what test.py crops to; 32: the network's own limit (8-pixel windows on the coarsest of its three 2x levels)


def _round_up(n, m):
    return (n + m - 1) // m * m


def plan_axis(H, T, ov, grain=64):
    """-> (tile extent th, [origins]) of one axis: see the module docstring.  ValueError for anything it does not cover."""
    if grain not in GRAINS:
        raise ValueError("grain %r: only %s are supported" % (grain, GRAINS))
    H, T, ov = int(H), int(T), int(ov)
    if T <= 0 or T % grain:
        raise ValueError("tile %d is not a positive multiple of %d" % (T, grain))
    if not 0 <= ov <= T // 2:
        raise ValueError("overlap %d outside [0, tile // 2 = %d]" % (ov, T // 2))
    if H < grain:
        raise ValueError("scene extent %d is smaller than %d" % (H, grain))
    th = min(T, _round_up(H, grain))
    if H <= th:
        return th, [0]
    n = -(-(H - ov) // (th - ov))
    return th, [(i * (H - th)) // (n - 1) for i in range(n)]


class TilePlan:
    """th, tw: tile extent; oy, ox: per-axis origins; origins: (oy, ox) of tile iy * nx + ix"""

    def __init__(self, H, W, th, tw, oy, ox, ov):
        self.H, self.W, self.th, self.tw, self.oy, self.ox, self.ov = H, W, th, tw, list(oy), list(ox), ov
        self.ny, self.nx = len(self.oy), len(self.ox)
        self.origins = [(y, x) for y in self.oy for x in self.ox]

    def __len__(self):
        return self.ny * self.nx


def plan_tiles(H, W, tile, ov, grain=64):
    th, oy = plan_axis(H, tile, ov, grain)
    tw, ox = plan_axis(W, tile, ov, grain)
    return TilePlan(int(H), int(W), th, tw, oy, ox, int(ov))


def plan_bands(Cs, C, ovb):
    """-> [band origins] of the windows of C bands over a scene of Cs bands: see the module docstring.  ValueError for an overlap
    outside [0, C // 2] (or a band count that is not positive)."""
    Cs, C, ovb = int(Cs), int(C), int(ovb)
    if Cs <= 0 or C <= 0:
        raise ValueError("band counts %d (scene), %d (model) must be positive" % (Cs, C))
    if not 0 <= ovb <= C // 2:
        raise ValueError("band overlap %d outside [0, bands // 2 = %d]" % (ovb, C // 2))
    if Cs <= C:
        return [0]
    n = -(-(Cs - ovb) // (C - ovb))
    return [(i * (Cs - C)) // (n - 1) for i in range(n)]


class SceneRestorer:
    """restorer(scene, task_id) -> restored scene: tiled inference with on-device gather and blend.

    net          MP_HSIR_Net, or any callable (x (B,C,th,tw) fp32, ids (B,) int64) -> (B,C,th,tw) fp32
    tile         requested tile extent.  Default 256: an extent the GPU suite already runs whole, and a 4x bilinear stretch of the
                 64x64 prompt map per side (the model is trained on 64x64 patches; TVSP resizes its prompt to whatever arrives)
                 instead of the 8x of a 512 cube.
    overlap      nominal overlap of neighbouring tiles, blended with linear ramps
    tile_batch   tiles per forward; the last batch of a scene is filled by repeating its last tile, so one shape serves them all
    graphed      an nn.Module is run through engine.GraphedForward (one capture for the one (tile_batch, C, th, tw) shape)
    grain        tile extents are multiples of it: 64 (test.py's crop granularity), or 32 (the network's own limit)
    ensemble     1: one forward per tile.  4 / 8: the mean over the transforms ENSEMBLE_MODES[ensemble] of degrade.augment's numbering
                 (the module docstring); 8 includes the quarter turns and needs square tiles (a ValueError at the first scene whose
                 plan has th != tw).  tile_batch then counts (transform, tile) items, packed across passes.
    bands        the model's band count C.  Default: for an nn.Module net.patch_embed.proj.weight.shape[1] (what its first convolution
                 takes); for any other callable None = the scene's own count.  A scene of another band count Cs goes through spectral
                 windows (the module docstring): ceil((Cs - ovb) / (C - ovb)) windows of C bands, or one mirror-padded window if
                 Cs < C, times the tiles; tile_batch then counts (transform, window, tile) items.  A scene of exactly C bands takes
                 the path it always took.
    band_overlap nominal overlap ovb of neighbouring windows in bands, 0 .. bands // 2, blended with the same linear ramps.  Default
                 bands // 4: the default of an option, not a tuned value -- its effect on quality is unmeasured (no trained
                 checkpoint), as is that of windows and of mirror-padded bands altogether.

    A tile sees the TILE's global spectral attention (the channel Gram is taken over the tile) and the tile's prompt stretch, not
    the scene's: tiled and whole-cube inference are two different functions of the input and are not expected to agree closely.
    A scene that is exactly one tile runs the same path with a batch of 1 and equals the plain forward bit for bit.
    The ensemble averages restorations of the same tile: a tile still sees its own spectral attention, under every transform.
    A spectral window sees the window's bands only, in its spectral attention as everywhere else.
    """

    def __init__(self, net, tile=256, overlap=32, tile_batch=4, graphed=True, grain=64, ensemble=1, bands=None, band_overlap=None):
        plan_axis(tile, tile, overlap, grain)        # argument check only (ValueError)
        if tile_batch < 1:
            raise ValueError("tile_batch %r" % (tile_batch,))
        if ensemble not in ENSEMBLE_MODES:
            raise ValueError("ensemble %r: 1 (off), 4 (flips and the half turn) or 8 (all flips and rotations)" % (ensemble,))
        self.tile, self.overlap, self.tile_batch, self.grain = tile, overlap, int(tile_batch), grain
        self.modes = ENSEMBLE_MODES[ensemble]
        if bands is None and isinstance(net, torch.nn.Module):
            bands = int(net.patch_embed.proj.weight.shape[1])
        if bands is None:
            if band_overlap is not None:
                raise ValueError("band_overlap %r without bands: a callable has no band count of its own" % (band_overlap,))
        else:
            bands = int(bands)
            band_overlap = bands // 4 if band_overlap is None else int(band_overlap)
            plan_bands(bands, bands, band_overlap)       # argument check only (ValueError)
        self.bands, self.band_overlap = bands, band_overlap
        if graphed and isinstance(net, torch.nn.Module):
            from .engine import GraphedForward
            net = GraphedForward(net)
        self.forward = net
        self._plans = {}           # (H, W, device) -> plan + its device origin arrays
        self._buffers = {}         # (plan key, C) -> static tile-batch input, task ids, restored-tile store
        self._band_plans = {}      # (Cs, H, W, device) -> the band origins and the item table of a scene that needs spectral windows

    def plan(self, H, W):
        return plan_tiles(H, W, self.tile, self.overlap, self.grain)

    def _device_plan(self, H, W, dev):
        key = (H, W, str(dev))
        e = self._plans.get(key)
        if e is None:
            p = self.plan(H, W)
            G = len(self.modes)
            if G == 8 and p.th != p.tw:
                raise ValueError("ensemble=8 turns tiles by 90 degrees and needs square tiles; a %d x %d scene under tile %d has %d x %d "
                                 "tiles: use ensemble=4 (the flips and the half turn)" % (H, W, self.tile, p.th, p.tw))
            B = min(self.tile_batch, len(p) * G)
            rows = p.origins + [p.origins[-1]] * (-len(p) % B)              # the tail batch repeats the last tile
            e = self._plans[key] = (p, B, torch.tensor(rows, dtype=torch.int32, device=dev).reshape(-1, 2),
                                    torch.tensor(p.oy, dtype=torch.int32, device=dev), torch.tensor(p.ox, dtype=torch.int32, device=dev))
        return e

    def _static_buffers(self, H, W, C, dev, B, p, Cs=None, n=None):
        """Cs, n: a scene under spectral windows -- its own band count joins the key, and the store holds n items of C bands"""
        key = (H, W, str(dev), C) if Cs is None else (H, W, str(dev), C, Cs)
        e = self._buffers.get(key)
        if e is None:
            self._buffers.clear()          # scenes of one shape follow each other; another shape releases the last one's store
            e = self._buffers[key] = (torch.empty((B, C, p.th, p.tw), dtype=torch.float32, device=dev),
                                      torch.empty((B,), dtype=torch.int64, device=dev),
                                      torch.empty((len(p) if n is None else n, C, p.th, p.tw), dtype=torch.float32, device=dev))
        return e

    def plan_bands(self, Cs):
        return plan_bands(Cs, self.bands, self.band_overlap)

    def _device_band_plan(self, Cs, H, W, dev):
        key = (Cs, H, W, str(dev))
        e = self._band_plans.get(key)
        if e is None:
            p, _, _, oy, ox = self._device_plan(H, W, dev)
            ob = self.plan_bands(Cs)
            rows = [(b, y, x) for b in ob for (y, x) in p.origins]          # item (ib * ny + iy) * nx + ix
            B = min(self.tile_batch, len(rows) * len(self.modes))
            e = self._band_plans[key] = (p, B, torch.tensor(rows, dtype=torch.int32, device=dev).reshape(-1, 3),
                                         torch.tensor(ob, dtype=torch.int32, device=dev), oy, ox)
        return e

    def _restore_windows(self, s3, task_id):
        """the scene's band count is not the model's: items are (window, tile) pairs, cut by the band gather at every ensemble setting"""
        Cs, H, W = s3.shape
        C, G = self.bands, len(self.modes)
        p, B, origins3, ob, oy, ox = self._device_band_plan(Cs, H, W, s3.device)
        n = origins3.shape[0]
        xin, ids, store = self._static_buffers(H, W, C, s3.device, B, p, Cs=Cs, n=n)
        ids.fill_(task_id)
        for k in range(0, n * G, B):               # items k .. k + B - 1 of the list j = g * n + s; a batch past the last repeats it
            ops.scene_gather_bands(s3, origins3, C, p.th, p.tw, k, self.modes, out=xin)
            y = self.forward(xin, ids)
            valid = min(B, n * G - k)
            if y.shape != xin.shape or y.dtype != torch.float32:
                raise RuntimeError("the network returned %s %s for tiles %s" % (tuple(y.shape), y.dtype, tuple(xin.shape)))
            if G == 1:
                store[k:k + valid].copy_(y[:valid])
            else:
                ops.scene_fold_d4(y.contiguous(), store, k, valid, self.modes)
        return ops.scene_blend_bands(store, ob, oy, ox, p.ov, self.band_overlap, Cs, H, W), store

    @torch.no_grad()
    def __call__(self, scene, task_id, return_tiles=False):
        """scene (C,H,W) or (1,C,H,W) fp32 on the GPU, task_id one int (or a 1-element tensor) -> restored, of the scene's shape.
        return_tiles (debugging): -> (restored, the (n,C,th,tw) restored tiles the blend read: the restorer's own store, overwritten
        by its next call)."""
        if torch.is_tensor(task_id):
            if task_id.numel() != 1:
                raise ValueError("one scene is restored under one task id (got %d): tiles are batched, and TVSP's prompt map is "
                                 "batch-invariant only when all samples of a batch share the id" % task_id.numel())
            task_id = int(task_id.reshape(-1)[0])
        if scene.dim() not in (3, 4) or (scene.dim() == 4 and scene.shape[0] != 1) or scene.dtype != torch.float32:
            raise ValueError("scene must be (C,H,W) or (1,C,H,W) fp32, got %s %s" % (tuple(scene.shape), scene.dtype))
        s3 = scene.reshape(scene.shape[-3:]).contiguous()
        C, H, W = s3.shape
        if self.bands is not None and C != self.bands:
            out, store = self._restore_windows(s3, int(task_id))
            out = out.reshape(scene.shape)
            return (out, store) if return_tiles else out
        p, B, origins, oy, ox = self._device_plan(H, W, s3.device)
        n = len(p)
        xin, ids, store = self._static_buffers(H, W, C, s3.device, B, p)
        ids.fill_(int(task_id))
        G = len(self.modes)
        for k in range(0, n * G, B):               # items k .. k + B - 1 of the list j = g * n + t; ensemble 1: the tiles themselves
            if G == 1:
                ops.scene_gather_tiles(s3, origins[k:k + B], p.th, p.tw, out=xin)
            else:
                ops.scene_gather_d4(s3, origins[:n], p.th, p.tw, k, self.modes, out=xin)
            y = self.forward(xin, ids)
            valid = min(B, n * G - k)
            if y.shape != xin.shape or y.dtype != torch.float32:
                raise RuntimeError("the network returned %s %s for tiles %s" % (tuple(y.shape), y.dtype, tuple(xin.shape)))
            if G == 1:
                store[k:k + valid].copy_(y[:valid])
            else:
                ops.scene_fold_d4(y.contiguous(), store, k, valid, self.modes)
        out = ops.scene_blend_tiles(store, oy, ox, p.ov, H, W).reshape(scene.shape)
        return (out, store) if return_tiles else out
