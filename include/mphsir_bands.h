/* libmphsir -- C ABI, spectral windows for whole-scene inference.  An addition to include/mphsir.h (its conventions hold: device pointers
 * owned by the caller, a call only enqueues work on `stream` and returns 0 or a negative MPHSIR_E* code without launching anything,
 * capturable).  The surface of mphsir.h itself is frozen by count (tests/test_cabi.py), so these entry points live in a header of their
 * own, as include/mphsir_accum.h does; mp-hsir_amd/_lib.py reads all of them with the same parser.
 *
 * A scene of Cs bands goes through a model of C bands as windows along the spectral axis: what mphsir_scene_gather / _gather_d4 /
 * _blend do in space, with one more axis (mp-hsir_amd/scene.py, SceneRestorer(bands=C)).
 *
 * Definitions.  C: the model's band count; Cs: the scene's; ovb: the nominal band overlap, 0 <= ovb <= C / 2.
 *   Band plan (host; the multi-tile branch of scene.plan_axis with grain 1):
 *     Cs <= C: one window at band origin 0; its bands Cs .. C-1 are mirror padding, source band m(c, Cs) (m: the mirror map of
 *              mphsir_scene_gather, torch's `reflect`)
 *     Cs >  C: n = ceil((Cs - ovb) / (C - ovb)) windows at origins (i * (Cs - C)) / (n - 1): the first at 0, the last ending at Cs,
 *              strictly ascending, neighbours sharing at least ovb bands, at most 3 windows over any band
 *   Items.  A scene has N = nb * ny * nx items; item s = (ib * ny + iy) * nx + ix sits at (ob[ib], oy[iy], ox[ix]).  With G ensemble
 *     passes the work list is j = g * N + s, pass-major: the numbering of mphsir_scene_fold_d4 with n_tiles = N, which folds such
 *     items as it folds tiles; the store is [N][C][th][tw].
 *
 * mphsir_scene_gather_bands: tiles [count][C][th][tw] fp32; tiles[i] = mode_{g_j}(T_{s_j}), j = min(j0 + i, G * n_tiles - 1) (a batch
 *   that runs past the last item repeats it), and element (c, u, v) of T_s reads
 *       scene[m(ob_s + c, Cs)][m(oy_s + u, H)][m(ox_s + v, W)]
 *   with {ob_s, oy_s, ox_s} row s of `origins` (DEVICE int32 [n_tiles][3]; any triple is legal, negative, overhanging and repeated
 *   ones included: every coordinate is folded into the scene, so no access depends on the table holding a valid plan; values within
 *   +-2^30).  mode_m and modes_packed as for mphsir_scene_gather_d4; G = 1 with mode 0 is the plain cut.  A bitwise copy.
 *   0 <= j0 < G * n_tiles, 0 < count <= 65535, th and tw multiples of 4, a transposing mode needs th == tw, Cs > 0.
 * mphsir_scene_blend_bands: scene [Cs][H][W] fp32 from the nb * ny * nx restored items [s][C][th][tw] fp32 at the per-axis origins
 *   ob [nb], oy [ny], ox [nx] (DEVICE int32):
 *       scene[c][y][x] = sum(w * item) / sum(w)      over the items that cover (c, y, x), in ascending s, in fp32
 *       w = wb(c - ob) * wy * wx,   wy, wx the ramps of mphsir_scene_blend (ov + 1),   wb the same ramp on the band axis:
 *       wb(u) = min(1, (u + 1) / (ovb + 1) if ob > 0, (C - u) / (ovb + 1) if ob + C < Cs)
 *   The covering set is an outer product, so sum(w) = sum(wb) * sum(wy * wx); the launch divides by that product (the band sum in
 *   ascending ib, the pixel sum in ascending iy * nx + ix).  Item bands that map beyond Cs (the mirror padding) and item positions
 *   outside the scene are never read; an item is dereferenced only at local coordinates checked against [0,C) x [0,th) x [0,tw).
 *   No atomics, one thread per output element: bitwise reproducible.  clamp01 != 0 clamps the result to [0, 1].  An element that no
 *   item covers comes out NaN.  With nb = 1, ob = {0} and Cs == C the result is bitwise mphsir_scene_blend's (every band factor is
 *   1.0).  th, tw multiples of 4, tiles 16-byte aligned, 0 <= ov, ovb < 2^24.
 * Both launch under MPHSIR_K_SCENE (the launch timer reports the family): MPHSIR_K_COUNT stays.
 * Refused (MPHSIR_EINVAL, nothing launched): another struct_size, a null pointer, and every size outside the ranges above. */
#ifndef MPHSIR_BANDS_H
#define MPHSIR_BANDS_H
#include "mphsir.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mphsir_scene_gather_bands_args {
    uint32_t struct_size;       /* = sizeof(this struct), set by the caller: any other value is rejected with MPHSIR_EINVAL */
    const float* scene;
    const int32_t* origins;
    float* tiles;
    int32_t j0, count, n_tiles, G, modes_packed, C, Cs, H, W, th, tw;
} mphsir_scene_gather_bands_args;
int mphsir_scene_gather_bands(const mphsir_scene_gather_bands_args* a, void* stream);

typedef struct mphsir_scene_blend_bands_args {
    uint32_t struct_size;
    const float* tiles;
    const int32_t* ob;
    const int32_t* oy;
    const int32_t* ox;
    float* scene;
    int32_t nb, ny, nx, C, Cs, H, W, th, tw, ov, ovb, clamp01;
} mphsir_scene_blend_bands_args;
int mphsir_scene_blend_bands(const mphsir_scene_blend_bands_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
