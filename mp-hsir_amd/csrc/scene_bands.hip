// Spectral windows for whole-scene inference: the blend that folds the restored items of a scene of Cs bands, cut into windows of the
// model's C bands as well as into spatial tiles, back into the scene (include/mphsir_bands.h holds the definitions, mp-hsir_amd/scene.py
// the plan; the gather of such items is the d4 gather with one more folded coordinate and lives in scene_d4.hip).
//
//   bands_blend   scene [Cs][H][W] <- sum(w * item) / sum(w) over the covering items (ib, iy, ix), in ascending item number,
//                 w = wb * (wy * wx) with the ramp of mphsir_planar.h on all three axes
//
// A streaming kernel without LDS, laid out as scene.hip's blend: one thread owns 4 consecutive x of one row and walks a chunk of
// BANDS_CH OUTPUT bands.  Everything that depends on the band axis alone -- which windows hold a band of the chunk, the local band, the
// band ramp, its sum -- is a function of the workgroup's indices and of the origin array, the same in every lane: scalar work.  The
// covering set is an outer product, so the denominator is (sum of wb) * (sum of wy * wx): the four per-pixel sums of scene.hip's
// blend, taken while the first window that holds a band of the chunk is walked, and one factor per band, summed over the windows when
// the band is written (not carried through the loops: a float that is the same in every lane still costs a vector register here).
// With one window at origin 0 and Cs == C every band factor is exactly 1.0 and the arithmetic is scene.hip's, operation by operation.
//
// No access depends on the origin arrays holding a valid plan: an item is dereferenced only at a local band checked against [0,C) and
// local coordinates checked against [0,th) x [0,tw); item bands beyond Cs never correspond to an output band and are never read.
// Origins are expected within +-2^30, as in scene.hip.
#include "mphsir_host.h"
#include "mphsir_planar.h"
#include "../../include/mphsir_bands.h"

namespace mphsir {

// Output bands per thread.  Half of scene.hip's SCENE_CH: the band weights of a window are the same in every lane but are floats, which
// this target keeps in vector registers, one per band beside the accumulators; with 8 bands the kernel needs 94 registers, with 4 it
// stays within the 64 that leave 8 waves per SIMD.
constexpr int BANDS_CH = 4;

struct BandsBlendDev {
    const float* tiles; const int* ob; const int* oy; const int* ox; float* scene;
    int nb, ny, nx, C, Cs, H, W, th, tw, ov, ovb, clamp01;
};

// grid (ceil(H * ceil(W/4) / 256), ceil(Cs / BANDS_CH))
__global__ __launch_bounds__(256) void bands_blend_kernel(BandsBlendDev a) {
    const int W4 = (a.W + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.H * W4) return;
    const int y = idx / W4, x = (idx - y * W4) * 4;
    const int c0 = blockIdx.y * BANDS_CH;
    const int nc = a.Cs - c0 < BANDS_CH ? a.Cs - c0 : BANDS_CH;
    const long tplane = (long)a.th * a.tw;
    const float ovp1 = (float)(a.ov + 1), ovbp1 = (float)(a.ovb + 1);
    float num[BANDS_CH][4], den[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < BANDS_CH; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) num[c][k] = 0.f;
    bool first = true;                                            // the pixel sums are taken under the first window that is walked
    for (int ib = 0; ib < a.nb; ++ib) {
        const int ob = a.ob[ib];
        if (ob >= c0 + nc || ob <= c0 - a.C) continue;           // no band of the chunk in this window
        float wb[BANDS_CH];                                       // 0: the band is not in the window (and is never read)
#pragma unroll
        for (int c = 0; c < BANDS_CH; ++c) {
            const int u = c0 + c - ob;
            wb[c] = c < nc && (unsigned)u < (unsigned)a.C ? ramp(u, ob, a.C, a.Cs, ovbp1) : 0.f;
        }
        for (int iy = 0; iy < a.ny; ++iy) {
            const int oy = a.oy[iy], uy = y - oy;
            if ((unsigned)uy >= (unsigned)a.th) continue;
            const float wy = ramp(uy, oy, a.th, a.H, ovp1);
            for (int ix = 0; ix < a.nx; ++ix) {
                const int ox = a.ox[ix], vx = x - ox;              // tile column of the quad's first pixel
                if (vx <= -4 || vx >= a.tw) continue;
                float w[4];
                bool in[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    in[k] = (unsigned)(vx + k) < (unsigned)a.tw && x + k < a.W;
                    w[k] = in[k] ? wy * ramp(vx + k, ox, a.tw, a.W, ovp1) : 0.f;
                    if (first) den[k] += w[k];
                }
                // band c0 of this item at the quad; may lie before the item (a band below the window, up to 3 floats before a row):
                // read only at bands with wb != 0 and where in[k]
                const long at = (((long)(ib * a.ny + iy) * a.nx + ix) * a.C + (c0 - ob)) * tplane + (long)uy * a.tw + vx;
                const bool vec = in[0] && in[3] && (vx & 3) == 0;
#pragma unroll
                for (int c = 0; c < BANDS_CH; ++c) {
                    if (wb[c] != 0.f) {
                        const float* src = a.tiles + (at + c * tplane);
                        f32x4 t;
                        if (vec) {
                            t = *reinterpret_cast<const f32x4*>(src);
                        } else {
#pragma unroll
                            for (int k = 0; k < 4; ++k) t[k] = in[k] ? src[k] : 0.f;
                        }
#pragma unroll
                        for (int k = 0; k < 4; ++k) num[c][k] += (wb[c] * w[k]) * t[k];
                    }
                }
            }
        }
        first = false;
    }
    float* dst = a.scene + (long)c0 * a.H * a.W + (long)y * a.W + x;
#pragma unroll
    for (int c = 0; c < BANDS_CH; ++c) {
        if (c < nc) {
            float sb = 0.f;                                       // the band factor of the denominator: the sum of wb in ascending window
            for (int ib = 0; ib < a.nb; ++ib) {
                const int ob = a.ob[ib], u = c0 + c - ob;
                if ((unsigned)u < (unsigned)a.C) sb += ramp(u, ob, a.C, a.Cs, ovbp1);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (x + k < a.W) {
                    float r = num[c][k] / (sb * den[k]);
                    if (a.clamp01) r = fminf(fmaxf(r, 0.f), 1.f);
                    dst[(long)c * a.H * a.W + k] = r;
                }
            }
        }
    }
}

}  // namespace mphsir

extern "C" int mphsir_scene_blend_bands(const mphsir_scene_blend_bands_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "scene_blend_bands");
    MPHSIR_REQUIRE(a->tiles && a->ob && a->oy && a->ox && a->scene, "scene_blend_bands: null pointer");
    MPHSIR_REQUIRE(a->nb > 0 && a->ny > 0 && a->nx > 0 && a->C > 0 && a->Cs > 0 && a->H > 0 && a->W > 0,
                   "scene_blend_bands: bad sizes (nb %d, ny %d, nx %d, C %d, Cs %d, H %d, W %d)", a->nb, a->ny, a->nx, a->C, a->Cs, a->H, a->W);
    MPHSIR_REQUIRE(a->th > 0 && a->tw > 0 && a->th % 4 == 0 && a->tw % 4 == 0 && aligned16(a->tiles),
                   "scene_blend_bands: tile %d x %d must be multiples of 4 and the tile buffer 16-byte aligned", a->th, a->tw);
    MPHSIR_REQUIRE(a->ov >= 0 && a->ov < (1 << 24), "scene_blend_bands: overlap %d out of range", a->ov);
    MPHSIR_REQUIRE(a->ovb >= 0 && a->ovb < (1 << 24), "scene_blend_bands: band overlap %d out of range", a->ovb);
    const long quads = (long)a->H * ((a->W + 3) / 4), chunks = (a->Cs + BANDS_CH - 1) / BANDS_CH;
    MPHSIR_REQUIRE(quads < (1L << 30) && (long)a->nb * a->ny * a->nx < (1L << 24) && (long)a->th * a->tw < (1L << 30) && chunks <= 65535 &&
                       a->C < (1 << 24) && a->Cs < (1 << 24),
                   "scene_blend_bands: scene or tile too large");
    BandsBlendDev d{a->tiles, a->ob, a->oy, a->ox, a->scene, a->nb, a->ny, a->nx, a->C, a->Cs, a->H, a->W, a->th, a->tw, a->ov, a->ovb, a->clamp01};
    MPHSIR_LAUNCH(MPHSIR_K_SCENE, bands_blend_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)chunks), dim3(256), 0,
                  reinterpret_cast<hipStream_t>(stream), d);
    return MPHSIR_OK;
}
