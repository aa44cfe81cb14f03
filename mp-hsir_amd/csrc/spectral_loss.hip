// Training loss with spectral terms: loss = L1 + w_sam SAM + w_sdiff SDIFF of `y` (restored) against `c` (clean), (B,C,H,W) fp32 each,
// and d loss / d y, in one launch pair (include/mphsir.h holds the definitions; mp-hsir_amd/ops.py, engine.SpectralLoss the Python side).
//
//   spectral_loss_kernel          a workgroup owns SL_PIX = 256 neighbouring pixels of one image, lane l of every wave the four pixels
//                                 4 l .. 4 l + 3 of them (one 16-byte access per plane where W % 4 == 0 and the pointers allow it, four
//                                 scalar ones otherwise: the same pixels, the same arithmetic, the same bits).  The cubes are planar, so a
//                                 thread walks bands at stride H W; the four waves take a quarter of the bands each (31 bands: 8, 8, 8, 7 --
//                                 a dependent chain of 8 loads instead of 31, and 512 workgroups at 32 x 31 x 64^2 instead of 128).
//                                 Walk 1 (statistics): per pixel sum x^2, sum c^2, sum (x - c)^2 of the wave's bands, and the thread's
//                                 sum |x - c| and sum |e| (e_k belongs to the wave that owns band k; it reads band k + 1 from the next
//                                 wave's quarter), all float64.  The per-pixel sums of the four waves meet in LDS and every wave adds them
//                                 in wave order, so all four hold the same theta, a, b of their pixels.
//                                 Walk 2 (gradient): the wave re-reads its bands (the workgroup's 256 x C x 8 bytes were just read:
//                                 cache-resident) and writes g = [(g_L1 + g_SDIFF) + (b x - a c)] m in fp32.
//                                 Wave 0 forms the angles and, with the waves' sums from LDS, the workgroup's three float64 partials.
//   spectral_loss_finish_kernel   one workgroup: the partials summed by thread in ascending block order, the lanes by a fixed shuffle tree,
//                                 the four waves in order; writes {loss, L1, SAM, SDIFF} as fp32, each rounded once.
//
// No atomics, no grid-wide wait, nothing zero-filled, no sum whose order depends on scheduling.
//
// Bounds: pixel p of image b, band k is element (b C + k) H W + p (64-bit); p < H W is checked per quad on the 16-byte path (H W % 4 == 0
// there: a quad never straddles the end of a plane) and per pixel on the scalar path; k < C.  A pixel outside the image is computed as
// y = c = 0, which adds 0 to every sum, and is never stored.  Workspace slot 3 blk + i, blk < B * blocks per image, lies inside the
// 24 * B * blocks bytes the host verified.
#include <math.h>

#include "mphsir_host.h"
#include "mphsir_planar.h"

// No multiply-add is fused in this file: whether a*b + c becomes one rounding or two would otherwise be the compiler's choice per
// instantiation, and the 16-byte path and the scalar path (and the CPU build the tests run) would differ in their last bits.
#pragma clang fp contract(off)

namespace mphsir {

constexpr int SL_NT = 256, SL_WAVES = SL_NT / 64;
constexpr int SL_PIX = 4 * 64;                      // pixels a workgroup owns: four per lane
static_assert(SL_WAVES == 4, "the ordered combines are written out for four waves");

struct SpectralLossDev {
    const float* y; const float* c; float* g; double* ws;
    long plane;                 // H * W
    int C, chunk, nbi;          // bands, bands per wave, workgroups per image
    int do_sam, do_sd;
    double sam_scale;           // w_sam / P
    float inv_n, inv_sd;        // 1 / (B C H W), w_sdiff / (B (C - 1) H W)
};

__device__ __forceinline__ float sl_sign(double v) { return v > 0.0 ? 1.f : (v < 0.0 ? -1.f : 0.f); }
// e = (x1 - x0) - (c1 - c0) in float64: the one expression both walks (and both waves that need an e at a quarter's edge) evaluate
__device__ __forceinline__ double sl_e(float x1, float x0, float c1, float c0) { return ((double)x1 - (double)x0) - ((double)c1 - (double)c0); }

// plane index of band k for a load that runs ahead of the walk: past the last band it repeats the last (in bounds, never used)
__device__ __forceinline__ long sl_band(int k, int C) { return k < C ? k : C - 1; }

// grid (B * nbi): workgroup blk owns pixels [(blk % nbi) * SL_PIX, + SL_PIX) of image blk / nbi
template <bool VEC> __global__ __launch_bounds__(SL_NT) void spectral_loss_kernel(SpectralLossDev a) {
    __shared__ double st[SL_WAVES][3][4][64];       // per-pixel sums of every wave: [wave][xx, cc, dd][pixel of the lane][lane]
    __shared__ double red[SL_WAVES][2];             // the waves' sum |x - c|, sum |e|

    const int lane = threadIdx.x & 63, wave = wave_id_uniform();
    const int b = blockIdx.x / a.nbi, bi = blockIdx.x - b * a.nbi;
    const long p0 = (long)bi * SL_PIX + 4 * lane;
    const long left = a.plane - p0;
    const int nv = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
    const int C = a.C;
    const int k0 = wave * a.chunk < C ? wave * a.chunk : C, k1 = k0 + a.chunk < C ? k0 + a.chunk : C;
    const long img = (long)b * C * a.plane + p0;                         // + k * plane
    const float* py = a.y + img;
    const float* pc = a.c + img;

    // ---- walk 1: statistics of bands [k0, k1) ----
    double sxx[4], scc[4], sdd[4], l1 = 0.0, sd = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) sxx[j] = scc[j] = sdd[j] = 0.0;
    if (k0 < k1) {
        // Two bands ahead of the arithmetic, without a branch around the loads (the band index is clamped to the image's last plane, a
        // repeated plane is never used): the chain of dependent loads is half as long as the quarter.  Band k + 1 is the next of this
        // quarter or -- for e_k alone -- the first of the next wave's.
        f32x4 x = clamp01(load4_if(py + sl_band(k0, C) * a.plane, VEC, nv)), c = load4_if(pc + sl_band(k0, C) * a.plane, VEC, nv);
        f32x4 xn = clamp01(load4_if(py + sl_band(k0 + 1, C) * a.plane, VEC, nv)), cn = load4_if(pc + sl_band(k0 + 1, C) * a.plane, VEC, nv);
        for (int k = k0; k < k1; ++k) {
            const f32x4 x2 = clamp01(load4_if(py + sl_band(k + 2, C) * a.plane, VEC, nv)), c2 = load4_if(pc + sl_band(k + 2, C) * a.plane, VEC, nv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double xv = x[j], cv = c[j], d = xv - cv;
                l1 += fabs(d);
                sxx[j] += xv * xv;
                scc[j] += cv * cv;
                sdd[j] += d * d;
            }
            if (a.do_sd && k + 1 < C) {
#pragma unroll
                for (int j = 0; j < 4; ++j) sd += fabs(sl_e(xn[j], x[j], cn[j], c[j]));
            }
            x = xn;
            c = cn;
            xn = x2;
            cn = c2;
        }
    }
    if (a.do_sam) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            st[wave][0][j][lane] = sxx[j];
            st[wave][1][j][lane] = scc[j];
            st[wave][2][j][lane] = sdd[j];
        }
    }
    l1 = wave_sum(l1);
    sd = wave_sum(sd);
    if (lane == 0) {
        red[wave][0] = l1;
        red[wave][1] = sd;
    }
    __syncthreads();

    // ---- per pixel: the sums of all bands in wave order, the angle (wave 0), the two scalars of the gradient ----
    float af[4], bf[4];
    double th = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) af[j] = bf[j] = 0.f;
    if (a.do_sam) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double X = sum4_ordered(&st[0][0][j][lane], 3 * 4 * 64), Cc = sum4_ordered(&st[0][1][j][lane], 3 * 4 * 64);
            const double D = sum4_ordered(&st[0][2][j][lane], 3 * 4 * 64);
            const double nx = sqrt(X), ny = sqrt(Cc);
            const bool has = nx != 0.0 && ny != 0.0;                         // true for a NaN: the loss becomes NaN
            const double dm = nx - ny, sp = nx + ny;
            const double s2 = floor0(D - dm * dm), t2 = floor0(sp * sp - D), h2 = s2 + t2;
            if (wave == 0 && has) th += 2.0 * atan2(sqrt(s2), sqrt(t2));
            const double sn = 2.0 * sqrt(s2 * t2) / h2, cs = (t2 - s2) / h2;  // sin, cos of theta = 2 atan2(sqrt s2, sqrt t2)
            if (has && finite(X) && finite(Cc) && finite(D) && sn >= MPHSIR_SAM_MIN_SIN) {
                af[j] = (float)(a.sam_scale / (sn * nx * ny));
                bf[j] = (float)(a.sam_scale * cs / (sn * X));
            }
        }
    }
    if (wave == 0) {
        th = wave_sum(th);
        if (lane == 0) {
            double* o = a.ws + 3 * (long)blockIdx.x;
            o[0] = sum4_ordered(&red[0][0], 2);
            o[1] = th;
            o[2] = sum4_ordered(&red[0][1], 2);
        }
    }
    if (a.g == nullptr || k0 >= k1) return;

    // ---- walk 2: the gradient of bands [k0, k1) ----
    float* pg = a.g + img;
    f32x4 yv = load4_if(py + sl_band(k0, C) * a.plane, VEC, nv), c = load4_if(pc + sl_band(k0, C) * a.plane, VEC, nv);
    f32x4 yn = load4_if(py + sl_band(k0 + 1, C) * a.plane, VEC, nv), cn = load4_if(pc + sl_band(k0 + 1, C) * a.plane, VEC, nv);
    f32x4 x = clamp01(yv);
    float sprev[4] = {0.f, 0.f, 0.f, 0.f};                                   // sign(e_{k-1})
    if (a.do_sd && k0 > 0) {
        const f32x4 xp = clamp01(load4_if(py + (long)(k0 - 1) * a.plane, VEC, nv)), cp = load4_if(pc + (long)(k0 - 1) * a.plane, VEC, nv);
#pragma unroll
        for (int j = 0; j < 4; ++j) sprev[j] = sl_sign(sl_e(x[j], xp[j], c[j], cp[j]));
    }
    for (int k = k0; k < k1; ++k) {
        const f32x4 y2 = load4_if(py + sl_band(k + 2, C) * a.plane, VEC, nv), c2 = load4_if(pc + sl_band(k + 2, C) * a.plane, VEC, nv);
        const f32x4 xn = clamp01(yn);
        f32x4 gv;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float se = (a.do_sd && k + 1 < C) ? sl_sign(sl_e(xn[j], x[j], cn[j], c[j])) : 0.f;
            const float gl1 = x[j] > c[j] ? a.inv_n : (x[j] < c[j] ? -a.inv_n : 0.f);
            const float gsd = (sprev[j] - se) * a.inv_sd;
            const float gsam = -(af[j] * c[j] - bf[j] * x[j]);
            gv[j] = (yv[j] >= 0.f && yv[j] <= 1.f) ? (gl1 + gsd) + gsam : 0.f;
            sprev[j] = se;
        }
        store4_if(pg + (long)k * a.plane, gv, VEC, nv);
        x = xn;
        yv = yn;
        c = cn;
        yn = y2;
        cn = c2;
    }
}

struct SpectralLossFinishDev {
    const double* ws; float* out;
    long nblk;
    double inv_n, inv_p, inv_sd, w_sam, w_sd;       // 1 / (B C H W), 1 / P, 1 / (B (C - 1) H W) or 0, the weights
};

__global__ __launch_bounds__(SL_NT) void spectral_loss_finish_kernel(SpectralLossFinishDev a) {
    __shared__ double red[SL_WAVES][3];
    const int t = threadIdx.x, lane = t & 63, wave = wave_id_uniform();
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (long i = t; i < a.nblk; i += SL_NT) {
        s0 += a.ws[3 * i];
        s1 += a.ws[3 * i + 1];
        s2 += a.ws[3 * i + 2];
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) {
        red[wave][0] = s0;
        red[wave][1] = s1;
        red[wave][2] = s2;
    }
    __syncthreads();
    if (t != 0) return;
    const double l1 = sum4_ordered(&red[0][0], 3) * a.inv_n;
    const double sam = a.w_sam != 0.0 ? sum4_ordered(&red[0][1], 3) * a.inv_p : 0.0;
    const double sdf = a.w_sd != 0.0 ? sum4_ordered(&red[0][2], 3) * a.inv_sd : 0.0;
    a.out[0] = (float)((l1 + a.w_sam * sam) + a.w_sd * sdf);
    a.out[1] = (float)l1;
    a.out[2] = (float)sam;
    a.out[3] = (float)sdf;
}

static long spectral_loss_blocks(int B, int C, int H, int W) {          // 0: sizes refused
    if (B < 1 || C < 1 || H < 1 || W < 1) return 0;
    const long plane = (long)H * W, nbi = (plane + SL_PIX - 1) / SL_PIX;
    return nbi * B < (1L << 31) ? nbi * B : 0;
}

}  // namespace mphsir

extern "C" int64_t mphsir_spectral_loss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    const long n = mphsir::spectral_loss_blocks(B, C, H, W);
    return n ? (int64_t)24 * n : MPHSIR_EINVAL;
}

extern "C" int mphsir_spectral_loss(const mphsir_spectral_loss_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "spectral_loss");
    MPHSIR_REQUIRE(a->y && a->clean && a->out && a->workspace, "spectral_loss: null pointer");
    const long nblk = spectral_loss_blocks(a->B, a->C, a->H, a->W);
    MPHSIR_REQUIRE(nblk > 0, "spectral_loss: bad sizes (B %d, C %d, H %d, W %d: each >= 1, at most 2^31 - 1 workgroups of 256 pixels)", a->B, a->C,
                   a->H, a->W);
    MPHSIR_REQUIRE(a->w_sam >= 0.f && a->w_sdiff >= 0.f && a->w_sam <= 3.4e38f && a->w_sdiff <= 3.4e38f,
                   "spectral_loss: the weights must be finite and >= 0 (w_sam %g, w_sdiff %g)", (double)a->w_sam, (double)a->w_sdiff);
    MPHSIR_REQUIRE(a->w_sam != 0.f || a->w_sdiff != 0.f, "spectral_loss: both weights are 0 -- that loss is mphsir_l1_clamp_loss");
    MPHSIR_REQUIRE(a->workspace_bytes >= 24 * nblk && (reinterpret_cast<uintptr_t>(a->workspace) & 7) == 0,
                   "spectral_loss: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)a->workspace_bytes, (long long)(24 * nblk));
    const long plane = (long)a->H * a->W;
    const double P = (double)a->B * (double)plane, n = P * (double)a->C;
    const double n_sd = a->C > 1 ? P * (double)(a->C - 1) : 0.0;
    const int do_sd = a->w_sdiff != 0.f && a->C > 1;
    SpectralLossDev d{a->y, a->clean, a->grad, static_cast<double*>(a->workspace), plane, a->C, (a->C + SL_WAVES - 1) / SL_WAVES,
                      (int)(nblk / a->B), a->w_sam != 0.f, do_sd, (double)a->w_sam / P, (float)(1.0 / n),
                      do_sd ? (float)((double)a->w_sdiff / n_sd) : 0.f};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (rows_aligned16(a->W, a->y, a->clean, a->grad))
        MPHSIR_LAUNCH(MPHSIR_K_SPECTRAL_LOSS, spectral_loss_kernel<true>, dim3((unsigned)nblk), dim3(SL_NT), 0, s, d);
    else
        MPHSIR_LAUNCH(MPHSIR_K_SPECTRAL_LOSS, spectral_loss_kernel<false>, dim3((unsigned)nblk), dim3(SL_NT), 0, s, d);
    SpectralLossFinishDev f{static_cast<const double*>(a->workspace), a->out, nblk, 1.0 / n, 1.0 / P, do_sd ? 1.0 / n_sd : 0.0,
                            (double)a->w_sam, do_sd ? (double)a->w_sdiff : 0.0};
    MPHSIR_LAUNCH(MPHSIR_K_SPECTRAL_LOSS_FINISH, spectral_loss_finish_kernel, dim3(1), dim3(SL_NT), 0, s, f);
    return MPHSIR_OK;
}
