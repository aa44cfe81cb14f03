// Scene quality in one pass: band-wise PSNR, band-wise SSIM and the mean spectral angle (SAM) of `restored` against `clean`,
// (B,C,H,W) fp32 each, in float64 (include/mphsir.h holds the definitions; mp-hsir_amd/metrics.py the Python side).
//
//   quality_partials   a workgroup owns Q_TH x Q_TW pixels of one image and walks the bands.  Per band it stages its pixels plus a
//                      3-pixel halo of both cubes in LDS (clipped to [0,1]; fp32 -> fp64 is exact, so the stage is fp32), forms the five
//                      7-wide row sums (x, y, xx, yy, xy) of every staged row in fp64 (LDS; a thread forms two neighbouring windows, which
//                      share six samples), then each thread adds 7 rows of them for the four window centres it owns (rows 3..6 are
//                      shared), evaluates SSIM there and adds (x - y)^2 of its own pixels.  The block's
//                      {sum ssim, sum (x-y)^2} of the band go to the workspace.  Across the band loop every thread keeps sum x^2,
//                      sum y^2, sum (x-y)^2 of its own pixels in registers; after the loop they become the pixel's angle and the
//                      block writes {sum angle, pixels counted}.
//   quality_finish     one wave per (image, band) and one per image: block partials summed by lane in ascending block order, the 64
//                      lane sums by a fixed shuffle tree; writes psnr, ssim, sam_deg, sam_pixels.
//
// No atomics, no sum whose order depends on scheduling: results are bitwise reproducible.  Window sums are plain 7-term sums (no
// running sums: nothing drifts).  Each cube is read once plus the halo ((Q_TH+6)(Q_TW+6) / (Q_TH Q_TW) = 1.41 of the cube, the
// halo mostly from L2); the next band's loads are issued before the current band's arithmetic and land in registers meanwhile, the
// stage is double-buffered so that a band costs two barriers.
//
// Bounds: every global read is at an image coordinate checked against [0,H) x [0,W) (positions outside are staged as 0 and only
// enter window sums that are never used); workspace slot (b, c, block) lies inside the 16 (C+1) blocks B bytes the host verified.
#include <math.h>

#include "mphsir_host.h"
#include "mphsir_planar.h"

namespace mphsir {

constexpr int Q_TW = 32, Q_TH = 32;                       // pixels a workgroup owns
constexpr int Q_R = 3;                                    // window radius: 7 x 7
constexpr int Q_SW = Q_TW + 2 * Q_R, Q_SH = Q_TH + 2 * Q_R;   // the stage
constexpr int Q_NT = 256;
constexpr int Q_RPT = Q_TH / (Q_NT / Q_TW);               // rows a thread owns in its column
constexpr int Q_LD = (Q_SW * Q_SH + Q_NT - 1) / Q_NT;     // staged elements per thread and cube
static_assert(Q_TW == 32 && Q_RPT == 4 && Q_R == 3, "thread map: 32 columns x 8 row groups of 4 rows; the shared window sums are written out for 7 rows");
typedef __attribute__((ext_vector_type(2))) double f64x2;

struct QualityDev {
    const float* x; const float* y; double* ws;
    int C, H, W, tiles_x, nblk;
};

// grid (blocks per image, B)
__global__ __launch_bounds__(Q_NT) void quality_partials_kernel(QualityDev a) {
    __shared__ float sx[2][Q_SH * Q_SW], sy[2][Q_SH * Q_SW];
    __shared__ double hs[5][Q_SH][Q_TW] __attribute__((aligned(16)));
    __shared__ double red[Q_NT / 64][2], red_sam[Q_NT / 64][2];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int blk = blockIdx.x, b = blockIdx.y;
    const int by = blk / a.tiles_x, bx = blk - by * a.tiles_x;
    const int y0 = by * Q_TH, x0 = bx * Q_TW;
    const long plane = (long)a.H * a.W;
    const float* px = a.x + (long)b * a.C * plane;
    const float* py = a.y + (long)b * a.C * plane;
    double* ws = a.ws + ((long)b * (a.C + 1) * a.nblk + blk) * 2;          // + c * nblk * 2

    int off[Q_LD];                                                          // plane offset of staged element t + k * Q_NT, -1 outside
#pragma unroll
    for (int k = 0; k < Q_LD; ++k) {
        const int e = t + k * Q_NT, r = e / Q_SW, c = e - r * Q_SW;
        const int gy = y0 - Q_R + r, gx = x0 - Q_R + c;
        off[k] = (e < Q_SW * Q_SH && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? gy * a.W + gx : -1;
    }
    const int tx = t & (Q_TW - 1), tg = t / Q_TW;
    bool pix[Q_RPT], win[Q_RPT];                                            // own pixel inside the image / a whole window around it
#pragma unroll
    for (int j = 0; j < Q_RPT; ++j) {
        const int gy = y0 + tg * Q_RPT + j, gx = x0 + tx;
        pix[j] = gy < a.H && gx < a.W;
        win[j] = gy >= Q_R && gy < a.H - Q_R && gx >= Q_R && gx < a.W - Q_R;
    }
    double axx[Q_RPT], ayy[Q_RPT], add[Q_RPT];
#pragma unroll
    for (int j = 0; j < Q_RPT; ++j) axx[j] = ayy[j] = add[j] = 0.0;

    float rx[Q_LD], ry[Q_LD];
#pragma unroll
    for (int k = 0; k < Q_LD; ++k) {
        rx[k] = off[k] >= 0 ? px[off[k]] : 0.f;
        ry[k] = off[k] >= 0 ? py[off[k]] : 0.f;
    }
    for (int c = 0; c < a.C; ++c) {
        float* bxs = sx[c & 1];
        float* bys = sy[c & 1];
#pragma unroll
        for (int k = 0; k < Q_LD; ++k) {
            const int e = t + k * Q_NT;
            if (e < Q_SW * Q_SH) {
                bxs[e] = clamp01(rx[k]);
                bys[e] = clamp01(ry[k]);
            }
        }
        if (c + 1 < a.C) {
            const float* nx = px + (long)(c + 1) * plane;
            const float* ny = py + (long)(c + 1) * plane;
#pragma unroll
            for (int k = 0; k < Q_LD; ++k) {
                rx[k] = off[k] >= 0 ? nx[off[k]] : 0.f;
                ry[k] = off[k] >= 0 ? ny[off[k]] : 0.f;
            }
        }
        __syncthreads();                     // the stage of band c is complete; everyone is done with hs and red of band c - 1
        if (t == 0 && c > 0) {
            double* o = ws + (long)(c - 1) * a.nblk * 2;
            o[0] = sum4_ordered(&red[0][0], 2);
            o[1] = sum4_ordered(&red[0][1], 2);
        }
        // row sums: staged row r, the windows centred on tile columns col and col + 1 share six of their seven samples
        for (int e = t; e < Q_SH * (Q_TW / 2); e += Q_NT) {
            const int r = e / (Q_TW / 2), col = (e - r * (Q_TW / 2)) * 2;
            const float* fx = bxs + r * Q_SW + col;
            const float* fy = bys + r * Q_SW + col;
            double xv[2 * Q_R + 2], yv[2 * Q_R + 2];
#pragma unroll
            for (int k = 0; k < 2 * Q_R + 2; ++k) {
                xv[k] = fx[k];
                yv[k] = fy[k];
            }
            double s0 = xv[1], s1 = yv[1], s2 = xv[1] * xv[1], s3 = yv[1] * yv[1], s4 = xv[1] * yv[1];
#pragma unroll
            for (int k = 2; k < 2 * Q_R + 1; ++k) {
                s0 += xv[k];
                s1 += yv[k];
                s2 += xv[k] * xv[k];
                s3 += yv[k] * yv[k];
                s4 += xv[k] * yv[k];
            }
            const double xa = xv[0], ya = yv[0], xb = xv[2 * Q_R + 1], yb = yv[2 * Q_R + 1];
            *reinterpret_cast<f64x2*>(&hs[0][r][col]) = f64x2{s0 + xa, s0 + xb};
            *reinterpret_cast<f64x2*>(&hs[1][r][col]) = f64x2{s1 + ya, s1 + yb};
            *reinterpret_cast<f64x2*>(&hs[2][r][col]) = f64x2{s2 + xa * xa, s2 + xb * xb};
            *reinterpret_cast<f64x2*>(&hs[3][r][col]) = f64x2{s3 + ya * ya, s3 + yb * yb};
            *reinterpret_cast<f64x2*>(&hs[4][r][col]) = f64x2{s4 + xa * ya, s4 + xb * yb};
        }
        __syncthreads();                     // hs of band c is complete
        double S[5][Q_RPT];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double v[Q_RPT + 2 * Q_R];
#pragma unroll
            for (int i = 0; i < Q_RPT + 2 * Q_R; ++i) v[i] = hs[q][tg * Q_RPT + i][tx];
            // the four windows of a thread share rows 3..6; plain sums of seven terms each, nothing is subtracted
            const double core = (v[3] + v[4]) + (v[5] + v[6]), a12 = v[1] + v[2], a78 = v[7] + v[8];
            S[q][0] = (v[0] + a12) + core;
            S[q][1] = (a12 + v[7]) + core;
            S[q][2] = (v[2] + a78) + core;
            S[q][3] = (a78 + v[9]) + core;
        }
        double ss = 0.0, dd = 0.0;
#pragma unroll
        for (int j = 0; j < Q_RPT; ++j) {
            const int e = (tg * Q_RPT + j + Q_R) * Q_SW + tx + Q_R;
            const double xv = bxs[e], yv = bys[e], d = xv - yv;            // 0 outside the image
            axx[j] += xv * xv;
            ayy[j] += yv * yv;
            add[j] += d * d;
            dd += d * d;
            const double inv = 1.0 / 49.0, cov = 49.0 / 48.0, c1 = 1e-4, c2 = 9e-4;
            const double ux = S[0][j] * inv, uy = S[1][j] * inv;
            const double vx = cov * (S[2][j] * inv - ux * ux), vy = cov * (S[3][j] * inv - uy * uy), vxy = cov * (S[4][j] * inv - ux * uy);
            const double s = ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
            if (win[j]) ss += s;
        }
        ss = wave_sum(ss);
        dd = wave_sum(dd);
        if (lane == 0) {
            red[wave][0] = ss;
            red[wave][1] = dd;
        }
    }
    // the angle of every own pixel: theta = 2 atan2(sqrt(d2 - (nx - ny)^2), sqrt((nx + ny)^2 - d2)); pixels without a norm are left out
    double th = 0.0, cnt = 0.0;
#pragma unroll
    for (int j = 0; j < Q_RPT; ++j) {
        const double nx = sqrt(axx[j]), ny = sqrt(ayy[j]);
        if (pix[j] && nx != 0.0 && ny != 0.0) {
            const double dm = nx - ny, sp = nx + ny;
            th += 2.0 * atan2(sqrt(floor0(add[j] - dm * dm)), sqrt(floor0(sp * sp - add[j])));
            cnt += 1.0;
        }
    }
    th = wave_sum(th);
    cnt = wave_sum(cnt);
    if (lane == 0) {
        red_sam[wave][0] = th;
        red_sam[wave][1] = cnt;
    }
    __syncthreads();
    if (t == 0) {
        double* o = ws + (long)(a.C - 1) * a.nblk * 2;
        o[0] = sum4_ordered(&red[0][0], 2);
        o[1] = sum4_ordered(&red[0][1], 2);
        o += (long)a.nblk * 2;
        o[0] = sum4_ordered(&red_sam[0][0], 2);
        o[1] = sum4_ordered(&red_sam[0][1], 2);
    }
}

struct QualityFinishDev {
    const double* ws; double* psnr; double* ssim; double* sam_deg; int64_t* sam_pixels;
    int C, H, W, nblk;
};

// grid (C + 1, B), one wave each: slot c < C is a band, slot C the image's angles
__global__ __launch_bounds__(64) void quality_finish_kernel(QualityFinishDev a) {
    const int c = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const double* p = a.ws + ((long)b * (a.C + 1) + c) * a.nblk * 2;
    double s0 = 0.0, s1 = 0.0;
    for (int i = lane; i < a.nblk; i += 64) {
        s0 += p[2 * (long)i];
        s1 += p[2 * (long)i + 1];
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if (lane != 0) return;
    if (c < a.C) {
        const double mse = s1 / ((double)a.H * (double)a.W);
        a.psnr[(long)b * a.C + c] = 10.0 * log10(1.0 / mse);
        a.ssim[(long)b * a.C + c] = s0 / ((double)(a.H - 2 * Q_R) * (double)(a.W - 2 * Q_R));
    } else {
        a.sam_deg[b] = s1 != 0.0 ? s0 / s1 * (180.0 / 3.14159265358979323846) : 0.0;
        a.sam_pixels[b] = (int64_t)s1;
    }
}

static bool quality_sizes_ok(int B, int C, int H, int W) {
    return B > 0 && B <= 65535 && C > 0 && C <= 65535 && H >= 2 * Q_R + 1 && W >= 2 * Q_R + 1 && (long)H * W < (1L << 31);
}
static long quality_blocks(int H, int W) { return (long)((H + Q_TH - 1) / Q_TH) * ((W + Q_TW - 1) / Q_TW); }

}  // namespace mphsir

extern "C" int64_t mphsir_quality_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    using namespace mphsir;
    if (!quality_sizes_ok(B, C, H, W)) return MPHSIR_EINVAL;
    return (int64_t)16 * (C + 1) * quality_blocks(H, W) * B;
}

extern "C" int mphsir_quality(const mphsir_quality_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "quality");
    MPHSIR_REQUIRE(a->restored && a->clean && a->psnr && a->ssim && a->sam_deg && a->sam_pixels && a->workspace, "quality: null pointer");
    MPHSIR_REQUIRE(a->H >= 2 * Q_R + 1 && a->W >= 2 * Q_R + 1, "quality: a band of %d x %d holds no 7 x 7 window", a->H, a->W);
    MPHSIR_REQUIRE(quality_sizes_ok(a->B, a->C, a->H, a->W), "quality: bad sizes (B %d, C %d, H %d, W %d; B, C <= 65535, H * W < 2^31)",
                   a->B, a->C, a->H, a->W);
    const int64_t need = mphsir_quality_workspace_bytes(a->B, a->C, a->H, a->W);
    MPHSIR_REQUIRE(a->workspace_bytes >= need && (reinterpret_cast<uintptr_t>(a->workspace) & 7) == 0,
                   "quality: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)a->workspace_bytes, (long long)need);
    const int tiles_x = (a->W + Q_TW - 1) / Q_TW;
    const long nblk = quality_blocks(a->H, a->W);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    QualityDev d{a->restored, a->clean, static_cast<double*>(a->workspace), a->C, a->H, a->W, tiles_x, (int)nblk};
    MPHSIR_LAUNCH(MPHSIR_K_QUALITY, quality_partials_kernel, dim3((unsigned)nblk, (unsigned)a->B), dim3(Q_NT), 0, s, d);
    QualityFinishDev f{static_cast<const double*>(a->workspace), a->psnr, a->ssim, a->sam_deg, a->sam_pixels, a->C, a->H, a->W, (int)nblk};
    MPHSIR_LAUNCH(MPHSIR_K_QUALITY, quality_finish_kernel, dim3((unsigned)(a->C + 1), (unsigned)a->B), dim3(64), 0, s, f);
    return MPHSIR_OK;
}
