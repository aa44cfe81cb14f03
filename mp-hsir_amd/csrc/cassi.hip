// The coded-aperture snapshot measurement (CASSI) of a clean batch, the reference's Degradation._sd_cassi (utils/degradation_utils.py:202-225;
// include/mphsir.h holds the definition):
//   mod[c,y,x] = clean[c,y,x] * M[my+y, mx+x];  meas[y,u] = sum over c, ascending, of mod[c,y,u-c*s];  out[c,y,x] = meas[y, x+c*s];
//   degraded = (out - min meas) / (max meas - min meas), under the sample's flip / rotation.
//
//   cassi_measure_kernel   a workgroup owns CS_ROWS rows of one sample's measurement: a thread owns columns u, walks the bands that reach u
//                          upward (a rounded product, then a rounded add, never one fma: the order and the rounding of the definition), writes meas to the
//                          workspace and folds it into a running min, max and NaN flag; the wave folds by shuffles, the four waves through
//                          LDS, thread 0 writes {min, max} of the block, both NaN when it holds one.  For a fixed band neighbouring lanes
//                          read neighbouring x of the cube and of the mask.
//   cassi_emit_kernel      a workgroup owns CE_ROWS OUTPUT rows of one (sample, band) plane: it combines the sample's block pairs (min /
//                          max are exact and commutative; a NaN pair poisons the result), computes every output pixel at its source
//                          position under the inverse of the sample's mode (D4::source) and writes whole rows of
//                          `degraded`, and of `clean_aug` when asked, as 16-byte vectors or element by element (uniform per launch).
//
// Two launches because the extremes are over the whole measurement of a sample; neither atomics nor a grid-wide wait.  meas holds
// Wm / W planes per sample (2.9 at C = 31, W = 64; 1.06 at W = 1024) against the C the pair reads and writes: the emit kernel reads
// it back through L2.  Under a transposing mode the emit kernel reads its sources along columns (CE_ROWS = 32 output rows are 32
// neighbouring source columns: every 128-byte line it touches is used whole by the workgroup) and still stores rows.
//
// Bounds.  my, mx and the mode come from device memory: my is clamped into [0, MH - H], mx into [0, MW - W] (the host has verified
// MH >= H, MW >= W), the mode is its low three bits.  Measure: y < H, 0 <= u - c s < W by the band range, u < Wm; block pair (b, blk)
// inside [B][nblk][2].  Emit: (sy, sx) inside the plane for every mode (a transposing mode has H == W, verified), sx + c s <= Wm - 1.
// All element offsets are 64-bit.
#include <math.h>

#include "mphsir_host.h"
#include "mphsir_planar.h"

#pragma clang fp contract(off)

namespace mphsir {

constexpr int CS_NT = 256;
constexpr int CS_ROWS = 4;           // measurement rows of a measure workgroup: 512 workgroups at 32 x 64 rows, 256 for one 1024-row scene
constexpr int CE_ROWS = 32;          // output rows of an emit workgroup

struct CassiDev {
    const float* clean; const float* mask; const int32_t* origin; const int32_t* task; const int32_t* aug;
    float* degraded; float* clean_aug; float* meas; float* part;
    int C, H, W, Wm, MH, MW, step, task_id, nblk, vec;
};

// The product and the sum of the definition, each rounded on its own.  Written as plain operators under the `fp contract(off)` above and
// not as __fmul_rn / __fadd_rn: the HIP headers define those as `a * b` / `a + b` inside the headers' own contraction mode, and once
// inlined the pair was fused into one v_fmac (seen in the gfx950 code, and as differing floats with a real-valued mask).
__device__ __forceinline__ float cs_mul(float a, float b) { return a * b; }
__device__ __forceinline__ float cs_add(float a, float b) { return a + b; }

// grid (nblk, B)
__global__ __launch_bounds__(CS_NT) void cassi_measure_kernel(CassiDev a) {
    __shared__ float red[CS_NT / 64][3];
    const int t = threadIdx.x;
    const int blk = blockIdx.x, b = blockIdx.y;
    if (a.task && a.task[b] != a.task_id) return;                 // uniform over the workgroup
    const int H = a.H, W = a.W, Wm = a.Wm, s = a.step;
    int my = a.origin ? a.origin[2 * b] : 0, mx0 = a.origin ? a.origin[2 * b + 1] : 0;
    my = my < 0 ? 0 : (my > a.MH - H ? a.MH - H : my);
    mx0 = mx0 < 0 ? 0 : (mx0 > a.MW - W ? a.MW - W : mx0);
    const int y0 = blk * CS_ROWS, rows = H - y0 < CS_ROWS ? H - y0 : CS_ROWS;
    const long plane = (long)H * W;
    const float* cube = a.clean + (long)b * a.C * plane;
    float* meas = a.meas + (long)b * H * Wm;
    float mn = INFINITY, mx = -INFINITY, bad = 0.f;
    for (int i = t; i < rows * Wm; i += CS_NT) {
        const int r = i / Wm, u = i - r * Wm, y = y0 + r;
        // the bands with 0 <= u - c s < W
        const int c0 = u < W ? 0 : (u - W) / s + 1;
        int c1 = u / s;
        c1 = c1 > a.C - 1 ? a.C - 1 : c1;
        const float* xp = cube + (long)c0 * plane + (long)y * W + (u - c0 * s);
        const float* mp = a.mask + (long)(my + y) * a.MW + mx0 + (u - c0 * s);
        float acc = 0.f;
        for (int c = c0; c <= c1; ++c) {
            acc = cs_add(acc, cs_mul(*xp, *mp));
            xp += plane - s;
            mp -= s;
        }
        meas[(long)y * Wm + u] = acc;
        mn = acc < mn ? acc : mn;
        mx = acc > mx ? acc : mx;
        bad = acc != acc ? 1.f : bad;
    }
    minmax_fold<CS_NT>(mn, mx, bad, red);
    if (t == 0) minmax_store(a.part + 2 * ((long)b * a.nblk + blk), mn, mx, bad);
}

// grid (ceil(H / CE_ROWS), C, B)
__global__ __launch_bounds__(CS_NT) void cassi_emit_kernel(CassiDev a) {
    __shared__ float red[CS_NT / 64][3];
    const int t = threadIdx.x;
    const int c = blockIdx.y, b = blockIdx.z;
    if (a.task && a.task[b] != a.task_id) return;
    float lo, den;
    minmax_combine<CS_NT>(a.part + 2 * (long)b * a.nblk, a.nblk, red, lo, den);      // the sample's extremes from its block pairs

    const int H = a.H, W = a.W, Wm = a.Wm;
    const D4 d4(a.aug ? a.aug[b] & 7 : 0);
    const long base = ((long)b * a.C + c) * H * W;
    const float* src = a.clean + base;
    const float* meas = a.meas + (long)b * H * Wm + c * a.step;
    float* od = a.degraded + base;
    float* oc = a.clean_aug ? a.clean_aug + base : nullptr;
    const int oy0 = blockIdx.x * CE_ROWS, rows = H - oy0 < CE_ROWS ? H - oy0 : CE_ROWS;
    // one output element: its source position under the inverse of the mode
    const auto element = [&](int oy, int ox, float& x) {
        int sy, sx;
        d4.source(oy, ox, H, W, sy, sx);
        if (oc) x = src[(long)sy * W + sx];
        return div_rn(meas[(long)sy * Wm + sx] - lo, den);
    };
    if (a.vec) {                                                  // uniform over the launch
        const int Q = W >> 2;
        for (int i = t; i < rows * Q; i += CS_NT) {
            const int r = i / Q, oy = oy0 + r, ox = 4 * (i - r * Q);
            f32x4 vd, vc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x = 0.f;
                vd[j] = element(oy, ox + j, x);
                vc[j] = x;
            }
            *reinterpret_cast<f32x4*>(od + (long)oy * W + ox) = vd;
            if (oc) *reinterpret_cast<f32x4*>(oc + (long)oy * W + ox) = vc;
        }
    } else {
        for (int i = t; i < rows * W; i += CS_NT) {
            const int r = i / W, oy = oy0 + r, ox = i - r * W;
            float x = 0.f;
            const float v = element(oy, ox, x);
            od[(long)oy * W + ox] = v;
            if (oc) oc[(long)oy * W + ox] = x;
        }
    }
}

// Wm = W + (C - 1) step; false for the shapes the pair refuses
static bool cassi_sizes_ok(long B, long C, long H, long W, long step, long& Wm) {
    if (B <= 0 || B > 65535 || C <= 0 || C > 65535 || H <= 0 || W <= 0 || step < 1 || step > 8) return false;
    Wm = W + (C - 1) * step;
    return H * W < (1L << 31) && H * Wm < (1L << 31) && B * C < (1L << 31);
}

}  // namespace mphsir

extern "C" int64_t mphsir_cassi_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t step) {
    long Wm;
    if (!mphsir::cassi_sizes_ok(B, C, H, W, step, Wm)) return MPHSIR_EINVAL;
    const int64_t meas = ((int64_t)B * H * Wm + 3) / 4 * 4, nblk = (H + mphsir::CS_ROWS - 1) / mphsir::CS_ROWS;
    return 4 * (meas + 2 * (int64_t)B * nblk);
}

extern "C" int mphsir_cassi(const mphsir_cassi_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "cassi");
    MPHSIR_REQUIRE(a->clean && a->mask && a->degraded && a->workspace, "cassi: null pointer");
    long Wm;
    MPHSIR_REQUIRE(a->step >= 1 && a->step <= 8, "cassi: step %d outside 1..8", a->step);
    MPHSIR_REQUIRE(cassi_sizes_ok(a->B, a->C, a->H, a->W, a->step, Wm),
                   "cassi: bad sizes (B %d, C %d in 1..65535; H %d, W %d with H * W, H * (W + (C - 1) step) and B * C below 2^31)", a->B, a->C, a->H, a->W);
    MPHSIR_REQUIRE(a->MH >= a->H && a->MW >= a->W && (long)a->MH * a->MW < (1L << 31), "cassi: a mask of %d x %d does not hold a plane of %d x %d", a->MH,
                   a->MW, a->H, a->W);
    MPHSIR_REQUIRE(a->H == a->W || !a->aug, "cassi: a plane of %d x %d is not square: aug must be NULL", a->H, a->W);
    MPHSIR_REQUIRE(a->degraded != a->clean && a->clean_aug != a->clean && a->clean_aug != a->degraded, "cassi: clean, degraded and clean_aug are distinct cubes");
    const int64_t need = mphsir_cassi_workspace_bytes(a->B, a->C, a->H, a->W, a->step);
    MPHSIR_REQUIRE(a->workspace_bytes >= need && aligned16(a->workspace), "cassi: workspace of %lld bytes, %lld needed (16-byte aligned)",
                   (long long)a->workspace_bytes, (long long)need);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int nblk = (a->H + CS_ROWS - 1) / CS_ROWS;
    const bool vec = rows_aligned16(a->W, a->clean, a->degraded, a->clean_aug);
    float* ws = static_cast<float*>(a->workspace);
    CassiDev d{a->clean, a->mask, a->origin, a->task, a->aug, a->degraded, a->clean_aug, ws, ws + ((int64_t)a->B * a->H * Wm + 3) / 4 * 4,
               a->C, a->H, a->W, (int)Wm, a->MH, a->MW, a->step, a->task_id, nblk, vec ? 1 : 0};
    MPHSIR_LAUNCH(MPHSIR_K_CASSI_MEASURE, cassi_measure_kernel, dim3((unsigned)nblk, (unsigned)a->B), dim3(CS_NT), 0, s, d);
    const dim3 grid((unsigned)((a->H + CE_ROWS - 1) / CE_ROWS), (unsigned)a->C, (unsigned)a->B);
    MPHSIR_LAUNCH(MPHSIR_K_CASSI_EMIT, cassi_emit_kernel, grid, dim3(CS_NT), 0, s, d);
    return MPHSIR_OK;
}
