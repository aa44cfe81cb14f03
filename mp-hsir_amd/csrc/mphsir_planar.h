// Device-side primitives shared by the fp32 planar "data-side" kernels (scene, scene_d4, degrade, cassi, patch_sample, quality,
// quality_meter, spectral_loss, optim, arena): the ones whose exact semantics the project relies on -- the NaN rule of the min / max
// fold, the order of the float64 sums, the D4 tables -- each defined once.  A file of its own: the token kernels include mphsir_dev.h
// and do not grow by this.  (The float64 wave_sum lives beside the float one in mphsir_dev.h.)
#pragma once
#include <math.h>

#include "mphsir_dev.h"

namespace mphsir {

__device__ __forceinline__ float div_rn(float a, float b) {
#if defined(__HIP__)
    return __fdiv_rn(a, b);          // correctly rounded whatever the fast-math flags of the build
#else
    return a / b;
#endif
}

// comparisons, not fminf / fmaxf: a NaN stays a NaN (torch.clamp's rule; fminf / fmaxf would return the bound)
__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }
__device__ __forceinline__ f32x4 clamp01(f32x4 v) { return f32x4{clamp01(v[0]), clamp01(v[1]), clamp01(v[2]), clamp01(v[3])}; }
__device__ __forceinline__ double floor0(double v) { return v < 0.0 ? 0.0 : v; }
// false for +-inf and for a NaN.  One exact comparison with the largest finite double, no reliance on a classification builtin under
// any math flag.
__device__ __forceinline__ bool finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// torch's `reflect` for any integer coordinate (period 2(n-1)); n == 1 maps everything to 0
__device__ __forceinline__ int mirror(int y, int n) {
    if ((unsigned)y < (unsigned)n) return y;
    const int p = 2 * (n - 1);
    if (p == 0) return 0;
    int m = y % p;
    m = m < 0 ? m + p : m;
    return m < n ? m : p - m;
}

// the blend weight w(u) of include/mphsir.h for a tile at origin o of extent t on an axis of extent n; ovp1 = overlap + 1 (scene.hip on
// the two spatial axes, scene_bands.hip on the band axis as well)
__device__ __forceinline__ float ramp(int u, int o, int t, int n, float ovp1) {
    float w = 1.f;
    if (o > 0) w = fminf(w, (float)(u + 1) / ovp1);
    if (o + t < n) w = fminf(w, (float)(t - u) / ovp1);
    return w;
}

// The eight flip / rotation transforms of degrade.augment (mode m: rot90 counter-clockwise by m / 2, then an up-down flip when m is
// odd).  Every mode is one index map: element (u, v) of the transformed plane is element (a, b) of the plane with
//       (p, q) = transposing ? (v, u) : (u, v),   a = fy ? rows - 1 - p : p,   b = fx ? cols - 1 - q : q
//   mode        0  1  2  3  4  5  6  7
//   transposing .  .  x  x  .  .  x  x      (m >> 1) & 1; the plane is square
//   fy          .  x  .  .  x  .  x  x      FY
//   fx          .  .  x  .  x  x  .  x      FX
// and the inverse reads through the same map the other way round.
struct D4 {
    static constexpr unsigned FY = 0xD2u;    // bit m: mode m flips rows    (1, 4, 6, 7)
    static constexpr unsigned FX = 0xB4u;    // bit m: mode m flips columns (2, 4, 5, 7)
    bool tr, fy, fx;
    __device__ __forceinline__ explicit D4(int m) : tr((m >> 1) & 1), fy((FY >> m) & 1), fx((FX >> m) & 1) {}
    // the source position (sy, sx) of output position (oy, ox) in an H x W plane
    __device__ __forceinline__ void source(int oy, int ox, int H, int W, int& sy, int& sx) const {
        const int p = tr ? ox : oy, q = tr ? oy : ox;
        sy = fy ? H - 1 - p : p;
        sx = fx ? W - 1 - q : q;
    }
};

// min, max and NaN flag over a workgroup of NT threads; valid in every thread after the call.  Comparisons, so that a NaN is seen
// (by the flag) and not dropped; the wave folds by shuffles, the waves through LDS.  min / max are exact and commutative: the result
// does not depend on the order.
template <int NT> __device__ __forceinline__ void minmax_fold(float& mn, float& mx, float& bad, float (*red)[3]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float o0 = __shfl_xor(mn, m), o1 = __shfl_xor(mx, m), o2 = __shfl_xor(bad, m);
        mn = o0 < mn ? o0 : mn;
        mx = o1 > mx ? o1 : mx;
        bad = o2 > bad ? o2 : bad;
    }
    if (lane == 0) {
        red[wave][0] = mn;
        red[wave][1] = mx;
        red[wave][2] = bad;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        mn = red[w][0] < mn ? red[w][0] : mn;
        mx = red[w][1] > mx ? red[w][1] : mx;
        bad = red[w][2] > bad ? red[w][2] : bad;
    }
}

// a workgroup's {min, max} pair as it goes to the workspace: both NaN when flagged
__device__ __forceinline__ void minmax_store(float* o, float mn, float mx, float bad) {
    o[0] = bad != 0.f ? NAN : mn;
    o[1] = bad != 0.f ? NAN : mx;
}

// a sample's extremes from its n pairs in the workspace -> lo = min, den = max - min in every thread; a NaN pair fails both
// comparisons, so it is flagged on its own and poisons both
template <int NT> __device__ __forceinline__ void minmax_combine(const float* part, int n, float (*red)[3], float& lo, float& den) {
    float mn = INFINITY, mx = -INFINITY, bad = 0.f;
    for (int i = threadIdx.x; i < n; i += NT) {
        const float v0 = part[2 * i], v1 = part[2 * i + 1];
        mn = v0 < mn ? v0 : mn;
        mx = v1 > mx ? v1 : mx;
        bad = v0 != v0 ? 1.f : bad;
    }
    minmax_fold<NT>(mn, mx, bad, red);
    lo = bad != 0.f ? NAN : mn;
    den = bad != 0.f ? NAN : mx - mn;
}

// the four waves' float64 results p[0], p[stride], p[2 stride], p[3 stride] in wave order: no sum whose order depends on scheduling
__device__ __forceinline__ double sum4_ordered(const double* p, int stride) { return ((p[0] + p[stride]) + p[2 * stride]) + p[3 * stride]; }

// four neighbouring floats of which the first nv exist (the others read as 0 and are not stored): one 16-byte access when `vec` (then
// nv is 0 or 4), element by element otherwise -- the same elements, the same bits
__device__ __forceinline__ f32x4 load4_if(const float* p, bool vec, int nv) {
    if (vec) return nv ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < nv ? p[j] : 0.f;
    return v;
}
__device__ __forceinline__ void store4_if(float* p, f32x4 v, bool vec, int nv) {
    if (vec) {
        if (nv) *reinterpret_cast<f32x4*>(p) = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j < nv) p[j] = v[j];
}

}  // namespace mphsir
