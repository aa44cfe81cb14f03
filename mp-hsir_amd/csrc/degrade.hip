// Training-batch degradation in one launch (include/mphsir.h holds the definitions; mp-hsir_amd/degrade.py the tensor functions whose
// element values these are).  clean [B][C][N][N] -> degraded, clean_aug, both under the sample's flip / rotation.
//
// One workgroup of 256 threads owns one (sample, band) plane.  The plane is staged once in LDS -- with a zero halo of k / 2 when the
// sample is a blur, so that the stencil walk has no bounds test -- and every OUTPUT pixel (oy, ox) is computed from the LDS plane at its
// source position (sy, sx) under the inverse of the sample's mode (D4::source): both outputs leave as whole rows,
// 256 bytes per wave and store, whatever the mode, and the clean cube is read once.  The kind, the mode and every per-sample parameter
// are uniform over the workgroup: scalar loads and scalar branches.
//
// LDS.  Row pitch = plane width | 1 (odd).  A wave writes 64 consecutive ox of one output row; in the source that is a row (stride 1:
// 64 consecutive dwords, one per bank) or, under a transposing mode, a column (stride = pitch: bank l * pitch mod 64, a permutation
// because the pitch is odd).  The stencil walk gives a thread four outputs along a source row (lanes 4 dwords apart along a row: with a
// pitch of 1 mod 4, as 85 for N = 64 with the largest halo, the 4 rows x 16 quads of a wave fall into 64 different banks; or a pitch apart
// along a column), and each tap shifts all 64 addresses alike -- the reads of the walk are conflict free in both cases.  The weights sit
// in LDS too (first version: scalar loads from global inside the tap loop -- 0.41 ms for a k = 21 plane, every tap waiting for its
// weight; now 2 k + 3 LDS reads per 4 k fmas).
// Budget: N = 64 with the 21 x 21 halo is 84 x 85 x 4 = 27.9 KiB + 4 KiB for the 32 x 32 low-resolution image of `sr` (the weights of a
// blur sample use the same region): five workgroups = 20 waves per CU by LDS; N = 128 is 86 + 16 KiB, one workgroup per CU.
//
// Draws: explicit (three cubes, read at the source index) or one Philox4x32-10 call per source element (counter = the element's linear
// index and the batch ordinal), so a draw does not depend on the launch geometry or on the mode.  The 32 x 32 -> high-word product is a
// 64-bit multiply in plain C++.  Contraction is off for the whole file: x + z * sigma and the like are a product and a sum, each rounded,
// as the tensor program computes them; the stencil and the bicubic taps ask for their fma by name.
//
// The tiled form (degrade_planes_kernel, mphsir_degrade_planes): planes of any H x W.  One workgroup owns one 64 x 64 OUTPUT tile of one
// plane (right and bottom tiles partial); under the inverse of the sample's mode that is a 64 x 64 rectangle of the source, staged in LDS
// with a halo of k / 2 that holds the real neighbours inside the plane and zero outside it -- the layout, the odd pitch (64 + 2 h) | 1
// and the weights in LDS are the plane form's at N = 64, and so is the budget: 27.9 + 4 KiB with the 21 x 21 halo, five workgroups =
// 20 waves per CU by LDS (<= 96 registers); without a blur in the menu 16.3 KiB, and the eight waves per SIMD bound it.  Every element
// goes through the device functions the plane form uses (dg_blur_quad, dg_sr_pixel, dg_draws, dg_value), so for a plane that both accept
// the two outputs are bitwise equal.  `sr`: the low-resolution pixels under the tile take their taps at the coordinates of the WHOLE
// plane, a footprint that drifts away from the tile as the plane grows: they are read from global memory (L2: 16 taps per f x f outputs),
// so no value depends on the tile grid.  W % 4 == 0 and 16-byte aligned cubes (an instance of their own, VEC): the tile is staged with
// dwordx4 loads and both outputs leave as dwordx4 stores (a stencil's under the modes that do not transpose).  Bound by HBM for every kind but the large stencils
// (441 fmas per output: the vector ALU) and gaussianN / complexN with generated draws (ten Philox rounds, log, cos: the vector ALU).
#include "mphsir_host.h"
#include "mphsir_planar.h"
#include <type_traits>

#pragma clang fp contract(off)

namespace mphsir {

constexpr int DG_NT = 256;
constexpr int DG_SS = MPHSIR_DEG_STENCIL_SIDE;

struct DegradeDev {
    const float* clean; float* degraded; float* clean_aug;
    const int* task; const int* aug; const float* param; const int* sub;
    const float* band_sigma; const uint8_t* band_flag; const uint8_t* col_dead; const float* col_off;
    const float* stencils; const float* cirrus; const float* atm; const float* haze_ratio;
    const float* z; const float* u0; const float* u1;
    const long long* ordinal_dev;
    unsigned long long seed; long long ordinal;
    int C, N, T, K, F, low_off;
    int H, W, ntx, nty;                                 // the tiled form: the plane and its tile grid
    int menu[MPHSIR_DEG_MAX_TASKS], ksize[MPHSIR_DEG_MAX_STENCILS], factor[MPHSIR_DEG_MAX_FACTORS];
};

struct Philox4 { uint32_t r[4]; };

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ float dg_unit(uint32_t r) { return (float)(r >> 8) * 5.9604644775390625e-08f; }       // [0, 1), exact

__device__ __forceinline__ float dg_normal(uint32_t r0, uint32_t r1) {
    const float a = (float)((r0 >> 8) + 1u) * 5.9604644775390625e-08f;                                           // (0, 1], exact
    return sqrtf(-2.0f * logf(a)) * cosf(6.283185307179586f * dg_unit(r1));
}

// the bicubic convolution kernel of F.interpolate (A = -0.75), as ATen's get_cubic_upsample_coefficients
__device__ __forceinline__ void dg_cubic(float t, float* w) {
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = x2 + 1.0f;
    w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

__device__ __forceinline__ int dg_clamp(int v, int n) { return v < 0 ? 0 : v >= n ? n - 1 : v; }

// The stencil walk of FOUR outputs that are neighbours along a source row: per stencil row k + 3 plane values and k weights (an LDS
// broadcast: the address is uniform) for 4 k fmas, against 8 k reads one output at a time.  Each output sums its taps rows first, then
// columns, one fma per tap.  row: the halo'd LDS cell of tap (0, 0) of output 0; tap (dy, dx) of output j is row[dy * pitch + j + dx].
__device__ __forceinline__ void dg_blur_quad(const float* row, const float* w, int k, int pitch, float* acc) {
    acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
    for (int dy = 0; dy < k; ++dy) {
        float d0 = row[0], d1 = row[1], d2 = row[2];
#pragma unroll 4
        for (int dx = 0; dx < k; ++dx) {
            const float d3 = row[dx + 3], wv = w[dx];
            acc[0] = fmaf(wv, d0, acc[0]); acc[1] = fmaf(wv, d1, acc[1]); acc[2] = fmaf(wv, d2, acc[2]); acc[3] = fmaf(wv, d3, acc[3]);
            d0 = d1; d1 = d2; d2 = d3;
        }
        row += pitch;
        w += k;
    }
}

// low-resolution pixel (ly, lx) of `sr`: the 4 x 4 border-clamped bicubic taps of the H x W plane img (row pitch `pitch`) at the
// align_corners coordinates scale * l, formed in fp32 as F.interpolate forms them
__device__ __forceinline__ float dg_sr_pixel(const float* img, int pitch, int H, int W, float scale_y, float scale_x, int ly, int lx) {
    const float ry = scale_y * (float)ly, rx = scale_x * (float)lx;
    const int iy = (int)floorf(ry), ix = (int)floorf(rx);
    float wy[4], wx[4];
    dg_cubic(ry - (float)iy, wy);
    dg_cubic(rx - (float)ix, wx);
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float* row = img + dg_clamp(iy - 1 + j, H) * pitch;
        float r = 0.f;
#pragma unroll
        for (int i2 = 0; i2 < 4; ++i2) r = fmaf(row[dg_clamp(ix - 1 + i2, W)], wx[i2], r);
        acc = fmaf(r, wy[j], acc);
    }
    return acc;
}

// the draws of the element at index el of its plane, e in the un-augmented cube: generated from (seed, ordinal, e) or read from the cubes
template <bool GEN>
__device__ __forceinline__ void dg_draws(int kind, long e, int el, uint32_t ord, uint32_t k0, uint32_t k1, const float* zp, const float* u0p,
                                         const float* u1p, float& z, float& u0, float& u1) {
    if (GEN) {
        const Philox4 r = philox4x32_10((uint32_t)e, (uint32_t)((unsigned long long)e >> 32), 0u, ord, k0, k1);
        if (kind != MPHSIR_DEG_INPAINT) z = dg_normal(r.r[0], r.r[1]);
        u0 = dg_unit(r.r[2]);
        u1 = dg_unit(r.r[3]);
    } else {
        z = zp[el]; u0 = u0p[el]; u1 = u1p[el];
    }
}

// per-(sample, band) scalars and table rows of the sample's kind only (few live scalar registers in the element loops): s0 = the band's
// sigma (complexN) or atmospheric light (haze), s1 = the band's haze exponent; tabf = the band's column offsets (complexN) or the
// sample's cirrus map (haze); dead = the band's dead columns.  W: the plane's width, plane: its elements
struct DgBand { float s0, s1; bool bflag; const float* tabf; const uint8_t* dead; };

__device__ __forceinline__ DgBand dg_band(const DegradeDev& a, int kind, int bc, int b, int c, int W, long plane) {
    DgBand t{0.f, 0.f, false, nullptr, nullptr};
    if (kind == MPHSIR_DEG_COMPLEX) {
        t.s0 = a.band_sigma[bc];
        t.tabf = a.col_off + (long)bc * W;
        t.dead = a.col_dead + (long)bc * W;
    }
    if (kind == MPHSIR_DEG_COMPLEX || kind == MPHSIR_DEG_BANDMISS) t.bflag = a.band_flag[bc] != 0;
    if (kind == MPHSIR_DEG_HAZE) {
        t.s0 = a.atm[bc];
        t.s1 = a.haze_ratio[c];
        t.tabf = a.cirrus + (long)b * plane;
    }
    return t;
}

// the degraded value of one element of a kind other than blur.  x: the clean element, (z, u0, u1): its draws, sx / el: its column / its
// index in the plane, lowv: its low-resolution pixel (sr)
__device__ __forceinline__ float dg_value(int kind, int sub, float par, const DgBand& t, int sx, int el, float x, float z, float u0, float u1,
                                          float lowv) {
    const float s0 = t.s0, s1 = t.s1;
    const bool bflag = t.bflag;
    const float* tabf = t.tabf;
    const uint8_t* dead = t.dead;
    float y;
    switch (kind) {
    case MPHSIR_DEG_GAUSSIAN:
        y = x + z * par;
        break;
    case MPHSIR_DEG_COMPLEX: {
        y = x + z * s0;
        y = y * (dead[sx] ? 0.f : 1.f);
        if (sub == 1 && bflag && u0 < par) y = u1 < 0.5f ? 1.f : 0.f;
        y = y - tabf[sx];
        break;
    }
    case MPHSIR_DEG_SR:
        y = lowv;
        break;
    case MPHSIR_DEG_INPAINT:
        y = x * (u0 > par ? 1.f : 0.f);
        break;
    case MPHSIR_DEG_BANDMISS:
        y = x * (bflag ? 0.f : 1.f);
        break;
    case MPHSIR_DEG_HAZE: {
        float t1 = 1.0f - par * tabf[el];
        t1 = t1 <= 0.f ? 1e-10f : t1;
        const float t = expf(s1 * logf(t1));
        y = x * t + s0 * (1.0f - t);
        break;
    }
    default:
        y = x;
    }
    return y;
}

// grid (B * C), 256 threads, dynamic LDS: the plane with the launch's largest halo, then the low-resolution image / the weights.
// GEN: generated draws (the product path) or explicit ones (tests): two instances, so that neither carries the other's pointers and keys
// as live scalars through the element loop (one kernel for both ran out of scalar registers by three).
template <bool GEN> __global__ __launch_bounds__(DG_NT) void degrade_batch_kernel(DegradeDev a) {
    HIP_DYNAMIC_SHARED(float, lds)
    const int tid = threadIdx.x;
    const int bc = blockIdx.x, b = bc / a.C, c = bc - b * a.C;
    const int N = a.N;
    const long base = (long)bc * N * N;
    const float* src = a.clean + base;
    const int kind = a.menu[dg_clamp(a.task[b], a.T)];
    const D4 d4(a.aug[b] & 7);
    const bool tr = d4.tr, fy = d4.fy, fx = d4.fx;
    const int sub = a.sub ? a.sub[b] : 0;
    const float par = a.param ? a.param[b] : 0.f;

    int h = 0, k = 1;
    const float* wts = nullptr;
    if (kind == MPHSIR_DEG_BLUR) {
        const int si = dg_clamp(sub, a.K);
        k = a.ksize[si];
        h = k >> 1;
        wts = a.stencils + (long)si * DG_SS * DG_SS;
    }
    const int P = N + 2 * h, pitch = P | 1;
    if (h) {
        for (int i = tid; i < P * pitch; i += DG_NT) lds[i] = 0.f;
        __syncthreads();
    }
    for (int y = tid >> 6; y < N; y += DG_NT / 64)
        for (int x = tid & 63; x < N; x += 64) lds[(y + h) * pitch + x + h] = src[y * N + x];
    __syncthreads();

    float* low = lds + a.low_off;                       // sr: the low-resolution image; blur: the k x k weights (a sample is one or the other)
    float* od = a.degraded + base;
    float* oc = a.clean_aug + base;
    if (kind == MPHSIR_DEG_BLUR) {
        // A thread owns FOUR outputs that are neighbours along a source row (dg_blur_quad).  Lanes run along the direction that is the
        // OUTPUT's x (source x in quads, or source y under a transposing mode), so each of the four stores of a wave stays within whole
        // output rows.
        for (int i = tid; i < k * k; i += DG_NT) low[i] = wts[(i / k) * DG_SS + i % k];
        __syncthreads();
        const int Q = (N + 3) >> 2;
        for (int i = tid; i < N * Q; i += DG_NT) {
            int sy, sx0;
            if (tr) { const int q = i / N; sy = i - q * N; sx0 = 4 * q; }
            else    { sy = i / Q; sx0 = 4 * (i - sy * Q); }
            float acc[4];
            dg_blur_quad(lds + sy * pitch + sx0, low, k, pitch, acc);
            const int A = fy ? N - 1 - sy : sy;
            const float* xs = lds + (sy + h) * pitch + sx0 + h;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (sx0 + j < N) {
                    const int Bv = fx ? N - 1 - (sx0 + j) : sx0 + j;
                    const int o = tr ? Bv * N + A : A * N + Bv;
                    od[o] = acc[j];
                    oc[o] = xs[j];
                }
            }
        }
        return;
    }
    int f = 1, n = N;
    if (kind == MPHSIR_DEG_SR) {
        f = a.factor[dg_clamp(sub, a.F)];
        n = N / f;
        const float scale = (float)(N - 1) / (float)(n - 1);
        for (int i = tid; i < n * n; i += DG_NT) {
            const int ly = i / n, lx = i - ly * n;
            low[i] = dg_sr_pixel(lds, pitch, N, N, scale, scale, ly, lx);
        }
        __syncthreads();
    }

    constexpr bool gen = GEN;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const uint32_t ord = (uint32_t)(a.ordinal_dev ? *a.ordinal_dev : a.ordinal);
    const bool needs_draws = kind == MPHSIR_DEG_GAUSSIAN || kind == MPHSIR_DEG_COMPLEX || kind == MPHSIR_DEG_INPAINT;
    const DgBand t = dg_band(a, kind, bc, b, c, N, (long)N * N);
    const float* zp = gen ? nullptr : a.z + base;
    const float* u0p = gen ? nullptr : a.u0 + base;
    const float* u1p = gen ? nullptr : a.u1 + base;

    for (int oy = tid >> 6; oy < N; oy += DG_NT / 64) {
        for (int ox = tid & 63; ox < N; ox += 64) {
            int sy, sx;
            d4.source(oy, ox, N, N, sy, sx);
            const float x = lds[(sy + h) * pitch + sx + h];
            const int el = sy * N + sx;
            float z = 0.f, u0 = 0.f, u1 = 0.f;
            if (needs_draws) dg_draws<GEN>(kind, base + el, el, ord, k0, k1, zp, u0p, u1p, z, u0, u1);
            const float y = dg_value(kind, sub, par, t, sx, el, x, z, u0, u1, kind == MPHSIR_DEG_SR ? low[(sy / f) * n + sx / f] : 0.f);
            od[oy * N + ox] = y;
            oc[oy * N + ox] = x;
        }
    }
}

// The tiled form.  grid (B * C * nty * ntx), 256 threads, dynamic LDS: a 64 x 64 tile with the launch's largest halo, then the
// low-resolution pixels under the tile / the weights.  Every global offset inside a plane is an int (H * W < 2^31, checked by the host),
// the plane's own offset a long.
constexpr int DG_T = 64;

template <bool GEN, bool VEC> __global__ __launch_bounds__(DG_NT) void degrade_planes_kernel(DegradeDev a) {
    HIP_DYNAMIC_SHARED(float, lds)
    const int tid = threadIdx.x;
    const int tiles = a.ntx * a.nty;
    const int bc = blockIdx.x / tiles, tile = blockIdx.x - bc * tiles, b = bc / a.C, c = bc - b * a.C;
    const int H = a.H, W = a.W;
    const long base = (long)bc * H * W;
    const float* src = a.clean + base;
    const int kind = a.menu[dg_clamp(a.task[b], a.T)];
    const D4 d4(a.aug ? a.aug[b] & 7 : 0);
    const bool tr = d4.tr, fy = d4.fy, fx = d4.fx;
    const int sub = a.sub ? a.sub[b] : 0;
    const float par = a.param ? a.param[b] : 0.f;

    // the OUTPUT tile, and the rectangle of the source it comes from under the inverse of the mode (a mode that transposes has H == W)
    const int ty = tile / a.ntx, tx = tile - ty * a.ntx;
    const int oy0 = ty * DG_T, ox0 = tx * DG_T;
    const int oth = H - oy0 < DG_T ? H - oy0 : DG_T, otw = W - ox0 < DG_T ? W - ox0 : DG_T;
    const int sth = tr ? otw : oth, stw = tr ? oth : otw;
    const int p0 = tr ? ox0 : oy0, q0 = tr ? oy0 : ox0;
    const int sy0 = fy ? H - p0 - sth : p0, sx0 = fx ? W - q0 - stw : q0;

    int h = 0, k = 1;
    const float* wts = nullptr;
    if (kind == MPHSIR_DEG_BLUR) {
        const int si = dg_clamp(sub, a.K);
        k = a.ksize[si];
        h = k >> 1;
        wts = a.stencils + (long)si * DG_SS * DG_SS;
    }
    float* od = a.degraded + base;
    float* oc = a.clean_aug ? a.clean_aug + base : nullptr;

    // LDS cell (ly, lx) = source element (sy0 - h + ly, sx0 - h + lx), zero outside the plane.  An sr sample whose clean copy is not
    // asked for reads no clean element here: its taps come from global memory.
    const int PH = sth + 2 * h, PW = stw + 2 * h, pitch = (DG_T + 2 * h) | 1;
    if (kind != MPHSIR_DEG_SR || oc) {
        if (VEC) {
            // W % 4 == 0: sx0 and stw are multiples of 4 and every row of the tile starts on 16 bytes; the halo columns one by one
            const int Q = stw >> 2;
            for (int i = tid; i < PH * Q; i += DG_NT) {
                const int ly = i / Q, qx = i - ly * Q, gy = sy0 - h + ly;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (gy >= 0 && gy < H) v = *reinterpret_cast<const f32x4*>(src + gy * W + sx0 + 4 * qx);
                float* d = lds + ly * pitch + h + 4 * qx;
                d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
            }
            for (int i = tid; i < PH * 2 * h; i += DG_NT) {
                const int ly = i / (2 * h), j = i - ly * 2 * h, lx = j < h ? j : stw + j;
                const int gy = sy0 - h + ly, gx = sx0 - h + lx;
                lds[ly * pitch + lx] = gy >= 0 && gy < H && gx >= 0 && gx < W ? src[gy * W + gx] : 0.f;
            }
        } else {
            for (int ly = tid >> 6; ly < PH; ly += DG_NT / 64)
                for (int lx = tid & 63; lx < PW; lx += 64) {
                    const int gy = sy0 - h + ly, gx = sx0 - h + lx;
                    lds[ly * pitch + lx] = gy >= 0 && gy < H && gx >= 0 && gx < W ? src[gy * W + gx] : 0.f;
                }
        }
    }
    float* low = lds + a.low_off;                       // sr: the low-resolution pixels under the tile; blur: the k x k weights
    if (kind == MPHSIR_DEG_BLUR) {
        for (int i = tid; i < k * k; i += DG_NT) low[i] = wts[(i / k) * DG_SS + i % k];
        __syncthreads();
        // as the plane form: four outputs along a source row per thread, lanes along the OUTPUT's x
        const int Q = (stw + 3) >> 2;
        for (int i = tid; i < sth * Q; i += DG_NT) {
            int ly, lx0;
            if (tr) { const int q = i / sth; ly = i - q * sth; lx0 = 4 * q; }
            else    { ly = i / Q; lx0 = 4 * (i - ly * Q); }
            float acc[4];
            dg_blur_quad(lds + ly * pitch + lx0, low, k, pitch, acc);
            const int sy = sy0 + ly, sx = sx0 + lx0;
            const int A = fy ? H - 1 - sy : sy;
            const float* xs = lds + (ly + h) * pitch + lx0 + h;
            if (VEC && !tr) {
                // the four are neighbours in the output row too, in reverse under a column flip
                const int o = A * W + (fx ? W - 4 - sx : sx);
                const f32x4 vd = {acc[fx ? 3 : 0], acc[fx ? 2 : 1], acc[fx ? 1 : 2], acc[fx ? 0 : 3]};
                *reinterpret_cast<f32x4*>(od + o) = vd;
                if (oc) {
                    const f32x4 vc = {xs[fx ? 3 : 0], xs[fx ? 2 : 1], xs[fx ? 1 : 2], xs[fx ? 0 : 3]};
                    *reinterpret_cast<f32x4*>(oc + o) = vc;
                }
                continue;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (lx0 + j < stw) {
                    const int Bv = fx ? W - 1 - (sx + j) : sx + j;
                    const int o = tr ? Bv * W + A : A * W + Bv;
                    od[o] = acc[j];
                    if (oc) oc[o] = xs[j];
                }
            }
        }
        return;
    }
    int f = 1, nlx = 1;
    if (kind == MPHSIR_DEG_SR) {
        // the low-resolution pixels that the tile's elements replicate, each from its taps in the WHOLE plane; `low` then moves so that
        // pixel (ly, lx) of the plane's low-resolution image is low[ly * nlx + lx]
        f = a.factor[dg_clamp(sub, a.F)];
        const int nh = H / f, nw = W / f;
        const float scale_y = (float)(H - 1) / (float)(nh - 1), scale_x = (float)(W - 1) / (float)(nw - 1);
        const int ly0 = sy0 / f, lx0 = sx0 / f, nly = (sy0 + sth - 1) / f - ly0 + 1;
        nlx = (sx0 + stw - 1) / f - lx0 + 1;
        for (int i = tid; i < nly * nlx; i += DG_NT) {
            const int ly = i / nlx, lx = i - ly * nlx;
            low[i] = dg_sr_pixel(src, W, H, W, scale_y, scale_x, ly0 + ly, lx0 + lx);
        }
        low -= ly0 * nlx + lx0;
    }
    __syncthreads();

    constexpr bool gen = GEN;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const uint32_t ord = (uint32_t)(a.ordinal_dev ? *a.ordinal_dev : a.ordinal);
    const bool needs_draws = kind == MPHSIR_DEG_GAUSSIAN || kind == MPHSIR_DEG_COMPLEX || kind == MPHSIR_DEG_INPAINT;
    DgBand t = dg_band(a, kind, bc, b, c, W, (long)H * W);
    if (kind == MPHSIR_DEG_COMPLEX) t.bflag = t.bflag && sub == 1;       // impulses: the subtype and the band's flag as one scalar
    const float* zp = gen ? nullptr : a.z + base;
    const float* u0p = gen ? nullptr : a.u0 + base;
    const float* u1p = gen ? nullptr : a.u1 + base;
    // The element loop, once for the kinds that take draws and once for the others, so that the twenty round keys of Philox and the
    // scalars of sr / haze are never live together (one loop for all kinds spilled scalar registers).  One output element: its source
    // position under the inverse of the mode, the clean value from LDS (no halo here: the pitch is 65, and xl is the tile moved so
    // that the plane's (sy, sx) is xl[sy * 65 + sx]), the degraded value.
    const float* xl = lds - (sy0 * (DG_T | 1) + sx0);
    const auto loop = [&](auto with_draws) {
        constexpr bool DRAWS = decltype(with_draws)::value;
        // the kinds of this loop, for the compiler to see (the subtype of complexN is folded into t.bflag above)
        const int kd = !DRAWS ? kind : kind == MPHSIR_DEG_COMPLEX ? MPHSIR_DEG_COMPLEX : kind == MPHSIR_DEG_INPAINT ? MPHSIR_DEG_INPAINT : MPHSIR_DEG_GAUSSIAN;
        const auto element = [&](int oy, int ox, float& x) {
            int sy, sx;
            d4.source(oy, ox, H, W, sy, sx);
            x = xl[sy * (DG_T | 1) + sx];
            const int el = sy * W + sx;
            float z = 0.f, u0 = 0.f, u1 = 0.f;
            if (DRAWS) dg_draws<GEN>(kind, base + el, el, ord, k0, k1, zp, u0p, u1p, z, u0, u1);
            return dg_value(kd, 1, par, t, sx, el, x, z, u0, u1, !DRAWS && kind == MPHSIR_DEG_SR ? low[(sy / f) * nlx + sx / f] : 0.f);
        };
        if (VEC) {
            // four neighbours of an output row per thread and one dwordx4 store per cube, whatever the mode: in the source they are
            // neighbours along a row or, under a transposing mode, along a column (lanes 4 rows apart: two lanes per LDS bank)
            const int Q = otw >> 2;
            for (int i = tid; i < oth * Q; i += DG_NT) {
                const int oyl = i / Q, oy = oy0 + oyl, ox = ox0 + 4 * (i - oyl * Q);
                f32x4 vd, vc;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float x;
                    vd[j] = element(oy, ox + j, x);
                    vc[j] = x;
                }
                *reinterpret_cast<f32x4*>(od + oy * W + ox) = vd;
                if (oc) *reinterpret_cast<f32x4*>(oc + oy * W + ox) = vc;
            }
            return;
        }
        // a wave per output row of the tile (at most 64 wide)
        const int ox = ox0 + (tid & 63);
        if ((tid & 63) >= otw) return;
        for (int oy = oy0 + (tid >> 6); oy < oy0 + oth; oy += DG_NT / 64) {
            float x;
            const float y = element(oy, ox, x);
            od[oy * W + ox] = y;
            if (oc) oc[oy * W + ox] = x;
        }
    };
    if (needs_draws) loop(std::true_type{});
    else loop(std::false_type{});
}

// What the two entry points share: the checks of the sizes, the plan and the draws, and the device's copy of the arguments.  planes: the
// tiled form (any H x W, clean_aug and aug optional).  -> kinds: bit k set when kind k is in the menu; hmax: the largest halo of the
// stencil table (0 without a blur in the menu); fmin: the smallest sr factor; given: how many of z / u0 / u1
static int degrade_prepare(const mphsir_degrade_args* a, const char* fn, bool planes, DegradeDev& d, unsigned& kinds, int& hmax, int& fmin, int& given) {
    MPHSIR_CHECK_ARGS(a, fn);
    MPHSIR_REQUIRE(a->clean && a->degraded && a->menu && a->task && (planes || (a->clean_aug && a->aug)), "%s: null pointer", fn);
    MPHSIR_REQUIRE(a->B > 0 && a->C > 0 && a->H > 0 && a->W > 0 && (long)a->B * a->C < (1L << 31), "%s: bad sizes (B %d, C %d, H %d, W %d)", fn, a->B, a->C,
                   a->H, a->W);
    if (planes) {
        MPHSIR_REQUIRE((long)a->H * a->W < (1L << 31), "%s: a plane of %d x %d has 2^31 elements or more", fn, a->H, a->W);
        MPHSIR_REQUIRE(a->H == a->W || !a->aug, "%s: a plane of %d x %d is not square: aug must be NULL (no flips / rotations of whole scenes)", fn, a->H,
                       a->W);
    } else {
        MPHSIR_REQUIRE(a->H == a->W, "%s: planes must be square, got %d x %d", fn, a->H, a->W);
        MPHSIR_REQUIRE((long)a->H * a->H <= 128L * 128L, "%s: a plane of %d x %d does not fit in LDS (N * N <= 128 * 128)", fn, a->H, a->H);
    }
    MPHSIR_REQUIRE(a->T > 0 && a->T <= MPHSIR_DEG_MAX_TASKS && a->K >= 0 && a->K <= MPHSIR_DEG_MAX_STENCILS && a->F >= 0 && a->F <= MPHSIR_DEG_MAX_FACTORS,
                   "%s: table sizes (T %d in 1..%d, K %d <= %d, F %d <= %d)", fn, a->T, MPHSIR_DEG_MAX_TASKS, a->K, MPHSIR_DEG_MAX_STENCILS, a->F,
                   MPHSIR_DEG_MAX_FACTORS);
    MPHSIR_REQUIRE((a->K == 0 || a->ksize) && (a->F == 0 || a->sr_factor), "%s: null pointer (ksize / sr_factor)", fn);
    given = (a->z != nullptr) + (a->u0 != nullptr) + (a->u1 != nullptr);
    MPHSIR_REQUIRE(given == 0 || given == 3, "%s: explicit draws are z, u0 and u1, all three or none (got %d of them)", fn, given);
    kinds = 0;
    for (int t = 0; t < a->T; ++t) {
        MPHSIR_REQUIRE(a->menu[t] >= MPHSIR_DEG_NONE && a->menu[t] <= MPHSIR_DEG_HAZE, "%s: unknown kind %d for task %d", fn, a->menu[t], t);
        d.menu[t] = a->menu[t];
        kinds |= 1u << a->menu[t];
    }
    const auto has = [&](int kind) { return (kinds >> kind) & 1u; };
    hmax = 0;
    fmin = 0;
    for (int i = 0; i < a->K; ++i) {
        MPHSIR_REQUIRE(a->ksize[i] >= 1 && (a->ksize[i] & 1) && a->ksize[i] <= MPHSIR_DEG_STENCIL_SIDE, "%s: stencil %d has side %d: must be odd and <= %d",
                       fn, i, a->ksize[i], MPHSIR_DEG_STENCIL_SIDE);
        d.ksize[i] = a->ksize[i];
        if (a->ksize[i] / 2 > hmax) hmax = a->ksize[i] / 2;
    }
    for (int i = 0; i < a->F; ++i) {
        const int f = a->sr_factor[i];
        if (planes)
            MPHSIR_REQUIRE(f >= 1 && a->H % f == 0 && a->W % f == 0 && a->H / f >= 2 && a->W / f >= 2,
                           "%s: sr factor %d must divide H = %d and W = %d and leave H / f >= 2 and W / f >= 2", fn, f, a->H, a->W);
        else
            MPHSIR_REQUIRE(f >= 1 && a->H % f == 0 && a->H / f >= 2, "%s: sr factor %d must divide N = %d and leave N / f >= 2", fn, f, a->H);
        d.factor[i] = f;
        if (fmin == 0 || f < fmin) fmin = f;
    }
    const bool perb = has(MPHSIR_DEG_GAUSSIAN) || has(MPHSIR_DEG_COMPLEX) || has(MPHSIR_DEG_INPAINT) || has(MPHSIR_DEG_HAZE);
    const bool subb = has(MPHSIR_DEG_COMPLEX) || has(MPHSIR_DEG_BLUR) || has(MPHSIR_DEG_SR);
    MPHSIR_REQUIRE((!perb || a->param) && (!subb || a->sub), "%s: a kind of the menu reads `param` / `sub`, which is NULL", fn);
    MPHSIR_REQUIRE(!has(MPHSIR_DEG_COMPLEX) || (a->band_sigma && a->band_flag && a->col_dead && a->col_off),
                   "%s: complexN reads band_sigma, band_flag, col_dead and col_off: one is NULL", fn);
    MPHSIR_REQUIRE(!has(MPHSIR_DEG_BANDMISS) || a->band_flag, "%s: bandmiss reads band_flag, which is NULL", fn);
    MPHSIR_REQUIRE(!has(MPHSIR_DEG_BLUR) || (a->K > 0 && a->stencils), "%s: blur needs a stencil table (K %d)", fn, a->K);
    MPHSIR_REQUIRE(!has(MPHSIR_DEG_SR) || a->F > 0, "%s: sr needs a factor table (F %d)", fn, a->F);
    MPHSIR_REQUIRE(!has(MPHSIR_DEG_HAZE) || (a->cirrus && a->atm && a->haze_ratio), "%s: haze reads cirrus, atm and haze_ratio: one is NULL", fn);
    if (!has(MPHSIR_DEG_BLUR)) hmax = 0;
    d.clean = a->clean; d.degraded = a->degraded; d.clean_aug = a->clean_aug;
    d.task = a->task; d.aug = a->aug; d.param = a->param; d.sub = a->sub;
    d.band_sigma = a->band_sigma; d.band_flag = a->band_flag; d.col_dead = a->col_dead; d.col_off = a->col_off;
    d.stencils = a->stencils; d.cirrus = a->cirrus; d.atm = a->atm; d.haze_ratio = a->haze_ratio;
    d.z = a->z; d.u0 = a->u0; d.u1 = a->u1;
    d.ordinal_dev = reinterpret_cast<const long long*>(a->ordinal_dev);
    d.seed = (unsigned long long)a->seed; d.ordinal = a->ordinal;
    d.C = a->C; d.N = a->H; d.H = a->H; d.W = a->W; d.T = a->T; d.K = a->K; d.F = a->F;
    return MPHSIR_OK;
}

// floats of dynamic LDS of the tiled form for a largest halo hmax and the sr factors of the plan (none: no sr in the menu): the tile (4
// floats of slack, as the plane form), then the low-resolution pixels under the tile or the weights of a blur sample.  A factor that
// divides 64 divides every tile origin too (it divides H and W): 64 / f pixels a side; any other f: 63 / f + 2 at most
static long degrade_planes_lds_floats(int hmax, const int32_t* factor, int F, bool blur, long* low_off) {
    long nl = 0;
    for (int i = 0; i < F; ++i) {
        const long n = DG_T % factor[i] == 0 ? DG_T / factor[i] : (DG_T - 1) / factor[i] + 2;
        if (n > nl) nl = n;
    }
    const long P = DG_T + 2 * hmax, plane = P * (P | 1) + 4;
    long low = nl * nl;
    if (blur && low < DG_SS * DG_SS) low = DG_SS * DG_SS;
    *low_off = plane;
    return plane + low;
}

}  // namespace mphsir

extern "C" int mphsir_degrade_batch(const mphsir_degrade_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    DegradeDev d{};
    unsigned kinds = 0;
    int hmax = 0, fmin = 0, given = 0;
    if (const int rc = degrade_prepare(a, "degrade_batch", false, d, kinds, hmax, fmin, given)) return rc;
    const auto has = [&](int kind) { return (kinds >> kind) & 1u; };
    const int N = a->H;
    // the plane (4 floats of slack: the last quad of a blur row may read past a row that is no multiple of 4 wide), then one region that
    // holds the low-resolution image of an sr sample or the weights of a blur sample
    const long P = N + 2 * hmax, plane = P * (P | 1) + 4;
    long low = has(MPHSIR_DEG_SR) ? (long)(N / fmin) * (N / fmin) : 0;
    if (has(MPHSIR_DEG_BLUR) && low < DG_SS * DG_SS) low = DG_SS * DG_SS;
    const size_t shmem = (size_t)(plane + low) * sizeof(float);
    MPHSIR_REQUIRE(shmem <= 160u * 1024u, "degrade_batch: %zu bytes of LDS for N = %d, halo %d: more than a workgroup can have", shmem, N, hmax);
    d.low_off = (int)plane;
    const dim3 grid((unsigned)(a->B * a->C));
    if (given == 0) {
        allow_big_lds(degrade_batch_kernel<true>, shmem);
        MPHSIR_LAUNCH(MPHSIR_K_DEGRADE, degrade_batch_kernel<true>, grid, dim3(DG_NT), shmem, reinterpret_cast<hipStream_t>(stream), d);
    } else {
        allow_big_lds(degrade_batch_kernel<false>, shmem);
        MPHSIR_LAUNCH(MPHSIR_K_DEGRADE, degrade_batch_kernel<false>, grid, dim3(DG_NT), shmem, reinterpret_cast<hipStream_t>(stream), d);
    }
    return MPHSIR_OK;
}

extern "C" int mphsir_degrade_planes(const mphsir_degrade_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    DegradeDev d{};
    unsigned kinds = 0;
    int hmax = 0, fmin = 0, given = 0;
    if (const int rc = degrade_prepare(a, "degrade_planes", true, d, kinds, hmax, fmin, given)) return rc;
    d.ntx = (a->W + DG_T - 1) / DG_T;
    d.nty = (a->H + DG_T - 1) / DG_T;
    const long blocks = (long)a->B * a->C * d.ntx * d.nty;
    MPHSIR_REQUIRE(blocks < (1L << 31), "degrade_planes: %ld tiles (B %d, C %d, %d x %d tiles of %d x %d): 2^31 or more", blocks, a->B, a->C, d.nty, d.ntx, DG_T,
                   DG_T);
    const bool vec = rows_aligned16(a->W, a->clean, a->degraded, a->clean_aug);
    long low_off = 0;
    const size_t shmem = (size_t)degrade_planes_lds_floats(hmax, a->sr_factor, (kinds >> MPHSIR_DEG_SR) & 1u ? a->F : 0, (kinds >> MPHSIR_DEG_BLUR) & 1u, &low_off) * sizeof(float);
    d.low_off = (int)low_off;
    const dim3 grid((unsigned)blocks);
    const auto launch = [&](auto kern) {
        allow_big_lds(kern, shmem);
        MPHSIR_LAUNCH(MPHSIR_K_DEGRADE, kern, grid, dim3(DG_NT), shmem, reinterpret_cast<hipStream_t>(stream), d);
        return (int)MPHSIR_OK;
    };
    if (given == 0) return vec ? launch(degrade_planes_kernel<true, true>) : launch(degrade_planes_kernel<true, false>);
    return vec ? launch(degrade_planes_kernel<false, true>) : launch(degrade_planes_kernel<false, false>);
}
