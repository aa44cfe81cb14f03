// Training-batch degradation in one launch (include/mphsir.h holds the definitions; mp-hsir_amd/degrade.py the tensor functions whose
// element values these are).  clean [B][C][N][N] -> degraded, clean_aug, both under the sample's flip / rotation.
//
// One workgroup of 256 threads owns one (sample, band) plane.  The plane is staged once in LDS -- with a zero halo of k / 2 when the
// sample is a blur, so that the stencil walk has no bounds test -- and every OUTPUT pixel (oy, ox) is computed from the LDS plane at its
// source position (sy, sx) under the inverse of the sample's mode (the index map of scene_d4.hip): both outputs leave as whole rows,
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
#include "mphsir_dev.h"
#include "mphsir_host.h"

#pragma clang fp contract(off)

namespace mphsir {

constexpr int DG_NT = 256;
constexpr int DG_SS = MPHSIR_DEG_STENCIL_SIDE;
constexpr unsigned D4Q_FY = 0xD2u;   // bit m: mode m flips rows    (scene_d4.hip)
constexpr unsigned D4Q_FX = 0xB4u;   // bit m: mode m flips columns

struct DegradeDev {
    const float* clean; float* degraded; float* clean_aug;
    const int* task; const int* aug; const float* param; const int* sub;
    const float* band_sigma; const uint8_t* band_flag; const uint8_t* col_dead; const float* col_off;
    const float* stencils; const float* cirrus; const float* atm; const float* haze_ratio;
    const float* z; const float* u0; const float* u1;
    const long long* ordinal_dev;
    unsigned long long seed; long long ordinal;
    int C, N, T, K, F, low_off;
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
    const int m = a.aug[b] & 7;
    const bool tr = (m >> 1) & 1, fy = (D4Q_FY >> m) & 1, fx = (D4Q_FX >> m) & 1;
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
        // A thread owns FOUR outputs that are neighbours along a source row: per stencil row it reads k + 3 plane values and k weights
        // (an LDS broadcast: the address is uniform) for 4 k fmas, against 8 k reads one output at a time.  Each output still sums its
        // taps rows first, then columns, one fma per tap.  Lanes run along the direction that is the OUTPUT's x (source x in quads, or
        // source y under a transposing mode), so each of the four stores of a wave stays within whole output rows.
        for (int i = tid; i < k * k; i += DG_NT) low[i] = wts[(i / k) * DG_SS + i % k];
        __syncthreads();
        const int Q = (N + 3) >> 2;
        for (int i = tid; i < N * Q; i += DG_NT) {
            int sy, sx0;
            if (tr) { const int q = i / N; sy = i - q * N; sx0 = 4 * q; }
            else    { sy = i / Q; sx0 = 4 * (i - sy * Q); }
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            const float* row = lds + sy * pitch + sx0;                     // tap (dy, dx) of output j: row[dy * pitch + j + dx]
            const float* w = low;
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
            const float ry = scale * (float)ly, rx = scale * (float)lx;
            const int iy = (int)floorf(ry), ix = (int)floorf(rx);
            float wy[4], wx[4];
            dg_cubic(ry - (float)iy, wy);
            dg_cubic(rx - (float)ix, wx);
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float* row = lds + dg_clamp(iy - 1 + j, N) * pitch;
                float r = 0.f;
#pragma unroll
                for (int i2 = 0; i2 < 4; ++i2) r = fmaf(row[dg_clamp(ix - 1 + i2, N)], wx[i2], r);
                acc = fmaf(r, wy[j], acc);
            }
            low[i] = acc;
        }
        __syncthreads();
    }

    constexpr bool gen = GEN;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const uint32_t ord = (uint32_t)(a.ordinal_dev ? *a.ordinal_dev : a.ordinal);
    const bool needs_draws = kind == MPHSIR_DEG_GAUSSIAN || kind == MPHSIR_DEG_COMPLEX || kind == MPHSIR_DEG_INPAINT;
    // per-(sample, band) scalars and table rows of the sample's kind only (few live scalar registers in the loop below): s0 = the band's
    // sigma (complexN) or atmospheric light (haze), s1 = the band's haze exponent; tabf = the band's column offsets (complexN) or the
    // sample's cirrus map (haze); dead = the band's dead columns; the explicit draws start at the plane
    float s0 = 0.f, s1 = 0.f;
    bool bflag = false;
    const float* tabf = nullptr;
    const uint8_t* dead = nullptr;
    if (kind == MPHSIR_DEG_COMPLEX) {
        s0 = a.band_sigma[bc];
        tabf = a.col_off + (long)bc * N;
        dead = a.col_dead + (long)bc * N;
    }
    if (kind == MPHSIR_DEG_COMPLEX || kind == MPHSIR_DEG_BANDMISS) bflag = a.band_flag[bc] != 0;
    if (kind == MPHSIR_DEG_HAZE) {
        s0 = a.atm[bc];
        s1 = a.haze_ratio[c];
        tabf = a.cirrus + (long)b * N * N;
    }
    const float* zp = gen ? nullptr : a.z + base;
    const float* u0p = gen ? nullptr : a.u0 + base;
    const float* u1p = gen ? nullptr : a.u1 + base;

    for (int oy = tid >> 6; oy < N; oy += DG_NT / 64) {
        for (int ox = tid & 63; ox < N; ox += 64) {
            const int p = tr ? ox : oy, q = tr ? oy : ox;
            const int sy = fy ? N - 1 - p : p, sx = fx ? N - 1 - q : q;
            const float x = lds[(sy + h) * pitch + sx + h];
            float z = 0.f, u0 = 0.f, u1 = 0.f;
            if (needs_draws) {
                const int el = sy * N + sx;
                if (gen) {
                    const long e = base + el;
                    const Philox4 r = philox4x32_10((uint32_t)e, (uint32_t)((unsigned long long)e >> 32), 0u, ord, k0, k1);
                    if (kind != MPHSIR_DEG_INPAINT) z = dg_normal(r.r[0], r.r[1]);
                    u0 = dg_unit(r.r[2]);
                    u1 = dg_unit(r.r[3]);
                } else {
                    z = zp[el]; u0 = u0p[el]; u1 = u1p[el];
                }
            }
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
                y = low[(sy / f) * n + sx / f];
                break;
            case MPHSIR_DEG_INPAINT:
                y = x * (u0 > par ? 1.f : 0.f);
                break;
            case MPHSIR_DEG_BANDMISS:
                y = x * (bflag ? 0.f : 1.f);
                break;
            case MPHSIR_DEG_HAZE: {
                float t1 = 1.0f - par * tabf[sy * N + sx];
                t1 = t1 <= 0.f ? 1e-10f : t1;
                const float t = expf(s1 * logf(t1));
                y = x * t + s0 * (1.0f - t);
                break;
            }
            default:
                y = x;
            }
            od[oy * N + ox] = y;
            oc[oy * N + ox] = x;
        }
    }
}

}  // namespace mphsir

extern "C" int mphsir_degrade_batch(const mphsir_degrade_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "degrade_batch");
    MPHSIR_REQUIRE(a->clean && a->degraded && a->clean_aug && a->menu && a->task && a->aug, "degrade_batch: null pointer");
    MPHSIR_REQUIRE(a->B > 0 && a->C > 0 && a->H > 0 && a->W > 0 && (long)a->B * a->C < (1L << 31), "degrade_batch: bad sizes (B %d, C %d, H %d, W %d)",
                   a->B, a->C, a->H, a->W);
    MPHSIR_REQUIRE(a->H == a->W, "degrade_batch: planes must be square, got %d x %d", a->H, a->W);
    const int N = a->H;
    MPHSIR_REQUIRE((long)N * N <= 128L * 128L, "degrade_batch: a plane of %d x %d does not fit in LDS (N * N <= 128 * 128)", N, N);
    MPHSIR_REQUIRE(a->T > 0 && a->T <= MPHSIR_DEG_MAX_TASKS && a->K >= 0 && a->K <= MPHSIR_DEG_MAX_STENCILS && a->F >= 0 && a->F <= MPHSIR_DEG_MAX_FACTORS,
                   "degrade_batch: table sizes (T %d in 1..%d, K %d <= %d, F %d <= %d)", a->T, MPHSIR_DEG_MAX_TASKS, a->K, MPHSIR_DEG_MAX_STENCILS, a->F,
                   MPHSIR_DEG_MAX_FACTORS);
    MPHSIR_REQUIRE((a->K == 0 || a->ksize) && (a->F == 0 || a->sr_factor), "degrade_batch: null pointer (ksize / sr_factor)");
    const int given = (a->z != nullptr) + (a->u0 != nullptr) + (a->u1 != nullptr);
    MPHSIR_REQUIRE(given == 0 || given == 3, "degrade_batch: explicit draws are z, u0 and u1, all three or none (got %d of them)", given);
    DegradeDev d{};
    unsigned kinds = 0;
    for (int t = 0; t < a->T; ++t) {
        MPHSIR_REQUIRE(a->menu[t] >= MPHSIR_DEG_NONE && a->menu[t] <= MPHSIR_DEG_HAZE, "degrade_batch: unknown kind %d for task %d", a->menu[t], t);
        d.menu[t] = a->menu[t];
        kinds |= 1u << a->menu[t];
    }
    const auto has = [&](int kind) { return (kinds >> kind) & 1u; };
    int hmax = 0, fmin = 0;
    for (int i = 0; i < a->K; ++i) {
        MPHSIR_REQUIRE(a->ksize[i] >= 1 && (a->ksize[i] & 1) && a->ksize[i] <= MPHSIR_DEG_STENCIL_SIDE,
                       "degrade_batch: stencil %d has side %d: must be odd and <= %d", i, a->ksize[i], MPHSIR_DEG_STENCIL_SIDE);
        d.ksize[i] = a->ksize[i];
        if (a->ksize[i] / 2 > hmax) hmax = a->ksize[i] / 2;
    }
    for (int i = 0; i < a->F; ++i) {
        const int f = a->sr_factor[i];
        MPHSIR_REQUIRE(f >= 1 && N % f == 0 && N / f >= 2, "degrade_batch: sr factor %d must divide N = %d and leave N / f >= 2", f, N);
        d.factor[i] = f;
        if (fmin == 0 || f < fmin) fmin = f;
    }
    const bool perb = has(MPHSIR_DEG_GAUSSIAN) || has(MPHSIR_DEG_COMPLEX) || has(MPHSIR_DEG_INPAINT) || has(MPHSIR_DEG_HAZE);
    const bool subb = has(MPHSIR_DEG_COMPLEX) || has(MPHSIR_DEG_BLUR) || has(MPHSIR_DEG_SR);
    MPHSIR_REQUIRE((!perb || a->param) && (!subb || a->sub), "degrade_batch: a kind of the menu reads `param` / `sub`, which is NULL");
    MPHSIR_REQUIRE(!has(MPHSIR_DEG_COMPLEX) || (a->band_sigma && a->band_flag && a->col_dead && a->col_off),
                   "degrade_batch: complexN reads band_sigma, band_flag, col_dead and col_off: one is NULL");
    MPHSIR_REQUIRE(!has(MPHSIR_DEG_BANDMISS) || a->band_flag, "degrade_batch: bandmiss reads band_flag, which is NULL");
    MPHSIR_REQUIRE(!has(MPHSIR_DEG_BLUR) || (a->K > 0 && a->stencils), "degrade_batch: blur needs a stencil table (K %d)", a->K);
    MPHSIR_REQUIRE(!has(MPHSIR_DEG_SR) || a->F > 0, "degrade_batch: sr needs a factor table (F %d)", a->F);
    MPHSIR_REQUIRE(!has(MPHSIR_DEG_HAZE) || (a->cirrus && a->atm && a->haze_ratio), "degrade_batch: haze reads cirrus, atm and haze_ratio: one is NULL");
    if (!has(MPHSIR_DEG_BLUR)) hmax = 0;
    // the plane (4 floats of slack: the last quad of a blur row may read past a row that is no multiple of 4 wide), then one region that
    // holds the low-resolution image of an sr sample or the weights of a blur sample
    const long P = N + 2 * hmax, plane = P * (P | 1) + 4;
    long low = has(MPHSIR_DEG_SR) ? (long)(N / fmin) * (N / fmin) : 0;
    if (has(MPHSIR_DEG_BLUR) && low < DG_SS * DG_SS) low = DG_SS * DG_SS;
    const size_t shmem = (size_t)(plane + low) * sizeof(float);
    MPHSIR_REQUIRE(shmem <= 160u * 1024u, "degrade_batch: %zu bytes of LDS for N = %d, halo %d: more than a workgroup can have", shmem, N, hmax);
    d.clean = a->clean; d.degraded = a->degraded; d.clean_aug = a->clean_aug;
    d.task = a->task; d.aug = a->aug; d.param = a->param; d.sub = a->sub;
    d.band_sigma = a->band_sigma; d.band_flag = a->band_flag; d.col_dead = a->col_dead; d.col_off = a->col_off;
    d.stencils = a->stencils; d.cirrus = a->cirrus; d.atm = a->atm; d.haze_ratio = a->haze_ratio;
    d.z = a->z; d.u0 = a->u0; d.u1 = a->u1;
    d.ordinal_dev = reinterpret_cast<const long long*>(a->ordinal_dev);
    d.seed = (unsigned long long)a->seed; d.ordinal = a->ordinal;
    d.C = a->C; d.N = N; d.T = a->T; d.K = a->K; d.F = a->F; d.low_off = (int)plane;
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
