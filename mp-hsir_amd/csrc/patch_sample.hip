// Training patches cut out of the resident scene store (mp-hsir_amd/scene_store.py; include/mphsir.h holds the definitions): a batch of
// records (level, y, x) -> out [B][C][P][P] = (p - min p) / (max p - min p), p the C x P x P window of the record's level in the arena.
//
//   patch_minmax_kernel      a workgroup owns one (sample, band) plane of the window: every thread folds the quads it reads into a running
//                            min, max and a NaN flag (comparisons, so that a NaN is seen and not dropped), the wave folds by shuffles, the
//                            four waves through LDS; thread 0 writes {min, max} of the plane to the workspace, both NaN when it holds one.
//   patch_normalise_kernel   a workgroup owns the same plane: it combines the C pairs of its sample (min / max are exact and commutative:
//                            the result does not depend on the order; a NaN pair poisons it), reads the plane a second time -- 16 KiB at
//                            P = 64 that its twin of launch 1 has just pulled through L2 -- and writes (v - lo) / (hi - lo) as 16-byte rows.
//
// Two launches because the extremes are over ALL bands of a sample: a plane cannot be normalised before every plane of its sample has
// been reduced, and the pair needs neither atomics nor a grid-wide wait.  A workgroup per plane (992 at 32 x 31, 3200 at 32 x 100)
// keeps every CU busy and every thread's loads independent (4 quads at P = 64, issued back to back).
//
// Source rows are read as 16-byte vectors when the plane's first element is 16-byte aligned and W % 4 == 0 (then every row start is);
// that holds for every grid record of a store cropped to multiples of 128 / 256.  Jittered origins and odd widths take the element-wise
// path, written as four dword loads per quad (the compiler is free to merge them into one 16-byte request, which gfx950 serves at dword
// alignment; the code does not rely on it).  The decision is uniform over the workgroup.
//
// Bounds: index, level, y, x come from device memory and are clamped into [0, n_records), [0, n_levels), [0, H - P], [0, W - P]; the
// host has verified on its copy of the level table that P <= H, P <= W and offset + C H W <= arena_elems for every level, so every read
// lies inside the arena.  All element offsets are 64-bit.  Workspace slot (b, c) lies inside the 8 B C bytes the host verified; out
// element (b, c, r, x) inside [B][C][P][P].
#include <math.h>

#include "mphsir_host.h"
#include "mphsir_planar.h"

namespace mphsir {

constexpr int PS_NT = 256;
constexpr int PS_MAX_P = 4096;
constexpr int PS_U = 4;              // quads a thread has in flight per round: the whole plane in one round at P = 64

struct PatchDev {
    const float* arena; const int64_t* levels; const int32_t* records; const int64_t* index; float* out; float* ws;
    int n_levels, n_records, C, P;
};

// the window of sample b, band c: pointer to its first element and the level's row pitch
__device__ __forceinline__ const float* ps_plane(const PatchDev& a, int b, int c, int& W) {
    long r = a.index ? (long)a.index[b] : (long)b;
    r = r < 0 ? 0 : (r >= a.n_records ? a.n_records - 1 : r);
    const int32_t* rec = a.records + 3 * r;
    int l = rec[0];
    l = l < 0 ? 0 : (l >= a.n_levels ? a.n_levels - 1 : l);
    const int64_t* lv = a.levels + 3 * (long)l;
    const long off = lv[0];
    const int H = (int)lv[1];
    W = (int)lv[2];
    int y = rec[1], x = rec[2];
    y = y < 0 ? 0 : (y > H - a.P ? H - a.P : y);
    x = x < 0 ? 0 : (x > W - a.P ? W - a.P : x);
    return a.arena + off + ((long)c * H + y) * (long)W + x;
}

// grid (C, B)
__global__ __launch_bounds__(PS_NT) void patch_minmax_kernel(PatchDev a) {
    __shared__ float red[PS_NT / 64][3];
    const int t = threadIdx.x;
    const int c = blockIdx.x, b = blockIdx.y;
    int W;
    const float* src = ps_plane(a, b, c, W);
    const bool vec = (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (W & 3) == 0;
    const int p4 = a.P >> 2, quads = a.P * p4;
    float mn = INFINITY, mx = -INFINITY, bad = 0.f;
    for (int q0 = t; q0 < quads; q0 += PS_U * PS_NT) {
        f32x4 v[PS_U];
#pragma unroll
        for (int u = 0; u < PS_U; ++u) {                  // all loads of the round first: PS_U independent 16-byte requests in flight
            const int q = q0 + u * PS_NT, r = q / p4, x = (q - r * p4) * 4;
            if (q < quads) v[u] = load4_if(src + (long)r * W + x, vec, 4);
        }
#pragma unroll
        for (int u = 0; u < PS_U; ++u) {
            if (q0 + u * PS_NT < quads) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    mn = v[u][k] < mn ? v[u][k] : mn;
                    mx = v[u][k] > mx ? v[u][k] : mx;
                    bad = v[u][k] != v[u][k] ? 1.f : bad;
                }
            }
        }
    }
    minmax_fold<PS_NT>(mn, mx, bad, red);
    if (t == 0) minmax_store(a.ws + 2 * ((long)b * a.C + c), mn, mx, bad);
}

// grid (C, B)
__global__ __launch_bounds__(PS_NT) void patch_normalise_kernel(PatchDev a) {
    __shared__ float red[PS_NT / 64][3];
    const int t = threadIdx.x;
    const int c = blockIdx.x, b = blockIdx.y;
    float lo, den;
    minmax_combine<PS_NT>(a.ws + 2 * (long)b * a.C, a.C, red, lo, den);      // the sample's extremes from its C plane pairs

    int W;
    const float* src = ps_plane(a, b, c, W);
    const bool vec = (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (W & 3) == 0;
    const int p4 = a.P >> 2, quads = a.P * p4;
    float* dst = a.out + ((long)b * a.C + c) * (long)a.P * a.P;
    for (int q0 = t; q0 < quads; q0 += PS_U * PS_NT) {
        f32x4 v[PS_U];
#pragma unroll
        for (int u = 0; u < PS_U; ++u) {
            const int q = q0 + u * PS_NT, r = q / p4, x = (q - r * p4) * 4;
            if (q < quads) v[u] = load4_if(src + (long)r * W + x, vec, 4);
        }
#pragma unroll
        for (int u = 0; u < PS_U; ++u) {
            const int q = q0 + u * PS_NT;
            if (q < quads) {
                f32x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = div_rn(v[u][k] - lo, den);
                *reinterpret_cast<f32x4*>(dst + 4 * (long)q) = o;
            }
        }
    }
}

static bool patch_sizes_ok(int B, int C) { return B > 0 && B <= 65535 && C > 0 && C <= 65535; }

}  // namespace mphsir

extern "C" int64_t mphsir_patch_sample_workspace_bytes(int32_t B, int32_t C) {
    if (!mphsir::patch_sizes_ok(B, C)) return MPHSIR_EINVAL;
    return (int64_t)8 * B * C;
}

extern "C" int mphsir_patch_sample(const mphsir_patch_sample_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "patch_sample");
    MPHSIR_REQUIRE(a->arena && a->levels && a->levels_host && a->records && a->out && a->workspace, "patch_sample: null pointer");
    MPHSIR_REQUIRE(patch_sizes_ok(a->B, a->C), "patch_sample: bad sizes (B %d, C %d; both in 1..65535)", a->B, a->C);
    MPHSIR_REQUIRE(a->P > 0 && a->P % 4 == 0 && a->P <= PS_MAX_P, "patch_sample: P %d must be a positive multiple of 4, at most %d", a->P, PS_MAX_P);
    MPHSIR_REQUIRE(aligned16(a->out), "patch_sample: out must be 16-byte aligned");
    MPHSIR_REQUIRE(a->n_levels > 0 && a->n_records > 0 && (a->index || a->n_records >= a->B),
                   "patch_sample: %d levels, %d records for a batch of %d (without an index array every sample has its own record)",
                   a->n_levels, a->n_records, a->B);
    const int64_t need = mphsir_patch_sample_workspace_bytes(a->B, a->C);
    MPHSIR_REQUIRE(a->workspace_bytes >= need && (reinterpret_cast<uintptr_t>(a->workspace) & 7) == 0,
                   "patch_sample: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)a->workspace_bytes, (long long)need);
    for (int l = 0; l < a->n_levels; ++l) {
        const int64_t off = a->levels_host[3 * (int64_t)l], H = a->levels_host[3 * (int64_t)l + 1], W = a->levels_host[3 * (int64_t)l + 2];
        MPHSIR_REQUIRE(H >= a->P && W >= a->P, "patch_sample: a window of %d x %d leaves level %d (%lld x %lld)", a->P, a->P, l, (long long)H, (long long)W);
        MPHSIR_REQUIRE(H * W < (1LL << 31) && off >= 0 && off <= a->arena_elems && (int64_t)a->C * H * W <= a->arena_elems - off,
                       "patch_sample: level %d (offset %lld, %d x %lld x %lld) leaves the arena of %lld elements", l, (long long)off, a->C,
                       (long long)H, (long long)W, (long long)a->arena_elems);
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PatchDev d{a->arena, a->levels, a->records, a->index, a->out, static_cast<float*>(a->workspace), a->n_levels, a->n_records, a->C, a->P};
    MPHSIR_LAUNCH(MPHSIR_K_PATCH_SAMPLE, patch_minmax_kernel, dim3((unsigned)a->C, (unsigned)a->B), dim3(PS_NT), 0, s, d);
    MPHSIR_LAUNCH(MPHSIR_K_PATCH_NORMALISE, patch_normalise_kernel, dim3((unsigned)a->C, (unsigned)a->B), dim3(PS_NT), 0, s, d);
    return MPHSIR_OK;
}
