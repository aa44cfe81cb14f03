// arena utilities: the two places where hundreds of tiny framework kernels per step are replaced by one launch each.
//
//  * reduce_parts: every split-M / per-workgroup partial buffer a backward function produced (gemm_tn tiles and
//    column sums, LayerNorm / rel-pos-bias / depthwise-tap / fold partials) is summed in a fixed order by ONE launch
//    over up to MPHSIR_REDUCE_MAX_SEGS segments (the reference: one at::sum per parameter gradient).  Fixed summation
//    order, no atomics: bitwise reproducible.
//  * pack_gather: all kernel-layout weights (cast to the compute dtype, padded, transposed, split, gathered) are one
//    gather from the flat fp32 parameter arena through a static int32 index map built once from the packers
//    (host: engine.PackPlan); index < 0 = zero padding.  Runs right after flat_adamw inside the captured step.
#include <stdlib.h>

#include "../../include/mphsir_accum.h"
#include "mphsir_host.h"
#include "mphsir_planar.h"

namespace mphsir {

struct RedSegDev {
    const float* src; float* dst;
    long n, stride, sbs, dbs, t0, nitems; // t0: first thread of this segment (a multiple of 64: waves never straddle segments)
    long src_ld, dst_ld;                  // 2-D form: row pitches (rows x n block of a wider matrix)
    int nsplit, vec, lg, rows, dcs;       // 2^lg adjacent lanes share one work item (4 consecutive outputs) and split the split axis
};
struct RedDev {
    RedSegDev s[MPHSIR_REDUCE_MAX_SEGS];
    int nseg; long threads;
};

__global__ __launch_bounds__(256) void reduce_parts_kernel(RedDev a) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.threads) return;            // whole waves only (threads is a multiple of 64)
    // constant indices only: a dynamically indexed by-value kernel argument would be copied to scratch by every lane
    RedSegDev s = a.s[0];
#pragma unroll
    for (int k = 1; k < MPHSIR_REDUCE_MAX_SEGS; ++k)
        if (k < a.nseg && t >= a.s[k].t0) s = a.s[k];
    const int G = 1 << s.lg;
    const long local = t - s.t0, item = local >> s.lg, ipr = (s.n + 3) / 4, ipb = ipr * s.rows;
    const int g = (int)(local & (G - 1));
    const bool live = item < s.nitems;
    const long b = live ? item / ipb : 0, rem = live ? item % ipb : 0, r = rem / ipr, i4 = (rem % ipr) * 4;
    const float* src = s.src + b * s.sbs + r * s.src_ld + i4;
    const int ne = (s.n - i4) < 4 ? (int)(s.n - i4) : 4;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if (live) {
        // 8 independent loads (16-byte ones where the source allows: bit 0 of `vec`) in flight per lane -- the kernel is a latency
        // chain of strided L2 reads -- summed in split order.  (Until round 5 only the all-vector segments did this; the others -- tap
        // gradients written transposed, the 450-wide relative-position-bias rows with 2048 splits -- walked their splits one by one
        // and set the time of the launch: 60 us for 69 MB.)
        int sp = g;
        if (s.vec & 1) {
            for (; sp + 7 * G < s.nsplit; sp += 8 * G) {
                f32x4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const f32x4*>(src + (long)(sp + u * G) * s.stride);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += v[u];
            }
            for (; sp < s.nsplit; sp += G) acc += *reinterpret_cast<const f32x4*>(src + (long)sp * s.stride);
        } else {
            for (; sp + 7 * G < s.nsplit; sp += 8 * G) {
                f32x4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    for (int e = 0; e < 4; ++e) v[u][e] = e < ne ? src[(long)(sp + u * G) * s.stride + e] : 0.f;
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += v[u];
            }
            for (; sp < s.nsplit; sp += G)
                for (int e = 0; e < ne; ++e) acc[e] += src[(long)sp * s.stride + e];
        }
    }
    // fixed xor tree over the lanes of the group: the summation order depends on (nsplit, G) only -> deterministic
    for (int m = 1; m < G; m <<= 1)
        for (int e = 0; e < 4; ++e) acc[e] += __shfl_xor(acc[e], m);
    if (live && g == 0) {
        float* dst = s.dst + b * s.dbs + r * s.dst_ld + i4 * s.dcs;
        if (s.vec & 2) *reinterpret_cast<f32x4*>(dst) = acc;
        else
            for (int e = 0; e < ne; ++e) dst[(long)e * s.dcs] = acc[e];
    }
}

// 4 elements per thread (one 16-byte store for fp32, 8 bytes for the 16-bit types) and one 256-thread workgroup per 1024 elements.  What was
// measured on the 12.8 M-element bf16 pack of the natural-scene net (rocprofv3, round 6): 8 elements per thread grid-strided over 4096
// workgroups 113 us; one piece per workgroup 99; 4 / 8 / 16 CONSECUTIVE pieces per workgroup (every source cache line used whole: the
// transposed copies otherwise re-fetch them, 311 MB read for 25.6 MB written) 139 / 143 / 131 -- the gather is bound by the number of
// distinct lines a wave asks for per instruction, not by bytes, and wants threads, not locality; 4 elements per thread 92.
template <class T>
__global__ __launch_bounds__(256) void pack_gather_kernel(const float* arena, const int* idx, T* dst, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n / 4) return;
    const int* ip = idx + i * 4;
    const int i0 = ip[0], i1 = ip[1], i2 = ip[2], i3 = ip[3];
    f32x4 v;
    v[0] = i0 >= 0 ? arena[i0] : 0.f;
    v[1] = i1 >= 0 ? arena[i1] : 0.f;
    v[2] = i2 >= 0 ? arena[i2] : 0.f;
    v[3] = i3 >= 0 ? arena[i3] : 0.f;
    store4<T>(dst + i * 4, v);
}

// multi_copy: the gradient hand-over.  autograd leaves ~370 freshly allocated fp32 gradient tensors; each goes to its slot of the flat
// gradient arena.  (torch._foreach_copy_ took 11 launches of its multi-tensor kernel, 0.2 ms per step.)  One launch: the table --
// rows {src, dst, n floats, first block} in DEVICE memory -- is searched by block index; a block moves up to 4096 floats.
constexpr int MC_BLOCK = 4096;
__global__ __launch_bounds__(256) void multi_copy_kernel(const long* __restrict__ table, int nseg) {
    const long b = blockIdx.x;
    int lo = 0, hi = nseg - 1;                               // the last row whose first block is <= b (wave-uniform: scalar loads)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[4 * mid + 3] <= b) lo = mid; else hi = mid - 1;
    }
    const float* src = reinterpret_cast<const float*>(table[4 * lo]);
    float* dst = reinterpret_cast<float*>(table[4 * lo + 1]);
    const long n = table[4 * lo + 2], e0 = (b - table[4 * lo + 3]) * MC_BLOCK;
    const long e1 = e0 + MC_BLOCK < n ? e0 + MC_BLOCK : n;
    if ((((unsigned long)src | (unsigned long)dst) & 15) == 0) {
        for (long e = e0 + 4 * threadIdx.x; e + 4 <= e1; e += 1024) *reinterpret_cast<f32x4*>(dst + e) = *reinterpret_cast<const f32x4*>(src + e);
        for (long e = e0 + ((e1 - e0) & ~3L) + threadIdx.x; e < e1; e += 256) dst[e] = src[e];
    } else {
        for (long e = e0 + threadIdx.x; e < e1; e += 256) dst[e] = src[e];
    }
}

// multi_accum: the same hand-over for gradient accumulation (K micro-batches per optimizer step): micro index 0 stores (dst is not
// read: whatever the arena held, a NaN included, is overwritten, so nothing is ever zero-filled), index >= 1 adds, one fp32 addition per
// element (no multiply anywhere: nothing a compiler could contract).  The index comes from the host or -- a captured launch that
// serves every micro-batch of a group -- from a device int32; either way it is the same for the whole grid: a scalar load and a
// scalar branch.  Table, blocks, row search, the 16-byte / per-element paths and the tail are multi_copy's; every dst element belongs
// to exactly one thread, so the result does not depend on the geometry.
// Bounds: exactly multi_copy's -- a block touches elements [e0, e1) of its row only, e1 <= n.
__global__ __launch_bounds__(256) void multi_accum_kernel(const long* __restrict__ table, int nseg, int micro, const int* __restrict__ micro_dev) {
    const int m = micro_dev != nullptr ? *micro_dev : micro;
    const long b = blockIdx.x;
    int lo = 0, hi = nseg - 1;                               // the last row whose first block is <= b (wave-uniform: scalar loads)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[4 * mid + 3] <= b) lo = mid; else hi = mid - 1;
    }
    const float* src = reinterpret_cast<const float*>(table[4 * lo]);
    float* dst = reinterpret_cast<float*>(table[4 * lo + 1]);
    const long n = table[4 * lo + 2], e0 = (b - table[4 * lo + 3]) * MC_BLOCK;
    const long e1 = e0 + MC_BLOCK < n ? e0 + MC_BLOCK : n;
    const bool vec = (((unsigned long)src | (unsigned long)dst) & 15) == 0;
    const long t0 = vec ? e0 + ((e1 - e0) & ~3L) : e0;       // where the per-element part begins
    if (m <= 0) {
        if (vec)
            for (long e = e0 + 4 * threadIdx.x; e + 4 <= e1; e += 1024) *reinterpret_cast<f32x4*>(dst + e) = *reinterpret_cast<const f32x4*>(src + e);
        for (long e = t0 + threadIdx.x; e < e1; e += 256) dst[e] = src[e];
    } else {
        if (vec)
            for (long e = e0 + 4 * threadIdx.x; e + 4 <= e1; e += 1024) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(dst + e), s = *reinterpret_cast<const f32x4*>(src + e);
                *reinterpret_cast<f32x4*>(dst + e) = d + s;
            }
        for (long e = t0 + threadIdx.x; e < e1; e += 256) dst[e] = dst[e] + src[e];
    }
}

// l1_clamp_loss: the training loss of the reference (train.py:58-61: clamp(restored, 0, 1), nn.L1Loss) and its gradient in one
// pass: part[block] = sum |clamp(y) - c| / n over the block's elements, g = sign(clamp(y) - c) * [0 <= y <= 1] / n (clamp's
// autograd passes the gradient where 0 <= y <= 1, bounds included; sign(0) = 0).  The caller sums the partials in order.
// The clamp PROPAGATES NaN like torch.clamp (two compares, both false for a NaN; fminf / fmaxf would return the bound and a
// diverged run would log a plausible finite loss): a NaN output makes the loss NaN, its gradient entry 0 as in the reference.
__global__ __launch_bounds__(256) void l1_clamp_loss_kernel(const float* __restrict__ y, const float* __restrict__ c, float* __restrict__ g,
                                                            float* __restrict__ part, long n, float inv_n) {
    __shared__ float red[4];
    float acc = 0.f;
    const long stride = (long)gridDim.x * 1024;
    for (long e = (long)blockIdx.x * 1024 + 4 * threadIdx.x; e < n; e += stride) {
        if (e + 4 <= n) {
            const f32x4 yv = *reinterpret_cast<const f32x4*>(y + e), cv = *reinterpret_cast<const f32x4*>(c + e);
            f32x4 gv;
            for (int i = 0; i < 4; ++i) {
                const float d = clamp01(yv[i]) - cv[i];
                acc += fabsf(d);
                gv[i] = (yv[i] >= 0.f && yv[i] <= 1.f) ? (d > 0.f ? inv_n : (d < 0.f ? -inv_n : 0.f)) : 0.f;
            }
            if (g) *reinterpret_cast<f32x4*>(g + e) = gv;
        } else {
            for (long k = e; k < n; ++k) {
                const float d = clamp01(y[k]) - c[k];
                acc += fabsf(d);
                if (g) g[k] = (y[k] >= 0.f && y[k] <= 1.f) ? (d > 0.f ? inv_n : (d < 0.f ? -inv_n : 0.f)) : 0.f;
            }
        }
    }
    acc = wave_sum(acc);
    if (lane_id() == 0) red[wave_id()] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) * inv_n;
}

}  // namespace mphsir

extern "C" int mphsir_multi_copy(const int64_t* table_dev, int32_t nseg, int64_t total_blocks, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_REQUIRE(table_dev && nseg > 0 && total_blocks > 0 && total_blocks < (1LL << 31), "multi_copy: bad arguments");
    static_assert(sizeof(long) == sizeof(int64_t), "table rows are 64-bit");
    MPHSIR_LAUNCH(MPHSIR_K_MULTI_COPY, multi_copy_kernel, dim3((unsigned)total_blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                  reinterpret_cast<const long*>(table_dev), (int)nseg);
    return MPHSIR_OK;
}

extern "C" int mphsir_multi_accum(const mphsir_multi_accum_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "multi_accum");
    MPHSIR_REQUIRE(a->table_dev && a->nseg > 0, "multi_accum: a null table or no rows (nseg %d)", a->nseg);
    MPHSIR_REQUIRE(a->total_blocks > 0 && a->total_blocks < (1LL << 31), "multi_accum: total_blocks %lld outside 1 .. 2^31 - 1", (long long)a->total_blocks);
    MPHSIR_REQUIRE(a->micro >= 0, "multi_accum: micro index %d is negative", a->micro);
    // under the hand-over's id: the launch timer reports the family (as the SSIM pair launches under the spectral-loss ids), MPHSIR_K_COUNT stays
    MPHSIR_LAUNCH(MPHSIR_K_MULTI_COPY, multi_accum_kernel, dim3((unsigned)a->total_blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                  reinterpret_cast<const long*>(a->table_dev), (int)a->nseg, (int)a->micro, reinterpret_cast<const int*>(a->micro_dev));
    return MPHSIR_OK;
}

extern "C" int mphsir_l1_clamp_loss(const float* y, const float* clean, float* grad, float* part, int64_t n, int32_t nblocks, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_REQUIRE(y && clean && part && n > 0 && nblocks > 0 && nblocks <= 65535, "l1_clamp_loss: bad arguments");
    MPHSIR_REQUIRE(aligned16(y) && aligned16(clean) && (grad == nullptr || aligned16(grad)), "l1_clamp_loss: 16-byte alignment required");
    MPHSIR_LAUNCH(MPHSIR_K_L1_LOSS, l1_clamp_loss_kernel, dim3((unsigned)nblocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                  y, clean, grad, part, (long)n, 1.0f / (float)n);
    return MPHSIR_OK;
}

extern "C" int mphsir_reduce_parts(const mphsir_reduce_seg* segs, int32_t nseg, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_REQUIRE(segs && nseg > 0 && nseg <= MPHSIR_REDUCE_MAX_SEGS, "reduce_parts: 1..%d segments per call", MPHSIR_REDUCE_MAX_SEGS);
    RedDev d;
    d.nseg = nseg;
    long threads = 0;
    for (int k = 0; k < nseg; ++k) {
        const mphsir_reduce_seg& g = segs[k];
        MPHSIR_REQUIRE(g.src && g.dst && g.n > 0 && g.nsplit > 0 && g.nbatch > 0, "reduce_parts: bad segment %d", k);
        const int rows = g.rows > 1 ? g.rows : 1, dcs = g.dst_col_stride > 0 ? g.dst_col_stride : 1;
        const long src_ld = rows > 1 ? (long)g.src_ld : 0, dst_ld = rows > 1 ? (long)g.dst_ld : 0;
        const bool vload = aligned16(g.src) && g.n % 4 == 0 && g.stride % 4 == 0 && g.src_batch_stride % 4 == 0 && src_ld % 4 == 0;
        const bool vstore = vload && aligned16(g.dst) && dcs == 1 && g.dst_batch_stride % 4 == 0 && dst_ld % 4 == 0;
        const long nitems = (long)g.nbatch * rows * ((g.n + 3) / 4);
        int lg = 0;                        // lanes per item: keep <= 32 splits per lane, and small segments still fill waves
        while (lg < 6 && (g.nsplit >> lg) > 32) ++lg;      // (<= 8 / <= 4 per lane measured in round 5: 21.10 / 21.29 against 21.09 ms per step)
        while (lg < 6 && (nitems << lg) < 8192 && (g.nsplit >> lg) > 4) ++lg;      // (32 k / 64 k / 128 k threads measured: no difference)
        d.s[k] = RedSegDev{g.src, g.dst, (long)g.n, (long)g.stride, (long)g.src_batch_stride, (long)g.dst_batch_stride, threads, nitems,
                           src_ld, dst_ld, g.nsplit, (vload ? 1 : 0) | (vstore ? 2 : 0), lg, rows, dcs};
        threads += ((nitems << lg) + 63) / 64 * 64;
    }
    d.threads = threads;
    MPHSIR_LAUNCH(MPHSIR_K_REDUCE_PARTS, reduce_parts_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0,
                  reinterpret_cast<hipStream_t>(stream), d);
    return MPHSIR_OK;
}

extern "C" int mphsir_pack_gather(const float* arena, const int32_t* index, void* dst, int64_t n, int dtype, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_REQUIRE(arena && index && dst, "pack_gather: null pointer");
    MPHSIR_REQUIRE(MPHSIR_DTYPE_OK(dtype), "pack_gather: dtype %d unsupported", dtype);
    const int vec = dtype == MPHSIR_F32 ? 4 : 8;
    MPHSIR_REQUIRE(n > 0 && n % vec == 0 && aligned16(index) && aligned16(dst), "pack_gather: n must be a multiple of %d, 16-byte alignment", vec);
    const dim3 grid((unsigned)((n / 4 + 255) / 256));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MPHSIR_F32) {
        MPHSIR_LAUNCH(MPHSIR_K_PACK_GATHER, pack_gather_kernel<float>, grid, dim3(256), 0, s, arena, index, reinterpret_cast<float*>(dst), (long)n);
    } else if (dtype == MPHSIR_BF16) {
        MPHSIR_LAUNCH(MPHSIR_K_PACK_GATHER, pack_gather_kernel<bf16_t>, grid, dim3(256), 0, s, arena, index, reinterpret_cast<bf16_t*>(dst), (long)n);
    } else {
        MPHSIR_LAUNCH(MPHSIR_K_PACK_GATHER, pack_gather_kernel<f16_t>, grid, dim3(256), 0, s, arena, index, reinterpret_cast<f16_t*>(dst), (long)n);
    }
    return MPHSIR_OK;
}

// ---- ssim_loss: the SSIM term of the training loss, w (1 - SSIM), and its gradient in one launch pair (include/mphsir.h holds the
// definitions; mp-hsir_amd/ops.py ssim_loss_grad, engine.SpectralLoss(ssim=) the Python side).  The SSIM is the one quality.hip reports.
//
//   ssim_loss_kernel          a workgroup owns SSL_TH x SSL_TW = 16 x 32 pixels of one image and walks the bands.  A pixel lies in the 49
//                             windows centred within 3 of it, and those reach 3 further: per band the workgroup stages its pixels plus a
//                             6-pixel halo of both cubes (x clipped to [0,1]; fp32 -> fp64 is exact, so the stage is fp32) and then, in
//                             float64 throughout,
//                               1. the five 7-wide row sums (x, c, xx, cc, xc) of every staged row at the 38 centre columns,
//                               2. seven rows of them per window centre (22 x 38 centres: the tile plus 3 around it) -> S_w and the three
//                                  coefficients a_w = d_w - ux_w b_w - uy_w c_w, b_w, c_w of include/mphsir.h, 0 where the window does not
//                                  lie inside the plane; S_w of the centres inside the tile is added to the thread's partial,
//                               3. the 7-wide row sums of the three coefficient maps at the 32 pixel columns,
//                               4. seven rows of them per pixel: g = scale (sum a + x_p sum b + c_p sum c), scale = -w / (49 B C Nw), rounded
//                                  to fp32 once, 0 where y_p is outside [0,1], written (or added to what `grad` holds: accumulate).
//                             The uncentred form (three box sums) loses log2(|terms| / |g|) ~ 10 bits on smooth planes -- of 53.
//                             The next band's loads are issued before the current band's arithmetic and land in registers meanwhile.
//                             The coefficient maps share their LDS with the stage (dead once the row sums exist), the second row sums
//                             with the first: 62.6 KB, two workgroups per CU; four barriers per band.
//                             After the last band the workgroup's float64 sum of S_w goes to its workspace slot.
//   ssim_loss_finish_kernel   one workgroup: the partials summed by thread in ascending block order, the lanes by a fixed shuffle tree, the
//                             four waves in order; writes {base + w (1 - SSIM), SSIM} as fp32, each rounded once.
//
// No atomics, nothing zero-filled, no sum whose order depends on scheduling.  Both launch under the kernel ids of the spectral-loss pair
// (MPHSIR_K_SPECTRAL_LOSS, MPHSIR_K_SPECTRAL_LOSS_FINISH: the loss family of the launch timer), as quality_meter launches under
// MPHSIR_K_QUALITY: MPHSIR_K_COUNT stays.  One path for every alignment: the loads and stores are per element.
//
// Bounds: every global read is at an image coordinate checked against [0,H) x [0,W) (H W < 2^31: the plane offset is an int; positions
// outside are staged as 0 and only enter windows whose coefficients are replaced by 0 and whose S is not counted); a gradient element is
// stored only where its pixel is inside the image; LDS indices: stage rows < 28, columns < 44; row sums [5][28][38], a pair of columns
// 2 i, 2 i + 1 <= 37 reads stage columns <= 44 - 1; coefficient maps [3][22][38], a pair of centre rows 2 i, 2 i + 1 <= 21 reads row sums
// <= 27; second row sums [3][22][32] read map columns <= 31 + 6; a pixel pair reads their rows <= 15 + 6.  Workspace slot blk < B * tiles
// lies inside the 8 B tiles bytes the host verified.
// Aliasing: `mp` is the stage, then the maps; `hs` the first row sums, then the second.  With a gradient a band has four barriers: stage
// written | B1 | stage read, hs written | B2 | hs read, maps written over the stage | B3 | maps read, hs rewritten | B4 | hs read; the next
// stage write comes behind B4 (the maps are dead), the next hs write behind the next B1 (step 4 is over).  WITHOUT a gradient (grad == NULL,
// the same for the whole workgroup) a band has B1 and B2 only and writes neither the maps nor the second row sums: the next stage write
// follows B2 of the same band (the stage's last readers, step 1 and cp, are in front of B2), the next hs write follows the next B1 (step
// 2, the last reader of hs, is in front of it).  Anything added behind step 2 on that path that reads `mp` or writes `hs` needs a barrier of
// its own.
//
// No multiply-add is fused from here on (spectral_loss.hip has the reason; the kernels above hold no a * b + c).
#pragma clang fp contract(off)

namespace mphsir {

constexpr int SSL_TH = 16, SSL_TW = 32, SSL_R = 3, SSL_NT = 256;
constexpr int SSL_SH = SSL_TH + 4 * SSL_R, SSL_SW = SSL_TW + 4 * SSL_R;         // the stage: 28 x 44
constexpr int SSL_CH = SSL_TH + 2 * SSL_R, SSL_CW = SSL_TW + 2 * SSL_R;         // window centres a workgroup evaluates: 22 x 38
constexpr int SSL_LD = (SSL_SH * SSL_SW + SSL_NT - 1) / SSL_NT;                 // staged elements per thread and cube
constexpr int SSL_RPT = SSL_TH / (SSL_NT / SSL_TW);                             // rows a thread owns in its column
constexpr int SSL_HS = 5 * SSL_SH * SSL_CW, SSL_MAPS = 3 * SSL_CH * SSL_CW;     // doubles
static_assert(SSL_RPT == 2 && SSL_CW % 2 == 0 && SSL_CH % 2 == 0 && SSL_TW % 2 == 0 && SSL_R == 3, "pairs of columns / rows share six of their seven samples");
static_assert(2 * SSL_SH * SSL_SW * 4 <= SSL_MAPS * 8 && 3 * SSL_CH * SSL_TW <= SSL_HS, "the maps lie over the stage, the second row sums over the first");
static_assert((SSL_HS + SSL_MAPS + 4) * 8 <= 64 * 1024, "static LDS");

struct SsimLossDev {
    const float* y; const float* c; float* g; double* ws;
    int C, H, W, tiles_x, tiles;
    int accumulate;
    double scale;               // -w / (49 B C Nw)
};

// the seven-term sums of two neighbouring positions from their eight samples: plain sums, nothing is subtracted
__device__ __forceinline__ void ssl_pair(const double* v, double& s0, double& s1) {
    const double core = ((v[1] + v[2]) + (v[3] + v[4])) + (v[5] + v[6]);
    s0 = v[0] + core;
    s1 = core + v[7];
}

// grid (B * tiles): workgroup blk owns tile blk % tiles of image blk / tiles
__global__ __launch_bounds__(SSL_NT) void ssim_loss_kernel(SsimLossDev a) {
    __shared__ double hs[SSL_HS];                   // [5][28][38] row sums, later [3][22][32] row sums of the coefficient maps
    __shared__ double mp[SSL_MAPS];                 // the fp32 stage [2][28][44], later the coefficient maps [3][22][38]
    __shared__ double red[SSL_NT / 64];
    float* sx = reinterpret_cast<float*>(mp);
    float* sc = sx + SSL_SH * SSL_SW;

    const int t = threadIdx.x, lane = t & 63, wave = wave_id_uniform();
    const int b = blockIdx.x / a.tiles, blk = blockIdx.x - b * a.tiles;
    const int by = blk / a.tiles_x, bx = blk - by * a.tiles_x;
    const int y0 = by * SSL_TH, x0 = bx * SSL_TW;
    const long plane = (long)a.H * a.W;
    const float* py = a.y + (long)b * a.C * plane;
    const float* pc = a.c + (long)b * a.C * plane;

    int off[SSL_LD];                                                        // plane offset of staged element t + k * SSL_NT, -1 outside
#pragma unroll
    for (int k = 0; k < SSL_LD; ++k) {
        const int e = t + k * SSL_NT, r = e / SSL_SW, c = e - r * SSL_SW;
        const int gy = y0 - 2 * SSL_R + r, gx = x0 - 2 * SSL_R + c;
        off[k] = (e < SSL_SW * SSL_SH && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? gy * a.W + gx : -1;
    }
    const int tx = t & (SSL_TW - 1), tg = t / SSL_TW;
    int own[SSL_RPT];                                                       // plane offset of the thread's own pixels, -1 outside
#pragma unroll
    for (int j = 0; j < SSL_RPT; ++j) {
        const int gy = y0 + tg * SSL_RPT + j, gx = x0 + tx;
        own[j] = (gy < a.H && gx < a.W) ? gy * a.W + gx : -1;
    }

    float rx[SSL_LD], rc[SSL_LD], ry[SSL_RPT];
#pragma unroll
    for (int k = 0; k < SSL_LD; ++k) {
        rx[k] = off[k] >= 0 ? py[off[k]] : 0.f;
        rc[k] = off[k] >= 0 ? pc[off[k]] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < SSL_RPT; ++j) ry[j] = own[j] >= 0 ? py[own[j]] : 0.f;

    double ss = 0.0;
    for (int c = 0; c < a.C; ++c) {
#pragma unroll
        for (int k = 0; k < SSL_LD; ++k) {
            const int e = t + k * SSL_NT;
            if (e < SSL_SW * SSL_SH) {
                sx[e] = clamp01(rx[k]);
                sc[e] = rc[k];
            }
        }
        float yo[SSL_RPT];                                                  // the raw y of the own pixels of band c: the mask is taken of it
#pragma unroll
        for (int j = 0; j < SSL_RPT; ++j) yo[j] = ry[j];
        if (c + 1 < a.C) {
            const float* ny = py + (long)(c + 1) * plane;
            const float* nc = pc + (long)(c + 1) * plane;
#pragma unroll
            for (int k = 0; k < SSL_LD; ++k) {
                rx[k] = off[k] >= 0 ? ny[off[k]] : 0.f;
                rc[k] = off[k] >= 0 ? nc[off[k]] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < SSL_RPT; ++j) ry[j] = own[j] >= 0 ? ny[own[j]] : 0.f;
        }
        __syncthreads();                     // the stage of band c is complete (everyone has left step 4 of band c - 1: see the barrier before it)

        // 1. row sums: staged row r, the windows centred on centre columns col and col + 1
        for (int e = t; e < SSL_SH * (SSL_CW / 2); e += SSL_NT) {
            const int r = e / (SSL_CW / 2), col = (e - r * (SSL_CW / 2)) * 2;
            const float* fx = sx + r * SSL_SW + col;
            const float* fc = sc + r * SSL_SW + col;
            double v[5][8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const double xv = fx[k], cv = fc[k];
                v[0][k] = xv;
                v[1][k] = cv;
                v[2][k] = xv * xv;
                v[3][k] = cv * cv;
                v[4][k] = xv * cv;
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                double* o = hs + (q * SSL_SH + r) * SSL_CW + col;
                ssl_pair(v[q], o[0], o[1]);
            }
        }
        float cp[SSL_RPT];                                                  // clean at the own pixels (0 outside the image)
#pragma unroll
        for (int j = 0; j < SSL_RPT; ++j) cp[j] = sc[(tg * SSL_RPT + j + 2 * SSL_R) * SSL_SW + tx + 2 * SSL_R];
        __syncthreads();                     // the row sums are complete; nobody reads the stage any more: the maps may overwrite it

        // 2. windows: centre rows 2 rp, 2 rp + 1 at centre column j -> S and the three coefficients
        for (int e = t; e < (SSL_CH / 2) * SSL_CW; e += SSL_NT) {
            const int rp = e / SSL_CW, j = e - rp * SSL_CW;
            double S[5][2];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                double v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = hs[(q * SSL_SH + 2 * rp + k) * SSL_CW + j];
                ssl_pair(v, S[q][0], S[q][1]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int ci = 2 * rp + i, gy = y0 - SSL_R + ci, gx = x0 - SSL_R + j;
                const bool valid = gy >= SSL_R && gy < a.H - SSL_R && gx >= SSL_R && gx < a.W - SSL_R;
                const bool mine = ci >= SSL_R && ci < SSL_R + SSL_TH && j >= SSL_R && j < SSL_R + SSL_TW;
                const double inv = 1.0 / 49.0, cov = 49.0 / 48.0, c1 = 1e-4, c2 = 9e-4;
                const double ux = S[0][i] * inv, uy = S[1][i] * inv;
                const double vx = cov * (S[2][i] * inv - ux * ux), vy = cov * (S[3][i] * inv - uy * uy), vxy = cov * (S[4][i] * inv - ux * uy);
                const double A1 = 2.0 * ux * uy + c1, A2 = 2.0 * vxy + c2, B1 = ux * ux + uy * uy + c1, B2 = vx + vy + c2;
                const double den = B1 * B2, s = (A1 * A2) / den;
                if (valid && mine) ss += s;
                if (a.g != nullptr) {
                    const double rden = 1.0 / den;
                    const double bw = -2.0 * cov * s * (B1 * rden), cw = 2.0 * cov * A1 * rden;
                    const double dw = 2.0 * uy * A2 * rden - 2.0 * ux * s * (B2 * rden);
                    const double aw = (dw - ux * bw) - uy * cw;
                    double* o = mp + ci * SSL_CW + j;
                    o[0] = valid ? aw : 0.0;
                    o[SSL_CH * SSL_CW] = valid ? bw : 0.0;
                    o[2 * SSL_CH * SSL_CW] = valid ? cw : 0.0;
                }
            }
        }
        if (a.g == nullptr) continue;        // the value alone (the same for every thread): the next stage is read by nobody now, and the
                                             // next row sums are written behind the next band's first barrier, after step 2's readers
        __syncthreads();                   // the maps are complete; nobody reads the first row sums any more

        // 3. row sums of the maps: centre row r, the pixels of tile columns col and col + 1
        for (int e = t; e < SSL_CH * (SSL_TW / 2); e += SSL_NT) {
            const int r = e / (SSL_TW / 2), col = (e - r * (SSL_TW / 2)) * 2;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double* m = mp + (q * SSL_CH + r) * SSL_CW + col;
                double v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = m[k];
                double* o = hs + (q * SSL_CH + r) * SSL_TW + col;
                ssl_pair(v, o[0], o[1]);
            }
        }
        __syncthreads();                     // the second row sums are complete; nobody reads the maps any more: the next stage may overwrite them

        // 4. the gradient of the thread's two pixels
        double G[3][2];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = hs[(q * SSL_CH + tg * SSL_RPT + k) * SSL_TW + tx];
            ssl_pair(v, G[q][0], G[q][1]);
        }
        float* pg = a.g + ((long)b * a.C + c) * plane;
#pragma unroll
        for (int j = 0; j < SSL_RPT; ++j) {
            if (own[j] < 0) continue;
            const double xv = clamp01(yo[j]), cv = cp[j];
            const double sum = (G[0][j] + xv * G[1][j]) + cv * G[2][j];
            const float g = (yo[j] >= 0.f && yo[j] <= 1.f) ? (float)(a.scale * sum) : 0.f;
            pg[own[j]] = a.accumulate ? pg[own[j]] + g : g;
        }
    }
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    if (t == 0) a.ws[blockIdx.x] = sum4_ordered(red, 1);
}

struct SsimLossFinishDev {
    const double* ws; const float* base; float* out;
    long nblk;
    double count, w;            // B C Nw, the weight
};

__global__ __launch_bounds__(SSL_NT) void ssim_loss_finish_kernel(SsimLossFinishDev a) {
    __shared__ double red[SSL_NT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = wave_id_uniform();
    double s = 0.0;
    for (long i = t; i < a.nblk; i += SSL_NT) s += a.ws[i];
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (t != 0) return;
    const double ssim = sum4_ordered(red, 1) / a.count;
    const double base = a.base != nullptr ? (double)a.base[0] : 0.0;
    a.out[0] = (float)(base + a.w * (1.0 - ssim));
    a.out[1] = (float)ssim;
}

static long ssim_loss_blocks(int B, int C, int H, int W) {              // 0: sizes refused
    if (B < 1 || C < 1 || H < 2 * SSL_R + 1 || W < 2 * SSL_R + 1 || (long)H * W >= (1L << 31)) return 0;
    const long tiles = (long)((H + SSL_TH - 1) / SSL_TH) * ((W + SSL_TW - 1) / SSL_TW);
    return tiles * B < (1L << 31) ? tiles * B : 0;
}

}  // namespace mphsir

extern "C" int64_t mphsir_ssim_loss_workspace_bytes(int32_t B, int32_t C, int32_t H, int32_t W) {
    const long n = mphsir::ssim_loss_blocks(B, C, H, W);
    return n ? (int64_t)8 * n : MPHSIR_EINVAL;
}

extern "C" int mphsir_ssim_loss(const mphsir_ssim_loss_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "ssim_loss");
    MPHSIR_REQUIRE(a->y && a->clean && a->out && a->workspace, "ssim_loss: null pointer");
    MPHSIR_REQUIRE(a->H >= 2 * SSL_R + 1 && a->W >= 2 * SSL_R + 1, "ssim_loss: a band of %d x %d holds no 7 x 7 window", a->H, a->W);
    const long nblk = ssim_loss_blocks(a->B, a->C, a->H, a->W);
    MPHSIR_REQUIRE(nblk > 0, "ssim_loss: bad sizes (B %d, C %d, H %d, W %d: B, C >= 1, H * W < 2^31, at most 2^31 - 1 workgroups of 16 x 32 pixels)",
                   a->B, a->C, a->H, a->W);
    MPHSIR_REQUIRE(a->w_ssim > 0.f && a->w_ssim <= 3.4e38f, "ssim_loss: the weight must be finite and > 0 (w_ssim %g)", (double)a->w_ssim);
    MPHSIR_REQUIRE(a->accumulate == 0 || (a->accumulate == 1 && a->grad != nullptr),
                   "ssim_loss: accumulate must be 0 or 1, and 1 needs a grad to add to (accumulate %d)", a->accumulate);
    MPHSIR_REQUIRE(a->workspace_bytes >= 8 * nblk && (reinterpret_cast<uintptr_t>(a->workspace) & 7) == 0,
                   "ssim_loss: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)a->workspace_bytes, (long long)(8 * nblk));
    const int tiles_x = (a->W + SSL_TW - 1) / SSL_TW;
    const double count = (double)a->B * (double)a->C * (double)(a->H - 2 * SSL_R) * (double)(a->W - 2 * SSL_R);
    SsimLossDev d{a->y, a->clean, a->grad, static_cast<double*>(a->workspace), a->C, a->H, a->W, tiles_x, (int)(nblk / a->B), a->accumulate,
                  -(double)a->w_ssim / (49.0 * count)};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    MPHSIR_LAUNCH(MPHSIR_K_SPECTRAL_LOSS, ssim_loss_kernel, dim3((unsigned)nblk), dim3(SSL_NT), 0, s, d);
    SsimLossFinishDev f{static_cast<const double*>(a->workspace), a->base_loss, a->out, nblk, count, (double)a->w_ssim};
    MPHSIR_LAUNCH(MPHSIR_K_SPECTRAL_LOSS_FINISH, ssim_loss_finish_kernel, dim3(1), dim3(SSL_NT), 0, s, f);
    return MPHSIR_OK;
}
