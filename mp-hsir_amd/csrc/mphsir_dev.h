// Device-side building blocks shared by every kernel of libmphsir (gfx950 / CDNA4 only).
//
//  * element types: float (exact-f32 parity path, v_mfma_f32_16x16x4_f32) and __bf16 (throughput
//    path, v_mfma_f32_16x16x32_bf16); every kernel is a template over T and accumulates in fp32.
//  * one MFMA "fragment" is 16 bytes per lane for both types: lane l holds elements
//    k0 + EPL*(l>>4) .. +EPL-1 of row (l&15) of a K-contiguous operand.  For bf16 that is the
//    native A/B map of the 16x16x32 instruction; for f32 the 4 elements feed 4 chained 16x16x4
//    instructions (the k order inside a 16-wide chunk is permuted identically for A and B, which
//    a dot product does not care about).
//  * C/D map (both types): lane l holds D[(l>>4)*4 + r][l&15], r = 0..3.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mphsir {

typedef __bf16 bf16_t;
typedef _Float16 f16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;

constexpr int WAVE = 64;

// Row padding of every K-contiguous LDS tile read through load_frag (ds_read_b128, lane l -> row l&15, 16-byte column
// l>>4).  ds_read_b128 is serviced in the lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ... (MI355X_MICROARCH.md
// §LDS): a group takes rows {0-3,12-15} of one 16-byte column and rows 4-11 of the next, so it is conflict free
// exactly when the row pitch is 32 (mod 64) bytes -- all tile widths here are multiples of 64 bytes, hence 32 bytes
// of padding (16 bytes, the usual choice, leaves a 2-way conflict in every group).
constexpr int LDS_PAD_BYTES = 32;

template <class T> struct ElemTraits;
template <> struct ElemTraits<float> {
    typedef f32x4 frag_t;     // 4 f32 per lane
    typedef f32x4 vec4_t;     // 4 consecutive elements
    static constexpr int EPL = 4;        // elements per lane per fragment
    static constexpr int KCHUNK = 16;    // K covered by one fragment pair
    static constexpr int DTYPE = 0;
};
template <> struct ElemTraits<bf16_t> {
    typedef bf16x8 frag_t;
    typedef bf16x4 vec4_t;
    static constexpr int EPL = 8;
    static constexpr int KCHUNK = 32;
    static constexpr int DTYPE = 1;
};

template <> struct ElemTraits<f16_t> {          // fp16 storage (the reference's 16-mixed precision, train.py:118): same tile
    typedef f16x8 frag_t;                        // shapes as bf16, v_mfma_f32_16x16x32_f16, fp32 accumulation
    typedef f16x4 vec4_t;
    static constexpr int EPL = 8;
    static constexpr int KCHUNK = 32;
    static constexpr int DTYPE = 2;
};

template <class T> __device__ __forceinline__ constexpr int round_up_k(int k) {
    return (k + ElemTraits<T>::KCHUNK - 1) / ElemTraits<T>::KCHUNK * ElemTraits<T>::KCHUNK;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & (WAVE - 1); }
__device__ __forceinline__ int wave_id() { return threadIdx.x >> 6; }
// The wave index as a SCALAR.  threadIdx-derived values live in VGPRs, so the compiler cannot know that `wave_id() < n` is
// the same for all 64 lanes: every such `if` becomes s_and_saveexec + s_cbranch_execz around the statements it guards (seen
// around every MFMA of a wave-uniform tile test).  readfirstlane moves the value to an SGPR: plain scalar branches.
__device__ __forceinline__ int wave_id_uniform() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// 16-byte fragment of a K-contiguous row-major operand (LDS or global): row0 + (lane&15), k0 + EPL*(lane>>4).
template <class T>
__device__ __forceinline__ typename ElemTraits<T>::frag_t load_frag(const T* base, int ld, int row0, int k0) {
    const int l = lane_id();
    const T* p = base + (size_t)(row0 + (l & 15)) * ld + k0 + ElemTraits<T>::EPL * (l >> 4);
    return *reinterpret_cast<const typename ElemTraits<T>::frag_t*>(p);
}

// acc[16x16] += A-frag (rows of the first operand) x B-frag (rows of the second operand), over KCHUNK.
__device__ __forceinline__ void mma(f32x4& acc, bf16x8 a, bf16x8 b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma(f32x4& acc, f16x8 a, f16x8 b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma(f32x4& acc, f32x4 a, f32x4 b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], acc, 0, 0, 0);
}

// Hardware-transposed LDS read (gfx950 ds_read_b64_tr_b16): per group of 16 lanes, lane 4q+p passes the address of
// row q, columns 4p..4p+3 of a 4x16 block of bf16; lane i gets column i of the 4 rows.  Two of them (rows k..k+3 and
// k+4..k+7) make the 16-byte fragment of a K-STRIDED (token-major) operand without a transposing store.
// EXEC must be all ones; every lane's address must be 8-byte aligned.
__device__ __forceinline__ bf16x4 lds_read_tr16(const bf16_t* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(p));
}
__device__ __forceinline__ f16x4 lds_read_tr16(const f16_t* p) {
    typedef __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16 fp16x4_b;       // the builtin's own vector type
    const fp16x4_b r = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_b*)(p));
    return __builtin_bit_cast(f16x4, r);
}

// Fragment of a K-STRIDED operand held row-major as [k][col] in LDS (pitch ld elements): row (l&15) of the fragment is
// column col0 + (l&15), its K elements are rows k0 + EPL*(l>>4) .. of the tile -- the same map load_frag yields for the
// transposed tile, without a transposed copy.  bf16: two hardware-transposed reads (rows +0..3 / +4..7; ld % 4 == 0,
// col0 % 4 == 0); f32: four strided 4-byte reads.
template <class T> __device__ __forceinline__ typename ElemTraits<T>::frag_t load_frag_tr(const T* base, int ld, int col0, int k0);
template <> __device__ __forceinline__ bf16x8 load_frag_tr<bf16_t>(const bf16_t* base, int ld, int col0, int k0) {
    const int l = lane_id(), g = l >> 4, q = (l & 15) >> 2, p = l & 3;
    const bf16_t* a = base + (size_t)(k0 + 8 * g + q) * ld + col0 + 4 * p;
    const bf16x4 lo = lds_read_tr16(a), hi = lds_read_tr16(a + 4 * ld);
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
template <> __device__ __forceinline__ f16x8 load_frag_tr<f16_t>(const f16_t* base, int ld, int col0, int k0) {
    const int l = lane_id(), g = l >> 4, q = (l & 15) >> 2, p = l & 3;
    const f16_t* a = base + (size_t)(k0 + 8 * g + q) * ld + col0 + 4 * p;
    const f16x4 lo = lds_read_tr16(a), hi = lds_read_tr16(a + 4 * ld);
    return f16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
template <> __device__ __forceinline__ f32x4 load_frag_tr<float>(const float* base, int ld, int col0, int k0) {
    const int l = lane_id();
    const float* a = base + (size_t)(k0 + 4 * (l >> 4)) * ld + col0 + (l & 15);
    return f32x4{a[0], a[ld], a[2 * ld], a[3 * ld]};
}

template <class T> __device__ __forceinline__ T from_f32(float x);
template <> __device__ __forceinline__ float from_f32<float>(float x) { return x; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float x) { return (bf16_t)x; }
template <> __device__ __forceinline__ f16_t from_f32<f16_t>(float x) { return (f16_t)x; }
template <class T> __device__ __forceinline__ float to_f32(T x) { return (float)x; }

// store 4 consecutive elements (from an accumulator column) -- 8 B (bf16) / 16 B (f32) aligned.
template <class T> __device__ __forceinline__ void store4(T* p, f32x4 v);
template <> __device__ __forceinline__ void store4<float>(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
template <> __device__ __forceinline__ void store4<bf16_t>(bf16_t* p, f32x4 v) {
    bf16x4 o;
    o[0] = (bf16_t)v[0]; o[1] = (bf16_t)v[1]; o[2] = (bf16_t)v[2]; o[3] = (bf16_t)v[3];
    *reinterpret_cast<bf16x4*>(p) = o;
}

template <> __device__ __forceinline__ void store4<f16_t>(f16_t* p, f32x4 v) {
    f16x4 o;
    o[0] = (f16_t)v[0]; o[1] = (f16_t)v[1]; o[2] = (f16_t)v[2]; o[3] = (f16_t)v[3];
    *reinterpret_cast<f16x4*>(p) = o;
}

// 4 consecutive elements -> fp32 (the counterpart of store4)
template <class T> __device__ __forceinline__ f32x4 load4(const T* p);
template <> __device__ __forceinline__ f32x4 load4<float>(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
template <> __device__ __forceinline__ f32x4 load4<bf16_t>(const bf16_t* p) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

template <> __device__ __forceinline__ f32x4 load4<f16_t>(const f16_t* p) {
    const f16x4 v = *reinterpret_cast<const f16x4*>(p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}

// 16-byte vector of T (8 bf16 / 8 f16 / 4 f32) <-> fp32 registers, for coalesced global/LDS traffic.
template <class T> struct Vec16;
template <> struct Vec16<float> {
    static constexpr int N = 4;
    f32x4 v;
    __device__ __forceinline__ float get(int i) const { return v[i]; }
    __device__ __forceinline__ void set(int i, float x) { v[i] = x; }
};
template <> struct Vec16<bf16_t> {
    static constexpr int N = 8;
    bf16x8 v;
    __device__ __forceinline__ float get(int i) const { return (float)v[i]; }
    __device__ __forceinline__ void set(int i, float x) { v[i] = (bf16_t)x; }
};
template <> struct Vec16<f16_t> {
    static constexpr int N = 8;
    f16x8 v;
    __device__ __forceinline__ float get(int i) const { return (float)v[i]; }
    __device__ __forceinline__ void set(int i, float x) { v[i] = (f16_t)x; }
};
// gather element e of four 16-byte vectors into 4 consecutive elements at p (a 4-row transpose step) without a
// float round trip: pure register shuffles
__device__ __forceinline__ void store_quad(float* p, const Vec16<float>& a, const Vec16<float>& b, const Vec16<float>& c,
                                           const Vec16<float>& d, int e) {
    *reinterpret_cast<f32x4*>(p) = f32x4{a.v[e], b.v[e], c.v[e], d.v[e]};
}
__device__ __forceinline__ void store_quad(bf16_t* p, const Vec16<bf16_t>& a, const Vec16<bf16_t>& b, const Vec16<bf16_t>& c,
                                           const Vec16<bf16_t>& d, int e) {
    *reinterpret_cast<bf16x4*>(p) = bf16x4{a.v[e], b.v[e], c.v[e], d.v[e]};
}

__device__ __forceinline__ void store_quad(f16_t* p, const Vec16<f16_t>& a, const Vec16<f16_t>& b, const Vec16<f16_t>& c,
                                           const Vec16<f16_t>& d, int e) {
    *reinterpret_cast<f16x4*>(p) = f16x4{a.v[e], b.v[e], c.v[e], d.v[e]};
}

template <class T> __device__ __forceinline__ Vec16<T> load16(const T* p) {
    Vec16<T> r;
    r.v = *reinterpret_cast<const decltype(r.v)*>(p);
    return r;
}
template <class T> __device__ __forceinline__ void store16(T* p, const Vec16<T>& x) {
    *reinterpret_cast<decltype(x.v)*>(p) = x.v;
}

// Hand-off through LDS between the lanes of ONE wave (wave-private staging buffers): the wave runs in lockstep and
// its DS operations complete in order, so no workgroup barrier is needed -- only a compiler-level ordering point.
__device__ __forceinline__ void wave_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LDS-DMA: lane l copies 16 bytes from (scalar base pointer) + (ITS unsigned byte offset) to (wave-uniform LDS address) + 16 l -- no destination
// registers, completion counted by vmcnt.  Written as inline assembly on purpose: hipcc models the builtin form
// (__builtin_amdgcn_global_load_lds) as a pending LDS write and then drains vmcnt(0) in front of every ds_read_b64_tr_b16 and
// every fence, which turns a ring of rows in flight into one synchronous load per step (seen in the ISA of spectral_rows.hip).
// As assembly the transfer is invisible to that bookkeeping; the code that issues it retires it with a counted
// s_waitcnt vmcnt(N) before the barrier that publishes the row.  (MPHSIR_LDS_DMA16 is the one customisation point of this
// header: the CPU emulation of the test suite supplies a memcpy.)
// M0 (the LDS destination base) is compiler-reserved and not preserved around a statement: it is written in the SAME statement
// that reads it, and saved / restored there (cdna_hip_programming.md, "LDS-DMA recipe").
// MPHSIR_LDS_DMA16P is the same transfer with a full 64-bit source POINTER per lane (a lane may point anywhere, e.g. at a page of
// zeros for rows outside the matrix).
#ifndef MPHSIR_LDS_DMA16
#define MPHSIR_LDS_DMA16(gbase, byte_off, lds_wave_base)                                                                \
    do {                                                                                                                \
        unsigned keep_m0_;                                                                                              \
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"  \
                     : "=&s"(keep_m0_) : "v"(byte_off), "s"(gbase), "s"((unsigned)(unsigned long long)(lds_wave_base)) : "memory"); \
    } while (0)
#define MPHSIR_LDS_DMA16P(gptr, lds_wave_base)                                                                          \
    do {                                                                                                                \
        unsigned keep_m0_;                                                                                              \
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"  \
                     : "=&s"(keep_m0_) : "v"(gptr), "s"((unsigned)(unsigned long long)(lds_wave_base)) : "memory");     \
    } while (0)
#endif

// Workgroup barrier that orders LDS traffic only.  __syncthreads() -- and even a fence that names only the local address space --
// makes hipcc drain the vector-memory counter (an LDS-DMA in flight is a pending LDS write to it: s_waitcnt vmcnt(0) lgkmcnt(0)),
// which would serialise a DMA ring and the global stores with every step.  So: this wave's LDS operations are retired by
// hand (lgkmcnt(0): DS operations complete in order), the compiler is told not to move memory operations across the point,
// and the rows that must have landed are retired by a counted vmcnt wait in front of the call.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0); vmcnt and expcnt left at their maxima
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);           // nothing of the next step is scheduled into this one (register pressure)
}
// s_waitcnt vmcnt(N) alone (gfx9 encoding: vmcnt = bits 3:0 and 15:14, expcnt 6:4 and lgkmcnt 11:8 left at their maxima)
template <int N> __device__ __forceinline__ void wait_vmcnt() { __builtin_amdgcn_s_waitcnt(0x0f70 | (N & 15) | ((N >> 4) << 14)); }

// Workgroups are dealt round-robin over the 8 XCDs (blockIdx b runs on XCD b % 8, each XCD has its own L2).  For
// streaming kernels whose neighbouring workgroups share input rows (3x3 stencils) this maps XCD x to one contiguous
// eighth of the logical block range, so the shared rows are fetched from HBM once and re-read from that XCD's L2
// (measured with FETCH_SIZE: the row-major order over-fetched 1.4-1.9x).  Launch with gridDim.x a multiple of 8.
__device__ __forceinline__ long xcd_contiguous_block() {
    return (long)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
}

// exact (erf) GELU, the reference's nn.GELU()/F.gelu default.
__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// Transcendental policy per compute dtype.  The fp32 (parity) path evaluates erf / exp with the library routines; the
// 16-bit (throughput) paths, whose results are rounded to 8 / 11 mantissa bits anyway, use the hardware exp2 for the softmaxes and
// polynomials for GELU and its derivative (below): the kernels that evaluate them are bound by VALU issue.
template <class T> struct Math;
template <> struct Math<float> {
    static __device__ __forceinline__ float exp(float x) { return expf(x); }
    static __device__ __forceinline__ float gelu(float x) { return gelu_erf(x); }
    static __device__ __forceinline__ void gelu_pair(float x, float& g, float& dg) {      // GELU(x), GELU'(x)
        const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
        g = x * cdf;
        dg = cdf + x * 0.39894228040143267794f * expf(-0.5f * x * x);
    }
};
template <> struct Math<bf16_t> {
    static __device__ __forceinline__ float exp(float x) { return __expf(x); }
    // GELU(x) and GELU'(x) = Phi(x) + x phi(x) for the backward kernels, both as polynomials in xc = clamp(x, -4, 4) like the forward
    // form below (Phi: the same coefficients; GELU' - 1/2: odd, degree 17; the polynomial's |error| <= 7.0e-5 inside the clamp -- a ripple of
    // 5.52e-5 up to |x| = 2.7 that grows to 6.2e-5 at 3.77 and 6.95e-5 at |x| = 4; this comment said 5.5e-5 until tests/test_devmath_*.py
    // measured it -- and <= 5.8e-4 in the tails beyond +-4, where the exact value runs from -5e-4 to 0 and from 1 + 5e-4 to 1.  The fp32 Horner
    // evaluation adds rounding on top: the terms of Q reach 68 at u = 16 against a sum of 0.13, up to 1.1e-5 seen, 3.0e-5 by the running error
    // bound of tests/devmath_ref.py) -- no rcp / exp, every fma packs two elements.  (Until round 4: erf by
    // Abramowitz-Stegun 7.1.26 with the hardware exp2 / rcp, ~17 VALU slots + two quarter-rate ones per element.)
    static __device__ __forceinline__ void gelu_pair(float x, float& g, float& dg) {
        const float xc = __builtin_amdgcn_fmed3f(x, -4.0f, 4.0f), u = xc * xc;
        float p = -1.580785614e-09f, q = 9.796149447e-10f;
        q = fmaf(q, u, -8.218865588e-08f);
        p = fmaf(p, u, 1.217110679e-07f);
        q = fmaf(q, u, 3.028365654e-06f);
        p = fmaf(p, u, -4.100865681e-06f);
        q = fmaf(q, u, -6.495783600e-05f);
        p = fmaf(p, u, 8.066738519e-05f);
        q = fmaf(q, u, 9.073287947e-04f);
        p = fmaf(p, u, -1.048204373e-03f);
        q = fmaf(q, u, -8.716330864e-03f);
        p = fmaf(p, u, 9.664873593e-03f);
        q = fmaf(q, u, 5.845612660e-02f);
        p = fmaf(p, u, -6.617537886e-02f);
        q = fmaf(q, u, -2.648265660e-01f);
        p = fmaf(p, u, 3.988475204e-01f);
        q = fmaf(q, u, 7.976095676e-01f);
        g = fmaxf(x, -4.0f) * fmaf(xc, p, 0.5f);
        dg = fmaf(xc, q, 0.5f);
    }
    // FORWARD GELU of the 16-bit paths without transcendentals.  By the counters the gated-MLP forward is bound by VALU issue (per
    // wave and 32-wide hidden chunk ~150 VALU slots against 24 MFMAs, a third of them the quarter-rate rcp / exp of the form above,
    // 88 % of a SIMD's issue cycles taken).  Phi(x) = 1/2 + xc P(xc^2), xc = clamp(x, -4, 4), P an even polynomial of degree 14
    // (minimax fit of the odd part of Phi on [0, 4] in x/4; the power-of-two scale is folded into the coefficients exactly):
    // the polynomial's |Phi - exact| <= 5.5e-5 everywhere (5.45e-5, reached beyond the clamp where Phi stays at its value at 4), i.e.
    // |GELU - exact| <= 5.5e-5 |x| for x > -4 and <= 2.2e-4 below -- under the rounding step of the 16-bit value it is stored as.  The fp32
    // evaluation adds up to 6e-7 (2.4e-6 by the running error bound): 5.51e-5 and 2.203e-4 are its measured maxima, which this comment
    // used to quote, rounded, as the bounds.  tests/test_devmath_*.py assert all of this on the device; coefficients: tests/devmath_ref.py.
    // Every operation packs two elements per instruction (v_pk_fma_f32) except the clamp and the max.
    static __device__ __forceinline__ float gelu(float x) {
        const float xc = __builtin_amdgcn_fmed3f(x, -4.0f, 4.0f), u = xc * xc;
        float p = -1.580785614e-09f;
        p = fmaf(p, u, 1.217110679e-07f);
        p = fmaf(p, u, -4.100865681e-06f);
        p = fmaf(p, u, 8.066738519e-05f);
        p = fmaf(p, u, -1.048204373e-03f);
        p = fmaf(p, u, 9.664873593e-03f);
        p = fmaf(p, u, -6.617537886e-02f);
        p = fmaf(p, u, 3.988475204e-01f);
        return fmaxf(x, -4.0f) * fmaf(xc, p, 0.5f);
    }
};
template <> struct Math<f16_t> : Math<bf16_t> {};      // 16-bit storage either way: the hardware exp / rcp policy

// wave-wide reductions by xor shuffles over the lanes selected by `mask_bits` (e.g. 1|2 = 4 lanes).
__device__ __forceinline__ float wave_sum(float v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
// float64: the sum over the wave in a fixed tree (m = 32 ... 1); every lane ends with the total
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

}  // namespace mphsir
