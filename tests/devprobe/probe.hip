// TEST INFRASTRUCTURE: element-wise probes of the device math in csrc/mphsir_dev.h (Math<T>::gelu / gelu_pair / exp, the LayerNorm
// rsqrtf form, the fp32 <-> 16-bit conversions, the reciprocal), so that tests/test_devmath_{emu,gpu}.py can hold each function against an
// fp64 reference at function-level bounds: the operation-level tolerances (TOL[bf16] = 1.5e-2) cannot see them.  Built by
// tests/devprobe/build_probe.py into a library of its own (gfx950: tests/devprobe/libmphsir_probe.so; emulator: beside
// libmphsir_emu.so) and never into the product.  Grid-stride kernels, every access checked against n, plain vector loads and stores:
// no LDS, no inline assembly, no atomics.
#include "mphsir_dev.h"

namespace mphsir {

enum { PROBE_GELU = 0, PROBE_GELU_PAIR = 1, PROBE_EXP = 2, PROBE_LN_RSTD = 3, PROBE_CVT = 4, PROBE_RCP = 5, PROBE_CVT_STORE4 = 6,
       PROBE_CVT_VEC16 = 7, PROBE_GELU_ERF = 8, PROBE_COUNT = 9 };

template <class T> __device__ __forceinline__ unsigned bits_of(T x);
template <> __device__ __forceinline__ unsigned bits_of<float>(float x) { return __builtin_bit_cast(unsigned, x); }
template <> __device__ __forceinline__ unsigned bits_of<bf16_t>(bf16_t x) { return __builtin_bit_cast(unsigned short, x); }
template <> __device__ __forceinline__ unsigned bits_of<f16_t>(f16_t x) { return __builtin_bit_cast(unsigned short, x); }

// out0: the first result as fp32; out1: the second result (GELU' of gelu_pair) or, for the conversions, the bit pattern of the T value
// as an integer stored in the float's 4 bytes.  C: the LayerNorm width of PROBE_LN_RSTD (in[i] is the sum of squared deviations d2).
template <class T, int WHAT>
__global__ __launch_bounds__(256) void probe_kernel(const float* __restrict__ in, float* __restrict__ out0, float* __restrict__ out1, long n, int C) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float x = in[i];
        float r0 = 0.f, r1 = 0.f;
        if (WHAT == PROBE_GELU) {
            r0 = Math<T>::gelu(x);
        } else if (WHAT == PROBE_GELU_PAIR) {
            Math<T>::gelu_pair(x, r0, r1);
        } else if (WHAT == PROBE_EXP) {
            r0 = Math<T>::exp(x);
        } else if (WHAT == PROBE_LN_RSTD) {
            const float d2 = x;
            r0 = rsqrtf(d2 / (float)C + 1e-5f);          // exactly as the kernels spell it
        } else if (WHAT == PROBE_CVT) {
            const T t = from_f32<T>(x);
            r0 = to_f32<T>(t);
            r1 = __builtin_bit_cast(float, bits_of<T>(t));
        } else if (WHAT == PROBE_RCP) {
            r0 = 1.0f / x;
        } else if (WHAT == PROBE_CVT_STORE4) {
            alignas(16) T tmp[4];
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            const int e = (int)(i & 3);
            v[e] = x;
            store4<T>(tmp, v);
            r0 = to_f32<T>(tmp[e]);
            r1 = __builtin_bit_cast(float, bits_of<T>(tmp[e]));
        } else if (WHAT == PROBE_CVT_VEC16) {
            Vec16<T> v;
            const int e = (int)(i % Vec16<T>::N);
            for (int k = 0; k < Vec16<T>::N; ++k) v.set(k, 0.f);
            v.set(e, x);
            r0 = v.get(e);
            r1 = __builtin_bit_cast(float, bits_of<T>(from_f32<T>(r0)));      // get() widens exactly: converting back is the stored pattern
        } else if (WHAT == PROBE_GELU_ERF) {
            r0 = gelu_erf(x);
        }
        out0[i] = r0;
        if (out1) out1[i] = r1;
    }
}

template <class T>
static int probe_launch(int what, const float* in, float* out0, float* out1, long n, int C, hipStream_t s) {
    const dim3 block(256), grid((unsigned)((n + 255) / 256 < 64 ? (n + 255) / 256 : 64));
#define PROBE_CASE(W)                                                                            \
    case W: hipLaunchKernelGGL((probe_kernel<T, W>), grid, block, 0, s, in, out0, out1, n, C); break;
    switch (what) {
        PROBE_CASE(PROBE_GELU) PROBE_CASE(PROBE_GELU_PAIR) PROBE_CASE(PROBE_EXP) PROBE_CASE(PROBE_LN_RSTD) PROBE_CASE(PROBE_CVT)
        PROBE_CASE(PROBE_RCP) PROBE_CASE(PROBE_CVT_STORE4) PROBE_CASE(PROBE_CVT_VEC16) PROBE_CASE(PROBE_GELU_ERF)
        default: return -1;
    }
#undef PROBE_CASE
    return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace mphsir

// what: the PROBE_* value; policy: 0 float, 1 bf16, 2 f16 (the MPHSIR_F32 / _BF16 / _F16 numbering); in, out0, out1 (optional): n floats
// each.  Returns 0, -1 (unknown what), -2 (bad argument) or -3 (launch failed).
extern "C" int mphsir_probe(int what, int policy, const float* in, float* out0, float* out1, int64_t n, int32_t C, void* stream) {
    using namespace mphsir;
    if (!in || !out0 || n <= 0 || C <= 0) return -2;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (policy) {
        case 0: return probe_launch<float>(what, in, out0, out1, (long)n, (int)C, s);
        case 1: return probe_launch<bf16_t>(what, in, out0, out1, (long)n, (int)C, s);
        case 2: return probe_launch<f16_t>(what, in, out0, out1, (long)n, (int)C, s);
    }
    return -2;
}
