// flat_adamw: one AdamW step over the flat fp32 parameter arena (all trainable tensors of the model
// laid out back to back), with the data-parallel gradient mean (1/world) folded in.
//
// Replaces torch.optim.AdamW(self.parameters(), lr) of the reference (train.py:69; defaults
// betas (0.9,0.999), eps 1e-8, weight_decay 1e-2, decoupled decay) and the 1/world_size scaling DDP
// applies after its all-reduce (train.py:118, strategy="auto").  Pure HBM streaming: 16 B per lane,
// grid-stride, 4 reads + 3 writes of 4 B per element.
//
// Further down, off unless the caller asks (engine.DataParallelEngine(grad_clip=, ema_decay=)): the global gradient norm in float64
// (grad_sqnorm_kernel + grad_norm_finish_kernel) and flat_adamw_ex_kernel, the same AdamW pass with the clip factor on the gradient and
// an EMA arena updated from the parameter it has just formed (5 reads + 4 writes then).
#include "mphsir_host.h"
#include "mphsir_planar.h"

namespace mphsir {

struct AdamDev {
    float* p; const float* g; float* m; float* v;
    long n;
    float lr, beta1, beta2, eps, wd, grad_scale, bc1, bc2_sqrt;
    const float* hyper;     // optional device [lr, bias_correction1, sqrt(bias_correction2)]: graph-replay friendly
    const float* scaler;    // optional device loss-scaler state (see mphsir_scaler_update): gradients are divided by scaler[0],
                            // the whole update is skipped when scaler[2] != 0, and the Adam step count is scaler[3] + 1
};

__global__ __launch_bounds__(256) void flat_adamw_kernel(AdamDev a) {
    if (a.hyper) { a.lr = a.hyper[0]; a.bc1 = a.hyper[1]; a.bc2_sqrt = a.hyper[2]; }
    if (a.scaler) {
        if (a.scaler[2] != 0.f) return;                       // a non-finite gradient somewhere: skip the step (GradScaler.step)
        const float t = a.scaler[3] + 1.0f;                   // skipped steps do not advance Adam's step count
        a.bc1 = 1.0f - powf(a.beta1, t);
        a.bc2_sqrt = sqrtf(1.0f - powf(a.beta2, t));
        a.grad_scale /= a.scaler[0];
    }
    const long nvec = a.n / 4;
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
        f32x4 p = reinterpret_cast<f32x4*>(a.p)[i];
        const f32x4 g = reinterpret_cast<const f32x4*>(a.g)[i];
        f32x4 m = reinterpret_cast<f32x4*>(a.m)[i];
        f32x4 v = reinterpret_cast<f32x4*>(a.v)[i];
        for (int e = 0; e < 4; ++e) {
            const float ge = g[e] * a.grad_scale;
            p[e] *= 1.0f - a.lr * a.wd;
            m[e] = a.beta1 * m[e] + (1.0f - a.beta1) * ge;
            v[e] = a.beta2 * v[e] + (1.0f - a.beta2) * ge * ge;
            const float denom = sqrtf(v[e]) / a.bc2_sqrt + a.eps;
            p[e] -= (a.lr / a.bc1) * (m[e] / denom);
        }
        reinterpret_cast<f32x4*>(a.p)[i] = p;
        reinterpret_cast<f32x4*>(a.m)[i] = m;
        reinterpret_cast<f32x4*>(a.v)[i] = v;
    }
}

// ---- dynamic loss scaling (the reference trains precision="16-mixed", train.py:118 = torch GradScaler) --------------------
// scaler state, device fp32[4]: [0] loss scale, [1] growth tracker (good steps in a row), [2] found-inf flag of the current
// step, [3] optimizer steps actually taken.
__global__ __launch_bounds__(256) void grad_check_kernel(const float* __restrict__ g, long n, float* scaler) {
    const long nvec = n / 4, stride = (long)gridDim.x * 256;
    bool bad = false;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
        const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
        // |x| <= FLT_MAX is false for inf and for NaN
        bad = bad || !(fabsf(v[0]) <= 3.402823466e38f) || !(fabsf(v[1]) <= 3.402823466e38f) || !(fabsf(v[2]) <= 3.402823466e38f) ||
              !(fabsf(v[3]) <= 3.402823466e38f);
    }
    if (bad) scaler[2] = 1.0f;          // every writer stores the same value: no ordering needed
}

__global__ void scaler_update_kernel(float* scaler, float growth, float backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (scaler[2] != 0.f) {             // GradScaler.update(): overflow -> back off, restart the streak
        scaler[0] *= backoff;
        scaler[1] = 0.f;
    } else {
        scaler[3] += 1.0f;
        scaler[1] += 1.0f;
        if (scaler[1] >= (float)interval) { scaler[0] *= growth; scaler[1] = 0.f; }
    }
    scaler[2] = 0.f;
}

// ---- global-norm clipping and EMA weights (include/mphsir.h: mphsir_grad_norm, mphsir_flat_adamw_ex) ------------------------------------
// grad_sqnorm_kernel       every thread adds the squares of its 16-byte vectors in float64 (grid-stride, the same geometry as the AdamW
//                          launch), the block's 256 sums are combined by a fixed shuffle tree and a fixed sum of the four wave results;
//                          one float64 partial per block goes to the workspace.
// grad_norm_finish_kernel  one workgroup: thread t adds partials t, t + 256, ... in ascending order (at most 8 of them), the same fixed
//                          tree combines the 256 sums, thread 0 writes norm, coef and the skip flag.
// No atomics, no order that depends on scheduling.  Bounds: vector i < n / 4 is checked in the loop; block b < nblk writes partial b and
// the host verified that the workspace holds nblk doubles; the finish reads partials i < nblk only.
constexpr int GN_MAX_BLOCKS = 256 * 8;

// the block's total in thread 0 (every thread of the block must call)
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return sum4_ordered(red, 1);
}

__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float* __restrict__ g, long n, double* __restrict__ part) {
    __shared__ double red[4];
    const long nvec = n / 4, stride = (long)gridDim.x * 256;
    double s = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
        const f32x4 v = reinterpret_cast<const f32x4*>(g)[i];
        const double a = v[0], b = v[1], c = v[2], d = v[3];
        s += (a * a + b * b) + (c * c + d * d);
    }
    const double tot = block_sum_f64(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

struct GradNormFinishDev {
    const double* part; int nblk;
    float grad_scale, max_norm;
    const float* scaler; float* stats;
};

__global__ __launch_bounds__(256) void grad_norm_finish_kernel(GradNormFinishDev a) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < a.nblk; i += 256) s += a.part[i];
    const double S = block_sum_f64(s, red);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(S) * (double)a.grad_scale / (a.scaler ? (double)a.scaler[0] : 1.0);
    a.stats[0] = (float)norm;
    if (finite(norm)) {
        const double c = (double)a.max_norm / (norm + 1e-6);
        a.stats[1] = (float)(c < 1.0 ? c : 1.0);
        a.stats[3] = 0.f;
    } else {
        a.stats[1] = 0.f;
        a.stats[2] += 1.0f;
        a.stats[3] = 1.0f;
    }
}

struct AdamExDev {
    float* p; const float* g; float* m; float* v; float* ema;
    long n;
    float lr, beta1, beta2, eps, wd, grad_scale, bc1, bc2_sqrt, ema_decay;
    const float* hyper;     // optional device [lr, bias_correction1, sqrt(bias_correction2), EMA decay (read when ema is given)]
    const float* scaler;    // optional loss-scaler state, as AdamDev
    const float* stats;     // optional [norm, coef, skipped, skip flag] of grad_norm_finish_kernel
};

// flat_adamw_kernel with the clip factor and the EMA: the statements on p / m / v are those of flat_adamw_kernel in the same order
// (ge times a coef of exactly 1 is ge), so that without stats and without ema the bits are the same.
template <bool EMA> __global__ __launch_bounds__(256) void flat_adamw_ex_kernel(AdamExDev a) {
    if (a.hyper) {
        a.lr = a.hyper[0]; a.bc1 = a.hyper[1]; a.bc2_sqrt = a.hyper[2];
        if (EMA) a.ema_decay = a.hyper[3];
    }
    if (a.scaler) {
        if (a.scaler[2] != 0.f) return;
        const float t = a.scaler[3] + 1.0f;
        a.bc1 = 1.0f - powf(a.beta1, t);
        a.bc2_sqrt = sqrtf(1.0f - powf(a.beta2, t));
        a.grad_scale /= a.scaler[0];
    }
    float coef = 1.0f;
    if (a.stats) {
        if (a.stats[3] != 0.f) return;                        // the norm was not finite: p, m, v and ema stay as they are
        coef = a.stats[1];
    }
    const float keep = 1.0f - a.ema_decay;
    const long nvec = a.n / 4;
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += stride) {
        f32x4 p = reinterpret_cast<f32x4*>(a.p)[i];
        const f32x4 g = reinterpret_cast<const f32x4*>(a.g)[i];
        f32x4 m = reinterpret_cast<f32x4*>(a.m)[i];
        f32x4 v = reinterpret_cast<f32x4*>(a.v)[i];
        f32x4 x;
        if (EMA) x = reinterpret_cast<f32x4*>(a.ema)[i];
        for (int e = 0; e < 4; ++e) {
            const float ge = (g[e] * a.grad_scale) * coef;
            p[e] *= 1.0f - a.lr * a.wd;
            m[e] = a.beta1 * m[e] + (1.0f - a.beta1) * ge;
            v[e] = a.beta2 * v[e] + (1.0f - a.beta2) * ge * ge;
            const float denom = sqrtf(v[e]) / a.bc2_sqrt + a.eps;
            p[e] -= (a.lr / a.bc1) * (m[e] / denom);
            if (EMA) x[e] += keep * (p[e] - x[e]);
        }
        reinterpret_cast<f32x4*>(a.p)[i] = p;
        reinterpret_cast<f32x4*>(a.m)[i] = m;
        reinterpret_cast<f32x4*>(a.v)[i] = v;
        if (EMA) reinterpret_cast<f32x4*>(a.ema)[i] = x;
    }
}

static long arena_blocks(int64_t n) {
    long blocks = (n / 4 + 255) / 256;
    return blocks > GN_MAX_BLOCKS ? GN_MAX_BLOCKS : blocks;
}

}  // namespace mphsir

extern "C" int64_t mphsir_grad_norm_workspace_bytes(int64_t n) {
    if (n <= 0 || n % 4 != 0) return MPHSIR_EINVAL;
    return (int64_t)8 * mphsir::arena_blocks(n);
}

extern "C" int mphsir_grad_norm(const mphsir_grad_norm_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "grad_norm");
    MPHSIR_REQUIRE(a->g && a->stats && a->workspace, "grad_norm: null pointer");
    MPHSIR_REQUIRE(a->n > 0 && a->n % 4 == 0, "grad_norm: arena length must be a positive multiple of 4 (pad the arena)");
    MPHSIR_REQUIRE(aligned16(a->g), "grad_norm: 16-byte alignment required");
    MPHSIR_REQUIRE(a->max_norm > 0.f, "grad_norm: max_norm must be positive (+inf: measure only), got %g", (double)a->max_norm);   // false for NaN
    const int64_t need = mphsir_grad_norm_workspace_bytes(a->n);
    MPHSIR_REQUIRE(a->workspace_bytes >= need && (reinterpret_cast<uintptr_t>(a->workspace) & 7) == 0,
                   "grad_norm: workspace of %lld bytes, %lld needed (8-byte aligned)", (long long)a->workspace_bytes, (long long)need);
    const long blocks = arena_blocks(a->n);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    MPHSIR_LAUNCH(MPHSIR_K_FLAT_ADAMW, grad_sqnorm_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a->g, (long)a->n, static_cast<double*>(a->workspace));
    GradNormFinishDev f{static_cast<const double*>(a->workspace), (int)blocks, a->grad_scale, a->max_norm, a->scaler, a->stats};
    MPHSIR_LAUNCH(MPHSIR_K_FLAT_ADAMW, grad_norm_finish_kernel, dim3(1), dim3(256), 0, s, f);
    return MPHSIR_OK;
}

extern "C" int mphsir_flat_adamw_ex(const mphsir_flat_adamw_ex_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "flat_adamw_ex");
    MPHSIR_REQUIRE(a->p && a->g && a->m && a->v, "flat_adamw_ex: null pointer");
    MPHSIR_REQUIRE(a->n > 0 && a->n % 4 == 0, "flat_adamw_ex: arena length must be a positive multiple of 4 (pad the arena)");
    MPHSIR_REQUIRE(aligned16(a->p) && aligned16(a->g) && aligned16(a->m) && aligned16(a->v) && aligned16(a->ema),
                   "flat_adamw_ex: 16-byte alignment required");
    MPHSIR_REQUIRE(a->step >= 1 || a->hyper || a->scaler, "flat_adamw_ex: step is 1-based");
    MPHSIR_REQUIRE(!a->ema || a->hyper || (a->ema_decay >= 0.f && a->ema_decay < 1.f), "flat_adamw_ex: ema_decay must lie in [0, 1), got %g",
                   (double)a->ema_decay);
    const float t = (float)(a->step > 0 ? a->step : 1);
    AdamExDev d{a->p, a->g, a->m, a->v, a->ema, (long)a->n, a->lr, a->beta1, a->beta2, a->eps, a->weight_decay, a->grad_scale,
                1.0f - powf(a->beta1, t), sqrtf(1.0f - powf(a->beta2, t)), a->ema_decay, a->hyper, a->scaler, a->stats};
    const long blocks = arena_blocks(a->n);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (a->ema)
        MPHSIR_LAUNCH(MPHSIR_K_FLAT_ADAMW, flat_adamw_ex_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, d);
    else
        MPHSIR_LAUNCH(MPHSIR_K_FLAT_ADAMW, flat_adamw_ex_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, d);
    return MPHSIR_OK;
}

extern "C" int mphsir_grad_check(const float* g, int64_t n, float* scaler, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_REQUIRE(g && scaler && n > 0 && n % 4 == 0 && aligned16(g), "grad_check: bad arguments");
    long blocks = (n / 4 + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    MPHSIR_LAUNCH(MPHSIR_K_FLAT_ADAMW, grad_check_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g, (long)n, scaler);
    return MPHSIR_OK;
}

extern "C" int mphsir_scaler_update(float* scaler, float growth_factor, float backoff_factor, int32_t growth_interval, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_REQUIRE(scaler && growth_factor >= 1.0f && backoff_factor > 0.f && backoff_factor <= 1.0f && growth_interval > 0, "scaler_update: bad arguments");
    MPHSIR_LAUNCH(MPHSIR_K_FLAT_ADAMW, scaler_update_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), scaler, growth_factor,
                  backoff_factor, (int)growth_interval);
    return MPHSIR_OK;
}

extern "C" int mphsir_flat_adamw_scaled(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                                        float weight_decay, float grad_scale, const float* hyper, const float* scaler, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_REQUIRE(p && g && m && v && scaler, "flat_adamw_scaled: null pointer");
    MPHSIR_REQUIRE(n > 0 && n % 4 == 0, "flat_adamw_scaled: arena length must be a positive multiple of 4 (pad the arena)");
    MPHSIR_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), "flat_adamw_scaled: 16-byte alignment required");
    AdamDev d{p, g, m, v, (long)n, lr, beta1, beta2, eps, weight_decay, grad_scale, 1.0f, 1.0f, hyper, scaler};
    long blocks = (n / 4 + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    MPHSIR_LAUNCH(MPHSIR_K_FLAT_ADAMW, flat_adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), d);
    return MPHSIR_OK;
}

extern "C" int mphsir_flat_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, int32_t step, float grad_scale, const float* hyper,
                                 void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_REQUIRE(p && g && m && v, "flat_adamw: null pointer");
    MPHSIR_REQUIRE(n > 0 && n % 4 == 0, "flat_adamw: arena length must be a positive multiple of 4 (pad the arena)");
    MPHSIR_REQUIRE(aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v), "flat_adamw: 16-byte alignment required");
    MPHSIR_REQUIRE(step >= 1 || hyper, "flat_adamw: step is 1-based");
    AdamDev d{p, g, m, v, (long)n, lr, beta1, beta2, eps, weight_decay, grad_scale,
              1.0f - powf(beta1, (float)(step > 0 ? step : 1)), sqrtf(1.0f - powf(beta2, (float)(step > 0 ? step : 1))), hyper, nullptr};
    long blocks = (n / 4 + 255) / 256;
    if (blocks > 256 * 8) blocks = 256 * 8;
    MPHSIR_LAUNCH(MPHSIR_K_FLAT_ADAMW, flat_adamw_kernel, dim3((unsigned)blocks), dim3(256), 0,
                  reinterpret_cast<hipStream_t>(stream), d);
    return MPHSIR_OK;
}
