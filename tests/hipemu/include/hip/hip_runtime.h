// ================================================================================================
// hipemu -- a CPU stand-in for <hip/hip_runtime.h>.            *** TEST INFRASTRUCTURE ONLY ***
//
// Lets the *unmodified* kernel sources under mp-hsir_amd/csrc/ (and the C-ABI host code that
// launches them) be compiled for x86 with clang++ and run under pytest on a machine without a GPU,
// so index arithmetic, LDS layouts, MFMA fragment maps and wave-shuffle reductions are checked on
// every CPU test run.  It is not a product path: the product library (libmphsir.so) is built by hipcc
// for gfx950 only, and the Python package refuses to run without it.
//
// Model: one workgroup at a time; every work-item is a fiber (hand-rolled x86-64 context switch);
// __syncthreads() and the wave-collective operations (shuffles, MFMA) are rendezvous points.
// A wave is 64 consecutive work-items.  Wave collectives must be reached by all 64 lanes (as on the
// hardware: MFMA needs EXEC all ones).  Global memory is host memory.
//
// Schedules: the order in which the scheduler resumes the fibers of a workgroup (and walks the blocks of a grid) is set through
// hipemu_set_schedule(mode, seed).  A kernel that orders its LDS traffic with barriers gives the same bits under every one of them;
// a kernel that misses a barrier gives different bits under some (tests/test_emu_schedules.py, tests/hipemu/selftest.hip).
//   0  ascending thread order (the default)          3  seeded random wave order and lane order, re-drawn at every pass
//   1  descending thread order                       4  laggard: wave seed % nwaves runs only in a pass in which no other fiber moved
//   2  descending wave order, lanes ascending        5  sprinter: wave seed % nwaves runs until it is stuck before any other wave
//   | HIPEMU_SCHED_DESC_BLOCKS: the blocks of a grid in descending order.
// Static and dynamic LDS are filled with 0xCD before every block.  A scheduler pass that resumed every live fiber and saw none of
// them leave a rendezvous or finish is a deadlock (a barrier not every thread reaches): reported and aborted.
// ================================================================================================
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>
#include <sys/mman.h>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)
// static LDS objects are collected in one section of the library so that run_block can poison them (the linker provides the bounds)
// (not in the AddressSanitizer build, HIPEMU_SANITIZE=1: a global in a named section gets no red zones, and that build is there for
// the out-of-tile index; the section is then empty and nothing is poisoned)
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define HIPEMU_PLAIN_STATIC_LDS 1
#endif
#endif
#ifdef HIPEMU_PLAIN_STATIC_LDS
#define __shared__ static
#else
#define __shared__ static __attribute__((section("hipemu_lds")))
#endif
extern "C" char __start_hipemu_lds[] __attribute__((weak, visibility("hidden")));
extern "C" char __stop_hipemu_lds[] __attribute__((weak, visibility("hidden")));
#define HIPEMU_SCHED_MODE_MASK 0xff
#define HIPEMU_SCHED_DESC_BLOCKS 0x100
#define HIP_DYNAMIC_SHARED(type, var) type* var = reinterpret_cast<type*>(hipemu::dyn_lds());

struct dim3 {
    unsigned x, y, z;
    constexpr dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};
typedef int hipError_t;
typedef void* hipStream_t;
typedef void* hipEvent_t;
enum { hipSuccess = 0 };
enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize = 8 };
inline hipError_t hipGetLastError() { return hipSuccess; }
inline hipError_t hipPeekAtLastError() { return hipSuccess; }
inline const char* hipGetErrorString(hipError_t) { return "hipemu"; }
template <class K> inline hipError_t hipFuncSetAttribute(K, hipFuncAttribute, int) { return hipSuccess; }
inline hipError_t hipEventCreate(hipEvent_t* e) { *e = nullptr; return hipSuccess; }
inline hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
inline hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }
inline hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { memset(p, v, n); return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
struct hipDeviceProp_t { char gcnArchName[64]; int multiProcessorCount; };
inline hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
inline hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) {
    strcpy(p->gcnArchName, "gfx950:hipemu"); p->multiProcessorCount = 256; return hipSuccess;
}

namespace hipemu {

constexpr int kWave = 64;
constexpr size_t kStack = 512 * 1024;
constexpr int kMaxThreads = 1024;

struct Fiber {
    void* sp;
    dim3 tid;
    int flat;
    bool done;
    int wait;           // 0 running, 1 at the block barrier, 2 at a wave rendezvous
};

struct WaveState {
    int count = 0, gen = 0;
    alignas(16) unsigned char xa[kWave][64];
    alignas(16) unsigned char xb[kWave][64];
};

struct State {
    dim3 bid, bdim, gdim;
    int nthreads = 0;
    int bar_count = 0, bar_gen = 0;
    Fiber fibers[kMaxThreads];
    WaveState waves[kMaxThreads / kWave];
    Fiber* cur = nullptr;
    void* sched_sp = nullptr;
    char* stacks = nullptr;
    std::vector<unsigned char> lds;
    std::function<void()> body;
    int sched = 0;                  // mode | flags (hipemu_set_schedule)
    uint64_t sched_seed = 0, rng = 0;
    uint64_t progress = 0;          // a fiber left a rendezvous or finished
    int max_waves = 0;              // the widest workgroup launched since the last hipemu_set_schedule
};

inline State& S() { static State s; return s; }

extern "C" void hipemu_switch(void** save_sp, void* load_sp);
#ifdef HIPEMU_IMPLEMENTATION
asm(R"(
.text
.globl hipemu_switch
.type hipemu_switch,@function
hipemu_switch:
    pushq %rbp
    pushq %rbx
    pushq %r12
    pushq %r13
    pushq %r14
    pushq %r15
    movq %rsp, (%rdi)
    movq %rsi, %rsp
    popq %r15
    popq %r14
    popq %r13
    popq %r12
    popq %rbx
    popq %rbp
    ret
.size hipemu_switch,.-hipemu_switch
)");
#endif

extern "C" void hipemu_set_schedule(int mode, uint64_t seed);
extern "C" int hipemu_get_schedule(uint64_t* seed);
extern "C" int hipemu_max_waves();      // waves of the widest workgroup launched since the last hipemu_set_schedule: what modes 4 and 5 can name
#ifdef HIPEMU_IMPLEMENTATION
extern "C" void hipemu_set_schedule(int mode, uint64_t seed) {
    State& s = S();
    if ((mode & HIPEMU_SCHED_MODE_MASK) > 5 || (mode & ~(HIPEMU_SCHED_MODE_MASK | HIPEMU_SCHED_DESC_BLOCKS)) || mode < 0) {
        fprintf(stderr, "hipemu: unknown schedule 0x%x\n", mode); abort();
    }
    s.sched = mode; s.sched_seed = seed; s.rng = seed; s.max_waves = 0;
}
extern "C" int hipemu_max_waves() { return S().max_waves; }
extern "C" int hipemu_get_schedule(uint64_t* seed) { if (seed) *seed = S().sched_seed; return S().sched; }
#endif

// splitmix64: the generator of the random schedule (fixed here so that a seed names one schedule on every machine)
inline uint64_t sched_rand() {
    uint64_t z = (S().rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline void sched_shuffle(int* v, int n) {
    for (int i = n - 1; i > 0; --i) { int j = (int)(sched_rand() % (uint64_t)(i + 1)); int t = v[i]; v[i] = v[j]; v[j] = t; }
}

inline void yield() { State& s = S(); hipemu_switch(&s.cur->sp, s.sched_sp); }

inline void fiber_entry() {
    State& s = S();
    s.body();
    s.cur->done = true;
    s.progress++;
    hipemu_switch(&s.cur->sp, s.sched_sp);
    abort();
}

inline void* dyn_lds() { return S().lds.data(); }

inline void block_sync() {
    State& s = S();
    int gen = s.bar_gen;
    if (++s.bar_count == s.nthreads) { s.bar_count = 0; s.bar_gen++; }
    else { s.cur->wait = 1; while (s.bar_gen == gen) yield(); s.cur->wait = 0; }
    s.progress++;
}

inline WaveState& my_wave() { State& s = S(); return s.waves[s.cur->flat / kWave]; }
inline int lane_id() { return S().cur->flat % kWave; }

inline void wave_sync() {
    State& s = S();
    WaveState& w = my_wave();
    int first = (s.cur->flat / kWave) * kWave;
    int n = s.nthreads - first < kWave ? s.nthreads - first : kWave;
    int gen = w.gen;
    if (++w.count == n) { w.count = 0; w.gen++; }
    else { s.cur->wait = 2; while (w.gen == gen) yield(); s.cur->wait = 0; }
    s.progress++;
}

template <class T> inline T wave_xchg(T v, int src_lane) {
    static_assert(sizeof(T) <= 64, "");
    WaveState& w = my_wave();
    memcpy(w.xa[lane_id()], &v, sizeof(T));
    wave_sync();
    T r;
    memcpy(&r, w.xa[src_lane & (kWave - 1)], sizeof(T));
    wave_sync();
    return r;
}

inline void resume(int t) {
    State& s = S();
    Fiber& f = s.fibers[t];
    if (f.done) return;
    s.cur = &f;
    hipemu_switch(&s.sched_sp, f.sp);
}
inline void resume_wave(int w, const int* lanes) {
    for (int l = 0; l < kWave; ++l) resume(w * kWave + (lanes ? lanes[l] : l));
}

[[noreturn]] inline void deadlock() {
    State& s = S();
    int at_block = 0, at_wave = 0, done = 0;
    for (int t = 0; t < s.nthreads; ++t) {
        at_block += s.fibers[t].wait == 1; at_wave += s.fibers[t].wait == 2; done += s.fibers[t].done;
    }
    fprintf(stderr, "hipemu: deadlock in block (%u,%u,%u) of grid (%u,%u,%u), %d threads: %d wait at the block barrier, %d at a wave "
                    "rendezvous, %d have finished (schedule 0x%x seed %llu)\n", s.bid.x, s.bid.y, s.bid.z, s.gdim.x, s.gdim.y, s.gdim.z,
            s.nthreads, at_block, at_wave, done, s.sched, (unsigned long long)s.sched_seed);
    fflush(stderr);
    abort();
}

// one scheduler pass: every live fiber is resumed at least once, in the order of the schedule
inline void sched_pass() {
    State& s = S();
    const int n = s.nthreads, nw = n / kWave, mode = s.sched & HIPEMU_SCHED_MODE_MASK;
    const int special = (int)(s.sched_seed % (uint64_t)nw);
    switch (mode) {
    default:
        for (int t = 0; t < n; ++t) resume(t);
        break;
    case 1:
        for (int t = n - 1; t >= 0; --t) resume(t);
        break;
    case 2:
        for (int w = nw - 1; w >= 0; --w) resume_wave(w, nullptr);
        break;
    case 3: {
        int waves[kMaxThreads / kWave], lanes[kWave];
        for (int w = 0; w < nw; ++w) waves[w] = w;
        sched_shuffle(waves, nw);
        for (int i = 0; i < nw; ++i) {
            for (int l = 0; l < kWave; ++l) lanes[l] = l;
            sched_shuffle(lanes, kWave);
            resume_wave(waves[i], lanes);
        }
        break;
    }
    case 4: {
        const uint64_t p0 = s.progress;
        for (int w = 0; w < nw; ++w) if (w != special) resume_wave(w, nullptr);
        if (s.progress == p0) resume_wave(special, nullptr);
        break;
    }
    case 5: {
        uint64_t p0;
        do { p0 = s.progress; resume_wave(special, nullptr); } while (s.progress != p0);
        for (int w = 0; w < nw; ++w) if (w != special) resume_wave(w, nullptr);
        break;
    }
    }
}

inline void run_block(dim3 bid, dim3 gdim, dim3 bdim, size_t shmem) {
    State& s = S();
    if (!s.stacks) {
        s.stacks = (char*)mmap(nullptr, kStack * kMaxThreads, PROT_READ | PROT_WRITE,
                               MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (s.stacks == MAP_FAILED) { perror("hipemu mmap"); abort(); }
    }
    s.bid = bid; s.gdim = gdim; s.bdim = bdim;
    s.nthreads = (int)(bdim.x * bdim.y * bdim.z);
    if (s.nthreads > kMaxThreads || s.nthreads % kWave) { fprintf(stderr, "hipemu: bad block size %d\n", s.nthreads); abort(); }
    if (s.nthreads / kWave > s.max_waves) s.max_waves = s.nthreads / kWave;
    s.bar_count = 0; s.bar_gen = 0;
    for (auto& w : s.waves) { w.count = 0; w.gen = 0; }
    if (s.lds.size() < shmem + 64) s.lds.resize(shmem + 64);
    memset(s.lds.data(), 0xCD, s.lds.size());   // poison: reads of unwritten LDS show up as garbage
    if (+__stop_hipemu_lds > +__start_hipemu_lds)  // static LDS of every kernel of the library: a block never sees what the last one left
        memset(__start_hipemu_lds, 0xCD, (size_t)(__stop_hipemu_lds - __start_hipemu_lds));
    for (int t = 0; t < s.nthreads; ++t) {
        Fiber& f = s.fibers[t];
        f.flat = t; f.done = false; f.wait = 0;
        f.tid = dim3(t % bdim.x, (t / bdim.x) % bdim.y, t / (bdim.x * bdim.y));
        void** top = (void**)(s.stacks + kStack * (t + 1));
        *--top = nullptr;                       // keeps rsp % 16 == 8 at fiber_entry's first instruction
        *--top = (void*)&fiber_entry;           // 'ret' target
        for (int r = 0; r < 6; ++r) *--top = nullptr;
        f.sp = top;
    }
    for (;;) {
        int live = 0;
        for (int t = 0; t < s.nthreads; ++t) live += !s.fibers[t].done;
        if (!live) break;
        const uint64_t p0 = s.progress;
        sched_pass();
        if (s.progress == p0) deadlock();       // every live fiber was resumed and none left its rendezvous
    }
    s.cur = nullptr;
}

template <class K, class... A> inline void launch(K kern, dim3 grid, dim3 block, size_t shmem, A... args) {
    State& s = S();
    s.body = [=]() { kern(args...); };
    const uint64_t nblocks = (uint64_t)grid.x * grid.y * grid.z;
    const bool desc = (s.sched & HIPEMU_SCHED_DESC_BLOCKS) != 0;
    for (uint64_t i = 0; i < nblocks; ++i) {    // ascending: x fastest, then y, then z; descending: the same walk backwards
        const uint64_t b = desc ? nblocks - 1 - i : i;
        run_block(dim3((unsigned)(b % grid.x), (unsigned)(b / grid.x % grid.y), (unsigned)(b / ((uint64_t)grid.x * grid.y))), grid, block, shmem);
    }
}

}  // namespace hipemu

#define threadIdx (hipemu::S().cur->tid)
#define blockIdx (hipemu::S().bid)
#define blockDim (hipemu::S().bdim)
#define gridDim (hipemu::S().gdim)
#define hipLaunchKernelGGL(kern, grid, block, shmem, stream, ...) \
    hipemu::launch(kern, dim3(grid), dim3(block), (size_t)(shmem), ##__VA_ARGS__)

inline void __syncthreads() { hipemu::block_sync(); }
template <class T> inline T __shfl_xor(T v, int mask, int = 64) { return hipemu::wave_xchg(v, hipemu::lane_id() ^ mask); }
template <class T> inline T __shfl(T v, int src, int = 64) { return hipemu::wave_xchg(v, src); }
template <class T> inline T __shfl_down(T v, unsigned d, int = 64) {
    int l = hipemu::lane_id(); return hipemu::wave_xchg(v, l + (int)d < 64 ? l + (int)d : l);
}
inline float atomicAdd(float* p, float v) { float o = *p; *p = o + v; return o; }
inline int atomicAdd(int* p, int v) { int o = *p; *p = o + v; return o; }
inline int atomicExch(int* p, int v) { int o = *p; *p = v; return o; }
inline void __threadfence() {}
#ifndef __HIP_MEMORY_SCOPE_AGENT          // __hip_atomic_load / _store / _fetch_add themselves are clang builtins on the host too
#define __HIP_MEMORY_SCOPE_AGENT 4
#endif
inline unsigned atomicAdd(unsigned* p, unsigned v) { unsigned o = *p; *p = o + v; return o; }
inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
inline float __expf(float x) { return expf(x); }
inline float __frcp_rn(float x) { return 1.0f / x; }
inline float __fdividef(float a, float b) { return a / b; }
#define __builtin_amdgcn_rcpf(x) (1.0f / (x))
#define __builtin_amdgcn_fmed3f(x, lo, hi) fminf(fmaxf((x), (lo)), (hi))

// ---- matrix-core emulation: fragment maps per cdna_hip_programming.md §3 -----------------------
namespace hipemu {
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;

// D[row][col] += sum_k A[row][k] * B[k][col]; lane l holds A[l&15][8*(l>>4)+j], B[8*(l>>4)+j][l&15],
// D[(l>>4)*4+r][l&15].
template <class V8> inline f32x4_t mfma_16x16x32(V8 a, V8 b, f32x4_t c) {
    WaveState& w = my_wave();
    int l = lane_id();
    memcpy(w.xa[l], &a, 16);
    memcpy(w.xb[l], &b, 16);
    wave_sync();
    int col = l & 15;
    for (int r = 0; r < 4; ++r) {
        int row = (l >> 4) * 4 + r;
        float acc = c[r];
        for (int k = 0; k < 32; ++k) {
            V8 fa, fb;
            memcpy(&fa, w.xa[row + 16 * (k >> 3)], 16);
            memcpy(&fb, w.xb[col + 16 * (k >> 3)], 16);
            acc = fmaf((float)fa[k & 7], (float)fb[k & 7], acc);
        }
        c[r] = acc;
    }
    wave_sync();
    return c;
}
// f32 16x16x4: lane l holds A[l&15][l>>4], B[l>>4][l&15]; exact fmaf chain in k order.
inline f32x4_t mfma_16x16x4_f32(float a, float b, f32x4_t c) {
    WaveState& w = my_wave();
    int l = lane_id();
    memcpy(w.xa[l], &a, 4);
    memcpy(w.xb[l], &b, 4);
    wave_sync();
    int col = l & 15;
    for (int r = 0; r < 4; ++r) {
        int row = (l >> 4) * 4 + r;
        float acc = c[r];
        for (int k = 0; k < 4; ++k) {
            float fa, fb;
            memcpy(&fa, w.xa[row + 16 * k], 4);
            memcpy(&fb, w.xb[col + 16 * k], 4);
            acc = fmaf(fa, fb, acc);
        }
        c[r] = acc;
    }
    wave_sync();
    return c;
}
// ds_read_b64_tr_b16 (cdna_hip_programming.md T10): per group of 16 lanes, lane 4q+p supplies the address of row q,
// columns 4p..4p+3 of a 4x16 block of 16-bit elements; lane i receives column i, row q in element q.
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4_t;
inline bf16x4_t ds_read_tr16_b64(const void* p) {
    WaveState& w = my_wave();
    int l = lane_id();
    memcpy(w.xa[l], &p, sizeof(p));
    wave_sync();
    int g = l & ~15, i = l & 15;
    bf16x4_t r;
    for (int q = 0; q < 4; ++q) {
        const char* src;
        memcpy(&src, w.xa[g + 4 * q + (i >> 2)], sizeof(src));
        __bf16 v;
        memcpy(&v, src + 2 * (i & 3), 2);
        r[q] = v;
    }
    wave_sync();
    return r;
}
}  // namespace hipemu
// DPP row shifts (v_mov_b32_dpp row_shl:n = 0x100+n: lane i <- lane i+n; row_shr:n = 0x110+n: lane i <- lane i-n, inside the
// 16-lane row; a lane whose source falls outside its row keeps `old` (bound_ctrl = 0) or gets 0) and ds_bpermute_b32.
namespace hipemu {
inline int update_dpp(int old, int src, int ctrl, int, int, bool bound_ctrl) {
    const int l = lane_id(), row = l & ~15, i = l & 15;
    int sl = -1;
    if (ctrl >= 0x101 && ctrl <= 0x10f) sl = i + (ctrl - 0x100) < 16 ? row + i + (ctrl - 0x100) : -1;
    else if (ctrl >= 0x111 && ctrl <= 0x11f) sl = i - (ctrl - 0x110) >= 0 ? row + i - (ctrl - 0x110) : -1;
    else { fprintf(stderr, "hipemu: dpp_ctrl 0x%x not emulated\n", ctrl); abort(); }
    const int v = wave_xchg(src, sl < 0 ? l : sl);
    return sl < 0 ? (bound_ctrl ? 0 : old) : v;
}
inline int ds_bpermute(int addr, int src) { return wave_xchg(src, (addr >> 2) & (kWave - 1)); }
}  // namespace hipemu
// LDS-DMA (global_load_lds): lane l copies `size` bytes from its own source address to the wave's LDS base + l * size
// (synchronous here); the raw barrier, the counted waits and address-space qualifiers mean nothing on the CPU.
namespace hipemu {
inline void global_load_lds(const void* src, void* dst, int size) { memcpy((char*)dst + (size_t)lane_id() * size, src, size); }
}  // namespace hipemu
#define address_space(n)
#define __builtin_amdgcn_global_load_lds(src, dst, size, off, aux) hipemu::global_load_lds((const void*)(src), (void*)(dst), size)
#define MPHSIR_LDS_DMA16(gbase, byte_off, lds_wave_base) hipemu::global_load_lds((const char*)(gbase) + (byte_off), (void*)(lds_wave_base), 16)
#define MPHSIR_LDS_DMA16P(gptr, lds_wave_base) hipemu::global_load_lds((const void*)(gptr), (void*)(lds_wave_base), 16)
#define __builtin_amdgcn_s_barrier() hipemu::block_sync()
#define __builtin_amdgcn_s_waitcnt(x) ((void)0)
#define __builtin_amdgcn_sched_barrier(x) ((void)0)
#define __builtin_amdgcn_update_dpp(old, src, ctrl, rm, bm, bc) hipemu::update_dpp(old, src, ctrl, rm, bm, bc)
#define __builtin_amdgcn_ds_bpermute(addr, src) hipemu::ds_bpermute(addr, src)
#define __builtin_amdgcn_s_memtime() 0ull
#define __builtin_amdgcn_readfirstlane(x) (x)      /* wave-uniform by contract: any lane's value */
#define __builtin_amdgcn_wave_barrier() hipemu::wave_sync()
#define __builtin_amdgcn_fence(...) ((void)0)
#define __builtin_amdgcn_ds_read_tr16_b64_v4bf16(p) hipemu::ds_read_tr16_b64((const void*)(p))
namespace hipemu {
typedef __attribute__((__vector_size__(4 * sizeof(__fp16)))) __fp16 fp16x4_b;
inline fp16x4_b ds_read_tr16_b64_f16(const void* p) {         // same lane exchange, 2-byte elements moved bit-wise
    const bf16x4_t r = ds_read_tr16_b64(p);
    fp16x4_b o;
    memcpy(&o, &r, sizeof(o));
    return o;
}
}  // namespace hipemu
#define __builtin_amdgcn_ds_read_tr16_b64_v4f16(p) hipemu::ds_read_tr16_b64_f16((const void*)(p))
#define __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, x, y, z) hipemu::mfma_16x16x32<hipemu::bf16x8_t>(a, b, c)
#define __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, x, y, z) hipemu::mfma_16x16x32<hipemu::f16x8_t>(a, b, c)
#define __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, x, y, z) hipemu::mfma_16x16x4_f32(a, b, c)
