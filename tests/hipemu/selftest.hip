// TEST INFRASTRUCTURE: kernels with planted synchronisation faults, each beside a correct twin (fixed != 0), for the schedules of the
// emulator (tests/test_emu_schedules.py).  Built by build_emu.py into a small library of its own (libhipemu_selftest.so) and never
// into the product or the emulated product library; CPU only.  Every faulty form gives the right answer under the default schedule
// (ascending threads, ascending blocks) and a different one under the schedule named at it; every twin gives the same bits under all.
#include <hip/hip_runtime.h>

#define ST_NT 256            // four waves

// (a) wave 0 writes LDS, wave 3 reads it; the faulty form has no barrier between the two.
//     Differs under descending waves (mode 2) and with wave 0 as the laggard (mode 4, seed 0).
__global__ void st_cross_wave(const float* in, float* out, int fixed) {
    __shared__ float box[64];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (wave == 0) box[lane] = 2.0f * in[blockIdx.x * 64 + lane];
    if (fixed) __syncthreads();
    if (wave == 3) out[blockIdx.x * 64 + lane] = box[63 - lane] + 1.0f;
}

// (b) a two-slot ring filled two tiles ahead by the last wave and read by the waves below it.  The consumers must be done with a slot
//     before the producer refills it ("slot free"); the faulty form has only the "slot full" barrier.
//     Differs with the producer as the sprinter (mode 5, seed 3).
__global__ void st_ring(const float* in, float* out, int tiles, int fixed) {
    __shared__ float ring[2][64];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const float* src = in + (size_t)blockIdx.x * tiles * 64;
    if (wave == 3) {
        ring[0][lane] = src[lane];
        if (tiles > 1) ring[1][lane] = src[64 + lane];
    }
    __syncthreads();
    float acc = 0.0f;
    for (int t = 0; t < tiles; ++t) {
        if (wave != 3) acc = acc * 0.5f + ring[t & 1][(lane + wave) & 63] * (float)(wave + 1);
        if (fixed) __syncthreads();                              // slot free
        if (wave == 3 && t + 2 < tiles) {
            // the wave rendezvous (a rotate and its inverse) keeps the thread that released the last barrier from running ahead of its
            // wave under the default schedule, as the lanes of a hardware wave cannot either
            const float v = __shfl(__shfl(src[(t + 2) * 64 + lane], (lane + 1) & 63), (lane + 63) & 63);
            ring[t & 1][lane] = v;
        }
        __syncthreads();                                         // slot full
    }
    if (wave != 3) out[((size_t)blockIdx.x * 3 + wave) * 64 + lane] = acc;
}

// (c) a static LDS accumulator; the faulty form adds to it without clearing it first.  `seen` receives the bits every block found in it.
__global__ void st_static_acc(const float* in, float* out, unsigned* seen, int fixed) {
    __shared__ float acc[64];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (wave == 0) {
        unsigned bits;
        memcpy(&bits, &acc[lane], 4);
        seen[blockIdx.x * 64 + lane] = bits;
        if (fixed) acc[lane] = 0.0f;
    }
    __syncthreads();
    for (int w = 0; w < ST_NT / 64; ++w) {
        if (wave == w) acc[lane] += in[(blockIdx.x * (ST_NT / 64) + w) * 64 + lane];
        __syncthreads();
    }
    if (wave == 0) out[blockIdx.x * 64 + lane] = acc[lane];
}

// (d) every block but the first reads what block 0 of the same launch wrote to global memory (a grid-wide dependence without a
//     grid-wide wait).  Differs under descending blocks.  The twin reads the input itself.
__global__ void st_cross_block(const float* in, float* mid, float* out, int fixed) {
    const int lane = threadIdx.x % 64;
    if (threadIdx.x >= 64) return;
    if (blockIdx.x == 0) mid[lane] = 3.0f * in[lane];
    const float v = fixed ? 3.0f * in[lane] : mid[lane];
    out[blockIdx.x * 64 + lane] = v + (float)blockIdx.x;
}

// (e) a block barrier only the first wave reaches: on the emulator a reported deadlock.  No twin; never launched outside a child process.
__global__ void st_divergent_barrier(float* out) {
    if (threadIdx.x < 64) __syncthreads();
    out[threadIdx.x] = 1.0f;
}

extern "C" {
void hipemu_selftest_cross_wave(const float* in, float* out, int blocks, int fixed) {
    hipLaunchKernelGGL(st_cross_wave, dim3(blocks), dim3(ST_NT), 0, nullptr, in, out, fixed);
}
void hipemu_selftest_ring(const float* in, float* out, int blocks, int tiles, int fixed) {
    hipLaunchKernelGGL(st_ring, dim3(blocks), dim3(ST_NT), 0, nullptr, in, out, tiles, fixed);
}
void hipemu_selftest_static_acc(const float* in, float* out, unsigned* seen, int blocks, int fixed) {
    hipLaunchKernelGGL(st_static_acc, dim3(blocks), dim3(ST_NT), 0, nullptr, in, out, seen, fixed);
}
void hipemu_selftest_cross_block(const float* in, float* mid, float* out, int blocks, int fixed) {
    hipLaunchKernelGGL(st_cross_block, dim3(blocks), dim3(ST_NT), 0, nullptr, in, mid, out, fixed);
}
void hipemu_selftest_divergent_barrier(float* out) {
    hipLaunchKernelGGL(st_divergent_barrier, dim3(1), dim3(128), 0, nullptr, out);
}
}
