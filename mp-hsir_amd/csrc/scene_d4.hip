// Self-ensemble for whole-scene inference: the network restores every tile under G of the eight flip / rotation transforms of
// degrade.augment (mode m: rot90 counter-clockwise by m / 2, then an up-down flip when m is odd) and the G restorations, each mapped
// back, are averaged into the tile store that scene_blend reads (mp-hsir_amd/scene.py; include/mphsir.h holds the definitions).
//
//   d4_gather   tiles [count][C][th][tw] <- mode_g(mirror-cut tile t of scene [C][H][W]) for the items j = g * n_tiles + t of a batch
//   d4_fold     store [n_tiles][C][th][tw] <- (store or 0) + sum over the batch's items of a tile, in ascending j, of inverse_mode_g(y)
//   bands_gather  the d4 gather with one more folded coordinate: an item has a band origin too and channel c of it is scene band
//               mirror(ob + c, Cs) (spectral windows: include/mphsir_bands.h); the same body, origin rows of three
//
// Every mode is one index map of the tile (struct D4 of mphsir_planar.h holds the table; a transposing mode has th == tw), and the fold
// reads y through the same map the other way round.
//
// Both are streaming kernels; a thread owns 4 consecutive x of one row of the TILE side and walks a chunk of channels, as in scene.hip.
// Non-transposing modes: the tile side moves as 16-byte vectors; a reversed row is the quad at the mirrored column, reversed in
// registers.  Transposing modes: a row of one side is a column of the other, so a workgroup owns a 32 x 32 square and passes it through
// LDS, D4_LC channels at a time: both global sides stay row-contiguous (128 bytes per row of the square, 8 lanes x 16 bytes on a tile
// side).  The LDS rows have a pitch of 33 dwords: the writers (32 lanes along a row, or 8 quads x 4 rows) and the readers (lane (r, c)
// of 4 x 8 reads element (4c + k, r): bank 4c + r + 33k mod 32) each touch 32 different banks per 32-lane group.  A 32-lane group is the
// unit that matters in a wave of 64: every LDS access here is a ds_read_b32 / ds_write_b32 (the pitch of 33 rules out wider ones), which
// gfx950 services as the two halves {0-31}, {32-63}, one LDS cycle each, with banks taken mod 32; lanes l and l + 32 are never in the
// same cycle, so that they share a bank costs nothing.
//
// The modes come by value and the item arithmetic uses validated scalars only; the one device array, `origins`, is read at t < n_tiles
// and its values are folded into the scene by the mirror map, so no access depends on it holding a valid plan (origins within +-2^30).
#include "mphsir_host.h"
#include "mphsir_planar.h"
#include "../../include/mphsir_bands.h"

namespace mphsir {

constexpr int D4_CH = 8;             // channels per thread of the gather (SCENE_CH of scene.hip)
constexpr int D4_LC = 4;             // channels per pass through LDS (4 * 32 * 33 * 4 = 16.5 KiB: 8 workgroups per CU stay resident) and per
                                     // thread of the fold, whose accumulators and loads in flight are 8 registers a channel
constexpr int D4_S = 32;             // side of a workgroup's square in the transposing modes
constexpr int D4_P = D4_S + 1;       // LDS row pitch in dwords

struct D4GatherDev {
    const float* scene; const int* origins; float* tiles;
    int j0, n_tiles, last, modes, C, Cs, H, W, th, tw;      // Cs: the scene's band count (the band form; else C)
};

typedef float (*D4Lds)[D4_S][D4_P];

// The body of both gathers.  `bands` is a literal in each of the two kernels below, so every test of it folds away: false is the d4 gather
// as it was (origin rows {oy, ox}, channel c of an item is scene band c), true reads rows {ob, oy, ox} and takes channel c from scene
// band mirror(ob + c, Cs).  The band is a function of the workgroup's indices alone, so its fold is scalar work.
__device__ __forceinline__ void d4_gather_body(const D4GatherDev& a, D4Lds lds, const bool bands) {
    const int jz = a.j0 + (int)blockIdx.z, j = jz < a.last ? jz : a.last;
    const int g = j / a.n_tiles, t = j - g * a.n_tiles;
    const D4 d4((a.modes >> (3 * g)) & 7);
    const bool fy = d4.fy, fx = d4.fx;
    const int* org = a.origins + (bands ? 3 : 2) * t;
    const int ob = bands ? org[0] : 0, oy = org[bands ? 1 : 0], ox = org[bands ? 2 : 1];
    const int c0 = blockIdx.y * D4_CH;
    const long plane = (long)a.H * a.W, tplane = (long)a.th * a.tw;
    long band[D4_CH];                                             // the scene plane of each channel of the chunk, in floats
#pragma unroll
    for (int c = 0; c < D4_CH; ++c) band[c] = (bands ? (long)mirror(ob + c0 + c, a.Cs) : (long)(c0 + c)) * plane;
    const float* src = a.scene;
    float* dst = a.tiles + ((long)blockIdx.z * a.C + c0) * tplane;
    const int tid = threadIdx.x;
    if (!d4.tr) {
        const int tw4 = a.tw >> 2;
        const int idx = blockIdx.x * 256 + tid;
        if (idx >= a.th * tw4) return;
        const int u = idx / tw4, v = (idx - u * tw4) * 4;
        const long row = (long)mirror(oy + (fy ? a.th - 1 - u : u), a.H) * a.W;
        int x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] = mirror(ox + (fx ? a.tw - 1 - (v + k) : v + k), a.W);
        src += row;
        dst += (long)u * a.tw + v;
#pragma unroll
        for (int c = 0; c < D4_CH; ++c) {
            if (c0 + c < a.C) {
                const float* s = src + band[c];
                f32x4 o;
                o[0] = s[x[0]]; o[1] = s[x[1]]; o[2] = s[x[2]]; o[3] = s[x[3]];
                *reinterpret_cast<f32x4*>(dst + c * tplane) = o;
            }
        }
        return;
    }
    // transposing: th == tw == n.  Output square rows U0.., columns V0..; element (u, v) of it is P(v, u), P the flipped tile.
    const int n = a.th, nb = (n + D4_S - 1) / D4_S;
    if ((int)blockIdx.x >= nb * nb) return;                       // whole workgroup: no barrier is skipped by a part of it
    const int U0 = ((int)blockIdx.x / nb) * D4_S, V0 = ((int)blockIdx.x % nb) * D4_S;
    const int lq = tid & 31, lp0 = tid >> 5;                      // loader: column q = U0 + lq of P, rows p = V0 + lp0 + 8k
    const int q = U0 + lq;
    const int col = mirror(ox + (fx ? n - 1 - q : q), a.W);
    long rows[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = V0 + lp0 + 8 * k;
        rows[k] = (long)mirror(oy + (fy ? n - 1 - p : p), a.H) * a.W;      // p >= n: a legal address whose value is never stored
    }
    const int ou = tid >> 3, ov = (tid & 7) * 4;                  // writer: row U0 + ou, columns V0 + ov .. + 3
    const bool wr = U0 + ou < n && V0 + ov < n;
    dst += (long)(U0 + ou) * n + V0 + ov;
#pragma unroll
    for (int h = 0; h < D4_CH; h += D4_LC) {
        if (h) __syncthreads();
#pragma unroll
        for (int c = 0; c < D4_LC; ++c) {
            if (c0 + h + c < a.C) {
                const float* s = src + band[h + c] + col;
#pragma unroll
                for (int k = 0; k < 4; ++k) lds[c][lp0 + 8 * k][lq] = s[rows[k]];
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < D4_LC; ++c) {
            if (wr && c0 + h + c < a.C) {
                f32x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = lds[c][ov + k][ou];
                *reinterpret_cast<f32x4*>(dst + (h + c) * tplane) = o;
            }
        }
    }
}

// grid (max(ceil(th * tw/4 / 256), ceil(th/32) * ceil(tw/32)), ceil(C / D4_CH), count)
__global__ __launch_bounds__(256) void d4_gather_kernel(D4GatherDev a) {
    __shared__ float lds[D4_LC][D4_S][D4_P];
    d4_gather_body(a, lds, false);
}

// the same grid; origins [n_tiles][3]
__global__ __launch_bounds__(256) void bands_gather_kernel(D4GatherDev a) {
    __shared__ float lds[D4_LC][D4_S][D4_P];
    d4_gather_body(a, lds, true);
}

struct D4FoldDev {
    const float* y; float* store;
    int j0, count, n_tiles, G, modes, C, th, tw, square;
};

// grid (square ? ceil(th/32)^2 : ceil(th * tw/4 / 256), ceil(C / D4_LC), min(count, n_tiles)); square: one of the G modes transposes,
// and every thread must own the same store elements under all modes of the call.  One kernel serves both ownerships: its 16.5 KiB of
// LDS, unused when no mode transposes, allow 8 workgroups = 32 waves per CU, which is what its registers (58) allow as well.
__global__ __launch_bounds__(256) void d4_fold_kernel(D4FoldDev a) {
    __shared__ float lds[D4_LC][D4_S][D4_P];
    const int tid = threadIdx.x;
    const int jf = a.j0 + (int)blockIdx.z;                        // this tile's first item of the call; the others follow n_tiles apart
    const int gf = jf / a.n_tiles, t = jf - gf * a.n_tiles;
    const int items = (a.count - (int)blockIdx.z + a.n_tiles - 1) / a.n_tiles;
    const int c0 = blockIdx.y * D4_LC;
    const long tplane = (long)a.th * a.tw;
    int ra, rb, A0 = 0, B0 = 0;                                   // the thread's quad: store row ra, columns rb .. rb + 3
    bool own;
    if (a.square) {
        const int nb = (a.th + D4_S - 1) / D4_S;
        A0 = ((int)blockIdx.x / nb) * D4_S, B0 = ((int)blockIdx.x % nb) * D4_S;
        ra = A0 + (tid >> 3), rb = B0 + (tid & 7) * 4;
        own = ra < a.th && rb < a.tw;
    } else {
        const int tw4 = a.tw >> 2;
        const int idx = blockIdx.x * 256 + tid;
        ra = idx / tw4, rb = (idx - ra * tw4) * 4;
        own = idx < a.th * tw4;
    }
    float* st = a.store + ((long)t * a.C + c0) * tplane + (long)ra * a.tw + rb;
    float acc[D4_LC][4];
#pragma unroll
    for (int c = 0; c < D4_LC; ++c) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (gf != 0 && own && c0 + c < a.C) v = *reinterpret_cast<const f32x4*>(st + c * tplane);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[c][k] = v[k];
    }
#pragma unroll 1
    for (int r = 0; r < items; ++r) {
        const int g = gf + r;
        const D4 d4((a.modes >> (3 * g)) & 7);
        const bool fy = d4.fy, fx = d4.fx;
        const float* y = a.y + ((long)((int)blockIdx.z + r * a.n_tiles) * a.C + c0) * tplane;
        if (!d4.tr) {
            if (own) {
                const float* s = y + (long)(fy ? a.th - 1 - ra : ra) * a.tw + (fx ? a.tw - 4 - rb : rb);
#pragma unroll
                for (int c = 0; c < D4_LC; ++c) {
                    if (c0 + c < a.C) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(s + c * tplane);
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[c][k] += fx ? v[3 - k] : v[k];
                    }
                }
            }
            continue;          // the mode belongs to the item, so it is uniform over the workgroup: all of it skips the barriers below, or none
        }
        // transposing (square, th == tw == n): store (a, b) takes y (u, v) = (fx ? n - 1 - b : b, fy ? n - 1 - a : a)
        const int n = a.th;
        const int Ub = fx ? n - D4_S - B0 : B0, Vb = fy ? n - D4_S - A0 : A0;      // the square of y this workgroup needs (may overhang)
        const int lu = tid >> 3, lv = (tid & 7) * 4;
        const bool ld = (unsigned)(Ub + lu) < (unsigned)n && (unsigned)(Vb + lv) < (unsigned)n;      // n, Vb, lv multiples of 4
        const float* s = y + (long)(Ub + lu) * n + Vb + lv;
        const int rv = fy ? D4_S - 1 - (tid >> 3) : (tid >> 3);
        const int ru = fx ? D4_S - 1 - (tid & 7) * 4 : (tid & 7) * 4, du = fx ? -1 : 1;
        __syncthreads();                                          // the readers of the previous item are done
#pragma unroll
        for (int c = 0; c < D4_LC; ++c) {
            if (ld && c0 + c < a.C) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(s + c * tplane);
#pragma unroll
                for (int k = 0; k < 4; ++k) lds[c][lu][lv + k] = v[k];
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < D4_LC; ++c) {
            if (own && c0 + c < a.C) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[c][k] += lds[c][ru + du * k][rv];
            }
        }
    }
    if (!own) return;
    const float scale = gf + items == a.G ? 1.f / (float)a.G : 1.f;
#pragma unroll
    for (int c = 0; c < D4_LC; ++c) {
        if (c0 + c < a.C)
            *reinterpret_cast<f32x4*>(st + c * tplane) = f32x4{acc[c][0] * scale, acc[c][1] * scale, acc[c][2] * scale, acc[c][3] * scale};
    }
}

// G in {1, 2, 4, 8} and nothing set above the 3 bits of each of the G passes (every 3-bit value is a mode)
static bool d4_modes_ok(int G, int modes) {
    return (G == 1 || G == 2 || G == 4 || G == 8) && modes >= 0 && (modes >> (3 * G)) == 0;
}

static bool d4_transposes(int G, int modes) {
    for (int g = 0; g < G; ++g)
        if ((modes >> (3 * g)) & 2) return true;
    return false;
}

}  // namespace mphsir

extern "C" int mphsir_scene_gather_d4(const mphsir_scene_gather_d4_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "scene_gather_d4");
    MPHSIR_REQUIRE(a->scene && a->origins && a->tiles, "scene_gather_d4: null pointer");
    MPHSIR_REQUIRE(a->count > 0 && a->count <= 65535 && a->C > 0 && a->H > 0 && a->W > 0,
                   "scene_gather_d4: bad sizes (count %d, C %d, H %d, W %d; count <= 65535)", a->count, a->C, a->H, a->W);
    MPHSIR_REQUIRE(d4_modes_ok(a->G, a->modes_packed),
                   "scene_gather_d4: G %d must be 1, 2, 4 or 8 and modes_packed 0x%x hold 3 bits for each of the G passes", a->G, a->modes_packed);
    MPHSIR_REQUIRE(a->n_tiles > 0 && a->n_tiles < (1 << 24) && a->j0 >= 0 && a->j0 < a->G * a->n_tiles,
                   "scene_gather_d4: item %d outside the %d x %d items", a->j0, a->G, a->n_tiles);
    MPHSIR_REQUIRE(a->th > 0 && a->tw > 0 && a->th % 4 == 0 && a->tw % 4 == 0 && aligned16(a->tiles),
                   "scene_gather_d4: tile %d x %d must be multiples of 4 and the tile buffer 16-byte aligned", a->th, a->tw);
    MPHSIR_REQUIRE(a->th == a->tw || !d4_transposes(a->G, a->modes_packed),
                   "scene_gather_d4: a transposing mode (2, 3, 6, 7) needs a square tile, got %d x %d", a->th, a->tw);
    const long quads = (long)a->th * (a->tw / 4), chunks = (a->C + D4_CH - 1) / D4_CH;
    MPHSIR_REQUIRE(quads < (1L << 30) && (long)a->H * a->W < (1L << 31) && chunks <= 65535, "scene_gather_d4: scene or tile too large");
    const long squares = (long)((a->th + D4_S - 1) / D4_S) * ((a->tw + D4_S - 1) / D4_S), lin = (quads + 255) / 256;
    D4GatherDev d{a->scene, a->origins, a->tiles, a->j0, a->n_tiles, a->G * a->n_tiles - 1, a->modes_packed, a->C, a->C, a->H, a->W, a->th, a->tw};
    MPHSIR_LAUNCH(MPHSIR_K_SCENE, d4_gather_kernel, dim3((unsigned)(lin > squares ? lin : squares), (unsigned)chunks, (unsigned)a->count), dim3(256),
                  0, reinterpret_cast<hipStream_t>(stream), d);
    return MPHSIR_OK;
}

extern "C" int mphsir_scene_gather_bands(const mphsir_scene_gather_bands_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "scene_gather_bands");
    MPHSIR_REQUIRE(a->scene && a->origins && a->tiles, "scene_gather_bands: null pointer");
    MPHSIR_REQUIRE(a->count > 0 && a->count <= 65535 && a->C > 0 && a->Cs > 0 && a->H > 0 && a->W > 0,
                   "scene_gather_bands: bad sizes (count %d, C %d, Cs %d, H %d, W %d; count <= 65535)", a->count, a->C, a->Cs, a->H, a->W);
    MPHSIR_REQUIRE(d4_modes_ok(a->G, a->modes_packed),
                   "scene_gather_bands: G %d must be 1, 2, 4 or 8 and modes_packed 0x%x hold 3 bits for each of the G passes", a->G, a->modes_packed);
    MPHSIR_REQUIRE(a->n_tiles > 0 && a->n_tiles < (1 << 24) && a->j0 >= 0 && a->j0 < a->G * a->n_tiles,
                   "scene_gather_bands: item %d outside the %d x %d items", a->j0, a->G, a->n_tiles);
    MPHSIR_REQUIRE(a->th > 0 && a->tw > 0 && a->th % 4 == 0 && a->tw % 4 == 0 && aligned16(a->tiles),
                   "scene_gather_bands: tile %d x %d must be multiples of 4 and the tile buffer 16-byte aligned", a->th, a->tw);
    MPHSIR_REQUIRE(a->th == a->tw || !d4_transposes(a->G, a->modes_packed),
                   "scene_gather_bands: a transposing mode (2, 3, 6, 7) needs a square tile, got %d x %d", a->th, a->tw);
    const long quads = (long)a->th * (a->tw / 4), chunks = (a->C + D4_CH - 1) / D4_CH;
    MPHSIR_REQUIRE(quads < (1L << 30) && (long)a->H * a->W < (1L << 31) && chunks <= 65535, "scene_gather_bands: scene or tile too large");
    const long squares = (long)((a->th + D4_S - 1) / D4_S) * ((a->tw + D4_S - 1) / D4_S), lin = (quads + 255) / 256;
    D4GatherDev d{a->scene, a->origins, a->tiles, a->j0, a->n_tiles, a->G * a->n_tiles - 1, a->modes_packed, a->C, a->Cs, a->H, a->W, a->th, a->tw};
    MPHSIR_LAUNCH(MPHSIR_K_SCENE, bands_gather_kernel, dim3((unsigned)(lin > squares ? lin : squares), (unsigned)chunks, (unsigned)a->count), dim3(256),
                  0, reinterpret_cast<hipStream_t>(stream), d);
    return MPHSIR_OK;
}

extern "C" int mphsir_scene_fold_d4(const mphsir_scene_fold_d4_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "scene_fold_d4");
    MPHSIR_REQUIRE(a->y && a->store, "scene_fold_d4: null pointer");
    MPHSIR_REQUIRE(a->C > 0 && a->th > 0 && a->tw > 0 && a->th % 4 == 0 && a->tw % 4 == 0 && aligned16(a->y) && aligned16(a->store),
                   "scene_fold_d4: C %d, tile %d x %d: extents must be multiples of 4 and both buffers 16-byte aligned", a->C, a->th, a->tw);
    MPHSIR_REQUIRE(d4_modes_ok(a->G, a->modes_packed),
                   "scene_fold_d4: G %d must be 1, 2, 4 or 8 and modes_packed 0x%x hold 3 bits for each of the G passes", a->G, a->modes_packed);
    MPHSIR_REQUIRE(a->n_tiles > 0 && a->n_tiles < (1 << 24) && a->j0 >= 0 && a->count > 0 && a->count <= a->G * a->n_tiles - a->j0,
                   "scene_fold_d4: items [%d, %d + %d) outside the %d x %d items", a->j0, a->j0, a->count, a->G, a->n_tiles);
    const int square = d4_transposes(a->G, a->modes_packed);
    MPHSIR_REQUIRE(a->th == a->tw || !square, "scene_fold_d4: a transposing mode (2, 3, 6, 7) needs a square tile, got %d x %d", a->th, a->tw);
    const long quads = (long)a->th * (a->tw / 4), chunks = (a->C + D4_LC - 1) / D4_LC;
    const int tiles = a->count < a->n_tiles ? a->count : a->n_tiles;
    MPHSIR_REQUIRE(quads < (1L << 30) && chunks <= 65535 && tiles <= 65535, "scene_fold_d4: tile too large, or more than 65535 tiles in one call");
    const long nb = (a->th + D4_S - 1) / D4_S;
    D4FoldDev d{a->y, a->store, a->j0, a->count, a->n_tiles, a->G, a->modes_packed, a->C, a->th, a->tw, square};
    MPHSIR_LAUNCH(MPHSIR_K_SCENE, d4_fold_kernel, dim3((unsigned)(square ? nb * nb : (quads + 255) / 256), (unsigned)chunks, (unsigned)tiles), dim3(256),
                  0, reinterpret_cast<hipStream_t>(stream), d);
    return MPHSIR_OK;
}
