// Whole-scene inference: a scene (C,H,W) is cut into overlapping tiles that the network restores one batch at a time, and the
// restored tiles are blended back into the scene (mp-hsir_amd/scene.py holds the tile plan; include/mphsir.h the definitions).
//
//   scene_gather   tiles [n][C][th][tw] <- scene [C][H][W] at n origins (device int32 pairs), mirror-mapped on every side
//   scene_blend    scene [C][H][W] <- sum(w * tile) / sum(w) over the covering tiles, in ascending tile number
//
// Both are streaming kernels without LDS.  One thread owns 4 consecutive x of one row and walks a chunk of SCENE_CH channels, so
// that the coordinate work (the mirror map; the scan of the origin arrays and the ramp weights, a handful of fp32 divisions)
// is paid once per 4 * SCENE_CH elements and the loads of a chunk are independent.  Tile extents are multiples of 4 floats and
// tile rows start 16-byte aligned: the tile side moves as 16-byte vectors (the blend, whose tile column is x - ox, whenever
// that is a multiple of 4 and the quad lies inside the tile; scalar otherwise).  W is arbitrary, so scene rows are not aligned:
// dword accesses there, consecutive lanes 16 bytes apart, four instructions covering every line they touch.
//
// No access depends on the origin arrays holding a valid plan: the gather folds every coordinate into [0,H) x [0,W); the blend
// dereferences tile (iy,ix) only at local coordinates it has checked against [0,th) x [0,tw) (the pointer `src` itself may be formed
// up to 3 floats outside a row and is then never read through).  Origins are expected within +-2^30, so that origin + coordinate
// stays inside int; the host cannot check device arrays, and beyond that range the sums wrap before they are folded / compared.
#include "mphsir_host.h"
#include "mphsir_planar.h"

namespace mphsir {

constexpr int SCENE_CH = 8;        // channels per thread

struct GatherDev {
    const float* scene; const int* origins; float* tiles;
    int C, H, W, th, tw;
};

// grid (ceil(th * tw/4 / 256), ceil(C / SCENE_CH), n)
__global__ __launch_bounds__(256) void scene_gather_kernel(GatherDev a) {
    const int tw4 = a.tw >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.th * tw4) return;
    const int u = idx / tw4, v = (idx - u * tw4) * 4;
    const int t = blockIdx.z;
    const int oy = a.origins[2 * t], ox = a.origins[2 * t + 1];
    const long row = (long)mirror(oy + u, a.H) * a.W;
    const int x0 = mirror(ox + v, a.W), x1 = mirror(ox + v + 1, a.W), x2 = mirror(ox + v + 2, a.W), x3 = mirror(ox + v + 3, a.W);
    const int c0 = blockIdx.y * SCENE_CH;
    const long plane = (long)a.H * a.W, tplane = (long)a.th * a.tw;
    const float* src = a.scene + c0 * plane + row;
    float* dst = a.tiles + ((long)t * a.C + c0) * tplane + (long)u * a.tw + v;
#pragma unroll
    for (int c = 0; c < SCENE_CH; ++c) {
        if (c0 + c < a.C) {
            const float* s = src + c * plane;
            f32x4 o;
            o[0] = s[x0]; o[1] = s[x1]; o[2] = s[x2]; o[3] = s[x3];
            *reinterpret_cast<f32x4*>(dst + c * tplane) = o;
        }
    }
}

struct BlendDev {
    const float* tiles; const int* oy; const int* ox; float* scene;
    int ny, nx, C, H, W, th, tw, ov, clamp01;
};

// grid (ceil(H * ceil(W/4) / 256), ceil(C / SCENE_CH))
__global__ __launch_bounds__(256) void scene_blend_kernel(BlendDev a) {
    const int W4 = (a.W + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.H * W4) return;
    const int y = idx / W4, x = (idx - y * W4) * 4;
    const int c0 = blockIdx.y * SCENE_CH;
    const int nc = a.C - c0 < SCENE_CH ? a.C - c0 : SCENE_CH;
    const long tplane = (long)a.th * a.tw;
    const float ovp1 = (float)(a.ov + 1);
    float num[SCENE_CH][4], den[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < SCENE_CH; ++c)
#pragma unroll
        for (int k = 0; k < 4; ++k) num[c][k] = 0.f;
    for (int iy = 0; iy < a.ny; ++iy) {
        const int oy = a.oy[iy], uy = y - oy;
        if ((unsigned)uy >= (unsigned)a.th) continue;
        const float wy = ramp(uy, oy, a.th, a.H, ovp1);
        for (int ix = 0; ix < a.nx; ++ix) {
            const int ox = a.ox[ix], vx = x - ox;              // tile column of the quad's first pixel
            if (vx <= -4 || vx >= a.tw) continue;
            float w[4];
            bool in[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                in[k] = (unsigned)(vx + k) < (unsigned)a.tw && x + k < a.W;
                w[k] = in[k] ? wy * ramp(vx + k, ox, a.tw, a.W, ovp1) : 0.f;
                den[k] += w[k];
            }
            const float* src = a.tiles + ((long)(iy * a.nx + ix) * a.C + c0) * tplane + (long)uy * a.tw + vx;
            if (in[0] && in[3] && (vx & 3) == 0) {
#pragma unroll
                for (int c = 0; c < SCENE_CH; ++c) {
                    if (c < nc) {
                        const f32x4 t = *reinterpret_cast<const f32x4*>(src + c * tplane);
#pragma unroll
                        for (int k = 0; k < 4; ++k) num[c][k] += w[k] * t[k];
                    }
                }
            } else {
#pragma unroll
                for (int c = 0; c < SCENE_CH; ++c) {
                    if (c < nc) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) num[c][k] += w[k] * (in[k] ? src[c * tplane + k] : 0.f);
                    }
                }
            }
        }
    }
    float* dst = a.scene + (long)c0 * a.H * a.W + (long)y * a.W + x;
#pragma unroll
    for (int c = 0; c < SCENE_CH; ++c) {
        if (c < nc) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (x + k < a.W) {
                    float r = num[c][k] / den[k];
                    if (a.clamp01) r = fminf(fmaxf(r, 0.f), 1.f);
                    dst[(long)c * a.H * a.W + k] = r;
                }
            }
        }
    }
}

}  // namespace mphsir

extern "C" int mphsir_scene_gather(const mphsir_scene_gather_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "scene_gather");
    MPHSIR_REQUIRE(a->scene && a->origins && a->tiles, "scene_gather: null pointer");
    MPHSIR_REQUIRE(a->n > 0 && a->n <= 65535 && a->C > 0 && a->H > 0 && a->W > 0, "scene_gather: bad sizes (n %d, C %d, H %d, W %d; n <= 65535)",
                   a->n, a->C, a->H, a->W);
    MPHSIR_REQUIRE(a->th > 0 && a->tw > 0 && a->th % 4 == 0 && a->tw % 4 == 0 && aligned16(a->tiles),
                   "scene_gather: tile %d x %d must be multiples of 4 and the tile buffer 16-byte aligned", a->th, a->tw);
    const long quads = (long)a->th * (a->tw / 4), chunks = (a->C + SCENE_CH - 1) / SCENE_CH;
    MPHSIR_REQUIRE(quads < (1L << 30) && (long)a->H * a->W < (1L << 31) && chunks <= 65535, "scene_gather: scene or tile too large");
    GatherDev d{a->scene, a->origins, a->tiles, a->C, a->H, a->W, a->th, a->tw};
    MPHSIR_LAUNCH(MPHSIR_K_SCENE, scene_gather_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)chunks, (unsigned)a->n), dim3(256), 0,
                  reinterpret_cast<hipStream_t>(stream), d);
    return MPHSIR_OK;
}

extern "C" int mphsir_scene_blend(const mphsir_scene_blend_args* a, void* stream) {
    using namespace mphsir;
    clear_error();
    MPHSIR_CHECK_ARGS(a, "scene_blend");
    MPHSIR_REQUIRE(a->tiles && a->oy && a->ox && a->scene, "scene_blend: null pointer");
    MPHSIR_REQUIRE(a->ny > 0 && a->nx > 0 && a->C > 0 && a->H > 0 && a->W > 0, "scene_blend: bad sizes (ny %d, nx %d, C %d, H %d, W %d)",
                   a->ny, a->nx, a->C, a->H, a->W);
    MPHSIR_REQUIRE(a->th > 0 && a->tw > 0 && a->th % 4 == 0 && a->tw % 4 == 0 && aligned16(a->tiles),
                   "scene_blend: tile %d x %d must be multiples of 4 and the tile buffer 16-byte aligned", a->th, a->tw);
    MPHSIR_REQUIRE(a->ov >= 0 && a->ov < (1 << 24), "scene_blend: overlap %d out of range", a->ov);
    const long quads = (long)a->H * ((a->W + 3) / 4), chunks = (a->C + SCENE_CH - 1) / SCENE_CH;
    MPHSIR_REQUIRE(quads < (1L << 30) && (long)a->ny * a->nx < (1L << 24) && (long)a->th * a->tw < (1L << 30) && chunks <= 65535,
                   "scene_blend: scene or tile too large");
    BlendDev d{a->tiles, a->oy, a->ox, a->scene, a->ny, a->nx, a->C, a->H, a->W, a->th, a->tw, a->ov, a->clamp01};
    MPHSIR_LAUNCH(MPHSIR_K_SCENE, scene_blend_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)chunks), dim3(256), 0,
                  reinterpret_cast<hipStream_t>(stream), d);
    return MPHSIR_OK;
}
