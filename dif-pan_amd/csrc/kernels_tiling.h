// Overlapping tiles (include/ddif.h states the grid, the weight and the blend -- ddif_tile_count / ddif_tile_origin / ddif_tile_weight are
// the only statement of them, used here as they stand).  Plain HIP, elementwise, vector loads and stores only:
//   tiles_cut_kernel     scenes (S, C, Hs, Ws) -> tiles (S ny nx, C, th, tw), NCHW: one item per tile element
//   tiles_blend_kernel   tiles -> scenes by the blend, NCHW: one item per scene element, its covers read in ascending tile index
//   tile_fuse_kernel     the per-step fusion, in place on the NHWC iterate of a plan: one item per scene element WITH MORE THAN ONE COVER (the plan's
//                        table lists those pixels) reads all its covers, blends, writes the result to every cover.  An item reads and writes the
//                        copies of its own scene element only, so no item reads what another writes
//   randn_tiled_kernel   x_T under tiling: the normal of a tile element is keyed by its SCENE pixel (every cover draws the same one)
#pragma once
#include "sampler_dev.h"
#include "tiling_args.h"

namespace ddif {

// tiles [first, first + count) of an axis cover coordinate y (origins are monotone, so the covers are consecutive)
__device__ __forceinline__ void tile_covers(int y, int L, int t, int ov, int n, int* first, int* count) {
    int f = 0, c = 0;
    for (int k = 0; k < n; ++k) {
        const int p = ddif_tile_origin(k, L, t, ov);
        if (p <= y && y < p + t) {
            if (c == 0) f = k;
            ++c;
        }
    }
    *first = f;
    *count = c;
}

__global__ void tiles_cut_kernel(const float* scene, TileGeom g, float* tiles) {
    const size_t per = (size_t)g.th * g.tw;
    const size_t total = (size_t)g.S * g.ny * g.nx * g.C * per;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int lx = (int)(i % g.tw), ly = (int)((i / g.tw) % g.th);
        const int c = (int)((i / per) % g.C);
        const size_t b = i / (per * g.C);
        const int k = (int)(b % ((size_t)g.ny * g.nx));
        const size_t s = b / ((size_t)g.ny * g.nx);
        const int y = ddif_tile_origin(k / g.nx, g.Hs, g.th, g.ov) + ly, x = ddif_tile_origin(k % g.nx, g.Ws, g.tw, g.ov) + lx;
        tiles[i] = scene[((s * g.C + c) * g.Hs + y) * g.Ws + x];
    }
}

__global__ void tiles_blend_kernel(const float* tiles, TileGeom g, float* scene) {
#pragma clang fp contract(off)
    const size_t per = (size_t)g.th * g.tw;
    const size_t total = (size_t)g.S * g.C * g.Hs * g.Ws;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % g.Ws), y = (int)((i / g.Ws) % g.Hs);
        const int c = (int)((i / ((size_t)g.Ws * g.Hs)) % g.C);
        const size_t s = i / ((size_t)g.Ws * g.Hs * g.C);
        int ky0, cy, kx0, cx;
        tile_covers(y, g.Hs, g.th, g.ov, g.ny, &ky0, &cy);
        tile_covers(x, g.Ws, g.tw, g.ov, g.nx, &kx0, &cx);
        int den = 0;
        for (int ky = ky0; ky < ky0 + cy; ++ky)
            for (int kx = kx0; kx < kx0 + cx; ++kx)
                den += ddif_tile_weight(y, ddif_tile_origin(ky, g.Hs, g.th, g.ov), g.th) * ddif_tile_weight(x, ddif_tile_origin(kx, g.Ws, g.tw, g.ov), g.tw);
        float v0 = 0.f, out = 0.f;
        for (int ky = ky0; ky < ky0 + cy; ++ky) {
            const int py = ddif_tile_origin(ky, g.Hs, g.th, g.ov);
            for (int kx = kx0; kx < kx0 + cx; ++kx) {
                const int px = ddif_tile_origin(kx, g.Ws, g.tw, g.ov);
                const size_t b = (s * g.ny + ky) * g.nx + kx;
                const float v = tiles[(b * g.C + c) * per + (size_t)(y - py) * g.tw + (x - px)];
                if (ky == ky0 && kx == kx0) {
                    v0 = out = v;
                } else {
                    const float r = (float)(ddif_tile_weight(y, py, g.th) * ddif_tile_weight(x, px, g.tw)) / (float)den;
                    out = out + r * (v - v0);
                }
            }
        }
        scene[i] = out;
    }
}

__global__ void randn_tiled_kernel(float* out, int C, TileTab t, unsigned long long seed, unsigned draw, unsigned long long tile0) {
    const size_t HW = (size_t)t.th * t.tw;
    const size_t total = (size_t)t.S * t.ny * t.nx * HW * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const size_t p = (i / C) % HW;
        const size_t b = i / ((size_t)C * HW);
        out[i] = philox_normal(seed, draw, tile_noise_key(t, tile0, C, b, c, p));
    }
}

__global__ void tile_fuse_kernel(float* img, int C, TileTab t) {
#pragma clang fp contract(off)
    const int* py = t.tab;
    const int* px = t.tab + t.ny;
    const int* ycov = px + t.nx;
    const int* xcov = ycov + t.Hs;
    const int* mpx = xcov + t.Ws;
    const size_t total = (size_t)t.S * t.npx * C;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int pix = mpx[(i / C) % t.npx];
        const size_t s = i / ((size_t)C * t.npx);
        const int y = pix / t.Ws, x = pix % t.Ws;
        const int ky0 = ycov[y] & 0xffff, cy = ycov[y] >> 16, kx0 = xcov[x] & 0xffff, cx = xcov[x] >> 16;
        int den = 0;
        for (int ky = ky0; ky < ky0 + cy; ++ky)
            for (int kx = kx0; kx < kx0 + cx; ++kx) den += ddif_tile_weight(y, py[ky], t.th) * ddif_tile_weight(x, px[kx], t.tw);
        float v0 = 0.f, out = 0.f;
        for (int ky = ky0; ky < ky0 + cy; ++ky)
            for (int kx = kx0; kx < kx0 + cx; ++kx) {
                const size_t b = (s * t.ny + ky) * t.nx + kx;
                const float v = img[((b * t.th + (y - py[ky])) * t.tw + (x - px[kx])) * C + c];
                if (ky == ky0 && kx == kx0) {
                    v0 = out = v;
                } else {
                    const float r = (float)(ddif_tile_weight(y, py[ky], t.th) * ddif_tile_weight(x, px[kx], t.tw)) / (float)den;
                    out = out + r * (v - v0);
                }
            }
        for (int ky = ky0; ky < ky0 + cy; ++ky)
            for (int kx = kx0; kx < kx0 + cx; ++kx) {
                const size_t b = (s * t.ny + ky) * t.nx + kx;
                img[((b * t.th + (y - py[ky])) * t.tw + (x - px[kx])) * C + c] = out;
            }
    }
}

}  // namespace ddif
