// Launch arguments of the overlapping-tile kernels (kernels_tiling.h, ddif_tiling.cpp); shared with the plan.  The grid, the weight and the blend are
// defined in include/ddif.h (ddif_tile_count / ddif_tile_origin / ddif_tile_weight) and nowhere else.
#pragma once
#include "../../include/ddif.h"
#include "ddif_dev.h"

namespace ddif {

// stand-alone cut / blend (NCHW scenes and tiles): origins come from ddif_tile_origin in the kernel
struct TileGeom {
    int S, C, Hs, Ws, th, tw, ov, ny, nx;
};

// A plan's device table (ints), built by Plan::set_tiling:
//   py[ny] | px[nx] | ycov[Hs] | xcov[Ws] | mpx[npx]
// ycov[y] = first covering tile row | (number of covering rows << 16) -- covers are consecutive, origins being monotone -- xcov alike;
// mpx = y * Ws + x of every scene pixel with more than one cover, ascending: the only pixels the per-step fusion visits.
struct TileTab {
    const int* tab;  // null: no tiling
    int S, Hs, Ws, th, tw, ny, nx, npx;
};

// element (b, p, c) of a plan's NHWC tensors -> its scene and scene pixel
__device__ __forceinline__ void tile_scene_pixel(const TileTab& t, size_t b, size_t p, size_t* scene, int* y, int* x) {
    const int k = (int)(b % ((size_t)t.ny * t.nx));
    *scene = b / ((size_t)t.ny * t.nx);
    *y = t.tab[k / t.nx] + (int)(p / t.tw);
    *x = t.tab[t.ny + k % t.nx] + (int)(p % t.tw);
}
// the Philox element of a scene pixel (include/ddif.h ddif_plan_set_tiling)
__device__ __forceinline__ unsigned long long tile_noise_key(const TileTab& t, unsigned long long tile0, int C, size_t b, int c, size_t p) {
    size_t s;
    int y, x;
    tile_scene_pixel(t, b, p, &s, &y, &x);
    return ((tile0 + s) * C + c) * ((unsigned long long)t.Hs * t.Ws) + (unsigned long long)y * t.Ws + x;
}

void tiles_cut_launch(const float* scene, const TileGeom& g, float* tiles, hipStream_t s);
void tiles_blend_launch(const float* tiles, const TileGeom& g, float* scene, hipStream_t s);
void tile_fuse_launch(float* img_nhwc, int C, const TileTab& t, hipStream_t s);
void randn_tiled_launch(float* out_nhwc, int C, const TileTab& t, unsigned long long seed, unsigned draw, unsigned long long tile0, hipStream_t s);

}  // namespace ddif
