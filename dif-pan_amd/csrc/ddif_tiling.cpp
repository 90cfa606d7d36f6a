// Host side of the overlapping-tile kernels (kernels_tiling.h): launch helpers for the plan (per-step fusion, scene-keyed x_T) and the stateless entry
// points of include/ddif.h (ddif_tiles_cut, ddif_tiles_blend).
#include "ddif_net.h"
#include "kernels_tiling.h"

namespace ddif {

static inline dim3 tiling_grid(size_t n) {
    size_t g = (n + 255) / 256;
    if (g > 8192) g = 8192;
    if (g < 1) g = 1;
    return dim3((unsigned)g);
}

void tiles_cut_launch(const float* scene, const TileGeom& g, float* tiles, hipStream_t s) {
    hipLaunchKernelGGL(tiles_cut_kernel, tiling_grid((size_t)g.S * g.ny * g.nx * g.C * g.th * g.tw), dim3(256), 0, s, scene, g, tiles);
}
void tiles_blend_launch(const float* tiles, const TileGeom& g, float* scene, hipStream_t s) {
    hipLaunchKernelGGL(tiles_blend_kernel, tiling_grid((size_t)g.S * g.C * g.Hs * g.Ws), dim3(256), 0, s, tiles, g, scene);
}
void tile_fuse_launch(float* img_nhwc, int C, const TileTab& t, hipStream_t s) {
    if (t.npx < 1) return;  // no pixel has two covers (overlap 0 on a multiple of the tile): nothing to fuse
    hipLaunchKernelGGL(tile_fuse_kernel, tiling_grid((size_t)t.S * t.npx * C), dim3(256), 0, s, img_nhwc, C, t);
}
void randn_tiled_launch(float* out_nhwc, int C, const TileTab& t, unsigned long long seed, unsigned draw, unsigned long long tile0, hipStream_t s) {
    hipLaunchKernelGGL(randn_tiled_kernel, tiling_grid((size_t)t.S * t.ny * t.nx * t.th * t.tw * C), dim3(256), 0, s, out_nhwc, C, t, seed, draw, tile0);
}

static int tile_geom(const char* who, const void* in, const void* out, int S, int C, int Hs, int Ws, int th, int tw, int ov, TileGeom* g) {
    if (!in || !out) return fail(DDIF_ERR_INVALID, "%s: NULL argument", who);
    if (S < 1 || C < 1 || th < 1 || tw < 1) return fail(DDIF_ERR_INVALID, "%s: S=%d C=%d tile %dx%d must all be >= 1", who, S, C, th, tw);
    if (ov < 0 || ov >= (th < tw ? th : tw)) return fail(DDIF_ERR_INVALID, "%s: overlap %d outside [0, min(tile_h, tile_w) = %d)", who, ov, th < tw ? th : tw);
    if (Hs < th || Ws < tw) return fail(DDIF_ERR_INVALID, "%s: a scene of %dx%d is smaller than the %dx%d tile", who, Hs, Ws, th, tw);
    const long long ny = ddif_tile_count(Hs, th, ov), nx = ddif_tile_count(Ws, tw, ov);
    if ((long long)S * ny * nx > 0x7fffffffLL) return fail(DDIF_ERR_INVALID, "%s: more than 2^31 tiles", who);
    *g = TileGeom{S, C, Hs, Ws, th, tw, ov, (int)ny, (int)nx};
    return 0;
}

}  // namespace ddif

extern "C" {

int ddif_tiles_cut(const float* scene, int S, int C, int Hs, int Ws, int tile_h, int tile_w, int overlap, float* tiles, void* stream) {
    ddif::TileGeom g;
    if (int e = ddif::tile_geom("ddif_tiles_cut", scene, tiles, S, C, Hs, Ws, tile_h, tile_w, overlap, &g)) return e;
    ddif::tiles_cut_launch(scene, g, tiles, (hipStream_t)stream);
    DDIF_HIPCHK(hipGetLastError());
    return DDIF_OK;
}

int ddif_tiles_blend(const float* tiles, int S, int C, int Hs, int Ws, int tile_h, int tile_w, int overlap, float* scene, void* stream) {
    ddif::TileGeom g;
    if (int e = ddif::tile_geom("ddif_tiles_blend", tiles, scene, S, C, Hs, Ws, tile_h, tile_w, overlap, &g)) return e;
    ddif::tiles_blend_launch(tiles, g, scene, (hipStream_t)stream);
    DDIF_HIPCHK(hipGetLastError());
    return DDIF_OK;
}

}  // extern "C"
