// Host side of the Q2n quality index (kernels_q2n.h): argument checks and the two launches; the block map of a call without map_out lives in the
// metric kernels' scratch.  The entry point is declared in include/ddif.h.
#include <cmath>
#include "ddif_net.h"
#include "kernels_q2n.h"

namespace ddif {
int metric_scratch(size_t n, double** out);  // ddif_aux.cpp: per-device scratch of the metric kernels, grown on demand

namespace {
template <int CP>
void q2n_launch(hipStream_t s, unsigned nwg, const float* gt, const float* pred, int C, int H, int W, float scale, int block, int shift, int nx, int ny, double* map) {
    hipLaunchKernelGGL(q2n_block_kernel<CP>, dim3(nwg), dim3(256), DDIF_Q2N_SMEM, s, gt, pred, C, H, W, scale, block, shift, nx, ny, map);
}
}  // namespace
}  // namespace ddif

extern "C" {

int ddif_q2n(const float* gt, const float* pred, int B, int C, int H, int W, float scale, int block, int shift, double* map_out, double* q_out, void* stream) {
    if (!gt) return ddif::fail(DDIF_ERR_INVALID, "ddif_q2n: gt is NULL");
    if (!pred) return ddif::fail(DDIF_ERR_INVALID, "ddif_q2n: pred is NULL");
    if (!q_out) return ddif::fail(DDIF_ERR_INVALID, "ddif_q2n: q_out is NULL");
    if (C < 1 || C > 8) return ddif::fail(DDIF_ERR_INVALID, "ddif_q2n: C=%d is outside 1..8 (Q2n is defined up to Q8)", C);
    if (block < 2 || block > 64) return ddif::fail(DDIF_ERR_INVALID, "ddif_q2n: block=%d is outside 2..64", block);
    if (shift < 1 || shift > block) return ddif::fail(DDIF_ERR_INVALID, "ddif_q2n: shift=%d is outside 1..block (block=%d)", shift, block);
    if (B < 1) return ddif::fail(DDIF_ERR_INVALID, "ddif_q2n: B=%d must be >= 1", B);
    if (H < 1) return ddif::fail(DDIF_ERR_INVALID, "ddif_q2n: H=%d must be >= 1", H);
    if (W < 1) return ddif::fail(DDIF_ERR_INVALID, "ddif_q2n: W=%d must be >= 1", W);
    if (!std::isfinite(scale) || !(scale > 0.f)) return ddif::fail(DDIF_ERR_INVALID, "ddif_q2n: scale=%g must be finite and > 0", (double)scale);
    const int ny = (H + shift - 1) / shift, nx = (W + shift - 1) / shift;
    const long long nblk = (long long)ny * nx;
    if (nblk * B > 0x7fffffffLL) return ddif::fail(DDIF_ERR_INVALID, "ddif_q2n: B=%d H=%d W=%d shift=%d: more than 2^31 blocks", B, H, W, shift);
    double* map = map_out;
    if (!map)
        if (int e = ddif::metric_scratch((size_t)(nblk * B), &map)) return e;
    hipStream_t s = (hipStream_t)stream;
    const unsigned nwg = (unsigned)(nblk * B);
    if (C == 1) ddif::q2n_launch<1>(s, nwg, gt, pred, C, H, W, scale, block, shift, nx, ny, map);
    else if (C == 2) ddif::q2n_launch<2>(s, nwg, gt, pred, C, H, W, scale, block, shift, nx, ny, map);
    else if (C <= 4) ddif::q2n_launch<4>(s, nwg, gt, pred, C, H, W, scale, block, shift, nx, ny, map);
    else ddif::q2n_launch<8>(s, nwg, gt, pred, C, H, W, scale, block, shift, nx, ny, map);
    hipLaunchKernelGGL(ddif::q2n_mean_kernel, dim3((unsigned)B), dim3(256), 64, s, (const double*)map, (int)nblk, q_out);
    DDIF_HIPCHK(hipGetLastError());
    return DDIF_OK;
}

}  // extern "C"
