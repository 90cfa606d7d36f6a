// Host side of the HybridL1SSIM loss (kernels_ssimloss.h): the three-launch tail the training plan takes under DDIF_LOSS_L1SSIM (tk::ssimloss_tail) and the
// stateless entry point of include/ddif.h (ddif_l1ssim_loss), which runs the same launches on plain tensors.
#include <cmath>
#include "ddif_plan.h"
#include "kernels_ssimloss.h"

namespace ddif {
namespace tk {

// gaussian(11, 1.5) / create_window (utils/loss_utils.py:11-27): the values in Python doubles, stored as fp32, divided by their fp32 sum.  (The reference's
// 2-D window is the fp32 outer product of this vector with itself; the kernels apply the vector along rows, then along columns.)
static void ssim_window(float* w) {
    float sum = 0.f;
    for (int k = 0; k < SSIM_K; ++k) {
        const double d = (double)(k - SSIM_K / 2);
        w[k] = (float)std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
        sum += w[k];
    }
    for (int k = 0; k < SSIM_K; ++k) w[k] = w[k] / sum;
}

static int ssim_tiles(int v) { return (v + SSIM_T - 1) / SSIM_T; }

size_t ssimloss_workgroups(int B, int C, int H, int W) { return (size_t)ssim_tiles(H) * ssim_tiles(W) * ((C + SSIM_CG - 1) / SSIM_CG) * B; }

int ssimloss_check(const char* who, int B, int C, int H, int W) {
    if (B < 1 || C < 1 || H < 1 || W < 1) return fail(DDIF_ERR_INVALID, "%s: B=%d C=%d H=%d W=%d (all >= 1)", who, B, C, H, W);
    if (B > 65535 || (C + SSIM_CG - 1) / SSIM_CG > 65535) return fail(DDIF_ERR_INVALID, "%s: B=%d C=%d exceed the launch grid (B <= 65535, C <= 262140)", who, B, C);
    if (ssimloss_workgroups(B, C, H, W) > 0x7fffffffULL || (long long)ssim_tiles(H) * ssim_tiles(W) > 0x7fffffffLL)
        return fail(DDIF_ERR_INVALID, "%s: B=%d C=%d H=%d W=%d: more than 2^31 tiles", who, B, C, H, W);
    return 0;
}

void ssimloss_tail(hipStream_t s, const float* img1, const float* img2, int B, int C, int H, int W, bool nhwc, float w_l1, float w_ssim, float upstream, const float* p2w,
                   float* maps, double* part, float* d_loss, float* d_img2) {
    SsimArgs a{};
    a.x = img1;
    a.y = img2;
    a.B = B, a.C = C, a.H = H, a.W = W;
    a.sb = (long long)C * H * W;
    if (nhwc) a.sc = 1, a.sw = C, a.sh = (long long)W * C;
    else a.sw = 1, a.sh = W, a.sc = (long long)H * W;
    a.n = (long long)B * a.sb;
    a.tiles_x = ssim_tiles(W);
    ssim_window(a.w);
    a.maps = d_img2 ? maps : nullptr;
    a.part = part;
    a.w_l1 = w_l1, a.w_ssim = w_ssim, a.upstream = upstream;
    a.scale = d_loss;
    a.dy = d_img2;
    const dim3 grid((unsigned)(ssim_tiles(H) * ssim_tiles(W)), (unsigned)((C + SSIM_CG - 1) / SSIM_CG), (unsigned)B);
    const int nwg = (int)ssimloss_workgroups(B, C, H, W);
    if (nhwc) hipLaunchKernelGGL(ssim_stats_kernel<true>, grid, dim3(256), ssim_stats_smem(), s, a);
    else hipLaunchKernelGGL(ssim_stats_kernel<false>, grid, dim3(256), ssim_stats_smem(), s, a);
    hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(256), (size_t)SSIM_FCH * 2 * sizeof(double), s, (const double*)part, nwg, a.n, w_l1, w_ssim, p2w, B, d_loss);
    if (!d_img2) return;
    if (nhwc) hipLaunchKernelGGL(ssim_grad_kernel<true>, grid, dim3(256), ssim_grad_smem(), s, a);
    else hipLaunchKernelGGL(ssim_grad_kernel<false>, grid, dim3(256), ssim_grad_smem(), s, a);
}

}  // namespace tk
}  // namespace ddif

extern "C" {

int ddif_l1ssim_loss(const float* img1, const float* img2, int B, int C, int H, int W, int nhwc, float w_l1, float w_ssim, float upstream, float* loss_out, float* d_img2,
                     void* stream) {
    using namespace ddif;
    hipStream_t s = (hipStream_t)stream;
    if (!img1 || !img2 || !loss_out) return fail(DDIF_ERR_INVALID, "ddif_l1ssim_loss: NULL argument");
    if (int e = tk::ssimloss_check("ddif_l1ssim_loss", B, C, H, W)) return e;
    // scratch of this call: [partials | the two loss floats | the three maps] in one allocation (not a hot path: the training step uses the plan's own)
    const size_t n = (size_t)B * C * H * W, nwg = tk::ssimloss_workgroups(B, C, H, W);
    const size_t part_bytes = nwg * 2 * sizeof(double), head = part_bytes + 64;
    char* buf = nullptr;
    DDIF_HIPCHK(hipMalloc((void**)&buf, head + (d_img2 ? 3 * n * sizeof(float) : 0)));
    float* d_loss = reinterpret_cast<float*>(buf + part_bytes);
    tk::ssimloss_tail(s, img1, img2, B, C, H, W, nhwc != 0, w_l1, w_ssim, upstream, nullptr, reinterpret_cast<float*>(buf + head), reinterpret_cast<double*>(buf), d_loss, d_img2);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(loss_out, d_loss, sizeof(float), hipMemcpyDefault, s);
    const hipError_t e2 = hipStreamSynchronize(s);  // the scratch goes away below
    (void)hipFree(buf);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(DDIF_ERR_HIP, "ddif_l1ssim_loss: %s", hipGetErrorString(e));
    return DDIF_OK;
}

}
