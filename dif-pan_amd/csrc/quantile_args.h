// Launch arguments of the per-sample quantile of |.| (kernels_quantile.h, ddif_quantile.cpp); shared with the plan and the C ABI.
#pragma once
#include "sampler_dev.h"

namespace ddif {

// What the kernel ranks: the value the step kernels threshold, recomputed on the fly from what the step already has, in their operand order.
enum { QUANT_RAW = 0,    // v = a[i]                                                      (ddif_dynamic_threshold)
       QUANT_DDPM = 1,   // v = x0 + lms[i], x0 = a[i] or pred_x0(tab6[k], xt[i], tab7[k], a[i])  (ddpm_step_kernel; diffusion_ddpm_pan.py:391-399)
       QUANT_DPM = 2 };  // v = x0 of dpm_x0_kernel's model_type branch                   (solver/dpm_solver.py:441-450)

struct QuantArgs {
    const float* a;    // [B][n]: raw values / the network output (NHWC: a sample is n contiguous values in every layout)
    const float* xt;   // [B][n] x_t (QUANT_DDPM with pred, QUANT_DPM)
    const float* lms;  // [B][n] (QUANT_DDPM)
    long long n;       // values per sample
    int form, pred;    // pred: QUANT_DDPM 0 x_start / 1 noise or v; QUANT_DPM the model_type (0 x_start, 1 noise, 2 v)
    const SamplerRun* run;  // QUANT_DDPM with pred: tab[6] / tab[7] at *step
    const int* step;
    float alpha, sigma;     // QUANT_DPM
    // QUANT_DPM under classifier-free guidance (solver/dpm_solver.py:334-338): a = the unconditional half of the network output, a2 = the conditional half
    // ([B][n] each, B guided samples); x0 comes from eps = eps_u + gscale * (eps_c - eps_u).  a2 == nullptr: no guidance.
    const float* a2;
    float gscale;
    // torch.quantile(.., p) (linear): rank r = fp32(p) * fp32(n - 1), order statistics floor(r) and ceil(r), weight r - floor(r)
    long long k_lo, k_hi;
    float w, max_val;
    float* s_out;      // [B]: max(quantile, max_val)
    float* stat_out;   // nullable [B][2]: the two order statistics themselves (tests)
};

// rank and weight as ATen evaluates them for fp32 input (one fp32 product, floor / ceil of it, one fp32 difference)
void quantile_rank(float ratio, long long n, long long* k_lo, long long* k_hi, float* w);
int quantile_prepare();
// one workgroup per sample; n <= QUANT_RESIDENT_MAX keeps the keys in LDS (one pass over memory), larger samples stream every pass
enum { QUANT_RESIDENT_MAX = 32768 };
void quantile_launch(const QuantArgs& a, int B, hipStream_t s);
// out[i] = clamp(x[i], symmetric ? -s[b] : 0, s[b]) / s[b]
void threshold_apply_launch(const float* x, const float* s_dev, int B, long long n, int symmetric, float* out, hipStream_t s);

}  // namespace ddif
