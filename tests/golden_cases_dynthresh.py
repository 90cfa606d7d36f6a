"""Seeded cases of dynamic thresholding (GaussianDiffusion clamp_type="dynamic", DPM_Solver correcting_x0_fn="dynamic_thresholding"), in the style of
golden_cases_objective.py: only seeds, shapes and keywords.  tools/make_golden.py --only dynthresh runs the real reference on them, in fp32 (the expected
output) and in fp64 (the case's own noise floor: `out_f64`, `gap`), and stores the reference's quantile per (step, sample) -- taken by wrapping its
dynamic_thresholding_fn -- as `quant`, so a test can check that a fixture exercises what it claims."""
from __future__ import annotations

# (case id, dataset, B, H, W, T, pred_mode, seed, expect_active)
# GaussianDiffusion's own attributes stay at the reference's values: dynamic_thresholding_ratio 0.8, thresholding_max_val 1.0.
#   wv3 16 x 16 noise: the quantile is above max_val in 38 of 40 (step, sample) pairs (counted on the stored `quant`: 577.8 down to 0.975, two below 1), from ~577 at the first step down to ~1; rank 0.8 * 2047 = 1637.6 (fractional)
#   gf2 32 x 32 x_start: 1.036 .. 1.060 in all 20 steps; rank 0.8 * 4095 = 3276 (integral: both order statistics coincide)
#   wv3 16 x 16 x_start: 0.76 .. 0.81, never above 1 -- every step takes the max_val branch (clamp(v, 0, 1) / 1)
DDPM_CASES = [
    ("dyn_ddpm_wv3_16_T20_noise", "wv3", 2, 16, 16, 20, "noise", 111, True),
    ("dyn_ddpm_gf2_32_T20_x_start", "gf2", 1, 32, 32, 20, "x_start", 113, True),
    ("dyn_ddpm_wv3_16_T20_x_start", "wv3", 2, 16, 16, 20, "x_start", 111, False),
]

# (case id, dataset, H, W, T, steps, order, model_type, seed, DPM_Solver keywords)   B = 1 (SURVEY D-8); shapes of golden_cases_objective.DPM_CASES
# The keywords are chosen so that the quantile exceeds thresholding_max_val in at least half of the evaluations: with x_start on the random-init weights of
# the fixtures |x0| stays well below 1 (x0 is the residual to the up-sampled LMS), so the default max_val = 1 would never let the quantile through.
DPM_CASES = [
    ("dyn_dpm_gf2_32_T1000_s10_o2_noise", "gf2", 32, 32, 1000, 10, 2, "noise", 131, dict(thresholding_max_val=1.0, dynamic_thresholding_ratio=0.995)),
    ("dyn_dpm_gf2_32_T1000_s10_o2_x_start", "gf2", 32, 32, 1000, 10, 2, "x_start", 131, dict(thresholding_max_val=0.05, dynamic_thresholding_ratio=0.995)),
    ("dyn_dpm_wv3_16_T500_s12_o3_noise", "wv3", 16, 16, 500, 12, 3, "noise", 133, dict(thresholding_max_val=1.0, dynamic_thresholding_ratio=0.995)),
    ("dyn_dpm_wv3_16_T500_s12_o3_x_start", "wv3", 16, 16, 500, 12, 3, "x_start", 133, dict(thresholding_max_val=0.05, dynamic_thresholding_ratio=0.9)),
]
PRED_OF_MODEL_TYPE = {"noise": "noise", "x_start": "x_start"}  # GaussianDiffusion's name of model_wrapper's model_type (only the net and the schedule are taken from it)


# Schedule of the DPM-Solver++ cases by model_type.  "noise" keeps the engine's cosine schedule (the first x0 = (x - sigma * eps) / alpha_T is ~6e4 and
# thresholding scales it back to [-1, 1]: the reference's fp32 <-> fp64 gap is ~1e-6).  With "x_start" the round trip eps = (x - alpha * o) / sigma,
# x0 = (x - sigma * eps) / alpha cancels to rounding noise that 1 / alpha_T (alpha_T ~ 5e-5 on the cosine schedule) amplifies, and nothing saturates behind it:
# there the reference ALONE differs from its fp64 self by 7e-5 .. 2e-4, 0.4 .. 0.7 of the tolerance, so those cases take the linear schedule of DDPM
# (1e-4 .. 2e-2 at T = 1000, scaled by 1000 / T; alpha_T ~ 6e-3), as golden_cases_objective.dpm_schedule does for "v".
def dpm_schedule(model_type: str, T: int) -> dict:
    """Keyword arguments of make_beta_schedule (the reference's and the drop-in's take the same)."""
    if model_type == "x_start":
        return dict(schedule="linear", n_timestep=T, linear_start=1e-4 * 1000 / T, linear_end=2e-2 * 1000 / T)
    return dict(schedule="cosine", n_timestep=T, cosine_s=8e-3)


def active_fraction(quant, max_val: float) -> float:
    """Share of the (step, sample) pairs whose quantile exceeds max_val, i.e. where thresholding rescales at all."""
    import numpy as np

    q = np.asarray(quant, dtype=np.float64).reshape(-1)
    return float((q > max_val).mean())
