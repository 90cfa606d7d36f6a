"""Seeded cases of the noise / v parameterisations (GaussianDiffusion pred_mode "noise" / "pred_v", model_wrapper model_type "noise" / "v"),
in the style of golden_cases.py: only seeds and shapes.  tools/make_golden.py --only objective runs the real reference on them, in fp32
(the expected output) and in fp64 (the case's own noise floor, stored next to it as `<key>_f64` and `gap::<key>`)."""
from __future__ import annotations

import golden_cases as gc

PRED_MODES = ("noise", "pred_v")
MODEL_TYPE = {"noise": "noise", "pred_v": "v"}  # solver/dpm_solver.py model_wrapper's name of the same parameterisation

# (case id stem, dataset, B, H, W, T, seed); one golden per pred_mode: f"{stem}_{pred_mode}"
DDPM_CASES = [
    ("obj_ddpm_wv3_16_T20", "wv3", 2, 16, 16, 20, 111),
    ("obj_ddpm_wv3_16_T100", "wv3", 2, 16, 16, 100, 112),
    ("obj_ddpm_gf2_32_T50", "gf2", 1, 32, 32, 50, 113),
]
# (stem, dataset, B, H, W, T, section_counts, seed)
DDIM_CASES = [
    ("obj_ddim_wv3_16_T500_25", "wv3", 2, 16, 16, 500, "ddim25", 121),
]
# (stem, dataset, H, W, T, steps, order, seed)   B = 1 (SURVEY D-8)
DPM_CASES = [
    ("obj_dpm_gf2_32_T1000_s10_o2", "gf2", 32, 32, 1000, 10, 2, 131),
    ("obj_dpm_wv3_16_T500_s12_o3", "wv3", 16, 16, 500, 12, 3, 133),
]
# Schedule of the DPM-Solver++ cases by parameterisation.  The run starts at t = T, where data_prediction_fn divides by alpha_T (x0 = (x - sigma * eps) / alpha).
# "noise" keeps the engine's cosine schedule (alpha_T ~ 5e-5: the first x0 saturates in the clamp corrector and the reference's fp32 <-> fp64 gap is ~1e-6).
# With "v", eps = alpha * o + sigma * x makes the numerator cancel to rounding noise that 1 / alpha_T amplifies: on the cosine schedule the reference ALONE differs
# from its fp64 self by 4e-4 .. 5e-4, four times the 1e-4 bar, so those cases take the linear schedule of DDPM (1e-4 .. 2e-2 at T = 1000, scaled by 1000 / T;
# alpha_T ~ 6e-3), where the gap is 1e-6 .. 5e-6.  Keyword arguments of make_beta_schedule (the reference's and the drop-in's take the same).
def dpm_schedule(pred_mode: str, T: int) -> dict:
    if pred_mode == "pred_v":
        return dict(schedule="linear", n_timestep=T, linear_start=1e-4 * 1000 / T, linear_end=2e-2 * 1000 / T)
    return dict(schedule="cosine", n_timestep=T, cosine_s=8e-3)


# p_losses in eval mode, pinned t as gc.LOSS_CASES: one file per (pred_mode, self-cond branch) holding loss / recon for l1, l2 x gamma 0, 0.5
# (stem, dataset, B, H, W, T, t values, self-cond branch, seed)
LOSS_CASES = [
    ("obj_loss_wv3_16_sc0", "wv3", 2, 16, 16, 500, [3, 250], False, 141),
    ("obj_loss_wv3_16_sc1", "wv3", 2, 16, 16, 500, [100, 7], True, 142),
]
LOSS_TYPES = ("l1", "l2")
P2_GAMMAS = (0.0, 0.5)


def loss_key(loss_type: str, gamma: float) -> str:
    return f"{loss_type}_g{int(round(gamma * 10)):02d}"


# the reference's own p_losses(...).backward() under .train(), masks captured as gc.TRAIN_GRAD_CASES does (self-conditioning branch not taken)
# (case id, dataset, B, H, W, T, t values, pred_mode, loss_type, p2 gamma, seed)
GRAD_CASES = [
    ("obj_grad_wv3_16_noise_l2", "wv3", 2, 16, 16, 500, [7, 431], "noise", "l2", 0.0, 162),
    ("obj_grad_wv3_16_pred_v_l1_p2", "wv3", 2, 16, 16, 500, [7, 431], "pred_v", "l1", 0.5, 163),
]
TRAIN_GRAD_FULL = gc.TRAIN_GRAD_FULL
