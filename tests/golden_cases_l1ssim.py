"""Seeded cases of loss_type="l1ssim" (the reference's HybridL1SSIM, utils/loss_utils.py:73-83), in the style of golden_cases_objective.py: only seeds and
shapes.  tools/make_golden.py --only l1ssim runs the real reference on them, in fp32 (the expected value) and in fp64 (the case's own noise floor, stored next to
it as `<key>_f64` and `gap::<key>`)."""
from __future__ import annotations

import golden_cases as gc

WEIGHTS = (1.0, 0.1)  # HybridL1SSIM's default weighted_r, what GaussianDiffusion.set_loss builds (:194-195)

# The operator alone on x = sx * randn, y = x + sn * randn (img1 = x, img2 = y), one generator seeded with `seed`, x drawn first.
# (case id, B, C, H, W, sx, sn, seed)
OP_CASES = [
    ("l1ssim_op_residual", 2, 8, 16, 16, 0.05, 0.02, 301),  # residual-like: what pred_mode x_start compares
    ("l1ssim_op_noise", 2, 8, 16, 16, 1.0, 0.5, 302),       # noise-like
    ("l1ssim_op_v", 2, 8, 16, 16, 0.7, 0.7, 303),           # v-like
    ("l1ssim_op_tiles", 1, 4, 32, 32, 1.0, 0.5, 304),       # more than one tile per image
    ("l1ssim_op_cave", 2, 31, 13, 19, 1.0, 0.5, 305),       # CAVE's channel count (no multiple of the channel group), odd sizes
    ("l1ssim_op_thin", 1, 3, 5, 37, 1.0, 0.5, 306),         # shorter than the window radius in one axis, three tiles in the other
    ("l1ssim_op_one", 1, 1, 1, 1, 1.0, 0.5, 307),           # degenerate
]


def op_inputs(case):
    import torch

    _, B, C, H, W, sx, sn, seed = case
    g = torch.Generator().manual_seed(seed)
    x = sx * torch.randn(B, C, H, W, generator=g)
    y = x + sn * torch.randn(B, C, H, W, generator=g)
    return x, y


PRED_MODES = ("x_start", "noise", "pred_v")
P2_GAMMAS = (0.0, 0.5)

# p_losses in eval mode, pinned t as golden_cases_objective.LOSS_CASES: one file per (pred_mode, self-cond branch) holding loss / recon for gamma 0, 0.5
# (stem, dataset, B, H, W, T, t values, self-cond branch, seed)
LOSS_CASES = [
    ("l1ssim_loss_wv3_16_sc0", "wv3", 2, 16, 16, 500, [3, 250], False, 311),
    ("l1ssim_loss_wv3_16_sc1", "wv3", 2, 16, 16, 500, [100, 7], True, 312),
]


def loss_key(gamma: float) -> str:
    return f"l1ssim_g{int(round(gamma * 10)):02d}"


# the reference's own p_losses(...).backward() under .train(), masks captured as gc.TRAIN_GRAD_CASES does (self-conditioning branch not taken)
# (case id, dataset, B, H, W, T, t values, pred_mode, p2 gamma, seed)
GRAD_CASES = [
    ("l1ssim_grad_wv3_16_x_start", "wv3", 2, 16, 16, 500, [7, 431], "x_start", 0.0, 321),
    ("l1ssim_grad_gf2_32_noise_p2", "gf2", 1, 32, 32, 500, [120], "noise", 0.5, 322),  # 32 x 32: the loss tail crosses tile borders inside the training step
]
TRAIN_GRAD_FULL = gc.TRAIN_GRAD_FULL
