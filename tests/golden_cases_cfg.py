"""Seeded cases of classifier-free guidance in DPM-Solver runs (model_wrapper with guidance_scale != 1 and an unconditional_condition; reference
solver/dpm_solver.py:330-338), in the style of golden_cases_dpmx.py: only seeds, shapes and keywords.  tools/make_golden.py --only cfg runs the real reference
on them in fp32 (the expected output) and in its fp64 twin (`out_f64`, `gap`; refused above a tenth of the tolerance), and stores the fp32 time of every
evaluation (`eval_t`) and, as a record that the golden tells a guided run from an unguided one, `guided_minus_unguided` = max|out - out at scale 1|.

B = 1 and model_type="noise" only: with "x_start" or "v" the reference's guided branch multiplies a (2,)-shaped alpha_t into a (2, C, H, W) tensor and raises
a broadcast RuntimeError at any W != 2.  cond = golden_cases.tiles_for(ds, 1, H, H, seed)["cond"]; the unconditional condition is zeros_like(cond) with the
first C (lms) channels kept (`unconditional_of`): the image-space clamp is the conditional sample's, and a network input without PAN detail is what a
condition-dropout training would show the network.  Random-init weights, x_T from torch.Generator().manual_seed(seed).

Tried and NOT qualifying (gap / tolerance of the reference alone): singlestep order 3, 12 steps, scale 3.0 (0.24); gf2 32 x 32 singlestep_fixed order 2,
9 steps, scale 0.5 (73)."""
from __future__ import annotations

import golden_cases_dpmx as gx

PP, NP, WV3 = gx.PP, gx.NP, gx.WV3


def _case(cid, scale, *a, **k):
    return dict(gx._case(cid, *a, **k), scale=float(scale))


CASES = [
    # the plain multistep DPM-Solver++ arguments: unguided they take ddif_plan_sample_dpmpp, guided the solver program
    _case("cfg_pp_ms_o3_s12_clamp_g1p5", 1.5, WV3, "cosine", PP, "multistep", 3, 12, "noise", "clamp"),
    _case("cfg_pp_ms_o2_s10_taylor_dyn_g2", 2.0, WV3, "cosine", PP, "multistep", 2, 10, "noise", "dyn", solver_type="taylor"),
    _case("cfg_np_ss_o3_s12_d2z_linear_g1p5", 1.5, WV3, "linear", NP, "singlestep", 3, 12, "noise", None, denoise_to_zero=True),
]
BY_ID = {c["cid"]: c for c in CASES}


def unconditional_of(cond, C):
    """zeros_like(cond) with the first C (lms) channels kept."""
    u = cond.clone()
    u[:, C:] = 0
    return u
