"""Seeded cases of the DPM-Solver runs beyond the plain multistep DPM-Solver++ one: singlestep / singlestep_fixed, solver_type="taylor",
algorithm_type="dpmsolver" (noise-prediction updates), denoise_to_zero and return_intermediate -- in the style of golden_cases_dynthresh.py: only seeds, shapes
and keywords.  tools/make_golden.py --only dpmx runs the real reference on them, in fp32 (the expected output) and in fp64 (the case's own noise floor:
`out_f64`, `gap`; the schedule scalars stay in the solver's fp32 in both), and stores, taken by wrapping the solver's `model`, the fp32 time of every evaluation
in execution order (`eval_t`) next to `orders` and `timesteps_outer` (singlestep) or `timesteps` (multistep); one case also stores the `inter` stack of a
return_intermediate=True run.

B = 1 (SURVEY D-8), cond = golden_cases.tiles_for(ds, 1, H, H, seed)["cond"], x_T from torch.Generator().manual_seed(seed), random-init weights.
"clamp" is the image-space clamp corrector (x0 + lms).clamp(0, 1) - lms; "dyn" correcting_x0_fn="dynamic_thresholding" with the reference's defaults.

algorithm_type="dpmsolver" runs on the LINEAR schedule only: on the cosine schedule alpha_T ~ 5e-5 and nothing saturates behind 1 / alpha_T (no corrector
applies to a noise prediction), so the reference alone differs from its fp64 self by up to 138 times the tolerance there (measured: noise max|golden| ~ 4e4;
x_start taylor order 3)."""
from __future__ import annotations

WV3 = ("wv3", 16, 500, 133)  # dataset, H = W, T, seed
GF2 = ("gf2", 32, 1000, 131)


def _case(cid, where, schedule, algorithm, method, order, steps, model_type, corrector, solver_type="dpmsolver", skip_type="time_uniform", denoise_to_zero=False,
          inter=False):
    ds, H, T, seed = where
    return dict(cid=cid, ds=ds, H=H, T=T, seed=seed, schedule=schedule, algorithm=algorithm, method=method, order=order, steps=steps, model_type=model_type,
                corrector=corrector, solver_type=solver_type, skip_type=skip_type, denoise_to_zero=denoise_to_zero, inter=inter)


PP, NP = "dpmsolver++", "dpmsolver"
CASES = [
    # ---- dpmsolver++ (cosine schedule unless the name says linear)
    _case("dpmx_pp_ss_o3_s12_noise", WV3, "cosine", PP, "singlestep", 3, 12, "noise", "clamp"),
    _case("dpmx_pp_ss_o3_s11_x_start", WV3, "cosine", PP, "singlestep", 3, 11, "x_start", "clamp", inter=True),  # orders 3, 3, 3, 2
    _case("dpmx_pp_ss_o3_s10_taylor_noise_logsnr", WV3, "cosine", PP, "singlestep", 3, 10, "noise", "clamp", solver_type="taylor", skip_type="logSNR"),  # 3, 3, 3, 1
    _case("dpmx_pp_ss_o2_s9_x_start_d2z_gf2", GF2, "cosine", PP, "singlestep", 2, 9, "x_start", "clamp", denoise_to_zero=True),
    _case("dpmx_pp_ssf_o3_s12_v_linear", WV3, "linear", PP, "singlestep_fixed", 3, 12, "v", "clamp"),
    _case("dpmx_pp_ss_o3_s12_noise_dyn", WV3, "cosine", PP, "singlestep", 3, 12, "noise", "dyn"),
    _case("dpmx_pp_ms_o2_s12_taylor_noise", WV3, "cosine", PP, "multistep", 2, 12, "noise", "clamp", solver_type="taylor"),
    _case("dpmx_pp_ms_o3_s6_x_start_d2z", WV3, "cosine", PP, "multistep", 3, 6, "x_start", "clamp", denoise_to_zero=True),
    # ---- dpmsolver (linear schedule, no corrector)
    _case("dpmx_np_ss_o3_s12_noise", WV3, "linear", NP, "singlestep", 3, 12, "noise", None),
    _case("dpmx_np_ss_o3_s11_taylor_x_start", WV3, "linear", NP, "singlestep", 3, 11, "x_start", None, solver_type="taylor"),
    _case("dpmx_np_ss_o3_s10_v_logsnr", WV3, "linear", NP, "singlestep", 3, 10, "v", None, skip_type="logSNR"),
    _case("dpmx_np_ss_o2_s9_x_start_d2z_gf2", GF2, "linear", NP, "singlestep", 2, 9, "x_start", None, denoise_to_zero=True),
    _case("dpmx_np_ms_o2_s10_noise_gf2", GF2, "linear", NP, "multistep", 2, 10, "noise", None),
    _case("dpmx_np_ms_o3_s12_x_start", WV3, "linear", NP, "multistep", 3, 12, "x_start", None),
    _case("dpmx_np_ms_o2_s12_taylor_noise_tq", WV3, "linear", NP, "multistep", 2, 12, "noise", None, solver_type="taylor", skip_type="time_quadratic"),
    _case("dpmx_np_ssf_o3_s12_taylor_noise", WV3, "linear", NP, "singlestep_fixed", 3, 12, "noise", None, solver_type="taylor"),
]
BY_ID = {c["cid"]: c for c in CASES}
PRED_OF_MODEL_TYPE = {"noise": "noise", "x_start": "x_start", "v": "pred_v"}  # GaussianDiffusion's name of model_wrapper's model_type (only the net and the betas are taken from it)


def schedule_kwargs(name: str, T: int) -> dict:
    """Keyword arguments of make_beta_schedule (the reference's and the drop-in's take the same); "linear" is golden_cases_objective.dpm_schedule's."""
    if name == "linear":
        return dict(schedule="linear", n_timestep=T, linear_start=1e-4 * 1000 / T, linear_end=2e-2 * 1000 / T)
    return dict(schedule="cosine", n_timestep=T, cosine_s=8e-3)


def sample_kwargs(case: dict) -> dict:
    return dict(steps=case["steps"], order=case["order"], skip_type=case["skip_type"], method=case["method"], denoise_to_zero=case["denoise_to_zero"],
                solver_type=case["solver_type"])
