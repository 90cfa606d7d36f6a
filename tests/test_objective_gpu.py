"""pred_mode "noise" / "pred_v", loss "l2" and p2 weighting on the gfx950 library, through the ctypes C ABI and the drop-in classes: every golden of
tests/golden_cases_objective.py (the real reference, fp32, with its fp64 twin on file), the bit-equality of an explicitly default objective and the
refusal of the plain entry points.  The checks live in tests/objective_parity.py, shared with tests/test_objective_emu.py.  On a tree without the
feature the drop-in raises DdifError for every one of these configurations."""
import pytest
import torch

import golden_cases_objective as go
import objective_parity as P
from ddif_testlib import use_gpu_library

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gpu_library()


@pytest.mark.parametrize("pm", go.PRED_MODES)
@pytest.mark.parametrize("case", go.DDPM_CASES, ids=lambda c: c[0])
def test_ddpm_matches_reference_golden(case, pm):
    P.run_ddpm(case, pm, DEV)


@pytest.mark.parametrize("pm", go.PRED_MODES)
@pytest.mark.parametrize("case", go.DDIM_CASES, ids=lambda c: c[0])
def test_ddim_matches_reference_golden(case, pm):
    P.run_ddim(case, pm, DEV)


@pytest.mark.parametrize("pm", go.PRED_MODES)
@pytest.mark.parametrize("case", go.DPM_CASES, ids=lambda c: c[0])
def test_dpm_solver_matches_reference_golden(case, pm):
    P.run_dpm(case, pm, DEV)


@pytest.mark.parametrize("pm", go.PRED_MODES)
@pytest.mark.parametrize("case", go.LOSS_CASES, ids=lambda c: c[0])
def test_p_losses_matches_reference_golden(case, pm, monkeypatch):
    P.run_loss(case, pm, DEV, monkeypatch)


@pytest.mark.parametrize("case", go.GRAD_CASES, ids=lambda c: c[0])
def test_p_losses_backward_matches_reference_golden(case, monkeypatch):
    P.run_grad(case, DEV, monkeypatch)


def test_explicit_default_objective_is_bit_identical():
    P.run_default_objective_is_bit_identical(DEV)


@pytest.mark.parametrize("kind,pm", [("ddpm", "noise"), ("ddpm", "pred_v"), ("ddim", "noise"), ("ddim", "pred_v")])
def test_sampler_epilogue_serves_a_prediction_objective_at_64x64(kind, pm):
    """At the benchmark tile size the update runs in the final conv's epilogue (132 launches per step): both branches of the prediction instantiation
    (DDPM and DDIM update behind the conversion) for both parameterisations, against the same steps with the epilogue's work done by torch on the raw
    network output -- the reference's expressions in the reference's order (:298-314, :418-442, :594-621).  Both sides round the same fp32 expressions, so
    the bar is the forward's 2e-5, relative to max(1, max|x|) for the unclamped DDIM iterates."""
    import golden_cases as gc

    ds, B, H, T, steps = "wv3", 1, 64, 50, 3
    C = gc.DATASETS[ds][0]
    cond = gc.tiles_for(ds, B, H, H, seed=5)["cond"].to(DEV)
    d = P.diffusion(ds, T, H, DEV, pm)
    gen = torch.Generator().manual_seed(5)
    xT = torch.randn(B, C, H, H, generator=gen).to(DEV)
    noise = torch.randn(steps, B, C, H, H, generator=gen).to(DEV)
    plan = d._plan(cond)
    assert plan.num_launches()["step"] == 132
    order = list(reversed(range(T)))[:steps]
    tm = [float(i) for i in order]
    to_x0 = d.predict_start_from_noise if pm == "noise" else d.predict_start_from_v
    img, lms = xT, cond[:, :C]
    if kind == "ddpm":
        c1, c2 = d.posterior_mean_coef1, d.posterior_mean_coef2
        cz = (0.5 * d.posterior_log_variance_clipped).exp()
        out = plan.sample_ddpm(tm, [float(c1[i]) for i in order], [float(c2[i]) for i in order], [float(cz[i]) for i in order], xT, noise,
                               0, 0, (0.0, 1.0), DEV, pred=d._pred_tables(order))
        for k, i in enumerate(order):
            t = torch.full((B,), i, device=DEV, dtype=torch.long)
            x0 = to_x0(img, t, d.model(img, t, cond, img))
            x0 = (x0 + lms).clamp(0, 1) - lms
            img = c1[i] * x0 + c2[i] * img + cz[i] * noise[k]
    else:
        sr, srm1 = d.sqrt_recip_alphas_cumprod, d.sqrt_recipm1_alphas_cumprod
        sqrt_ap = torch.sqrt(d.alphas_cumprod_prev)
        dirc = torch.sqrt(1 - d.alphas_cumprod_prev)  # eta = 0
        out = plan.sample_ddim(tm, [float(sr[i]) for i in order], [float(srm1[i]) for i in order], [float(sqrt_ap[i]) for i in order],
                               [float(dirc[i]) for i in order], [0.0] * steps, xT, None, 0, 0, None, DEV, pred=d._pred_tables(order))
        for i in order:
            t = torch.full((B,), i, device=DEV, dtype=torch.long)
            x0 = to_x0(img, t, d.model(img, t, cond, img))
            eps = (sr[i] * img - x0) / srm1[i]
            img = x0 * sqrt_ap[i] + dirc[i] * eps
    err, scale = float((out - img).abs().max()), max(1.0, float(img.abs().max()))
    print(f"{kind} {pm} at 64x64: max|epilogue - torch| {err:.3e}, max|x| {float(img.abs().max()):.3g}")
    assert bool(torch.isfinite(out).all())
    assert err <= 2e-5 * (scale if kind == "ddim" else 1.0)


def test_plain_entry_points_refuse_a_prediction_objective():
    P.run_plain_entry_points_refuse_a_prediction_objective(DEV)
