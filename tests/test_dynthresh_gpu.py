"""Dynamic thresholding on the gfx950 library: the selection kernel (csrc/kernels_quantile.h) against torch.sort and torch.quantile at every size of
tests/dynthresh_checks.py -- both the LDS-resident and the streaming path -- every golden of tests/golden_cases_dynthresh.py (the real reference, fp32,
with its fp64 twin and its quantiles on file) through the drop-in classes, the batch / alone equality, the resident path inside a captured step pair at the
benchmark tile size, and the switch's contract: mode 0 is today's program, bit for bit.  The checks live in tests/dynthresh_checks.py, shared with
tests/test_dynthresh_emu.py.  On a tree without the feature the symbols do not exist and the drop-in raises DdifError."""
import pytest
import torch

import dynthresh_checks as K
import golden_cases as gc
import golden_cases_dynthresh as gd
from ddif_testlib import use_gpu_library

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gpu_library()


@pytest.mark.parametrize("n", K.SIZES)
def test_quantile_and_threshold_match_torch(_lib, n):
    K.run_op(_lib, n, DEV)


@pytest.mark.parametrize("case", gd.DDPM_CASES, ids=lambda c: c[0])
def test_ddpm_matches_reference_golden(case):
    K.run_ddpm(case, DEV)


@pytest.mark.parametrize("case", gd.DPM_CASES, ids=lambda c: c[0])
def test_dpm_solver_matches_reference_golden(case):
    K.run_dpm(case, DEV)


def test_batch_equals_tiles_alone():
    K.run_batch_equals_tiles(gd.DDPM_CASES[0], DEV)


def test_mode0_is_bit_identical():
    K.run_mode0_is_bit_identical(DEV)


def test_set_threshold_rejects_bad_arguments():
    K.run_set_threshold_rejects(DEV)


def test_dynamic_thresholding_fn_of_both_classes():
    K.run_front_door_methods(DEV)


@pytest.mark.parametrize("pm", ["x_start", "noise"])
def test_resident_quantile_inside_a_captured_step_pair_at_64x64(pm):
    """One 64 x 64 WV3 tile (32 768 values per sample: the last LDS-resident size), 4 steps with supplied noise -- enough for the loop to capture and replay its
    step pair -- against the same steps with the thresholding done by torch on the plan's raw network output, the reference's expressions in the reference's
    order (:327-344, :391-399, :418-442).  Both sides round the same fp32 expressions, so the bar is the forward's 2e-5.  With the switch off the plan is the
    benchmark's: 132 launches per step, and the dynamic run does not change that program.
    The quantile must MATTER in every step, or s = max_val and a wrong selection would go unnoticed: with "noise" it lies far above the reference's
    max_val = 1; with "x_start" on these weights |x0 + lms| has its 0.8 quantile near 0.8, so that parametrisation sets thresholding_max_val = 0.5 (the
    attribute is read at call time).  Asserted on the torch side, per step."""
    ds, B, H, T, steps = "wv3", 1, 64, 50, 4
    C = gc.DATASETS[ds][0]
    cond = gc.tiles_for(ds, B, H, H, seed=5)["cond"].to(DEV)
    d = K.diffusion(ds, T, H, DEV, pm)
    max_val = 1.0 if pm == "noise" else 0.5
    d.thresholding_max_val = max_val
    gen = torch.Generator().manual_seed(5)
    xT = torch.randn(B, C, H, H, generator=gen).to(DEV)
    noise = torch.randn(steps, B, C, H, H, generator=gen).to(DEV)
    plan = d._plan(cond)
    assert plan.get_threshold() == ("ddpm", K.np.float32(0.8), max_val)
    assert plan.num_launches()["step"] == 132
    order = list(reversed(range(T)))[:steps]
    c1, c2 = d.posterior_mean_coef1, d.posterior_mean_coef2
    cz = (0.5 * d.posterior_log_variance_clipped).exp()
    out = plan.sample_ddpm([float(i) for i in order], [float(c1[i]) for i in order], [float(c2[i]) for i in order], [float(cz[i]) for i in order], xT, noise,
                           0, 0, (0.0, 1.0), DEV, pred=d._pred_tables(order))
    img, lms = xT, cond[:, :C]
    dd = K.diffusion(ds, T, H, DEV, pm, clamp_type="abs")  # the raw network output comes from a plan with the switch off (the module forward states nothing)
    active = 0
    for k, i in enumerate(order):
        t = torch.full((B,), i, device=DEV, dtype=torch.long)
        o = dd.model(img, t, cond, img)
        x0 = o if pm == "x_start" else dd.predict_start_from_noise(img, t, o)
        v = (x0 + lms).cpu()
        active += int(float(torch.quantile(v.abs().reshape(B, -1), 0.8, dim=1).min()) > max_val)
        x0 = K.threshold_torch(v, 0.8, max_val, symmetric=False).to(DEV) - lms
        img = c1[i] * x0 + c2[i] * img + cz[i] * noise[k]
    err = float((out - img).abs().max())
    print(f"dynamic DDPM {pm} at 64x64: max|library - torch| {err:.3e}, quantile above max_val in {active} of {steps} steps")
    assert active == steps, (pm, active)
    assert bool(torch.isfinite(out).all())
    assert err <= 2e-5
    plan.set_threshold("off")
    assert plan.num_launches()["step"] == 132
