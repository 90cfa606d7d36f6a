"""The schedule of the DPM-Solver runs beyond plain multistep DPM-Solver++ -- no kernels, no library: for every golden of tests/golden_cases_dpmx.py the
drop-in's orders, outer time steps and the fp32 time of every network evaluation, on its generic path and in the solver program it builds for
ddif_plan_sample_dpm, equal what was recorded from the real reference (both sides fp32 torch on the CPU: torch.equal); and the reference's quirks and
delegations.  The checks live in tests/dpmx_checks.py.  On a tree without the feature DPM_Solver.sample raises DdifError for these arguments."""
import pytest
import torch

import dpmx_checks as K
import golden_cases_dpmx as gx


@pytest.mark.parametrize("case", gx.CASES, ids=lambda c: c["cid"])
def test_schedule_equals_the_reference(case):
    K.run_host_schedule(case)


def test_singlestep_order1_logsnr_raises_the_reference_index_error():
    """K = 1 there: two outer times for `steps` first-order updates (reference :537-547, 1229-1230)."""
    slv = K.host_solver(gx.BY_ID["dpmx_pp_ss_o3_s12_noise"])
    with pytest.raises(IndexError):
        slv.sample(torch.zeros(1, 2, 4, 4), steps=3, order=1, skip_type="logSNR", method="singlestep")
    out = slv.sample(torch.ones(1, 2, 4, 4), steps=3, order=1, skip_type="time_uniform", method="singlestep")  # the other skip types are fine
    assert bool(torch.isfinite(out).all())
    with pytest.raises(IndexError):
        K.program_of(slv, dict(gx.BY_ID["dpmx_pp_ss_o3_s12_noise"], steps=3, order=1, skip_type="logSNR"))


def test_lower_order_final_applies_to_multistep_below_ten_steps_only():
    from ddif.solver.dpm_solver import DPM_Solver

    assert DPM_Solver._multistep_orders(6, 3, True) == [1, 2, 3, 3, 2, 1]
    assert DPM_Solver._multistep_orders(6, 3, False) == [1, 2, 3, 3, 3, 3]
    assert DPM_Solver._multistep_orders(10, 3, True) == [1, 2] + [3] * 8
    slv = K.host_solver(gx.BY_ID["dpmx_pp_ss_o3_s12_noise"])
    _, rec = K.record_run(slv, torch.zeros(1, 2, 4, 4), steps=6, order=3, method="singlestep", lower_order_final=True)
    assert rec["orders"] == [3, 2, 1]  # singlestep: its own order list, whatever lower_order_final says


@pytest.mark.parametrize("method,algorithm", [("multistep", "dpmsolver++"), ("singlestep", "dpmsolver"), ("singlestep_fixed", "dpmsolver++")])
def test_inverse_is_sample_with_the_times_swapped(method, algorithm):
    case = dict(gx.BY_ID["dpmx_np_ss_o3_s12_noise"], algorithm=algorithm)
    fn = lambda x, t: 0.25 * x + t.reshape(-1, 1, 1, 1)
    x = torch.randn(2, 2, 4, 4, generator=torch.Generator().manual_seed(1))
    kw = dict(steps=6, order=3, method=method, solver_type="taylor")
    a = K.host_solver(case, fn).inverse(x, **kw)
    ns = K.host_solver(case).noise_schedule
    b = K.host_solver(case, fn).sample(x, t_start=1.0 / ns.total_N, t_end=ns.T, **kw)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    c = K.host_solver(case, fn).inverse(x, t_start=0.1, t_end=0.7, **kw)
    assert torch.equal(c, K.host_solver(case, fn).sample(x, t_start=0.1, t_end=0.7, **kw)) and not torch.equal(c, a)


def test_adaptive_is_still_refused():
    from ddif import DdifError

    slv = K.host_solver(gx.BY_ID["dpmx_pp_ss_o3_s12_noise"])
    with pytest.raises(DdifError, match="norm"):
        slv.sample(torch.zeros(1, 2, 4, 4), method="adaptive")
    with pytest.raises(ValueError):
        slv.sample(torch.zeros(1, 2, 4, 4), method="euler")


def test_add_noise_and_update_method_defaults():
    slv = K.host_solver(gx.BY_ID["dpmx_np_ss_o3_s12_noise"], lambda x, t: 0.5 * x)
    ns = slv.noise_schedule
    x = torch.randn(2, 2, 4, 4, generator=torch.Generator().manual_seed(2))
    t = torch.tensor([0.3, 0.8])
    noise = torch.randn(2, 2, 2, 4, 4, generator=torch.Generator().manual_seed(3))
    xt = slv.add_noise(x, t, noise)
    assert xt.shape == (2, 2, 2, 4, 4)
    for i in range(2):
        assert torch.equal(xt[i], ns.marginal_alpha(t[i:i + 1]) * x + ns.marginal_std(t[i:i + 1]) * noise[i])
    assert slv.add_noise(x, t[:1], noise[:1]).shape == x.shape
    s, e = torch.tensor([0.8]), torch.tensor([0.5])
    x2, im = slv.singlestep_dpm_solver_second_update(x, s, e, return_intermediate=True)  # r1 = 0.5
    assert set(im) == {"model_s", "model_s1"} and torch.equal(x2, slv.singlestep_dpm_solver_update(x, s, e, 2))
    x3, im = slv.singlestep_dpm_solver_third_update(x, s, e, return_intermediate=True, solver_type="taylor")  # r1 = 1/3, r2 = 2/3
    assert set(im) == {"model_s", "model_s1", "model_s2"} and torch.equal(x3, slv.singlestep_dpm_solver_update(x, s, e, 3, solver_type="taylor"))
    assert torch.equal(slv.denoise_to_zero_fn(x, e), slv.data_prediction_fn(x, e))
    with pytest.raises(ValueError):
        slv.singlestep_dpm_solver_second_update(x, s, e, solver_type="heun")
