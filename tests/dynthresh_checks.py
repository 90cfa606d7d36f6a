"""The checks of dynamic thresholding, shared by tests/test_dynthresh_emu.py (host-emulated build, CPU tensors) and tests/test_dynthresh_gpu.py (the gfx950
library): the selection kernel against torch.sort / torch.quantile, and every golden of tests/golden_cases_dynthresh.py through the drop-in classes.

The torch restatement of the reference's two dynamic_thresholding_fn (diffusion_ddpm_pan.py:327-344, solver/dpm_solver.py:424-433) is `threshold_torch`.

Tolerances
  * order statistics, s and the batch / alone comparison: bit equality.  s is compared with torch.quantile on the CPU, whose lerp of the two order statistics is
    one fused multiply-add on the side of the nearer end (w < 0.5 ? fma(w, b - a, a) : fma(w - 1, b - a, b)), which the kernel restates;
  * out against clamp(x, lo, s) / s evaluated by torch in fp32 on the RETURNED s: bit equality.  In the lower-bound-0 form alone the sign of a ZERO result is
    left out of the comparison (both sides' zeros are made +0 first, nothing else is touched): clamp(-0.0, 0.0, s) is +0 or -0 depending on which max the
    backend's vector unit implements, in torch as on the GPU.  The symmetric form has no such case (its lower bound is -s) and is compared as it is;
  * samplers: the project's bar -- atol 1e-4 for the clamped DDPM loop, 1e-4 * max(1, max|golden|) for DPM-Solver++ (unclamped iterates) -- with the golden's
    own fp32 <-> fp64 gap asserted below a tenth of it, as tests/objective_parity.py does."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import golden_cases as gc
import golden_cases_dynthresh as gd
import objective_parity as P
from ddif_testlib import make_net, reference_noise_stream

SIZES = (1, 2, 63, 64, 65, 1000, 2048, 7936, 32768, 32769, 507904)  # below one wave .. not a multiple of the workgroup .. last resident, first streaming .. CAVE 128 x 128 x 31
RATIOS = (0.0, 0.5, 0.8, 0.995, 1.0)
DATA = ("normal", "ties", "equal", "zeros_denormals", "range")
B = 3


def threshold_torch(x0, p, max_val, symmetric):
    s = torch.quantile(x0.abs().reshape(x0.shape[0], -1), p, dim=1)
    s = torch.maximum(s, max_val * torch.ones_like(s)).reshape((-1,) + (1,) * (x0.dim() - 1))
    return torch.clamp(x0, -s if symmetric else torch.zeros_like(s), s) / s


def make_data(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "normal":  # normals, with signs
        return torch.randn(B, n, generator=g) * 1.7
    if kind == "ties":  # a clamped image: half the values exactly 0.0, a quarter exactly 1.0 -- the ties span every rank of RATIOS but the last
        x = torch.rand(B, n, generator=g)
        u = torch.rand(B, n, generator=g)
        return torch.where(u < 0.5, torch.zeros_like(x), torch.where(u < 0.75, torch.ones_like(x), x))
    if kind == "equal":
        return torch.full((B, n), -0.37)
    if kind == "zeros_denormals":  # +0, -0 and denormals of both signs (their keys differ in the LOWEST bytes only)
        bits = torch.randint(0, 1 << 12, (B, n), generator=g, dtype=torch.int32)
        bits = torch.where(torch.rand(B, n, generator=g) < 0.3, torch.zeros_like(bits), bits)
        sign = torch.where(torch.rand(B, n, generator=g) < 0.5, torch.full_like(bits, -(1 << 31)), torch.zeros_like(bits))
        return (bits | sign).view(torch.float32)
    if kind == "range":  # 577 : 1e-3, the spread of the first DDPM step of the noise golden
        e = torch.rand(B, n, generator=g) * (np.log(577.0) - np.log(1e-3)) + np.log(1e-3)
        return torch.exp(e) * torch.where(torch.rand(B, n, generator=g) < 0.5, -1.0, 1.0)
    raise KeyError(kind)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _plus_zero(t):
    """Zeros of either sign -> +0; every other value untouched."""
    return torch.where(t == 0, torch.zeros_like(t), t)


def quantile_stats(lib, x, p):
    """include/ddif_testops.h ddif_quantile_abs_stats -> (s [B], stats [B, 2])."""
    fn = lib.dll.ddif_quantile_abs_stats
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    s = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    st = torch.empty((x.shape[0], 2), dtype=torch.float32, device=x.device)
    stream = None if x.device.type != "cuda" else C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
    lib.check(fn(C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], float(p), C.c_void_p(s.data_ptr()), C.c_void_p(st.data_ptr()), stream), "ddif_quantile_abs_stats")
    return s.cpu(), st.cpu()


def run_op(lib, n, dev):
    from ddif.runtime import dynamic_threshold

    worst = 0
    for di, kind in enumerate(DATA):
        x = make_data(kind, n, 1000 * di + (n % 997))
        xs = torch.sort(x.abs(), dim=1).values
        xd = x.to(dev)
        for p in RATIOS:
            r = np.float32(p) * np.float32(n - 1)
            lo, hi = int(np.floor(r)), int(np.ceil(r))
            s, st = quantile_stats(lib, xd, p)
            what = f"n={n} {kind} p={p}"
            assert torch.equal(_bits(st[:, 0]), _bits(xs[:, lo])), (what, "rank floor(r)", st[:, 0], xs[:, lo])
            assert torch.equal(_bits(st[:, 1]), _bits(xs[:, hi])), (what, "rank ceil(r)", st[:, 1], xs[:, hi])
            q = torch.quantile(x.abs(), p, dim=1)
            ulp = (_bits(s) - _bits(q)).abs().max().item()
            worst = max(worst, ulp)
            assert ulp == 0, (what, "s vs torch.quantile", s, q)
            # (past the resident size one max_val and one form per case, alternating: every further call streams the sample five more times)
            for max_val in ((1.0, 1e-3) if kind in ("normal", "range") and n <= 32769 else (1.0,)):
                for sym in ((False, True) if n <= 32769 else (bool(RATIOS.index(p) & 1),)):
                    out, s2 = dynamic_threshold(xd, p, max_val, sym)
                    s2 = s2.cpu()
                    assert torch.equal(_bits(s2), _bits(torch.maximum(q, torch.full_like(q, max_val)))), (what, max_val)
                    sb = s2.reshape(B, 1)
                    want = torch.clamp(x, -sb if sym else torch.zeros_like(sb), sb) / sb
                    got = out.cpu()
                    if not sym:  # (the one ambiguity: the sign of clamp(-0.0, 0.0, s))
                        got, want = _plus_zero(got), _plus_zero(want)
                    assert torch.equal(_bits(got), _bits(want)), (what, max_val, sym)
                    want = torch.clamp(x, -sb if sym else torch.zeros_like(sb), sb) / sb
                    assert torch.equal(want, threshold_torch(x, p, max_val, sym))  # (the four-line restatement says the same)
            _, s1 = dynamic_threshold(xd[1:2].contiguous(), p, 1e-3, True)  # a sample of a batch gives what the sample alone gives
            _, s3 = dynamic_threshold(xd, p, 1e-3, True)
            assert torch.equal(_bits(s1), _bits(s3[1:2])), (what, "alone vs batch")
    print(f"n={n}: worst |s - torch.quantile| over {len(DATA) * len(RATIOS)} cases: {worst} ulp")


def diffusion(ds, T, size, dev, pred_mode, schedule=None, clamp_type="dynamic"):
    from ddif.diffusion.diffusion_ddpm_pan import GaussianDiffusion, make_beta_schedule

    d = GaussianDiffusion(P.net_for(ds, dev), image_size=size, channels=gc.DATASETS[ds][0], pred_mode=pred_mode, loss_type="l2", device=dev, clamp_range=(0, 1),
                          clamp_type=clamp_type)
    d.set_new_noise_schedule(betas=make_beta_schedule(**(schedule or dict(schedule="cosine", n_timestep=T, cosine_s=8e-3))), device=dev)
    return d


def check_activity(g, cid, expect_active):
    """The fixture exercises what it claims: the reference's own quantiles, stored per (step, sample)."""
    frac = gd.active_fraction(g["quant"], float(g["max_val"]))
    print(f"{cid}: the reference's quantile {float(g['quant'].min()):.4g} .. {float(g['quant'].max()):.4g}, above max_val {float(g['max_val'])} in {frac:.0%} of the (step, sample) pairs")
    if expect_active:
        assert frac >= 0.5, (cid, frac)
    else:
        assert frac == 0.0, (cid, frac)


def _compare(out, g, what, relative):
    ref = torch.from_numpy(g["out"])
    tol = 1e-4 * (max(1.0, float(ref.abs().max())) if relative else 1.0)
    err = float((out.cpu() - ref).abs().max())
    print(f"{what}: max|out - golden| {err:.3e} (max|golden| {float(ref.abs().max()):.3g}, tolerance {tol:.3e})")
    P.check_gap(g["gap"], tol, what)
    assert bool(torch.isfinite(out).all())
    assert err <= tol, (what, err, tol)


def run_ddpm(case, dev):
    cid, ds, Bn, H, W, T, pm, seed, expect_active = case
    g = P.load(cid)
    check_activity(g, cid, expect_active)
    C_ = gc.DATASETS[ds][0]
    cond = gc.tiles_for(ds, Bn, H, W, seed=seed)["cond"]
    d = diffusion(ds, T, H, dev, pm)
    xT, noise = reference_noise_stream(seed, (Bn, C_, H, W), T)
    out = d(cond.to(dev), mode="ddpm_sample", x_T=xT.to(dev), noise=noise.to(dev))
    _compare(out, g, cid, relative=False)
    return out


def run_dpm(case, dev):
    from ddif.solver.dpm_solver import DPM_Solver, NoiseScheduleVP, model_wrapper

    cid, ds, H, W, T, steps, order, mt, seed, kw = case
    g = P.load(cid)
    check_activity(g, cid, True)
    assert float(g["max_val"]) == float(kw["thresholding_max_val"])
    C_ = gc.DATASETS[ds][0]
    cond = gc.tiles_for(ds, 1, H, W, seed=seed)["cond"].to(dev)
    xT = torch.randn(1, C_, H, W, generator=torch.Generator().manual_seed(seed)).to(dev)
    d = diffusion(ds, T, H, dev, gd.PRED_OF_MODEL_TYPE[mt], schedule=gd.dpm_schedule(mt, T), clamp_type="abs")
    ns = NoiseScheduleVP("discrete", betas=d.betas)
    fn = model_wrapper(d.model, ns, model_type=mt, guidance_type="classifier-free", guidance_scale=1.0, condition=cond)
    slv = DPM_Solver(fn, ns, algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding", **kw)
    fused = slv._fused_target()
    assert fused is not None and fused[2] == "dynamic"  # the whole run inside libddif
    out = slv.sample(xT, steps=steps, order=order, skip_type="time_uniform", method="multistep")
    _compare(out, g, cid, relative=True)
    plan = d.model.plan_for(1, H, W, dev)
    assert plan.get_threshold() == ("solver", np.float32(kw["dynamic_thresholding_ratio"]), np.float32(kw["thresholding_max_val"]))
    plan.set_threshold("off")


def run_batch_equals_tiles(case, dev):
    """A DDPM golden run as a batch equals its tiles run alone, bit for bit (the quantile of a sample does not depend on its neighbours)."""
    cid, ds, Bn, H, W, T, pm, seed, _ = case
    assert Bn > 1
    C_ = gc.DATASETS[ds][0]
    cond = gc.tiles_for(ds, Bn, H, W, seed=seed)["cond"].to(dev)
    d = diffusion(ds, T, H, dev, pm)
    xT, noise = reference_noise_stream(seed, (Bn, C_, H, W), T)
    xT, noise = xT.to(dev), noise.to(dev)
    whole = d(cond, mode="ddpm_sample", x_T=xT, noise=noise).clone()
    for b in range(Bn):
        one = d(cond[b:b + 1].contiguous(), mode="ddpm_sample", x_T=xT[b:b + 1].contiguous(), noise=noise[:, b:b + 1].contiguous())
        assert torch.equal(one, whole[b:b + 1]), (cid, b, float((one - whole[b:b + 1]).abs().max()))


def _ddpm_args(d, T, steps, xT, noise, dev):
    c1, c2 = d.posterior_mean_coef1.cpu(), d.posterior_mean_coef2.cpu()
    cz = (0.5 * d.posterior_log_variance_clipped.cpu()).exp()
    order = list(reversed(range(T)))[:steps]
    return ([float(i) for i in order], [float(c1[i]) for i in order], [float(c2[i]) for i in order], [float(cz[i]) for i in order], xT, noise, 0, 0, (0.0, 1.0), dev)


def run_mode0_is_bit_identical(dev, Bn=2, steps=4):
    """A plan with mode 0 set EXPLICITLY -- also after a detour through modes 1 and 2 -- reproduces an untouched plan bit for bit in the DDPM, DDIM and
    DPM-Solver++ loops, with the same number of launches; modes 1 / 2 change only the loop they name.  steps >= 4 lets the GPU library capture and replay
    its step pair; the emulator, which has no graphs, runs one tile for two steps."""
    ds, H, W, T = "wv3", 16, 16, 20
    C_ = gc.DATASETS[ds][0]
    cond = gc.tiles_for(ds, Bn, H, W, seed=9)["cond"].to(dev)
    gen = torch.Generator().manual_seed(9)
    xT = torch.randn(Bn, C_, H, W, generator=gen).to(dev)
    noise = torch.randn(steps, Bn, C_, H, W, generator=gen).to(dev)
    d = diffusion(ds, T, H, dev, "x_start", clamp_type="abs")
    args = _ddpm_args(d, T, steps, xT, noise, dev)
    sr, srm1 = d.sqrt_recip_alphas_cumprod.cpu(), d.sqrt_recipm1_alphas_cumprod.cpu()
    order = list(reversed(range(T)))[:steps]
    ddim = ([float(i) for i in order], [float(sr[i]) for i in order], [float(srm1[i]) for i in order], [float(torch.sqrt(d.alphas_cumprod_prev.cpu()[i])) for i in order],
            [float(torch.sqrt(1 - d.alphas_cumprod_prev.cpu()[i])) for i in order], [0.0] * steps, xT, None, 0, 0, None, dev)
    dpm = dict(n_evals=2, order=2, t_model=[900.0, 400.0], alpha=[0.3, 0.8], sigma=[0.95, 0.6], ord=[1, 2], cx=[0.8, 0.5], a_phi1=[-0.3, -0.4],
               inv_r0=[0.0, 1.1], inv_r1=[0.0] * 2, r0_frac=[0.0] * 2, inv_r01=[0.0] * 2, a_phi2=[0.0] * 2, a_phi3=[0.0] * 2)
    net = make_net(ds, dev)  # a net (and plan) of its own: no earlier test has stated a threshold on it
    plan = net.plan_for(Bn, H, W, dev)
    plan.set_cond(cond, force=True)
    n0 = plan.num_launches()
    assert plan.get_threshold() == ("off", 0.0, 1.0)  # what the library holds for a new plan
    base = [plan.sample_ddpm(*args).clone(), plan.sample_ddim(*ddim).clone(), plan.sample_dpmpp(dpm, xT, (0.0, 1.0)).clone(), plan.sample_dpmpp(dpm, xT, None).clone()]

    def all_four():
        return [plan.sample_ddpm(*args), plan.sample_ddim(*ddim), plan.sample_dpmpp(dpm, xT, (0.0, 1.0)), plan.sample_dpmpp(dpm, xT, None)]

    plan.lib.check(plan.lib.dll.ddif_plan_set_threshold(plan.h, 0, 0.8, 1.0), "ddif_plan_set_threshold")  # explicitly off
    assert plan.num_launches() == n0
    assert all(torch.equal(a, b) for a, b in zip(all_four(), base))
    plan.set_threshold("ddpm", 0.8, 0.25)
    assert plan.get_threshold() == ("ddpm", np.float32(0.8), 0.25) and plan.num_launches() == n0
    got = [plan.sample_ddpm(*args).clone(), plan.sample_ddim(*ddim), plan.sample_dpmpp(dpm, xT, (0.0, 1.0)), plan.sample_dpmpp(dpm, xT, None)]
    assert not torch.equal(got[0], base[0])  # mode 1 changes the DDPM loop ...
    assert all(torch.equal(a, b) for a, b in zip(got[1:], base[1:]))  # ... and nothing else (DDIM never thresholds, as in the reference)
    noclamp = list(args)
    noclamp[8] = None  # clamp_range=None: clip_noise gates both clamps
    plan.set_threshold("off")
    ref_noclamp = plan.sample_ddpm(*noclamp).clone()
    plan.set_threshold("ddpm", 0.8, 0.25)
    assert torch.equal(plan.sample_ddpm(*noclamp), ref_noclamp)
    assert torch.equal(plan.sample_ddpm(*args), got[0])  # (and back: the captured pair follows the switch)
    plan.set_threshold("solver", 0.9, 0.25)
    assert torch.equal(plan.sample_ddpm(*args), base[0]) and torch.equal(plan.sample_ddim(*ddim), base[1])
    assert not torch.equal(plan.sample_dpmpp(dpm, xT, None), base[3])
    plan.set_threshold("off")
    assert plan.get_threshold() == ("off", 0.0, 1.0) and plan.num_launches() == n0
    assert all(torch.equal(a, b) for a, b in zip(all_four(), base))


def run_set_threshold_rejects(dev):
    from ddif import DdifError

    ds, Bn, H, W = "wv3", 1, 16, 16
    C_ = gc.DATASETS[ds][0]
    net = P.net_for(ds, dev)
    plan = net.plan_for(Bn, H, W, dev)
    plan.set_cond(gc.tiles_for(ds, Bn, H, W, seed=2)["cond"].to(dev), force=True)
    plan.set_threshold("off")  # (the plan is shared with the golden tests, and the switch is sticky)
    dll = plan.lib.dll
    try:
        for mode, ratio, max_val in ((3, 0.8, 1.0), (-1, 0.8, 1.0), (1, 1.5, 1.0), (1, -0.1, 1.0), (2, float("nan"), 1.0), (1, 0.8, -1.0), (2, 0.8, float("inf")), (2, 0.8, float("nan"))):
            assert dll.ddif_plan_set_threshold(plan.h, mode, ratio, max_val) == -1, (mode, ratio, max_val)  # DDIF_ERR_INVALID
            assert plan.get_threshold() == ("off", 0.0, 1.0)  # ... and nothing was changed
        plan.set_threshold("solver", 0.995, 1.0)
        dpm = dict(n_evals=1, order=1, t_model=[900.0], alpha=[0.3], sigma=[0.95], ord=[1], cx=[0.8], a_phi1=[-0.3], inv_r0=[0.0], inv_r1=[0.0], r0_frac=[0.0], inv_r01=[0.0],
                   a_phi2=[0.0], a_phi3=[0.0])
        xT = torch.zeros(Bn, C_, H, W, device=dev)
        try:
            plan.sample_dpmpp(dpm, xT, (0.0, 1.0))  # mode 2 together with the image-space clamp
            raise AssertionError("expected DdifError")
        except DdifError as e:
            assert "clamp" in str(e)
        plan.sample_dpmpp(dpm, xT, None)
        try:
            plan.set_threshold("imagen")
            raise AssertionError("expected DdifError")
        except DdifError:
            pass
    finally:
        plan.set_threshold("off")


def run_front_door_methods(dev):
    """GaussianDiffusion.dynamic_thresholding_fn and DPM_Solver.dynamic_thresholding_fn run the stateless op on device tensors and read their two attributes
    at call time; a solver built with the keyword takes the generic loop through the same method when the run cannot be fused."""
    from ddif.solver.dpm_solver import DPM_Solver, NoiseScheduleVP

    ds, H = "wv3", 16
    d = diffusion(ds, 20, H, dev, "x_start")
    x = make_data("range", 8 * H * H, 77).reshape(B, 8, H, H)
    got = d.dynamic_thresholding_fn(x.to(dev), None).cpu()
    assert torch.equal(got, threshold_torch(x, 0.8, 1.0, symmetric=False))
    d.dynamic_thresholding_ratio, d.thresholding_max_val = 0.5, 0.125
    assert torch.equal(d.dynamic_thresholding_fn(x.to(dev), None).cpu(), threshold_torch(x, 0.5, 0.125, symmetric=False))
    ns = NoiseScheduleVP("discrete", betas=d.betas)
    slv = DPM_Solver(lambda x_, t_: x_, ns, algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding", thresholding_max_val=0.5, dynamic_thresholding_ratio=0.9)
    assert slv.correcting_x0_fn == slv.dynamic_thresholding_fn and slv._fused_target() is None  # not a ddif model: the generic loop, through the method
    assert torch.equal(slv.dynamic_thresholding_fn(x.to(dev), None).cpu(), threshold_torch(x, 0.9, 0.5, symmetric=True))
    y = slv.data_prediction_fn(x.to(dev), torch.tensor([0.5]))
    assert float(y.abs().max()) <= 1.0
