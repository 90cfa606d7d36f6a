"""The checks of classifier-free guidance in DPM-Solver runs (model_wrapper with guidance_scale != 1 and an unconditional_condition; reference
solver/dpm_solver.py:330-338), shared by tests/test_cfg_host.py (no library), tests/test_cfg_emu.py (host-emulated build, CPU tensors) and
tests/test_cfg_gpu.py (the gfx950 library).

Tolerances
  * model_wrapper's guided model_fn on a lambda model against the hand-written fp32 expression: the same torch ops in the same order -> torch.equal;
  * the guided form of csrc/kernels_misc.h dpm_eval_update_kernel against its torch restatement (dpmx_checks.model_value_torch / update_torch, every scalar
    broadcast to a full tensor so that each torch op is one correctly rounded fp32 operation per element, as each kernel operation is with contraction off):
    bit equality, and both halves of the written state equal;
  * goldens (the real reference, fp32): the project's bar for solver iterates, 1e-4 * max(1, max|golden|), with the golden's own fp32 <-> fp64 gap asserted
    below a tenth of it; the same rule, over max|generic run|, for the model types the reference cannot run under guidance;
  * batch against tiles alone, return_intermediate against the plain run, guidance_scale == 1 against no unconditional_condition: bit equality."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import dpmx_checks as K
import golden_cases as gc
import golden_cases_cfg as gcfg
import golden_cases_dpmx as gx
import objective_parity as P


# ---- model_wrapper on the host: no library ----------------------------------------------------------------------------------------------------------------
def host_schedule(T=500):
    from ddif.diffusion.diffusion_ddpm_pan import make_beta_schedule
    from ddif.solver.dpm_solver import NoiseScheduleVP

    return NoiseScheduleVP("discrete", betas=torch.as_tensor(make_beta_schedule(**gx.schedule_kwargs("linear", T))).float())


def lambda_model(calls=None):
    """A per-sample elementwise model of x, t and cond (so a doubled batch gives what its halves give alone, bit for bit); records its arguments."""
    def model(x, t, cond):
        if calls is not None:
            calls.append((x.clone(), t.clone(), cond.clone()))
        return 0.3 * x + 0.5 * cond[:, :x.shape[1]] - 0.25 * cond[:, x.shape[1]:x.shape[1] + 1] + 1e-3 * t.reshape(-1, 1, 1, 1)
    return model


def host_inputs(B, seed=7, C_=2, H=4):
    g = torch.Generator().manual_seed(seed)
    x, cond = torch.randn(B, C_, H, H, generator=g), torch.randn(B, C_ + 1, H, H, generator=g)
    uncond = torch.randn(B, C_ + 1, H, H, generator=g)  # differs from cond in EVERY channel
    t = torch.full((B,), 0.37)
    return x, t, cond, uncond


def run_host_guided_model_fn(model_type, B, scale=1.75):
    """The guided model_fn equals the hand-written fp32 expression (reference :296-303 on each half, then :338), from ONE model call on
    [unconditional; conditional] with t repeated."""
    from ddif.solver.dpm_solver import model_wrapper

    ns = host_schedule()
    x, t, cond, uncond = host_inputs(B)
    calls = []
    fn = model_wrapper(lambda_model(calls), ns, model_type=model_type, guidance_type="classifier-free", guidance_scale=scale, condition=cond,
                       unconditional_condition=uncond)
    got = fn(x, t)
    assert len(calls) == 1, "one network call per evaluation"
    x_in, t_in, c_in = calls[0]
    t_model = (t - 1.0 / ns.total_N) * 1000.0
    assert torch.equal(x_in, torch.cat([x, x])) and torch.equal(t_in, torch.cat([t_model, t_model])) and torch.equal(c_in, torch.cat([uncond, cond]))
    model = lambda_model()
    a, s = ns.marginal_alpha(t).reshape(-1, 1, 1, 1), ns.marginal_std(t).reshape(-1, 1, 1, 1)

    def eps_of(c):
        o = model(x, t_model, c)
        return o if model_type == "noise" else (x - a * o) / s if model_type == "x_start" else a * o + s * x
    eps_u, eps_c = eps_of(uncond), eps_of(cond)
    want = eps_u + scale * (eps_c - eps_u)
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert torch.equal(got, want), (model_type, B, float((got - want).abs().max()))
    assert not torch.equal(got, eps_c)
    meta = fn.ddif
    assert meta["guidance_scale"] == scale and meta["unconditional_condition"] is uncond and meta["condition"] is cond


def run_host_single_call_without_guidance():
    """guidance_scale == 1.0 or unconditional_condition=None: the single conditional evaluation (:331-332)."""
    from ddif.solver.dpm_solver import model_wrapper

    ns = host_schedule()
    x, t, cond, uncond = host_inputs(2)
    plain = model_wrapper(lambda_model(), ns, model_type="v", guidance_type="classifier-free", guidance_scale=1.0, condition=cond)(x, t)
    for scale, u in ((1.0, uncond), (2.5, None), (1.0, None)):
        calls = []
        fn = model_wrapper(lambda_model(calls), ns, model_type="v", guidance_type="classifier-free", guidance_scale=scale, condition=cond, unconditional_condition=u)
        got = fn(x, t)
        assert len(calls) == 1 and torch.equal(calls[0][0], x) and torch.equal(calls[0][2], cond) and calls[0][1].shape == t.shape
        assert torch.equal(got, plain)


def run_host_guided_generic_solver():
    """A guided model_fn that is not a ddif network goes through the generic loops of every method: finite, and different from the unguided run."""
    from ddif.solver.dpm_solver import DPM_Solver, model_wrapper

    ns = host_schedule()
    x, _, cond, uncond = host_inputs(2)
    for method, algorithm in (("multistep", "dpmsolver++"), ("singlestep", "dpmsolver"), ("singlestep_fixed", "dpmsolver++")):
        outs = []
        for scale in (1.0, 2.0):
            fn = model_wrapper(lambda_model(), ns, model_type="noise", guidance_type="classifier-free", guidance_scale=scale, condition=cond,
                               unconditional_condition=uncond)
            slv = DPM_Solver(fn, ns, algorithm_type=algorithm)
            assert slv._fused_target() is None
            assert (slv._guidance() is None) == (scale == 1.0)
            outs.append(slv.sample(x, steps=6, order=3, method=method))
        assert bool(torch.isfinite(outs[1]).all()) and not torch.equal(outs[0], outs[1])


def run_host_wrapper_validation():
    from ddif import DdifError
    from ddif.solver.dpm_solver import model_wrapper

    ns = host_schedule()
    x, t, cond, uncond = host_inputs(2)
    kw = dict(model_type="noise", guidance_type="classifier-free", guidance_scale=2.0, condition=cond)
    bad = [uncond[:1], uncond[:, :2], uncond.double()]
    if torch.cuda.is_available():
        bad.append(uncond.to("cuda:0"))
    for u in bad:
        try:
            model_wrapper(lambda_model(), ns, unconditional_condition=u, **kw)
            raise AssertionError("expected DdifError")
        except DdifError as e:
            assert "unconditional_condition" in str(e)
    for scale in (float("inf"), float("nan")):
        try:
            model_wrapper(lambda_model(), ns, unconditional_condition=uncond, **dict(kw, guidance_scale=scale))
            raise AssertionError("expected DdifError")
        except DdifError as e:
            assert "finite" in str(e)
    try:  # classifier guidance stays refused exactly as it is
        model_wrapper(lambda_model(), ns, model_type="noise", guidance_type="classifier", guidance_scale=2.0, condition=cond, classifier_fn=lambda *a: None)
        raise AssertionError("expected DdifError")
    except DdifError as e:
        assert "classifier guidance" in str(e)


# ---- the guided form of dpm_eval_update_kernel ------------------------------------------------------------------------------------------------------------
def eval_update_guided(lib, dev, net, xe, lms, thr, per, scale, alpha, sigma, lo, hi, do_clamp, model_type, algorithm, form, order, x, ms, c):
    """include/ddif_testops.h ddif_dpm_eval_update_guided -> (m_out [n], out [2n]) on the CPU; ms: three tensors of n floats or None (= the value of this launch)."""
    fn = lib.dll.ddif_dpm_eval_update_guided
    vp, f32, i32, i64 = C.c_void_p, C.c_float, C.c_int, C.c_int64
    fn.argtypes = [vp, vp, vp, vp, i64, i64, f32, f32, f32, f32, f32, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.POINTER(C.c_float), vp, vp, vp]
    n = net.numel() // 2
    dv = lambda t: None if t is None else t.to(dev).contiguous()
    net, xe, lms, thr, x = dv(net), dv(xe), dv(lms), dv(thr), dv(x)
    ms = [dv(m) for m in ms]
    m_out = torch.empty(n, dtype=torch.float32, device=dev)
    out = torch.full((2 * n,), float("nan"), dtype=torch.float32, device=dev)
    carr = (C.c_float * 9)(*[float(v) for v in list(c) + [0.0] * (9 - len(c))])
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = None if torch.device(dev).type != "cuda" else C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib.check(fn(p(net), p(xe), p(lms), p(thr), n, per, scale, alpha, sigma, lo, hi, int(do_clamp), model_type, algorithm, K.FORMS[form], order, p(x), p(ms[0]), p(ms[1]),
                 p(ms[2]), carr, p(m_out), p(out), stream), "ddif_dpm_eval_update_guided")
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize(dev)
    return m_out.cpu(), out.cpu()


def guided_model_value_torch(net_u, net_c, xe, lms_c, thr_rows, scale, alpha, sigma, lo, hi, do_clamp, model_type, eps_only):
    """model_type conversion of both halves against the same iterate, eps_u + scale * (eps_c - eps_u), then what an unguided noise prediction goes through."""
    conv = lambda o: K.model_value_torch(o, xe, None, None, alpha, sigma, lo, hi, False, model_type, True)
    eps_u, eps_c = conv(net_u), conv(net_c)
    eps = eps_u + K._full(xe, scale) * (eps_c - eps_u)
    return K.model_value_torch(eps, xe, lms_c, thr_rows, alpha, sigma, lo, hi, do_clamp, 1, eps_only)


def run_guided_forms(lib, dev, n=1000):
    """Every model_type x both algorithms x {no corrector, clamp, thresholding rows}: the evaluation alone and fused update forms behind it, n = 1000 values per
    half (four workgroups of 256: the last one is partly idle).  The unconditional half carries other lms bits than the conditional one, and a second
    thresholding table that would be indexed by a kernel walking 2n items is absent: a corrector reading the wrong half fails."""
    g = torch.Generator().manual_seed(2424)
    rnd = lambda m, scale=1.0: torch.randn(m, generator=g) * scale
    net = rnd(2 * n)
    xh, xeh = rnd(n, 0.9), rnd(n, 1.3)
    x, xe = torch.cat([xh, xh]), torch.cat([xeh, xeh])  # a state register holds the same bits in both halves
    lms = torch.rand(2 * n, generator=g)
    assert not torch.equal(lms[:n], lms[n:])
    old = [rnd(n, 1.1), rnd(n, 0.7), rnd(n, 1.9)]
    per = n // 4
    thr = torch.tensor([0.31, 0.77, 1.0, 2.5])
    thr_rows = thr.repeat_interleave(per)
    alpha, sigma, scale = float(np.float32(0.61803)), float(np.float32(0.78615)), float(np.float32(1.7))
    c9 = [0.9371, -0.2113, 0.4177, float(np.float32(1 / 0.31)), float(np.float32(1 / 0.69)), 0.31, 0.69, float(np.float32(0.69) - np.float32(0.31)), -0.0613]
    cm = [0.9371, -0.2113, 1.271, 0.853, 0.5931, 0.4713, 0.4177, -0.0613, 0.0]
    cl3 = [0.9371, -0.2113, 0.7391, 1.271, 0, 0, 0, 0, 0]
    updates = [("multi", 1, cm, 0), ("multi", 3, cm, 0), ("multi", 3, cm, 2), ("lin1", 0, cl3, 0), ("lin2", 0, cl3, 1), ("tay3", 0, c9, 2)]  # (.., which register is fresh)
    checked = 0
    for algorithm in (0, 1):
        for model_type in (0, 1, 2):
            for corr in ("none", "clamp", "thr"):
                if algorithm == 1 and corr != "none":
                    continue  # (no corrector on a noise-prediction evaluation, as in dpmx_checks.run_forms)
                do_clamp, th = corr == "clamp", (thr if corr == "thr" else None)
                want_m = guided_model_value_torch(net[:n], net[n:], xeh, lms[n:], thr_rows if corr == "thr" else None, scale, alpha, sigma, 0.0, 1.0, do_clamp, model_type,
                                                  algorithm == 1)
                m, o = eval_update_guided(lib, dev, net, xe, lms, th, per, scale, alpha, sigma, 0.0, 1.0, do_clamp, model_type, algorithm, "none", 0, None, [None] * 3, [])
                assert torch.equal(m, want_m), ("model value", algorithm, model_type, corr, float((m - want_m).abs().max()))
                assert torch.equal(o[:n], want_m) and torch.equal(o[n:], want_m), ("model value to both halves", algorithm, model_type, corr)
                if corr == "clamp":  # the test can tell: the unconditional half's lms gives another value
                    assert not torch.equal(want_m, guided_model_value_torch(net[:n], net[n:], xeh, lms[:n], None, scale, alpha, sigma, 0.0, 1.0, True, model_type, False))
                for form, order, c, fresh in updates:
                    ms = [None if j == fresh else old[j] for j in range(3)]
                    mt = [want_m if j == fresh else old[j] for j in range(3)]
                    want = K.update_torch(form, order, xh, mt[0], mt[1], mt[2], c)
                    m, o = eval_update_guided(lib, dev, net, xe, lms, th, per, scale, alpha, sigma, 0.0, 1.0, do_clamp, model_type, algorithm, form, order, x, ms, c)
                    assert torch.equal(m, want_m), ("stored model value", form, order, fresh)
                    assert torch.equal(o[:n], o[n:]), ("both halves of the written state", algorithm, model_type, corr, form, order)
                    assert torch.equal(o[:n], want), ("fused update", algorithm, model_type, corr, form, order, fresh, float((o[:n] - want).abs().max()))
                    checked += 1
    # scale 1 is arithmetic too (eps_u + (eps_c - eps_u)); the unguided entry point on the conditional half is the other thing
    want1 = guided_model_value_torch(net[:n], net[n:], xeh, lms[n:], None, 1.0, alpha, sigma, 0.0, 1.0, False, 0, True)
    m1, _ = eval_update_guided(lib, dev, net, xe, lms, None, per, 1.0, alpha, sigma, 0.0, 1.0, False, 0, 1, "none", 0, None, [None] * 3, [])
    assert torch.equal(m1, want1)
    print(f"dpm_eval_update_kernel, guided: {checked} fused (model value, update) combinations equal torch bit for bit on 2 x {n} values")


# ---- through DPM_Solver.sample ----------------------------------------------------------------------------------------------------------------------------
def solver_for(case, dev, B=1, scale="case", with_uncond=True, tiles=None, **solver_kw):
    """(solver, x_T, cond, uncond, diffusion) of a case on `dev` with B tiles (tile 0 is the golden's); tiles: indices to keep."""
    from ddif.diffusion.diffusion_ddpm_pan import GaussianDiffusion, make_beta_schedule
    from ddif.solver.dpm_solver import DPM_Solver, ImageSpaceClamp, NoiseScheduleVP, model_wrapper

    ds, H, T, seed = case["ds"], case["H"], case["T"], case["seed"]
    C_ = gc.DATASETS[ds][0]
    cond = gc.tiles_for(ds, 1, H, H, seed=seed)["cond"]
    xT = torch.randn(1, C_, H, H, generator=torch.Generator().manual_seed(seed))
    if B > 1:
        cond = torch.cat([cond, gc.tiles_for(ds, B - 1, H, H, seed=seed + 1)["cond"]])
        xT = torch.cat([xT, torch.randn(B - 1, C_, H, H, generator=torch.Generator().manual_seed(seed + 1))])
    if tiles is not None:
        cond, xT = cond[tiles], xT[tiles]
    cond, xT = cond.to(dev).contiguous(), xT.to(dev).contiguous()
    uncond = gcfg.unconditional_of(cond, C_)
    d = GaussianDiffusion(P.net_for(ds, dev), image_size=H, channels=C_, pred_mode=gx.PRED_OF_MODEL_TYPE[case["model_type"]], loss_type="l2", device=dev, clamp_range=(0, 1))
    d.set_new_noise_schedule(betas=make_beta_schedule(**gx.schedule_kwargs(case["schedule"], T)), device=dev)
    ns = NoiseScheduleVP("discrete", betas=d.betas)
    fn = model_wrapper(d.model, ns, model_type=case["model_type"], guidance_type="classifier-free", guidance_scale=case["scale"] if scale == "case" else scale,
                       condition=cond, unconditional_condition=uncond if with_uncond else None)
    corr = {"clamp": ImageSpaceClamp(cond[:, :C_], 0.0, 1.0), "dyn": "dynamic_thresholding", None: None}[case["corrector"]]
    return DPM_Solver(fn, ns, algorithm_type=case["algorithm"], correcting_x0_fn=corr, **solver_kw), xT, cond, uncond, d


def _reset(d, case, dev, batches=(2,)):
    for B in batches:  # the plans the run used (plans are shared between tests, and the threshold switch is sticky)
        d.model.plan_for(B, case["H"], case["H"], dev).set_threshold("off")


class guided_calls:
    """Counts PlanHandle.sample_dpm_guided / sample_dpm / sample_dpmpp calls."""

    def __enter__(self):
        from ddif.runtime import PlanHandle

        self.cls, self.orig, self.n = PlanHandle, {}, dict(sample_dpm_guided=0, sample_dpm=0, sample_dpmpp=0)
        for name in self.n:
            self.orig[name] = getattr(PlanHandle, name)

            def counted(plan, *a, _name=name, **k):
                self.n[_name] += 1
                return self.orig[_name](plan, *a, **k)
            setattr(PlanHandle, name, counted)
        return self.n

    def __exit__(self, *a):
        for name, fn in self.orig.items():
            setattr(self.cls, name, fn)


def run_golden(case, dev):
    g = P.load(case["cid"])
    ref, tol = torch.from_numpy(g["out"]), K.tolerance(g)
    P.check_gap(g["gap"], tol, case["cid"])
    assert float(g["guided_minus_unguided"]) > 100 * tol  # an unguided run cannot pass
    slv, xT, cond, uncond, d = solver_for(case, dev)
    try:
        assert slv._fused_target() is not None and slv._guidance() is not None
        with K.forward_forbidden(), guided_calls() as n:
            out = slv.sample(xT, **gx.sample_kwargs(case))
        assert n == dict(sample_dpm_guided=1, sample_dpm=0, sample_dpmpp=0), n
        err = float((out.cpu() - ref).abs().max())
        print(f"{case['cid']}: max|out - golden| {err:.3e} (max|golden| {float(ref.abs().max()):.3g}, tolerance {tol:.3e})")
        assert out.shape == xT.shape and bool(torch.isfinite(out).all())
        assert err <= tol, (case["cid"], err, tol)
    finally:
        _reset(d, case, dev)
    return out


def run_generic_agrees(model_type, dev):
    """model_type "x_start" / "v" under guidance: the reference raises a broadcast error there, so the yardstick is the drop-in's generic loop (the network
    through its front door on the doubled batch, torch for the rest), forced by correcting_xt_fn = identity.  Tolerance: the golden rule over the generic run."""
    for cid in ("cfg_pp_ms_o3_s12_clamp_g1p5", "cfg_np_ss_o3_s12_d2z_linear_g1p5"):
        case = dict(gcfg.BY_ID[cid], model_type=model_type, steps=6)
        slv, xT, cond, uncond, d = solver_for(case, dev)
        try:
            with K.forward_forbidden(), guided_calls() as n:
                fused = slv.sample(xT, **gx.sample_kwargs(case))
            assert n["sample_dpm_guided"] == 1
            gen, _, _, _, _ = solver_for(case, dev)
            gen.correcting_xt_fn = lambda x, t, step: x
            assert gen._fused_target() is None
            generic = gen.sample(xT, **gx.sample_kwargs(case))
            tol = 1e-4 * max(1.0, float(generic.abs().max()))
            err = float((fused - generic).abs().max())
            print(f"{cid} as {model_type}: max|fused - generic| {err:.3e} (max|generic| {float(generic.abs().max()):.3g}, tolerance {tol:.3e})")
            assert bool(torch.isfinite(fused).all()) and err <= tol, (cid, model_type, err, tol)
            plain, _, _, _, _ = solver_for(case, dev, scale=1.0)
            assert float((plain.sample(xT, **gx.sample_kwargs(case)) - fused).abs().max()) > 100 * tol  # guidance is visible at this tolerance
        finally:
            _reset(d, case, dev, batches=(1, 2))


def run_batch_equals_tiles(dev, B=3):
    """Three guided 16 x 16 tiles in one call equal each tile run alone, bit for bit -- under the clamp, under dynamic thresholding (one s_b per guided
    sample) and on the noise-prediction path; return_intermediate returns Bg-sized images whose last entry is the plain run's result."""
    for cid in ("cfg_pp_ms_o3_s12_clamp_g1p5", "cfg_pp_ms_o2_s10_taylor_dyn_g2", "cfg_np_ss_o3_s12_d2z_linear_g1p5"):
        case = dict(gcfg.BY_ID[cid], steps=5)
        slv, xT, cond, uncond, d = solver_for(case, dev, B=B)
        try:
            with K.forward_forbidden():
                whole = slv.sample(xT, **gx.sample_kwargs(case)).clone()
                whole2, inter = slv.sample(xT, return_intermediate=True, **gx.sample_kwargs(case))
            assert whole.shape == xT.shape and torch.equal(whole2, whole)
            assert isinstance(inter, list) and all(t.shape == xT.shape for t in inter) and torch.equal(inter[-1], whole)
            if case["method"] == "multistep":
                assert len(inter) == case["steps"] + 1 and torch.equal(inter[0], xT)  # the initial x (:1190-1191)
            for b in range(B):
                one, x1, _, _, _ = solver_for(case, dev, B=B, tiles=slice(b, b + 1))
                with K.forward_forbidden():
                    alone = one.sample(x1, **gx.sample_kwargs(case))
                assert torch.equal(alone, whole[b:b + 1]), (cid, b, float((alone - whole[b:b + 1]).abs().max()))
        finally:
            _reset(d, case, dev, batches=(2, 2 * B))


def run_scale_one_is_the_old_path(dev):
    """guidance_scale=1.0 with an unconditional_condition on board: the bits of the same run without one, through the entry points it took before."""
    for cid, entry in (("cfg_pp_ms_o3_s12_clamp_g1p5", "sample_dpmpp"), ("cfg_np_ss_o3_s12_d2z_linear_g1p5", "sample_dpm")):
        case = dict(gcfg.BY_ID[cid], steps=5)
        outs = []
        for with_uncond in (True, False):
            slv, xT, cond, uncond, d = solver_for(case, dev, scale=1.0, with_uncond=with_uncond)
            assert slv._guidance() is None and slv._fused_target() is not None
            with K.forward_forbidden(), guided_calls() as n:
                outs.append(slv.sample(xT, **gx.sample_kwargs(case)).clone())
            assert n == {**dict(sample_dpm_guided=0, sample_dpm=0, sample_dpmpp=0), entry: 1}, n
        assert torch.equal(outs[0], outs[1])


def run_validation(dev):
    """ddif_plan_sample_dpm_guided refuses, with DDIF_ERR_INVALID (-1) / DDIF_ERR_STATE, an odd plan batch, a scale that is not finite, NULL arguments and a
    plan without cond; PlanHandle.sample_dpm_guided and model_wrapper raise DdifError."""
    from ddif import DdifError
    from ddif_testlib import make_net

    ds, H = "wv3", 16
    C_ = gc.DATASETS[ds][0]
    net = make_net(ds, dev)  # its own plans: no other test has given them a cond
    ev = dict(kind="eval", t_model=400.0, alpha=0.8, sigma=0.6, src=0, dst=0)
    up = dict(kind="update", form="lin1", order=0, src=0, dst=0, m=[0, 0, 0], c=[0.9, -0.2])
    ops = [ev, up]
    p = lambda t: C.c_void_p(t.data_ptr())
    x1 = torch.zeros(1, C_, H, H, device=dev)
    out = torch.empty_like(x1)
    plan2 = net.plan_for(2, H, H, dev)
    dll = plan2.lib.dll
    prog, keep = plan2.dpm_program(ops, "dpmsolver++")
    st = dll.ddif_plan_sample_dpm_guided(plan2.h, C.byref(prog), 1.5, p(x1), 0.0, 0.0, 0, p(out), None, None)
    assert st not in (0, -1) and b"ddif_plan_set_cond" in dll.ddif_last_error(), st  # cond not set: DDIF_ERR_STATE
    try:
        plan2.sample_dpm_guided(ops, "dpmsolver++", 1.5, x1, None)
        raise AssertionError("expected DdifError")
    except DdifError as e:
        assert "ddif_plan_set_cond" in str(e)
    cond2 = gc.tiles_for(ds, 2, H, H, seed=2)["cond"].to(dev)
    plan2.set_cond(cond2, force=True)
    plan2.set_threshold("off")
    plan2.set_objective("noise", plan2.objective[1])
    for scale in (float("inf"), float("-inf"), float("nan")):
        assert dll.ddif_plan_sample_dpm_guided(plan2.h, C.byref(prog), scale, p(x1), 0.0, 0.0, 0, p(out), None, None) == -1 and b"finite" in dll.ddif_last_error()
        try:
            plan2.sample_dpm_guided(ops, "dpmsolver++", scale, x1, None)
            raise AssertionError("expected DdifError")
        except DdifError as e:
            assert "finite" in str(e)
    assert dll.ddif_plan_sample_dpm_guided(plan2.h, None, 1.5, p(x1), 0.0, 0.0, 0, p(out), None, None) == -1 and b"NULL" in dll.ddif_last_error()
    assert dll.ddif_plan_sample_dpm_guided(plan2.h, C.byref(prog), 1.5, None, 0.0, 0.0, 0, p(out), None, None) == -1
    assert dll.ddif_plan_sample_dpm_guided(plan2.h, C.byref(prog), 1.5, p(x1), 0.0, 0.0, 0, None, None, None) == -1
    bad, keep2 = plan2.dpm_program([ev, dict(up, m=[1, 0, 0])], "dpmsolver++")  # the program validation of ddif_plan_sample_dpm applies
    assert dll.ddif_plan_sample_dpm_guided(plan2.h, C.byref(bad), 1.5, p(x1), 0.0, 0.0, 0, p(out), None, None) == -1 and b"before it is written" in dll.ddif_last_error()
    try:  # x_T is Bg = 1 image, not the plan's 2
        plan2.sample_dpm_guided(ops, "dpmsolver++", 1.5, torch.zeros(2, C_, H, H, device=dev), None)
        raise AssertionError("expected DdifError")
    except DdifError as e:
        assert "x_T" in str(e)
    for B in (1, 3):  # an odd plan batch cannot hold [unconditional; conditional]
        plan = net.plan_for(B, H, H, dev)
        plan.set_cond(gc.tiles_for(ds, B, H, H, seed=2)["cond"].to(dev), force=True)
        assert dll.ddif_plan_sample_dpm_guided(plan.h, C.byref(prog), 1.5, p(x1), 0.0, 0.0, 0, p(out), None, None) == -1 and b"odd" in dll.ddif_last_error()
        try:
            plan.sample_dpm_guided(ops, "dpmsolver++", 1.5, x1, None)
            raise AssertionError("expected DdifError")
        except DdifError as e:
            assert "odd" in str(e)
    n0 = plan2.num_launches()
    good, inter = plan2.sample_dpm_guided(ops + [dict(kind="emit", src=0), dict(ev, kind="final"), dict(kind="emit", src=0)], "dpmsolver", 1.5, x1, (0.0, 1.0))
    assert good.shape == x1.shape and bool(torch.isfinite(good).all()) and inter.shape == (2,) + tuple(x1.shape) and torch.equal(inter[1], good)
    assert plan2.num_launches() == n0  # ddif_plan_num_launches does not change
    run_host_wrapper_validation()
