"""The checks of the DPM-Solver solver programs (singlestep / singlestep_fixed, solver_type="taylor", algorithm_type="dpmsolver", denoise_to_zero,
return_intermediate), shared by tests/test_dpmx_host.py (no kernels), tests/test_dpmx_emu.py (host-emulated build, CPU tensors) and tests/test_dpmx_gpu.py
(the gfx950 library).

Tolerances
  * schedule (orders, outer time steps, the time of every evaluation): both sides are the same fp32 torch expressions on the CPU -> torch.equal;
  * the elementwise forms of csrc/kernels_misc.h dpm_eval_update_kernel against `model_value_torch` / `update_torch` below, the torch restatement of the
    kernel's documented expressions (every scalar broadcast to a full tensor first, so that each torch op is one correctly rounded fp32 operation per
    element, as each kernel operation is with contraction off): bit equality;
  * samplers: the project's bar for unclamped solver iterates, 1e-4 * max(1, max|golden|), with the golden's own fp32 <-> fp64 gap asserted below a tenth of
    it (tools/make_golden.py refuses a noisier case);
  * batch against tiles alone, return_intermediate against the plain run, the plain multistep run against ddif_plan_sample_dpmpp: bit equality."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import golden_cases as gc
import golden_cases_dpmx as gx
import objective_parity as P

FORMS = {"none": 0, "multi": 1, "lin2": 2, "tay3": 3, "lin1": 4}  # include/ddif.h DDIF_DPM_FORM_* (0: the evaluation alone)


# ---- schedule: no kernels ------------------------------------------------------------------------------------------------------------------------------
def host_solver(case, model_fn=None):
    """The drop-in solver of a case over a model that is not a ddif network (default: zeros): the generic path, CPU tensors, no library."""
    from ddif.diffusion.diffusion_ddpm_pan import make_beta_schedule
    from ddif.solver.dpm_solver import DPM_Solver, NoiseScheduleVP

    betas = torch.as_tensor(make_beta_schedule(**gx.schedule_kwargs(case["schedule"], case["T"]))).float()
    ns = NoiseScheduleVP("discrete", betas=betas)
    return DPM_Solver(model_fn or (lambda x, t: torch.zeros_like(x)), ns, algorithm_type=case["algorithm"])


def record_run(slv, x, **kw):
    """Run slv.sample with the recorders tools/make_golden.py puts on the reference: (result, dict(eval_t, orders, timesteps_outer))."""
    rec = dict(eval_t=[], orders=[])
    model, gts, gos = slv.model, slv.get_time_steps, slv.get_orders_and_timesteps_for_singlestep_solver
    ssu, msu = slv.singlestep_dpm_solver_update, slv.multistep_dpm_solver_update

    def w_model(x_, t_):
        rec["eval_t"].append(t_.detach().reshape(-1)[:1].clone())
        return model(x_, t_)

    def w_gts(*a, **k):
        r = gts(*a, **k)
        rec.setdefault("first_grid", r.detach().clone())
        return r

    def w_gos(*a, **k):
        r = gos(*a, **k)
        rec["outer"] = r[0].detach().clone()
        return r

    def w_ssu(x_, s_, t_, order, **k):
        rec["orders"].append(int(order))
        return ssu(x_, s_, t_, order, **k)

    def w_msu(x_, ml, tl, t_, order, **k):
        rec["orders"].append(int(order))
        return msu(x_, ml, tl, t_, order, **k)
    slv.model, slv.get_time_steps, slv.get_orders_and_timesteps_for_singlestep_solver = w_model, w_gts, w_gos
    slv.singlestep_dpm_solver_update, slv.multistep_dpm_solver_update = w_ssu, w_msu
    out = slv.sample(x, **kw)
    return out, dict(eval_t=torch.cat(rec["eval_t"]), orders=rec["orders"], timesteps_outer=rec.get("outer", rec.get("first_grid")))


def program_of(slv, case, return_intermediate=False):
    ns = slv.noise_schedule
    return slv._build_program(case["steps"], case["order"], case["skip_type"], case["method"], True, case["denoise_to_zero"], case["solver_type"], return_intermediate,
                              ns.T, 1.0 / ns.total_N)


def run_host_schedule(case):
    """orders, timesteps_outer and the time of every evaluation of the drop-in -- on its generic path AND in the solver program it hands to the library --
    equal the arrays recorded from the reference."""
    g = P.load(case["cid"])
    want_t, want_o, want_outer = torch.from_numpy(g["eval_t"]), [int(v) for v in g["orders"]], torch.from_numpy(g["timesteps_outer"])
    assert want_t.dtype == torch.float32 and want_outer.dtype == torch.float32
    slv = host_solver(case)
    assert slv._fused_target() is None
    _, rec = record_run(slv, torch.zeros(1, 2, 4, 4), **gx.sample_kwargs(case))
    assert rec["orders"] == want_o, (case["cid"], rec["orders"], want_o)
    assert torch.equal(rec["timesteps_outer"], want_outer), (case["cid"], rec["timesteps_outer"], want_outer)
    assert torch.equal(rec["eval_t"], want_t), (case["cid"], rec["eval_t"], want_t)
    ops = program_of(host_solver(case), case)
    got = torch.cat([op["t"] for op in ops if op["kind"] in ("eval", "final")])
    assert got.dtype == torch.float32 and torch.equal(got, want_t), (case["cid"], got, want_t)
    assert sum(op["kind"] == "final" for op in ops) == int(case["denoise_to_zero"])
    per = case["order"] if case["method"] == "singlestep_fixed" else 1  # singlestep_fixed spends steps // order * order evaluations, the others all of `steps`
    assert len(got) == case["steps"] // per * per + int(case["denoise_to_zero"])


# ---- the elementwise forms --------------------------------------------------------------------------------------------------------------------------------
def _full(like, v):
    return torch.full_like(like, float(np.float32(v)))


def model_value_torch(o, x, lms, thr_rows, alpha, sigma, lo, hi, do_clamp, model_type, eps_only):
    a, s = _full(x, alpha), _full(x, sigma)
    if model_type == 0:
        eps = (x - a * o) / s
    elif model_type == 1:
        eps = o
    else:
        eps = a * o + s * x
    if eps_only:
        return eps
    x0 = (x - s * eps) / a
    if do_clamp:
        return torch.minimum(torch.maximum(x0 + lms, _full(x, lo)), _full(x, hi)) - lms
    if thr_rows is not None:
        return torch.minimum(torch.maximum(x0, -thr_rows), thr_rows) / thr_rows
    return x0


def update_torch(form, order, x, m0, m1, m2, c):
    c = [_full(x, v) for v in c]
    v = c[0] * x - c[1] * m0
    if form == "lin1" or (form == "multi" and order == 1):
        return v
    if form == "multi" and order == 2:
        return v - (_full(x, 0.5) * c[1]) * (c[2] * (m0 - m1))
    if form == "multi":
        d10, d11 = c[2] * (m0 - m1), c[3] * (m1 - m2)
        d1 = d10 + c[4] * (d10 - d11)
        d2 = c[5] * (d10 - d11)
        return (v + c[6] * d1) - c[7] * d2
    if form == "lin2":
        return v + c[2] * (c[3] * (m1 - m2))
    d10, d11 = c[3] * (m1 - m0), c[4] * (m2 - m0)
    d1 = (c[6] * d10 - c[5] * d11) / c[7]
    d2 = (_full(x, 2.0) * (d11 - d10)) / c[7]
    return (v + c[2] * d1) - c[8] * d2


def eval_update(lib, dev, net, xe, lms, thr, per, alpha, sigma, lo, hi, do_clamp, model_type, algorithm, form, order, x, ms, c, want_m=True):
    """include/ddif_testops.h ddif_dpm_eval_update -> (m_out, out) on the CPU; ms: three tensors or None (None = the value of this launch)."""
    fn = lib.dll.ddif_dpm_eval_update
    vp, f32, i32, i64 = C.c_void_p, C.c_float, C.c_int, C.c_int64
    fn.argtypes = [vp, vp, vp, vp, i64, i64, f32, f32, f32, f32, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.POINTER(C.c_float), vp, vp, vp]
    n = (net if net is not None else x).numel()
    dv = lambda t: None if t is None else t.to(dev).contiguous()
    net, xe, lms, thr, x = dv(net), dv(xe), dv(lms), dv(thr), dv(x)
    ms = [dv(m) for m in ms]
    m_out = torch.empty(n, dtype=torch.float32, device=dev) if (net is not None and want_m) else None
    out = torch.empty(n, dtype=torch.float32, device=dev)
    carr = (C.c_float * 9)(*[float(v) for v in list(c) + [0.0] * (9 - len(c))])
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = None if torch.device(dev).type != "cuda" else C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lib.check(fn(p(net), p(xe), p(lms), p(thr), n, per, alpha, sigma, lo, hi, int(do_clamp), model_type, algorithm, FORMS[form], order, p(x), p(ms[0]), p(ms[1]), p(ms[2]),
                 carr, p(m_out), p(out), stream), "ddif_dpm_eval_update")
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize(dev)
    return (None if m_out is None else m_out.cpu()), out.cpu()


def run_forms(lib, dev, n=1000):
    """Every form, both algorithms, every model_type and corrector, the fresh model value in every register position, and the update on its own."""
    g = torch.Generator().manual_seed(4242)
    rnd = lambda scale=1.0: torch.randn(n, generator=g) * scale
    net, xe, x, lms = rnd(), rnd(1.3), rnd(0.9), torch.rand(n, generator=g)
    old = [rnd(1.1), rnd(0.7), rnd(1.9)]
    per = n // 4
    thr = torch.tensor([0.31, 0.77, 1.0, 2.5])
    thr_rows = thr.repeat_interleave(per)
    alpha, sigma = float(np.float32(0.61803)), float(np.float32(0.78615))
    # r1 = 0.31, r2 = 0.69: r2 - r1 = 0.38 and every difference below is no power of two
    c9 = [0.9371, -0.2113, 0.4177, float(np.float32(1 / 0.31)), float(np.float32(1 / 0.69)), 0.31, 0.69, float(np.float32(0.69) - np.float32(0.31)), -0.0613]
    cm = [0.9371, -0.2113, 1.271, 0.853, 0.5931, 0.4713, 0.4177, -0.0613, 0.0]
    cl = [0.9371, -0.2113, -0.7391, 1.0, 0, 0, 0, 0, 0]
    cl3 = [0.9371, -0.2113, 0.7391, 1.271, 0, 0, 0, 0, 0]
    updates = [("multi", 1, cm), ("multi", 2, cm), ("multi", 3, cm), ("lin1", 0, cl), ("lin2", 0, cl), ("lin2", 0, cl3), ("tay3", 0, c9)]
    checked = 0
    for algorithm in (0, 1):
        for model_type in (0, 1, 2):
            for corr in ("none", "clamp", "thr"):
                if algorithm == 1 and corr != "none":
                    continue  # (the library never hands a corrector to a noise-prediction evaluation; the final denoise runs as algorithm 0)
                do_clamp, th = corr == "clamp", (thr if corr == "thr" else None)
                want_m = model_value_torch(net, xe, lms, thr_rows if corr == "thr" else None, alpha, sigma, 0.0, 1.0, do_clamp, model_type, algorithm == 1)
                m, o = eval_update(lib, dev, net, xe, lms, th, per, alpha, sigma, 0.0, 1.0, do_clamp, model_type, algorithm, "none", 0, None, [None] * 3, [])
                assert torch.equal(m, want_m) and torch.equal(o, want_m), ("model value", algorithm, model_type, corr)
                for form, order, c in updates:
                    nm = order if form == "multi" else 1 if form == "lin1" else 3
                    for fresh in range(nm):  # which model register this launch writes
                        ms = [None if j == fresh else old[j] for j in range(3)]
                        mt = [want_m if j == fresh else old[j] for j in range(3)]
                        want = update_torch(form, order, x, mt[0], mt[1], mt[2], c)
                        m, o = eval_update(lib, dev, net, xe, lms, th, per, alpha, sigma, 0.0, 1.0, do_clamp, model_type, algorithm, form, order, x, ms, c)
                        assert torch.equal(m, want_m), ("stored model value", form, order, fresh)
                        assert torch.equal(o, want), ("fused update", algorithm, model_type, corr, form, order, fresh, float((o - want).abs().max()))
                        checked += 1
    for form, order, c in updates:  # the update alone: the second kernel of the two-kernel composition
        want = update_torch(form, order, x, old[0], old[1], old[2], c)
        _, o = eval_update(lib, dev, None, None, None, None, per, alpha, sigma, 0.0, 1.0, False, 0, 0, form, order, x, old, c)
        assert torch.equal(o, want), ("update alone", form, order)
    assert not torch.equal(update_torch("tay3", 0, x, old[0], old[1], old[2], c9), update_torch("lin2", 0, x, old[0], old[1], old[2], cl))
    print(f"dpm_eval_update_kernel: {checked} fused (model value, update) combinations and {len(updates)} updates alone equal torch bit for bit on {n} values")


# ---- goldens through the drop-in --------------------------------------------------------------------------------------------------------------------------
def solver_for(case, dev, B=1, corrector="case", **solver_kw):
    """(solver, x_T, cond, diffusion) of a case on `dev` with B tiles (tile 0 is the golden's)."""
    from ddif.diffusion.diffusion_ddpm_pan import GaussianDiffusion, make_beta_schedule
    from ddif.solver.dpm_solver import DPM_Solver, ImageSpaceClamp, NoiseScheduleVP, model_wrapper

    ds, H, T, seed = case["ds"], case["H"], case["T"], case["seed"]
    C_ = gc.DATASETS[ds][0]
    cond = gc.tiles_for(ds, 1, H, H, seed=seed)["cond"]
    xT = torch.randn(1, C_, H, H, generator=torch.Generator().manual_seed(seed))
    if B > 1:
        more = gc.tiles_for(ds, B - 1, H, H, seed=seed + 1)["cond"]
        cond = torch.cat([cond, more])
        xT = torch.cat([xT, torch.randn(B - 1, C_, H, H, generator=torch.Generator().manual_seed(seed + 1))])
    cond, xT = cond.to(dev).contiguous(), xT.to(dev).contiguous()
    d = GaussianDiffusion(P.net_for(ds, dev), image_size=H, channels=C_, pred_mode=gx.PRED_OF_MODEL_TYPE[case["model_type"]], loss_type="l2", device=dev, clamp_range=(0, 1))
    d.set_new_noise_schedule(betas=make_beta_schedule(**gx.schedule_kwargs(case["schedule"], T)), device=dev)
    ns = NoiseScheduleVP("discrete", betas=d.betas)
    fn = model_wrapper(d.model, ns, model_type=case["model_type"], guidance_type="classifier-free", guidance_scale=1.0, condition=cond)
    which = case["corrector"] if corrector == "case" else corrector
    corr = {"clamp": ImageSpaceClamp(cond[:, :C_], 0.0, 1.0), "dyn": "dynamic_thresholding", None: None}[which]
    return DPM_Solver(fn, ns, algorithm_type=case["algorithm"], correcting_x0_fn=corr, **solver_kw), xT, cond, d


class forward_forbidden:
    """UNetSR3.forward raises inside: a run that falls to the per-evaluation Python loop fails."""

    def __enter__(self):
        from ddif.models.sr3_dwt import UNetSR3

        self.cls, self.fwd = UNetSR3, UNetSR3.forward

        def boom(*a, **k):
            raise AssertionError("UNetSR3.forward was called: the run left the library")
        UNetSR3.forward = boom

    def __exit__(self, *a):
        self.cls.forward = self.fwd


def tolerance(g):
    return 1e-4 * max(1.0, float(np.abs(g["out"]).max()))


def _reset(d, B, H, dev):
    d.model.plan_for(B, H, H, dev).set_threshold("off")  # (plans are shared between tests, and the switch is sticky)


def run_golden(case, dev, check_inter=True):
    g = P.load(case["cid"])
    ref, tol = torch.from_numpy(g["out"]), tolerance(g)
    P.check_gap(g["gap"], tol, case["cid"])
    slv, xT, cond, d = solver_for(case, dev)
    try:
        assert slv._fused_target() is not None
        with forward_forbidden():
            out = slv.sample(xT, **gx.sample_kwargs(case))
        err = float((out.cpu() - ref).abs().max())
        print(f"{case['cid']}: max|out - golden| {err:.3e} (max|golden| {float(ref.abs().max()):.3g}, tolerance {tol:.3e})")
        assert bool(torch.isfinite(out).all())
        assert err <= tol, (case["cid"], err, tol)
        if case["inter"] and check_inter:
            want = torch.from_numpy(g["inter"])
            with forward_forbidden():
                out2, inter = slv.sample(xT, return_intermediate=True, **gx.sample_kwargs(case))
            assert torch.equal(out2, out), "return_intermediate changes the result"
            assert isinstance(inter, list) and len(inter) == want.shape[0]
            got = torch.stack([t.cpu() for t in inter])
            ierr = float((got - want).abs().max())
            itol = 1e-4 * max(1.0, float(want.abs().max()))
            print(f"{case['cid']}: intermediates max|inter - golden| {ierr:.3e} (max|golden| {float(want.abs().max()):.3g}, tolerance {itol:.3e})")
            assert ierr <= itol, (case["cid"], ierr, itol)
            assert torch.equal(inter[-1], out)
    finally:
        _reset(d, 1, case["H"], dev)
    return out


def run_intermediates_multistep(dev):
    """Multistep: the stack starts with the initial x (:1190-1191) and ends, after the final denoise, with the result; the run's result is the plain run's."""
    case = dict(gx.BY_ID["dpmx_pp_ms_o3_s6_x_start_d2z"])
    slv, xT, cond, d = solver_for(case, dev)
    with forward_forbidden():
        out = slv.sample(xT, **gx.sample_kwargs(case))
        out2, inter = slv.sample(xT, return_intermediate=True, **gx.sample_kwargs(case))
    assert torch.equal(out, out2)
    assert len(inter) == case["steps"] + 2 and torch.equal(inter[0], xT) and torch.equal(inter[-1], out)


def run_batch_equals_tiles(dev, B=3):
    """Singlestep order 3, 5 evaluations (orders 3, 2), both algorithms: a batch of three 16 x 16 tiles equals each tile alone, bit for bit."""
    for cid in ("dpmx_pp_ss_o3_s12_noise", "dpmx_np_ss_o3_s12_noise"):
        case = dict(gx.BY_ID[cid], steps=5)
        slv, xT, cond, d = solver_for(case, dev, B=B)
        with forward_forbidden():
            whole = slv.sample(xT, **gx.sample_kwargs(case)).clone()
        for b in range(B):
            from ddif.solver.dpm_solver import DPM_Solver, ImageSpaceClamp, model_wrapper

            cb = cond[b:b + 1].contiguous()
            fn = model_wrapper(d.model, slv.noise_schedule, model_type=case["model_type"], guidance_type="classifier-free", guidance_scale=1.0, condition=cb)
            corr = ImageSpaceClamp(cb[:, :xT.shape[1]], 0.0, 1.0) if case["corrector"] == "clamp" else None
            one = DPM_Solver(fn, slv.noise_schedule, algorithm_type=case["algorithm"], correcting_x0_fn=corr)
            with forward_forbidden():
                alone = one.sample(xT[b:b + 1].contiguous(), **gx.sample_kwargs(case))
            assert torch.equal(alone, whole[b:b + 1]), (cid, b, float((alone - whole[b:b + 1]).abs().max()))


def run_generic_agrees(case, dev):
    """correcting_xt_fn = identity forces the reference's loop over the update methods (the network through its front door): within the tolerance of the fused run."""
    g = P.load(case["cid"])
    tol = tolerance(g)
    slv, xT, cond, d = solver_for(case, dev)
    with forward_forbidden():
        fused = slv.sample(xT, **gx.sample_kwargs(case))
    gen, _, _, _ = solver_for(case, dev)
    gen.correcting_xt_fn = lambda x, t, step: x
    assert gen._fused_target() is None
    generic = gen.sample(xT, **gx.sample_kwargs(case))
    err = float((fused - generic).abs().max())
    print(f"{case['cid']}: max|fused - generic| {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol, (case["cid"], err, tol)


def run_plain_multistep_unchanged(dev):
    """The plain multistep DPM-Solver++ run still goes through ddif_plan_sample_dpmpp: DPM_Solver.sample equals PlanHandle.sample_dpmpp called directly with
    tables built here, bit for bit, and sample_dpm is not reached."""
    from ddif.runtime import PlanHandle

    cid, ds, H, W, T, steps, order, seed = [c for c in gc.DPM_CASES if c[0] == "dpm_wv3_16_T500_s12_o3"][0]
    case = dict(cid=cid, ds=ds, H=H, T=T, seed=seed, schedule="cosine", algorithm="dpmsolver++", model_type="x_start", corrector="clamp")
    slv, xT, cond, d = solver_for(case, dev)
    calls = []
    orig = PlanHandle.sample_dpm
    PlanHandle.sample_dpm = lambda self, *a, **k: calls.append(1) or orig(self, *a, **k)
    try:
        with forward_forbidden():
            out = slv.sample(xT, steps=steps, order=order, skip_type="time_uniform", method="multistep").clone()
    finally:
        PlanHandle.sample_dpm = orig
    assert not calls
    g = P.load(cid)
    assert float((out.cpu() - torch.from_numpy(g["out"])).abs().max()) <= 1e-4 * max(1.0, float(np.abs(g["out"]).max()))
    ns = slv.noise_schedule
    ts = slv.get_time_steps("time_uniform", ns.T, 1.0 / ns.total_N, steps)
    ords = [min(k + 1, order) for k in range(steps)]
    coefs = [slv._update_coefs([ts[j].reshape(1) for j in range(max(0, k - 2), k + 1)], ts[k + 1].reshape(1), ords[k]) for k in range(steps)]
    keys = ("cx", "a_phi1", "inv_r0", "inv_r1", "r0_frac", "inv_r01", "a_phi2", "a_phi3")
    tabs = dict(n_evals=steps, order=order, t_model=[float((ts[k] - 1.0 / ns.total_N) * 1000.0) for k in range(steps)],
                alpha=[float(ns.marginal_alpha(ts[k].reshape(1))) for k in range(steps)], sigma=[float(ns.marginal_std(ts[k].reshape(1))) for k in range(steps)], ord=ords,
                **{k: [c[k] for c in coefs] for k in keys})
    plan = d.model.plan_for(1, H, H, dev)
    direct = plan.sample_dpmpp(tabs, xT, (0.0, 1.0))
    assert torch.equal(direct, out)


# ---- program validation -----------------------------------------------------------------------------------------------------------------------------------
def run_validation(dev):
    from ddif import DdifError
    from ddif.runtime import DpmProgram

    ds, H = "wv3", 16
    C_ = gc.DATASETS[ds][0]
    net = P.net_for(ds, dev)
    plan = net.plan_for(1, H, H, dev)
    plan.set_cond(gc.tiles_for(ds, 1, H, H, seed=2)["cond"].to(dev), force=True)
    plan.set_threshold("off")
    plan.set_objective("x_start", plan.objective[1])
    xT = torch.zeros(1, C_, H, H, device=dev)
    ev = lambda src, dst, kind="eval": dict(kind=kind, t_model=400.0, alpha=0.8, sigma=0.6, src=src, dst=dst)
    up = lambda form, order, src, dst, m: dict(kind="update", form=form, order=order, src=src, dst=dst, m=m, c=[0.9, -0.2, 0.1, 1.0])
    bad = [
        ("before it is written", [ev(1, 0)]),                                            # state register 1 evaluated before any update wrote it
        ("before it is written", [ev(0, 0), up("lin2", 0, 0, 0, [0, 1, 0])]),             # model register 1 read, never written
        ("before it is written", [up("lin1", 0, 0, 0, [0, 0, 0]), ev(0, 0)]),             # the update precedes the evaluation it needs
        ("before it is written", [ev(0, 0), dict(kind="emit", src=2)]),
        ("order", [ev(0, 0), up("multi", 4, 0, 0, [0, 0, 0])]),
        ("order", [ev(0, 0), up("multi", 0, 0, 0, [0, 0, 0])]),
        ("register", [ev(0, 3)]),
        ("register", [ev(0, 0), up("lin1", 0, 0, -1, [0, 0, 0])]),
        ("register", [ev(0, 0), up("lin2", 0, 0, 0, [0, 7, 0])]),
        ("inter_out", None),                                                              # an emit without a stack: through the raw entry point below
    ]
    for needle, ops in bad:
        if ops is None:
            continue
        try:
            plan.sample_dpm(ops, "dpmsolver++", xT, None)
            raise AssertionError(f"expected DdifError for {ops}")
        except DdifError as e:
            assert "status -1" in str(e) and needle in str(e), (needle, str(e))
    dll = plan.lib.dll
    out = torch.empty_like(xT)
    p = lambda t: C.c_void_p(t.data_ptr())
    prog, keep = plan.dpm_program([ev(0, 0), up("lin1", 0, 0, 0, [0, 0, 0]), dict(kind="emit", src=0)], "dpmsolver++")
    assert dll.ddif_plan_sample_dpm(plan.h, C.byref(prog), p(xT), 0.0, 0.0, 0, p(out), None, None) == -1 and b"inter_out" in dll.ddif_last_error()
    assert dll.ddif_plan_sample_dpm(plan.h, None, p(xT), 0.0, 0.0, 0, p(out), None, None) == -1                       # no program
    null_ops = DpmProgram(2, 0, None)
    assert dll.ddif_plan_sample_dpm(plan.h, C.byref(null_ops), p(xT), 0.0, 0.0, 0, p(out), None, None) == -1 and b"NULL" in dll.ddif_last_error()  # a null table
    prog, keep = plan.dpm_program([ev(0, 0), up("lin1", 0, 0, 0, [0, 0, 0])], "dpmsolver++")
    prog.algorithm = 2
    assert dll.ddif_plan_sample_dpm(plan.h, C.byref(prog), p(xT), 0.0, 0.0, 0, p(out), None, None) == -1
    prog.algorithm, prog.n_ops = 0, 0
    assert dll.ddif_plan_sample_dpm(plan.h, C.byref(prog), p(xT), 0.0, 0.0, 0, p(out), None, None) == -1
    keep[0].kind = 9
    prog.n_ops = 2
    assert dll.ddif_plan_sample_dpm(plan.h, C.byref(prog), p(xT), 0.0, 0.0, 0, p(out), None, None) == -1
    try:
        plan.set_threshold("solver", 0.995, 1.0)
        try:
            plan.sample_dpm([ev(0, 0), up("lin1", 0, 0, 0, [0, 0, 0])], "dpmsolver++", xT, (0.0, 1.0))  # mode 2 together with the image-space clamp
            raise AssertionError("expected DdifError")
        except DdifError as e:
            assert "clamp" in str(e)
    finally:
        plan.set_threshold("off")
    n0 = plan.num_launches()
    good, inter = plan.sample_dpm([ev(0, 0), up("lin1", 0, 0, 1, [0, 0, 0]), ev(1, 1), up("lin2", 0, 0, 0, [0, 1, 0]), dict(kind="emit", src=0), ev(0, 0, "final"),
                                   dict(kind="emit", src=0)], "dpmsolver", xT, (0.0, 1.0))
    assert bool(torch.isfinite(good).all()) and inter.shape == (2,) + tuple(xT.shape) and torch.equal(inter[1], good)
    assert plan.num_launches() == n0  # ddif_plan_num_launches does not change
