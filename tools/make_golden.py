#!/usr/bin/env python3
"""Generate tests/golden/*.npz|json by running the REAL reference (imported from /root/reference) on the seeded
cases of tests/golden_cases.py.  Runs only in the build container; the reference never travels.  Nothing but
numeric vectors (inputs' checksums, expected outputs) and the reference's state-dict key/shape manifest is
written into the repository.

    python tools/make_golden.py [--only fwd,sched,ddpm,ddim,dpm,loss,psnr] [--skip-long]
    python tools/make_golden.py --only ddpmbig,dpmbig,ddpmfull     (round 6: the config-exact cases; not part of the default set)
    python tools/make_golden.py --only objective                   (pred_mode noise / pred_v, l2, p2 weighting: tests/golden_cases_objective.py;
                                                                    each output also from an fp64 run of the reference; not part of the default set)
    python tools/make_golden.py --only dynthresh                   (clamp_type="dynamic" / correcting_x0_fn="dynamic_thresholding": tests/golden_cases_dynthresh.py;
                                                                    fp32 + fp64 as above, plus the reference's quantile per (step, sample); not part of the default set)
    python tools/make_golden.py --only l1ssim                      (loss_type="l1ssim": the HybridL1SSIM operator, p_losses and its backward pass:
                                                                    tests/golden_cases_l1ssim.py; fp32 + fp64 as above; not part of the default set)
    python tools/make_golden.py --only dpmx                        (DPM-Solver singlestep / singlestep_fixed, solver_type="taylor", algorithm_type="dpmsolver",
                                                                    denoise_to_zero, return_intermediate: tests/golden_cases_dpmx.py; fp32 + fp64 as above,
                                                                    plus orders, outer time steps and the time of every evaluation; not part of the default set)
    python tools/make_golden.py --only cfg                         (classifier-free guidance in DPM-Solver runs: tests/golden_cases_cfg.py; fp32 + fp64 as above,
                                                                    plus the time of every evaluation; not part of the default set)
    python tools/make_golden.py --only q2n                         (the Q2n index: tests/golden_cases_q2n.py; block values from a composition of the reference's
                                                                    norm_blocco / onion_mult / onion_mult2D in fp64, with each block's sensitivity to summation
                                                                    order; not part of the default set)
"""
import argparse
import json
import os
import random
import sys
import time
import types

sys.dont_write_bytecode = True
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_cases as gc  # noqa: E402

REF = os.environ.get("DDIF_REFERENCE", "/root/reference")


def import_reference():
    class DropPath(nn.Module):  # stand-in for timm.models.layers.DropPath (timm is not installed)
        def __init__(self, drop_prob=0.0, scale_by_keep=True):
            super().__init__()
            self.drop_prob, self.scale_by_keep = drop_prob, scale_by_keep

        def forward(self, x):
            if self.drop_prob == 0.0 or not self.training:
                return x
            keep = 1 - self.drop_prob
            m = x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep)
            return x * (m.div_(keep) if self.scale_by_keep and keep > 0 else m)

    for name in ("timm", "timm.models", "timm.models.layers"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["timm.models.layers"].DropPath = DropPath
    sys.path.insert(0, REF)
    import builtins

    _print = builtins.print
    builtins.print = lambda *a, **k: None  # the constructor prints "use attn: res 8"
    try:
        from models.sr3_dwt import UNetSR3
        from diffusion import diffusion_ddpm_pan as D
        from solver import dpm_solver as S
    finally:
        builtins.print = _print
    D.tqdm = lambda it, **kw: it
    return UNetSR3, D, S


def build_ref_net(UNetSR3, ds):
    cfg = gc.cfg_for(ds)
    import builtins

    _print = builtins.print
    builtins.print = lambda *a, **k: None
    try:
        net = UNetSR3(
            in_channel=cfg["in_channel"], out_channel=cfg["out_channel"], lms_channel=cfg["lms_channel"],
            pan_channel=cfg["pan_channel"], inner_channel=32, norm_groups=1, channel_mults=(1, 2, 2, 4),
            attn_res=(8,), dropout=0.2, image_size=64, self_condition=True)
    finally:
        builtins.print = _print
    net.load_state_dict(gc.weights_for(ds), strict=True)
    net.eval()
    return net


def chk(t):
    return float(t.double().sum()), float(t.double().abs().max())


def save(name, **arrs):
    path = os.path.join(gc.GOLDEN_DIR, name + ".npz")
    np.savez(path, **{k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()})
    print(f"  wrote {os.path.relpath(path, ROOT)} ({os.path.getsize(path) / 1024:.0f} KiB)")


def make_diffusion(D, net, C, T, size):
    d = D.GaussianDiffusion(net, image_size=size, channels=C, pred_mode="x_start", loss_type="l1", device="cpu",
                            clamp_range=(0, 1))
    d.set_new_noise_schedule(betas=D.make_beta_schedule(schedule="cosine", n_timestep=T, cosine_s=8e-3))
    return d


def make_objective(UNetSR3, D, S, net_for):
    """The noise / v parameterisations (tests/golden_cases_objective.py).  Every case runs twice: the reference as it is (fp32: the expected output)
    and the reference in fp64 -- net and diffusion `.double()`, `net.forward` wrapped to cast x / self_cond (the diffusion calls `model.forward`
    directly, so module hooks on the net do not fire), the positional encoding's output cast -- with the same fp32 random draws.  `<key>_f64` and
    `gap::<key>` = max|fp32 - fp64| put the case's own noise floor on file."""
    import copy

    import golden_cases_objective as go

    nets64 = {}

    def net64_for(ds):
        if ds not in nets64:
            n = copy.deepcopy(net_for(ds)).double()
            fwd = n.forward
            n.forward = lambda x, t, cond=None, self_cond=None: fwd(x.double(), t, None if cond is None else cond.double(), None if self_cond is None else self_cond.double())
            n.noise_level_mlp[0].register_forward_hook(lambda m, i, o: o.double())
            nets64[ds] = n
        return nets64[ds]

    def diffusion(ds, T, size, pred_mode, loss_type="l2", gamma=0.0, f64=False, schedule=None):
        net = net64_for(ds) if f64 else net_for(ds)
        d = D.GaussianDiffusion(net, image_size=size, channels=gc.DATASETS[ds][0], pred_mode=pred_mode, loss_type=loss_type, device="cpu", clamp_range=(0, 1),
                                p2_loss_weight_gamma=gamma)
        d.set_new_noise_schedule(betas=D.make_beta_schedule(**(schedule or dict(schedule="cosine", n_timestep=T, cosine_s=8e-3))))
        return d.double() if f64 else d

    too_noisy = []

    def both(run):
        a, b = run(False), run(True)
        gap = float((a.double() - b).abs().max())
        return a, b, gap

    def report(cid, gap, ref, tol):
        print(f"  {cid}: fp32-fp64 gap {gap:.2e}, max|golden| {ref:.3g}, tolerance {tol:.2e} -> gap / tolerance = {gap / tol:.3f}")
        if gap > 0.1 * tol:
            too_noisy.append(cid)

    for stem, ds, B, H, W, T, seed in go.DDPM_CASES:
        cond = gc.tiles_for(ds, B, H, W, seed=seed)["cond"]
        for pm in go.PRED_MODES:
            def run(f64):
                d = diffusion(ds, T, H, pm, f64=f64)  # (before seeding: building a net draws from the generator)
                torch.manual_seed(seed)
                return d(cond.double() if f64 else cond, mode="ddpm_sample")
            out, out64, gap = both(run)
            report(f"{stem}_{pm}", gap, float(out.abs().max()), 1e-4)
            save(f"{stem}_{pm}", out=out, out_f64=out64, gap=gap, cond_chk=chk(cond))

    for stem, ds, B, H, W, T, sect, seed in go.DDIM_CASES:
        cond = gc.tiles_for(ds, B, H, W, seed=seed)["cond"]
        for pm in go.PRED_MODES:
            def run(f64):
                d = diffusion(ds, T, H, pm, f64=f64)
                torch.manual_seed(seed)
                return d(cond.double() if f64 else cond, mode="ddim_sample", section_counts=sect)
            out, out64, gap = both(run)
            report(f"{stem}_{pm}", gap, float(out.abs().max()), 1e-4 * max(1.0, float(out.abs().max())))
            save(f"{stem}_{pm}", out=out, out_f64=out64, gap=gap, cond_chk=chk(cond))

    for stem, ds, H, W, T, steps, order, seed in go.DPM_CASES:
        C = gc.DATASETS[ds][0]
        cond = gc.tiles_for(ds, 1, H, W, seed=seed)["cond"]
        xT = torch.randn(1, C, H, W, generator=torch.Generator().manual_seed(seed))
        for pm in go.PRED_MODES:
            def run(f64):
                d = diffusion(ds, T, H, pm, f64=f64, schedule=go.dpm_schedule(pm, T))
                cnd, x = (cond.double(), xT.double()) if f64 else (cond, xT)
                # the schedule scalars (alpha, sigma, lambda, the float model time) stay in the solver's own fp32 in both runs: the twin doubles the
                # tensor arithmetic -- net and diffusion -- and nothing else
                ns = S.NoiseScheduleVP("discrete", betas=d.betas.float())
                lms = cnd[:, :C]
                fn = S.model_wrapper(d.model, ns, model_type=go.MODEL_TYPE[pm], guidance_type="classifier-free", guidance_scale=1.0, condition=cnd)
                slv = S.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", correcting_x0_fn=lambda x0, t, lms=lms: (x0 + lms).clamp(0, 1.0) - lms)
                with torch.no_grad():
                    return slv.sample(x, steps=steps, order=order, skip_type="time_uniform", method="multistep")
            out, out64, gap = both(run)
            report(f"{stem}_{pm}", gap, float(out.abs().max()), 1e-4 * max(1.0, float(out.abs().max())))
            save(f"{stem}_{pm}", out=out, out_f64=out64, gap=gap, cond_chk=chk(cond))

    def pinned(tt, sc_branch):
        class Pin:
            def __enter__(self):
                self.ri, self.rr = torch.randint, random.random
                D.torch.randint = lambda *a, **k: tt
                D.random.random = (lambda: 0.0) if sc_branch else (lambda: 1.0)

            def __exit__(self, *a):
                D.torch.randint, D.random.random = self.ri, self.rr
        return Pin()

    for stem, ds, B, H, W, T, tvals, sc_branch, seed in go.LOSS_CASES:
        C = gc.DATASETS[ds][0]
        tiles = gc.tiles_for(ds, B, H, W, seed=seed)
        cond, res = tiles["cond"], tiles["gt"] - tiles["lms"]
        noise = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed))
        tt = torch.tensor(tvals, dtype=torch.long)
        for pm in go.PRED_MODES:
            arrs = {}
            for lt in go.LOSS_TYPES:
                for gamma in go.P2_GAMMAS:
                    res32 = {}

                    def run(f64, what):
                        if (f64, "done") not in res32:
                            d = diffusion(ds, T, H, pm, loss_type=lt, gamma=gamma, f64=f64)
                            with pinned(tt, sc_branch), torch.no_grad():
                                cast = (lambda v: v.double()) if f64 else (lambda v: v)
                                loss, recon = d(cast(res), mode="train", noise=cast(noise), cond=cast(cond))
                            res32[(f64, "loss")], res32[(f64, "recon")], res32[(f64, "done")] = loss.reshape(1), recon, True
                        return res32[(f64, what)]
                    k = go.loss_key(lt, gamma)
                    loss, loss64, gl = both(lambda f64: run(f64, "loss"))
                    recon, recon64, gr = both(lambda f64: run(f64, "recon"))
                    report(f"{stem}_{pm} {k} loss", gl, float(loss), 1e-6)
                    report(f"{stem}_{pm} {k} recon", gr, float(recon.abs().max()), 2e-5)
                    arrs.update({f"loss_{k}": loss, f"loss_{k}_f64": loss64, f"gap::loss_{k}": gl, f"recon_{k}": recon, f"recon_{k}_f64": recon64, f"gap::recon_{k}": gr})
            save(f"{stem}_{pm}", cond_chk=chk(cond), **arrs)

    for cid, ds, B, H, W, T, tvals, pm, lt, gamma, seed in go.GRAD_CASES:
        C = gc.DATASETS[ds][0]
        tiles = gc.tiles_for(ds, B, H, W, seed=seed)
        cond, res = tiles["cond"], tiles["gt"] - tiles["lms"]
        noise = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed))
        tt = torch.tensor(tvals, dtype=torch.long)
        drops, paths = [], []

        def run(f64):
            d = diffusion(ds, T, H, pm, loss_type=lt, gamma=gamma, f64=f64)
            net = d.model
            hooks, k = [], [0, 0]
            for m in net.modules():  # fp32 run: capture the masks (execution order); fp64 run: impose them
                if isinstance(m, nn.Dropout):
                    if not f64:
                        hooks.append(m.register_forward_hook(lambda mod, inp, out: drops.append(((out != 0) | (inp[0] == 0)).detach())))
                    else:
                        def imp(mod, inp, out):
                            k[0] += 1
                            return inp[0] * drops[k[0] - 1].double() / (1 - mod.p)
                        hooks.append(m.register_forward_hook(imp))
                elif type(m).__name__ == "DropPath":
                    if not f64:
                        hooks.append(m.register_forward_hook(lambda mod, inp, out: paths.append(((out.detach().flatten(1).abs().sum(1) != 0).float() / (1 - mod.drop_prob)))))
                    else:
                        def impp(mod, inp, out):
                            k[1] += 1
                            return inp[0] * paths[k[1] - 1].double().reshape(-1, 1, 1, 1)
                        hooks.append(m.register_forward_hook(impp))
            net.train()
            for prm in net.parameters():
                prm.requires_grad_(True)
                prm.grad = None
            torch.manual_seed(seed)
            cast = (lambda v: v.double()) if f64 else (lambda v: v)
            try:
                with pinned(tt, False):
                    loss, recon = d(cast(res), mode="train", noise=cast(noise), cond=cast(cond))
                loss.backward()
            finally:
                net.eval()
                for hk in hooks:
                    hk.remove()
            names = [n for n, _ in net.named_parameters()]
            norms = np.array([float(prm.grad.double().norm()) if prm.grad is not None else -1.0 for _, prm in net.named_parameters()], dtype=np.float64)
            full = {"grad::" + n: prm.grad.detach().clone() for n, prm in net.named_parameters() if any(n == f or n.startswith(f) for f in go.TRAIN_GRAD_FULL)}
            for prm in net.parameters():
                prm.grad = None
                prm.requires_grad_(False)
            return float(loss.detach()), recon.detach(), names, norms, full

        loss, recon, names, norms, full = run(False)
        loss64, recon64, _, norms64, full64 = run(True)
        rel = float(np.max(np.abs(norms - norms64) / np.maximum(norms64, 1e-4)))
        gfull = max(float((full[k].double() - full64[k]).abs().max()) / max(float(full64[k].abs().max()), 1e-5) for k in full)
        print(f"  {cid}: loss gap {abs(loss - loss64):.2e} (tolerance 1e-6), worst relative grad-norm gap {rel:.2e} (tolerance 2e-4), worst relative full-gradient gap {gfull:.2e} (tolerance 5e-5)")
        if not (abs(loss - loss64) <= 1e-7 and rel <= 2e-5 and gfull <= 5e-6):
            too_noisy.append(cid)
        arrs = {f"drop_{k}": np.packbits(d_.numpy().reshape(-1)) for k, d_ in enumerate(drops)}
        arrs.update({f"drop_{k}_shape": np.array(d_.shape) for k, d_ in enumerate(drops)})
        save(cid, loss=loss, loss_f64=loss64, recon=recon, recon_f64=recon64, n_drop=len(drops), paths=torch.stack(paths), p_drop=0.2, names=np.array(names), grad_norms=norms,
             grad_norms_f64=norms64, **{"gap::loss": abs(loss - loss64), "gap::grad_norms_rel": rel, "gap::grad_full_rel": gfull}, **arrs, **full)
    assert not too_noisy, f"the reference's own fp32-fp64 gap exceeds a tenth of the tolerance: change these cases: {too_noisy}"


def make_dynthresh(UNetSR3, D, S, net_for):
    """Dynamic thresholding (tests/golden_cases_dynthresh.py).  As make_objective: the reference as it is (fp32: the expected output) and its fp64 twin with the
    same fp32 random draws; `quant` = what torch.quantile returned inside the fp32 run's dynamic_thresholding_fn, per (step, sample), in execution order."""
    import copy

    import golden_cases_dynthresh as gd

    nets64 = {}

    def net64_for(ds):
        if ds not in nets64:
            n = copy.deepcopy(net_for(ds)).double()
            fwd = n.forward
            n.forward = lambda x, t, cond=None, self_cond=None: fwd(x.double(), t, None if cond is None else cond.double(), None if self_cond is None else self_cond.double())
            n.noise_level_mlp[0].register_forward_hook(lambda m, i, o: o.double())
            nets64[ds] = n
        return nets64[ds]

    def diffusion(ds, T, size, pred_mode, f64, schedule=None, clamp_type="dynamic"):
        net = net64_for(ds) if f64 else net_for(ds)
        d = D.GaussianDiffusion(net, image_size=size, channels=gc.DATASETS[ds][0], pred_mode=pred_mode, loss_type="l2", device="cpu", clamp_range=(0, 1),
                                clamp_type=clamp_type)
        d.set_new_noise_schedule(betas=D.make_beta_schedule(**(schedule or dict(schedule="cosine", n_timestep=T, cosine_s=8e-3))))
        return d.double() if f64 else d

    def record(obj, quant):
        """Wrap obj.dynamic_thresholding_fn (an instance attribute shadows the method; DPM_Solver stored the bound method already, so patch that slot too)."""
        orig = obj.dynamic_thresholding_fn

        def wrapped(x0, t):
            quant.append(torch.quantile(torch.abs(x0).reshape((x0.shape[0], -1)), obj.dynamic_thresholding_ratio, dim=1).detach().clone())
            return orig(x0, t)
        obj.dynamic_thresholding_fn = wrapped
        if getattr(obj, "correcting_x0_fn", None) is not None:
            obj.correcting_x0_fn = wrapped

    too_noisy, idle = [], []

    def finish(cid, run, max_val, expect_active, tol_of, cond):
        q32, q64 = [], []
        out, out64 = run(False, q32), run(True, q64)
        gap = float((out.double() - out64).abs().max())
        tol = tol_of(out)
        quant = torch.stack(q32).float()
        frac = gd.active_fraction(quant.numpy(), max_val)
        print(f"  {cid}: fp32-fp64 gap {gap:.2e}, max|golden| {float(out.abs().max()):.3g}, tolerance {tol:.2e} -> gap / tolerance = {gap / tol:.3f}; quantile "
              f"{float(quant.min()):.4g} .. {float(quant.max()):.4g}, above max_val {max_val} in {int(round(frac * quant.numel()))} of {quant.numel()} (step, sample) pairs")
        if gap > 0.1 * tol:
            too_noisy.append(cid)
        if expect_active and frac < 0.5:
            idle.append(cid)
        save(cid, out=out, out_f64=out64, gap=gap, quant=quant, max_val=max_val, cond_chk=chk(cond))

    for cid, ds, B, H, W, T, pm, seed, expect_active in gd.DDPM_CASES:
        cond = gc.tiles_for(ds, B, H, W, seed=seed)["cond"]

        def run(f64, quant):
            d = diffusion(ds, T, H, pm, f64)  # (before seeding: building a net draws from the generator)
            record(d, quant)
            torch.manual_seed(seed)
            return d(cond.double() if f64 else cond, mode="ddpm_sample")
        finish(cid, run, 1.0, expect_active, lambda out: 1e-4, cond)

    for cid, ds, H, W, T, steps, order, mt, seed, kw in gd.DPM_CASES:
        C = gc.DATASETS[ds][0]
        cond = gc.tiles_for(ds, 1, H, W, seed=seed)["cond"]
        xT = torch.randn(1, C, H, W, generator=torch.Generator().manual_seed(seed))

        def run(f64, quant):
            d = diffusion(ds, T, H, gd.PRED_OF_MODEL_TYPE[mt], f64, schedule=gd.dpm_schedule(mt, T), clamp_type="abs")
            cnd, x = (cond.double(), xT.double()) if f64 else (cond, xT)
            ns = S.NoiseScheduleVP("discrete", betas=d.betas.float())  # the schedule scalars stay in the solver's own fp32 in both runs, as in make_objective
            fn = S.model_wrapper(d.model, ns, model_type=mt, guidance_type="classifier-free", guidance_scale=1.0, condition=cnd)
            slv = S.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", correcting_x0_fn="dynamic_thresholding", **kw)
            record(slv, quant)
            with torch.no_grad():
                return slv.sample(x, steps=steps, order=order, skip_type="time_uniform", method="multistep")
        finish(cid, run, float(kw["thresholding_max_val"]), True, lambda out: 1e-4 * max(1.0, float(out.abs().max())), cond)
    assert not too_noisy, f"the reference's own fp32-fp64 gap exceeds a tenth of the tolerance: change these cases: {too_noisy}"
    assert not idle, f"thresholding is active in less than half of the (step, sample) pairs: change these cases: {idle}"


def make_dpmx(UNetSR3, D, S, net_for):
    """DPM-Solver beyond the plain multistep DPM-Solver++ run (tests/golden_cases_dpmx.py).  As make_dynthresh: the reference as it is (fp32: the expected
    output) and its fp64 twin, schedule scalars in the solver's own fp32 in both.  From the fp32 run, by wrapping instance attributes of the solver: `eval_t`
    (the time handed to `slv.model` at every evaluation, in execution order), `orders` (the order argument of every singlestep / multistep update call) and
    `timesteps_outer` (what get_orders_and_timesteps_for_singlestep_solver returned, else the first get_time_steps grid)."""
    import copy

    import golden_cases_dpmx as gx

    nets64 = {}

    def net64_for(ds):
        if ds not in nets64:
            n = copy.deepcopy(net_for(ds)).double()
            fwd = n.forward
            n.forward = lambda x, t, cond=None, self_cond=None: fwd(x.double(), t, None if cond is None else cond.double(), None if self_cond is None else self_cond.double())
            n.noise_level_mlp[0].register_forward_hook(lambda m, i, o: o.double())
            nets64[ds] = n
        return nets64[ds]

    too_noisy = []
    for case in gx.CASES:
        cid, ds, H, T, seed, mt = case["cid"], case["ds"], case["H"], case["T"], case["seed"], case["model_type"]
        C = gc.DATASETS[ds][0]
        cond = gc.tiles_for(ds, 1, H, H, seed=seed)["cond"]
        xT = torch.randn(1, C, H, H, generator=torch.Generator().manual_seed(seed))
        betas = D.make_beta_schedule(**gx.schedule_kwargs(case["schedule"], T))
        betas = torch.as_tensor(betas).float()

        def run(f64, rec, inter=False):
            net = net64_for(ds) if f64 else net_for(ds)
            cnd, x = (cond.double(), xT.double()) if f64 else (cond, xT)
            ns = S.NoiseScheduleVP("discrete", betas=betas)
            fn = S.model_wrapper(net, ns, model_type=mt, guidance_type="classifier-free", guidance_scale=1.0, condition=cnd)
            lms = cnd[:, :C]
            corr = {"clamp": lambda x0, t: (x0 + lms).clamp(0, 1.0) - lms, "dyn": "dynamic_thresholding", None: None}[case["corrector"]]
            slv = S.DPM_Solver(fn, ns, algorithm_type=case["algorithm"], correcting_x0_fn=corr)
            if rec is not None:
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
            with torch.no_grad():
                return slv.sample(x, return_intermediate=inter, **gx.sample_kwargs(case))

        rec = dict(eval_t=[], orders=[])
        t0 = time.time()
        out, out64 = run(False, rec), run(True, None)
        gap = float((out.double() - out64).abs().max())
        tol = 1e-4 * max(1.0, float(out.abs().max()))
        eval_t = torch.cat(rec["eval_t"])
        assert eval_t.dtype == torch.float32
        outer = rec.get("outer", rec["first_grid"])
        extra = {}
        if case["inter"]:
            out_i, inter = run(False, None, inter=True)
            assert torch.equal(out_i, out)
            extra["inter"] = torch.stack(inter)
        print(f"  {cid}: fp32-fp64 gap {gap:.2e}, max|golden| {float(out.abs().max()):.3g}, tolerance {tol:.2e} -> gap / tolerance = {gap / tol:.3f}; orders {rec['orders']}, "
              f"{eval_t.numel()} evaluations, {time.time() - t0:.1f}s")
        if gap > 0.1 * tol:
            too_noisy.append(cid)
        save(cid, out=out, out_f64=out64, gap=gap, eval_t=eval_t, orders=np.asarray(rec["orders"], dtype=np.int64), timesteps_outer=outer, cond_chk=chk(cond), **extra)
    assert not too_noisy, f"the reference's own fp32-fp64 gap exceeds a tenth of the tolerance: change these cases: {too_noisy}"


def make_cfg(UNetSR3, D, S, net_for):
    """Classifier-free guidance in DPM-Solver runs (tests/golden_cases_cfg.py): model_wrapper with guidance_scale != 1 and an unconditional_condition (reference
    solver/dpm_solver.py:330-338: one network call on [unconditional; conditional]).  As make_dpmx: the reference as it is (fp32: the expected output) and its
    fp64 twin, schedule scalars in the solver's own fp32 in both; `eval_t` by wrapping the solver's `model`.  `guided_minus_unguided` is the distance to the
    same run at scale 1: a golden that an unguided run would pass shows nothing."""
    import copy

    import golden_cases_cfg as gcfg
    import golden_cases_dpmx as gx

    nets64 = {}

    def net64_for(ds):
        if ds not in nets64:
            n = copy.deepcopy(net_for(ds)).double()
            fwd = n.forward
            n.forward = lambda x, t, cond=None, self_cond=None: fwd(x.double(), t, None if cond is None else cond.double(), None if self_cond is None else self_cond.double())
            n.noise_level_mlp[0].register_forward_hook(lambda m, i, o: o.double())
            nets64[ds] = n
        return nets64[ds]

    too_noisy = []
    for case in gcfg.CASES:
        cid, ds, H, T, seed, mt = case["cid"], case["ds"], case["H"], case["T"], case["seed"], case["model_type"]
        C = gc.DATASETS[ds][0]
        cond = gc.tiles_for(ds, 1, H, H, seed=seed)["cond"]
        uncond = gcfg.unconditional_of(cond, C)
        xT = torch.randn(1, C, H, H, generator=torch.Generator().manual_seed(seed))
        betas = torch.as_tensor(D.make_beta_schedule(**gx.schedule_kwargs(case["schedule"], T))).float()

        def run(f64, rec, scale):
            net = net64_for(ds) if f64 else net_for(ds)
            cnd, unc, x = (cond.double(), uncond.double(), xT.double()) if f64 else (cond, uncond, xT)
            ns = S.NoiseScheduleVP("discrete", betas=betas)
            fn = S.model_wrapper(net, ns, model_type=mt, guidance_type="classifier-free", guidance_scale=scale, condition=cnd, unconditional_condition=unc)
            lms = cnd[:, :C]
            corr = {"clamp": lambda x0, t: (x0 + lms).clamp(0, 1.0) - lms, "dyn": "dynamic_thresholding", None: None}[case["corrector"]]
            slv = S.DPM_Solver(fn, ns, algorithm_type=case["algorithm"], correcting_x0_fn=corr)
            if rec is not None:
                model = slv.model

                def w_model(x_, t_):
                    rec["eval_t"].append(t_.detach().reshape(-1)[:1].clone())
                    return model(x_, t_)
                slv.model = w_model
            with torch.no_grad():
                return slv.sample(x, **gx.sample_kwargs(case))

        rec = dict(eval_t=[])
        t0 = time.time()
        out, out64, plain = run(False, rec, case["scale"]), run(True, None, case["scale"]), run(False, None, 1.0)
        gap = float((out.double() - out64).abs().max())
        tol = 1e-4 * max(1.0, float(out.abs().max()))
        diff = float((out - plain).abs().max())
        eval_t = torch.cat(rec["eval_t"])
        assert eval_t.dtype == torch.float32
        print(f"  {cid}: fp32-fp64 gap {gap:.2e}, max|golden| {float(out.abs().max()):.3g}, tolerance {tol:.2e} -> gap / tolerance = {gap / tol:.3f}; "
              f"max|guided - unguided| {diff:.3g}, {eval_t.numel()} evaluations, {time.time() - t0:.1f}s")
        assert diff > 100 * tol, f"{cid}: the guided golden is within {diff:.2e} of the unguided run"
        if gap > 0.1 * tol:
            too_noisy.append(cid)
        save(cid, out=out, out_f64=out64, gap=gap, eval_t=eval_t, guided_minus_unguided=diff, cond_chk=chk(cond))
    assert not too_noisy, f"the reference's own fp32-fp64 gap exceeds a tenth of the tolerance: change these cases: {too_noisy}"


def make_l1ssim(UNetSR3, D, S, net_for):
    """loss_type="l1ssim" (tests/golden_cases_l1ssim.py).  As make_objective, whose twin construction, pinning of t and mask capture this repeats for the one loss:
    the reference as it is (fp32: the expected value) and its fp64 twin with the same fp32 random draws, `<key>_f64` and `gap::<key>` next to every value.
    HybridL1SSIM keeps its window as a plain attribute and rebuilds it `type_as` the input (utils/loss_utils.py:133-142), so the twin filters with the SAME
    fp32-rounded weights in double arithmetic."""
    import copy

    import golden_cases_l1ssim as gl

    nets64 = {}

    def net64_for(ds):
        if ds not in nets64:
            n = copy.deepcopy(net_for(ds)).double()
            fwd = n.forward
            n.forward = lambda x, t, cond=None, self_cond=None: fwd(x.double(), t, None if cond is None else cond.double(), None if self_cond is None else self_cond.double())
            n.noise_level_mlp[0].register_forward_hook(lambda m, i, o: o.double())
            nets64[ds] = n
        return nets64[ds]

    def diffusion(ds, T, size, pred_mode, gamma, f64):
        net = net64_for(ds) if f64 else net_for(ds)
        d = D.GaussianDiffusion(net, image_size=size, channels=gc.DATASETS[ds][0], pred_mode=pred_mode, loss_type="l1ssim", device="cpu", clamp_range=(0, 1),
                                p2_loss_weight_gamma=gamma)
        d.set_new_noise_schedule(betas=D.make_beta_schedule(schedule="cosine", n_timestep=T, cosine_s=8e-3))
        assert isinstance(d.loss_func, D.HybridL1SSIM) and tuple(d.loss_func.loss.weighted_ratio) == gl.WEIGHTS
        return d.double() if f64 else d

    too_noisy = []

    def report(cid, gap, tol):
        print(f"  {cid}: fp32-fp64 gap {gap:.2e}, tolerance {tol:.2e} -> gap / tolerance = {gap / tol:.3f}")
        if gap > 0.1 * tol:
            too_noisy.append(cid)

    class Pin:
        def __init__(self, tt, sc_branch):
            self.tt, self.sc = tt, sc_branch

        def __enter__(self):
            self.ri, self.rr = torch.randint, random.random
            D.torch.randint = lambda *a, **k: self.tt
            D.random.random = (lambda: 0.0) if self.sc else (lambda: 1.0)

        def __exit__(self, *a):
            D.torch.randint, D.random.random = self.ri, self.rr

    # ---- the operator: HybridL1SSIM(channel=C)(x, y) and autograd's gradients with respect to both arguments
    for case in gl.OP_CASES:
        cid, C = case[0], case[2]
        x, y = gl.op_inputs(case)
        res = {}
        for f64 in (False, True):
            a, b = (v.double() if f64 else v.clone() for v in (x, y))
            a.requires_grad_(True), b.requires_grad_(True)
            loss = D.HybridL1SSIM(channel=C)(a, b)
            loss.backward()
            res[f64] = (loss.detach().reshape(1), a.grad.detach(), b.grad.detach())
        (l, g1, g2), (l64, g1_64, g2_64) = res[False], res[True]
        gap_l = float((l.double() - l64).abs().max())
        rel = lambda g, g64: float((g.double() - g64).abs().max()) / max(float(g64.abs().max()), 1e-5)
        report(f"{cid} loss", gap_l, 1e-6)
        report(f"{cid} d/d img1 (relative)", rel(g1, g1_64), 5e-5)
        report(f"{cid} d/d img2 (relative)", rel(g2, g2_64), 5e-5)
        save(cid, x=x, y=y, loss=l, loss_f64=l64, grad1=g1, grad1_f64=g1_64, grad2=g2, grad2_f64=g2_64,
             **{"gap::loss": gap_l, "gap::grad1_rel": rel(g1, g1_64), "gap::grad2_rel": rel(g2, g2_64)})

    # ---- p_losses in eval mode
    for stem, ds, B, H, W, T, tvals, sc_branch, seed in gl.LOSS_CASES:
        C = gc.DATASETS[ds][0]
        tiles = gc.tiles_for(ds, B, H, W, seed=seed)
        cond, res_ = tiles["cond"], tiles["gt"] - tiles["lms"]
        noise = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed))
        tt = torch.tensor(tvals, dtype=torch.long)
        for pm in gl.PRED_MODES:
            arrs = {}
            for gamma in gl.P2_GAMMAS:
                out = {}
                for f64 in (False, True):
                    d = diffusion(ds, T, H, pm, gamma, f64)
                    cast = (lambda v: v.double()) if f64 else (lambda v: v)
                    with Pin(tt, sc_branch), torch.no_grad():
                        loss, recon = d(cast(res_), mode="train", noise=cast(noise), cond=cast(cond))
                    out[f64] = (loss.reshape(1), recon)
                k = gl.loss_key(gamma)
                (loss, recon), (loss64, recon64) = out[False], out[True]
                gl_, gr = float((loss.double() - loss64).abs().max()), float((recon.double() - recon64).abs().max())
                report(f"{stem}_{pm} {k} loss", gl_, 1e-6)
                report(f"{stem}_{pm} {k} recon", gr, 2e-5)
                arrs.update({f"loss_{k}": loss, f"loss_{k}_f64": loss64, f"gap::loss_{k}": gl_, f"recon_{k}": recon, f"recon_{k}_f64": recon64, f"gap::recon_{k}": gr})
            save(f"{stem}_{pm}", cond_chk=chk(cond), **arrs)

    # ---- p_losses(...).backward() under .train(): the fp32 run captures the Dropout / DropPath masks, the fp64 run imposes them
    for cid, ds, B, H, W, T, tvals, pm, gamma, seed in gl.GRAD_CASES:
        C = gc.DATASETS[ds][0]
        tiles = gc.tiles_for(ds, B, H, W, seed=seed)
        cond, res_ = tiles["cond"], tiles["gt"] - tiles["lms"]
        noise = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed))
        tt = torch.tensor(tvals, dtype=torch.long)
        drops, paths = [], []

        def run(f64):
            d = diffusion(ds, T, H, pm, gamma, f64)
            net = d.model
            hooks, k = [], [0, 0]
            for m in net.modules():
                if isinstance(m, nn.Dropout):
                    if not f64:
                        hooks.append(m.register_forward_hook(lambda mod, inp, out: drops.append(((out != 0) | (inp[0] == 0)).detach())))
                    else:
                        def imp(mod, inp, out):
                            k[0] += 1
                            return inp[0] * drops[k[0] - 1].double() / (1 - mod.p)
                        hooks.append(m.register_forward_hook(imp))
                elif type(m).__name__ == "DropPath":
                    if not f64:
                        hooks.append(m.register_forward_hook(lambda mod, inp, out: paths.append(((out.detach().flatten(1).abs().sum(1) != 0).float() / (1 - mod.drop_prob)))))
                    else:
                        def impp(mod, inp, out):
                            k[1] += 1
                            return inp[0] * paths[k[1] - 1].double().reshape(-1, 1, 1, 1)
                        hooks.append(m.register_forward_hook(impp))
            net.train()
            for prm in net.parameters():
                prm.requires_grad_(True)
                prm.grad = None
            torch.manual_seed(seed)
            cast = (lambda v: v.double()) if f64 else (lambda v: v)
            try:
                with Pin(tt, False):
                    loss, recon = d(cast(res_), mode="train", noise=cast(noise), cond=cast(cond))
                loss.backward()
            finally:
                net.eval()
                for hk in hooks:
                    hk.remove()
            names = [n for n, _ in net.named_parameters()]
            norms = np.array([float(prm.grad.double().norm()) if prm.grad is not None else -1.0 for _, prm in net.named_parameters()], dtype=np.float64)
            full = {"grad::" + n: prm.grad.detach().clone() for n, prm in net.named_parameters() if any(n == f or n.startswith(f) for f in gl.TRAIN_GRAD_FULL)}
            for prm in net.parameters():
                prm.grad = None
                prm.requires_grad_(False)
            return float(loss.detach()), recon.detach(), names, norms, full

        loss, recon, names, norms, full = run(False)
        loss64, recon64, _, norms64, full64 = run(True)
        rel = float(np.max(np.abs(norms - norms64) / np.maximum(norms64, 1e-4)))
        gfull = max(float((full[k].double() - full64[k]).abs().max()) / max(float(full64[k].abs().max()), 1e-5) for k in full)
        grec = float((recon.double() - recon64).abs().max())
        print(f"  {cid}: loss gap {abs(loss - loss64):.2e} (tolerance 1e-6), recon gap {grec:.2e} (tolerance 2e-5), worst relative grad-norm gap {rel:.2e} (tolerance 2e-4), "
              f"worst relative full-gradient gap {gfull:.2e} (tolerance 5e-5)")
        if not (abs(loss - loss64) <= 1e-7 and grec <= 2e-6 and rel <= 2e-5 and gfull <= 5e-6):
            too_noisy.append(cid)
        arrs = {f"drop_{k}": np.packbits(d_.numpy().reshape(-1)) for k, d_ in enumerate(drops)}
        arrs.update({f"drop_{k}_shape": np.array(d_.shape) for k, d_ in enumerate(drops)})
        save(cid, loss=loss, loss_f64=loss64, recon=recon, recon_f64=recon64, n_drop=len(drops), paths=torch.stack(paths), p_drop=0.2, names=np.array(names), grad_norms=norms,
             grad_norms_f64=norms64, **{"gap::loss": abs(loss - loss64), "gap::recon": grec, "gap::grad_norms_rel": rel, "gap::grad_full_rel": gfull}, **arrs, **full)
    assert not too_noisy, f"the reference's own fp32-fp64 gap exceeds a tenth of the tolerance: change the seed or the pinned t of these cases: {too_noisy}"


def make_q2n():
    """The Q2n index (tests/golden_cases_q2n.py; include/ddif.h ddif_q2n states the definition).  The reference's own `q2n` cannot be the oracle: it takes
    `qu[:, :, i]` on an (N, bs, bs, C) array (utils/_metric_legacy.py:193: a column, not a band), and raises for N > 1, for band counts that are no power
    of two and for some sizes.  Its building blocks are right, so the expected block values are a composition of ITS norm_blocco, onion_mult and
    onion_mult2D, imported here, along the definition: bands zero-padded to a power of two, blocks cut with clamped indices (edge replication, which is
    what its padding does wherever it runs), fp64 throughout.  Per (image pair, block) the file holds Q, the per-band s and t, T3, the bias, and
    `sens`: the largest change of Q under N_PERMUTATIONS random permutations of the block's pixels -- the composition's own sensitivity to summation
    order, which the tests scale their tolerance by."""
    import importlib.util

    import golden_cases_q2n as gq

    spec = importlib.util.spec_from_file_location("_ref_metric_legacy", os.path.join(REF, "utils", "_metric_legacy.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)

    def block_q(g, f):  # (bs, bs, Cp) fp64 each
        bs, Cp = g.shape[0], g.shape[-1]
        n = bs * bs
        z1, z2 = np.empty_like(g), np.empty_like(f)
        s, t = np.zeros(Cp), np.zeros(Cp)
        for k in range(Cp):
            z1[..., k], s[k], t[k] = R.norm_blocco(g[..., k])
            y = (f[..., k] - s[k] + 1) if s[k] == 0 else ((f[..., k] - s[k]) / t[k] + 1)
            z2[..., k] = y if k == 0 else -y
        m1, m2 = z1.mean(axis=(0, 1)), z2.mean(axis=(0, 1))
        n1, n2 = (m1 ** 2).sum(), (m2 ** 2).sum()
        T3 = n / (n - 1) * ((z1 ** 2).sum(axis=-1).mean() + (z2 ** 2).sum(axis=-1).mean() - n1 - n2)
        bias = 2 * np.sqrt(n1) * np.sqrt(n2) / (n1 + n2)
        if T3 == 0:
            q = np.zeros(Cp)
            q[-1] = bias
        else:
            qu = R.onion_mult2D(z1[None], z2[None])[0]
            q = n / (n - 1) * (qu.mean(axis=(0, 1)) - R.onion_mult(m1.copy(), m2.copy())) * bias * 2 / T3
        return float(np.sqrt((q ** 2).sum())), s, t, float(T3), float(bias)

    def run(case, gt, preds, regular):
        name, B, C, H, W, block, shift = case
        Cp = 1 << (C - 1).bit_length()
        ny, nx = -(-H // shift), -(-W // shift)
        prng = np.random.default_rng(4242)
        arrs = dict(gt=gt, geometry=np.array([B, C, H, W, block, shift, ny, nx]))

        def padded(img):  # (C, H, W) uint16 -> (H, W, Cp) fp64
            out = np.zeros((H, W, Cp))
            out[..., :C] = np.transpose(img.astype(np.float64), (1, 2, 0))
            return out

        for pair, pred in preds.items():
            qmap, sens, T3, bias = (np.zeros((B, ny, nx)) for _ in range(4))
            s, t = np.zeros((B, ny, nx, Cp)), np.zeros((B, ny, nx, Cp))
            for b in range(B):
                G, F_ = padded(gt[b]), padded(pred[b])
                for j in range(ny):
                    rows = np.minimum(j * shift + np.arange(block), H - 1)
                    for i in range(nx):
                        cols = np.minimum(i * shift + np.arange(block), W - 1)
                        g, f = G[np.ix_(rows, cols)], F_[np.ix_(rows, cols)]
                        qmap[b, j, i], s[b, j, i], t[b, j, i], T3[b, j, i], bias[b, j, i] = block_q(g, f)
                        gf, ff = g.reshape(-1, Cp), f.reshape(-1, Cp)
                        for _ in range(gq.N_PERMUTATIONS):
                            p = prng.permutation(block * block)
                            sens[b, j, i] = max(sens[b, j, i], abs(block_q(gf[p].reshape(g.shape), ff[p].reshape(f.shape))[0] - qmap[b, j, i]))
            if regular:  # (the zero bands appended up to Cp have t = 1e-8 by construction: the rule is about the C real ones)
                assert (t[..., :C] >= 1).all() and (T3 != 0).all(), f"{name}/{pair}: a block of a regular case is degenerate"
                assert np.isfinite(qmap).all() and (qmap <= 1 + 1e-12).all() and (qmap >= 0).all(), (name, pair)
            if pair == "identical":
                assert np.abs(qmap - 1).max() <= 1e-12, (name, float(np.abs(qmap - 1).max()))  # (the composition's own rounding: a few 1e-14 at most)
            arrs.update({f"pred_{pair}": pred, f"map_{pair}": qmap, f"sens_{pair}": sens, f"s_{pair}": s, f"t_{pair}": t, f"T3_{pair}": T3,
                         f"bias_{pair}": bias})
            print(f"  {name}/{pair}: Q2n {qmap.mean(axis=(1, 2))}, order sensitivity <= {sens.max():.2e}")
        out = gq.path(name)
        np.savez_compressed(out, **arrs)
        size = os.path.getsize(out)
        assert size < 1 << 20, (name, size)
        print(f"  wrote {os.path.relpath(out, ROOT)} ({size / 1024:.0f} KiB)")

    for case in gq.CASES:
        run(case, *gq.images(case), regular=True)
    run(gq.DEGENERATE, *gq.degenerate_images(), regular=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="manifest,fwd,fwdbig,trunc,dpmskip,trainfwd,traingrad,sched,ddpm,ddim,dpm,loss,psnr")
    ap.add_argument("--skip-long", action="store_true")
    args = ap.parse_args()
    only = set(args.only.split(","))
    os.makedirs(gc.GOLDEN_DIR, exist_ok=True)
    torch.set_num_threads(8)
    UNetSR3, D, S = import_reference()
    nets = {}

    def net_for(ds):
        if ds not in nets:
            nets[ds] = build_ref_net(UNetSR3, ds)
        return nets[ds]

    if "manifest" in only:
        for ds in gc.DATASETS:
            import builtins
            _print = builtins.print
            builtins.print = lambda *a, **k: None
            cfg = gc.cfg_for(ds)
            fresh = UNetSR3(in_channel=cfg["in_channel"], out_channel=cfg["out_channel"],
                            lms_channel=cfg["lms_channel"], pan_channel=cfg["pan_channel"], inner_channel=32,
                            norm_groups=1, channel_mults=(1, 2, 2, 4), attn_res=(8,), dropout=0.2, image_size=64,
                            self_condition=True)
            builtins.print = _print
            man = [[k, list(v.shape)] for k, v in fresh.state_dict().items()]
            with open(os.path.join(gc.GOLDEN_DIR, f"manifest_{ds}.json"), "w") as f:
                json.dump(dict(n_params=sum(p.numel() for p in fresh.parameters()), keys=man), f)
            print(f"  manifest_{ds}.json: {len(man)} tensors")

    if "fwd" in only:
        for case in gc.FORWARD_CASES:
            x, t, cond, sc = gc.forward_inputs(case)
            with torch.no_grad():
                y = net_for(case[1])(x, t, cond, sc)
            save(case[0], y=y, x_chk=chk(x), cond_chk=chk(cond))

    if "fwdbig" in only:
        for case in gc.FORWARD_BIG_CASES:
            x, t, cond, sc = gc.forward_inputs(case)
            with torch.no_grad():
                y = net_for(case[1])(x, t, cond, sc)
            save(case[0], y=y, x_chk=chk(x), cond_chk=chk(cond))

    if "trunc" in only:
        import builtins

        for cid, ds, B, H, W, T, which, n, seed in gc.DDPM_TRUNC_CASES:
            C = gc.DATASETS[ds][0]
            cond = gc.tiles_for(ds, B, H, W, seed=seed)["cond"]
            d = make_diffusion(D, net_for(ds), C, T, H)
            # the reference loop itself, iterating only the first / last n timesteps: p_sample_loop looks `reversed` up
            # in its module globals, so a module-level stand-in truncates the iteration without touching its code
            D.reversed = (lambda r: iter(list(builtins.reversed(r))[:n])) if which == "first" else (lambda r: iter(list(builtins.reversed(r))[-n:]))
            try:
                torch.manual_seed(seed)
                t0 = time.time()
                out = d(cond, mode="ddpm_sample")
            finally:
                del D.reversed
            print(f"  {cid}: {time.time() - t0:.1f}s")
            save(cid, out=out, cond_chk=chk(cond))

    if "dpmskip" in only:
        for cid, ds, H, W, T, steps, order, seed, skip in gc.DPM_SKIP_CASES:
            C = gc.DATASETS[ds][0]
            cond = gc.tiles_for(ds, 1, H, W, seed=seed)["cond"]
            d = make_diffusion(D, net_for(ds), C, T, H)
            ns = S.NoiseScheduleVP("discrete", betas=d.betas)
            lms = cond[:, :C]
            fn = S.model_wrapper(net_for(ds), ns, model_type="x_start", guidance_type="classifier-free",
                                 guidance_scale=1.0, condition=cond)
            slv = S.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", correcting_x0_fn=lambda x0, t, lms=lms: (x0 + lms).clamp(0, 1.0) - lms)
            xT = torch.randn(1, C, H, W, generator=torch.Generator().manual_seed(seed))
            with torch.no_grad():
                out = slv.sample(xT, steps=steps, order=order, skip_type=skip, method="multistep")
            save(cid, out=out, cond_chk=chk(cond))

    if "trainfwd" in only:
        for cid, ds, B, H, W, tvals, seed in gc.TRAIN_FWD_CASES:
            C = gc.DATASETS[ds][0]
            net = net_for(ds)
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(B, C, H, W, generator=g)
            sc = torch.randn(B, C, H, W, generator=g)
            cond = gc.tiles_for(ds, B, H, W, seed=seed)["cond"]
            t = torch.tensor(tvals, dtype=torch.long)
            drops, paths, hooks = [], [], []
            for m in net.modules():  # module order is not execution order: record in the hooks, which fire in execution order
                if isinstance(m, nn.Dropout):
                    hooks.append(m.register_forward_hook(lambda mod, inp, out: drops.append((out != 0) | (inp[0] == 0))))
                elif type(m).__name__ == "DropPath":
                    hooks.append(m.register_forward_hook(lambda mod, inp, out: paths.append((out.flatten(1).abs().sum(1) != 0).float() / (1 - mod.drop_prob))))
            net.train()
            torch.manual_seed(seed)
            try:
                with torch.no_grad():
                    y = net(x, t, cond, sc)
            finally:
                net.eval()
                for hk in hooks:
                    hk.remove()
            arrs = {f"drop_{k}": np.packbits(d.numpy().reshape(-1)) for k, d in enumerate(drops)}
            arrs.update({f"drop_{k}_shape": np.array(d.shape) for k, d in enumerate(drops)})
            save(cid, y=y, n_drop=len(drops), paths=torch.stack(paths), p_drop=0.2, **arrs)

    if "traingrad" in only:
        # G7: one training forward + backward of the REAL reference under .train() (same inputs / seed / masks as trainfwd), L1 loss against
        # a fixed target: the norm of every parameter's gradient, and a handful of full gradients
        for cid, ds, B, H, W, tvals, seed in gc.TRAIN_GRAD_CASES:
            C = gc.DATASETS[ds][0]
            net = net_for(ds)
            g = torch.Generator().manual_seed(seed)
            x = torch.randn(B, C, H, W, generator=g)
            sc = torch.randn(B, C, H, W, generator=g)
            target = torch.rand(B, C, H, W, generator=g)
            cond = gc.tiles_for(ds, B, H, W, seed=seed)["cond"]
            t = torch.tensor(tvals, dtype=torch.long)
            drops, paths, hooks = [], [], []
            for m in net.modules():
                if isinstance(m, nn.Dropout):
                    hooks.append(m.register_forward_hook(lambda mod, inp, out: drops.append(((out != 0) | (inp[0] == 0)).detach())))
                elif type(m).__name__ == "DropPath":
                    hooks.append(m.register_forward_hook(lambda mod, inp, out: paths.append(((out.detach().flatten(1).abs().sum(1) != 0).float() / (1 - mod.drop_prob)))))
            net.train()
            for prm in net.parameters():
                prm.requires_grad_(True)
                prm.grad = None
            torch.manual_seed(seed)
            try:
                y = net(x, t, cond, sc)
                loss = F.l1_loss(y, target)
                loss.backward()
            finally:
                net.eval()
                for hk in hooks:
                    hk.remove()
            names = [k for k, _ in net.named_parameters()]
            norms = np.array([float(prm.grad.norm()) if prm.grad is not None else -1.0 for _, prm in net.named_parameters()], dtype=np.float64)
            full = {}
            for k, prm in net.named_parameters():
                if any(k == f or k.startswith(f) for f in gc.TRAIN_GRAD_FULL):
                    full["grad::" + k] = prm.grad.detach().clone()
            for prm in net.parameters():
                prm.grad = None
            arrs = {f"drop_{k}": np.packbits(d.numpy().reshape(-1)) for k, d in enumerate(drops)}
            arrs.update({f"drop_{k}_shape": np.array(d.shape) for k, d in enumerate(drops)})
            save(cid, y=y.detach(), loss=float(loss), n_drop=len(drops), paths=torch.stack(paths), p_drop=0.2, names=np.array(names), grad_norms=norms, **arrs, **full)

    if "sched" in only:
        out = {}
        for T in gc.SCHEDULE_T:
            d = make_diffusion(D, net_for("wv3"), 8, T, 64)
            for k, v in d.named_buffers():
                if "." not in k:
                    out[f"T{T}.{k}"] = v.clone()
        for T in gc.DDIM_FROM:
            d = make_diffusion(D, net_for("wv3"), 8, T, 64)
            use = d.space_timesteps(d.num_timesteps, "ddim25")
            out[f"ddim25_from_T{T}.keep"] = np.array(sorted(use))
            d.space_new_betas(use)
            for k, v in d.named_buffers():
                if "." not in k:
                    out[f"ddim25_from_T{T}.{k}"] = v.clone()
        save("schedules", **out)

    ddpm_cases = list(gc.DDPM_CASES) if "ddpm" in only else []
    if "ddpmbig" in only:  # round 6: two more configs[1] tiles (about a minute each on 8 cores)
        ddpm_cases += gc.DDPM_BIG_CASES
    if "ddpmfull" in only:  # round 6: the full CAVE 128 x 128 T = 2000 chain (one-off: 15-25 minutes on 8 cores)
        ddpm_cases += gc.DDPM_FULL_CASES
    if ddpm_cases:
        for cid, ds, B, H, W, T, seed in ddpm_cases:
            if args.skip_long and T * H * W > 100 * 32 * 32:
                continue
            C = gc.DATASETS[ds][0]
            cond = gc.tiles_for(ds, B, H, W, seed=seed)["cond"]
            d = make_diffusion(D, net_for(ds), C, T, H)
            snaps = {}
            want = gc.DDPM_SNAPSHOTS.get(cid, [])
            if want:
                orig = d.p_sample
                count = [0]

                def wrapped(*a, **k):
                    r = orig(*a, **k)
                    count[0] += 1
                    if count[0] in want:
                        snaps[f"after_{count[0]}"] = r.clone()
                    return r

                d.p_sample = wrapped
            torch.manual_seed(seed)
            t0 = time.time()
            out = d(cond, mode="ddpm_sample")
            print(f"  {cid}: {time.time() - t0:.1f}s")
            save(cid, out=out, cond_chk=chk(cond), **snaps)

    if "ddim" in only:
        for cid, ds, B, H, W, T, sect, seed in gc.DDIM_CASES:
            C = gc.DATASETS[ds][0]
            cond = gc.tiles_for(ds, B, H, W, seed=seed)["cond"]
            d = make_diffusion(D, net_for(ds), C, T, H)
            torch.manual_seed(seed)
            out = d(cond, mode="ddim_sample", section_counts=sect)
            save(cid, out=out, cond_chk=chk(cond), num_timesteps_after=d.num_timesteps)

    dpm_cases = list(gc.DPM_CASES) if "dpm" in only else []
    if "dpmbig" in only:  # round 6: configs[2] at the benchmarked tile size
        dpm_cases += gc.DPM_BIG_CASES
    if dpm_cases:
        for cid, ds, H, W, T, steps, order, seed in dpm_cases:
            C = gc.DATASETS[ds][0]
            cond = gc.tiles_for(ds, 1, H, W, seed=seed)["cond"]
            d = make_diffusion(D, net_for(ds), C, T, H)
            ns = S.NoiseScheduleVP("discrete", betas=d.betas)
            lms = cond[:, :C]

            def corr(x0, t, lms=lms):
                return (x0 + lms).clamp(0, 1.0) - lms

            fn = S.model_wrapper(net_for(ds), ns, model_type="x_start", guidance_type="classifier-free",
                                 guidance_scale=1.0, condition=cond)
            slv = S.DPM_Solver(fn, ns, algorithm_type="dpmsolver++", correcting_x0_fn=corr)
            g = torch.Generator().manual_seed(seed)
            xT = torch.randn(1, C, H, W, generator=g)
            with torch.no_grad():
                out = slv.sample(xT, steps=steps, order=order, skip_type="time_uniform", method="multistep")
            save(cid, out=out, cond_chk=chk(cond))

    if "loss" in only:
        for cid, ds, B, H, W, T, tvals, sc_branch, seed in gc.LOSS_CASES:
            C = gc.DATASETS[ds][0]
            tiles = gc.tiles_for(ds, B, H, W, seed=seed)
            cond = tiles["cond"]
            res = tiles["gt"] - tiles["lms"]
            d = make_diffusion(D, net_for(ds), C, T, H)
            g = torch.Generator().manual_seed(seed)
            noise = torch.randn(B, C, H, W, generator=g)
            tt = torch.tensor(tvals, dtype=torch.long)
            _ri, _rr = torch.randint, random.random
            D.torch.randint = lambda *a, **k: tt
            D.random.random = (lambda: 0.0) if sc_branch else (lambda: 1.0)
            try:
                with torch.no_grad():
                    loss, recon = d(res, mode="train", noise=noise, cond=cond)
            finally:
                D.torch.randint, D.random.random = _ri, _rr
            save(cid, loss=loss, recon=recon, cond_chk=chk(cond))

    if "objective" in only:
        make_objective(UNetSR3, D, S, net_for)
    if "dynthresh" in only:
        make_dynthresh(UNetSR3, D, S, net_for)
    if "l1ssim" in only:
        make_l1ssim(UNetSR3, D, S, net_for)
    if "dpmx" in only:
        make_dpmx(UNetSR3, D, S, net_for)
    if "cfg" in only:
        make_cfg(UNetSR3, D, S, net_for)
    if "q2n" in only:
        make_q2n()

    if "psnr" in only:
        import importlib.util

        g = torch.Generator().manual_seed(5)
        a = torch.rand(8, 33, 35, generator=g)
        b = (a + 0.05 * torch.randn(8, 33, 35, generator=g)).clamp(0, 1)
        spec = importlib.util.spec_from_file_location("_ml", os.path.join(REF, "utils", "_metric_legacy.py"))
        ml = importlib.util.module_from_spec(spec)
        try:
            spec.loader.exec_module(ml)
            acc = ml.analysis_accu(a.permute(1, 2, 0), b.permute(1, 2, 0), 4, choices=5)  # what AnalysisPanAcc calls (utils/metric.py:27-29)
            save("psnr", ref_psnr=acc["PSNR"], sam=acc["SAM"], ergas=acc["ERGAS"], cc=acc["CC"])
        except Exception as e:  # pragma: no cover
            print("  psnr fixture skipped:", repr(e))


if __name__ == "__main__":
    main()
