"""The checks of the noise / v parameterisations, shared by tests/test_objective_emu.py (host-emulated build, CPU tensors) and
tests/test_objective_gpu.py (the gfx950 library): every golden of tests/golden_cases_objective.py through the drop-in classes, which drive
the C ABI (ddif_plan_set_objective, the _ex entry points).

Tolerances
  * clamped DDPM: the project's bar -- atol 1e-4 per pixel, PSNR within 1e-3 dB;
  * unclamped runs (DDIM; DPM-Solver++ evaluates the network on unclamped iterates): the same bar in relative form, 1e-4 * max(1, max|golden|);
    the PSNR leg is skipped where max|golden| > 1 (PSNR is undefined for that range);
  * loss values and gradients: the comparison of test_train_graph for traingrad_wv3_16 (loss 1e-6; norms 2e-4 * max(ref, 1e-4); full gradients
    5e-5 * max(max|ref|, 1e-5));
  * recon_x0 of p_losses: 2e-5 absolute, the bar of test_gpu_parity.test_p_losses_forward_matches_reference_golden.  recon_x0 of the noise mode is amplified by
    1 / sqrt(alpha_bar_t), so the pinned t of the cases stay where one fp32 ulp of it is well below that bar (t <= 250 of 500).
Every golden stores the reference's own fp32 <-> fp64 gap; `check_gap` asserts it is below a tenth of the tolerance used.

The DPM-Solver++ cases take their schedule from golden_cases_objective.dpm_schedule: cosine for "noise", linear for "v", where the reference's own fp32
arithmetic is well conditioned at t = T (the reasoning and the figures are there)."""
from __future__ import annotations

import os

import numpy as np
import torch

import golden_cases as gc
import golden_cases_objective as go
from ddif_testlib import make_net, reference_noise_stream
from oracle import ddif_oracle as O

_nets = {}


def net_for(ds, dev):
    key = (ds, str(dev))
    if key not in _nets:
        _nets[key] = make_net(ds, dev)
    return _nets[key]


def load(name):
    return np.load(os.path.join(gc.GOLDEN_DIR, name + ".npz"))


def diffusion(ds, T, size, dev, pred_mode, loss_type="l2", gamma=0.0, schedule=None):
    from ddif.diffusion.diffusion_ddpm_pan import GaussianDiffusion, make_beta_schedule

    d = GaussianDiffusion(net_for(ds, dev), image_size=size, channels=gc.DATASETS[ds][0], pred_mode=pred_mode, loss_type=loss_type, device=dev,
                          clamp_range=(0, 1), p2_loss_weight_gamma=gamma)
    d.set_new_noise_schedule(betas=make_beta_schedule(**(schedule or dict(schedule="cosine", n_timestep=T, cosine_s=8e-3))), device=dev)
    return d


def check_gap(gap, tol, what):
    print(f"{what}: reference fp32-fp64 gap {float(gap):.3e}, tolerance {tol:.3e}")
    assert float(gap) <= 0.1 * tol, (what, float(gap), tol)


def _compare(out, g, what, psnr_args=None, relative=False):
    """relative: an unclamped run (DDIM, DPM-Solver++) -- the 1e-4 bar scales with max(1, max|golden|); clamped DDPM keeps atol 1e-4."""
    ref = torch.from_numpy(g["out"])
    scale = max(1.0, float(ref.abs().max())) if relative else 1.0
    tol = 1e-4 * scale
    err = float((out.cpu() - ref).abs().max())
    print(f"{what}: max|out - golden| {err:.3e} (max|golden| {float(ref.abs().max()):.3g}, tolerance {tol:.3e})")
    check_gap(g["gap"], tol, what)
    assert bool(torch.isfinite(out).all())
    assert err <= tol, (what, err, tol)
    if psnr_args is not None and float(ref.abs().max()) <= 1.0:
        lms, gt = psnr_args
        sr, sr_ref = (out.cpu() + lms).clip(0, 1), (ref + lms).clip(0, 1)
        dp = abs(O.psnr(sr, gt) - O.psnr(sr_ref, gt))
        print(f"{what}: |dPSNR| {dp:.3e} dB")
        assert dp <= 1e-3, (what, dp)


def run_ddpm(case, pm, dev):
    stem, ds, B, H, W, T, seed = case
    g = load(f"{stem}_{pm}")
    C = gc.DATASETS[ds][0]
    tiles = gc.tiles_for(ds, B, H, W, seed=seed)
    cond = tiles["cond"]
    d = diffusion(ds, T, H, dev, pm)
    xT, noise = reference_noise_stream(seed, (B, C, H, W), T)
    out = d(cond.to(dev), mode="ddpm_sample", x_T=xT.to(dev), noise=noise.to(dev))
    _compare(out, g, f"{stem}_{pm}", (cond[:, :C], tiles["gt"]))


def run_ddim(case, pm, dev):
    stem, ds, B, H, W, T, sect, seed = case
    g = load(f"{stem}_{pm}")
    C = gc.DATASETS[ds][0]
    tiles = gc.tiles_for(ds, B, H, W, seed=seed)
    cond = tiles["cond"]
    d = diffusion(ds, T, H, dev, pm)
    n_keep = len(O.ddim_stride_set(T, sect))
    xT, noise = reference_noise_stream(seed, (B, C, H, W), n_keep)
    out = d(cond.to(dev), mode="ddim_sample", section_counts=sect, x_T=xT.to(dev), noise=noise.to(dev))
    assert d.num_timesteps == n_keep
    _compare(out, g, f"{stem}_{pm}", (cond[:, :C], tiles["gt"]), relative=True)


def run_dpm(case, pm, dev):
    from ddif.solver.dpm_solver import DPM_Solver, ImageSpaceClamp, NoiseScheduleVP, model_wrapper

    stem, ds, H, W, T, steps, order, seed = case
    g = load(f"{stem}_{pm}")
    C = gc.DATASETS[ds][0]
    tiles = gc.tiles_for(ds, 1, H, W, seed=seed)
    cond = tiles["cond"].to(dev)
    xT = torch.randn(1, C, H, W, generator=torch.Generator().manual_seed(seed)).to(dev)
    d = diffusion(ds, T, H, dev, pm, schedule=go.dpm_schedule(pm, T))
    ns = NoiseScheduleVP("discrete", betas=d.betas)
    fn = model_wrapper(d.model, ns, model_type=go.MODEL_TYPE[pm], guidance_type="classifier-free", guidance_scale=1.0, condition=cond)
    slv = DPM_Solver(fn, ns, algorithm_type="dpmsolver++", correcting_x0_fn=ImageSpaceClamp(cond[:, :C], 0.0, 1.0))
    assert slv._fused_target() is not None  # the whole run inside libddif
    out = slv.sample(xT, steps=steps, order=order, skip_type="time_uniform", method="multistep")
    _compare(out, g, f"{stem}_{pm}", (tiles["cond"][:, :C], tiles["gt"]), relative=True)


def run_loss(case, pm, dev, monkeypatch):
    import ddif.diffusion.diffusion_ddpm_pan as M

    stem, ds, B, H, W, T, tvals, sc_branch, seed = case
    g = load(f"{stem}_{pm}")
    C = gc.DATASETS[ds][0]
    tiles = gc.tiles_for(ds, B, H, W, seed=seed)
    res = (tiles["gt"] - tiles["lms"]).to(dev)
    noise = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed)).to(dev)
    tt = torch.tensor(tvals, dtype=torch.long, device=dev)
    monkeypatch.setattr(M.torch, "randint", lambda *a, **k: tt)
    monkeypatch.setattr(M.random, "random", (lambda: 0.0) if sc_branch else (lambda: 1.0))
    for lt in go.LOSS_TYPES:
        for gamma in go.P2_GAMMAS:
            k = go.loss_key(lt, gamma)
            d = diffusion(ds, T, H, dev, pm, loss_type=lt, gamma=gamma)
            loss, recon = d(res, mode="train", noise=noise, cond=tiles["cond"].to(dev))
            check_gap(g[f"gap::loss_{k}"], 1e-6, f"{stem}_{pm} {k} loss")
            ref_recon = torch.from_numpy(g[f"recon_{k}"])
            check_gap(g[f"gap::recon_{k}"], 2e-5, f"{stem}_{pm} {k} recon")
            el, er = abs(float(loss) - float(g[f"loss_{k}"].reshape(-1)[0])), float((recon.cpu() - ref_recon).abs().max())
            print(f"{stem}_{pm} {k}: |loss - golden| {el:.3e} (loss {float(loss):.6f}), max|recon - golden| {er:.3e}")
            assert el <= 1e-6, (k, el)
            assert er <= 2e-5, (k, er)


def _masks(g):
    masks = []
    for k in range(int(g["n_drop"])):
        shp = tuple(int(v) for v in g[f"drop_{k}_shape"])
        bits = np.unpackbits(g[f"drop_{k}"])[: int(np.prod(shp))].reshape(shp)
        masks.append(torch.from_numpy(bits.astype(np.float32)) / (1.0 - float(g["p_drop"])))
    return masks, torch.from_numpy(g["paths"])


def run_grad(case, dev, monkeypatch):
    """The drop-in's own p_losses(...).backward() under .train() with the reference's masks pinned: loss, recon_x0, the gradient norm of every
    parameter and the full gradients the golden carries."""
    import ddif.diffusion.diffusion_ddpm_pan as M

    cid, ds, B, H, W, T, tvals, pm, lt, gamma, seed = case
    g = load(cid)
    check_gap(g["gap::loss"], 1e-6, f"{cid} loss")
    check_gap(g["gap::grad_norms_rel"], 2e-4, f"{cid} gradient norms (relative)")
    check_gap(g["gap::grad_full_rel"], 5e-5, f"{cid} full gradients (relative)")
    C = gc.DATASETS[ds][0]
    tiles = gc.tiles_for(ds, B, H, W, seed=seed)
    res = (tiles["gt"] - tiles["lms"]).to(dev)
    noise = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed)).to(dev)
    tt = torch.tensor(tvals, dtype=torch.long, device=dev)
    monkeypatch.setattr(M.torch, "randint", lambda *a, **k: tt)
    monkeypatch.setattr(M.random, "random", lambda: 1.0)
    masks, paths = _masks(g)
    net = make_net(ds, dev).train()  # a net of its own: the step refreshes the packed weights on the device
    try:
        from ddif.diffusion.diffusion_ddpm_pan import GaussianDiffusion, make_beta_schedule

        d = GaussianDiffusion(net, image_size=H, channels=C, pred_mode=pm, loss_type=lt, device=dev, clamp_range=(0, 1), p2_loss_weight_gamma=gamma)
        d.set_new_noise_schedule(betas=make_beta_schedule(schedule="cosine", n_timestep=T, cosine_s=8e-3), device=dev)
        net.set_train_masks([m.to(dev) for m in masks], paths)
        for p in net.parameters():
            p.grad = None
        loss, recon = d(res, mode="train", noise=noise, cond=tiles["cond"].to(dev))
        loss.backward()
        el = abs(float(loss.detach()) - float(g["loss"]))
        er = float((recon.detach().cpu() - torch.from_numpy(g["recon"])).abs().max())
        print(f"{cid}: |loss - golden| {el:.3e} (loss {float(g['loss']):.6f}), max|recon - golden| {er:.3e}")
        assert el <= 1e-6, el
        assert er <= 2e-5, er
        grads = {n: p.grad for n, p in net.named_parameters()}
        names = [str(n) for n in g["names"]]
        assert set(names) == set(grads.keys())
        worst = 0.0
        for n, ref in zip(names, g["grad_norms"]):
            assert grads[n] is not None, f"no gradient for {n}"
            got = float(grads[n].double().norm())
            assert got == got, f"gradient of {n} was not written"
            worst = max(worst, abs(got - float(ref)) / max(float(ref), 1e-4))
            assert abs(got - float(ref)) <= 2e-4 * max(float(ref), 1e-4), (n, got, float(ref))
        for k in g.files:
            if k.startswith("grad::"):
                ref = torch.from_numpy(g[k])
                got = grads[k[6:]].cpu()
                assert got.shape == ref.shape, k
                err = float((got - ref).abs().max())
                assert err <= 5e-5 * max(float(ref.abs().max()), 1e-5), (k, err, float(ref.abs().max()))
        print(f"{cid}: worst relative grad-norm error over {len(names)} parameters: {worst:.2e}")
    finally:
        net.set_train_masks(None, None)
        net.eval()


def run_default_objective_is_bit_identical(dev):
    """A plan whose objective is set EXPLICITLY to (x_start, l1) -- also after a detour through another objective -- reproduces the default path bit for
    bit, for a DDPM run and for a training step, with the same number of launches."""
    ds, B, H, W, T, steps = "wv3", 2, 16, 16, 20, 4
    C = gc.DATASETS[ds][0]
    tiles = gc.tiles_for(ds, B, H, W, seed=9)
    cond = tiles["cond"].to(dev)
    gen = torch.Generator().manual_seed(9)
    xT = torch.randn(B, C, H, W, generator=gen)
    noise = torch.randn(steps, B, C, H, W, generator=gen)
    d = diffusion(ds, T, H, dev, "x_start", "l1")
    c1, c2 = d.posterior_mean_coef1.cpu(), d.posterior_mean_coef2.cpu()
    cz = (0.5 * d.posterior_log_variance_clipped.cpu()).exp()
    order = list(reversed(range(T)))[:steps]
    args = ([float(i) for i in order], [float(c1[i]) for i in order], [float(c2[i]) for i in order], [float(cz[i]) for i in order], xT.to(dev),
            noise.to(dev).contiguous(), 0, 0, (0.0, 1.0), dev)
    net = make_net(ds, dev)  # a net (and plan) of its own: no earlier test has stated an objective on it
    plan = net.plan_for(B, H, W, dev)
    assert plan.objective == ("x_start", "l1")
    plan.set_cond(cond, force=True)
    n0 = plan.num_launches()
    base = plan.sample_ddpm(*args).clone()  # the default path: no objective call has reached the library
    assert plan.get_objective() == ("x_start", "l1")  # what the library holds for a new plan
    plan.lib.check(plan.lib.dll.ddif_plan_set_objective(plan.h, 0, 0), "ddif_plan_set_objective")  # explicitly (x_start, l1)
    assert plan.num_launches() == n0
    assert torch.equal(plan.sample_ddpm(*args), base)
    sr, srm1 = d.sqrt_recip_alphas_cumprod.cpu(), d.sqrt_recipm1_alphas_cumprod.cpu()
    plan.set_objective("noise", "l2")
    assert plan.get_objective() == ("noise", "l2")  # sticky in the library, not only in the Python handle
    assert plan.num_launches() == n0
    other = plan.sample_ddpm(*args, pred=([float(sr[i]) for i in order], [float(srm1[i]) for i in order])).clone()
    assert not torch.equal(other, base)
    plan.set_objective("x_start", "l1")
    assert plan.get_objective() == ("x_start", "l1")
    assert plan.num_launches() == n0
    again = plan.sample_ddpm(*args)
    assert torch.equal(again, base)

    tnet = make_net(ds, dev).train()
    try:
        tplan = tnet.plan_for(B, H, W, dev, train=True)
        tnet._net.refresh_from_device(tnet.named_parameters())
        tplan.set_cond(cond, force=True)
        tplan.random_train_masks(77, 0, 0.2, 0.2)
        grads = {n: torch.full_like(p, float("nan")) for n, p in tnet.named_parameters()}
        tplan.train_bind(list(grads.items()))
        x0 = (tiles["gt"] - tiles["lms"]).to(dev)
        z = noise[0].to(dev)
        t = torch.tensor([3, 17], dtype=torch.long, device=dev)
        a, s = d._schedule_rows(t)
        n1 = tplan.num_launches()
        l0, p0 = tplan.train_step(x0, z, a, s, t, None)
        l0, p0 = l0.clone(), p0.clone()
        g0 = {n: v.clone() for n, v in grads.items()}
        tplan.lib.check(tplan.lib.dll.ddif_plan_set_objective(tplan.h, 0, 0), "ddif_plan_set_objective")  # explicitly (x_start, l1)
        le, pe = tplan.train_step(x0, z, a, s, t, None)
        assert torch.equal(le, l0) and torch.equal(pe, p0) and all(torch.equal(grads[n], g0[n]) for n in g0)
        tplan.set_objective("pred_v", "l2")
        assert tplan.get_objective() == ("pred_v", "l2")
        tplan.train_step(x0, z, a, s, t, None, rows=(a, s, None))
        assert not torch.equal(grads["final_conv.block.3.weight"], g0["final_conv.block.3.weight"])
        tplan.set_objective("x_start", "l1")
        assert tplan.num_launches() == n1
        l1, p1 = tplan.train_step(x0, z, a, s, t, None)
        assert torch.equal(l1, l0) and torch.equal(p1, p0)
        for n in g0:
            assert torch.isfinite(g0[n]).all() and torch.equal(grads[n], g0[n]), n
    finally:
        tnet.eval()


def run_plain_entry_points_refuse_a_prediction_objective(dev):
    """The plain sampler entry points cannot serve a noise / v plan (no conversion tables): DdifError, not a wrong image."""
    import ctypes as C_

    from ddif import DdifError
    from ddif.runtime import DdpmTables, _FP, _farr, _ptr

    ds, B, H, W = "wv3", 1, 16, 16
    C = gc.DATASETS[ds][0]
    net = net_for(ds, dev)
    plan = net.plan_for(B, H, W, dev)
    plan.set_cond(gc.tiles_for(ds, B, H, W, seed=2)["cond"].to(dev), force=True)
    plan.set_objective("noise", "l1")
    try:
        keep = [_farr([1.0]), _farr([0.5]), _farr([0.5]), _farr([0.0])]
        tabs = DdpmTables(1, *[C_.cast(a, _FP) for a in keep])
        xT = torch.zeros(B, C, H, W, device=dev)
        out = torch.empty_like(xT)
        rc = plan.lib.dll.ddif_plan_sample_ddpm(plan.h, C_.byref(tabs), _ptr(xT), None, 0, 0, 0.0, 1.0, 1, _ptr(out), None)
        assert rc == -1  # DDIF_ERR_INVALID
        try:
            plan.sample_ddpm([1.0], [0.5], [0.5], [0.0], xT, None, 0, 0, (0.0, 1.0), dev)
            raise AssertionError("expected DdifError")
        except DdifError:
            pass
    finally:
        plan.set_objective("x_start", "l1")
