"""The checks of loss_type="l1ssim", shared by tests/test_l1ssim_emu.py (host-emulated build, CPU tensors) and tests/test_l1ssim_gpu.py (the gfx950 library):
every golden of tests/golden_cases_l1ssim.py -- the real reference's HybridL1SSIM, p_losses and p_losses(...).backward(), fp32 with the fp64 twin on file --
through the C ABI (ddif_l1ssim_loss, ddif_plan_set_objective with DDIF_LOSS_L1SSIM) and the drop-in classes.

Tolerances are the project's existing bars (tests/objective_parity.py): loss values 1e-6; recon_x0 2e-5; gradient norms 2e-4 * max(ref, 1e-4); gradients
5e-5 * max(max|ref|, 1e-5).  Every golden stores the reference's own fp32 <-> fp64 gap; `check_gap` asserts it is below a tenth of the tolerance used."""
from __future__ import annotations

import torch

import golden_cases as gc
import golden_cases_l1ssim as gl
from ddif_testlib import make_net
from objective_parity import _masks, check_gap, load

_golden = {}


def golden(name):
    if name not in _golden:
        _golden[name] = load(name)
    return _golden[name]


def _diffusion(net, ds, T, size, dev, pred_mode, gamma):
    from ddif.diffusion.diffusion_ddpm_pan import GaussianDiffusion, HybridL1SSIM, make_beta_schedule

    d = GaussianDiffusion(net, image_size=size, channels=gc.DATASETS[ds][0], pred_mode=pred_mode, loss_type="l1ssim", device=dev, clamp_range=(0, 1),
                          p2_loss_weight_gamma=gamma)
    d.set_new_noise_schedule(betas=make_beta_schedule(schedule="cosine", n_timestep=T, cosine_s=8e-3), device=dev)
    assert isinstance(d.loss_func, HybridL1SSIM) and d.loss_func.weighted_r == gl.WEIGHTS
    return d


_nets = {}


def _net_for(ds, dev):
    key = (ds, str(dev))
    if key not in _nets:
        _nets[key] = make_net(ds, dev)
    return _nets[key]


def _grad_err(got, ref):
    return float((got.cpu() - ref).abs().max()), 5e-5 * max(float(ref.abs().max()), 1e-5)


def run_op(case, dev, nhwc):
    """ddif_l1ssim_loss on the golden's inputs, in one layout: the value, the gradient with respect to img2 and -- arguments swapped -- to img1, twice."""
    from ddif import runtime as rt

    cid = case[0]
    g = golden(cid)
    check_gap(g["gap::loss"], 1e-6, f"{cid} loss")
    check_gap(g["gap::grad1_rel"], 5e-5, f"{cid} d/d img1 (relative)")
    check_gap(g["gap::grad2_rel"], 5e-5, f"{cid} d/d img2 (relative)")
    x, y = torch.from_numpy(g["x"]), torch.from_numpy(g["y"])
    assert torch.equal(x, gl.op_inputs(case)[0]) and torch.equal(y, gl.op_inputs(case)[1])  # the stored inputs are the seeded ones
    to = (lambda v: v.permute(0, 2, 3, 1).contiguous().to(dev)) if nhwc else (lambda v: v.to(dev))
    back = (lambda v: v.permute(0, 3, 1, 2).cpu()) if nhwc else (lambda v: v.cpu())
    a, b = to(x), to(y)
    assert float(rt.l1ssim_loss(a, b, gl.WEIGHTS, nhwc=nhwc)) == float(rt.l1ssim_loss(a, b, gl.WEIGHTS, grad=True, nhwc=nhwc)[0])  # value-only call = the full one
    for which, (p, q), key in (("img2", (a, b), "grad2"), ("img1", (b, a), "grad1")):
        loss, grad = rt.l1ssim_loss(p, q, gl.WEIGHTS, grad=True, nhwc=nhwc)
        loss2, grad2 = rt.l1ssim_loss(p, q, gl.WEIGHTS, grad=True, nhwc=nhwc)
        el = abs(float(loss) - float(g["loss"].reshape(-1)[0]))
        eg, tol = _grad_err(back(grad), torch.from_numpy(g[key]))
        print(f"{cid} {'nhwc' if nhwc else 'nchw'} d/d {which}: |loss - golden| {el:.3e} (loss {float(loss):.7f}), max|grad - golden| {eg:.3e} (tolerance {tol:.3e})")
        assert el <= 1e-6, (cid, which, el)
        assert bool(torch.isfinite(grad).all()) and eg <= tol, (cid, which, eg, tol)
        assert torch.equal(loss, loss2) and torch.equal(grad, grad2), f"{cid}: two calls differ"
    # upstream scales the gradient and nothing else
    _, gh = rt.l1ssim_loss(a, b, gl.WEIGHTS, grad=True, upstream=0.5, nhwc=nhwc)
    assert torch.equal(gh * 2, rt.l1ssim_loss(a, b, gl.WEIGHTS, grad=True, nhwc=nhwc)[1])


def run_op_identical_arguments(case, dev):
    from ddif import runtime as rt

    x = torch.from_numpy(golden(case[0])["x"]).to(dev)
    loss, grad = rt.l1ssim_loss(x, x.clone(), gl.WEIGHTS, grad=True)
    print(f"{case[0]} img2 = img1: loss {float(loss):.3e}, max|grad| {float(grad.abs().max()):.3e}")
    assert abs(float(loss)) <= 1e-6
    assert bool(torch.isfinite(grad).all())


def run_op_module(case, dev):
    """HybridL1SSIM(...)(a, b).backward() through the drop-in module: the golden's value and both gradients, and one argument alone."""
    from ddif.diffusion.diffusion_ddpm_pan import HybridL1SSIM

    cid, C = case[0], case[2]
    g = golden(cid)
    a = torch.from_numpy(g["x"]).to(dev).requires_grad_(True)
    b = torch.from_numpy(g["y"]).to(dev).requires_grad_(True)
    loss = HybridL1SSIM(channel=C)(a, b)
    assert loss.dim() == 0
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"].reshape(-1)[0])) <= 1e-6
    for t, key in ((a, "grad1"), (b, "grad2")):
        eg, tol = _grad_err(t.grad, torch.from_numpy(g[key]))
        print(f"{cid} module {key}: max|grad - golden| {eg:.3e} (tolerance {tol:.3e})")
        assert eg <= tol, (cid, key, eg, tol)
    b2 = torch.from_numpy(g["y"]).to(dev).requires_grad_(True)
    (HybridL1SSIM(channel=C, weighted_r=gl.WEIGHTS)(a.detach(), b2) * 3.0).backward()  # the target carries no gradient, as in p_losses; upstream 3
    eg, tol = _grad_err(b2.grad / 3.0, torch.from_numpy(g["grad2"]))
    assert eg <= tol, (cid, eg, tol)


def run_loss(case, pm, dev, monkeypatch):
    import ddif.diffusion.diffusion_ddpm_pan as M

    stem, ds, B, H, W, T, tvals, sc_branch, seed = case
    g = golden(f"{stem}_{pm}")
    C = gc.DATASETS[ds][0]
    tiles = gc.tiles_for(ds, B, H, W, seed=seed)
    res = (tiles["gt"] - tiles["lms"]).to(dev)
    noise = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed)).to(dev)
    tt = torch.tensor(tvals, dtype=torch.long, device=dev)
    monkeypatch.setattr(M.torch, "randint", lambda *a, **k: tt)
    monkeypatch.setattr(M.random, "random", (lambda: 0.0) if sc_branch else (lambda: 1.0))
    for gamma in gl.P2_GAMMAS:
        k = gl.loss_key(gamma)
        d = _diffusion(_net_for(ds, dev), ds, T, H, dev, pm, gamma)
        loss, recon = d(res, mode="train", noise=noise, cond=tiles["cond"].to(dev))
        check_gap(g[f"gap::loss_{k}"], 1e-6, f"{stem}_{pm} {k} loss")
        check_gap(g[f"gap::recon_{k}"], 2e-5, f"{stem}_{pm} {k} recon")
        el = abs(float(loss) - float(g[f"loss_{k}"].reshape(-1)[0]))
        er = float((recon.cpu() - torch.from_numpy(g[f"recon_{k}"])).abs().max())
        print(f"{stem}_{pm} {k}: |loss - golden| {el:.3e} (loss {float(loss):.6f}), max|recon - golden| {er:.3e}")
        assert el <= 1e-6, (k, el)
        assert er <= 2e-5, (k, er)


def run_grad(case, dev, monkeypatch):
    """The drop-in's own p_losses(...).backward() under .train() with the reference's masks pinned -- loss, recon_x0, the gradient norm of every parameter and
    the full gradients the golden carries -- then the same step through train_step_into: the same loss and bit-equal gradients."""
    import ddif.diffusion.diffusion_ddpm_pan as M

    cid, ds, B, H, W, T, tvals, pm, gamma, seed = case
    g = golden(cid)
    check_gap(g["gap::loss"], 1e-6, f"{cid} loss")
    check_gap(g["gap::recon"], 2e-5, f"{cid} recon")
    check_gap(g["gap::grad_norms_rel"], 2e-4, f"{cid} gradient norms (relative)")
    check_gap(g["gap::grad_full_rel"], 5e-5, f"{cid} full gradients (relative)")
    C = gc.DATASETS[ds][0]
    tiles = gc.tiles_for(ds, B, H, W, seed=seed)
    res = (tiles["gt"] - tiles["lms"]).to(dev)
    cond = tiles["cond"].to(dev)
    noise = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(seed)).to(dev)
    tt = torch.tensor(tvals, dtype=torch.long, device=dev)
    monkeypatch.setattr(M.torch, "randint", lambda *a, **k: tt)
    monkeypatch.setattr(M.random, "random", lambda: 1.0)
    masks, paths = _masks(g)
    net = make_net(ds, dev).train()  # a net of its own: the step refreshes the packed weights on the device
    try:
        d = _diffusion(net, ds, T, H, dev, pm, gamma)
        net.set_train_masks([m.to(dev) for m in masks], paths)
        for p in net.parameters():
            p.grad = None
        loss, recon = d(res, mode="train", noise=noise, cond=cond)
        loss.backward()
        assert net.plan_for(B, H, W, dev, train=True).get_objective() == (pm, "l1ssim")  # what the library holds for the plan that ran the step
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
        worst_full = 0.0
        for k in g.files:
            if k.startswith("grad::"):
                ref = torch.from_numpy(g[k])
                got = grads[k[6:]].cpu()
                assert got.shape == ref.shape, k
                err, tol = _grad_err(got, ref)
                worst_full = max(worst_full, err / tol * 5e-5)
                assert err <= tol, (k, err, tol)
        print(f"{cid}: worst relative grad-norm error over {len(names)} parameters {worst:.2e}, worst relative full-gradient error {worst_full:.2e}")
        # the engine's entry: gradients written straight into given tensors
        into = [torch.full_like(p, float("nan")) for p in net.parameters()]
        loss2, recon2 = d.train_step_into(res, cond, into, noise=noise)
        assert torch.equal(loss2.detach().reshape(()), loss.detach().reshape(())) and torch.equal(recon2, recon.detach())
        for (n, p), t in zip(net.named_parameters(), into):
            assert torch.equal(t, p.grad), f"train_step_into: the gradient of {n} differs from p_losses(...).backward()"
    finally:
        net.set_train_masks(None, None)
        net.eval()


def run_default_path_untouched(dev):
    """A sampling plan and a training plan set to (x_start, l1ssim) and back to (x_start, l1): the DDPM run, and the l1 step's loss, prediction and every
    gradient, reproduce bit for bit with the same number of launches; get_objective() reports l1ssim while it is set."""
    from objective_parity import diffusion

    ds, B, H, W, T, steps = "wv3", 2, 16, 16, 20, 2
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
    plan.set_cond(cond, force=True)
    n0 = plan.num_launches()
    base = plan.sample_ddpm(*args).clone()
    m0 = plan.memory()["total_bytes"]  # (after the first run: the sampler's tables are allocated on first use)
    plan.set_objective("x_start", "l1ssim")
    assert plan.get_objective() == ("x_start", "l1ssim")  # sticky in the library, not only in the Python handle
    assert plan.num_launches() == n0
    assert plan.memory()["total_bytes"] == m0  # the maps scratch belongs to plans that train under the loss
    assert torch.equal(plan.sample_ddpm(*args), base)  # the loss does not concern a sampler
    plan.set_objective("x_start", "l1")
    assert plan.get_objective() == ("x_start", "l1") and plan.num_launches() == n0
    assert torch.equal(plan.sample_ddpm(*args), base)

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
        n1, m1 = tplan.num_launches(), tplan.memory()["total_bytes"]
        l0, p0 = tplan.train_step(x0, z, a, s, t, None)
        l0, p0 = l0.clone(), p0.clone()
        g0 = {n: v.clone() for n, v in grads.items()}
        tplan.set_objective("x_start", "l1ssim")
        assert tplan.get_objective() == ("x_start", "l1ssim")
        assert tplan.memory()["total_bytes"] >= m1 + 3 * 4 * x0.numel()  # the three maps, allocated now
        ls, ps = tplan.train_step(x0, z, a, s, t, None)
        assert torch.equal(ps, p0)  # the same forward ...
        assert not torch.equal(ls, l0) and not torch.equal(grads["final_conv.block.3.weight"], g0["final_conv.block.3.weight"])  # ... under another loss
        assert all(bool(torch.isfinite(v).all()) for v in grads.values())
        tplan.set_objective("x_start", "l1")
        assert tplan.get_objective() == ("x_start", "l1") and tplan.num_launches() == n1
        l1, p1 = tplan.train_step(x0, z, a, s, t, None)
        assert torch.equal(l1, l0) and torch.equal(p1, p0)
        for n in g0:
            assert bool(torch.isfinite(g0[n]).all()) and torch.equal(grads[n], g0[n]), n
    finally:
        tnet.eval()


def run_refusal_gone(dev):
    from ddif.diffusion.diffusion_ddpm_pan import GaussianDiffusion, HybridL1SSIM

    d = GaussianDiffusion(_net_for("wv3", dev), image_size=16, channels=8, loss_type="l1ssim", device=dev)  # the reference's other defaults
    assert isinstance(d.loss_func, HybridL1SSIM) and d.loss_type == "l1ssim"


def run_bad_arguments(dev):
    from ddif import DdifError
    from ddif import runtime as rt

    x = torch.zeros(1, 2, 4, 4, device=dev)
    for bad in (lambda: rt.l1ssim_loss(x, torch.zeros(1, 2, 4, 5, device=dev)), lambda: rt.l1ssim_loss(x[0], x[0]), lambda: rt.l1ssim_loss(x, x, (1.0,))):
        try:
            bad()
            raise AssertionError("expected DdifError")
        except DdifError:
            pass
