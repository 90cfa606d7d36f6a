"""The checks of overlapping tiles with per-step fusion (include/ddif.h ddif_plan_set_tiling, ddif_tiles_cut, ddif_tiles_blend), shared by
tests/test_tiling_emu.py (host-emulated build, CPU tensors) and tests/test_tiling_gpu.py (the gfx950 library).

Common shape: the gf2 fixture net (C = 4), tile 16 x 16, scene 24 x 36, overlap 8 -> ys = [0, 8], xs = [0, 8, 16, 20]: 8 tiles, a last column shifted flush
with the border, a band with three covers in x and so up to six covers per pixel.  Runs are 4 steps (enough for the GPU library to capture and replay its
step pair).

Tolerances: none.  Every comparison is bit equality (torch.equal):
  * cut / blend kernels against the torch restatement in ddif/sharding.py -- both are the same IEEE fp32 operations in the same order (den exact,
    r_k = w_k / den, out = (v_0 + r_1 (v_1 - v_0)) + r_2 (v_2 - v_0) ..., contraction off);
  * a fused run against the step-by-step yardstick: the network is deterministic and a tile of a batch is bit-equal to the tile alone, the yardstick runs
    the same unfused update kernel, so nothing but the fusion differs, and the fusion is the blend above;
  * tiling on at overlap 0 against tiling off: the unfused update kernel against the sampler epilogue of the final conv, which evaluate the same
    expressions operand for operand (csrc/kernels_misc.h ddpm_step_kernel / ddim_step_kernel);
  * the noise checks compare the library's normals with themselves under another tiling of the same scene.
These pin the MECHANICS of tiling.  Seam quality cannot be judged with the random-init fixture weights and is not."""
from __future__ import annotations

import numpy as np
import torch

import golden_cases as gc
from ddif_testlib import make_net

DS, TILE, HS, WS, OV, T, STEPS = "gf2", 16, 24, 36, 8, 20, 4
C_ = gc.DATASETS[DS][0]
YS, XS = [0, 8], [0, 8, 16, 20]
_CTX = {}


def _diffusion(dev, pred_mode="x_start"):
    """One network + diffusion per (library, device, objective) for the whole module: plans are cached on the network."""
    from ddif import runtime
    from ddif.diffusion.diffusion_ddpm_pan import GaussianDiffusion, make_beta_schedule

    key = (runtime.library_loaded_path(), str(dev), pred_mode)
    if key not in _CTX:
        d = GaussianDiffusion(make_net(DS, dev), image_size=TILE, channels=C_, pred_mode=pred_mode, loss_type="l2", device=dev, clamp_range=(0, 1))
        d.set_new_noise_schedule(betas=make_beta_schedule(schedule="cosine", n_timestep=T, cosine_s=8e-3), device=dev)
        _CTX[key] = d
    return _CTX[key]


def _plan(d, cond, tiling):
    plan = d.model.plan_for(cond.shape[0], cond.shape[2], cond.shape[3], cond.device)
    plan.set_objective(d.pred_mode, "l2")
    plan.set_threshold("off")
    plan.set_tiling(tiling)
    plan.set_cond(cond, force=True)
    return plan


def _ddpm(d, plan, xT, noise, dev, k0=0, steps=STEPS, seed=0, tile0=0, clamp=(0.0, 1.0)):
    order = list(reversed(range(T)))[k0:k0 + steps]
    c1, c2 = d.posterior_mean_coef1.cpu(), d.posterior_mean_coef2.cpu()
    cz = (0.5 * d.posterior_log_variance_clipped.cpu()).exp()
    return plan.sample_ddpm([float(i) for i in order], [float(c1[i]) for i in order], [float(c2[i]) for i in order], [float(cz[i]) for i in order], xT, noise,
                            seed, tile0, clamp, dev, pred=d._pred_tables(order)).clone()


def _ddim(d, plan, xT, noise, dev, k0=0, steps=STEPS, seed=0, tile0=0, eta=1.0):
    order = list(reversed(range(T)))[k0:k0 + steps]
    a, ap = d.alphas_cumprod.cpu(), d.alphas_cumprod_prev.cpu()
    sigma = eta * torch.sqrt((1 - ap) / (1 - a)) * torch.sqrt(1 - a / ap)
    dirc = torch.sqrt(1 - ap - sigma ** 2)
    sr, srm1 = d.sqrt_recip_alphas_cumprod.cpu(), d.sqrt_recipm1_alphas_cumprod.cpu()
    return plan.sample_ddim([float(j) for j in order], [float(sr[j]) for j in order], [float(srm1[j]) for j in order], [float(torch.sqrt(ap[j])) for j in order],
                            [float(dirc[j]) for j in order], [float(sigma[j]) for j in order], xT, noise, seed, tile0, None, dev, pred=d._pred_tables(order)).clone()


def _scene_fields(S, seed, dev):
    """cond of S scenes cut into tiles, and a scene-sized x_T / per-step noise cut the same way (so that they agree in the overlaps)."""
    from ddif.sharding import cut_tiles_torch

    cond = cut_tiles_torch(gc.tiles_for(DS, S, HS, WS, seed=seed)["cond"], TILE, OV)
    g = torch.Generator().manual_seed(seed)
    xT = cut_tiles_torch(torch.randn(S, C_, HS, WS, generator=g), TILE, OV)
    noise = torch.stack([cut_tiles_torch(torch.randn(S, C_, HS, WS, generator=g), TILE, OV) for _ in range(STEPS)])
    return cond.to(dev), xT.to(dev), noise.to(dev)


def _copy_stitch(tiles, H, W, overlap, S=1):
    """Paste the tiles in ascending order (later covers overwrite earlier ones)."""
    from ddif.sharding import tile_grid

    ys, xs = tile_grid(H, W, tiles.shape[-1], overlap)
    t, per = tiles.shape[-1], len(ys) * len(xs)
    out = torch.empty((S, tiles.shape[1], H, W), dtype=tiles.dtype)
    for s in range(S):
        for k, (py, px) in enumerate((py, px) for py in ys for px in xs):
            out[s, :, py:py + t, px:px + t] = tiles[s * per + k].cpu()
    return out


# ---- 2. cut / blend kernels against the torch restatement -------------------------------------------------------------------------------------------------
def run_cut_blend(dev, Cc):
    from ddif import runtime as R
    from ddif.sharding import blend_tiles_torch, cut_tiles_torch, tile_grid

    g = torch.Generator().manual_seed(100 + Cc)
    for S, H, W, t, ov in ((1, HS, WS, TILE, OV), (2, HS, WS, TILE, OV), (1, 33, 17, 16, 5), (2, 16, 40, 16, 12), (1, 32, 32, 16, 0)):
        ys, xs = tile_grid(H, W, t, ov)
        per = len(ys) * len(xs)
        scene = torch.randn(S, Cc, H, W, generator=g)
        tiles = R.tiles_cut(scene.to(dev), t, ov, per).cpu()
        assert tiles.shape == (S * per, Cc, t, t)
        assert torch.equal(tiles, cut_tiles_torch(scene, t, ov)), ("cut", S, H, W, t, ov)
        assert torch.equal(R.tiles_blend(tiles.to(dev), S, H, W, ov).cpu(), scene), ("blend(cut(scene)) == scene", S, H, W, t, ov)  # equal inputs give v_0
        rnd = torch.randn(S * per, Cc, t, t, generator=g)  # unequal tiles: the weighted blend itself
        want = blend_tiles_torch(rnd, H, W, ov, S)
        got = R.tiles_blend(rnd.to(dev), S, H, W, ov).cpu()
        assert torch.equal(got, want), ("blend", S, H, W, t, ov, float((got - want).abs().max()))
        if ov and per > 1:
            assert not torch.equal(got, _copy_stitch(rnd, H, W, ov, S))  # (the blend does something)


# ---- 3. tiling on at overlap 0 == tiling off ------------------------------------------------------------------------------------------------------------------
def run_overlap0_equals_untiled(dev, sampler):
    """2 x 2 tiles of a 32 x 32 scene, host x_T and noise.  Tiling on takes the unfused tail (update kernel as a launch of its own, nothing to fuse), tiling off the
    sampler epilogue of the final conv: the same expressions, the same bits."""
    from ddif.sharding import cut_tiles

    d = _diffusion(dev, "x_start" if sampler == "ddpm" else "noise")
    cond = cut_tiles(gc.tiles_for(DS, 1, 32, 32, seed=31)["cond"][0], TILE).to(dev)
    g = torch.Generator().manual_seed(31)
    xT = torch.randn(4, C_, TILE, TILE, generator=g).to(dev)
    noise = torch.randn(STEPS, 4, C_, TILE, TILE, generator=g).to(dev)
    run = _ddpm if sampler == "ddpm" else _ddim
    plan = _plan(d, cond, None)
    n0 = plan.num_launches()["step"]
    off = run(d, plan, xT, noise, dev)
    plan.set_tiling((1, 32, 32, 0))
    assert plan.num_launches()["step"] == n0 + 2  # update + counter; no fusion launch at overlap 0
    on = run(d, plan, xT, noise, dev)
    diff = float((on - off).abs().max())
    print(f"{sampler}: tiling on at overlap 0 vs off: max|diff| = {diff:.3e}")
    assert torch.equal(on, off), diff
    plan.set_tiling(None)
    assert plan.num_launches()["step"] == n0
    assert torch.equal(run(d, plan, xT, noise, dev), off)


# ---- 4. one fused call == the step-by-step yardstick ----------------------------------------------------------------------------------------------------------
def run_fused_equals_yardstick(dev, sampler):
    from ddif.sharding import blend_tiles_torch, cut_tiles_torch

    d = _diffusion(dev)
    cond, xT, noise = _scene_fields(1, 41, dev)
    run = _ddpm if sampler == "ddpm" else _ddim
    plan = _plan(d, cond, (1, HS, WS, OV))
    n_t = plan.num_launches()["step"]
    fused = run(d, plan, xT, noise, dev)
    plan.set_tiling((8, TILE, TILE, 0))  # eight one-tile scenes: the same unfused update kernel, nothing fused
    assert plan.num_launches()["step"] == n_t - 1
    img = xT
    for k in range(STEPS):
        out = run(d, plan, img, noise[k:k + 1].contiguous(), dev, k0=k, steps=1)
        img = cut_tiles_torch(blend_tiles_torch(out.cpu(), HS, WS, OV), TILE, OV).to(dev)
    diff = float((fused - img).abs().max())
    print(f"{sampler}: fused call vs step-by-step yardstick: max|diff| = {diff:.3e}")
    assert torch.equal(fused, img), diff
    unfused = run(d, plan, xT, noise, dev)  # (the fusion matters: independent tiles end elsewhere)
    assert not torch.equal(unfused, fused)
    plan.set_tiling(None)


# ---- 5. covers agree --------------------------------------------------------------------------------------------------------------------------------------------
def run_covers_agree(dev):
    from ddif.sharding import blend_tiles, cut_tiles_torch

    d = _diffusion(dev)
    cond, _, _ = _scene_fields(1, 51, dev)
    plan = _plan(d, cond, (1, HS, WS, OV))
    a = _ddpm(d, plan, None, None, dev, seed=7)
    b = _ddpm(d, plan, None, None, dev, seed=7)
    assert torch.equal(a, b)  # two runs are bit-identical
    stitched = _copy_stitch(a, HS, WS, OV)
    assert torch.equal(cut_tiles_torch(stitched, TILE, OV), a.cpu())  # every cover holds the bits of the last one pasted: all covers agree
    assert torch.equal(blend_tiles(a, HS, WS, OV).cpu(), stitched[0])  # ... so the blend reduces to copies (the kernel on GPU tensors)
    assert bool(torch.isfinite(a).all())
    plan.set_tiling(None)


# ---- 6. noise is per scene pixel ---------------------------------------------------------------------------------------------------------------------------------
def run_noise_is_per_scene_pixel(dev):
    """DDPM, one step, caller tables: (coef_x0, coef_xt, coef_z) = (0, 0, 1) returns the step's z, (0, 1, 0) returns x_T -- after the fusion, which changes no
    bit of covers that agree.  Stitched, both are the same field for overlap 8 and overlap 12 on the same scene and seed; tile-keyed noise fails that."""
    from ddif.sharding import cut_tiles_torch, tile_grid

    d = _diffusion(dev)

    def field(S, ov, seed, tile0, tabs):
        cond = cut_tiles_torch(gc.tiles_for(DS, S, HS, WS, seed=61)["cond"], TILE, ov).to(dev)
        plan = _plan(d, cond, (S, HS, WS, ov))
        out = plan.sample_ddpm([float(T - 1)], [tabs[0]], [tabs[1]], [tabs[2]], None, None, seed, tile0, None, dev).clone()
        st = _copy_stitch(out, HS, WS, ov, S)
        assert torch.equal(cut_tiles_torch(st, TILE, ov), out.cpu())  # the covers agree
        plan.set_tiling(None)
        return st

    assert tile_grid(HS, WS, TILE, 12) == ([0, 4, 8], [0, 4, 8, 12, 16, 20])
    z8 = field(1, OV, 5, 0, (0.0, 0.0, 1.0))
    assert torch.equal(z8, field(1, 12, 5, 0, (0.0, 0.0, 1.0)))
    assert not torch.equal(z8, field(1, OV, 6, 0, (0.0, 0.0, 1.0)))  # another seed, another field
    assert abs(float(z8.mean())) < 0.1 and 0.9 < float(z8.std()) < 1.1  # (it is a field of standard normals: 3456 of them)
    two = field(2, OV, 5, 0, (0.0, 0.0, 1.0))
    assert torch.equal(two[0], z8[0])
    assert torch.equal(two[1], field(1, OV, 5, 1, (0.0, 0.0, 1.0))[0])  # tile0 counts scenes
    assert not torch.equal(two[1], two[0])
    x8 = field(1, OV, 5, 0, (0.0, 1.0, 0.0))  # x_T alike
    assert torch.equal(x8, field(1, 12, 5, 0, (0.0, 1.0, 0.0)))
    assert not torch.equal(x8, z8)  # x_T is draw 0, the first step's z draw 1


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def run_refusals(dev):
    import pytest
    from ddif.runtime import DdifError

    d = _diffusion(dev)
    cond, xT, noise = _scene_fields(1, 71, dev)
    plan = _plan(d, cond, None)
    base = _ddpm(d, plan, xT, noise, dev, steps=1)
    for bad, what in (((1, HS, WS, 4), "batch"), ((2, HS, WS, OV), "batch"), ((1, HS, WS, TILE), "overlap"), ((1, HS, WS, -1), "overlap"),
                      ((8, 8, WS, 0), "smaller"), ((0, HS, WS, OV), "n_scenes")):
        with pytest.raises(DdifError, match=what):
            plan.set_tiling(bad)
        assert plan.tiling is None
    plan.set_tiling((1, HS, WS, OV))
    plan.set_threshold("ddpm", 0.8, 1.0)
    with pytest.raises(DdifError, match="thresholding"):
        _ddpm(d, plan, xT, noise, dev, steps=1)
    plan.set_threshold("off")
    dpm = dict(n_evals=2, order=2, t_model=[900.0, 400.0], alpha=[0.3, 0.8], sigma=[0.95, 0.6], ord=[1, 2], cx=[0.8, 0.5], a_phi1=[-0.3, -0.4],
               inv_r0=[0.0, 1.1], inv_r1=[0.0] * 2, r0_frac=[0.0] * 2, inv_r01=[0.0] * 2, a_phi2=[0.0] * 2, a_phi3=[0.0] * 2)
    with pytest.raises(DdifError, match="final"):
        plan.sample_dpmpp(dpm, xT, (0.0, 1.0))
    ops = [dict(kind="eval", t_model=900.0, alpha=0.3, sigma=0.95, src=0, dst=0), dict(kind="update", form="lin1", order=1, src=0, dst=0, m=[0, 0, 0], c=[0.8, -0.3])]
    with pytest.raises(DdifError, match="final"):
        plan.sample_dpm(ops, "dpmsolver++", xT, None)
    plan.set_tiling(None)
    assert torch.equal(_ddpm(d, plan, xT, noise, dev, steps=1), base)  # off again: the untiled run, bit for bit
    assert bool(torch.isfinite(plan.sample_dpmpp(dpm, xT, (0.0, 1.0))).all())  # ... and the solver runs again


# ---- 8. test_fn ------------------------------------------------------------------------------------------------------------------------------------------------------
DIVISION = 1023.0


def scene_data(N, H, W, seed=81):
    t = gc.tiles_for(DS, N, H, W, seed=seed)
    return {k: (t[k] * DIVISION).round().numpy() for k in ("gt", "lms", "pan")}


def test_fn_kwargs(dev):
    return dict(state_dict=gc.weights_for(DS), n_steps=STEPS, sampler="ddpm_sample", device=str(dev), dataset_name=DS, division=DIVISION, seed=3)


def run_test_fn(dev):
    from ddif import runtime as R
    from ddif.diffusion_engine import build_model, test_fn
    from ddif.sharding import blend_tiles_torch, cut_tiles_torch

    data = scene_data(2, HS, WS)
    kw = test_fn_kwargs(dev)
    step = test_fn(data=data, tile=TILE, overlap=OV, fuse="step", **kw)
    final = test_fn(data=data, tile=TILE, overlap=OV, fuse="final", **kw)
    for r in (step, final):
        assert r["sr"].shape == (2, C_, HS, WS) and r["sr"].dtype == np.float32
        assert float(r["sr"].min()) >= 0.0 and float(r["sr"].max()) <= DIVISION
        assert len(r["psnr"]) == 2 and r["metrics"].shape == (2, 4)
    assert not np.array_equal(step["sr"], final["sr"])
    # the direct plan run: both scenes in one tiled plan, the library's scene-keyed noise, tile0 = 0
    _, d = build_model(DS, STEPS, dev, state_dict=kw["state_dict"], image_size=WS)
    cond = R.cond_assemble(torch.from_numpy(data["lms"]).to(dev), torch.from_numpy(data["pan"]).to(dev), DIVISION, 0)
    cond_t = cut_tiles_torch(cond.cpu(), TILE, OV).to(dev)
    plan = d._plan(cond_t, tiling=(2, HS, WS, OV))
    order = list(reversed(range(STEPS)))
    c1, c2 = d.posterior_mean_coef1.cpu(), d.posterior_mean_coef2.cpu()
    cz = (0.5 * d.posterior_log_variance_clipped.cpu()).exp()
    res = plan.sample_ddpm([float(i) for i in order], [float(c1[i]) for i in order], [float(c2[i]) for i in order], [0.0 if i == 0 else float(cz[i]) for i in order],
                           None, None, 3, 0, (0.0, 1.0), dev)
    sr = blend_tiles_torch((res + cond_t[:, :C_]).clip(0, 1).cpu(), HS, WS, OV, 2)
    assert np.array_equal(step["sr"], (sr.numpy() * DIVISION).clip(0, DIVISION))
    # overlap = 0 is today's path
    d32 = scene_data(1, 32, 32, seed=82)
    assert np.array_equal(test_fn(data=d32, tile=TILE, overlap=0, fuse="step", **kw)["sr"], test_fn(data=d32, tile=TILE, **kw)["sr"])
    with pytest_raises(R.DdifError):
        test_fn(data=scene_data(1, 8, WS), tile=TILE, overlap=OV, **kw)  # a scene smaller than a tile
    with pytest_raises(R.DdifError):
        test_fn(data=data, tile=TILE, overlap=OV, fuse="blur", **kw)


def pytest_raises(exc):
    import pytest

    return pytest.raises(exc)
