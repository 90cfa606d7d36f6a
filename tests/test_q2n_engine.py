"""Q2n in the engine (host-emulated build, CPU tensors): `engine_google(..., q2n=True)` adds "Q2n" to every validation record and `test_fn(..., q2n=True)`
adds `q2n`, one value per scene, in the whole-scene and in the tiled branch; with the default both return exactly the keys they returned before.  The
configuration is the smallest one tests/test_engine.py uses (GF2, 16 x 16, 50 diffusion steps, DDIM-25).  On a tree without the feature the keyword
does not exist.

What is under test is the engine's handling of the metric, so the two network-heavy calls are replaced by cheap deterministic stand-ins: a 25-step
sampling run or a training step of the emulated network takes a minute here and has its own tests (tests/test_train_graph.py, tests/test_engine.py).
Cond assembly, the cut, the metric kernels and the records are the real ones."""
import random

import numpy as np
import pytest
import torch

import golden_cases as gc
from ddif import diffusion_engine as E
from ddif import runtime
from ddif_testlib import use_emulator

DS, H, DIV = "gf2", 16, 1023.0


@pytest.fixture(scope="module", autouse=True)
def _lib():
    lib = use_emulator()
    assert lib.emulated
    return lib


@pytest.fixture(autouse=True)
def _cheap_network_calls(monkeypatch):
    from ddif.diffusion.diffusion_ddpm_pan import GaussianDiffusion

    def sample(self, x_in, *args, **kw):  # residual = a small pull of lms towards pan: sr stays close to, and different from, gt
        C = self.channels
        return 0.03 * (x_in[:, C:C + 1] - x_in[:, :C])

    def train_step(self, x_start, cond, grads, noise=None):
        for g in grads:
            g.zero_()
        return torch.zeros((), device=x_start.device), x_start

    monkeypatch.setattr(GaussianDiffusion, "ddim_sample_loop", sample)
    monkeypatch.setattr(GaussianDiffusion, "train_step_into", train_step)


def _raw(n, seed):
    t = gc.tiles_for(DS, n, H, H, seed=seed)
    return dict(lms=(t["lms"] * DIV).round().numpy(), pan=(t["pan"] * DIV).round().numpy(), gt=(t["gt"] * DIV).round().numpy())


def _q2n_of(out, data):
    """what the flag must report: runtime.q2n of (gt, sr) / division without the last row and column, scale = division, 32 / 32"""
    gt = torch.from_numpy(data["gt"] / np.float32(DIV))[:, :, :-1, :-1].contiguous()
    sr = torch.from_numpy((out["sr"] / DIV).astype(np.float32))[:, :, :-1, :-1].contiguous()
    return runtime.q2n(gt, sr, scale=DIV, block=32, shift=32).numpy()


@pytest.mark.parametrize("tile", [None, 8], ids=["whole", "tiled"])
def test_test_fn_reports_q2n_per_scene(tile):
    N = 2
    data = _raw(N, 8)
    kw = dict(batch_size=4, n_steps=50, device="cpu", dataset_name=DS, division=DIV, data=data, state_dict=gc.weights_for(DS), seed=5, tile=tile)
    out = E.test_fn(None, None, q2n=True, **kw)
    assert set(out) == {"sr", "psnr", "metrics", "q2n"}
    q = out["q2n"]
    print(f"test_fn(tile={tile}) q2n = {q}")
    assert q.shape == (N,) and q.dtype == np.float64 and np.isfinite(q).all() and (q > 0).all() and (q < 1 + 1e-12).all()
    # sr comes back in raw units after a clip: the recomputation sees the same counts up to the fp32 round trip of * division / division
    assert np.abs(q - _q2n_of(out, data)).max() <= 1e-6
    if tile is None:  # the default returns today's keys and the same images
        base = E.test_fn(None, None, **kw)
        assert set(base) == {"sr", "psnr", "metrics"} and np.array_equal(base["sr"], out["sr"])
        no_gt = E.test_fn(None, None, q2n=True, **{**kw, "data": {k: v for k, v in data.items() if k != "gt"}})
        assert set(no_gt) == {"sr", "psnr", "metrics"}  # nothing to compare against: no key


def test_engine_google_records_q2n():
    train, valid = _raw(2, 1), _raw(2, 2)

    def run(**extra):
        torch.manual_seed(5)
        random.seed(5)
        return E.engine_google(train, valid, dataset_name=DS, image_n_channel=4, image_size=H, n_steps=50, max_iterations=1, device="cpu", batch_size=2,
                               lr_d=1e-3, valid_every=1, log=lambda *_: None, **extra)

    out = run(q2n=True)
    (it, rec), = out["validation"]
    print(f"engine_google validation record: {rec}")
    assert it == 1 and set(rec) == {"SAM", "ERGAS", "PSNR", "CC", "SSIM", "Q2n"}
    assert 0 < rec["Q2n"] < 1 + 1e-12
    base = run()
    (_, rec0), = base["validation"]
    assert set(rec0) == {"SAM", "ERGAS", "PSNR", "CC", "SSIM"} and set(base) == set(out)
    assert all(rec0[k] == rec[k] for k in rec0)  # the flag changes nothing else
