"""bench.py --dump-outputs without a GPU: what it writes for a comparison of two builds (float32 .npy files, 64 MB in all, small arrays whole,
the same sample of a large one on every run) and that a plain command line runs neither the extras of --full nor a dump."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    saved = dict(os.environ)  # bench.py sets HIP / HSA defaults for its own process at import: keep them out of this one
    try:
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        import bench

        return bench
    finally:
        os.environ.clear()
        os.environ.update(saved)


def test_plain_command_line_has_no_full_extras_and_no_dump():
    a = _bench().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = _bench().parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_float32_bounded_and_reproducible(tmp_path):
    bench = _bench()
    arrays = {"loss": torch.tensor([0.25], dtype=torch.float64), "sr": torch.randn(2, 3, 4, 4),
              "ramp": torch.arange(16_000_000, dtype=torch.float32), "noise": torch.randn(2_000_000, generator=torch.Generator().manual_seed(1))}
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), arrays)
    bench.dump_outputs(str(b), arrays)
    files = sorted(os.listdir(a))
    assert files == ["loss.npy", "noise.npy", "ramp.npy", "sr.npy"]
    assert sum(os.path.getsize(a / f) for f in files) <= 64 * 1000 * 1000
    for f in files:
        x = np.load(a / f)
        assert x.dtype == np.float32 and np.array_equal(x, np.load(b / f)), f
    assert np.load(a / "loss.npy").tolist() == [0.25]
    assert np.array_equal(np.load(a / "sr.npy"), arrays["sr"].numpy())
    ramp = np.load(a / "ramp.npy")  # cut to a sorted sample of its elements: strictly increasing, every value one of the ramp's
    assert 0 < ramp.size < 16_000_000 and (np.diff(ramp) > 0).all() and (ramp == np.round(ramp)).all() and ramp.max() < 16_000_000
