"""The channel-split form of linattn_fused_kernel (kernels_lafuse.h CS = 2: 64 pixels on four waves = 2 pixel blocks x 2 channel halves, the 16 x 16 level) must give
the BITS of the four-wave 128-pixel form it replaces: the plan picks it by batch size, so a tile's result may not depend on it.

Child processes (DDIF_LA_CSPLIT is read once per process; DDIF_DUMP_PLAN=1 makes every fused site say its form, `[ddif la] ... csplit=N`), each running, per case,
one forward of the batch, one forward of tile 1 alone and a 4-step device-RNG DDPM chain:

  * DDIF_LA_CSPLIT=0 and =1 agree with torch.equal on the forward and on the chain, the default run really contains channel-split sites and the other none;
  * under defaults tile 1 run alone is torch.equal to tile 1 inside the B = 3 batch.

Shapes: one WV3 tile of 64 x 64 at B = 2 and B = 3 (the 16 x 16 level with 128 + 64 = 192 and 64 + 64 = 128 feature channels: both instantiations, an odd batch), GF2
32 x 32 at B = 2 (there the 16 x 16 level is the second, with other channel counts: the fused sites outside the rule must stay what they were).  The channel-split
instantiations exist for the channel counts of the THIRD level only, which a 32 x 32 image does not have at 16 x 16: the emulator leg (-m "not gpu") runs the WV3
forwards at 64 x 64, B = 2 (17 s each there: no chain, no third tile) and the GF2 case as it is."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import torch
import golden_cases as gc
from ddif_testlib import make_diffusion, make_net, use_emulator, use_gpu_library
where, out = sys.argv[1], sys.argv[2]
if where == "gpu":
    use_gpu_library()
    dev = torch.device("cuda:0")
else:
    assert use_emulator().emulated
    dev = torch.device("cpu")
res = {}
for arg in sys.argv[3:]:
    ds, B, H, chain = arg.split(":")
    B, H = int(B), int(H)
    C = gc.DATASETS[ds][0]
    g = torch.Generator().manual_seed(91 + B)
    x = torch.randn(B, C, H, H, generator=g).to(dev)
    t = torch.tensor([900, 12, 431][:B]).to(dev)
    cond = gc.tiles_for(ds, B, H, H, seed=92)["cond"].to(dev)
    net = make_net(ds, dev)
    res[arg + ":y"] = net(x, t, cond).cpu()
    res[arg + ":y1"] = net(x[1:2].contiguous(), t[1:2].contiguous(), cond[1:2].contiguous()).cpu()
    if chain == "chain":
        d = make_diffusion(net, C, 4, H, dev)
        res[arg + ":chain"] = d(cond, mode="ddpm_sample", seed=3, tile0=0, device_rng=True).cpu()
torch.save(res, out)
"""


def _run(where, cases, tmp_path):
    res = {}
    for flag in ("0", "1"):
        e = dict(os.environ)
        e["DDIF_LA_CSPLIT"] = flag
        e["DDIF_DUMP_PLAN"] = "1"
        f = str(tmp_path / ("csplit%s.pt" % flag))
        r = subprocess.run([sys.executable, "-c", CODE % (os.path.join(ROOT, "dif-pan_amd"), ROOT, os.path.join(ROOT, "tests")), where, f] + cases, env=e, cwd=ROOT,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]  # (a child that did not end well: the second one is not started)
        sites = [ln for ln in r.stderr.splitlines() if ln.startswith("[ddif la]")]
        res[flag] = (torch.load(f), sum("csplit=2" in ln for ln in sites), len(sites))
    print("fused linear-attention sites: %d, channel-split under defaults: %d, under DDIF_LA_CSPLIT=0: %d" % (res["1"][2], res["1"][1], res["0"][1]))
    assert res["0"][1] == 0 and res["1"][1] >= 4 and res["1"][2] > res["1"][1], (res["0"][1:], res["1"][1:])
    for k, v in res["1"][0].items():
        assert bool(torch.isfinite(v).all()), k
        assert torch.equal(v, res["0"][0][k]), (k, float((v - res["0"][0][k]).abs().max()))
    for arg in cases:
        if arg.split(":")[1] == "3":  # tile 1 alone = tile 1 of the batch, under defaults
            assert torch.equal(res["1"][0][arg + ":y1"], res["1"][0][arg + ":y"][1:2]), arg


@pytest.mark.gpu
def test_channel_split_form_gives_the_same_bits_on_the_gpu(tmp_path):
    _run("gpu", ["wv3:2:64:chain", "wv3:3:64:chain", "gf2:2:32:chain"], tmp_path)


def test_channel_split_form_gives_the_same_bits_on_the_emulator(tmp_path):
    _run("emu", ["wv3:2:64:forward", "gf2:2:32:chain"], tmp_path)
