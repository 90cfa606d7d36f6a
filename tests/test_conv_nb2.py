"""64-cout work items on the f16x2 3x3 conv path (csrc/conv_variants.h cfg 67 / 68: NB = 2) must give the BITS of the 32-cout items they replace (cfg 27 / 28),
conv outputs AND GroupNorm partials: the plan picks them by the item count of a launch, so a tile's result may not depend on them.

Child processes (DDIF_NB2, DDIF_XF, DDIF_TILE16 are read once per process; DDIF_DUMP_PLAN=1 makes every conv launch say its tiling, `[ddif plan] ... cfg=N`).
Both legs run with DDIF_XF=0 (no x_conv fold: the fold of the 32 x 32 level exists only on 64-cout items and is no bit-for-bit twin of the 1x1 launch; it has
tests/test_xf64.py) and differ in DDIF_NB2 = 1 (64-cout items wherever an instantiation exists, whatever the item count) / 0 (the launch program without them):

  * every stage tap of one forward evaluation is torch.equal between the legs, for every case;
  * a device-RNG DDPM chain is torch.equal between the legs;
  * on the DDIF_NB2=1 leg tile 1 run alone is torch.equal to tile 1 inside the B = 3 batch;
  * the on leg really ran 64-cout items for every prologue / epilogue combination of the 64-channel sites (ffn.0: SiLU epilogue; ffn.3(ffn.2): residual;
    res.conv1: GroupNorm + SiLU prologue; res.conv2: that prologue + residual), the off leg none.

Cases, (B, H = W, grid cap): the WV3 network at 64 x 64, the smallest tile that puts 64-channel convs on this kernel (its 32 x 32 level), at B = 2 and B = 3; the
same with the persistent grids capped to 3 workgroups (ddif_debug_set_grid_cap), so that a workgroup pipelines several 64-cout items across pixel tiles and samples;
one 80 x 80 tile, whose 40 x 40 level has partial 16 x 16 tiles with a MISSING bottom half tile (40 = 2 x 16 + 8: guarded stores, the tiles_y8 edge of the half-tile
partials) and whose 80 x 80 level has full ones.  DDIF_TILE16=1 keeps the eight-wave 16 x 16 tilings at these batch sizes (cfg 67 where the combination has one,
the four-wave 68 elsewhere); one more pair of legs at DDIF_TILE16=0 runs every site on 68.

The emulator legs (-m "not gpu"; 9 s per 64 x 64 tile and forward there) keep every kind of check on fewer cases: a capped B = 2 batch with tile 1 alone, the
80 x 80 tile, and a 2-step chain of one tile, under DDIF_NB2=1 as on the GPU (the default rule takes no launch of fewer than 64 items)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, H, grid cap, chain steps, also tile 1 alone)
GPU_CASES = [(2, 64, 0, 4, False), (3, 64, 0, 4, True), (2, 64, 3, 0, False), (3, 64, 3, 0, False), (1, 80, 0, 0, False)]
GPU_CASES_SMALL_TILES = [(2, 64, 0, 0, False), (1, 80, 3, 0, False)]
EMU_CASES = [(2, 64, 3, 0, True), (1, 80, 0, 0, False), (1, 64, 0, 2, False)]
# (pro, epi) of kernels_conv.h for the four 64-channel site classes
COMBOS = {"ffn.0": ("pro=0", "epi=8"), "ffn.3(ffn.2)": ("pro=0", "epi=4"), "res.conv1": ("pro=2", "epi=0"), "res.conv2": ("pro=2", "epi=4")}

CODE = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import torch
import golden_cases as gc
import ddif_testops as T
from ddif import runtime
from ddif_testlib import make_diffusion, make_net, use_emulator, use_gpu_library
where, out = sys.argv[1], sys.argv[2]
if where == "gpu":
    use_gpu_library()
    dev = torch.device("cuda:0")
else:
    assert use_emulator().emulated
    dev = torch.device("cpu")
ds = "wv3"
C = gc.DATASETS[ds][0]
res = {}
for arg in sys.argv[3:]:
    B, H, cap, steps, single = (int(v) for v in arg.split(":"))
    g = torch.Generator().manual_seed(131 + 7 * B + H)
    x = torch.randn(B, C, H, H, generator=g).to(dev)
    sc = torch.randn(B, C, H, H, generator=g).to(dev)
    t = torch.tensor([900, 12, 431][:B])
    cond = gc.tiles_for(ds, B, H, H, seed=132)["cond"].to(dev)

    def tapped(xx, tt, cc, ss, cap_):
        net = make_net(ds, dev)
        try:
            runtime.set_debug_grid_cap(cap_)
            plan = net.plan_for(xx.shape[0], H, H, dev)
        finally:
            runtime.set_debug_grid_cap(0)
        plan.set_cond(cc, force=True)
        y, taps = T.plan_forward_taps(plan, xx, tt, ss, None)
        return y.cpu(), {k: v.cpu() for k, v in taps.items()}

    y, taps = tapped(x, t, cond, sc, cap)
    res[arg + ":y"] = y
    for k, v in taps.items():
        res[arg + ":tap:" + k] = v
    if single:
        y1, taps1 = tapped(x[1:2].contiguous(), t[1:2], cond[1:2].contiguous(), sc[1:2].contiguous(), 0)
        res[arg + ":y1"] = y1
        for k, v in taps1.items():
            res[arg + ":tap1:" + k] = v
    if steps:
        net = make_net(ds, dev)
        d = make_diffusion(net, C, steps, H, dev)
        res[arg + ":chain"] = d(cond, mode="ddpm_sample", seed=3, tile0=0, device_rng=True).cpu()
torch.save(res, out)
"""

_lost = []


def _leg(where, nb2, tile16, cases, tmp_path):
    if _lost:  # whatever took a child down is not handed the device again
        pytest.fail("not started: the child of leg %s did not end well" % (_lost[0],))
    e = dict(os.environ)
    e.update({"DDIF_NB2": nb2, "DDIF_XF": "0", "DDIF_DUMP_PLAN": "1"})
    e.pop("DDIF_TILE16", None)
    if tile16 is not None:
        e["DDIF_TILE16"] = tile16
    f = str(tmp_path / ("nb2_%s_%s.pt" % (nb2, tile16)))
    args = ["%d:%d:%d:%d:%d" % (c[:4] + (c[4] and nb2 == "1",)) for c in cases]  # (tile 1 alone: on the 64-cout items only)
    try:
        r = subprocess.run([sys.executable, "-c", CODE % (os.path.join(ROOT, "dif-pan_amd"), ROOT, os.path.join(ROOT, "tests")), where, f] + args, env=e, cwd=ROOT,
                           capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired as ex:
        _lost.append((nb2, tile16))
        pytest.fail("time limit: %s" % ((ex.stderr or b"")[-3000:],))
    if r.returncode != 0:
        _lost.append((nb2, tile16))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    lines = [ln.split() for ln in r.stderr.splitlines() if ln.startswith("[ddif plan]")]
    return torch.load(f), lines, args


def _nb2_lines(lines):
    return [ln for ln in lines if "cfg=67" in ln or "cfg=68" in ln]


def _compare(where, tile16, cases, tmp_path, want_cfgs):
    on, on_lines, args = _leg(where, "1", tile16, cases, tmp_path)
    off, off_lines, _ = _leg(where, "0", tile16, cases, tmp_path)
    got = _nb2_lines(on_lines)
    per = {name: sum(1 for ln in got if pe[0] in ln and pe[1] in ln and "ks=3" in ln) for name, pe in COMBOS.items()}
    cfgs = sorted({f for ln in got for f in ln if f in ("cfg=67", "cfg=68")})
    print("%s, DDIF_TILE16=%s: %d conv launches of the on leg on 64-cout items %s, by site class %s; off leg %d" % (where, tile16, len(got), cfgs, per, len(_nb2_lines(off_lines))))
    assert not _nb2_lines(off_lines)
    assert all(n >= 1 for n in per.values()), per
    assert cfgs == want_cfgs, cfgs
    on = {":".join(k.split(":", 5)[:4] + ["0"] + k.split(":", 5)[5:]): v for k, v in on.items()}  # (the case ids of the off leg: its flag "tile 1 alone" is 0)
    args = [a[:-1] + "0" for a in args]
    singles_asked = sum(c[4] for c in cases)
    assert sorted(k for k in on if ":y1" not in k and ":tap1:" not in k) == sorted(off)
    n_taps = 0
    for k in sorted(off):
        assert bool(torch.isfinite(on[k]).all()), k
        assert torch.equal(on[k], off[k]), (k, float((on[k] - off[k]).abs().max()))
        n_taps += ":tap:" in k
    assert n_taps >= 40 * len(args), n_taps  # every layer output and attention stage tensor of every case
    singles = 0
    for arg in args:
        if arg + ":y1" in on:  # tile 1 alone = tile 1 of the batch, on the 64-cout items
            assert torch.equal(on[arg + ":y1"], on[arg + ":y"][1:2]), arg
            for k in on:
                if k.startswith(arg + ":tap1:"):
                    kb = arg + ":tap:" + k[len(arg) + 6:]
                    if on[kb].shape[0] == int(arg.split(":")[0]):  # (cond-only taps have the batch too; a tap without a batch axis of its own would not)
                        assert torch.equal(on[k], on[kb][1:2]), k
                        singles += 1
    assert singles_asked == sum(1 for k in on if k.endswith(":y1"))
    return singles


@pytest.mark.gpu
def test_64_cout_items_give_the_bits_of_32_cout_items_on_the_gpu(tmp_path):
    assert _compare("gpu", "1", GPU_CASES, tmp_path, ["cfg=67", "cfg=68"]) >= 40


@pytest.mark.gpu
def test_64_cout_items_on_the_four_wave_tiling_everywhere_on_the_gpu(tmp_path):
    _compare("gpu", "0", GPU_CASES_SMALL_TILES, tmp_path, ["cfg=68"])


def test_64_cout_items_give_the_bits_of_32_cout_items_on_the_emulator(tmp_path):
    assert _compare("emu", None, EMU_CASES, tmp_path, ["cfg=67", "cfg=68"]) >= 40
