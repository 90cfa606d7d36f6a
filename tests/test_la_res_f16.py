"""attn_res(xn) of the fused linear-attention kernels on f16x2 (kernels_lafuse.h / kernels_lafuse8.h RF16) against what it replaces.

Three legs, each in a fresh child process (DDIF_LA_RES_F16 is read once per process; DDIF_DUMP_PLAN=1 makes the plan say which math every site runs, `[ddif la]` lines):

  f16x2     defaults: every fused site must report res=f16x2
  bf16x3    DDIF_LA_RES_F16=0: every fused site must report res=bf16x3 (the path of the rounds before)
  fallback  defaults, on a net whose every attn_res.weight is scaled to max|w| = 80, past the half-pack range (|w| < 64): no half pack exists, every fused site
            must report res=bf16x3

In every leg every linear-attention stage tap is compared with the fp64 oracle ON THE TAPPED INPUT under the bound of tests/test_stage_parity.py, unchanged
(MARGIN x e_ref = 16 x e_ref per site, which already budgets 22 operand bits: f16x2 and bf16x3 both carry 22), with that file's own run_library_leg; the fallback leg's
oracle runs on the same scaled weights.  The f16x2 and bf16x3 legs also hold the forward goldens of the real reference to their 2e-5.  The child prints every row
(e_ref, error, ratio) and every golden margin; the parent prints them again (-s) so that both legs' margins can be recorded side by side.

Shapes: one WV3 tile of 64 x 64 at B = 2 and B = 3 (linattn_fused at TH = 64, 32, 16 with 64 / 96 / 128 / 192 feature channels, linattn8_fused with 256 and 192, an odd
batch), GF2 32 x 32 at B = 2.  On the emulator (-m "not gpu"): WV3 and GF2 at 32 x 32, B = 2 (TH = 32, 16 and the 8 x 8 kernel).

Measured margins (MI355X, largest err / e_ref over the linear-attention sites of a leg; bound 16): see profiles/r10/README.md."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEGS = ("f16x2", "bf16x3", "fallback")
GPU_CASES = {"wv3_64_b2": ("wv3", 2, 64, 64, 0, False), "wv3_64_b3": ("wv3", 3, 64, 64, 0, False), "gf2_32_b2": ("gf2", 2, 32, 32, 0, False)}
EMU_CASES = {"wv3_32_b2": ("wv3", 2, 32, 32, 0, True), "gf2_32_b2": ("gf2", 2, 32, 32, 0, True)}
GPU_GOLDENS = ("fwd_wv3_64", "fwd_gf2_32", "fwd_wv3_16_b")
EMU_GOLDENS = ("fwd_gf2_32", "fwd_wv3_16_b")
RES_ABSMAX = 80.0  # the fallback leg's max|attn_res.weight|: past DDIF_F16_WMAX = 63.9 (csrc/ddif_dev.h)


# ------------------------------------------------------------------------------------------------ child
def _child(where, leg, out_path):
    for p in (os.path.join(ROOT, "dif-pan_amd"), os.path.join(ROOT, "tests"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch

    import golden_cases as gc
    import test_stage_parity as SP
    from ddif_testlib import make_net, use_emulator, use_gpu_library

    if where == "gpu":
        use_gpu_library()
        dev, cases, goldens = "cuda:0", GPU_CASES, GPU_GOLDENS
    else:
        assert use_emulator().emulated
        dev, cases, goldens = "cpu", EMU_CASES, EMU_GOLDENS
    SP.CASES.update(cases)  # (this process only: run_library_leg looks its case up there)
    kind = "stressed"
    if leg == "fallback":
        # the stressed weights with every attn_res.weight scaled to max|w| = RES_ABSMAX, handed to run_library_leg / stage_refs through the weight cache they read
        kind = "resbig"
        for ds in sorted({v[0] for v in cases.values()}):
            sd = {k: v.clone() for k, v in SP.weights(ds, "stressed").items()}
            n = 0
            for k in sd:
                if k.endswith("cond_inj.attn_res.weight"):
                    sd[k] *= RES_ABSMAX / float(sd[k].abs().max())
                    n += 1
            assert n > 0
            SP._sd_cache[(ds, kind, torch.float32)] = sd
            SP._sd_cache[(ds, kind, torch.float64)] = {k: v.double() for k, v in sd.items()}
    res = {"rows": [], "goldens": {}}
    for case in cases:
        la = set(SP.sites(cases[case][0])[1])
        rows = SP.run_library_leg(case, kind, dev, where)  # asserts err <= MARGIN x e_ref at every attention site
        res["rows"] += [r for r in rows if r.split()[4] in la]
    if leg != "fallback":
        for cid in goldens:
            case = [c for c in gc.FORWARD_CASES if c[0] == cid][0]
            g = np.load(os.path.join(gc.GOLDEN_DIR, cid + ".npz"))
            x, t, cond, sc = gc.forward_inputs(case)
            net = make_net(case[1], dev)
            y = net(x.to(dev), t.to(dev), cond.to(dev), None if sc is None else sc.to(dev)).cpu()
            err = float((y - torch.from_numpy(g["y"])).abs().max())
            print("golden %-5s %-8s %-14s max|y - reference| %.3e  (tolerance 2e-5)" % (where, leg, cid, err))
            res["goldens"][cid] = err
            assert err <= 2e-5, (cid, err)
    with open(out_path, "w") as f:
        json.dump(res, f)


# ------------------------------------------------------------------------------------------------ parent
_lost = []


def _run_leg(where, leg, tmp_path):
    if _lost:  # whatever took a child down is not handed the GPU again
        pytest.fail("not started: the child of leg %s did not end well" % _lost[0])
    e = dict(os.environ)
    e.pop("DDIF_LA_RES_F16", None)
    if leg == "bf16x3":
        e["DDIF_LA_RES_F16"] = "0"
    e["DDIF_DUMP_PLAN"] = "1"
    out = str(tmp_path / ("%s_%s.json" % (where, leg)))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", where, leg, out], env=e, cwd=ROOT, capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired as ex:
        _lost.append(leg)
        pytest.fail("time limit: %s" % ((ex.stdout or b"")[-3000:],))
    if r.returncode != 0:
        _lost.append(leg)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    res = json.load(open(out))
    sites = [ln.split() for ln in r.stderr.splitlines() if ln.startswith("[ddif la]")]
    said = sorted({f for ln in sites for f in ln if f.startswith("res=")})
    print("leg %s: %d fused linear-attention sites report %s" % (leg, len(sites), said))
    for row in res["rows"]:
        print(row)
    for cid, err in res["goldens"].items():
        print("golden %-14s max|y - reference| %.3e" % (cid, err))
    ratios = [float(row.split()[-1]) for row in res["rows"]]
    print("leg %s: largest err / e_ref over %d linear-attention stage taps: %.2f  (bound %.0f)" % (leg, len(ratios), max(ratios), 16.0))
    assert len(sites) >= 4 and len(ratios) >= 4
    assert said == ["res=f16x2" if leg == "f16x2" else "res=bf16x3"], said
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("leg", LEGS)
def test_linear_attention_stages_on_the_gpu(leg, tmp_path):
    _run_leg("gpu", leg, tmp_path)


@pytest.mark.parametrize("leg", LEGS)
def test_linear_attention_stages_on_the_emulator(leg, tmp_path):
    _run_leg("emu", leg, tmp_path)


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    _child(*sys.argv[2:5])
