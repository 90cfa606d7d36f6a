"""The x_conv + FiLM fold on 64-cout producer items (kernels_conv.h EPI_XF2 with NB = 2, csrc/ddif_xf.cpp "conv3x3_gn_silu_res_xfilm64"): ResnetBlock.block2 of the
32 x 32 level writes the NEXT block's y = FiLM(x_conv(.)) from its accumulator registers, 64 -> 64 channels as a K = 64 register GEMM, and its GroupNorm partials.

The fold is no bit-for-bit twin of the 1x1 launch it replaces (exact-fp32 MFMA in another K order against the split-operand conv), so it is held to the fp64 oracle,
stage by stage as tests/test_stage_parity.py does it: for each of the two blocks whose y the fold writes (encoder blocks of the second level behind another encoder
block), the block -- CondInjection + ResnetBlock, oracle/ddif_oracle.py -- runs in fp64 on the LIBRARY's tapped block input and is compared with the library's tapped
block output (y reaches it directly: the block output is ResnetBlock's h + y).  Bound: that file's own, err <= MARGIN x e_ref with its MARGIN = 16 and e_ref = the fp32
oracle's distance from the fp64 one on the same input.  Every row (e_ref, error, ratio) is printed.

Child processes (switches are read once per process):
  fold     DDIF_NB2=1 (64-cout items whatever the item count: two tiles do not fill a GPU): both sites must report the fold, the stage bound must hold with and
           without a capped grid (several items per workgroup), and the forward golden of the real reference at 64 x 64 must keep its 2e-5;
  nofold   DDIF_NB2=1 DDIF_XF=0: the same stages on the 1x1 launches (the rows to compare with), no fold reported.
The fold is taken under DDIF_NB2=1 only.  Its y differs in the last bits from the 1x1 launch's, so a site has to fold at every batch size or at none (a tile of a batch
is bit-equal to the tile run alone, tests/test_gpu_batch64.py): the default rule, which goes by the item count of a launch, cannot select it, and folding at every batch
size would change the 132-launch program of small batches that other tests pin.
Launch counts, from plans built only (nothing runs; 64 tiles on the GPU, two on the emulated device): the denoising step has 130 launches under DDIF_NB2=1, 132 by default
and under DDIF_NB2=0 (the launch program before this change).  DDIF_XF=0 switches EVERY fold off, the four of the 64 x 64 level and the Downsample included: 136
launches, as before this change (tests/golden/plan_signature_emu.json)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = "fwd_wv3_64"


def _child(where, out_path):
    for p in (os.path.join(ROOT, "dif-pan_amd"), os.path.join(ROOT, "tests"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    import numpy as np
    import torch

    import ddif_testops as T
    import golden_cases as gc
    import test_stage_parity as SP
    from ddif import runtime
    from ddif_testlib import make_net, use_emulator, use_gpu_library
    from oracle import ddif_oracle as O

    if where.startswith("gpu"):
        use_gpu_library()
        dev = torch.device("cuda:0")
    else:
        assert use_emulator().emulated
        dev = torch.device("cpu")
    res = {"rows": [], "launches": {}}
    ds = "wv3"
    cfg = gc.cfg_for(ds)
    if where.endswith("count"):  # plans only
        for B in (64 if where.startswith("gpu") else 2,):
            res["launches"][str(B)] = make_net(ds, dev).plan_for(B, 64, 64, dev).num_launches()["step"]
        json.dump(res, open(out_path, "w"))
        return
    downs = O.layer_plan(cfg)["downs"]
    # encoder blocks of 64 -> 64 channels behind an encoder block without attention: their y is what the fold writes
    # ... at the second level (one Downsample above: 32 x 32 of a 64 x 64 tile; the lower levels run on the low-resolution kernel)
    sites = [i for i in range(1, len(downs)) if downs[i]["kind"] == "enc" and downs[i - 1]["kind"] == "enc" and not downs[i - 1]["attn"] and
             downs[i]["cin"] == 64 and downs[i]["cout"] == 64 and sum(L["kind"] == "down" for L in downs[:i]) == 1]
    assert len(sites) == 2, sites
    sd32, sd64 = SP.weights(ds, "fixture"), SP.weights(ds, "fixture", torch.float64)
    C, P = cfg["lms_channel"], cfg["pan_channel"]
    g = cfg["norm_groups"]

    def block(sd, i, x, t, cond):
        p = "downs.%d" % i
        temb = O.time_embedding(sd, t.to(x.dtype), cfg["inner_channel"])
        cL = O._resize(cond[:, : C + P].to(x.dtype), x.shape[-2:])
        return O.resnet_block(sd, p + ".res_block", O.cond_injection(sd, p + ".cond_inj", x, cL, g), temb, g)

    for B, cap in ((2, 0), (3, 3)) if where.startswith("gpu") else ((2, 3),):
        gen = torch.Generator().manual_seed(171 + B)
        x = torch.randn(B, gc.DATASETS[ds][0], 64, 64, generator=gen)
        sc = torch.randn(B, gc.DATASETS[ds][0], 64, 64, generator=gen)
        t = torch.tensor([5, 700, 321][:B], dtype=torch.long)
        cond = gc.tiles_for(ds, B, 64, 64, seed=172)["cond"]
        net = make_net(ds, dev)
        try:
            runtime.set_debug_grid_cap(cap)
            plan = net.plan_for(B, 64, 64, dev)
        finally:
            runtime.set_debug_grid_cap(0)
        plan.set_cond(cond.to(dev), force=True)
        need = sorted({"downs.%d" % j for i in sites for j in (i - 1, i)})
        y, got = T.plan_forward_taps(plan, x.to(dev), t, sc.to(dev), need)
        assert bool(torch.isfinite(y).all())
        got = {k: v.cpu() for k, v in got.items()}
        for i in sites:
            xin, out = got["downs.%d" % (i - 1)], got["downs.%d" % i]
            with torch.no_grad():
                r64 = block(sd64, i, xin.double(), t, cond)
                r32 = block(sd32, i, xin, t, cond)
            e_ref, err = SP.rel(r32, r64), SP.rel(out, r64)
            row = "%-10s B=%d cap=%d downs.%d  e_ref %.3e  err %.3e  ratio %6.2f" % (where, B, cap, i, e_ref, err, err / e_ref)
            print(row)
            res["rows"].append(row)
    case = [c for c in gc.FORWARD_CASES if c[0] == GOLDEN][0]
    gold = np.load(os.path.join(gc.GOLDEN_DIR, GOLDEN + ".npz"))
    x, t, cond, sc = gc.forward_inputs(case)
    y = make_net(case[1], dev)(x.to(dev), t.to(dev), cond.to(dev), sc.to(dev)).cpu()
    res["golden"] = float((y - torch.from_numpy(gold["y"])).abs().max())
    print("golden %s max|y - reference| %.3e  (tolerance 2e-5)" % (GOLDEN, res["golden"]))
    json.dump(res, open(out_path, "w"))


_lost = []


def _run(where, env, tmp_path, tag):
    if _lost:  # whatever took a child down is not handed the device again
        pytest.fail("not started: the child %s did not end well" % _lost[0])
    e = dict(os.environ)
    for k in ("DDIF_NB2", "DDIF_XF", "DDIF_TILE16"):
        e.pop(k, None)
    e.update(env)
    e["DDIF_DUMP_PLAN"] = "1"
    out = str(tmp_path / (tag + ".json"))
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", where, out], env=e, cwd=ROOT, capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired as ex:
        _lost.append(tag)
        pytest.fail("time limit: %s" % ((ex.stdout or b"")[-3000:],))
    if r.returncode != 0:
        _lost.append(tag)
    assert r.returncode == 0, (r.stdout + r.stderr)[-6000:]
    res = json.load(open(out))
    n = sum(1 for ln in r.stderr.splitlines() if ln.startswith("[ddif plan]") and "conv3x3_gn_silu_res_xfilm64" in ln)
    assert n % 2 == 0, n  # (a plan is built in two passes, the dry one for buffer lifetimes: every launch reports twice)
    res["folds"] = n // 2
    return res


def _stages(where, tmp_path):
    import test_stage_parity as SP

    fold = _run(where, {"DDIF_NB2": "1"}, tmp_path, "fold")
    legs = [("fold", fold)]
    if where == "gpu":  # (the emulator leg does without the rows to compare with: 30 s per child there)
        legs.append(("nofold", _run(where, {"DDIF_NB2": "1", "DDIF_XF": "0"}, tmp_path, "nofold")))
    for tag, res in legs:
        for row in res["rows"]:
            print(tag, row)
        print(tag, "forward golden %s: %.3e (tolerance 2e-5); fold launches reported: %d" % (GOLDEN, res["golden"], res["folds"]))
    n_plans = len(fold["rows"]) // 2 + 1  # the tapped plans and the golden's
    assert fold["folds"] == 2 * n_plans and all(res["folds"] == 0 for tag, res in legs[1:]), ([res["folds"] for tag, res in legs], n_plans)
    for tag, res in legs:
        assert len(res["rows"]) >= 2
        for row in res["rows"]:
            assert float(row.split()[-1]) <= SP.MARGIN, row
        assert res["golden"] <= 2e-5, res["golden"]


def _counts(where, tmp_path):
    B = "64" if where == "gpu" else "2"
    forced = _run(where + "_count", {"DDIF_NB2": "1"}, tmp_path, "count_forced")
    default = _run(where + "_count", {}, tmp_path, "count_default")
    nonb2 = _run(where + "_count", {"DDIF_NB2": "0"}, tmp_path, "count_nonb2")
    noxf = _run(where + "_count", {"DDIF_XF": "0"}, tmp_path, "count_noxf")
    print("step launches at B = %s: DDIF_NB2=1 %d (64-channel folds %d), default %d, DDIF_NB2=0 %d, DDIF_XF=0 %d" % (
        B, forced["launches"][B], forced["folds"], default["launches"][B], nonb2["launches"][B], noxf["launches"][B]))
    assert forced["launches"][B] == 130 and default["launches"][B] == 132 and nonb2["launches"][B] == 132 and noxf["launches"][B] == 136, (
        forced["launches"], default["launches"], nonb2["launches"], noxf["launches"])
    assert forced["folds"] == 2 and default["folds"] == 0 and nonb2["folds"] == 0 and noxf["folds"] == 0


@pytest.mark.gpu
def test_folded_blocks_match_the_fp64_oracle_on_the_gpu(tmp_path):
    _stages("gpu", tmp_path)


@pytest.mark.gpu
def test_step_launch_counts_on_the_gpu(tmp_path):
    _counts("gpu", tmp_path)


def test_folded_blocks_match_the_fp64_oracle_on_the_emulator(tmp_path):
    _stages("emu", tmp_path)


def test_step_launch_counts_on_the_emulator(tmp_path):
    _counts("emu", tmp_path)


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    _child(*sys.argv[2:4])
