"""Stage-level parity of the CONV stages of an inference plan: every stage against the fp64 oracle ON THE LIBRARY'S OWN TAPPED INPUT.

tests/test_stage_parity.py does this for the attention kernels; the general implicit-GEMM conv (csrc/kernels_conv.h) and the split-K conv of the low levels
(csrc/kernels_lr.h) were held only by end-to-end goldens (2e-5 .. 1e-4 on the network output, behind up to 130 launches and ~40 GroupNorms) and by bit-equality
of one conv form against another, which shows that two forms agree and not that either is right.  The plan builder notes every layer output as a tap
(include/ddif_testops.h); this file reads all of them.  One tapped forward per leg, then per stage

  stage                 input (tapped, fp32)                 output compared                        oracle (oracle/ddif_oracle.py)
  stem                  cat[self_cond, x]                    downs.0                                conv3x3
  enc   downs.i         downs.{i-1}, RAW cond[:, :C+P]       downs.i.attn.in | downs.i              cond_injection(_resize(c_enc)) + resnet_block
  down  downs.i         downs.{i-1}                          downs.i                                conv3x3 stride 2
  res   mid.i           previous layer                       mid.0.attn.in / mid.1                  resnet_block
  cond  <ci>            RAW cond[:, -(C+3P):]                <ci>.cond                              _resize
  ffn   <ci>            <ci>.a                               <ci>.out                               ffn.3(ffn.2(silu(ffn.0(a)))) + a
  res   ups.i           <ci>.out                             ups.i.attn.in | ups.i                  resnet_block (res_conv where present)
  up    ups.i           ups.{i-1}                            ups.i                                  nearest x2 + conv3x3
  final                 last ups tap                         the forward's return value             GroupNorm + SiLU + conv3x3

(the encoder stage starts from the raw cond, so the cond-only program -- resize, body.0, GroupNorm, body.3 -- is part of what is checked).  The stage list
(stage_list) also carries the attention stages of test_stage_parity.py and the aliases, in execution order: a tap that is another tap under a second name
(<ci>.cur = the previous layer, <ci>.skip = the encoder layer it pops, <layer> = <layer>.attn.out) must be torch.equal to it, and EVERY tap of the plan must be
the output of a stage of this file, of an attention stage of test_stage_parity.py, or such an alias -- an orphan fails the leg by name.

Bound: test_stage_parity.py's, nothing fixed in advance.  e_ref = rel(fp32 oracle stage, fp64 oracle stage) on the same tapped input; the library must keep
rel(library, fp64) <= MARGIN x e_ref with that file's MARGIN (16), for every stage alike.  Every row (where, case, weights, switches, stage, shape, e_ref, err,
ratio) is printed; DDIF_STAGE_PARITY_TABLE=<file> appends them there (profiles/stage_parity_conv.txt is such a file from an MI355X run).

Weights: "fixture" and "stressed" of test_stage_parity.py, "trained" = test_range_guard.trained_like(ds, 11) (GroupNorm gains 0.5 .. 8, every third Block
conv x 20: the convs see trained-like magnitudes), and "strong" = those with biases and time biases that keep pace (strengthened(): what the sensitivity proof
needs).

CPU-only checks: the stage functions of this file, run as a chain with the oracle's attention stages, ARE O.unet_forward to the last bit
(test_stage_chain_is_the_oracle_forward); and every fault an end-to-end test can miss (MUTATIONS: transposed taps, a seam column read as padding, a dropped bias,
a neighbour's time bias, statistics from half the rows, ...) moves its stage's fp64 output by at least SENSITIVITY x the bound of that stage, at every site
(test_mutations_move_every_conv_stage_far_beyond_its_bound): a kernel with one of these faults cannot pass a leg.

The per-process conv switches (DDIF_X3, DDIF_F16, DDIF_LR, DDIF_S2_F16, DDIF_XF, DDIF_NB2) run one leg of this file in a fresh child process each (bottom of the
file).  The benchmark batch (B = 64: 16 x 16 tilings, 64-cout items and eight-wave forms that only a full GPU selects) is tied to the small-batch legs by
bit-equality of EVERY tap of samples 0, 37, 63 with a B = 1 plan on that tile (test_batch64_taps_equal_single_tile_taps)."""
import os
import subprocess
import sys
import time

import pytest
import torch
import torch.nn.functional as F

import golden_cases as gc
import test_stage_parity as SP
from ddif_testlib import use_emulator, use_gpu_library
from oracle import ddif_oracle as O
from test_range_guard import trained_like
from test_stage_parity import MARGIN, SENSITIVITY, _make_net, rel, sites

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# id -> (data set, B, H, W, grid cap, runs on the emulator)
CASES = {
    # the 1 x 1 bottom level, 2 x 2 and 4 x 4 above it
    "wv3_8_b2": ("wv3", 2, 8, 8, 0, True),
    # the low-resolution kernel at 16^2 / 8^2 / 4^2, the general kernel at 32^2
    "gf2_32_b2": ("gf2", 2, 32, 32, 0, True),
    # the same with grids capped to 3 workgroups: several items and samples per workgroup
    "gf2_32_b3_cap3": ("gf2", 3, 32, 32, 3, True),
    # partial tiles, H != W, a 3 x 5 bottom level
    "wv3_24x40_b1": ("wv3", 1, 24, 40, 0, True),
    # 31 / 34-channel inputs (channel padding), the scalar output path of the final conv (31 channels)
    "cave_32_b1": ("cave", 1, 32, 32, 0, True),
    # the 64^2 tilings, the x_conv + FiLM folds (EPI_XF)   (one emulator leg: a 64 x 64 forward costs the emulator ~15 s)
    "wv3_64_b2": ("wv3", 2, 64, 64, 0, True),
    # the same kernels on a capped grid   (GPU only)
    "wv3_64_b3_cap3": ("wv3", 3, 64, 64, 3, False),
}
MUTATION_CASES = ("gf2_32_b2", "wv3_24x40_b1", "cave_32_b1")
# (the "strong" legs: the weights the sensitivity proof holds on -- see strengthened() -- are weights a library leg runs on, at the cases of the proof)
GPU_LEGS = ([(c, "fixture") for c in CASES] + [(c, "trained") for c in CASES] + [("wv3_64_b2", "stressed"), ("wv3_8_b2", "stressed")] +
            [(c, "strong") for c in MUTATION_CASES])
EMU_LEGS = [(c, "trained") for c, v in CASES.items() if v[5]] + [("gf2_32_b2", "fixture"), ("wv3_8_b2", "stressed")] + [(c, "strong") for c in MUTATION_CASES]
TRAINED_SEED = 11

_SWITCHES = ("DDIF_X3", "DDIF_F16", "DDIF_LR", "DDIF_S2_F16", "DDIF_XF", "DDIF_NB2")


# ------------------------------------------------------------------------------------------------ weights, inputs
def strengthened(ds):
    """trained_like(ds, 11) with the additive per-channel terms of the ResnetBlocks keeping pace with the conv outputs they are added to.  trained_like scales
    every third Block conv x 20 and leaves its bias and the block's time bias alone, so under "trained" a dropped bias or a neighbour's time bias is worth
    little: measured on the three cases of the sensitivity proof, block1:nobias moved its stage by 1.5 - 48 x the bound at 11 encoder sites, block2:nobias by
    12 - 42 x at 21 ResnetBlock sites, time_bias_of_neighbour by 6 - 11 x at three, gn2_half_rows by 22 - 32 x at two (wv3_24x40_b1 downs.6 / downs.7, where
    block2 carries ~1 % of the block output) -- SENSITIVITY asks 50.  Here: the Block convs trained_like left alone x 4 (every ResnetBlock branch carries
    weight), every Block conv bias x its conv's gain (20 or 4) x 2, every time-bias Linear x the gain of the block1 conv it is added to.  Measured under these
    weights: every mutation at every site >= 66 x the bound (the smallest: conv:nobias of a Downsample, 66 - 78 x; then block2:nobias 77 x, wv3_24x40_b1
    downs.14), and the fp32 oracle still follows the fp64 one to 3e-6 of the network output's largest value (the network has not turned chaotic)."""
    fx = gc.weights_for(ds)
    sd = trained_like(ds, TRAINED_SEED)
    for k in sorted(sd):
        if not k.endswith(".block.3.weight"):
            continue
        gain = 20.0
        if torch.equal(sd[k], fx[k]):
            gain = 4.0
            sd[k] = sd[k] * gain
        b = k[:-len("weight")] + "bias"
        sd[b] = sd[b] * (2.0 * gain)
        if ".block1." in k:
            q = k.split(".block1.")[0] + ".noise_func.noise_func.0."
            sd[q + "weight"] = sd[q + "weight"] * gain
            sd[q + "bias"] = sd[q + "bias"] * gain
    return sd


def weights(ds, kind, dtype=torch.float32):
    """SP.weights, plus the kinds "trained" and "strong".  They are entered into that file's cache, so that SP.weights / SP._make_net know them too."""
    if kind in ("trained", "strong") and (ds, kind, dtype) not in SP._sd_cache:
        sd = trained_like(ds, TRAINED_SEED) if kind == "trained" else strengthened(ds)
        SP._sd_cache[(ds, kind, dtype)] = {k: v.to(dtype) for k, v in sd.items()}
    return SP.weights(ds, kind, dtype)


def inputs(case):
    """SP.inputs (seeded by the case id; t = [5, 700, 321][:B]) for the cases of this file: it reads the shape from its own table."""
    if case in SP.CASES:
        assert SP.CASES[case][:5] == CASES[case][:5]
        return SP.inputs(case)
    SP.CASES[case] = CASES[case]
    try:
        return SP.inputs(case)
    finally:
        del SP.CASES[case]


# ------------------------------------------------------------------------------------------------ the stage list
def stage_list(ds):
    """The network as stages in execution order: dicts of kind, p (state-dict prefix), ins (tap names; "@..." = a network input), out (tap name; "@y" = the
    network output).  Kinds stem / enc / down / res / cond / ffn / up / final are the stages of this file; "sa" and "la" are the attention stages of
    test_stage_parity.py; "alias" is a tap that is its input under another name."""
    plan = O.layer_plan(gc.cfg_for(ds))
    out, feats, prev = [], [], None

    def S(kind, p, ins, o):
        out.append(dict(kind=kind, p=p, ins=tuple(ins), out=o))

    def block_tail(p, L):  # ResnetBlocWithAttn: the block's output is the layer's, or the input of its self-attention
        if L.get("attn"):
            S("sa", p + ".attn", (p + ".attn.in",), p + ".attn.out")
            S("alias", p, (p + ".attn.out",), p)

    for i, L in enumerate(plan["downs"]):
        p = "downs.%d" % i
        if L["kind"] == "stem":
            S("stem", p, ("@sc", "@x"), p)
        elif L["kind"] == "down":
            S("down", p, (prev,), p)
        else:
            S("enc", p, (prev, "@c_enc", "@t"), p + ".attn.in" if L["attn"] else p)
            block_tail(p, L)
        feats.append(p)
        prev = p
    for i, L in enumerate(plan["mid"]):
        p = "mid.%d" % i
        S("res", p, (prev, "@t"), p + ".attn.in" if L["attn"] else p)
        block_tail(p, L)
        prev = p
    for i, L in enumerate(plan["ups"]):
        p = "ups.%d" % i
        if L["kind"] == "up":
            S("up", p, (prev,), p)
        else:
            ci = p + ".cond_inj"
            S("alias", ci, (prev,), ci + ".cur")
            S("alias", ci, (feats.pop(),), ci + ".skip")
            S("cond", ci, ("@c_dec", ci + ".cur"), ci + ".cond")
            S("la", ci, (ci + ".cur", ci + ".skip", ci + ".cond"), ci + ".a")
            S("ffn", ci, (ci + ".a",), ci + ".out")
            S("res", p, (ci + ".out", "@t"), p + ".attn.in" if L["attn"] else p)
            block_tail(p, L)
        prev = p
    assert not feats
    S("final", "final_conv", (prev,), "@y")
    return out


OWN = ("stem", "enc", "down", "res", "cond", "ffn", "up", "final")


def stage_name(st):
    return "%s %s" % (st["kind"], st["p"])


# ------------------------------------------------------------------------------------------------ the stages, with the mutations of the sensitivity check
def _c3(x, w, b, tag, mut, stride=1):
    """3 x 3 conv, padding 1, with the faults of any 3 x 3 conv as mut = "<tag>:<fault>": "transposed" (ky / kx taps swapped), "nobias", "seam" (the input
    column right of the W/2 seam is read as zero padding by the output column left of it, as a tile's right edge would)."""
    fault = mut[len(tag) + 1:] if mut is not None and mut.startswith(tag + ":") else None
    if fault == "transposed":
        w = w.transpose(2, 3)
    if fault == "nobias":
        b = None
    y = F.conv2d(x, w, b, stride=stride, padding=1)
    if fault == "seam":
        s = x.shape[-1] // 2
        if (s - 1) % stride:  # (stride 2: output column j reads 2j - 1 .. 2j + 1, so the column a left neighbour reads last is odd)
            s += 1
        j = (s - 1) // stride
        x0 = x.clone()
        x0[..., s] = 0
        y = y.clone()
        y[..., j] = F.conv2d(x0, w, b, stride=stride, padding=1)[..., j]
    return y


def _gn_half_rows(x, sd, key):
    """GroupNorm(1 group) with its statistics taken from the upper half of the rows only."""
    h = x[:, :, : x.shape[2] // 2]
    m = h.mean((1, 2, 3), keepdim=True)
    v = h.var((1, 2, 3), unbiased=False, keepdim=True)
    return (x - m) / torch.sqrt(v + 1e-5) * sd[key + ".weight"].view(1, -1, 1, 1) + sd[key + ".bias"].view(1, -1, 1, 1)


def stem_stage(sd, p, sc, x, mut=None):
    xx = torch.cat([x, sc] if mut == "halves_swapped" else [sc, x], dim=1)
    return _c3(xx, sd[p + ".weight"], sd[p + ".bias"], "conv", mut)


def down_stage(sd, p, x, mut=None):
    if mut == "odd_pixels":  # centred on input (2i + 1, 2j + 1) instead of (2i, 2j)
        x = F.pad(x[..., 1:, 1:], (0, 1, 0, 1))
    return _c3(x, sd[p + ".conv.weight"], sd[p + ".conv.bias"], "conv", mut, stride=2)


def up_stage(sd, p, x, mut=None):
    if mut == "source_rounded_up":  # source pixel (y + 1) // 2 instead of y // 2
        H, W = x.shape[-2:]
        iy = ((torch.arange(2 * H) + 1) // 2).clamp(max=H - 1)
        ix = ((torch.arange(2 * W) + 1) // 2).clamp(max=W - 1)
        x = x[..., iy, :][..., ix]
    else:
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    return _c3(x, sd[p + ".conv.weight"], sd[p + ".conv.bias"], "conv", mut)


def res_stage(sd, cfg, p, x, t, mut=None):
    """O.resnet_block (eval) behind O.time_embedding."""
    g = cfg["norm_groups"]
    temb = O.time_embedding(sd, t, cfg["inner_channel"])
    h = _c3(O._swish(O._gn(x, sd, p + ".block1.block.0", g)), sd[p + ".block1.block.3.weight"], sd[p + ".block1.block.3.bias"], "block1", mut)
    tb = F.linear(temb, sd[p + ".noise_func.noise_func.0.weight"], sd[p + ".noise_func.noise_func.0.bias"])
    if mut == "time_bias_of_neighbour":
        tb = tb.roll(1, 0)
    h = h + tb.view(x.shape[0], -1, 1, 1)
    if mut == "gn2_half_rows":
        assert g == 1
        n2 = _gn_half_rows(h, sd, p + ".block2.block.0")
    else:
        n2 = O._gn(h, sd, p + ".block2.block.0", g)
    h = _c3(O._swish(n2), sd[p + ".block2.block.3.weight"], sd[p + ".block2.block.3.bias"], "block2", mut)
    if mut == "no_residual":
        return h
    if (p + ".res_conv.weight") in sd:
        if mut == "res_conv_skipped":  # x itself on the channels both have
            c = h.shape[1]
            x = x[:, :c] if x.shape[1] >= c else F.pad(x, (0, 0, 0, 0, 0, c - x.shape[1]))
        else:
            x = F.conv2d(x, sd[p + ".res_conv.weight"], sd[p + ".res_conv.bias"])
    return h + x


def enc_stage(sd, cfg, p, x, c_enc, t, mut=None):
    """O.cond_injection on the resized RAW cond, then the ResnetBlock."""
    g = cfg["norm_groups"]
    q = p + ".cond_inj"
    cL = O._resize(c_enc, x.shape[-2:])
    if mut == "cond_of_neighbour":
        cL = cL.roll(1, 0)
    y = _c3(cL, sd[q + ".body.0.weight"], None, "body0", mut)
    y = F.silu(O._gn(y, sd, q + ".body.1", g))
    y = F.conv2d(y, sd[q + ".body.3.weight"], sd[q + ".body.3.bias"])
    scale, shift = y.chunk(2, dim=1)
    if mut == "film_swapped":
        scale, shift = shift, scale
    xc = F.conv2d(x, sd[q + ".x_conv.weight"], sd[q + ".x_conv.bias"])
    y = xc * scale + shift if mut == "film_scale_only" else xc * (1 + scale) + shift
    return res_stage(sd, cfg, p + ".res_block", y, t, mut)


def ffn_stage(sd, p, a, mut=None):
    """The feed-forward half of O.fast_attn_cond_injection (eval)."""
    f = _c3(a, sd[p + ".ffn.0.weight"], None, "ffn0", mut)
    f = _c3(f if mut == "no_silu" else F.silu(f), sd[p + ".ffn.2.weight"], None, "ffn2", mut)
    f = F.conv2d(f, sd[p + ".ffn.3.weight"], None if mut == "ffn3_nobias" else sd[p + ".ffn.3.bias"])
    return f if mut == "no_residual" else f + a


def final_stage(sd, cfg, x, mut=None):
    g = cfg["norm_groups"]
    if mut == "gn_half_rows":
        assert g == 1
        n = _gn_half_rows(x, sd, "final_conv.block.0")
    else:
        n = O._gn(x, sd, "final_conv.block.0", g)
    return _c3(n if mut == "no_silu" else O._swish(n), sd["final_conv.block.3.weight"], sd["final_conv.block.3.bias"], "conv", mut)


def apply(st, sd, cfg, ins, mut=None):
    kind, p = st["kind"], st["p"]
    if kind == "stem":
        return stem_stage(sd, p, *ins, mut=mut)
    if kind == "down":
        return down_stage(sd, p, *ins, mut=mut)
    if kind == "up":
        return up_stage(sd, p, *ins, mut=mut)
    if kind == "enc":
        return enc_stage(sd, cfg, p, *ins, mut=mut)
    if kind == "res":
        return res_stage(sd, cfg, p + ".res_block", *ins, mut=mut)
    if kind == "ffn":
        return ffn_stage(sd, p, *ins, mut=mut)
    if kind == "final":
        return final_stage(sd, cfg, *ins, mut=mut)
    assert mut is None
    g = cfg["norm_groups"]
    if kind == "cond":
        return O._resize(ins[0], ins[1].shape[-2:])
    if kind == "sa":
        return O.self_attention(sd, p, ins[0], g)
    if kind == "la":
        return O.linear_attention_mix(sd, p, torch.cat([ins[0], ins[1]], dim=1), ins[2], g)
    assert kind == "alias"
    return ins[0]


_C3 = ("transposed", "nobias", "seam")
_RES = ["block1:" + f for f in _C3] + ["block2:" + f for f in _C3] + ["time_bias_of_neighbour", "gn2_half_rows", "no_residual", "res_conv_skipped"]
MUTATIONS = {
    "stem": ["conv:" + f for f in _C3] + ["halves_swapped"],
    "down": ["conv:" + f for f in _C3] + ["odd_pixels"],
    "up": ["conv:" + f for f in _C3] + ["source_rounded_up"],
    "res": _RES,
    "enc": ["body0:transposed", "body0:seam", "film_swapped", "film_scale_only", "cond_of_neighbour"] + _RES,  # (body.0 has no bias)
    "ffn": ["ffn0:transposed", "ffn0:seam", "ffn2:transposed", "ffn2:seam", "no_silu", "no_residual", "ffn3_nobias"],  # (ffn.0 / ffn.2 have no bias)
    "final": ["conv:" + f for f in _C3] + ["no_silu", "gn_half_rows"],
}


def noop_by_construction(st, mut, sd, B):
    """The only mutations a site may skip: a neighbouring sample where there is one sample, a res_conv where there is none."""
    if mut in ("time_bias_of_neighbour", "cond_of_neighbour"):
        return B < 2
    if mut == "res_conv_skipped":
        return (st["p"] + ".res_block.res_conv.weight") not in sd
    return False


def _cast(ins, dtype):
    return tuple(v.to(dtype) for v in ins)


def chain(ds, sd, x, t, cond, sc, rec=None):
    """The whole stage list run on the network inputs, every stage fed by the stages before it.  rec: {stage index: its input tensors}."""
    cfg = gc.cfg_for(ds)
    C, P = cfg["lms_channel"], cfg["pan_channel"]
    val = {"@sc": sc, "@x": x, "@t": t, "@c_enc": cond[:, : C + P], "@c_dec": cond[:, -(C + 3 * P):]}
    for k, st in enumerate(stage_list(ds)):
        ins = tuple(val[n] for n in st["ins"])
        if rec is not None:
            rec[k] = ins
        val[st["out"]] = apply(st, sd, cfg, ins)
    return val["@y"]


# ------------------------------------------------------------------------------------------------ CPU only
def test_stage_list_covers_every_layer_and_attention_site():
    for ds in ("wv3", "gf2", "cave"):
        sa, la, layers = sites(ds)
        outs = [st["out"] for st in stage_list(ds)]
        assert len(outs) == len(set(outs))
        want = set(layers) | {p + s for p in sa for s in (".in", ".out")} | {p + s for p in la for s in (".cur", ".skip", ".cond", ".a", ".out")} | {"@y"}
        assert set(outs) == want, sorted(set(outs) ^ want)


def test_stage_chain_is_the_oracle_forward():
    """The stage functions of this file (mut=None), chained with the oracle's attention stages, reproduce O.unet_forward bit for bit in fp64: the restated
    stages are the oracle, and the stage list wires them as the network does."""
    case = "gf2_32_b2"
    ds = CASES[case][0]
    for kind in ("trained", "fixture"):
        sd = weights(ds, kind, torch.float64)
        x, t, cond, sc = (v.double() for v in inputs(case))
        with torch.no_grad():
            want = O.unet_forward(sd, gc.cfg_for(ds), x, t, cond, sc)
            got = chain(ds, sd, x, t, cond, sc)
        assert torch.equal(got, want), kind


@pytest.mark.parametrize("case", MUTATION_CASES)
def test_mutations_move_every_conv_stage_far_beyond_its_bound(case):
    """No library involved.  For every stage of this file, on the fp64 oracle's own stage input: each mutation of the fp64 stage moves the stage output by at
    least SENSITIVITY x the bound a library leg uses for that stage (MARGIN x e_ref).  This is what proves the legs can fail.  Weights: "strong", the
    trained-like ones strengthened where plain "trained" falls short of SENSITIVITY (strengthened() has the measured numbers); the legs run on them too."""
    ds, B = CASES[case][:2]
    cfg = gc.cfg_for(ds)
    sd32, sd64 = weights(ds, "strong"), weights(ds, "strong", torch.float64)
    x, t, cond, sc = (v.double() for v in inputs(case))
    rec = {}
    weak, skipped, n = [], [], 0
    with torch.no_grad():
        chain(ds, sd64, x, t, cond, sc, rec)
        for k, st in enumerate(stage_list(ds)):
            if st["kind"] not in MUTATIONS:
                continue
            ins32 = _cast(rec[k], torch.float32)  # what a library stage is handed: fp32 tensors
            ins64 = _cast(ins32, torch.float64)
            r64 = apply(st, sd64, cfg, ins64)
            e_ref = rel(apply(st, sd32, cfg, ins32), r64)
            bound = MARGIN * e_ref
            for mut in MUTATIONS[st["kind"]]:
                if noop_by_construction(st, mut, sd64, B):
                    skipped.append((stage_name(st), mut))
                    continue
                moved = rel(apply(st, sd64, cfg, ins64, mut), r64)
                n += 1
                print("%-14s %-24s %-24s e_ref %.2e  moved %.2e = %8.0f x bound" % (case, stage_name(st), mut, e_ref, moved, moved / bound))
                if not moved >= SENSITIVITY * bound:
                    weak.append((stage_name(st), mut, moved, bound))
    print("%s: %d mutations applied, %d skipped as no-ops by construction" % (case, n, len(skipped)))
    assert all(m in ("time_bias_of_neighbour", "cond_of_neighbour", "res_conv_skipped") for _, m in skipped)
    assert not weak, weak


# ------------------------------------------------------------------------------------------------ library legs
def run_library_leg(case, kind, device, where):
    """One tapped forward of `case` on the loaded library; every conv stage against the fp64 oracle on the tapped input.  Returns the table rows."""
    import ddif_testops as T
    from ddif import runtime

    ds, B, H, W, cap, _ = CASES[case]
    cfg = gc.cfg_for(ds)
    C, P = cfg["lms_channel"], cfg["pan_channel"]
    x, t, cond, sc = inputs(case)
    stages = stage_list(ds)
    sd32, sd64 = weights(ds, kind), weights(ds, kind, torch.float64)
    net = _make_net(ds, kind, device)
    try:
        runtime.set_debug_grid_cap(cap)
        plan = net.plan_for(B, H, W, torch.device(device))
    finally:
        runtime.set_debug_grid_cap(0)
    names = [n for n, *_ in T.plan_taps(plan)]
    assert len(names) == len(set(names))
    # coverage: every tap is the output of a stage of this file, of an attention stage of test_stage_parity.py, or an alias of one of those
    by_out = {st["out"]: st for st in stages}
    orphans = sorted(n for n in names if n not in by_out)
    assert not orphans, "taps that no stage writes: %s" % orphans
    absent = sorted(o for o in by_out if o != "@y" and o not in names)
    assert not absent, "stage outputs without a tap: %s" % absent
    before = plan.num_launches()
    plan.set_cond(cond.to(device), force=True)
    t0 = time.perf_counter()
    y, got = T.plan_forward_taps(plan, x.to(device), t, sc.to(device), None)
    assert plan.num_launches() == before
    if where == "gpu" or H * W < 4096:  # the tapped forward is the plain forward (a second 64 x 64 forward costs the emulator ~15 s)
        assert torch.equal(y, plan.forward(x.to(device), t, sc.to(device)))
    val = {k: v.cpu() for k, v in got.items()}
    t1 = time.perf_counter()
    bad_taps = [k for k, v in val.items() if not bool(torch.isfinite(v).all())]
    assert not bad_taps and bool(torch.isfinite(y).all()), bad_taps
    val.update({"@y": y.cpu(), "@sc": sc, "@x": x, "@t": t, "@c_enc": cond[:, : C + P], "@c_dec": cond[:, -(C + 3 * P):]})
    switches = " ".join("%s=%s" % (k[5:], os.environ[k]) for k in _SWITCHES if k in os.environ) or "-"
    rows, bad = [], []
    with torch.no_grad():
        for st in stages:
            ins, out = tuple(val[n] for n in st["ins"]), val[st["out"]]
            if st["kind"] == "alias":
                assert torch.equal(out, ins[0]), "%s is not %s" % (st["out"], st["ins"][0])
                continue
            if st["kind"] not in OWN:
                continue
            r64 = apply(st, sd64, cfg, _cast(ins, torch.float64))
            e_ref = rel(apply(st, sd32, cfg, _cast(ins, torch.float32)), r64)
            assert r64.shape == out.shape, (stage_name(st), r64.shape, out.shape)
            err = rel(out, r64)
            # (e_ref = 0: the resize to the full resolution is the identity in any precision -- and must be in the library: ratio 0, or inf)
            ratio = err / e_ref if e_ref > 0 else (0.0 if err == 0 else float("inf"))
            row = "%-5s %-15s %-9s %-12s %-22s %4dx%-3d %4d  e_ref %.3e  err %.3e  ratio %6.2f" % (
                where, case, kind, switches, stage_name(st), out.shape[2], out.shape[3], ins[0].shape[1], e_ref, err, ratio)
            rows.append(row)
            print(row)
            if not err <= MARGIN * e_ref:
                bad.append(row)
    t2 = time.perf_counter()
    print("%-5s %-15s %-9s %-12s time: forward(s) + copies %.2f s, fp32 + fp64 oracle stages %.2f s" % (where, case, kind, switches, t1 - t0, t2 - t1))
    path = os.environ.get("DDIF_STAGE_PARITY_TABLE")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(rows) + "\n")
    assert not bad, "\n" + "\n".join(bad)
    return rows


@pytest.mark.parametrize("case,kind", EMU_LEGS, ids=["%s-%s" % ck for ck in EMU_LEGS])
def test_conv_stages_match_the_fp64_oracle_on_the_emulator(case, kind):
    lib = use_emulator()
    assert lib.emulated
    run_library_leg(case, kind, "cpu", "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind", GPU_LEGS, ids=["%s-%s" % ck for ck in GPU_LEGS])
def test_conv_stages_match_the_fp64_oracle_on_the_gpu(case, kind):
    use_gpu_library()
    run_library_leg(case, kind, "cuda:0", "gpu")


# ------------------------------------------------------------------------------------------------ the benchmark batch
@pytest.mark.gpu
def test_batch64_taps_equal_single_tile_taps():
    """No oracle.  wv3 64 x 64, B = 64 (16 x 16 tilings, 64-cout items, eight-wave forms: what only a full GPU selects): every tap of samples 0, 37 and 63 is
    bit-equal to the tap of a B = 1 plan run on that tile -- the stage parity of the small-batch legs holds for every layer of the benchmark batch."""
    import ddif_testops as T

    use_gpu_library()
    dev = torch.device("cuda:0")
    ds, B, H, W = "wv3", 64, 64, 64
    spot = [0, 37, 63]
    g = torch.Generator().manual_seed(gc.zlib_seed("conv_stage_b64"))
    x = torch.randn(B, 8, H, W, generator=g).to(dev)
    sc = torch.randn(B, 8, H, W, generator=g).to(dev)
    t = torch.randint(0, 1000, (B,), generator=g)
    cond = gc.tiles_for(ds, B, H, W, seed=641)["cond"].to(dev)
    net = _make_net(ds, "fixture", dev)
    plan = net.plan_for(B, H, W, dev)
    plan.set_cond(cond, force=True)
    names = [n for n, *_ in T.plan_taps(plan)]
    assert len(names) == len([st for st in stage_list(ds) if st["out"] != "@y"])  # every layer, attention and cond_inj tap
    idx = torch.tensor(spot, device=dev)
    big = {}
    y = None
    for k in range(0, len(names), 8):  # at most 8 taps of the whole batch on the device at a time
        y, got = T.plan_forward_taps(plan, x, t, sc, names[k:k + 8])
        for n, v in got.items():
            big[n] = v.index_select(0, idx).cpu()
        del got
    big["@y"] = y.index_select(0, idx).cpu()
    one = net.plan_for(1, H, W, dev)
    assert [n for n, *_ in T.plan_taps(one)] == names
    differ = []
    for k, b in enumerate(spot):
        one.set_cond(cond[b:b + 1].contiguous(), force=True)
        y1, got = T.plan_forward_taps(one, x[b:b + 1].contiguous(), t[b:b + 1], sc[b:b + 1].contiguous(), None)
        got["@y"] = y1
        for n, v in got.items():
            if not torch.equal(v[0].cpu(), big[n][k]):
                differ.append((b, n))
    assert bool(torch.isfinite(big["@y"]).all())
    assert not differ, differ


# ------------------------------------------------------------------------------------------------ the conv switches
# The library reads its switches once per process: a fresh child process per setting runs ONE leg of this file, with a time limit.  A child that fails, dies or
# runs into its time limit fails its test with its output shown, and no further child is started: whatever took it down is not handed the device again.
GPU_SETTINGS = [{"DDIF_X3": "0"}, {"DDIF_F16": "0"}, {"DDIF_LR": "0"}, {"DDIF_S2_F16": "0"}, {"DDIF_XF": "0"}, {"DDIF_NB2": "1"}]
EMU_SETTINGS = [{"DDIF_LR": "0"}, {"DDIF_XF": "0"}, {"DDIF_F16": "0"}]
_lost = []


def _ids(settings):
    return ["+".join("%s=%s" % (k[5:], v) for k, v in e.items()) for e in settings]


def _leg_in_child(env, marker, select, prefix):
    if _lost:
        pytest.fail("not started: the child under %s did not end well" % _lost[0])
    e = dict(os.environ)
    e.update(env)
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", marker, "-x", "-q", "-s", "-k", select, "-p", "no:cacheprovider"],
                           env=e, cwd=ROOT, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as ex:
        _lost.append(env)
        pytest.fail("time limit: %s" % ((ex.stdout or b"")[-3000:],))
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith(prefix)]
    print("".join(ln + "\n" for ln in rows))  # the stage rows (e_ref, error, ratio) of this setting
    tail = (r.stdout + r.stderr)[-6000:]
    if r.returncode != 0 or "1 passed" not in r.stdout:
        _lost.append(env)
    assert r.returncode == 0, tail
    assert "1 passed" in r.stdout and "no tests ran" not in r.stdout, tail
    assert len(rows) > 50, tail


@pytest.mark.gpu
@pytest.mark.parametrize("env", GPU_SETTINGS, ids=_ids(GPU_SETTINGS))
def test_gpu_leg_under_conv_switch(env):
    _leg_in_child(env, "gpu", "match_the_fp64_oracle_on_the_gpu and wv3_64_b2 and fixture", "gpu ")


@pytest.mark.parametrize("env", EMU_SETTINGS, ids=_ids(EMU_SETTINGS))
def test_emulator_leg_under_conv_switch(env):
    _leg_in_child(env, "not gpu", "match_the_fp64_oracle_on_the_emulator and gf2_32_b2 and fixture", "emu ")
