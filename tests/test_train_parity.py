"""The native training step (csrc/ddif_train.cpp: train-mode NHWC forward + the reverse launch program) against fp64 autograd, PARAMETER BY PARAMETER.

tests/test_train_graph.py and the objective / l1ssim checks hold the step at square 16^2 / 32^2 / 64^2 tiles, on the seeded fixture weights, against fp32
autograd and under bounds relative to each tensor's norm with a floor (2e-4 ||g|| + 2e-6 gmax, or norms only under 2e-4 max(ref, 1e-4)): hundreds of
parameters whose gradient norm is below 1e-4 are not checked at all by such a floor.  Here one `train_forward_backward` per leg runs on the plan's own Philox
masks (p = 0.2 / 0.2, read back with `train_masks()`), and oracle/ddif_oracle.py `unet_forward(..., drop_masks, path_scales)` + torch autograd runs twice on
the CPU on the same inputs and masks, in fp64 (the reference) and in fp32 (the yardstick).  Per leg

  prediction        rel(y_lib, y_64) <= MARGIN x rel(y_32, y_64)                     (rel: max-abs over max-abs, as in test_stage_parity.py)
  loss              |loss_lib - loss_64| <= MARGIN x |loss_32 - loss_64| + 1 ulp(fp32)
  EVERY parameter   ||g_lib - g_64||_2 <= MARGIN x e_ref + FLOOR,   e_ref = ||g_32 - g_64||_2 of that parameter

MARGIN is test_stage_parity.py's (16).  FLOOR = 2^-24 x max|g_64| over the leg (the fp32 rounding of the largest per-element term) covers only e_ref = 0:
reference gradients that are exactly zero (the ffn branch under a DropPath scale of 0; the q branch where a softmax line has one element).  Where the zero
comes from a DropPath scale of exactly 0 the library's gradient must be EXACTLY zero.  No parameter is skipped: the gradients are bound pre-filled with NaN
and a leg fails by name on a NaN, and on any difference between `named_parameters()` and the oracle's keys.  Every leg also proves it is not vacuous: at
least MIN_LIVE parameters with ||g_64|| >= 1e-6 gmax, and with B >= 2 no DropPath site with every scale 0 (MASK_SEED is chosen for that).

Every parameter prints a row (where, case, weights, name, ||g|| / gmax, e_ref, err, ratio); DDIF_TRAIN_PARITY_TABLE=<file> appends them there
(profiles/train_parity.txt holds such rows from an MI355X run).

CASES: the smallest shapes at which each geometry can go wrong -- see the table.  The emulator runs the ones marked so: a step costs it 10 - 20 s, the eight
wv3 legs and the three objectives ~150 s in all; gf2_32_b2 (22 s a step) runs on the GPU only.  On the MI355X a leg takes ~1.2 s, the oracle's two runs included.
Weights: "fixture", "trained" (test_range_guard.trained_like(ds, 11) through test_conv_stage_parity.weights) and, on two cases, "stressed" (peaked
attention, test_stage_parity.py).  The objectives noise / l2, pred_v / l1 / p2 gamma 0.5 and x_start / l1ssim run the same comparison through
ddif_plan_train_step_ex on wv3_16_b2 under "trained" weights (test_training_step_under_another_objective_...): target, weighting and HybridL1SSIM are built
on the CPU in the run's precision.

What the 24 x 40 case found: a line group of csrc/kernels_linattn.h with more than 256 (line, channel quad) pairs left lines
un-normalised -- prediction 4.6e-4 off, 674 of 702 gradients beyond the bound, on the emulator and on the MI355X.  la_lines() now limits the group;
test_nhwc_linear_attention_with_many_short_lines holds the three kernels at such shapes.

CPU-only: FAULTS -- twelve faults of a backward pass (un-flipped taps, a bias gradient from half the rows, a dropped GroupNorm / softmax Jacobian term, a
mask forgotten in the backward, a neighbour's DropPath scale or time bias, swapped softmax axes, swapped FiLM gradients, the wrong 2 x 2 of an up- or
down-sampling) applied to the fp64 oracle graph: each moves a NAMED parameter gradient by at least SENSITIVITY x MARGIN x e_ref of that parameter
(test_faults_move_a_named_gradient_far_beyond_its_bound).  A reverse program with one of these faults cannot pass a leg."""
import math
import os
import time

import pytest
import torch
import torch.nn.functional as F

import golden_cases as gc
import test_conv_stage_parity as CSP
import test_stage_parity as SP
from ddif_testlib import use_emulator, use_gpu_library
from oracle import ddif_oracle as O
from test_backward_ops import BACKENDS, _dev  # (the other test files carry copies of these two)
from test_stage_parity import MARGIN, SENSITIVITY, rel

# id -> (data set, B, H, W, grid cap, runs on the emulator)
CASES = {
    # anchors the bound to the shape the reference golden pins
    "wv3_16_b2": ("wv3", 2, 16, 16, 0, True),
    # a 1 x 1 bottom level, 2 x 2 and 4 x 4 above it; softmax lines of one element (an exactly-zero q branch)
    "wv3_8_b2": ("wv3", 2, 8, 8, 0, True),
    # H != W, a 3 x 5 bottom level: the row and column line groups of csrc/kernels_linattn.h differ per axis
    "wv3_24x40_b1": ("wv3", 1, 24, 40, 0, True),
    # the same with sample strides
    "wv3_24x40_b2": ("wv3", 2, 24, 40, 0, False),
    # 4-band cond widths, 16 tokens
    "gf2_32_b2": ("gf2", 2, 32, 32, 0, False),
    # 31 / 34 channels: the zero-padded channels of the weight gradient, unpad_weight_kernel
    "cave_32_b1": ("cave", 1, 32, 32, 0, False),
    # grids capped to 3 workgroups: several items and samples per workgroup in the reverse program
    "wv3_32_b3_cap3": ("wv3", 3, 32, 32, 3, False),
}
STRESSED_CASES = ("wv3_16_b2", "wv3_24x40_b1")
LEGS = [(c, k) for c in CASES for k in ("fixture", "trained")] + [(c, "stressed") for c in STRESSED_CASES]
EMU_LEGS = [(c, k) for c, k in LEGS if CASES[c][5]]

MASK_SEED = 4242
P_DROPOUT = P_DROPPATH = 0.2
MIN_LIVE = 300          # parameters with ||g_64|| >= LIVE x gmax, in every leg
LIVE = 1e-6
ULP32 = 2.0 ** -23


# ------------------------------------------------------------------------------------------------ inputs, masks
def inputs(case):
    """SP.inputs (seeded by the case id; t = [5, 700, 321][:B]) plus an L1 target in [0, 1)."""
    SP.CASES[case], keep = CASES[case], SP.CASES.get(case)
    try:
        x, t, cond, sc = SP.inputs(case)
    finally:
        if keep is None:
            del SP.CASES[case]
        else:
            SP.CASES[case] = keep
    g = torch.Generator().manual_seed(gc.zlib_seed("train_" + case))
    return x, t, cond, sc, torch.rand(x.shape, generator=g)


def dec_sites(ds):
    """State-dict prefixes of the decoder blocks, in execution order: DropPath site k is the ffn branch of dec_sites(ds)[k]."""
    return ["ups.%d" % i for i, L in enumerate(O.layer_plan(gc.cfg_for(ds))["ups"]) if L["kind"] == "dec"]


def train_plan(case, kind, device):
    """(net in .train(), its train-mode plan with the masks of MASK_SEED drawn, masks on the CPU, DropPath scales (sites, B) on the CPU)."""
    from ddif import runtime

    ds, B, H, W, cap, _ = CASES[case]
    CSP.weights(ds, kind)  # (enters "trained" into SP's cache)
    net = SP._make_net(ds, kind, device).train()
    try:
        runtime.set_debug_grid_cap(cap)
        plan = net.plan_for(B, H, W, torch.device(device), train=True)
    finally:
        runtime.set_debug_grid_cap(0)
    plan.random_train_masks(MASK_SEED, 0, P_DROPOUT, P_DROPPATH)
    masks, paths = plan.train_masks()
    return net, plan, [m.cpu() for m in masks], paths.cpu()


# ------------------------------------------------------------------------------------------------ the oracle side
def l1_objective(target):
    return lambda y: (y - target.to(y.dtype)).abs().mean()


def oracle_grads(ds, sd, x, t, cond, sc, masks, paths, objective, dtype, forward=None):
    """(prediction, loss, {name: gradient}) of the oracle forward + autograd in `dtype`.  forward: a restated forward with the signature of O.unet_forward."""
    P = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point()}
    full = dict(sd)
    full.update(P)
    y = (forward or O.unet_forward)(full, gc.cfg_for(ds), x(dtype) if callable(x) else x.to(dtype), t.to(dtype), cond.to(dtype), sc.to(dtype),
                                    drop_masks=[m.to(dtype) for m in masks], path_scales=[p.to(dtype) for p in paths])
    loss = objective(y)
    loss.backward()
    missing = sorted(k for k, v in P.items() if v.grad is None)
    assert not missing, "the oracle graph does not reach %s" % missing
    return y.detach(), loss.detach(), {k: v.grad for k, v in P.items()}


_ref_cache = {}


def references(case, kind, masks, paths, tag="l1", objective=None, extra=None):
    """The fp64 and fp32 oracle runs of a leg, computed once per (case, weights, objective) and left unchanged.  extra = (x or a function dtype -> x, t)
    replaces the network input and the timesteps (the objectives: x_t is formed in the run's dtype); objective: a function y -> loss (y in the run's dtype)."""
    key = (case, kind, tag)
    hit = _ref_cache.get(key)
    if hit is not None and len(hit[0]) == len(masks) and all(torch.equal(a, b) for a, b in zip(hit[0], masks)) and torch.equal(hit[1], paths):
        return hit[2], hit[3]
    ds = CASES[case][0]
    x, t, cond, sc, target = inputs(case)
    if extra is not None:
        x, t = extra
    objective = objective or l1_objective(target)
    sd = CSP.weights(ds, kind, torch.float64)
    r64 = oracle_grads(ds, sd, x, t, cond, sc, masks, paths, objective, torch.float64)
    r32 = oracle_grads(ds, CSP.weights(ds, kind), x, t, cond, sc, masks, paths, objective, torch.float32)
    _ref_cache[key] = (masks, paths, r64, r32)
    return r64, r32


def leaf_condition(case, g64, paths):
    """What keeps a leg from being vacuous: enough live gradients, and with B >= 2 no DropPath branch that is dead for the whole batch."""
    B = CASES[case][1]
    norms = {n: float(g.norm()) for n, g in g64.items()}
    gmax = max(norms.values())
    live = sum(1 for v in norms.values() if v >= LIVE * gmax)
    dead = [dec_sites(CASES[case][0])[k] for k in range(paths.shape[0]) if float(paths[k].abs().max()) == 0.0]
    assert live >= MIN_LIVE, "%s: only %d of %d parameters have ||g_64|| >= %g gmax" % (case, live, len(norms), LIVE)
    if B >= 2:
        assert not dead, "%s: DropPath scale 0 for every sample at %s -- choose another MASK_SEED" % (case, dead)
        zero = sorted(n for n, g in g64.items() if ".cond_inj.ffn." in n and not bool(g.any()))
        assert not zero, zero
    return live, dead


# ------------------------------------------------------------------------------------------------ the comparison
def compare(where, case, kind, tag, y, loss, grads, names, r64, r32, paths):
    """The assertions of a leg on what the library returned (CPU tensors).  Returns the table rows."""
    ds = CASES[case][0]
    y64, l64, g64 = r64
    y32, l32, g32 = r32
    label = kind if tag == "l1" else "%s/%s" % (kind, tag)
    assert sorted(names) == sorted(g64), "named_parameters() and the oracle's keys differ: %s" % sorted(set(names) ^ set(g64))
    unwritten = sorted(n for n in names if bool(torch.isnan(grads[n]).any()))
    assert not unwritten, "gradients not written (still NaN): %s" % unwritten
    live, dead = leaf_condition(case, g64, paths)
    bad = []
    # prediction and loss
    e_y, err_y = rel(y32, y64), rel(y, y64)
    e_l, err_l = abs(float(l32) - float(l64)), abs(float(loss) - float(l64))
    print("%-5s %-15s %-9s prediction  e_ref %.3e  err %.3e  ratio %6.2f" % (where, case, label, e_y, err_y, err_y / e_y))
    print("%-5s %-15s %-9s loss %.9f  e_ref %.3e  err %.3e" % (where, case, label, float(l64), e_l, err_l))
    if not err_y <= MARGIN * e_y:
        bad.append("prediction: rel(y_lib, y_64) %.3e > %g x %.3e" % (err_y, MARGIN, e_y))
    if not err_l <= MARGIN * e_l + ULP32 * abs(float(l64)):
        bad.append("loss: |loss_lib - loss_64| %.3e > %g x %.3e + 1 ulp" % (err_l, MARGIN, e_l))
    # every parameter
    gmax = max(float(g.norm()) for g in g64.values())
    floor = 2.0 ** -24 * max(float(g.abs().max()) for g in g64.values())
    dead_ffn = tuple(p + ".cond_inj.ffn." for p in dead)
    rows = []
    for n in names:
        got, ref = grads[n].double(), g64[n]
        assert got.shape == ref.shape, (n, got.shape, ref.shape)
        e_ref, err = float((g32[n].double() - ref).norm()), float((got - ref).norm())
        ratio = err / e_ref if e_ref > 0 else (0.0 if err == 0 else float("inf"))
        row = "%-5s %-15s %-9s %-52s |g|/gmax %.3e  e_ref %.3e  err %.3e  ratio %8.2f" % (where, case, label, n, float(ref.norm()) / gmax, e_ref, err, ratio)
        rows.append(row)
        print(row)
        if not err <= MARGIN * e_ref + floor:
            bad.append(row)
        if n.startswith(dead_ffn) and dead_ffn:  # a DropPath scale of exactly 0: exactly no gradient
            assert not bool(ref.any()), n
            if bool(got.any()):
                bad.append(row + "   (must be exactly zero: DropPath scale 0)")
    print("%-5s %-15s %-9s %d parameters, %d live, floor %.3e, %d beyond the bound" % (where, case, label, len(names), live, floor, len(bad)))
    path = os.environ.get("DDIF_TRAIN_PARITY_TABLE")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(rows) + "\n")
    assert not bad, "\n" + "\n".join(bad[:40]) + ("\n... %d in all" % len(bad) if len(bad) > 40 else "")
    return rows


def run_library_leg(case, kind, device, where):
    """One native training step of `case` on the loaded library against the two oracle runs."""
    x, t, cond, sc, target = inputs(case)
    t0 = time.perf_counter()
    net, plan, masks, paths = train_plan(case, kind, device)
    net._net.refresh_from_device(net.named_parameters())  # fills the dgrad packs
    plan.set_cond(cond.to(device), force=True)
    grads = {n: torch.full_like(p, float("nan")) for n, p in net.named_parameters()}
    plan.train_bind(list(grads.items()))
    loss, y = plan.train_forward_backward(x.to(device), t, sc.to(device), target.to(device))
    loss, y = loss.cpu(), y.cpu()
    got = {n: g.cpu() for n, g in grads.items()}
    t1 = time.perf_counter()
    r64, r32 = references(case, kind, masks, paths)
    t2 = time.perf_counter()
    print("%-5s %-15s %-9s time: plan + step + copies %.2f s, fp64 + fp32 oracle and autograd %.2f s" % (where, case, kind, t1 - t0, t2 - t1))
    return compare(where, case, kind, "l1", y, loss, got, list(grads), r64, r32, paths)


GPU_ONLY_LEGS = [ck for ck in LEGS if ck not in EMU_LEGS]


@pytest.mark.parametrize("case,kind", GPU_ONLY_LEGS, ids=["%s-%s" % ck for ck in GPU_ONLY_LEGS])
def test_gpu_only_legs_are_not_vacuous(case, kind):
    """The leaf condition of the legs the CPU suite does not run, on the CPU: the masks the GPU will draw (Philox: the emulator draws the same), the fp64
    oracle graph, enough live gradients and no DropPath branch dead for a whole batch of two or more."""
    masks, paths = emulator_masks(case, kind)
    sd = CSP.weights(CASES[case][0], kind, torch.float64)
    x, t, cond, sc, target = inputs(case)
    _, _, g64 = oracle_grads(CASES[case][0], sd, x, t, cond, sc, masks, paths, l1_objective(target), torch.float64)
    live, dead = leaf_condition(case, g64, paths)
    print("%-15s %-9s %d live of %d, DropPath sites dead for the batch: %s" % (case, kind, live, len(g64), dead))


@pytest.mark.parametrize("case,kind", EMU_LEGS, ids=["%s-%s" % ck for ck in EMU_LEGS])
def test_training_step_matches_fp64_autograd_on_the_emulator(case, kind):
    lib = use_emulator()
    assert lib.emulated
    run_library_leg(case, kind, "cpu", "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind", LEGS, ids=["%s-%s" % ck for ck in LEGS])
def test_training_step_matches_fp64_autograd_on_the_gpu(case, kind):
    use_gpu_library()
    run_library_leg(case, kind, "cuda:0", "gpu")


# ------------------------------------------------------------------------------------------------ the sensitivity proof (CPU only, no library)
# The oracle forward restated (train mode) with one hook per fault.  A fault of the BACKWARD only is written as a forward expression with the same value and
# another gradient: v(A) + B - v(B) has A's value and B's gradient (v = detach), and a term whose factor is detached loses that factor's Jacobian.
def _v(t):
    return t.detach()


def _conv3(x, w, b, fault=None, stride=1):
    """3 x 3 conv, padding 1.  Faults: "unflipped" (dL/dx correlates dy with the taps as they are -- the gradient of a conv with flipped taps), "odd_pixels"
    (stride 2: dL/dx of a conv centred on input (2i + 1, 2j + 1)), "bias_half_rows" (dL/db summed over the upper half of the rows)."""
    if fault == "unflipped":
        y = F.conv2d(_v(x), w, None, stride=stride, padding=1) + F.conv2d(x, _v(w).flip(2, 3), None, stride=stride, padding=1) \
            - F.conv2d(_v(x), _v(w).flip(2, 3), None, stride=stride, padding=1)
    elif fault == "odd_pixels":
        sh = lambda u: F.pad(u[..., 1:, 1:], (0, 1, 0, 1))  # noqa: E731
        y = F.conv2d(_v(x), w, None, stride=stride, padding=1) + F.conv2d(sh(x), _v(w), None, stride=stride, padding=1) \
            - F.conv2d(sh(_v(x)), _v(w), None, stride=stride, padding=1)
    elif fault == "bias_half_rows" or b is None:
        y = F.conv2d(x, w, None, stride=stride, padding=1)
    else:
        return F.conv2d(x, w, b, stride=stride, padding=1)
    if b is None:
        return y
    if fault == "bias_half_rows":
        rows = torch.zeros(1, 1, y.shape[2], 1, dtype=y.dtype)
        rows[:, :, : y.shape[2] // 2] = 1
        return y + _v(b).view(1, -1, 1, 1) + (b - _v(b)).view(1, -1, 1, 1) * rows
    return y + b.view(1, -1, 1, 1)


def _gn1(x, sd, key, fault=None):
    """GroupNorm, one group.  Fault "gn_no_projection": the backward without the x_hat * mean(dy * x_hat) term -- the Jacobian of 1 / sigma."""
    if fault != "gn_no_projection":
        return O._gn(x, sd, key, 1)
    m = x.mean((1, 2, 3), keepdim=True)
    r = torch.rsqrt(x.var((1, 2, 3), unbiased=False, keepdim=True) + 1e-5)
    return (x - m) * _v(r) * sd[key + ".weight"].view(1, -1, 1, 1) + sd[key + ".bias"].view(1, -1, 1, 1)


def f_resnet_block(sd, p, x, temb, mask, fault):
    ft = fault[0] if fault and fault[1] == p else None
    h = _conv3(O._swish(_gn1(x, sd, p + ".block1.block.0")), sd[p + ".block1.block.3.weight"], sd[p + ".block1.block.3.bias"],
               "bias_half_rows" if ft == "bias_half_rows" else None)
    tb = F.linear(temb, sd[p + ".noise_func.noise_func.0.weight"], sd[p + ".noise_func.noise_func.0.bias"])
    if ft == "time_bias_of_neighbour":
        tb = tb.roll(1, 0)
    h = h + tb.view(x.shape[0], -1, 1, 1)
    a2 = O._swish(_gn1(h, sd, p + ".block2.block.0", ft))
    if mask is not None:
        a2 = a2 + _v(a2 * mask - a2) if ft == "dropout_mask_forgotten" else a2 * mask
    h = _conv3(a2, sd[p + ".block2.block.3.weight"], sd[p + ".block2.block.3.bias"], "unflipped" if ft == "unflipped" else None)
    if (p + ".res_conv.weight") in sd:
        x = F.conv2d(x, sd[p + ".res_conv.weight"], sd[p + ".res_conv.bias"])
    return h + x


def f_self_attention(sd, p, x, fault, n_head=8):
    B, C, H, W = x.shape
    d = C // n_head
    qkv = F.conv2d(O._gn(x, sd, p + ".norm", 1), sd[p + ".qkv.weight"]).view(B, n_head, 3 * d, H * W)
    q, k, v = qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
    s = torch.einsum("bncp,bncq->bnpq", q, k) / math.sqrt(C)
    if fault and fault == ("sa_softmax_no_rowsum", p):  # exp(s - max) / Z with Z held: the Jacobian keeps its diagonal a_i only
        e = torch.exp(s - _v(s.max(-1, keepdim=True).values))
        a = e / _v(e.sum(-1, keepdim=True))
    else:
        a = torch.softmax(s, dim=-1)
    o = torch.einsum("bnpq,bncq->bncp", a, v).reshape(B, C, H, W)
    return F.conv2d(o, sd[p + ".out.weight"], sd[p + ".out.bias"]) + x


def f_cond_injection(sd, p, x, cL, fault):
    y = F.conv2d(cL, sd[p + ".body.0.weight"], None, padding=1)
    y = F.silu(O._gn(y, sd, p + ".body.1", 1))
    y = F.conv2d(y, sd[p + ".body.3.weight"], sd[p + ".body.3.bias"])
    scale, shift = y.chunk(2, dim=1)
    xc = F.conv2d(x, sd[p + ".x_conv.weight"], sd[p + ".x_conv.bias"])
    if fault and fault == ("film_grads_swapped", p):  # scale receives dy (shift's gradient), shift receives dy * xc (scale's)
        return xc * (1 + _v(scale)) + _v(shift) + (scale - _v(scale)) + (shift - _v(shift)) * _v(xc)
    return xc * (1 + scale) + shift


def f_fast_attn(sd, p, x, cL, path_scale, fault, heads=8):
    ft = fault[0] if fault and fault[1] == p else None
    B, Cf, H, W = x.shape
    xn = O._gn(x, sd, p + ".prenorm_x", 1)
    q = F.conv2d(F.conv2d(xn, sd[p + ".q.0.weight"], None, padding=1, groups=Cf), sd[p + ".q.1.weight"], sd[p + ".q.1.bias"])
    kv = F.conv2d(F.conv2d(cL, sd[p + ".kv.0.weight"], None, padding=1, groups=cL.shape[1]), sd[p + ".kv.1.weight"], sd[p + ".kv.1.bias"])
    k, v = kv.chunk(2, dim=1)
    q = q.softmax(dim=-1 if ft == "q_softmax_over_W" else -2)
    k = k.softmax(dim=-2 if ft == "k_softmax_over_H" else -1)
    qd = q.shape[1]
    d = qd // heads
    q = q.reshape(B, heads, d, H * W) * (1.0 / math.sqrt(d))
    k = k.reshape(B, heads, d, H * W)
    v = v.reshape(B, heads, d, H * W)
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    o = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(B, qd, H, W)
    a = F.conv2d(o, sd[p + ".attn_out.weight"], sd[p + ".attn_out.bias"])
    if (p + ".attn_res.weight") in sd:
        a = a + F.conv2d(xn, sd[p + ".attn_res.weight"], sd[p + ".attn_res.bias"])
    else:
        a = a + xn
    f = F.conv2d(a, sd[p + ".ffn.0.weight"], None, padding=1)
    f = F.conv2d(F.silu(f), sd[p + ".ffn.2.weight"], None, padding=1)
    f = F.conv2d(f, sd[p + ".ffn.3.weight"], sd[p + ".ffn.3.bias"])
    if path_scale is not None:
        f = f * (path_scale.roll(1, 0) if ft == "droppath_of_neighbour" else path_scale).view(-1, 1, 1, 1)
    return f + a


def faulty_forward(fault=None):
    """O.unet_forward (train mode, masks given) restated on the functions above; fault = (name, state-dict prefix of its site) or None."""
    def forward(sd, cfg, x, time, cond, self_cond, drop_masks, path_scales):
        assert cfg["norm_groups"] == 1 and cfg["self_condition"]
        masks, paths = iter(drop_masks), iter(path_scales)
        C, P = cfg["lms_channel"], cfg["pan_channel"]
        plan = O.layer_plan(cfg)
        x = torch.cat([self_cond, x], dim=1)
        temb = O.time_embedding(sd, time, cfg["inner_channel"])
        c_enc, c_dec = cond[:, : C + P], cond[:, -(C + 3 * P):]
        feats = []
        for i, L in enumerate(plan["downs"]):
            p = "downs.%d" % i
            if L["kind"] == "stem":
                x = F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"], padding=1)
            elif L["kind"] == "down":
                x = _conv3(x, sd[p + ".conv.weight"], sd[p + ".conv.bias"], "odd_pixels" if fault == ("downsample_odd_pixels", p) else None, stride=2)
            else:
                x = f_cond_injection(sd, p + ".cond_inj", x, O._resize(c_enc, x.shape[-2:]), fault)
                x = f_resnet_block(sd, p + ".res_block", x, temb, next(masks), fault)
                if L["attn"]:
                    x = f_self_attention(sd, p + ".attn", x, fault)
            feats.append(x)
        for i, L in enumerate(plan["mid"]):
            p = "mid.%d" % i
            x = f_resnet_block(sd, p + ".res_block", x, temb, next(masks), fault)
            if L["attn"]:
                x = f_self_attention(sd, p + ".attn", x, fault)
        for i, L in enumerate(plan["ups"]):
            p = "ups.%d" % i
            if L["kind"] == "up":
                up = F.interpolate(x, scale_factor=2, mode="nearest")
                if fault == ("upsample_wrong_2x2", p):  # the backward sums the 2 x 2 of source pixel (y + 1) // 2
                    H, W = x.shape[-2:]
                    iy = ((torch.arange(2 * H) + 1) // 2).clamp(max=H - 1)
                    ix = ((torch.arange(2 * W) + 1) // 2).clamp(max=W - 1)
                    wrong = x[..., iy, :][..., ix]
                    up = _v(up) + wrong - _v(wrong)
                x = F.conv2d(up, sd[p + ".conv.weight"], sd[p + ".conv.bias"], padding=1)
            else:
                x = torch.cat([x, feats.pop()], dim=1)
                x = f_fast_attn(sd, p + ".cond_inj", x, O._resize(c_dec, x.shape[-2:]), next(paths), fault)
                x = f_resnet_block(sd, p + ".res_block", x, temb, next(masks), fault)
                if L["attn"]:
                    x = f_self_attention(sd, p + ".attn", x, fault)
        x = O._swish(O._gn(x, sd, "final_conv.block.0", 1))
        return F.conv2d(x, sd["final_conv.block.3.weight"], sd["final_conv.block.3.bias"], padding=1)
    return forward


def fault_list(ds, paths):
    """[(fault, site, the parameter whose gradient it must move)] for a data set: one site per fault, the parameter right upstream of it."""
    plan = O.layer_plan(gc.cfg_for(ds))
    enc = "downs.%d" % [i for i, L in enumerate(plan["downs"]) if L["kind"] == "enc"][1]
    down = "downs.%d" % [i for i, L in enumerate(plan["downs"]) if L["kind"] == "down"][0]
    before_down = "downs.%d" % (int(down[6:]) - 1)
    up_i = [i for i, L in enumerate(plan["ups"]) if L["kind"] == "up"][-1]
    up, before_up = "ups.%d" % up_i, "ups.%d" % (up_i - 1)
    dec = dec_sites(ds)
    la = dec[len(dec) // 2]
    differ = [dec[k] for k in range(paths.shape[0]) if float(paths[k].max()) != float(paths[k].min())]
    dp = differ[-1] if differ else dec[-1]  # the last site whose samples drew different scales
    sa = ["ups.%d" % i for i, L in enumerate(plan["ups"]) if L.get("attn")][-1]
    rb = enc + ".res_block"
    return [
        ("unflipped", rb, rb + ".block2.block.0.weight"),
        ("bias_half_rows", rb, rb + ".block1.block.3.bias"),
        ("gn_no_projection", rb, rb + ".block1.block.3.weight"),
        ("dropout_mask_forgotten", rb, rb + ".block2.block.0.weight"),
        ("droppath_of_neighbour", dp + ".cond_inj", dp + ".cond_inj.ffn.3.weight"),
        ("q_softmax_over_W", la + ".cond_inj", la + ".cond_inj.q.1.weight"),
        ("k_softmax_over_H", la + ".cond_inj", la + ".cond_inj.kv.1.weight"),
        ("sa_softmax_no_rowsum", sa + ".attn", sa + ".attn.qkv.weight"),
        ("time_bias_of_neighbour", rb, rb + ".noise_func.noise_func.0.weight"),
        ("film_grads_swapped", enc + ".cond_inj", enc + ".cond_inj.body.3.weight"),
        ("upsample_wrong_2x2", up, before_up + ".res_block.block2.block.3.weight"),
        ("downsample_odd_pixels", down, before_down + ".res_block.block2.block.3.weight"),
    ]


NEIGHBOUR_FAULTS = ("droppath_of_neighbour", "time_bias_of_neighbour")  # no-ops by construction where there is one sample
FAULT_CASES = ("wv3_16_b2", "wv3_24x40_b1", "gf2_32_b2")
FAULT_WEIGHTS = ("fixture", "trained")
# Measured (factor = moved / bound; SENSITIVITY asks 50).  "fixture": every fault at every case >= 109 (the smallest: k_softmax_over_H on the square cases, 313
# at wv3_16_b2 and 109 at gf2_32_b2 against 3400 at wv3_24x40_b1; everything else >= 1000).  "trained": every fault >= 387 (gn_no_projection, gf2_32_b2) but
# two.  The self-attention sites sit at the bottom level, where trained-like gains leave gradients of ~1e-7 of the largest one (about half of the 702
# parameters are below 1e-6 gmax under these weights): sa_softmax_no_rowsum moves ups.3.attn.qkv.weight by 1 - 2 x its bound, FLOOR included, so under
# "trained" a leg cannot see it -- the "fixture" leg of the same case does (>= 1000).  k_softmax_over_H reaches 21 (wv3_16_b2) and 1 (gf2_32_b2) on the square
# cases under "trained" and 3372 at wv3_24x40_b1: asserted there.
NOT_SEEN_UNDER_TRAINED = {"sa_softmax_no_rowsum": FAULT_CASES, "k_softmax_over_H": ("wv3_16_b2", "gf2_32_b2")}


def emulator_masks(case, kind):
    """The masks a leg of `case` runs under (Philox: the same on the emulator and on the GPU), without running a step."""
    use_emulator()
    _, _, masks, paths = train_plan(case, kind, "cpu")
    return masks, paths


def test_restated_forward_is_the_oracle_forward_and_backward():
    """faulty_forward(None) IS O.unet_forward under masks: the same prediction and the same gradients, to the last bit, in fp64."""
    case, kind = "wv3_8_b2", "trained"
    ds = CASES[case][0]
    masks, paths = emulator_masks(case, kind)
    x, t, cond, sc, target = inputs(case)
    sd = CSP.weights(ds, kind, torch.float64)
    y0, l0, g0 = oracle_grads(ds, sd, x, t, cond, sc, masks, paths, l1_objective(target), torch.float64)
    y1, l1, g1 = oracle_grads(ds, sd, x, t, cond, sc, masks, paths, l1_objective(target), torch.float64, forward=faulty_forward(None))
    assert torch.equal(y0, y1) and torch.equal(l0, l1)
    assert sorted(g0) == sorted(g1) and all(torch.equal(g0[n], g1[n]) for n in g0)


@pytest.mark.parametrize("kind", FAULT_WEIGHTS)
@pytest.mark.parametrize("case", FAULT_CASES)
def test_faults_move_a_named_gradient_far_beyond_its_bound(case, kind):
    """No library step involved.  Each fault of FAULTS, applied to the fp64 oracle graph at one site, moves the gradient of the parameter right upstream of
    it by at least SENSITIVITY x the bound a leg holds that parameter to (MARGIN x e_ref + FLOOR) -- under the weights and masks the legs run on: every
    fault under "fixture", and under "trained" all but NOT_SEEN_UNDER_TRAINED (measured factors there).  The swapped k axis is weak on square tiles under
    "trained"; the 24 x 40 case is where the axes cannot cancel (H != W), and there it is asserted under both."""
    ds, B = CASES[case][:2]
    masks, paths = emulator_masks(case, kind)
    x, t, cond, sc, target = inputs(case)
    (y64, l64, g64), (_, _, g32) = references(case, kind, masks, paths)
    floor = 2.0 ** -24 * max(float(g.abs().max()) for g in g64.values())
    sd = CSP.weights(ds, kind, torch.float64)
    weak, skipped = [], []
    for fault, site, name in fault_list(ds, paths):
        if fault in NEIGHBOUR_FAULTS and B < 2:
            skipped.append(fault)
            continue
        _, _, g = oracle_grads(ds, sd, x, t, cond, sc, masks, paths, l1_objective(target), torch.float64, forward=faulty_forward((fault, site)))
        assert name in g, name
        bound = MARGIN * float((g32[name].double() - g64[name]).norm()) + floor
        moved = float((g[name] - g64[name]).norm())
        most = max(g, key=lambda n: float((g[n] - g64[n]).norm()) / (MARGIN * float((g32[n].double() - g64[n]).norm()) + floor))
        print("%-15s %-9s %-24s at %-22s %-48s moved %.3e = %9.0f x bound   (most moved: %s)" % (case, kind, fault, site, name, moved, moved / bound, most))
        if kind == "trained" and case in NOT_SEEN_UNDER_TRAINED.get(fault, ()):
            continue  # (printed above; the "fixture" run of this case asserts it)
        if not moved >= SENSITIVITY * bound:
            weak.append((fault, site, name, moved, bound))
    assert all(f in NEIGHBOUR_FAULTS for f in skipped)
    assert not weak, weak


# ------------------------------------------------------------------------------------------------ the other objectives, through train_step
# (pred_mode, loss_type, p2 gamma): the two parameterisations of golden_cases_objective.GRAD_CASES, pinned there at fixture weights only; T and t are theirs.
# x_t = a x0 + s noise with the schedule rows of oracle.schedule_tables; target noise / v = a noise - s x0 (diffusion_ddpm_pan.py:304-308); F.mse_loss /
# F.l1_loss; p2: the reference's loss_func has already reduced to a scalar, so the weighting is loss x mean_b(p2_loss_weight[t_b]) (:762-764).
OBJECTIVE_CASE, OBJECTIVE_WEIGHTS = "wv3_16_b2", "trained"


def hybrid_l1_ssim(img1, img2, weights):
    """HybridL1SSIM as csrc/kernels_ssimloss.h states it: L1 x w_l1 + (1 - mean(ssim_map)) x w_ssim; the map from the 11 x 11 Gaussian window (sigma 1.5: the
    taps in fp32, divided by their fp32 sum -- constants, the same in every precision), zero padding 5, per channel; C1 = 0.01^2, C2 = 0.03^2."""
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(k * k) / (2.0 * 1.5 * 1.5)).float()
    g = g / g.sum()
    C = img1.shape[1]
    win = (g.view(-1, 1) @ g.view(1, -1)).to(img1.dtype).expand(C, 1, 11, 11).contiguous()
    f = lambda u: F.conv2d(u, win, padding=5, groups=C)  # noqa: E731
    mu1, mu2 = f(img1), f(img2)
    s11, s22, s12 = f(img1 * img1) - mu1 * mu1, f(img2 * img2) - mu2 * mu2, f(img1 * img2) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return (img1 - img2).abs().mean() * weights[0] + (1 - smap.mean()) * weights[1]


def objective_setup(pm, lt, gamma):
    """(x0, noise, a, s, t, p2 rows or None, x_t as a function of the dtype, the loss as a function of the prediction) of an objective leg, built on the CPU."""
    import golden_cases_objective as go

    import golden_cases_l1ssim as gl

    (T, tvals), = {(c[5], tuple(c[6])) for c in go.GRAD_CASES} | {(c[5], tuple(c[6])) for c in gl.GRAD_CASES[:1]}
    assert (pm, lt, gamma) in [(c[7], c[8], c[9]) for c in go.GRAD_CASES] + [(c[7], "l1ssim", c[8]) for c in gl.GRAD_CASES[:1]]
    noise, _, _, _, x0 = inputs(OBJECTIVE_CASE)  # (the seeded randn tensor serves as the noise, the rand one as x_start)
    tabs = O.schedule_tables(O.cosine_betas(T), p2_gamma=gamma)
    t = torch.tensor(tvals, dtype=torch.long)
    a, s = tabs["sqrt_alphas_cumprod"][t], tabs["sqrt_one_minus_alphas_cumprod"][t]
    w = tabs["p2_loss_weight"][t] if gamma else None

    def r(v, dtype):
        return v.to(dtype).view(-1, 1, 1, 1)

    def x_t(dtype):
        return r(a, dtype) * x0.to(dtype) + r(s, dtype) * noise.to(dtype)

    def objective(y):
        d = y.dtype
        target = x0.to(d) if pm == "x_start" else (noise.to(d) if pm == "noise" else r(a, d) * noise.to(d) - r(s, d) * x0.to(d))
        if lt == "l1ssim":
            loss = hybrid_l1_ssim(target, y, gl.WEIGHTS)
        else:
            loss = ((y - target) ** 2).mean() if lt == "l2" else (y - target).abs().mean()
        return loss * w.to(d).mean() if w is not None else loss

    return x0, noise, a, s, t, w, x_t, objective


def run_objective_leg(pm, lt, gamma, device, where):
    import ctypes as C

    from ddif.runtime import _ptr, _row, _stream

    case, kind = OBJECTIVE_CASE, OBJECTIVE_WEIGHTS
    _, _, cond, sc, _ = inputs(case)
    x0, noise, a, s, t, w, x_t, objective = objective_setup(pm, lt, gamma)
    net, plan, masks, paths = train_plan(case, kind, device)
    net._net.refresh_from_device(net.named_parameters())
    plan.set_objective(pm, lt)
    plan.set_cond(cond.to(device), force=True)
    grads = {n: torch.full_like(p, float("nan")) for n, p in net.named_parameters()}
    plan.train_bind(list(grads.items()))
    # PlanHandle.train_step with the raw network output asked for (it returns recon_x0): the same entry point, ddif_plan_train_step_ex
    tabs = O.schedule_tables(O.cosine_betas(500))
    rec = (None, None) if pm == "x_start" else (tabs["sqrt_recip_alphas_cumprod"][t], tabs["sqrt_recipm1_alphas_cumprod"][t])
    rst, keep = plan._objective_rows(rec + (w,), torch.device(device)) if (w is not None or pm != "x_start") else (None, [])
    dx0, dnoise, dsc = x0.to(device).contiguous(), noise.to(device).contiguous(), sc.to(device).contiguous()
    ra, rs, rt = _row(a, dx0.device), _row(s, dx0.device), _row(t, dx0.device)
    loss = torch.empty((), dtype=torch.float32, device=dx0.device)
    pred = torch.empty_like(dx0)
    plan.lib.check(plan.lib.dll.ddif_plan_train_step_ex(plan.h, _ptr(dx0), _ptr(dnoise), C.c_void_p(ra.data_ptr()), C.c_void_p(rs.data_ptr()), C.c_void_p(rt.data_ptr()),
                                                        _ptr(dsc), None if rst is None else C.byref(rst), _ptr(loss), _ptr(pred), None, _stream(plan.lib, dx0.device)), "ddif_plan_train_step_ex")
    loss, pred = loss.cpu(), pred.cpu()
    got = {n: g.cpu() for n, g in grads.items()}
    tag = "%s-%s-p2_%g" % (pm, lt, gamma)
    r64, r32 = references(case, kind, masks, paths, tag=tag, objective=objective, extra=(x_t, t))
    return compare(where, case, kind, tag, pred, loss, got, list(grads), r64, r32, paths)


OBJECTIVES = [("noise", "l2", 0.0), ("pred_v", "l1", 0.5), ("x_start", "l1ssim", 0.0)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("pm,lt,gamma", OBJECTIVES, ids=["%s-%s-p2_%g" % o for o in OBJECTIVES])
def test_training_step_under_another_objective_matches_fp64_autograd(backend, pm, lt, gamma):
    dev = _dev(backend)
    run_objective_leg(pm, lt, gamma, str(dev), "emu" if backend == "emu" else "gpu")


# ------------------------------------------------------------------------------------------------ what the 24 x 40 leg found, at the kernel
# csrc/kernels_linattn.h gives every (line, channel quad) of a line group one thread: a group of more than 1024 / C lines left the lines past the 256th pair
# un-normalised.  Only lines shorter than 6 pixels can be that many, and on a square image there are never enough of them: a 3 x 5 level with 256 channels
# (the decoder's first block at 24 x 40), 4 x 8 with 192 or 256, 2 x 16 with 256.  Forward and both backward kernels, against fp64 autograd.
SHORT_LINES = [(1, 3, 5, 256), (2, 5, 3, 256), (1, 4, 8, 192), (2, 8, 4, 192), (1, 2, 16, 256), (1, 16, 2, 160)]


def _la_core(q, kv, heads=8):
    """The attention core of O.linear_attention_mix on NHWC pre-softmax q (B, H, W, C) and kv (B, H, W, 2C)."""
    B, H, W, C = q.shape
    q = q.permute(0, 3, 1, 2).softmax(dim=-2)
    k, v = kv.permute(0, 3, 1, 2).chunk(2, dim=1)
    k = k.softmax(dim=-1)
    d = C // heads
    q = q.reshape(B, heads, d, H * W) * (1.0 / math.sqrt(d))
    ctx = torch.einsum("bhdn,bhen->bhde", k.reshape(B, heads, d, H * W), v.reshape(B, heads, d, H * W))
    return torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(B, C, H, W).permute(0, 2, 3, 1)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", SHORT_LINES, ids=["%dx%dx%dx%d" % s for s in SHORT_LINES])
def test_nhwc_linear_attention_with_many_short_lines(backend, shape):
    import ddif_testops as T

    dev = _dev(backend)
    B, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    q, kv, dout = torch.randn(B, H, W, C, generator=g), torch.randn(B, H, W, 2 * C, generator=g), torch.randn(B, H, W, C, generator=g)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        a, b = q.to(dtype).requires_grad_(True), kv.to(dtype).requires_grad_(True)
        o = _la_core(a, b)
        o.backward(dout.to(dtype))
        ref[dtype] = (o.detach(), a.grad, b.grad)
    out, ws = T.linattn_nhwc(q.to(dev), kv.to(dev))
    dq, dkv = T.linattn_nhwc_backward(q.to(dev), kv.to(dev), dout.to(dev), ws)
    for name, got, r64, r32 in zip(("out", "dq", "dkv"), (out, dq, dkv), ref[torch.float64], ref[torch.float32]):
        e_ref, err = rel(r32, r64), rel(got.cpu(), r64)
        print("%-4s %s e_ref %.3e  err %.3e  ratio %.2f" % (name, shape, e_ref, err, err / e_ref))
        assert err <= MARGIN * e_ref, (name, shape, err, e_ref)
