"""Stage-level parity: every attention stage of an inference plan against the fp64 oracle ON THE KERNEL'S OWN INPUT.

Why not end to end: on the seeded weights of ddif/synth.py the bottleneck self-attention is near uniform (largest probability 0.02 of 64 keys), and the GroupNorms and
~30 layers behind it damp even a wholly wrong attention (uniform softmax, keys rolled by one, scale 1/sqrt(d), transposed scores) to < 1e-5 at the network output --
half the 2e-5 tolerance of the forward goldens.  So the kernels are checked where they write: the plan builder notes stage taps (include/ddif_testops.h
ddif_plan_tap_info), one eager forward copies the tapped tensors out (ddif_plan_forward_taps), and for

  * every SelfAttention site        "<block>.attn.in" -> "<block>.attn.out"            attn_block_kernel (64 tokens) / qkv conv + self_attn_mfma_kernel + out conv
  * every FastAttnCondInjection     "<ci>.cur", "<ci>.skip", "<ci>.cond" -> "<ci>.a"   linattn_fused_kernel / linattn8_fused_kernel / the three-launch path

the oracle's stage (O.self_attention, O.linear_attention_mix) runs in fp64 on the LIBRARY's tapped input and is compared with the library's tapped output.
Nothing upstream or downstream takes part, so nothing damps or amplifies.

Weights: the fixture state dict (near-uniform regime) and a stressed one: q and k rows x 5 in every attn.qkv.weight, cond_inj.q.1 / kv.1 weight and bias x 3.

Bound (per stage, nothing fixed in advance): e_ref = max|fp32 oracle stage - fp64 oracle stage| / max|fp64 stage output| on the same tapped input; the library may
differ from fp64 by at most MARGIN = 16 x e_ref: 4 for the split operands (f16x2 / bf16x3: 22 operand bits against 24) x 4 for accumulation order (the fp64 GroupNorm
partials only help).  Every stage prints  e_ref, the library's error and their ratio; DDIF_STAGE_PARITY_TABLE=<file> appends the rows there (profiles/stage_parity.txt
is such a file from an MI355X run).

CPU-only checks keep a weak input from hiding a failure: the conditions on the 64-token score matrices (test_stressed_inputs_...) and, per site, the distance every
mutation of the fp64 stage moves the stage output -- at least 50 x the site's bound (test_mutations_...): a kernel with one of these faults cannot pass.

Cases (one forward each): see CASES.  The per-process switches (DDIF_ATTN_NW, DDIF_ATTN_SPLIT, DDIF_ATTN_F16, DDIF_LAFUSE, DDIF_LA8, DDIF_LA6, DDIF_LA_NW) run the
wv3 64 x 64 case of this file in a fresh child process each: tests/test_env_switches.py::test_attention_stages_under_switch."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

import golden_cases as gc
from ddif_testlib import CTOR_KEYS, use_emulator, use_gpu_library
from oracle import ddif_oracle as O

MARGIN = 16.0       # library error <= MARGIN x e_ref   (4: split operands, 22 of 24 bits; 4: accumulation order)
SENSITIVITY = 50.0  # every mutation moves the stage output by >= SENSITIVITY x MARGIN x e_ref

# id -> (data set, B, H, W, grid cap, runs on the emulator)
CASES = {
    # 64-token attn_block_kernel in its default form (4 workgroups per sample, f16x2 qkv); linattn_fused at 64^2 / 32^2 / 16^2; linattn8_fused with 256- / 192-channel inputs
    "wv3_64_b2": ("wv3", 2, 64, 64, 0, True),
    # the same kernels with their grids capped to 3 workgroups: each walks several samples / query parts / strips (sample and part strides)
    "wv3_64_b3_cap3": ("wv3", 3, 64, 64, 3, False),
    # 16 tokens on the generic self_attn_mfma_kernel; C = 4 cond widths in the kv convs
    "gf2_32_b2": ("gf2", 2, 32, 32, 0, True),
    # 15 tokens: a partial tile, odd count, H != W -- row and column softmax lengths differ, an axis mix-up cannot cancel
    "wv3_24x40_b1": ("wv3", 1, 24, 40, 0, True),
    # 256 tokens: several 64-query tiles per head in the generic kernel; 16^2 bottleneck-level linear attention  (GPU only: minutes on the emulator)
    "cave_128_b1": ("cave", 1, 128, 128, 0, False),
}
EMU_CASES = [c for c, v in CASES.items() if v[5]]
# the emulator runs a 64 x 64 forward in tens of seconds: one such leg (stressed weights), both weight sets at the small sizes
EMU_LEGS = [(c, w) for c in EMU_CASES for w in ("stressed", "fixture") if not (c == "wv3_64_b2" and w == "fixture")]

SA_MUTATIONS = ("uniform_softmax", "keys_rolled", "scale_sqrt_d", "scores_transposed", "head_k_from_neighbour")
LA_MUTATIONS = ("softmax_axes_swapped", "k_softmax_uniform", "head_k_from_neighbour")

# Stages a case's tap list may lack, by name, with the reason.  None: every layer output is a chain tensor or a skip connection and is written to memory -- also by
# the convs that carry the next block's x_conv + FiLM as a SECOND output (EPI_XF), and by ups.<last>, which the final conv reads; only the network output itself may
# stay unwritten (sampler epilogue), and that is no stage.  No self-attention site and no decoder linear-attention site may ever be listed here.
ABSENT = {}


# ------------------------------------------------------------------------------------------------ weights, inputs
_sd_cache = {}


def weights(ds, kind, dtype=torch.float32):
    key = (ds, kind, dtype)
    if key not in _sd_cache:
        sd = {k: v.clone() for k, v in gc.weights_for(ds).items()}
        if kind == "stressed":
            for k in sd:
                if k.endswith("attn.qkv.weight"):  # (3C, C, 1, 1), per-head [q | k | v] interleave over 8 heads: q and k rows x 5
                    w = sd[k].view(8, 3, sd[k].shape[0] // 24, -1)
                    w[:, :2] *= 5.0
                elif ".cond_inj.q.1." in k or ".cond_inj.kv.1." in k:
                    sd[k] *= 3.0
        else:
            assert kind == "fixture"
        _sd_cache[key] = {k: v.to(dtype) for k, v in sd.items()}
    return _sd_cache[key]


def inputs(case):
    ds, B, H, W = CASES[case][:4]
    C = gc.DATASETS[ds][0]
    seed = gc.zlib_seed("stage_" + case)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    sc = torch.randn(B, C, H, W, generator=g)
    t = torch.tensor([5, 700, 321][:B], dtype=torch.long)
    cond = gc.tiles_for(ds, B, H, W, seed=seed % 1000)["cond"]
    return x, t, cond, sc


def sites(ds):
    """(self-attention prefixes, decoder cond_inj prefixes, layer prefixes) of the engine network, from the oracle's layer list."""
    plan = O.layer_plan(gc.cfg_for(ds))
    sa, la, layers = [], [], []
    for grp in ("downs", "mid", "ups"):
        for i, L in enumerate(plan[grp]):
            p = "%s.%d" % (grp, i)
            layers.append(p)
            if L.get("attn"):
                sa.append(p + ".attn")
            if L["kind"] == "dec":
                la.append(p + ".cond_inj")
    return sa, la, layers


# ------------------------------------------------------------------------------------------------ the two stages, with the mutations of the sensitivity check
def sa_stage(sd, p, x, mut=None, n_head=8):
    """O.self_attention restated with hooks for the mutations (mut=None is checked against the oracle itself)."""
    B, C, H, W = x.shape
    d, N = C // n_head, H * W
    qkv = F.conv2d(O._gn(x, sd, p + ".norm", 1), sd[p + ".qkv.weight"]).view(B, n_head, 3 * d, N)
    q, k, v = qkv[:, :, :d], qkv[:, :, d:2 * d], qkv[:, :, 2 * d:]
    if mut == "head_k_from_neighbour":
        k = k.clone()
        k[:, 3] = qkv[:, 4, d:2 * d]
    s = torch.einsum("bncp,bncq->bnpq", q, k) / math.sqrt(d if mut == "scale_sqrt_d" else C)
    if mut == "scores_transposed":
        s = s.transpose(-1, -2)
    a = torch.softmax(s, dim=-1)
    if mut == "uniform_softmax":
        a = torch.full_like(a, 1.0 / N)
    if mut == "keys_rolled":
        a = a.roll(1, dims=-1)
    o = torch.einsum("bnpq,bncq->bncp", a, v).reshape(B, C, H, W)
    return F.conv2d(o, sd[p + ".out.weight"], sd[p + ".out.bias"]) + x


def la_stage(sd, p, x, cL, mut=None, heads=8):
    """O.linear_attention_mix restated with hooks for the mutations."""
    B, Cf, H, W = x.shape
    xn = O._gn(x, sd, p + ".prenorm_x", 1)
    q = F.conv2d(F.conv2d(xn, sd[p + ".q.0.weight"], None, padding=1, groups=Cf), sd[p + ".q.1.weight"], sd[p + ".q.1.bias"])
    kv = F.conv2d(F.conv2d(cL, sd[p + ".kv.0.weight"], None, padding=1, groups=cL.shape[1]), sd[p + ".kv.1.weight"], sd[p + ".kv.1.bias"])
    k, v = kv.chunk(2, dim=1)
    swap = mut == "softmax_axes_swapped"
    q = q.softmax(dim=-1 if swap else -2)
    k = k.softmax(dim=-2 if swap else -1)
    if mut == "k_softmax_uniform":
        k = torch.full_like(k, 1.0 / W)
    qd = q.shape[1]
    d = qd // heads
    q = q.reshape(B, heads, d, H * W) * (1.0 / math.sqrt(d))
    k = k.reshape(B, heads, d, H * W)
    v = v.reshape(B, heads, d, H * W)
    if mut == "head_k_from_neighbour":
        k = k.clone()
        k[:, 3] = k[:, 4].clone()
    ctx = torch.einsum("bhdn,bhen->bhde", k, v)
    o = torch.einsum("bhde,bhdn->bhen", ctx, q).reshape(B, qd, H, W)
    a = F.conv2d(o, sd[p + ".attn_out.weight"], sd[p + ".attn_out.bias"])
    if (p + ".attn_res.weight") in sd:
        return a + F.conv2d(xn, sd[p + ".attn_res.weight"], sd[p + ".attn_res.bias"])
    return a + xn


def rel(a, b):
    """max|a - b| relative to the largest absolute value of the stage output b."""
    return float((a.double() - b.double()).abs().max()) / float(b.double().abs().max())


def stage_refs(ds, kind, p, ins):
    """(fp64 stage output, e_ref) of one site on fp32 inputs `ins` (x,) or (x, cL)."""
    sd32, sd64 = weights(ds, kind), weights(ds, kind, torch.float64)
    with torch.no_grad():
        if len(ins) == 1:
            r64 = O.self_attention(sd64, p, ins[0].double(), 1)
            r32 = O.self_attention(sd32, p, ins[0], 1)
        else:
            r64 = O.linear_attention_mix(sd64, p, ins[0].double(), ins[1].double(), 1)
            r32 = O.linear_attention_mix(sd32, p, ins[0], ins[1], 1)
    return r64, rel(r32, r64)


# ------------------------------------------------------------------------------------------------ CPU only: the oracle's own stage inputs
_oracle_cache = {}


def oracle_run(case, kind, dtype):
    """One oracle forward in `dtype` that also keeps the input(s) of every attention stage: (image, {site: (x,) | (x, cL)})."""
    key = (case, kind, dtype)
    if key not in _oracle_cache:
        ds = CASES[case][0]
        sd = weights(ds, kind, dtype)
        x, t, cond, sc = inputs(case)
        seen = {}
        sa0, la0 = O.self_attention, O.fast_attn_cond_injection

        def sa(sd_, p, xx, groups, n_head=8):
            seen[p] = (xx.detach().clone(),)
            return sa0(sd_, p, xx, groups, n_head)

        def la(sd_, p, xx, cL, groups, heads=8, path_scale=None):
            seen[p] = (xx.detach().clone(), cL.detach().clone())
            return la0(sd_, p, xx, cL, groups, heads, path_scale)

        O.self_attention, O.fast_attn_cond_injection = sa, la
        try:
            with torch.no_grad():
                y = O.unet_forward(sd, gc.cfg_for(ds), x.to(dtype), t.to(dtype), cond.to(dtype), sc.to(dtype))
        finally:
            O.self_attention, O.fast_attn_cond_injection = sa0, la0
        _oracle_cache[key] = (y, seen)
    return _oracle_cache[key]


def test_stage_functions_restate_the_oracle():
    """The mutation-capable stage functions of this file with mut=None ARE the oracle's stages (same operations in the same order: equal to the last bit)."""
    _, seen = oracle_run("gf2_32_b2", "stressed", torch.float64)
    sd = weights("gf2", "stressed", torch.float64)
    sa, la, _ = sites("gf2")
    assert sorted(seen) == sorted(sa + la)
    with torch.no_grad():
        for p in sa:
            assert torch.equal(sa_stage(sd, p, *seen[p]), O.self_attention(sd, p, seen[p][0], 1)), p
        for p in la:
            assert torch.equal(la_stage(sd, p, *seen[p]), O.linear_attention_mix(sd, p, seen[p][0], seen[p][1], 1)), p
            # ... and the split of fast_attn_cond_injection left the whole block what it was: a + ffn(a)
            a = O.linear_attention_mix(sd, p, *seen[p], 1)
            f = F.conv2d(a, sd[p + ".ffn.0.weight"], None, padding=1)
            f = F.conv2d(F.conv2d(F.silu(f), sd[p + ".ffn.2.weight"], None, padding=1), sd[p + ".ffn.3.weight"], sd[p + ".ffn.3.bias"])
            assert torch.equal(O.fast_attn_cond_injection(sd, p, *seen[p], 1), f + a), p


def test_stressed_inputs_are_peaked_but_well_conditioned_at_the_64_token_sites():
    """Conditions on the inputs of the wv3 64 x 64 case, so that a weak input cannot hide a failure: at every 64-token site the largest softmax probability is
    >= 0.3 (fixture weights: 0.02 -- any key permutation is invisible), no score row spreads over more than 40 (exp() stays far from fp32 underflow), and the
    fp32 and fp64 oracles still agree on the final image to 5e-6 (the stress has not made the network chaotic: a reference exists)."""
    case, ds = "wv3_64_b2", "wv3"
    y64, seen = oracle_run(case, "stressed", torch.float64)
    y32, _ = oracle_run(case, "stressed", torch.float32)
    sd = weights(ds, "stressed", torch.float64)
    sa, _, _ = sites(ds)
    assert len(sa) == 8
    peak = {}
    for p in sa:
        (x,) = seen[p]
        B, C, H, W = x.shape
        assert H * W == 64
        qkv = F.conv2d(O._gn(x, sd, p + ".norm", 1), sd[p + ".qkv.weight"]).view(B, 8, 3 * (C // 8), 64)
        d = C // 8
        s = torch.einsum("bncp,bncq->bnpq", qkv[:, :, :d], qkv[:, :, d:2 * d]) / math.sqrt(C)
        pmax = float(torch.softmax(s, -1).max())
        spread = float((s.max(-1).values - s.min(-1).values).max())
        print("%-28s largest probability %.3f  largest row spread %.2f" % (p, pmax, spread))
        peak[p] = pmax
        assert spread <= 40.0, (p, spread)
    # 0.39 - 0.67 at the four encoder / middle sites.  The four decoder sites stay flatter under the same gain (0.05 - 0.09 against the fixture's 0.02); what each
    # site's input is worth is measured site by site in test_mutations_move_every_stage_far_beyond_its_bound (every mutation: > 50 x the bound there too)
    assert max(peak.values()) >= 0.3, peak
    assert all(peak[p] >= 0.3 for p in ("downs.13.attn", "downs.14.attn", "downs.15.attn", "mid.0.attn")), peak
    diff = float((y32.double() - y64).abs().max())
    print("fp32 oracle vs fp64 oracle, final image: %.3e" % diff)
    assert diff <= 5e-6, diff


@pytest.mark.parametrize("case", [c for c in CASES if c != "wv3_64_b3_cap3"])  # (the capped case has the sites and weights of wv3_64_b2)
def test_mutations_move_every_stage_far_beyond_its_bound(case):
    """No library involved.  For every site, on the fp64 oracle's own stage input: each mutation of the fp64 stage (the faults an end-to-end test cannot see) moves
    the stage output by at least SENSITIVITY x the bound the library leg uses for that site (MARGIN x e_ref).  This is what proves the parity legs can fail."""
    ds = CASES[case][0]
    _, seen = oracle_run(case, "stressed", torch.float64)
    sd = weights(ds, "stressed", torch.float64)
    sa, la, _ = sites(ds)
    weak = []
    with torch.no_grad():
        for p in sa + la:
            ins = tuple(t.float() for t in seen[p])  # what a library stage would be handed: fp32 tensors
            r64, e_ref = stage_refs(ds, "stressed", p, ins)
            bound = MARGIN * e_ref
            for mut in (SA_MUTATIONS if p in sa else LA_MUTATIONS):
                ins64 = tuple(t.double() for t in ins)
                moved = rel(sa_stage(sd, p, *ins64, mut=mut) if p in sa else la_stage(sd, p, *ins64, mut=mut), r64)
                print("%-14s %-24s %-22s e_ref %.2e  moved %.2e = %7.0f x bound" % (case, p, mut, e_ref, moved, moved / bound))
                if moved < SENSITIVITY * bound:
                    weak.append((p, mut, moved, bound))
    assert not weak, weak


# ------------------------------------------------------------------------------------------------ library legs
_SWITCHES = ("DDIF_ATTN_NW", "DDIF_ATTN_SPLIT", "DDIF_ATTN_F16", "DDIF_LAFUSE", "DDIF_LA8", "DDIF_LA6", "DDIF_LA_NW")


def _make_net(ds, kind, device):
    from ddif.models.sr3_dwt import UNetSR3

    cfg = gc.cfg_for(ds)
    net = UNetSR3(**{k: cfg[k] for k in CTOR_KEYS})
    net.load_state_dict(weights(ds, kind))
    return net.to(device).eval()


def run_library_leg(case, kind, device, where):
    """One tapped forward of `case` on the loaded library; every attention stage against the fp64 oracle on the tapped input.  Returns the table rows."""
    import ddif_testops as T
    from ddif import runtime

    ds, B, H, W, cap, _ = CASES[case]
    x, t, cond, sc = inputs(case)
    sa, la, layers = sites(ds)
    net = _make_net(ds, kind, device)
    try:
        runtime.set_debug_grid_cap(cap)
        plan = net.plan_for(B, H, W, torch.device(device))
    finally:
        runtime.set_debug_grid_cap(0)
    taps = T.plan_taps(plan)
    names = [n for n, *_ in taps]
    want = set(layers) | {p + s for p in sa for s in (".in", ".out")} | {p + s for p in la for s in (".cur", ".skip", ".cond", ".a", ".out")}
    assert set(names) == want - set(ABSENT) and len(names) == len(set(names)), sorted(set(names) ^ want)
    before = plan.num_launches()
    plan.set_cond(cond.to(device), force=True)
    need = [p + s for p in sa for s in (".in", ".out")] + [p + s for p in la for s in (".cur", ".skip", ".cond", ".a", ".out")] + [layers[-1]]
    y, got = T.plan_forward_taps(plan, x.to(device), t, sc.to(device), need)
    assert plan.num_launches() == before
    if where == "gpu" or H * W < 4096:  # the tapped forward is the plain forward: same launches on the same buffers (a second 64 x 64 forward costs the emulator 17 s)
        assert torch.equal(y, plan.forward(x.to(device), t, sc.to(device)))
    got = {k: v.cpu() for k, v in got.items()}
    switches = " ".join("%s=%s" % (k[5:], os.environ[k]) for k in _SWITCHES if k in os.environ) or "-"
    rows, bad = [], []
    for p in sa + la:
        if p in sa:
            ins, out = (got[p + ".in"],), got[p + ".out"]
        else:
            ins, out = (torch.cat([got[p + ".cur"], got[p + ".skip"]], dim=1), got[p + ".cond"]), got[p + ".a"]
        assert all(bool(torch.isfinite(v).all()) for v in ins + (out,)), p
        r64, e_ref = stage_refs(ds, kind, p, ins)
        err = rel(out, r64)
        row = "%-5s %-15s %-9s %-22s %-26s %4dx%-3d %4d  e_ref %.3e  err %.3e  ratio %6.2f" % (
            where, case, kind, switches, p, ins[0].shape[2], ins[0].shape[3], ins[0].shape[1], e_ref, err, err / e_ref)
        rows.append(row)
        print(row)
        if not err <= MARGIN * e_ref:
            bad.append(row)
    path = os.environ.get("DDIF_STAGE_PARITY_TABLE")
    if path:
        with open(path, "a") as f:
            f.write("\n".join(rows) + "\n")
    assert not bad, "\n" + "\n".join(bad)
    return rows


@pytest.mark.parametrize("case,kind", EMU_LEGS, ids=["%s-%s" % ck for ck in EMU_LEGS])
def test_stages_match_the_fp64_oracle_on_the_emulator(case, kind):
    lib = use_emulator()
    assert lib.emulated
    run_library_leg(case, kind, "cpu", "emu")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["stressed", "fixture"])
@pytest.mark.parametrize("case", list(CASES))
def test_stages_match_the_fp64_oracle_on_the_gpu(case, kind):
    use_gpu_library()
    run_library_leg(case, kind, "cuda:0", "gpu")
