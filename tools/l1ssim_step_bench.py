"""What training under loss_type="l1ssim" costs (HybridL1SSIM; csrc/kernels_ssimloss.h) against the engine's loss_type="l1".

  1. `step`: the batch-32 training iteration of bench.py's wv3_train_b32 (train_step_into + fused clip / AdamW / EMA, 64 x 64 x 8 tiles) under l1 and under
     l1ssim as a same-process INTERLEAVED pair: l1, l1ssim, l1, l1ssim, ... blocks of `--iters` iterations, each block ended by a device synchronise, so that
     clock and thermal drift hit both alike; the median of the rounds is reported.  The self-conditioning draw is pinned off: every iteration is one forward
     and one backward pass.  The `l1` leg is THIS build under the default objective, not a library built from the parent commit (`baseline` says so); under
     that objective this build issues the parent's launches with the parent's bits (tests/test_l1ssim_gpu.py test_default_path_is_untouched).
  2. `tail`: the three launches alone -- ssim_stats_kernel, ssim_final_kernel, ssim_grad_kernel on NHWC tensors of the same size -- under
     `rocprofv3 --kernel-trace --stats`, in a run of its own; the per-kernel averages are read from its kernel_stats.csv.

The parent process never touches the GPU: each part is a child process of its own under its own time limit, and the second starts only if the first ended
well.

    python tools/l1ssim_step_bench.py [--batch 32] [--rounds 7] [--iters 10] [--out DIR]        prints one JSON line; DIR keeps the rocprofv3 files (default: a temporary directory)"""
import argparse
import csv
import glob
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dif-pan_amd"), ROOT]
STEP_LIMIT_S, TAIL_LIMIT_S = 420, 300


def part_step(args):
    import torch

    from ddif import runtime
    from ddif.diffusion import diffusion_ddpm_pan as M
    from ddif.diffusion_engine import gradient_bucket
    from ddif.layout import engine_cfg
    from ddif.models.sr3_dwt import UNetSR3
    from ddif.synth import synth_state_dict, synth_tiles

    dev = torch.device("cuda:0")
    C, P, B, H, T = 8, 1, args.batch, 64, 3000
    cfg = engine_cfg(C, P)
    keys = ("in_channel", "out_channel", "inner_channel", "lms_channel", "pan_channel", "norm_groups", "channel_mults", "attn_res", "res_blocks", "dropout",
            "image_size", "self_condition")
    net = UNetSR3(**{k: cfg[k] for k in keys})
    net.load_state_dict(synth_state_dict(cfg, 1234))
    net = net.to(dev).train()
    d = M.GaussianDiffusion(net, image_size=H, channels=C, pred_mode="x_start", loss_type="l1", device=dev, clamp_range=(0, 1))
    d.set_new_noise_schedule(betas=M.make_beta_schedule("cosine", T, cosine_s=8e-3), device=dev)
    tiles = synth_tiles(B, C, P, H, H, seed=100)
    cond = tiles["cond"].to(dev)
    res = (tiles["gt"].to(dev) - cond[:, :C]).contiguous()
    params = [p for p in net.parameters()]
    _, grads = gradient_bucket(params)
    for p, g in zip(params, grads):
        p.grad = g
    ema = [p.detach().clone() for p in params]
    opt = runtime.FusedAdamW(params, grads, ema, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    torch.manual_seed(7)
    random.seed(7)
    M.random.random = lambda: 1.0  # no self-conditioning pass: every iteration is the same work

    def block(loss_type, n):
        d.loss_type = loss_type  # the training step reads it when it states the plan's objective
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss, _ = d.train_step_into(res, cond, grads)
            opt.step(max_grad_norm=0.003, ema_mode=1, ema_decay=0.995)
            net.mark_weights_dirty()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n, float(loss)

    last = {}
    for lt in ("l1", "l1ssim"):  # plans, scratch, clocks
        block(lt, 3)
    ms = {"l1": [], "l1ssim": []}
    for _ in range(args.rounds):
        for lt in ("l1", "l1ssim"):
            t, last[lt] = block(lt, args.iters)
            ms[lt].append(t)
    plan = net.plan_for(B, H, H, dev, train=True)
    assert plan.get_objective() == ("x_start", "l1ssim")
    out = dict(baseline="this build under the default objective (x_start, l1), not a build of the parent commit", batch=B, tile=[H, H, C], rounds=args.rounds,
               iters_per_block=args.iters, iter_ms_l1=statistics.median(ms["l1"]), iter_ms_l1ssim=statistics.median(ms["l1ssim"]),
               iter_ms_l1_all=[round(v, 4) for v in ms["l1"]], iter_ms_l1ssim_all=[round(v, 4) for v in ms["l1ssim"]], last_loss=last)
    out["overhead_ms"] = out["iter_ms_l1ssim"] - out["iter_ms_l1"]
    out["overhead_pct"] = 100.0 * out["overhead_ms"] / out["iter_ms_l1"]
    print(json.dumps(out))


def part_tail(args):
    import torch

    from ddif import runtime

    dev = torch.device("cuda:0")
    B, H, C = args.batch, 64, 8
    g = torch.Generator().manual_seed(3)
    x = (0.05 * torch.randn(B, H, H, C, generator=g)).to(dev)
    y = (x.cpu() + 0.02 * torch.randn(B, H, H, C, generator=g)).to(dev)
    for _ in range(args.tail_calls):
        runtime.l1ssim_loss(x, y, grad=True, nhwc=True)
    torch.cuda.synchronize()
    print(json.dumps(dict(calls=args.tail_calls)))


def run_child(cmd, limit):
    """One GPU step under its own time limit; (ok, stdout).  A step that fails or runs out of time ends the measurement: nothing else is started."""
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        return False, f"time limit of {limit} s"
    if r.returncode != 0:
        return False, f"exit status {r.returncode}: {r.stderr[-2000:]}"
    return True, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--tail-calls", type=int, default=40)
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", choices=("step", "tail"), default=None, help="(internal) run one part in this process")
    args = ap.parse_args()
    if args.part == "step":
        return part_step(args)
    if args.part == "tail":
        return part_tail(args)
    me = [sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--rounds", str(args.rounds), "--iters", str(args.iters), "--tail-calls", str(args.tail_calls)]
    if args.out is None:
        args.out = tempfile.mkdtemp(prefix="l1ssim_bench_")
    os.makedirs(args.out, exist_ok=True)
    ok, text = run_child(me + ["--part", "step"], STEP_LIMIT_S)
    if not ok:
        print(json.dumps(dict(error="step: " + text)))
        return 1
    res = json.loads(text.strip().splitlines()[-1])
    prof = os.path.join(args.out, "tail_prof")
    ok, text = run_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "p", "--"] + me + ["--part", "tail"], TAIL_LIMIT_S)
    if not ok:
        res["tail_error"] = text
        print(json.dumps(res))
        return 1
    tail = {}
    for f in glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            for k in ("ssim_stats_kernel", "ssim_final_kernel", "ssim_grad_kernel"):
                if k in r["Name"]:
                    tail[k + "_us"] = float(r["AverageNs"]) / 1e3
                    tail[k + "_calls"] = int(r["Calls"])
    if len(tail) == 6:
        tail["tail_us"] = sum(tail[k + "_us"] for k in ("ssim_stats_kernel", "ssim_final_kernel", "ssim_grad_kernel"))
        tail["tail_pct_of_l1_iteration"] = 100.0 * tail["tail_us"] / (1e3 * res["iter_ms_l1"])
    res["tail"] = tail
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
