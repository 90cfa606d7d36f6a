#!/usr/bin/env python3
"""Time of ddif_q2n next to ddif_metrics on the GPU, same process, same inputs (the figures of DESIGN.md "Q2n"):

    python tools/q2n_bench.py [--iters 2000] [--out q2n_bench.json]

Shapes: (B = 64, C = 8, 64 x 64), a validation batch of WV3 tiles, and (B = 1, C = 8, 512 x 512), one full scene.  Integer-valued random counts in
[0, 2047]; each call is warmed up, then `iters` back-to-back calls are timed with device events in three windows (the median is reported).  Needs a
GPU: there is nothing to fall back to."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dif-pan_amd"))
from ddif import runtime  # noqa: E402


def timed(fn, iters):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        windows.append(e0.elapsed_time(e1) * 1e3 / iters)
    return sorted(windows)[1], windows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "q2n_bench needs a GPU"
    dev = torch.device("cuda:0")
    lib = runtime.get_lib()
    assert not lib.emulated
    rows = []
    for B, C, H in ((64, 8, 64), (1, 8, 512)):
        g = torch.Generator().manual_seed(B)
        gt = torch.randint(0, 2048, (B, C, H, H), generator=g).float().to(dev)
        pred = (gt + torch.randint(-30, 31, (B, C, H, H), generator=g).float().to(dev)).clamp_(0, 2047)
        q_us, q_w = timed(lambda: runtime.q2n(gt, pred, 1.0, 32, 32), args.iters)
        m_us, m_w = timed(lambda: runtime.metrics(gt, pred, 4.0), args.iters)
        row = dict(B=B, C=C, H=H, W=H, q2n_us=q_us, metrics_us=m_us, q2n_windows_us=q_w, metrics_windows_us=m_w,
                   q2n_mean=float(runtime.q2n(gt, pred, 1.0, 32, 32).mean()))
        print(json.dumps(row))
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
