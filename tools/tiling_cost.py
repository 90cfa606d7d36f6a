"""What per-step tile fusion costs (ddif_plan_set_tiling; csrc/kernels_tiling.h): ms per DDPM step of the engine's WV3 configuration, B = 64 tiles of
64 x 64 x 8, T = 100, device noise, as

    untiled   tiling off: the update runs in the final conv's sampler epilogue (no tail launches)
    tail      tiling on at overlap 0 (8 x 8 tiles of a 512 x 512 scene): the unfused tail -- update kernel, counter -- and nothing to fuse
    tiled     tiling on, 8 x 8 grid with overlap 16 (a 400 x 400 scene): the unfused tail + tile_fuse_kernel

Every leg runs in a CHILD process of its own (this process never touches the GPU), and the legs are interleaved round by round -- A, B, C, A, B, C, ... -- so
that clock and thermal drift hit all alike; the median over the rounds is reported.  `--baseline-tree DIR` adds the `untiled` leg of ANOTHER built checkout
(the parent commit: its own package and its own lib/libddif.so), which is the honest A of the A/B: boxes differ by +-5 %, only a same-box pair means anything.

    python tools/tiling_cost.py [--baseline-tree DIR] [--rounds 5] [--T 100]        prints one JSON line"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {"untiled": None, "tail": (1, 512, 512, 0), "tiled": (1, 400, 400, 16)}


def leg(tree, mode, T, reps):
    sys.path[:0] = [os.path.join(tree, "dif-pan_amd"), tree]
    import torch

    from ddif.diffusion.diffusion_ddpm_pan import GaussianDiffusion, make_beta_schedule
    from ddif.layout import engine_cfg
    from ddif.models.sr3_dwt import UNetSR3
    from ddif.synth import synth_state_dict, synth_tiles

    dev = torch.device("cuda:0")
    cfg = engine_cfg(8, 1)
    keys = ("in_channel", "out_channel", "inner_channel", "lms_channel", "pan_channel", "norm_groups", "channel_mults", "attn_res", "res_blocks", "dropout",
            "image_size", "self_condition")
    net = UNetSR3(**{k: cfg[k] for k in keys})
    net.load_state_dict(synth_state_dict(cfg, 1234))
    net = net.to(dev).eval()
    B, H = 64, 64
    cond = synth_tiles(B, 8, 1, H, H, seed=100)["cond"].to(dev)  # (timing only: the tiles need not be cut from one scene)
    d = GaussianDiffusion(net, image_size=H, channels=8, pred_mode="x_start", loss_type="l1", device=dev, clamp_range=(0, 1))
    d.set_new_noise_schedule(betas=make_beta_schedule("cosine", T, cosine_s=8e-3), device=dev)
    kw = {} if LEGS[mode] is None else {"tiling": LEGS[mode]}

    def loop():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        d(cond, mode="ddpm_sample", seed=7, device_rng=True, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / T

    loop()  # plan, captured pair, clocks
    ms = [loop() for _ in range(reps)]
    plan = d._plan(cond, **kw)
    print(json.dumps(dict(ms=ms, launches=plan.num_launches()["step"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--leg", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg[0], args.leg[1], args.T, args.reps)
    legs = [("this", ROOT, m) for m in LEGS]
    if args.baseline_tree:
        legs.insert(0, ("baseline", os.path.abspath(args.baseline_tree), "untiled"))
    ms = {f"{w}_{m}": [] for w, _, m in legs}
    launches = {}
    for _ in range(args.rounds):
        for w, tree, m in legs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", tree, m, "--T", str(args.T), "--reps", str(args.reps)], capture_output=True, text=True,
                               timeout=300)
            if r.returncode != 0:
                sys.stderr.write(r.stderr)
                raise SystemExit(f"leg {w} {m} failed with status {r.returncode}")
            out = json.loads(r.stdout.strip().splitlines()[-1])
            ms[f"{w}_{m}"] += out["ms"]
            launches[f"{w}_{m}"] = out["launches"]
    res = dict(batch=64, tile=64, channels=8, T=args.T, rounds=args.rounds, reps=args.reps, step_ms={k: round(statistics.median(v), 4) for k, v in ms.items()},
               step_ms_min_max={k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()}, launches_per_step=launches)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
