"""What a classifier-free-guided DPM-Solver run costs (ddif_plan_sample_dpm_guided) next to an unguided run of twice as many tiles (ddif_plan_sample_dpm).

The GF2 scene of the benchmark (64 x 64 x 4 tiles, cosine schedule, T = 1000, image-space clamp corrector), multistep order 2 with solver_type="taylor" so that
BOTH legs are solver programs with one launch behind each network evaluation: guided at Bg tiles (the network's batch is 2 * Bg: [unconditional; conditional])
against unguided at B = 2 * Bg tiles -- the same plan batch, the same launch count, the same network work.  One process, the two legs INTERLEAVED (unguided,
guided, unguided, guided, ...) so that clock and thermal drift hit both alike.  Expectation: equal time; the guided evaluation launch reads two network halves
and writes two state halves for each item where the unguided one reads and writes one of each -- the same bytes.  A record, not a threshold: read the
same-process ratio only.

    python tools/cfg_bench.py [--guided-batch 32] [--nfe 20] [--rounds 7] [--scale 1.5]        prints one JSON line"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dif-pan_amd"), ROOT]
import torch  # noqa: E402

from ddif.diffusion.diffusion_ddpm_pan import make_beta_schedule  # noqa: E402
from ddif.layout import engine_cfg  # noqa: E402
from ddif.models.sr3_dwt import UNetSR3  # noqa: E402
from ddif.solver.dpm_solver import DPM_Solver, ImageSpaceClamp, NoiseScheduleVP, model_wrapper  # noqa: E402
from ddif.synth import synth_state_dict, synth_tiles  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--guided-batch", type=int, default=32)
    ap.add_argument("--nfe", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.5)
    args = ap.parse_args()
    assert args.rounds >= 3 and args.scale != 1.0
    dev = torch.device("cuda:0")
    C_, H, T = 4, 64, 1000
    cfg = engine_cfg(C_, 1)
    keys = ("in_channel", "out_channel", "inner_channel", "lms_channel", "pan_channel", "norm_groups", "channel_mults", "attn_res", "res_blocks", "dropout",
            "image_size", "self_condition")
    net = UNetSR3(**{k: cfg[k] for k in keys})
    net.load_state_dict(synth_state_dict(cfg, 1234))
    net = net.to(dev).eval()
    Bg = args.guided_batch
    B = 2 * Bg
    cond = synth_tiles(B, C_, 1, H, H, seed=100)["cond"].to(dev)
    ns = NoiseScheduleVP("discrete", betas=torch.as_tensor(make_beta_schedule("cosine", T, cosine_s=8e-3)).float())
    xT = torch.randn(B, C_, H, H, device=dev)

    def solver(c, scale, uncond):
        fn = model_wrapper(net, ns, model_type="noise", guidance_type="classifier-free", guidance_scale=scale, condition=c, unconditional_condition=uncond)
        slv = DPM_Solver(fn, ns, algorithm_type="dpmsolver++", correcting_x0_fn=ImageSpaceClamp(c[:, :C_].contiguous(), 0.0, 1.0))
        assert slv._fused_target() is not None and (slv._guidance() is None) == (uncond is None)
        return slv
    cg = cond[:Bg].contiguous()
    ug = cg.clone()
    ug[:, C_:] = 0  # the lms channels kept, no PAN
    legs = dict(unguided=(solver(cond, 1.0, None), xT), guided=(solver(cg, args.scale, ug), xT[:Bg].contiguous()))

    def run(leg):
        slv, x = legs[leg]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = slv.sample(x, steps=args.nfe, order=2, skip_type="time_uniform", method="multistep", solver_type="taylor")
        torch.cuda.synchronize()
        assert out.shape == x.shape and bool(torch.isfinite(out).all())
        return 1e3 * (time.perf_counter() - t0)

    for leg in legs:  # plans, clocks
        run(leg)
        run(leg)
    ms = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            ms[leg].append(run(leg))
    med = {leg: statistics.median(v) for leg, v in ms.items()}
    res = dict(baseline="the unguided leg of this build at the same plan batch (ddif_plan_sample_dpm), not a build of the parent commit", guided_tiles=Bg, unguided_tiles=B,
               plan_batch=B, tile=H, nfe=args.nfe, rounds=args.rounds, guidance_scale=args.scale, run_ms_unguided=med["unguided"], run_ms_guided=med["guided"],
               run_ms_unguided_all=[round(v, 3) for v in ms["unguided"]], run_ms_guided_all=[round(v, 3) for v in ms["guided"]],
               eval_ms_unguided=med["unguided"] / args.nfe, eval_ms_guided=med["guided"] / args.nfe,
               guided_over_unguided_pct=100.0 * (med["guided"] - med["unguided"]) / med["unguided"],
               guided_inside_unguided_spread=bool(min(ms["unguided"]) <= med["guided"] <= max(ms["unguided"])))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
