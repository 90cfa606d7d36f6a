"""What a singlestep DPM-Solver run costs next to the multistep one at equal NFE (ddif_plan_sample_dpm against ddif_plan_sample_dpmpp).

The GF2 scene of the benchmark (64 tiles of 64 x 64 x 4, cosine schedule, T = 1000, image-space clamp corrector): DPM_Solver.sample(method="singlestep",
order=3, steps=48) -- sixteen third-order steps, 48 network evaluations, one library call on a solver program -- against
DPM_Solver.sample(method="multistep", order=2, steps=48), the benchmark's own path, whose launches this build does not change (tests/test_dpmx_gpu.py
test_plain_multistep_dpmsolverpp_is_unchanged): that leg is the yardstick.  One process, the two legs INTERLEAVED (multi, single, multi, single, ...) so that
clock and thermal drift hit both alike.  Expectation: equal NFE = equal time (the network is > 99 % of an evaluation), i.e. the singlestep median lies inside
the spread of the multistep legs of the same run; `single_inside_multi_spread` says whether it did.

    python tools/dpm_ss_bench.py [--batch 64] [--nfe 48] [--rounds 5]        prints one JSON line"""
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
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--nfe", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert args.rounds >= 3 and args.nfe % 3 == 0
    dev = torch.device("cuda:0")
    C_, H, T = 4, 64, 1000
    cfg = engine_cfg(C_, 1)
    keys = ("in_channel", "out_channel", "inner_channel", "lms_channel", "pan_channel", "norm_groups", "channel_mults", "attn_res", "res_blocks", "dropout",
            "image_size", "self_condition")
    net = UNetSR3(**{k: cfg[k] for k in keys})
    net.load_state_dict(synth_state_dict(cfg, 1234))
    net = net.to(dev).eval()
    B = args.batch
    cond = synth_tiles(B, C_, 1, H, H, seed=100)["cond"].to(dev)
    ns = NoiseScheduleVP("discrete", betas=torch.as_tensor(make_beta_schedule("cosine", T, cosine_s=8e-3)).float())
    fn = model_wrapper(net, ns, model_type="x_start", guidance_type="classifier-free", guidance_scale=1.0, condition=cond)
    slv = DPM_Solver(fn, ns, algorithm_type="dpmsolver++", correcting_x0_fn=ImageSpaceClamp(cond[:, :C_].contiguous(), 0.0, 1.0))
    assert slv._fused_target() is not None
    xT = torch.randn(B, C_, H, H, device=dev)
    legs = dict(multi=dict(method="multistep", order=2), single=dict(method="singlestep", order=3))

    def run(leg):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = slv.sample(xT, steps=args.nfe, skip_type="time_uniform", **legs[leg])
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        return 1e3 * (time.perf_counter() - t0)

    for leg in legs:  # plans, clocks
        run(leg)
        run(leg)
    ms = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            ms[leg].append(run(leg))
    med = {leg: statistics.median(v) for leg, v in ms.items()}
    res = dict(baseline="the multistep leg of this build: the unchanged ddif_plan_sample_dpmpp path, not a build of the parent commit", batch=B, tile=H, nfe=args.nfe,
               rounds=args.rounds, run_ms_multi=med["multi"], run_ms_single=med["single"], run_ms_multi_all=[round(v, 3) for v in ms["multi"]],
               run_ms_single_all=[round(v, 3) for v in ms["single"]], eval_ms_multi=med["multi"] / args.nfe, eval_ms_single=med["single"] / args.nfe,
               single_over_multi_pct=100.0 * (med["single"] - med["multi"]) / med["multi"],
               single_inside_multi_spread=bool(min(ms["multi"]) <= med["single"] <= max(ms["multi"])))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
