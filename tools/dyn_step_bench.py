"""What a dynamically thresholded DDPM step costs (GaussianDiffusion clamp_type="dynamic"; csrc/kernels_quantile.h).

  1. The step pair: the engine's WV3 configuration (B tiles of 64 x 64 x 8, T-step DDPM loop, device noise) with the absolute clamp -- the final conv's
     sampler epilogue, 132 launches per step -- against the same loop with the plan's threshold mode 1 (the unfused tail: quantile kernel, update, counter),
     as a same-process INTERLEAVED pair: abs, dyn, abs, dyn, ... so that clock and thermal drift hit both alike; the median of the rounds is reported.
     The `abs` leg is THIS build with the switch off, not a library built from the parent commit; the output says so (`baseline`).  With the switch off
     this build issues the parent's launches with the parent's bits (tests/test_dynthresh_gpu.py test_mode0_is_bit_identical).
  2. The quantile kernel alone (ddif_dynamic_threshold without an output) at the LDS-resident size (64 x 64 x 8 = 32 768 values) and the streaming size
     (CAVE 128 x 128 x 31 = 507 904 values), on standard normals and on a clamped image (half zeros, a quarter ones: the contended histogram).

    python tools/dyn_step_bench.py [--batch 64] [--T 40] [--rounds 7]        prints one JSON line"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "dif-pan_amd"), ROOT]
import torch  # noqa: E402

from ddif import runtime  # noqa: E402
from ddif.diffusion.diffusion_ddpm_pan import GaussianDiffusion, make_beta_schedule  # noqa: E402
from ddif.layout import engine_cfg  # noqa: E402
from ddif.models.sr3_dwt import UNetSR3  # noqa: E402
from ddif.synth import synth_state_dict, synth_tiles  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--T", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cfg = engine_cfg(8, 1)
    keys = ("in_channel", "out_channel", "inner_channel", "lms_channel", "pan_channel", "norm_groups", "channel_mults", "attn_res", "res_blocks", "dropout",
            "image_size", "self_condition")
    net = UNetSR3(**{k: cfg[k] for k in keys})
    net.load_state_dict(synth_state_dict(cfg, 1234))
    net = net.to(dev).eval()
    B, H, T = args.batch, 64, args.T
    cond = synth_tiles(B, 8, 1, H, H, seed=100)["cond"].to(dev)
    d = GaussianDiffusion(net, image_size=H, channels=8, pred_mode="x_start", loss_type="l1", device=dev, clamp_range=(0, 1))
    d.set_new_noise_schedule(betas=make_beta_schedule("cosine", T, cosine_s=8e-3), device=dev)
    xT = torch.randn(B, 8, H, H, device=dev)

    def loop(kind):
        d.clamp_type = kind
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d(cond, mode="ddpm_sample", x_T=xT, seed=7)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / T

    for kind in ("abs", "dynamic"):  # plans, captured pairs, clocks
        loop(kind)
        loop(kind)
    ms = {"abs": [], "dynamic": []}
    for _ in range(args.rounds):
        for kind in ("abs", "dynamic"):
            ms[kind].append(loop(kind))
    d.clamp_type = "dynamic"
    plan = d._plan(cond)
    launches = plan.num_launches()["step"]  # the step program (the network); the sampler tail is not part of it
    assert plan.get_threshold()[0] == "ddpm"
    # abs: the update runs in the final conv's epilogue (no tail).  dynamic: quantile_abs_kernel, ddpm_step_kernel, step_advance_kernel behind the program
    # (Plan::run_sampler); rocprofv3 --kernel-trace --stats on this script counts them.
    tail_dynamic = 3
    res = dict(baseline="this build with the threshold switch off (mode 0), not a build of the parent commit", batch=B, tile=H, T=T, rounds=args.rounds, step_ms_abs=statistics.median(ms["abs"]), step_ms_dynamic=statistics.median(ms["dynamic"]),
               step_ms_abs_all=[round(v, 4) for v in ms["abs"]], step_ms_dynamic_all=[round(v, 4) for v in ms["dynamic"]],
               launches_step_program=launches, launches_abs=launches, launches_dynamic=launches + tail_dynamic)
    res["overhead_ms"] = res["step_ms_dynamic"] - res["step_ms_abs"]
    res["overhead_pct"] = 100.0 * res["overhead_ms"] / res["step_ms_abs"]

    lib = runtime.get_lib()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    kern = {}
    for name, Bq, n in (("resident_32768", B, 32768), ("streaming_507904", 8, 507904)):
        for data in ("normal", "clamped"):
            if data == "normal":
                x = torch.randn(Bq, n, device=dev)
            else:
                u = torch.rand(Bq, n, device=dev)
                x = torch.where(u < 0.5, torch.zeros_like(u), torch.where(u < 0.75, torch.ones_like(u), torch.rand_like(u)))
            s = torch.empty(Bq, device=dev)
            call = lambda: lib.check(lib.dll.ddif_dynamic_threshold(C.c_void_p(x.data_ptr()), Bq, n, 0.8, 1.0, 0, None, C.c_void_p(s.data_ptr()), stream), "ddif_dynamic_threshold")
            for _ in range(5):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 50
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            kern[f"{name}_{data}_us"] = 1e3 * e0.elapsed_time(e1) / reps
            kern[f"{name}_workgroups"] = Bq
    res["quantile_kernel"] = kern
    print(json.dumps(res))


if __name__ == "__main__":
    main()
