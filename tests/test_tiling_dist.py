"""World-size-2 coverage of test_fn(tile=, overlap=, fuse="step") on the CPU: gloo backend, kernels under the test-only host emulator.  Rank r samples the
scenes i % 2 == r, each with all its tiles in one tiled plan, and the finished scenes are all-gathered; the result must equal the single-process run, which
holds both scenes in ONE plan, bit for bit (noise is keyed by scene index and scene pixel, scenes never mix)."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import tiling_checks as K
from ddif_testlib import use_emulator


def _run(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HIPEMU_THREADS="4")
    torch.set_num_threads(2)
    use_emulator()
    from ddif.diffusion_engine import test_fn

    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    out = test_fn(data=K.scene_data(2, K.HS, K.WS), tile=K.TILE, overlap=K.OV, fuse="step", **K.test_fn_kwargs("cpu"))
    if rank == world - 1:
        q.put(out["sr"])
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _spawn(world, port):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_run, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = q.get(timeout=900)
    for p in procs:
        p.join(timeout=900)
        assert p.exitcode == 0
    return torch.from_numpy(out)


def test_two_rank_step_fusion_equals_single_process():
    one = _spawn(1, 29641)
    two = _spawn(2, 29642)
    assert one.shape == (2, K.C_, K.HS, K.WS)
    assert torch.equal(one, two)
    assert not torch.equal(one[0], one[1])
