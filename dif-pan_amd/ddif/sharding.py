"""Tile sharding across the GPUs of one node.

Tiles (batch entries) are independent through the whole sampler, so a scene's tiles are split into contiguous
blocks, one per rank; every rank runs the full sampler on its block with a full weight replica and NO data-path
collective.  The only exchange is one all-gather of the fused tiles (RCCL over xGMI; `nccl` backend) to stitch the
scene.  The reference itself never tiles (it feeds whole images, diffusion_engine.py:373-377); by default tiles here are
non-overlapping and the stitch is a pure index permutation.

Overlapping tiles.  The grid, the weight and the blend are stated in include/ddif.h and here, and nowhere else:
  grid, per axis   scene extent L, tile t, 0 <= overlap < t, L >= t: stride = t - overlap; n = 1 if L == t else ceil((L - t) / stride) + 1; origin
                   p_k = min(k * stride, L - t) -- the last tile is shifted flush with the border.  Tiles row-major (k = ky * nx + kx), scenes outermost.
  weight           of tile k at a scene pixel (y, x) it covers: w_k = wy * wx, wy = min(y - py_k + 1, py_k + t - y), wx alike (integers, exact in fp32)
  blend            over the covering tiles in ascending k, fp32: den = sum w_k; r_k = w_k / den; out = v_0 + sum_{k >= 1} r_k * (v_k - v_0), added in order.
                   One cover: a copy.  Equal inputs: exactly v_0.
`tile_grid`, `cut_tiles(overlap=)` and `blend_tiles` follow them; on GPU tensors they run the library's kernels (ddif_tiles_cut / ddif_tiles_blend), on host
tensors the torch restatement below (which is also what the tests hold the kernels against, bit for bit).
"""
from __future__ import annotations

from typing import List, Tuple

import torch
import torch.distributed as dist


def shard_range(n_tiles: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous block [lo, hi) of tile indices owned by `rank`; n_tiles must divide evenly."""
    if n_tiles % world:
        raise ValueError(f"{n_tiles} tiles do not split evenly over {world} ranks")
    per = n_tiles // world
    return rank * per, (rank + 1) * per


def _axis_origins(L: int, tile: int, overlap: int) -> List[int]:
    stride = tile - overlap
    n = 1 if L == tile else -(-(L - tile) // stride) + 1
    return [min(k * stride, L - tile) for k in range(n)]


def tile_grid(H: int, W: int, tile: int, overlap: int) -> Tuple[List[int], List[int]]:
    """(ys, xs): the tile origins per axis of the overlapping grid (module docstring)."""
    H, W, tile, overlap = int(H), int(W), int(tile), int(overlap)
    if tile < 1 or not 0 <= overlap < tile:
        raise ValueError(f"overlap {overlap} outside [0, tile = {tile})")
    if H < tile or W < tile:
        raise ValueError(f"a scene of {H}x{W} is smaller than the tile {tile}")
    return _axis_origins(H, tile, overlap), _axis_origins(W, tile, overlap)


def _axis_weight(L: int, p: int, tile: int) -> torch.Tensor:
    """wy of the tile at origin p for every coordinate of the axis (0 where the tile does not cover it)."""
    y = torch.arange(L)
    w = torch.minimum(y - p + 1, p + tile - y)
    return torch.where((y >= p) & (y < p + tile), w, torch.zeros_like(w))


def cut_tiles_torch(scene: torch.Tensor, tile: int, overlap: int) -> torch.Tensor:
    """Torch restatement of ddif_tiles_cut: (C, H, W) or (S, C, H, W) -> (S*ny*nx, C, tile, tile)."""
    sc = scene if scene.dim() == 4 else scene.unsqueeze(0)
    ys, xs = tile_grid(sc.shape[-2], sc.shape[-1], tile, overlap)
    return torch.stack([sc[s, :, py:py + tile, px:px + tile] for s in range(sc.shape[0]) for py in ys for px in xs]).contiguous()


def blend_tiles_torch(tiles: torch.Tensor, H: int, W: int, overlap: int, n_scenes: int = 1) -> torch.Tensor:
    """Torch restatement of ddif_tiles_blend: (S*ny*nx, C, t, t) -> (S, C, H, W).  Every torch op is one correctly rounded fp32 operation per element in the
    kernel's order: den exact, r_k = w_k / den, out = (v_0 + r_1 (v_1 - v_0)) + r_2 (v_2 - v_0) ...; where tile k does not cover a pixel nothing is added."""
    n, C, t, _ = tiles.shape
    ys, xs = tile_grid(H, W, t, overlap)
    per = len(ys) * len(xs)
    if n != n_scenes * per:
        raise ValueError(f"{n} tiles are not {n_scenes} scenes of {len(ys)} x {len(xs)}")
    w = [torch.outer(_axis_weight(H, py, t), _axis_weight(W, px, t)) for py in ys for px in xs]  # (H, W) int64 each
    den = torch.stack(w).sum(0).to(torch.float32)
    out = torch.empty((n_scenes, C, H, W), dtype=tiles.dtype, device=tiles.device)
    for s in range(n_scenes):
        v0 = torch.zeros((C, H, W), dtype=tiles.dtype, device=tiles.device)
        acc = torch.zeros_like(v0)
        seen = torch.zeros((H, W), dtype=torch.bool)
        for k, (py, px) in enumerate((py, px) for py in ys for px in xs):
            v = torch.zeros_like(v0)
            v[:, py:py + t, px:px + t] = tiles[s * per + k]
            cov = w[k] > 0
            first = (cov & ~seen).to(tiles.device)
            later = (cov & seen).to(tiles.device)
            v0 = torch.where(first, v, v0)
            acc = torch.where(first, v, acc)
            r = (w[k].to(torch.float32) / den).to(tiles.device)
            acc = torch.where(later, acc + r * (v - v0), acc)
            seen |= cov
        out[s] = acc
    return out


def cut_tiles(scene: torch.Tensor, tile: int, overlap: int = 0) -> torch.Tensor:
    """(C, H, W) -> (ny*nx, C, tile, tile), row-major over the tile grid.  overlap > 0: the overlapping grid of `tile_grid` (any H, W >= tile; a
    (S, C, H, W) batch of scenes is accepted too, scenes outermost) -- the library's kernel on GPU tensors, the torch restatement on host tensors."""
    if overlap:
        if scene.is_cuda:
            from .runtime import tiles_cut

            sc = scene if scene.dim() == 4 else scene.unsqueeze(0)
            ys, xs = tile_grid(sc.shape[-2], sc.shape[-1], tile, overlap)
            return tiles_cut(sc, tile, overlap, len(ys) * len(xs))
        return cut_tiles_torch(scene, tile, overlap)
    C, H, W = scene.shape
    if H % tile or W % tile:
        raise ValueError("scene size must be a multiple of the tile size")
    ny, nx = H // tile, W // tile
    return scene.reshape(C, ny, tile, nx, tile).permute(1, 3, 0, 2, 4).reshape(ny * nx, C, tile, tile).contiguous()


def stitch_tiles(tiles: torch.Tensor, ny: int, nx: int) -> torch.Tensor:
    """Inverse of cut_tiles: (ny*nx, C, h, w) -> (C, ny*h, nx*w)."""
    n, C, h, w = tiles.shape
    assert n == ny * nx
    return tiles.reshape(ny, nx, C, h, w).permute(2, 0, 3, 1, 4).reshape(C, ny * h, nx * w).contiguous()


def blend_tiles(tiles: torch.Tensor, H: int, W: int, overlap: int, n_scenes: int = 1) -> torch.Tensor:
    """Tiles of the overlapping grid -> (C, H, W) (or (S, C, H, W) with n_scenes > 1) by the weighted blend of the module docstring: the stitch of tiles that
    were sampled independently ("final" blending), and of a fused run, where all covers agree and it reduces to copies."""
    if tiles.is_cuda:
        from .runtime import tiles_blend

        tile_grid(H, W, tiles.shape[-1], overlap)  # argument check
        out = tiles_blend(tiles, n_scenes, H, W, overlap)
    else:
        out = blend_tiles_torch(tiles, H, W, overlap, n_scenes)
    return out[0] if n_scenes == 1 else out


def _collectives_on(t: torch.Tensor) -> bool:
    """Run the stitch collective?  Yes with more than one rank; at world size 1 only when the group is RCCL ("nccl") and the tensor lives on a GPU -- a one-rank
    gloo group (a CPU-side launcher, a unit test) must not be handed CUDA tensors."""
    if not dist.is_initialized():
        return False
    if dist.get_world_size() > 1:
        return True
    return dist.get_backend() == "nccl" and t.is_cuda


def sample_sharded(diffusion, cond_all: torch.Tensor, mode: str = "ddpm_sample", seed: int = 0, x_T: torch.Tensor = None,
                   tile_base: int = 0, **kw) -> torch.Tensor:
    """Sample every tile of `cond_all` (n_tiles, 2C+4P, h, w; the same tensor on every rank) with the tiles split over
    the ranks of the default process group, then all-gather.  Returns sr = clip(residual + lms, 0, 1) for ALL tiles on
    every rank.  The noise stream is keyed by global tile index (`tile_base` + index in `cond_all`), so the result does
    not depend on the world size or on how a scene's tiles are batched.  `x_T` (n_tiles, C, h, w), optional, pins the
    initial noise (parity tests); by default it comes from the same counter-based generator."""
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    lo, hi = shard_range(cond_all.shape[0], rank, world)
    cond = cond_all[lo:hi].contiguous()
    C = diffusion.channels
    if x_T is not None:
        kw = dict(kw, x_T=x_T[lo:hi].contiguous())
    res = diffusion(cond, mode=mode, seed=seed, tile0=tile_base + lo, device_rng=x_T is None, **kw)
    sr = (res + cond[:, :C]).clip(0, 1)  # diffusion_engine.py:446-447
    if not _collectives_on(sr):
        return sr
    # (with an RCCL process group the collective runs even at world size 1 -- a copy -- so that a 1-GPU run under a launcher exercises RCCL: tests/test_rccl_world1.py)
    out = torch.empty((cond_all.shape[0],) + tuple(sr.shape[1:]), dtype=sr.dtype, device=sr.device)
    dist.all_gather_into_tensor(out, sr.contiguous())
    return out


def scene_grid(n_tiles: int) -> Tuple[int, int]:
    """(ny, nx) with ny * nx == n_tiles and ny the largest divisor <= sqrt(n_tiles): 64 -> 8 x 8, 32 -> 4 x 8, 8 -> 2 x 4."""
    ny = int(n_tiles ** 0.5)
    while ny > 1 and n_tiles % ny:
        ny -= 1
    return max(1, ny), n_tiles // max(1, ny)


def sample_scene_dpmpp(net, diffusion, cond_all: torch.Tensor, x_T_all: torch.Tensor, steps: int = 50, order: int = 2, grid=None) -> torch.Tensor:
    """BASELINE configs[2]: ONE scene = `cond_all` (n_tiles, 2C+4P, h, w; the same on every rank) sampled with DPM-Solver++ multistep, the tiles
    split in contiguous blocks over the ranks of the default process group (strong scaling: n_tiles / world per GPU), one all-gather, then the
    stitch.  `x_T_all` (n_tiles, C, h, w) is the scene's initial noise (the same on every rank; each rank uses its block), so the fused scene does
    not depend on the number of GPUs.  Returns the fused scene (C, ny h, nx w) on every rank.

    Tiling is a DESIGN DECISION of this build, not a property of the reference: the reference feeds the whole scene through the network
    (diffusion_engine.py:373-377), where GroupNorm(1 group) statistics span the whole scene, the 3x3 convs see their neighbours across what
    would be tile edges (here: zero padding at every tile edge) and the H/8 self-attention attends over the whole scene.  A tiled run is
    therefore NOT the same function as the whole-scene run; each tile is the reference's computation ON THAT TILE
    (what `test_fn` does with 64 x 64 training-size inputs), and whole scenes up to the 4 GiB tensor limit can still go through one plan."""
    from .solver.dpm_solver import DPM_Solver, ImageSpaceClamp, NoiseScheduleVP, model_wrapper

    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    n = cond_all.shape[0]
    ny, nx = grid if grid is not None else scene_grid(n)
    lo, hi = shard_range(n, rank, world)
    cond = cond_all[lo:hi].contiguous()
    C = diffusion.channels
    lms = cond[:, :C].contiguous()
    ns = NoiseScheduleVP("discrete", betas=diffusion.betas)
    fn = model_wrapper(net, ns, model_type="x_start", guidance_type="classifier-free", guidance_scale=1.0, condition=cond)
    solver = DPM_Solver(fn, ns, algorithm_type="dpmsolver++", correcting_x0_fn=ImageSpaceClamp(lms, 0.0, 1.0))
    res = solver.sample(x_T_all[lo:hi].contiguous(), steps=steps, order=order, skip_type="time_uniform", method="multistep")
    sr = (res + lms).clip(0, 1)  # diffusion_engine.py:446-447
    if _collectives_on(sr):
        out = torch.empty((n,) + tuple(sr.shape[1:]), dtype=sr.dtype, device=sr.device)
        dist.all_gather_into_tensor(out, sr.contiguous())
        sr = out
    return stitch_tiles(sr, ny, nx)
