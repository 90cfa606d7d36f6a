"""The overlapping tile grid and its torch restatement (ddif/sharding.py): no kernels, no library."""
import math

import pytest
import torch

from ddif.sharding import blend_tiles, blend_tiles_torch, cut_tiles, cut_tiles_torch, stitch_tiles, tile_grid


@pytest.mark.parametrize("t", [16, 5])
def test_tile_grid_matches_the_closed_form(t):
    for L in (t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1, 36, 100):
        for ov in sorted({0, 1, t // 2, t - 1}):
            ys, xs = tile_grid(L, 100, t, ov)
            stride = t - ov
            n = 1 if L == t else math.ceil((L - t) / stride) + 1
            assert ys == [min(k * stride, L - t) for k in range(n)], (L, t, ov)
            assert ys[0] == 0 and ys[-1] == L - t and all(a <= b for a, b in zip(ys, ys[1:]))  # monotone, flush with both borders
            covered = torch.zeros(L, dtype=torch.int64)
            for p in ys:
                covered[p:p + t] += 1
            assert int(covered.min()) >= 1, (L, t, ov)  # every pixel is covered
            assert xs == tile_grid(L, 100, t, ov)[1]  # the axes are independent
    assert tile_grid(24, 36, 16, 8) == ([0, 8], [0, 8, 16, 20])


def test_overlap_0_on_a_multiple_reproduces_cut_tiles():
    scene = torch.randn(3, 32, 48, generator=torch.Generator().manual_seed(1))
    old = cut_tiles(scene, 16)
    assert torch.equal(cut_tiles(scene, 16, overlap=0), old)
    assert torch.equal(cut_tiles_torch(scene, 16, 0), old)
    assert torch.equal(blend_tiles(old, 32, 48, 0), stitch_tiles(old, 2, 3))
    with pytest.raises(ValueError):
        cut_tiles(torch.zeros(3, 24, 36), 16)  # the default keeps refusing non-multiples


def test_bad_arguments_raise():
    for H, W, t, ov in ((24, 36, 16, 16), (24, 36, 16, -1), (8, 36, 16, 4), (24, 8, 16, 4), (24, 36, 0, 0)):
        with pytest.raises(ValueError):
            tile_grid(H, W, t, ov)
    with pytest.raises(ValueError):
        blend_tiles_torch(torch.zeros(7, 4, 16, 16), 24, 36, 8)  # the grid has 8 tiles


def test_host_cut_and_blend_follow_the_definition():
    g = torch.Generator().manual_seed(2)
    scene = torch.randn(2, 4, 24, 36, generator=g)
    tiles = cut_tiles(scene, 16, overlap=8)
    assert tiles.shape == (16, 4, 16, 16)
    assert torch.equal(tiles[8 + 7], scene[1, :, 8:24, 20:36])  # scene 1, tile (1, 3): the last column is shifted flush with the border
    assert torch.equal(blend_tiles(tiles, 24, 36, 8, n_scenes=2), scene)  # equal inputs give v_0 exactly
    # the definition, pixel by pixel, on unequal tiles of one scene
    rnd = torch.randn(8, 4, 16, 16, generator=g)
    out = blend_tiles(rnd, 24, 36, 8)
    ys, xs = tile_grid(24, 36, 16, 8)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    for y, x in ((0, 0), (10, 3), (9, 18), (23, 35), (12, 21), (5, 19)):
        cov = [(k, min(y - py + 1, py + 16 - y) * min(x - px + 1, px + 16 - x)) for k, (py, px) in enumerate((py, px) for py in ys for px in xs)
               if py <= y < py + 16 and px <= x < px + 16]
        den = f32(float(sum(w for _, w in cov)))
        k0 = cov[0][0]
        py0, px0 = ys[k0 // 4], xs[k0 % 4]
        v0 = rnd[k0, :, y - py0, x - px0]
        acc = v0.clone()
        for k, w in cov[1:]:
            v = rnd[k, :, y - ys[k // 4], x - xs[k % 4]]
            acc = acc + (f32(float(w)) / den) * (v - v0)
        assert torch.equal(out[:, y, x], acc), (y, x, len(cov))
    assert len([1 for py in ys for px in xs if py <= 12 < py + 16 and px <= 21 < px + 16]) == 6  # up to six covers per pixel
