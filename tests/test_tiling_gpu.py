"""Overlapping tiles with per-step fusion on the gfx950 library: cut / blend kernels against the torch restatement,
tiling at overlap 0 against tiling off, one fused call against the step-by-step yardstick, agreement of the covers, scene-keyed noise, the refusals and
test_fn.  The checks live in tests/tiling_checks.py, shared with tests/test_tiling_emu.py.  On a tree without the feature the symbols do not exist."""
import pytest
import torch

import tiling_checks as K
from ddif_testlib import use_gpu_library

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gpu_library()


@pytest.mark.parametrize("Cc", [4, 12])
def test_cut_and_blend_kernels_match_the_torch_restatement(Cc):
    K.run_cut_blend(DEV, Cc)


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_tiling_on_at_overlap_0_equals_tiling_off(sampler):
    K.run_overlap0_equals_untiled(DEV, sampler)


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_one_fused_call_equals_the_step_by_step_yardstick(sampler):
    K.run_fused_equals_yardstick(DEV, sampler)


def test_covers_agree_under_the_device_rng():
    K.run_covers_agree(DEV)


def test_noise_is_per_scene_pixel():
    K.run_noise_is_per_scene_pixel(DEV)


def test_refusals_and_off_again():
    K.run_refusals(DEV)


def test_test_fn_overlap_step_and_final():
    K.run_test_fn(DEV)
