"""Classifier-free guidance in DPM-Solver runs on the gfx950 library: every golden of tests/golden_cases_cfg.py (the real reference, fp32, with its fp64 twin
on file) through DPM_Solver.sample as ONE library call -- UNetSR3.forward is patched to raise while it runs; the model types the reference cannot run under
guidance against the drop-in's generic loop; batch / alone equality and the intermediates; guidance_scale == 1 on its old path; the guided form of the
evaluation kernel bit for bit; validation.  The checks live in tests/cfg_checks.py, shared with tests/test_cfg_emu.py.  On a tree without the feature the
symbols do not exist and model_wrapper raises DdifError."""
import pytest
import torch

import cfg_checks as G
import golden_cases_cfg as gcfg
from ddif_testlib import use_gpu_library

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gpu_library()


def test_guided_forms_match_torch_bit_for_bit(_lib):
    G.run_guided_forms(_lib, DEV)


@pytest.mark.parametrize("case", gcfg.CASES, ids=lambda c: c["cid"])
def test_guided_run_matches_reference_golden(case):
    G.run_golden(case, DEV)


@pytest.mark.parametrize("model_type", ["x_start", "v"])
def test_model_types_the_reference_cannot_guide_agree_with_the_generic_loop(model_type):
    G.run_generic_agrees(model_type, DEV)


def test_guided_batch_equals_tiles_alone_and_intermediates():
    G.run_batch_equals_tiles(DEV)


def test_scale_one_with_an_unconditional_condition_is_the_old_path():
    G.run_scale_one_is_the_old_path(DEV)


def test_guided_validation():
    G.run_validation(DEV)
