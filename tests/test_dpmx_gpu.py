"""The DPM-Solver solver programs on the gfx950 library: every golden of tests/golden_cases_dpmx.py (the real reference, fp32, with its fp64 twin on file)
through DPM_Solver.sample as ONE library call -- UNetSR3.forward is patched to raise while it runs -- the intermediates, the batch / alone equality, the generic
loop against the fused run, the elementwise forms bit for bit, program validation, and the unchanged plain multistep DPM-Solver++ path.  The checks live in
tests/dpmx_checks.py, shared with tests/test_dpmx_emu.py.  On a tree without the feature the symbols do not exist and the drop-in raises DdifError."""
import pytest
import torch

import dpmx_checks as K
import golden_cases_dpmx as gx
from ddif_testlib import use_gpu_library

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gpu_library()


def test_forms_match_torch_bit_for_bit(_lib):
    K.run_forms(_lib, DEV)


@pytest.mark.parametrize("case", gx.CASES, ids=lambda c: c["cid"])
def test_matches_reference_golden(case):
    K.run_golden(case, DEV)


def test_multistep_intermediates_start_with_x_and_end_with_the_result():
    K.run_intermediates_multistep(DEV)


def test_batch_equals_tiles_alone():
    K.run_batch_equals_tiles(DEV)


def test_generic_loop_agrees_with_the_fused_run():
    K.run_generic_agrees(gx.BY_ID["dpmx_pp_ss_o3_s11_x_start"], DEV)


def test_plain_multistep_dpmsolverpp_is_unchanged():
    K.run_plain_multistep_unchanged(DEV)


def test_program_validation():
    K.run_validation(DEV)
