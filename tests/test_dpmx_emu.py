"""The DPM-Solver solver programs on the HOST-EMULATED build of the kernel sources (CPU tensors): the elementwise forms of dpm_eval_update_kernel
(csrc/kernels_misc.h) against their torch restatement, bit for bit; the two cheapest goldens of tests/golden_cases_dpmx.py through DPM_Solver.sample (the
emulated network takes seconds per evaluation: the rest runs on the GPU only); and the program validation of ddif_plan_sample_dpm.  The checks live in
tests/dpmx_checks.py, shared with tests/test_dpmx_gpu.py.  On a tree without the feature the symbols do not exist and the drop-in raises DdifError."""
import pytest

import dpmx_checks as K
import golden_cases_dpmx as gx
from ddif_testlib import use_emulator

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    lib = use_emulator()
    assert lib.emulated
    return lib


def test_emulated_forms_match_torch_bit_for_bit(_lib):
    K.run_forms(_lib, DEV)


def test_emulated_singlestep_dpmsolverpp_matches_reference_golden():
    K.run_golden(gx.BY_ID["dpmx_pp_ss_o3_s10_taylor_noise_logsnr"], DEV)  # orders 3, 3, 3, 1: lin1, lin2 and tay3 behind the clamp corrector


def test_emulated_singlestep_dpmsolver_taylor_matches_reference_golden():
    K.run_golden(gx.BY_ID["dpmx_np_ss_o3_s11_taylor_x_start"], DEV)  # orders 3, 3, 3, 2: the noise-prediction family, no corrector


def test_emulated_program_validation():
    K.run_validation(DEV)
