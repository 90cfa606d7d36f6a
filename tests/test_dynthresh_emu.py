"""Dynamic thresholding on the HOST-EMULATED build of the kernel sources (CPU tensors): the selection kernel (csrc/kernels_quantile.h) against torch.sort and
torch.quantile at every size of tests/dynthresh_checks.py -- both the LDS-resident and the streaming path -- and, through the same C ABI and drop-in classes
as the GPU suite, the two smallest goldens of tests/golden_cases_dynthresh.py and the switch's argument checks (the emulated network takes seconds per
step: the batch / alone equality and the mode-0 identity run on the GPU only).  The checks live in
tests/dynthresh_checks.py, shared with tests/test_dynthresh_gpu.py.  On a tree without the feature the symbols do not exist and the drop-in raises DdifError."""
import pytest

import dynthresh_checks as K
import golden_cases_dynthresh as gd
from ddif_testlib import use_emulator

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    lib = use_emulator()
    assert lib.emulated
    return lib


@pytest.mark.parametrize("n", K.SIZES)
def test_emulated_quantile_and_threshold_match_torch(_lib, n):
    K.run_op(_lib, n, DEV)


def test_emulated_ddpm_matches_reference_golden():
    K.run_ddpm(gd.DDPM_CASES[0], DEV)  # wv3 16 x 16, noise: the quantile from ~577 down to ~1, fractional rank


def test_emulated_dpm_solver_matches_reference_golden():
    K.run_dpm(gd.DPM_CASES[3], DEV)  # wv3 16 x 16, order 3, x_start


def test_emulated_set_threshold_rejects_bad_arguments():
    K.run_set_threshold_rejects(DEV)


def test_emulated_dynamic_thresholding_fn_of_both_classes():
    K.run_front_door_methods(DEV)
