"""The Q2n index (Q4 / Q8) on the HOST-EMULATED build of the kernel sources (CPU tensors), through the same C ABI and Python binding as the GPU suite.  The
checks live in tests/q2n_checks.py, shared with tests/test_q2n_gpu.py.  On a tree without the feature every one of these fails: the library has no ddif_q2n
and the binding no q2n / q_avg."""
import pytest

import golden_cases_q2n as gq
import q2n_checks as K
from ddif_testlib import use_emulator

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    lib = use_emulator()
    assert lib.emulated
    return lib


@pytest.mark.parametrize("case", gq.CASES, ids=lambda c: c[0])
def test_emulated_blocks_match_the_golden(case):
    K.run_fixture(case, DEV)


@pytest.mark.parametrize("case", gq.CASES, ids=lambda c: c[0])
def test_emulated_identical_images_score_one(case):
    K.run_identical(case, DEV)


def test_emulated_degenerate_blocks():
    K.run_degenerate(DEV)


def test_emulated_quantisation_rounds():
    K.run_rounding(DEV)


def test_emulated_batch_and_repeat_are_bit_equal():
    K.run_batch_and_repeat(DEV)


def test_emulated_q_avg_is_the_mean_of_single_band_calls():
    K.run_q_avg(DEV)


def test_emulated_refusals_name_the_argument():
    K.run_validation(DEV)
