"""The Q2n index (Q4 / Q8) on the gfx950 library, through the ctypes C ABI and the Python binding: every fixture of tests/golden_cases_q2n.py value for value,
identical images, the degenerate blocks, the rounding rule, bit-equality across batches and repeats, q_avg and the refusals.  The checks live in
tests/q2n_checks.py, shared with tests/test_q2n_emu.py.  On a tree without the feature every one of these fails: the library has no ddif_q2n and the binding
no q2n / q_avg."""
import pytest
import torch

import golden_cases_q2n as gq
import q2n_checks as K
from ddif_testlib import use_gpu_library

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gpu_library()


@pytest.mark.parametrize("case", gq.CASES, ids=lambda c: c[0])
def test_blocks_match_the_golden(case):
    K.run_fixture(case, DEV)


@pytest.mark.parametrize("case", gq.CASES, ids=lambda c: c[0])
def test_identical_images_score_one(case):
    K.run_identical(case, DEV)


def test_degenerate_blocks():
    K.run_degenerate(DEV)


def test_quantisation_rounds():
    K.run_rounding(DEV)


def test_batch_and_repeat_are_bit_equal():
    K.run_batch_and_repeat(DEV)


def test_q_avg_is_the_mean_of_single_band_calls():
    K.run_q_avg(DEV)


def test_refusals_name_the_argument():
    K.run_validation(DEV)
