"""loss_type="l1ssim" on the gfx950 library, through the ctypes C ABI and the drop-in classes: every golden of tests/golden_cases_l1ssim.py (the real
reference's HybridL1SSIM, p_losses and p_losses(...).backward(), fp32 with the fp64 twin on file), the bit-equality of the default path around a detour
through the new loss, and the construction that used to raise.  The checks live in tests/l1ssim_checks.py, shared with tests/test_l1ssim_emu.py.  On a tree
without the feature every one of these fails: GaussianDiffusion raises DdifError for the loss, the plan refuses the objective and the library has no
ddif_l1ssim_loss."""
import pytest
import torch

import golden_cases_l1ssim as gl
import l1ssim_checks as K
from ddif_testlib import use_gpu_library

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    return use_gpu_library()


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("case", gl.OP_CASES, ids=lambda c: c[0])
def test_operator_matches_reference_golden(case, nhwc):
    K.run_op(case, DEV, nhwc)


@pytest.mark.parametrize("case", gl.OP_CASES, ids=lambda c: c[0])
def test_operator_on_identical_arguments(case):
    K.run_op_identical_arguments(case, DEV)


@pytest.mark.parametrize("case", gl.OP_CASES, ids=lambda c: c[0])
def test_module_backward_matches_reference_golden(case):
    K.run_op_module(case, DEV)


@pytest.mark.parametrize("pm", gl.PRED_MODES)
@pytest.mark.parametrize("case", gl.LOSS_CASES, ids=lambda c: c[0])
def test_p_losses_matches_reference_golden(case, pm, monkeypatch):
    K.run_loss(case, pm, DEV, monkeypatch)


@pytest.mark.parametrize("case", gl.GRAD_CASES, ids=lambda c: c[0])
def test_training_step_matches_reference_golden(case, monkeypatch):
    K.run_grad(case, DEV, monkeypatch)


def test_default_path_is_untouched():
    K.run_default_path_untouched(DEV)


def test_l1ssim_constructs():
    K.run_refusal_gone(DEV)


def test_operator_refuses_bad_arguments():
    K.run_bad_arguments(DEV)
