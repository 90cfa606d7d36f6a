"""loss_type="l1ssim" on the HOST-EMULATED build of the kernel sources (CPU tensors), through the same C ABI and drop-in classes as the GPU suite: every
golden of tests/golden_cases_l1ssim.py (the real reference, fp32, with its fp64 twin on file).  The checks themselves live in tests/l1ssim_checks.py, shared
with tests/test_l1ssim_gpu.py.  On a tree without the feature every one of these fails: GaussianDiffusion raises DdifError for the loss, the plan refuses the
objective and the library has no ddif_l1ssim_loss."""
import pytest

import golden_cases_l1ssim as gl
import l1ssim_checks as K
from ddif_testlib import use_emulator

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    lib = use_emulator()
    assert lib.emulated
    return lib


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("case", gl.OP_CASES, ids=lambda c: c[0])
def test_emulated_operator_matches_reference_golden(case, nhwc):
    K.run_op(case, DEV, nhwc)


@pytest.mark.parametrize("case", gl.OP_CASES, ids=lambda c: c[0])
def test_emulated_operator_on_identical_arguments(case):
    K.run_op_identical_arguments(case, DEV)


@pytest.mark.parametrize("case", gl.OP_CASES, ids=lambda c: c[0])
def test_emulated_module_backward_matches_reference_golden(case):
    K.run_op_module(case, DEV)


@pytest.mark.parametrize("pm", gl.PRED_MODES)
@pytest.mark.parametrize("case", gl.LOSS_CASES, ids=lambda c: c[0])
def test_emulated_p_losses_matches_reference_golden(case, pm, monkeypatch):
    K.run_loss(case, pm, DEV, monkeypatch)


@pytest.mark.parametrize("case", gl.GRAD_CASES, ids=lambda c: c[0])
def test_emulated_training_step_matches_reference_golden(case, monkeypatch):
    K.run_grad(case, DEV, monkeypatch)


def test_emulated_default_path_is_untouched():
    K.run_default_path_untouched(DEV)


def test_emulated_l1ssim_constructs():
    K.run_refusal_gone(DEV)


def test_emulated_operator_refuses_bad_arguments():
    K.run_bad_arguments(DEV)
