"""pred_mode "noise" / "pred_v", loss "l2" and p2 weighting on the HOST-EMULATED build of the kernel sources (CPU tensors), through the same C ABI
and drop-in classes as the GPU suite: every golden of tests/golden_cases_objective.py (the real reference, fp32, with its fp64 twin on file).
The checks themselves live in tests/objective_parity.py, shared with tests/test_objective_gpu.py.  On a tree without the feature the drop-in raises
DdifError for every one of these configurations."""
import pytest

import golden_cases_objective as go
import objective_parity as P
from ddif_testlib import use_emulator

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    lib = use_emulator()
    assert lib.emulated
    return lib


@pytest.mark.parametrize("pm", go.PRED_MODES)
@pytest.mark.parametrize("case", go.DDPM_CASES, ids=lambda c: c[0])
def test_emulated_ddpm_matches_reference_golden(case, pm):
    P.run_ddpm(case, pm, DEV)


@pytest.mark.parametrize("pm", go.PRED_MODES)
@pytest.mark.parametrize("case", go.DDIM_CASES, ids=lambda c: c[0])
def test_emulated_ddim_matches_reference_golden(case, pm):
    P.run_ddim(case, pm, DEV)


@pytest.mark.parametrize("pm", go.PRED_MODES)
@pytest.mark.parametrize("case", go.DPM_CASES, ids=lambda c: c[0])
def test_emulated_dpm_solver_matches_reference_golden(case, pm):
    P.run_dpm(case, pm, DEV)


@pytest.mark.parametrize("pm", go.PRED_MODES)
@pytest.mark.parametrize("case", go.LOSS_CASES, ids=lambda c: c[0])
def test_emulated_p_losses_matches_reference_golden(case, pm, monkeypatch):
    P.run_loss(case, pm, DEV, monkeypatch)


@pytest.mark.parametrize("case", go.GRAD_CASES, ids=lambda c: c[0])
def test_emulated_p_losses_backward_matches_reference_golden(case, monkeypatch):
    P.run_grad(case, DEV, monkeypatch)


def test_emulated_explicit_default_objective_is_bit_identical():
    P.run_default_objective_is_bit_identical(DEV)


def test_emulated_plain_entry_points_refuse_a_prediction_objective():
    P.run_plain_entry_points_refuse_a_prediction_objective(DEV)
