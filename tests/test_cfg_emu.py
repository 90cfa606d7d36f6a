"""Classifier-free guidance in DPM-Solver runs on the HOST-EMULATED build of the kernel sources (CPU tensors): the guided form of dpm_eval_update_kernel
(csrc/kernels_misc.h) against its torch restatement, bit for bit, the clamp included; the cheapest golden of tests/golden_cases_cfg.py through
DPM_Solver.sample (the emulated network takes a second per evaluation on the doubled batch: the rest runs on the GPU only) -- the one under dynamic
thresholding, whose selection launch computes the guided eps as well; and the validation of ddif_plan_sample_dpm_guided.  The checks live in tests/cfg_checks.py, shared with
tests/test_cfg_gpu.py.  On a tree without the feature the symbols do not exist and model_wrapper raises DdifError."""
import pytest

import cfg_checks as G
import golden_cases_cfg as gcfg
from ddif_testlib import use_emulator

DEV = "cpu"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    lib = use_emulator()
    assert lib.emulated
    return lib


def test_emulated_guided_forms_match_torch_bit_for_bit(_lib):
    G.run_guided_forms(_lib, DEV)


def test_emulated_guided_multistep_thresholding_matches_reference_golden():
    G.run_golden(gcfg.BY_ID["cfg_pp_ms_o2_s10_taylor_dyn_g2"], DEV)


def test_emulated_guided_validation():
    G.run_validation(DEV)
