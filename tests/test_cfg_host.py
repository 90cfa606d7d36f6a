"""Classifier-free guidance in model_wrapper (reference solver/dpm_solver.py:330-338) -- no kernels, no library: the guided model_fn on a lambda model equals
the hand-written fp32 expression for every model type, from one model call on [unconditional; conditional]; guidance_scale == 1 or no unconditional condition
is the single conditional call; the generic solver loops carry a guided model_fn; a mismatched unconditional_condition is refused.  The checks live in
tests/cfg_checks.py.  On a tree without the feature model_wrapper raises DdifError for guidance_scale != 1."""
import pytest

import cfg_checks as G


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("model_type", ["noise", "x_start", "v"])
def test_guided_model_fn_equals_the_hand_written_expression(model_type, B):
    G.run_host_guided_model_fn(model_type, B)


def test_scale_one_or_no_unconditional_condition_is_the_single_conditional_call():
    G.run_host_single_call_without_guidance()


def test_generic_loops_carry_a_guided_model_fn():
    G.run_host_guided_generic_solver()


def test_mismatched_unconditional_condition_and_bad_scales_are_refused():
    G.run_host_wrapper_validation()
