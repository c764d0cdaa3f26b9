"""The filter stage as one autograd node (functional.FilterStageFn) on the MI355X: tests/stage_checks.py."""
import contextlib

import pytest

import stage_checks as SC

pytestmark = pytest.mark.gpu
NULL = contextlib.nullcontext


@pytest.mark.parametrize('heads', [4, 8])
def test_hooks_on_leaf_inputs_see_finished_gradients(hip, monkeypatch, heads):
    SC.check_leaf_inputs(hip[0], hip[1], NULL, monkeypatch, heads)


def test_hook_on_the_stack_output_of_the_per_layer_path(hip, monkeypatch):
    SC.check_per_layer_hook(hip[0], hip[1], NULL, monkeypatch)


@pytest.mark.parametrize('fused,fold', list(SC.CALL_LISTS))
def test_step_launches_what_the_three_nodes_launched(hip, monkeypatch, fused, fold):
    SC.check_call_list(hip[0], hip[1], NULL, monkeypatch, fused, fold)
