"""The filter stage as one autograd node (functional.FilterStageFn) on the host emulation: tests/stage_checks.py."""
import pytest
import torch

import stage_checks as SC
from feta_tmlr_amd import _lib

CPU = torch.device('cpu')


@pytest.mark.parametrize('heads', [4, 8])
def test_hooks_on_leaf_inputs_see_finished_gradients(emu, monkeypatch, heads):
    SC.check_leaf_inputs(emu, CPU, lambda: _lib.override_for_tests(emu), monkeypatch, heads)


def test_hook_on_the_stack_output_of_the_per_layer_path(emu, monkeypatch):
    SC.check_per_layer_hook(emu, CPU, lambda: _lib.override_for_tests(emu), monkeypatch)


@pytest.mark.parametrize('fused,fold', list(SC.CALL_LISTS))
def test_step_launches_what_the_three_nodes_launched(emu, monkeypatch, fused, fold):
    SC.check_call_list(emu, CPU, lambda: _lib.override_for_tests(emu), monkeypatch, fused, fold)
