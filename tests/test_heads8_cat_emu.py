"""The 8-head (d_h = 8) form of the folded filter launches (feta_spec_filter_cat_fwd / _bwd) on the host SIMT emulation of
the kernel sources: kernels against the fp64 oracle and autograd, head isolation, predicates, rejections, and the model
through the fold (heads8_cat_checks.py)."""
import pytest
import torch

import heads8_cat_checks as HC
from feta_tmlr_amd import _lib

CPU = torch.device('cpu')


def hook_of(emu):
    return lambda: _lib.override_for_tests(emu)


def test_predicates(emu):
    HC.check_predicates(emu)


def test_rejections(emu):
    HC.check_rejections(emu, CPU, None)


@pytest.mark.parametrize('kw', HC.FWD_CASES)
def test_forward_kernel_matches_oracle(emu, kw):
    HC.check_fwd(emu, CPU, None, **kw)


@pytest.mark.parametrize('kw', HC.BWD_CASES)
def test_backward_kernel_matches_autograd(emu, kw):
    HC.check_bwd(emu, CPU, None, **kw)


def test_heads_of_a_wave_do_not_mix(emu):
    HC.check_head_isolation(emu, CPU, None)


@pytest.mark.parametrize('batch_norm', [True, False])
def test_training_step_takes_the_folded_launches(emu, monkeypatch, batch_norm):
    HC.check_launch_names(emu, CPU, hook_of(emu), monkeypatch, batch_norm)


@pytest.mark.parametrize('batch_norm', [True, False])
def test_fold_on_and_off_match_oracle(emu, monkeypatch, batch_norm):
    HC.check_fold_on_off(emu, CPU, hook_of(emu), monkeypatch, batch_norm, bsz=3)


@pytest.mark.parametrize('batch_norm', [True, False])
def test_inference_forward_takes_the_fold(emu, monkeypatch, batch_norm):
    HC.check_inference(emu, CPU, hook_of(emu), monkeypatch, batch_norm)
