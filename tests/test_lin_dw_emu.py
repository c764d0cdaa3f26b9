"""dW of the coefficient generator's linear as a role of the attention backward, on the host SIMT emulation (lin_dw_checks.py)."""
import pytest
import torch

import lin_dw_checks as LD
from feta_tmlr_amd import _lib

CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def blk(emu):
    """B = 4 graphs of 5 .. 37 nodes and the launch without the role, computed once"""
    b = LD.block_case(emu, CPU, None)
    return b, LD.launch(emu, None, b)


@pytest.fixture(scope='module')
def cases():
    memo = {}

    def get(rc):
        if rc not in memo:
            memo[rc] = LD.dw_case(rc[0], rc[1], CPU)
        return memo[rc]
    return get


@pytest.mark.parametrize('rc', LD.SHAPES)
def test_role_beside_the_main_grid(emu, blk, cases, rc):
    LD.check_kernel(emu, None, blk[0], cases(rc), blk[1])


def test_role_column_sums_and_main_grid_in_one_launch(emu, blk, cases):
    LD.check_all_roles(emu, None, blk[0], cases((128, 256)), blk[1])


def test_two_launches_are_bit_equal(emu, blk, cases):
    LD.check_kernel(emu, None, blk[0], cases((128, 256)), blk[1], twice=True)


def test_more_tiles_than_free_slots(emu, blk, cases, monkeypatch):
    case = cases((64, 256))
    one = LD.check_kernel(emu, None, blk[0], case, blk[1])
    LD.check_rounds(emu, CPU, None, case, one, monkeypatch)


def test_bad_arguments_are_rejected(emu, blk):
    LD.check_rejects(emu, CPU, None, blk[0])


@pytest.mark.parametrize('bsz,n_pad', [(16, 37), (32, 13), (48, 13)])
def test_model_role_on_off_and_oracle(emu, monkeypatch, bsz, n_pad):
    """B = 16, 32, 48: one, two and three contraction chunks.  N_pad = 37 as at the headline for the first; the two larger
    batches on graphs of up to 13 nodes here (an emulated step of them at N_pad = 37 takes minutes) and at N_pad = 37 on the
    MI355X (test_lin_dw_gpu.py)"""
    LD.check_model(emu, CPU, lambda: _lib.override_for_tests(emu), monkeypatch, bsz, n_pad=n_pad)


def test_model_with_8_heads(emu, monkeypatch):
    """d_h = 8, order 4: C = 256; 8 graphs of up to 13 nodes = 64 rows, the smallest shape the role takes"""
    LD.check_model(emu, CPU, lambda: _lib.override_for_tests(emu), monkeypatch, 8, heads=8, order=4, n_pad=13)


def test_fallbacks(emu, monkeypatch):
    LD.check_fallbacks(emu, CPU, lambda: _lib.override_for_tests(emu), monkeypatch)


def test_two_phase_backward_keeps_the_library(emu, monkeypatch):
    LD.check_two_phase(emu, CPU, lambda: _lib.override_for_tests(emu), monkeypatch)


def test_descriptor_layout_agrees():
    import test_abi
    test_abi.test_descriptor_layouts_agree('feta_lin_dw', 'LinDw')
