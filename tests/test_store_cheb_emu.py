"""The store's feed of filter_mode='cheb' (lhat) and of the Laplacian-PE sign flip - feta_batch_gather_ex and the eager
training step on store.batch - in the host SIMT emulation (store_cheb_checks.py; the MI355X runs the same checks, and the
captured step, in test_store_cheb_gpu.py)."""
import pytest
import torch

import store_cheb_checks as CC
from feta_tmlr_amd import _lib

CPU = torch.device('cpu')
SHAPES = [('lhat', 16, 5), ('lhat', 21, 5), ('edge', 16, 5), ('edge', 21, 5), ('spectral', 16, 5), ('spectral', 21, 5),
          ('big', 72, 3), ('big', 75, 3)]


def _ctx(emu):
    return lambda: _lib.override_for_tests(emu)


@pytest.mark.parametrize('kind,n_pad,bsz', SHAPES)
def test_lhat_equals_the_stagers(emu, kind, n_pad, bsz):
    CC.check_lhat_equals_stager(CPU, _ctx(emu), emu, kind, n_pad, bsz)


@pytest.mark.parametrize('n_pad', [16, 21])
def test_null_extras_equal_the_plain_launch(emu, n_pad):
    CC.check_null_extras(CPU, _ctx(emu), emu, n_pad)


@pytest.mark.parametrize('kind,n_pad', [('spectral', 16), ('spectral', 21), ('lap3', 21)])
def test_lap_sign_equals_lap_sign_flip(emu, kind, n_pad):
    CC.check_lap_sign(CPU, _ctx(emu), kind, n_pad)


def test_invalid_ids_give_zero_lhat_blocks(emu):
    CC.check_invalid_ids(CPU, _ctx(emu))


def test_descriptor_checks(emu):
    CC.check_descriptor(emu, CPU, None)


def test_gather_ex_descriptor_layout_agrees():
    CC.check_struct_layout()


@pytest.mark.parametrize('task,share', [('tu', 1), ('tu', 0)])
def test_cheb_store_steps_follow_the_stager_trajectory(emu, task, share):
    CC.check_trajectory_eager(task, share, CPU, _ctx(emu), emu)


def test_cheb_model_without_lhat_is_refused(emu):
    CC.check_refusal(CPU, _ctx(emu))


def test_lap_signs_is_the_draw_of_lap_sign_flip():
    """train.lap_sign_flip keeps its results and its draws: the same values as before the helper was factored out, and the
    generator ends in the same state"""
    from feta_tmlr_amd import train as T
    lap = torch.randn(3, 7, 5, generator=CC.G(1))
    g1, g2, g3 = CC.G(9), CC.G(9), CC.G(9)
    flip = torch.rand(5, generator=g1)
    want = lap * torch.where(flip >= 0.5, torch.ones_like(flip), -torch.ones_like(flip)).unsqueeze(0)
    assert torch.equal(T.lap_sign_flip(lap, generator=g2), want)
    assert torch.equal(lap * T.lap_signs(5, g3), want)
    assert torch.equal(g1.get_state(), g2.get_state()) and torch.equal(g1.get_state(), g3.get_state())
