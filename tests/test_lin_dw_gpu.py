"""dW of the coefficient generator's linear as a role of the attention backward, on the MI355X (lin_dw_checks.py)."""
import contextlib

import pytest
import torch

import coeff_saved_checks as CS
import lin_dw_checks as LD
from feta_tmlr_amd import train as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def blk(hip):
    """B = 4 graphs of 5 .. 37 nodes and the launch without the role, computed once"""
    abi, dev, stream = hip
    b = LD.block_case(abi, dev, stream)
    return b, LD.launch(abi, stream, b)


@pytest.fixture(scope='module')
def cases(hip):
    memo = {}

    def get(rc):
        if rc not in memo:
            memo[rc] = LD.dw_case(rc[0], rc[1], hip[1])
        return memo[rc]
    return get


@pytest.mark.parametrize('rc', LD.SHAPES)
def test_role_beside_the_main_grid(hip, blk, cases, rc):
    LD.check_kernel(hip[0], hip[2], blk[0], cases(rc), blk[1])


def test_role_column_sums_and_main_grid_in_one_launch(hip, blk, cases):
    LD.check_all_roles(hip[0], hip[2], blk[0], cases((128, 256)), blk[1])


def test_two_launches_are_bit_equal(hip, blk, cases):
    LD.check_kernel(hip[0], hip[2], blk[0], cases((128, 256)), blk[1], twice=True)


def test_more_tiles_than_free_slots(hip, blk, cases, monkeypatch):
    abi, dev, stream = hip
    case = cases((128, 512))
    one = LD.check_kernel(abi, stream, blk[0], case, blk[1])
    LD.check_rounds(abi, dev, stream, case, one, monkeypatch)


def test_bad_arguments_are_rejected(hip, blk):
    LD.check_rejects(hip[0], hip[1], hip[2], blk[0])


@pytest.mark.parametrize('bsz', [16, 32, 48])
def test_model_role_on_off_and_oracle(hip, monkeypatch, bsz):
    LD.check_model(hip[0], hip[1], contextlib.nullcontext, monkeypatch, bsz)


def test_model_with_8_heads(hip, monkeypatch):
    """d_h = 8, order 4: C = 256; 8 graphs of up to 13 nodes = 64 rows, the smallest shape the role takes"""
    LD.check_model(hip[0], hip[1], contextlib.nullcontext, monkeypatch, 8, heads=8, order=4, n_pad=13)


def test_fallbacks(hip, monkeypatch):
    LD.check_fallbacks(hip[0], hip[1], contextlib.nullcontext, monkeypatch)


def test_two_phase_backward_keeps_the_library(hip, monkeypatch):
    LD.check_two_phase(hip[0], hip[1], contextlib.nullcontext, monkeypatch)


def test_captured_step_replays_equal(hip, monkeypatch):
    """the captured training step with the role inside: two replays from the same state give the same gradients"""
    LD.library_linear(monkeypatch)
    monkeypatch.setenv('FETA_LIN_DW_ROLE', '2')
    dev = hip[1]
    model, batch9, cache = LD.small_model(dev, 16)
    crit = T.make_criterion('zinc', nb_class=1)
    opt = T.make_optimizer('zinc', model.parameters(), lr=1e-3, capturable=True)
    with CS.Counter(hip[0]) as c:
        graphed = T.GraphedTrainStep('zinc', model, crit, opt, batch9, cache)
    assert 'feta_attn_block_bwd_sums_dw' in c.calls, c.calls
    snap = graphed._snapshot()
    grads = []
    for _ in range(2):
        graphed(batch9, cache)
        torch.cuda.synchronize()
        grads.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
        graphed._restore(snap)
    assert grads[0].keys() == grads[1].keys() and 'encoder.linear.weight' in grads[0]
    for k in grads[0]:
        assert bool(torch.isfinite(grads[0][k]).all()) and torch.equal(grads[0][k], grads[1][k]), k
