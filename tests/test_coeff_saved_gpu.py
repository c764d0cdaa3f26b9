"""The coefficient generator's backward in two parts on the MI355X (coeff_saved_checks.py)."""
import contextlib

import pytest
import torch

import coeff_saved_checks as CS
from feta_tmlr_amd import functional as FF
from feta_tmlr_amd import train as T
from test_coeff_saved_emu import HOSTED, STANDALONE, cases  # noqa: F401  (the shapes and the shared fp64 references)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('key', STANDALONE)
def test_standalone_kernels(hip, cases, key):  # noqa: F811
    abi, dev, stream = hip
    CS.check_standalone(abi, dev, stream, cases(key))


@pytest.mark.parametrize('key', HOSTED)
def test_hosted_roles(hip, cases, key, monkeypatch):  # noqa: F811
    abi, dev, stream = hip
    case = cases(key)
    CS.check_roles(abi, dev, stream, case, CS.check_standalone(abi, dev, stream, case), monkeypatch)


def test_role_is_bounded_to_two_blocks_per_workgroup(hip):
    CS.check_fits(*hip)
    # K <= 32 instantiations hold one workgroup per CU: 256 slots, 128 free beside 128 graphs - four blocks each, not taken
    assert not hip[0].spec_cat_fwd_coeff_fits(128, 37, 32, 512)


def test_batch_that_nearly_fills_a_round(hip, monkeypatch):
    CS.check_batch_that_nearly_fills_a_round(hip[0], hip[1], contextlib.nullcontext, monkeypatch)


def test_empty_block_writes_zeros(hip):
    CS.check_empty_block(*hip)


def test_bad_arguments_are_rejected(hip):
    CS.check_rejects(*hip)


def test_model_switch_on_off_and_oracle(hip, monkeypatch):
    CS.check_model(hip[0], hip[1], contextlib.nullcontext, monkeypatch)


def test_fallbacks(hip, monkeypatch):
    CS.check_fallbacks(hip[0], hip[1], contextlib.nullcontext, monkeypatch)


def test_captured_step_replays_equal(hip, monkeypatch):
    """the captured training step with the saved form inside: two replays from the same state give the same gradients"""
    monkeypatch.setattr(FF, 'USE_COEFF_DSUM', True)
    dev = hip[1]
    model, batch9, cache = CS.headline_model(dev)
    crit = T.make_criterion('zinc', nb_class=1)
    opt = T.make_optimizer('zinc', model.parameters(), lr=1e-3, capturable=True)
    with CS.Counter(hip[0]) as c:
        graphed = T.GraphedTrainStep('zinc', model, crit, opt, batch9, cache)
    assert 'feta_spec_filter_cat_fwd_coeff' in c.calls and 'feta_ffn_bwd_coeff_saved' in c.calls, c.calls
    snap = graphed._snapshot()
    grads = []
    for _ in range(2):
        graphed(batch9, cache)
        torch.cuda.synchronize()
        grads.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
        graphed._restore(snap)
    assert grads[0].keys() == grads[1].keys() and 'encoder.gcn.weight' in grads[0]
    for k in grads[0]:
        assert bool(torch.isfinite(grads[0][k]).all()) and torch.equal(grads[0][k], grads[1][k]), k
