"""The one-launch training forward of LayerNorm stacks (feta_encoder_fwd_save) on the MI355X: the checks of
tests/train_fwd_checks.py on the real library, and the hipGraph-captured training step with the switch on."""
import contextlib

import pytest
import torch

import kernel_checks as KC
import train_fwd_checks as TF
from feta_tmlr_amd import train as T
from feta_tmlr_amd.transformer import layers as LY

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NOHOOK = contextlib.nullcontext


@pytest.mark.parametrize('n,n_min,nl,ff', TF.KERNEL_CASES)
def test_fwd_save_matches_fp64(hip, n, n_min, nl, ff):
    abi, dev, stream = hip
    print(TF.check_kernel(abi, dev, stream, 3, n, 4, nl, ff, seed=n + nl, n_min=n_min))


@pytest.mark.parametrize('n,heads,opts', [
    (21, 4, dict(use_pe=False)),
    (21, 4, dict(use_degree=False)),
    (21, 4, dict(in_proj_bias=False)),
    (21, 8, {}),
    (37, 8, {}),
])
def test_fwd_save_matches_fp64_variants(hip, n, heads, opts):
    abi, dev, stream = hip
    TF.check_kernel(abi, dev, stream, 3, n, heads, 2, 128, seed=n, n_min=2, **opts)


def test_fwd_save_walks_graphs(hip, monkeypatch):
    abi, dev, stream = hip
    monkeypatch.setenv('FETA_INFER_MAX_GRID', '2')
    TF.check_kernel(abi, dev, stream, 5, 21, 4, 2, 128, seed=4, n_min=3)


@pytest.mark.parametrize('n,n_min,nl,ff,heads,dtype', [
    (21, 3, 2, 128, 4, torch.float32),
    (37, 2, 3, 128, 4, torch.float32),
    (37, 2, 2, 64, 8, torch.float32),
    (37, 2, 3, 128, 4, BF16),
    (64, 40, 2, 64, 4, BF16),
])
def test_fwd_save_equals_two_launch_form(hip, n, n_min, nl, ff, heads, dtype):
    print(TF.check_same_as_two_launch(NOHOOK, hip[1], 3, n, heads, nl, ff, seed=n + nl, n_min=n_min, dtype=dtype))


@pytest.mark.parametrize('heads,dtype,seed', TF.MODEL_VARIANTS)
def test_model_switch_on_equals_off(hip, monkeypatch, heads, dtype, seed):
    TF.check_model_switch(hip[1], NOHOOK, hip[0], monkeypatch, heads, dtype, seed)


def test_launch_counts(hip, monkeypatch):
    TF.check_launch_counts(hip[1], NOHOOK, hip[0], monkeypatch)


@pytest.mark.parametrize('what', ['tie', 'bn', 'n65', 'bf16_h8'])
def test_predicate_says_no(hip, monkeypatch, what):
    TF.check_predicate_says_no(hip[1], NOHOOK, hip[0], monkeypatch, what)


def test_graphed_train_step_with_one_launch_forward(hip):
    """two replays of the captured step (switch on) == two eager steps (switch on): the by-value layer table, the save
    pointers and the layer strides survive capture.  Tolerances of test_train_gpu.test_graphed_train_step_equals_eager_steps."""
    dev = hip[1]
    model_a, batch9, cache = TF.model_case(dev)
    model_b, _, _ = TF.model_case(dev)
    model_b.load_state_dict(model_a.state_dict())
    for m in (model_a, model_b):
        LY.set_one_launch_forward(m, True)
    crit = T.make_criterion('zinc', nb_class=1)
    opt_a = T.make_optimizer('zinc', model_a.parameters(), lr=1e-3)
    opt_b = T.make_optimizer('zinc', model_b.parameters(), lr=1e-3, capturable=True)
    calls = {}
    abi = hip[0]
    orig = abi.encoder_fwd_save

    def counted(*a, **kw):
        calls['n'] = calls.get('n', 0) + 1
        return orig(*a, **kw)
    abi.encoder_fwd_save = counted
    try:
        graphed = T.GraphedTrainStep('zinc', model_b, crit, opt_b, batch9, cache)
        assert calls.get('n', 0) >= 1            # (the captured step is the one-launch form)
        lrs = [1e-3, 5e-4]
        for lr in lrs:
            la = T.train_step('zinc', model_a, crit, opt_a, batch9, T.prepare_cache(model_a, batch9, cache), lr=lr)
            graphed.set_lr(lr)
            lb = graphed(batch9, cache)
            KC.assert_close('loss', lb.cpu(), la.cpu().double(), tol=3e-5)
    finally:
        abi.encoder_fwd_save = orig
    for (k, pa), (_, pb) in zip(model_a.named_parameters(), model_b.named_parameters()):
        if pa not in opt_a.state:
            assert torch.equal(pa, pb), k
            continue
        sig = opt_a.state[pa]['exp_avg'].abs() > 1e-6
        assert float((pa.detach() - pb.detach()).abs().max()) <= 2 * max(lrs) * 1.01, k
        if sig.any():
            KC.assert_close('param ' + k, pb.detach()[sig].cpu(), pa.detach()[sig].cpu().double(), tol=3e-5)
