"""8 heads (d_h = 8) through the fused attention-block kernels (ABI 13) on the MI355X: the checks of test_heads8_emu.py
through libfeta_hip.so, at the emulation's shapes and at batches that fill the chip, and the ZINC default of the reference
(8 heads, 10 layers) exactly as bench.py times it - one captured hipGraph per step against the fp64 oracle."""
import contextlib

import pytest

import heads8_checks as H8
import test_heads8_emu as E

pytestmark = pytest.mark.gpu


def test_predicates(hip):
    E.check_predicates(hip[0])


def test_rejections(hip):
    E.check_rejections(*hip)


@pytest.mark.parametrize('env,kw', E.FWD_CASES + [
    ({}, dict(bsz=128, n_pad=37, n_min=9, norm='bn', stats=True)),                  # the BASELINE batch: two workgroups per graph
    ({}, dict(bsz=128, n_pad=37, n_min=9, norm='ln')),
    ({}, dict(bsz=300, n_pad=64, n_min=2, norm='bn', stats=True, with_pe=False)),   # workgroups walk the batch
    ({}, dict(bsz=64, n_pad=64, n_min=30, norm='ln')),                              # four row tiles, two workgroups per graph
])
def test_forward_kernel_matches_oracle(hip, monkeypatch, env, kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    H8.check_fwd(hip[0], hip[1], hip[2], heads=8, **kw)


@pytest.mark.parametrize('env,kw', E.BWD_CASES + [
    ({}, dict(bsz=128, n_pad=37, n_min=9, form='bn')),
    ({}, dict(bsz=128, n_pad=37, n_min=9, form='bn', split=True)),
    ({}, dict(bsz=128, n_pad=37, n_min=9, form='ln', split=True)),
    ({}, dict(bsz=300, n_pad=64, n_min=2, form='bn', with_pe=False)),               # the LOOP instantiation at its own batch
    ({}, dict(bsz=300, n_pad=64, n_min=2, form='ln')),
    ({}, dict(bsz=64, n_pad=64, n_min=30, form='ln', split=True)),
])
def test_backward_kernel_matches_autograd(hip, monkeypatch, env, kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    H8.check_bwd(hip[0], hip[1], hip[2], heads=8, **kw)


def test_four_head_descriptor_default_is_unchanged(hip):
    H8.check_fwd(hip[0], hip[1], hip[2], heads=4, bsz=3, n_pad=21, norm='bn', stats=True)
    H8.check_bwd(hip[0], hip[1], hip[2], heads=4, bsz=3, n_pad=21, form='bn', split=True)


@pytest.mark.parametrize('batch_norm,bsz', [(True, 3), (False, 3), (True, 128), (False, 128)])
def test_stack_equals_three_launches(hip, monkeypatch, batch_norm, bsz):
    H8.check_stack_equals_three_launches(hip[1], contextlib.nullcontext, monkeypatch, batch_norm, bsz=bsz)


@pytest.mark.parametrize('batch_norm', [True, False])
def test_launch_count(hip, monkeypatch, batch_norm):
    H8.check_launch_count(hip[1], contextlib.nullcontext, hip[0], monkeypatch, batch_norm)


def test_bf16_storage_is_untouched(hip, monkeypatch):
    H8.check_bf16_untouched(hip[1], contextlib.nullcontext, hip[0], monkeypatch)


ZINC_DEFAULT = ['--heads', '8', '--layers', '10']


@pytest.mark.parametrize('argv', [ZINC_DEFAULT, ZINC_DEFAULT + ['--layer-norm'], ['--heads', '8']])
def test_timed_configuration_matches_oracle(hip, argv):
    """What bench.py times at the reference's ZINC default (experiments/run_transformer_gengcn.py:35-36: 8 heads of 8, 10
    layers; B = 128, N_pad = 37, K = 16), BatchNorm and LayerNorm, and at 3 layers: the captured hipGraph against
    oracle.encoder_gengcn at the project's bars (output kernel_checks.TOL, gradients 3e-5 relative), through
    feta_attn_block_fwd / _bwd.

    The layer count is the full 10: the commit before this one, whose 8-head path is the three-launch one, passes the same
    check at 10 layers and B = 128 on the MI355X (output error 1.97e-6 BatchNorm / 1.34e-6 LayerNorm, largest absolute
    gradient error 1.6e-4 / 2.0e-4); the block kernels measure 2.02e-6 / 1.52e-6 and 1.3e-4 / 2.3e-4 - inside the bars and
    well inside 4x (kernel_checks.GUARD_FACTOR) of the three-launch path's errors.  EXPERIMENTS.md has the log."""
    errs, used_graph = H8.check_bench_step_heads8(hip[1], contextlib.nullcontext, hip[0], argv)
    assert used_graph
