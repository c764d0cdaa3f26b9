"""8 heads (d_h = 8) through the fused attention-block kernels (ABI 13), on the host SIMT emulation of the kernel
sources: predicates, forward and backward kernels against the fp64 oracle in every form of the launch, the stack against
its three-launch form, the launch count, bf16 left alone, and what bench.py times at --heads 8."""
import pytest
import torch

import heads8_checks as H8
from feta_tmlr_amd import _abi, _lib

CPU = torch.device('cpu')


def check_predicates(abi):
    assert abi.lib.feta_version() == 13 and _abi.ABI_VERSION == 13
    for n in (1, 37, 64):
        assert abi.attn_block_supported(n, 64, 8) and abi.attn_block_bwd_supported(n, 64, 8)
        assert abi.attn_block_supported(n, 64, 4) and abi.attn_block_bwd_supported(n, 64, 4)
    assert not abi.attn_block_supported(65, 64, 8) and not abi.attn_block_bwd_supported(65, 64, 8)
    for heads in (2, 16):
        assert not abi.attn_block_supported(37, 64, heads) and not abi.attn_block_bwd_supported(37, 64, heads)
    assert not abi.attn_block_supported(37, 32, 8) and not abi.attn_block_bwd_supported(37, 32, 8)
    assert not abi.attn_out_supported(100, 64, 8)
    assert abi.attn_out_supported(100, 64, 4)


def test_predicates(emu):
    check_predicates(emu)


def check_rejections(abi, dev, stream):
    """the descriptors refuse what has no 8-head form, with a message: other head counts, bf16 storage, feta_attn_out"""
    c = H8.block_case(8, 2, 14, 3, 0)
    with pytest.raises(ValueError, match='H=16'):
        H8.run_forward(abi, dev, stream, dict(c, heads=16), None)
    d, m = 64, 28
    f32 = lambda t: t.float().contiguous().to(dev)
    new = lambda *s: torch.zeros(s, device=dev)
    with pytest.raises(ValueError, match='4 heads only'):
        desc = abi.attn_block_desc(2, 14, 8 ** -0.5, heads=8, x=f32(c['x0']).view(m, d), w_in=f32(c['p']['w_in']),
                                   w_out=f32(c['p']['w_out']), n_real=c['n_real'].to(dev), qkv=new(m, 3 * d), out=new(m, d),
                                   attn_stats=new(2, 8, 14, 2), y=new(m, d))
        abi._check(abi.lib.feta_attn_out_fwd(_abi.C.byref(desc), stream), 'feta_attn_out_fwd')


def test_rejections(emu):
    check_rejections(emu, CPU, None)


# N_pad in {14, 21, 37, 64}: 1 to 4 row tiles; every batch has a full graph and (bsz > 1) a graph with one real node
FWD_CASES = [
    ({}, dict(bsz=3, n_pad=14, norm='ln')),
    ({}, dict(bsz=3, n_pad=21, norm='bn', stats=True, with_pe=False, tie_qk=True)),
    ({}, dict(bsz=2, n_pad=21, norm=None, stats=True, rowscale=False)),
    (dict(FETA_BLOCK_FWD_WGS='1'), dict(bsz=3, n_pad=37, n_min=9, norm='bn', stats=True)),
    (dict(FETA_BLOCK_FWD_WGS='2'), dict(bsz=3, n_pad=37, n_min=9, norm='ln')),
    (dict(FETA_BLOCK_FWD_WGS='2', FETA_BLOCK_MAX_GRID='2'), dict(bsz=4, n_pad=37, n_min=9, norm='bn', stats=True)),
    (dict(FETA_BLOCK_FWD_WGS='1', FETA_BLOCK_MAX_GRID='2'), dict(bsz=5, n_pad=21, norm='ln', stats=True)),
    (dict(FETA_BLOCK_FWD_WGS='1'), dict(bsz=2, n_pad=64, n_min=40, norm='ln', with_pe=False, need_attn=False)),
    (dict(FETA_BLOCK_FWD_WGS='2'), dict(bsz=2, n_pad=64, n_min=40, norm='bn', stats=True)),
    (dict(FETA_BLOCK_FWD_WAVES='4'), dict(bsz=3, n_pad=21, norm='bn', stats=True)),     # ignored for 8 heads
]


@pytest.mark.parametrize('env,kw', FWD_CASES)
def test_forward_kernel_matches_oracle(emu, monkeypatch, env, kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    H8.check_fwd(emu, CPU, None, heads=8, **kw)


BWD_CASES = [
    ({}, dict(bsz=3, n_pad=14, form='ln')),
    ({}, dict(bsz=3, n_pad=14, form='bn', split=True)),
    ({}, dict(bsz=3, n_pad=21, form='bn', first_layer=True)),
    ({}, dict(bsz=2, n_pad=21, form='ln', split=True, first_layer=True, with_dout2=False)),
    ({}, dict(bsz=3, n_pad=37, n_min=9, form='bn')),
    ({}, dict(bsz=3, n_pad=37, n_min=9, form='ln', split=True)),
    ({}, dict(bsz=2, n_pad=64, n_min=40, form='ln', with_pe=False)),
    ({}, dict(bsz=2, n_pad=64, n_min=40, form='bn', split=True)),
    (dict(FETA_BLOCK_BWD_MAX_GRID='2'), dict(bsz=5, n_pad=21, form='bn')),       # the LOOP instantiation
    (dict(FETA_BLOCK_BWD_MAX_GRID='2'), dict(bsz=5, n_pad=37, n_min=9, form='ln')),
    (dict(FETA_BLOCK_BWD_MAX_GRID='2'), dict(bsz=3, n_pad=64, n_min=40, form='bn')),
    (dict(FETA_BLOCK_BWD_MAX_GRID='2'), dict(bsz=3, n_pad=14, form='ln', first_layer=True)),
]


@pytest.mark.parametrize('env,kw', BWD_CASES)
def test_backward_kernel_matches_autograd(emu, monkeypatch, env, kw):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    H8.check_bwd(emu, CPU, None, heads=8, **kw)


def test_four_head_descriptor_default_is_unchanged(emu):
    """H = 0 / heads=4 is the 4-head form: the generalised checks agree with the oracle there as well"""
    H8.check_fwd(emu, CPU, None, heads=4, bsz=3, n_pad=21, norm='bn', stats=True)
    H8.check_bwd(emu, CPU, None, heads=4, bsz=3, n_pad=21, form='bn', split=True)


@pytest.mark.parametrize('batch_norm', [True, False])
def test_stack_equals_three_launches(emu, monkeypatch, batch_norm):
    H8.check_stack_equals_three_launches(CPU, lambda: _lib.override_for_tests(emu), monkeypatch, batch_norm)


@pytest.mark.parametrize('batch_norm', [True, False])
def test_launch_count(emu, monkeypatch, batch_norm):
    H8.check_launch_count(CPU, lambda: _lib.override_for_tests(emu), emu, monkeypatch, batch_norm)


def test_bf16_storage_is_untouched(emu, monkeypatch):
    H8.check_bf16_untouched(CPU, lambda: _lib.override_for_tests(emu), emu, monkeypatch)


SMALL8 = ['--heads', '8', '--layers', '2', '--batch', '4', '--n-pad', '21', '--k-eig', '8', '--no-graph']
DEEP8 = ['--heads', '8', '--layers', '10', '--batch', '8', '--n-pad', '37', '--k-eig', '16', '--no-graph']


@pytest.mark.parametrize('argv', [SMALL8, SMALL8 + ['--layer-norm'], DEEP8, DEEP8 + ['--layer-norm']])
def test_bench_step_matches_oracle(emu, argv):
    """what bench.py times at --heads 8 (small shapes; and the ZINC default's 10 layers at a small batch), BatchNorm and
    LayerNorm, against oracle.encoder_gengcn - through the one-launch block kernels"""
    H8.check_bench_step_heads8(CPU, lambda: _lib.override_for_tests(emu), emu, argv)
