"""The one-launch training forward of LayerNorm stacks (feta_encoder_fwd_save) on the host SIMT emulation of the kernel
source: the saved tensors against fp64 and against the two-launch form, the model with the switch on against the switch
off and the fp64 oracle, the launches of a step, the predicate, and the ABI (descriptor layout, rejected arguments)."""
import ctypes

import pytest
import torch

import infer_checks as IC
import train_fwd_checks as TF
from feta_tmlr_amd import _abi, _lib
from test_infer_emu import _header_struct_fields

CPU = torch.device('cpu')
BF16 = torch.bfloat16


def _hook(emu):
    return lambda: _lib.override_for_tests(emu)


@pytest.mark.parametrize('n,n_min,nl,ff', TF.KERNEL_CASES)
def test_fwd_save_matches_fp64(emu, n, n_min, nl, ff):
    TF.check_kernel(emu, CPU, None, 3, n, 4, nl, ff, seed=n + nl, n_min=n_min)


@pytest.mark.parametrize('n,heads,opts', [
    (21, 4, dict(use_pe=False)),
    (21, 4, dict(use_degree=False)),
    (21, 4, dict(in_proj_bias=False)),
    (21, 8, {}),
    (37, 8, {}),
])
def test_fwd_save_matches_fp64_variants(emu, n, heads, opts):
    TF.check_kernel(emu, CPU, None, 3, n, heads, 2, 128, seed=n, n_min=2, **opts)


def test_fwd_save_walks_graphs(emu, monkeypatch):
    """more graphs than workgroups: each workgroup runs several graphs one after the other"""
    monkeypatch.setenv('FETA_INFER_MAX_GRID', '2')
    TF.check_kernel(emu, CPU, None, 5, 21, 4, 2, 128, seed=4, n_min=3)


def test_fwd_save_carries_column_sums(emu):
    """pending column sums ride in trailing workgroups of the launch (a tall and a wide segment)"""
    x, pe, degree, n_real, layers = TF.make_case(2, 5, 64, 1, seed=1)
    g = torch.Generator().manual_seed(3)
    tall, wide = torch.randn(70, 24, generator=g), torch.randn(5, 4096, generator=g)
    o1, o2 = torch.full((24,), float('nan')), torch.full((4096,), float('nan'))
    n, bsz, d = x.shape
    t = dict(qkv=torch.empty(1, n * bsz, 192), out_save=torch.empty(1, n * bsz, 64), attn_stats=torch.empty(1, bsz, 4, n, 2),
             y1=torch.empty(1, n * bsz, 64), h=torch.empty(1, n * bsz, 64), y2=torch.empty(1, n * bsz, 64))
    table = [dict({k: v.float() for k, v in layers[0].items()}, n1_eps=IC.EPS, n2_eps=IC.EPS, tie_qk=0)]
    y = torch.full((n * bsz, d), float('nan'))
    emu.encoder_fwd_save(bsz, n, 4, 64, table, None, x=x.float(), pe=pe.float(), n_real=n_real, y=y,
                         sums=[(tall, o1), (wide, o2)], **t)
    assert torch.isfinite(y).all()
    torch.testing.assert_close(o1, tall.sum(0), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(o2, wide.sum(0), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize('n,n_min,nl,ff,heads,dtype', [
    (21, 3, 2, 128, 4, torch.float32),
    (37, 2, 3, 128, 4, torch.float32),
    (37, 2, 2, 64, 8, torch.float32),
    (37, 2, 3, 128, 4, BF16),
    (64, 40, 2, 64, 4, BF16),
])
def test_fwd_save_equals_two_launch_form(emu, n, n_min, nl, ff, heads, dtype):
    TF.check_same_as_two_launch(_hook(emu), CPU, 3, n, heads, nl, ff, seed=n + nl, n_min=n_min, dtype=dtype)


@pytest.mark.parametrize('heads,dtype,seed', TF.MODEL_VARIANTS)
def test_model_switch_on_equals_off(emu, monkeypatch, heads, dtype, seed):
    TF.check_model_switch(CPU, _hook(emu), emu, monkeypatch, heads, dtype, seed)


def test_launch_counts(emu, monkeypatch):
    TF.check_launch_counts(CPU, _hook(emu), emu, monkeypatch)


@pytest.mark.parametrize('what', ['tie', 'bn', 'n65', 'bf16_h8'])
def test_predicate_says_no(emu, monkeypatch, what):
    TF.check_predicate_says_no(CPU, _hook(emu), emu, monkeypatch, what)


def test_switch_defaults_off():
    from feta_tmlr_amd import fused_stack
    from feta_tmlr_amd.transformer.models import DiffGraphTransformerGenGCN
    import os
    assert fused_stack.USE_LN_ONE_LAUNCH == (os.environ.get('FETA_LN_ONE_LAUNCH', '0') != '0')
    model = DiffGraphTransformerGenGCN(9, 1, 64, 4, dim_feedforward=128, dropout=0.0, nb_layers=1, batch_norm=False)
    assert model.encoder.one_launch_forward is None


def test_fwd_save_descriptor_layout_agrees():
    kinds = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_int64: 'int64'}
    assert ([(n, kinds[t]) for n, t in _abi.EncoderFwdSave._fields_] == _header_struct_fields('feta_encoder_fwd_save'))


def test_fwd_save_rejects_bad_arguments(emu):
    """FETA_E_ARG with a message, before any launch: the outputs keep their NaN poison"""
    assert emu.encoder_fwd_save_supported(37, 64, 4, 128, 3) and emu.encoder_fwd_save_supported(64, 64, 8, 64, 16)
    assert emu.encoder_fwd_save_supported(37, 64, 4, 128, 3, BF16)
    assert not emu.encoder_fwd_save_supported(37, 64, 8, 128, 3, BF16)
    assert not emu.encoder_fwd_save_supported(37, 64, 4, 128, 3, tie_qk=True)
    assert not emu.encoder_fwd_save_supported(65, 64, 4, 128, 3)
    x, pe, degree, n_real, layers = TF.make_case(2, 5, 64, 2, seed=1)
    n, bsz, d = x.shape
    m = n * bsz
    table = [dict({k: v.float() for k, v in p.items()}, n1_eps=IC.EPS, n2_eps=IC.EPS, tie_qk=0) for p in layers]
    nan = lambda *s, dt=torch.float32: torch.full(s, float('nan'), dtype=dt)

    def call(heads=4, dtype=torch.float32, layer_norm=True, tab=table, **over):
        t = dict(qkv=nan(2, m, 192, dt=dtype), out_save=nan(2, m, 64, dt=dtype), attn_stats=nan(2, bsz, heads, n, 2),
                 y1=nan(2, m, 64, dt=dtype), h=nan(2, m, 64, dt=dtype), y2=nan(2, m, 64, dt=dtype), y=nan(m, d))
        if dtype != torch.float32:
            t.update(out=nan(m, d), y2_last_f32=nan(m, d))
        t.update(over)
        emu.encoder_fwd_save(bsz, n, heads, 64, tab, None, dtype=dtype, layer_norm=layer_norm, x=x.to(dtype),
                             pe=pe.to(dtype), n_real=n_real, **t)
        return t

    assert torch.isfinite(call()['y']).all()        # (the arguments are fine as they stand)
    with pytest.raises(ValueError, match='norm kind'):
        call(layer_norm=False)
    with pytest.raises(ValueError, match='tie_qk'):
        call(tab=[dict(table[0], tie_qk=1), table[1]])
    with pytest.raises(ValueError, match='4 heads'):
        call(heads=8, dtype=BF16)
    with pytest.raises(ValueError, match='null save pointer'):
        call(h=None)
    with pytest.raises(ValueError, match='16-byte aligned'):
        call(y1=nan(2 * m * 64 + 8).view(-1)[1:2 * m * 64 + 1].view(2, m, 64))
    y = nan(m, d)
    with pytest.raises(ValueError, match='null save pointer'):
        call(qkv=None, y=y)
    assert torch.isnan(y).all()
