"""The one-launch inference stack on bf16 storage (feta_encoder_infer_ex) on the host SIMT emulation of the kernel
source: the bf16 kernel against the fp64 eval-mode reference under the bar of infer_lp_checks, the fp32 form of the _ex
entry against feta_encoder_infer, the descriptor's layout, and which launches a bf16-storage model's forward issues under
torch.inference_mode() and under torch.no_grad()."""
import copy
import ctypes
import os
import re

import pytest
import torch

import infer_checks as IC
import infer_lp_checks as LC
from feta_tmlr_amd import _abi, _lib
from feta_tmlr_amd.transformer import data as D
from feta_tmlr_amd.transformer.layers import set_storage_dtype
from feta_tmlr_amd.transformer.models import DiffGraphTransformerGenGCN

CPU = torch.device('cpu')
BF16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('in_dtype', [torch.float32, BF16], ids=['in_fp32', 'in_bf16'])
@pytest.mark.parametrize('bsz,n,nl,ff,batch_norm,opts', [
    (2, 5, 1, 64, True, {}),
    (3, 17, 2, 128, True, dict(n_min=3)),
    (1, 1, 1, 128, False, {}),
    (2, 16, 1, 64, False, dict(use_pe=False, in_proj_bias=False, n_min=9)),
    (2, 37, 2, 128, True, dict(use_degree=False, n_min=20)),
    (2, 17, 1, 128, False, dict(tie_qk=True, n_min=2, need_attn=False)),
])
def test_encoder_infer_bf16_matches_fp64(emu, bsz, n, nl, ff, batch_norm, opts, in_dtype):
    """Emulator figures (err / scale, worst of y, concat, attn; new | today): 4.7e-3 | 4.4e-3, 8.0e-3 | 8.0e-3,
    3.5e-3 | 4.5e-3, 3.6e-3 | 3.8e-3, 8.4e-3 | 8.4e-3, 4.9e-3 | 6.1e-3 - every case inside BF16_TOL = 2e-2 on its own."""
    with _lib.override_for_tests(emu):
        LC.check_infer_lp(emu, CPU, None, bsz, n, nl, ff, batch_norm, seed=n + nl, in_dtype=in_dtype, **opts)


def test_in_dtype_fp32_and_bf16_are_bitwise_equal(emu):
    """x and pe are rounded while they are staged: bf16-representable values give the same bits either way"""
    x, pe, degree, n_real, layers = LC.make_case(3, 21, 128, 2, True, seed=5, n_min=4)
    a = LC.run_kernel(emu, CPU, None, x, pe, degree, n_real, layers, 4, True, in_dtype=torch.float32)
    b = LC.run_kernel(emu, CPU, None, x, pe, degree, n_real, layers, 4, True, in_dtype=BF16)
    for name, u, v in zip(('y', 'concat', 'attn'), a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v), name


def test_encoder_infer_bf16_walks_graphs(emu, monkeypatch):
    """more graphs than workgroups: each workgroup runs several graphs one after the other"""
    monkeypatch.setenv('FETA_INFER_MAX_GRID', '2')
    with _lib.override_for_tests(emu):
        LC.check_infer_lp(emu, CPU, None, 3, 9, 2, 64, True, seed=3, n_min=2)


@pytest.mark.parametrize('heads', [4, 8])
def test_ex_entry_in_fp32_is_the_fp32_kernel(emu, heads):
    """dtype = FETA_F32 through feta_encoder_infer_ex == feta_encoder_infer, bit for bit"""
    x, pe, degree, n_real, layers = IC.make_case(3, 19, 128, 2, True, seed=heads, n_min=3)
    old = IC.run_kernel(emu, CPU, None, x, pe, degree, n_real, layers, heads, True)
    new = LC.run_kernel(emu, CPU, None, x, pe, degree, n_real, layers, heads, True, dtype=torch.float32)
    for name, u, v in zip(('y', 'concat', 'attn'), old, new):
        assert torch.isfinite(u).all() and torch.equal(u, v), name


def test_ex_predicate_and_rejections(emu):
    assert emu.encoder_infer_ex_supported(64, 64, 4, 128, 16, BF16)
    assert emu.encoder_infer_ex_supported(64, 64, 8, 128, 16, torch.float32)
    assert not emu.encoder_infer_ex_supported(64, 64, 8, 128, 16, BF16)     # bf16 storage has no d_h = 8 form
    assert not emu.encoder_infer_ex_supported(65, 64, 4, 128, 16, BF16)
    assert not emu.encoder_infer_ex_supported(64, 64, 4, 256, 16, BF16)
    assert not emu.encoder_infer_ex_supported(64, 64, 4, 128, 17, BF16)
    assert not emu.lib.feta_encoder_infer_ex_supported(64, 64, 4, 128, 16, 2)   # no such dtype
    x, pe, degree, n_real, layers = LC.make_case(1, 5, 64, 1, True)
    with pytest.raises(ValueError, match='H=8'):
        LC.run_kernel(emu, CPU, None, x, pe, degree, n_real, layers, 8, True)
    with pytest.raises(ValueError, match='in_dtype'):       # the fp32 form reads fp32 x and pe
        LC.run_kernel(emu, CPU, None, x, pe, degree, n_real, layers, 4, True, in_dtype=BF16, dtype=torch.float32)
    with pytest.raises(ValueError, match='16-byte aligned'):    # bf16 rows that start in the middle of a 16-byte unit
        n, bsz, d = x.shape
        xb = torch.zeros(n * bsz * d + 2, dtype=BF16)[2:].view(n, bsz, d)
        table = [dict({k: v.float() for k, v in p.items()}, n1_eps=IC.EPS, n2_eps=IC.EPS, tie_qk=0) for p in layers]
        y = torch.empty(n, bsz, d)
        emu.encoder_infer_ex(bsz, n, 4, 64, table, False, None, dtype=BF16, x=xb, pe=None, n_real=n_real,
                             y=y, out=torch.empty_like(y))
    del layers[0]['n2_var']        # the checks the two entry points share
    with pytest.raises(ValueError, match='running_mean and running_var'):
        LC.run_kernel(emu, CPU, None, x, pe, degree, n_real, layers, 4, True)


def _header_struct_fields(name):
    """(field, kind) list of a struct of include/feta_hip.h, comments removed"""
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'feta_hip.h')).read(), flags=re.S)
    body = re.search(r'struct %s \{(.*?)\}' % name, txt, flags=re.S).group(1)
    kinds = {'int': 'int', 'float': 'float', 'int64_t': 'int64', 'int32_t': 'int'}
    fields = []
    for decl in filter(None, (' '.join(d.split()) for d in body.split(';'))):
        words = decl.replace('const ', '').replace('*', ' ').split()
        kind = 'ptr' if '*' in decl else kinds[words[0]]
        fields += [(f.strip(), kind) for f in ' '.join(words[1:]).split(',')]
    return fields


def test_ex_descriptor_layout_agrees():
    kinds = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_int64: 'int64'}
    mirror = [(n, kinds[t]) for n, t in _abi.EncoderInferEx._fields_]
    assert mirror == _header_struct_fields('feta_encoder_infer_ex')
    # the fields of feta_encoder_infer, then dtype and in_dtype
    assert mirror[:-2] == _header_struct_fields('feta_encoder_infer') and [n for n, _ in mirror[-2:]] == ['dtype', 'in_dtype']


class _CountingAbi:
    """proxy of an Abi that counts the calls of its methods"""

    def __init__(self, abi):
        self._abi, self.calls = abi, {}

    def __getattr__(self, name):
        v = getattr(self._abi, name)
        if not callable(v):
            return v

        def counted(*a, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            return v(*a, **kw)
        return counted


def _model(batch_norm, layers, seed, heads=4, bsz=3, stat_spread=1.0):
    torch.manual_seed(seed)
    model = DiffGraphTransformerGenGCN(9, 1, 64, heads, dim_feedforward=128, dropout=0.0, nb_layers=layers,
                                       batch_norm=batch_norm, filter_order=4, heads_share_graph=True,
                                       filter_mode='spectral')
    IC.randomise_eval_state(model, seed, stat_spread)
    ds = D.SyntheticGraphDataset('zinc', bsz, in_dim=9, seed=seed, n_min=5, n_max=18)
    n_pad = max(g.num_nodes for g in ds.samples)
    batch9, cache = D.collate(ds.samples, k_eig=n_pad)
    return model.eval(), batch9, cache


def _forward(model, batch9, cache):
    x, mask, pe, _, degree, _, edge_index, batch, fi = batch9
    out, _, _ = model(x, edge_index, batch, fi, mask, pe, degree=degree, return_filter_coeff=True, graph_cache=cache)
    return out


@pytest.mark.parametrize('batch_norm,layers,seed', [(True, 3, 2), (False, 2, 4)], ids=['batchnorm3', 'layernorm2'])
def test_bf16_model_takes_one_launch_under_inference_mode(emu, batch_norm, layers, seed):
    """a 4-head model on bf16 storage in eval(): under inference_mode the whole stack is ONE feta_encoder_infer_ex call
    and no per-layer launch; under no_grad today's layer-by-layer bf16 path runs, untouched; the fp32 twin still makes
    its one feta_encoder_infer call.  The stack's outputs meet the bf16 bar from the model's own parameters, the final
    output the model-level bar against the fp32 twin."""
    import feta_tmlr_amd.transformer.models as M
    model32, batch9, cache = _model(batch_norm, layers, seed)
    model = set_storage_dtype(copy.deepcopy(model32), BF16).eval()
    proxy = _CountingAbi(emu)
    seen = []
    orig = M.encoder_stack_infer

    def spy(src, pe, degree_rows, n_real, layers_, need_attn=True):
        res = orig(src, pe, degree_rows, n_real, layers_, need_attn)
        seen.append((src.clone(), None if pe is None else pe.clone(), res))
        return res
    with _lib.override_for_tests(proxy):
        M.encoder_stack_infer = spy
        try:
            with torch.inference_mode():
                out_i = _forward(model, batch9, cache)
        finally:
            M.encoder_stack_infer = orig
        infer_calls = dict(proxy.calls)
        proxy.calls.clear()
        with torch.no_grad():
            out_n = _forward(model, batch9, cache)
        nograd_calls = dict(proxy.calls)
        proxy.calls.clear()
        with torch.inference_mode():
            out_32 = _forward(model32, batch9, cache)
        f32_calls = dict(proxy.calls)
    assert infer_calls.get('encoder_infer_ex') == 1, infer_calls
    for k in ('encoder_infer', 'attn_block_fwd', 'attn_block_launch', 'ffn_fwd', 'ffn_launch', 'attn_fwd'):
        assert k not in infer_calls, infer_calls
    assert 'encoder_infer_ex' not in nograd_calls and 'encoder_infer' not in nograd_calls, nograd_calls
    # today's no_grad path, untouched: the general bf16 attention core per layer for an eval BatchNorm stack (no fused
    # stack takes it), the fused bf16 training forward per layer for a LayerNorm stack
    assert nograd_calls.get('attn_fwd' if batch_norm else 'attn_block_fwd') == layers, nograd_calls
    assert f32_calls.get('encoder_infer') == 1 and 'encoder_infer_ex' not in f32_calls, f32_calls
    # the stack was handed the fp32 rows and pe (no cast launch in front of it) and returned fp32
    (src, pe_seen, got), = seen
    assert src.dtype == torch.float32 and pe_seen.dtype == torch.float32 and all(t.dtype == torch.float32 for t in got)
    degree = batch9[4]
    with _lib.override_for_tests(emu):
        LC.check_stack_against_fp64_lp(CPU, got, model.encoder, src, pe_seen, degree, cache.n_real)
    LC.assert_model_output('model output', out_i, out_n, out_32)


def test_infer_supported_on_bf16_storage(emu):
    from feta_tmlr_amd.fused_stack import infer_supported
    model, _, _ = _model(True, 2, 2)
    layers = set_storage_dtype(model, BF16).encoder.layers
    with _lib.override_for_tests(emu):
        assert infer_supported(layers, 18, 64)
        assert not infer_supported(layers, 65, 64)            # N > 64
        layers[1].storage_dtype = torch.float32               # mixed storage types
        assert not infer_supported(layers, 18, 64)
        layers[0].storage_dtype = torch.float32               # ... all fp32 again: the fp32 launch
        assert infer_supported(layers, 18, 64)
        model8, _, _ = _model(True, 2, 2, heads=8)
        assert infer_supported(model8.encoder.layers, 18, 64)
        assert not infer_supported(set_storage_dtype(model8, BF16).encoder.layers, 18, 64)   # bf16 has no d_h = 8 form
