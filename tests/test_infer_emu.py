"""The one-launch inference stack (feta_encoder_infer, ABI 12) on the host SIMT emulation of the kernel source: kernel
against the fp64 eval-mode reference, the ctypes mirrors against the header, and which launches a model's forward issues
under torch.inference_mode() and under torch.no_grad()."""
import ctypes
import os
import re

import pytest
import torch

import infer_checks as IC
from feta_tmlr_amd import _abi, _lib
from feta_tmlr_amd.transformer import data as D
from feta_tmlr_amd.transformer.models import DiffGraphTransformerGenGCN

CPU = torch.device('cpu')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('bsz,n,heads,nl,ff,batch_norm,opts', [
    (2, 5, 4, 1, 64, True, {}),
    (3, 17, 8, 2, 128, True, dict(n_min=3)),
    (1, 1, 4, 1, 128, False, {}),
    (2, 16, 8, 1, 64, False, dict(use_pe=False, in_proj_bias=False, n_min=9)),
    (2, 37, 4, 2, 128, True, dict(use_degree=False, n_min=20)),
    (2, 17, 4, 1, 128, False, dict(tie_qk=True, n_min=2, need_attn=False)),
    (3, 5, 8, 2, 64, False, dict(tie_qk=True, use_pe=False, use_degree=False, n_min=1)),
])
def test_encoder_infer_matches_fp64(emu, bsz, n, heads, nl, ff, batch_norm, opts):
    IC.check_infer(emu, CPU, None, bsz, n, heads, nl, ff, batch_norm, seed=n + nl, **opts)


def test_encoder_infer_walks_graphs(emu, monkeypatch):
    """more graphs than workgroups: each workgroup runs several graphs one after the other"""
    monkeypatch.setenv('FETA_INFER_MAX_GRID', '2')
    IC.check_infer(emu, CPU, None, 3, 9, 4, 2, 64, True, seed=3, n_min=2)


def test_encoder_infer_rejects_bad_arguments(emu):
    x, pe, degree, n_real, layers = IC.make_case(1, 5, 64, 1, True)
    assert emu.encoder_infer_supported(5, 64, 4, 64, 1) and emu.encoder_infer_supported(64, 64, 8, 128, 16)
    assert not emu.encoder_infer_supported(65, 64, 4, 64, 1)
    assert not emu.encoder_infer_supported(5, 64, 2, 64, 1)
    assert not emu.encoder_infer_supported(5, 64, 4, 256, 1)
    assert not emu.encoder_infer_supported(5, 64, 4, 64, 17)
    del layers[0]['n2_var']        # a BatchNorm without its running statistics
    with pytest.raises(ValueError, match='running_mean and running_var'):
        IC.run_kernel(emu, CPU, None, x, pe, degree, n_real, layers, 4, True)


def _header_struct_fields(name):
    txt = re.sub(r'/\*.*?\*/', '', open(ROOT + '/include/feta_hip.h').read(), flags=re.S)
    m = re.search(r'(?:typedef )?struct %s \{(.*?)\}' % name, txt, flags=re.S)
    fields = []
    for decl in m.group(1).split(';'):
        decl = ' '.join(decl.split())
        if not decl:
            continue
        base = decl.replace('const ', '').replace('struct ', '').replace('*', ' ').split()
        kind = 'ptr' if '*' in decl else {'int': 'int', 'float': 'float', 'int64_t': 'int64', 'int32_t': 'int'}[base[0]]
        fields += [(f.strip(), kind) for f in ' '.join(base[1:]).split(',')]
    return fields


@pytest.mark.parametrize('cname,pyname', [('feta_encoder_layer', 'EncoderLayer'), ('feta_encoder_infer', 'EncoderInfer')])
def test_infer_descriptor_layouts_agree(cname, pyname):
    kinds = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_int64: 'int64'}
    assert [(n, kinds[t]) for n, t in getattr(_abi, pyname)._fields_] == _header_struct_fields(cname)


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


def _model(batch_norm, layers=3, heads=4, seed=2, bsz=3):
    torch.manual_seed(seed)
    model = DiffGraphTransformerGenGCN(9, 1, 64, heads, dim_feedforward=128, dropout=0.0, nb_layers=layers,
                                       batch_norm=batch_norm, filter_order=4, heads_share_graph=True,
                                       filter_mode='spectral')
    IC.randomise_eval_state(model, seed)
    ds = D.SyntheticGraphDataset('zinc', bsz, in_dim=9, seed=seed, n_min=5, n_max=18)
    n_pad = max(g.num_nodes for g in ds.samples)
    batch9, cache = D.collate(ds.samples, k_eig=n_pad)
    return model.eval(), batch9, cache


def _forward(model, batch9, cache):
    x, mask, pe, _, degree, _, edge_index, batch, fi = batch9
    out, _, coeff = model(x, edge_index, batch, fi, mask, pe, degree=degree, return_filter_coeff=True, graph_cache=cache)
    return out, coeff


def test_inference_mode_takes_one_launch_and_no_grad_is_unchanged(emu):
    """a 3-layer BatchNorm model in eval(): under inference_mode the whole stack is ONE feta_encoder_infer call and no
    per-layer launch; under no_grad the layer-by-layer path of today runs and the new entry point is not called.  Both
    give the same output, and the stack's output agrees with the fp64 eval-mode reference."""
    from feta_tmlr_amd import fused_stack
    model, batch9, cache = _model(True)
    proxy = _CountingAbi(emu)
    seen = []
    orig = fused_stack.encoder_stack_infer

    def spy(src, pe, degree_rows, n_real, layers, need_attn=True):
        res = orig(src, pe, degree_rows, n_real, layers, need_attn)
        seen.append((src.clone(), res))
        return res
    import feta_tmlr_amd.transformer.models as M
    with _lib.override_for_tests(proxy):
        M.encoder_stack_infer, keep = spy, M.encoder_stack_infer
        try:
            with torch.inference_mode():
                out_i, coeff_i = _forward(model, batch9, cache)
        finally:
            M.encoder_stack_infer = keep
        infer_calls = dict(proxy.calls)
        proxy.calls.clear()
        with torch.no_grad():
            out_n, coeff_n = _forward(model, batch9, cache)
        nograd_calls = dict(proxy.calls)
    assert infer_calls.get('encoder_infer') == 1, infer_calls
    for k in ('rowlin_fwd', 'rowlin_fwd_ex', 'attn_fwd', 'attn_block_fwd', 'attn_block_launch', 'ffn_fwd', 'ffn_launch'):
        assert k not in infer_calls, infer_calls
    assert 'encoder_infer' not in nograd_calls and nograd_calls.get('rowlin_fwd', 0) > 0, nograd_calls
    IC.KC.assert_close('output (inference_mode vs no_grad)', out_i, out_n.double(), tol=2e-6)
    IC.KC.assert_close('coefficients (inference_mode vs no_grad)', coeff_i, coeff_n.double(), tol=2e-6)
    # the stack itself against fp64, from the model's own parameters
    (src, (y, concat, attn)), = seen
    x, mask, pe, _, degree, _, _, _, _ = batch9
    ry, rc, ra = IC.reference(src.double(), pe.double(), degree.double(), cache.n_real, IC.model_layer_params(model.encoder),
                              4, True)
    IC.KC.assert_close('stack output', y, ry)
    IC.KC.assert_close('stack concat', concat, rc)
    IC.KC.assert_close('stack attn', attn, ra)


def test_layernorm_model_inference_mode_equals_no_grad(emu):
    model, batch9, cache = _model(False, layers=2, heads=8, seed=4)
    with _lib.override_for_tests(emu):
        with torch.inference_mode():
            out_i, coeff_i = _forward(model, batch9, cache)
        with torch.no_grad():
            out_n, coeff_n = _forward(model, batch9, cache)
    IC.KC.assert_close('output (inference_mode vs no_grad)', out_i, out_n.double(), tol=2e-6)
    IC.KC.assert_close('coefficients (inference_mode vs no_grad)', coeff_i, coeff_n.double(), tol=2e-6)


def test_infer_supported_turns_away_what_the_kernel_does_not_cover(emu):
    from feta_tmlr_amd.fused_stack import infer_supported
    model, _, _ = _model(True, layers=2)
    layers = model.encoder.layers
    with _lib.override_for_tests(emu):
        assert infer_supported(layers, 18, 64)
        assert not infer_supported(layers, 65, 64)            # N > 64
        layers[1].norm2.train()                               # batch statistics
        assert not infer_supported(layers, 18, 64)
        layers[1].norm2.eval()
        layers[0].self_attn.stab = 'clamp5'
        assert not infer_supported(layers, 18, 64)
