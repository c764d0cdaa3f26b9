"""The one-launch inference stack on bf16 storage (feta_encoder_infer_ex) on the MI355X: the bf16 kernel against the
fp64 eval-mode reference at the shapes that are timed, bf16-storage model shells under torch.inference_mode() against
today's bf16 path and the fp32-storage twin, train.evaluate, and a captured replay.  The bar and its guard:
infer_lp_checks."""
import copy

import pytest
import torch

import infer_checks as IC
import infer_lp_checks as LC
import train_checks as TC
from bench_checks import BF16_MODEL_TOL
from feta_tmlr_amd import train as T
from feta_tmlr_amd.transformer import data as D
from feta_tmlr_amd.transformer.layers import set_storage_dtype
from feta_tmlr_amd.transformer.models import DiffGraphTransformerGenGCN

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.mark.parametrize('in_dtype', [torch.float32, BF16], ids=['in_fp32', 'in_bf16'])
@pytest.mark.parametrize('name,bsz,n,nl,ff,batch_norm', [
    ('config3', 128, 37, 3, 128, True),
    ('mutag_layernorm', 32, 28, 3, 128, False),
    ('molhiv_batchnorm', 1024, 64, 3, 128, True),     # more graphs than workgroups: the walking loop
    ('molhiv_layernorm', 1024, 64, 3, 128, False),
])
def test_encoder_infer_bf16_matches_fp64(hip, name, bsz, n, nl, ff, batch_norm, in_dtype):
    abi, dev, stream = hip
    LC.check_infer_lp(abi, dev, stream, bsz, n, nl, ff, batch_norm, seed=11, in_dtype=in_dtype, n_min=max(1, n // 4))


def test_ex_entry_in_fp32_is_the_fp32_kernel(hip):
    abi, dev, stream = hip
    for heads in (4, 8):
        x, pe, degree, n_real, layers = IC.make_case(128, 37, 128, 3, True, seed=heads, n_min=9)
        old = IC.run_kernel(abi, dev, stream, x, pe, degree, n_real, layers, heads, True)
        new = LC.run_kernel(abi, dev, stream, x, pe, degree, n_real, layers, heads, True, dtype=torch.float32)
        for name, u, v in zip(('y', 'concat', 'attn'), old, new):
            assert torch.isfinite(u).all() and torch.equal(u, v), (heads, name)


def _shell(shape, batch_norm, layers, bsz, n_max, seed, stat_spread=1.0, var_scale=1.0):
    torch.manual_seed(seed)
    model = DiffGraphTransformerGenGCN(28, 1, 64, 4, dim_feedforward=128, dropout=0.0, nb_layers=layers,
                                       batch_norm=batch_norm, filter_order=4, heads_share_graph=True,
                                       filter_mode='spectral')
    IC.randomise_eval_state(model, seed, stat_spread)
    if var_scale != 1.0:
        with torch.no_grad():
            for l in model.encoder.layers:
                l.norm1.running_var.mul_(var_scale), l.norm2.running_var.mul_(var_scale)
    ds = D.SyntheticGraphDataset(shape, bsz, in_dim=28, seed=seed, n_max=n_max)
    n_pad = max(g.num_nodes for g in ds.samples)
    batch9, cache = D.collate(ds.samples, k_eig=min(n_pad, 16), device='cuda:0')
    return model.to('cuda:0').eval(), batch9, cache


@pytest.mark.parametrize('shape,batch_norm,layers,bsz,n_max,spread,var_scale', [
    ('molhiv', True, 3, 1024, 64, 1.0, 1.0),
    ('molhiv', False, 3, 1024, 64, 1.0, 1.0),
    ('zinc', True, 3, 128, None, 1.0, 1.0),
    ('zinc', True, 10, 128, None, 0.25, 2.0),     # depth: ten eval BatchNorm layers, see the docstring
])
def test_bf16_model_inference_mode(monkeypatch, shape, batch_norm, layers, bsz, n_max, spread, var_scale):
    """The ten-layer case runs with stat_spread = 0.25 AND running_var doubled.  With stat_spread = 0.25 alone the case
    failed the guard on the comparison path (MI355X, seed 5: today's bf16 layer path is off by 4.5e-2 on the last layer's
    attn against a guard of 4e-2; new path 4.8e-2), and so did every other setting tried on the host emulation for
    today's path alone: stat_spread 0.1 / 0.15 / 0.5 / 0.75 / 1.0 over seeds 1 - 11 (19 of 20 fail, attn off by 3.5e-2 to
    1.8e-1) - lowering stat_spread makes it worse, because gamma = 1 + 0.3 randn keeps its spread and an eval BatchNorm
    with variance near 1 normalises nothing, so the residual stream grows from layer to layer (|y| ~ 30 - 40) and the
    softmax of the last layer is sharp enough for one bf16 rounding to move it.  Doubling running_var makes every eval
    BatchNorm shrink its input by 2^-1/2: |y| ~ 1.3 after ten layers, today's path within 1.6e-2 of fp64 (emulation,
    seeds 5 - 7)."""
    import feta_tmlr_amd.transformer.models as M
    model32, batch9, cache = _shell(shape, batch_norm, layers, bsz, n_max, seed=5, stat_spread=spread, var_scale=var_scale)
    model = set_storage_dtype(copy.deepcopy(model32), BF16).eval()
    seen = []
    orig = M.encoder_stack_infer

    def spy(src, pe, degree_rows, n_real, layers_, need_attn=True):
        res = orig(src, pe, degree_rows, n_real, layers_, need_attn)
        seen.append((layers_[0].storage_dtype, src.clone(), pe.clone(), res))
        return res
    monkeypatch.setattr(M, 'encoder_stack_infer', spy)
    x, mask, pe, _, degree, _, edge_index, batch, fi = batch9
    run = lambda m: m(x, edge_index, batch, fi, mask, pe, degree=degree, return_filter_coeff=True, graph_cache=cache)[0]
    with torch.inference_mode():
        out_i = run(model)
    with torch.no_grad():
        out_n = run(model)
    assert len(seen) == 1 and seen[0][0] == BF16, 'the one-launch bf16 stack was not taken'
    with torch.inference_mode():
        out_32 = run(model32)
    _, src, pe_seen, got = seen[0]
    assert src.dtype == torch.float32 and pe_seen.dtype == torch.float32
    LC.check_stack_against_fp64_lp(src.device, got, model.encoder, src, pe_seen, degree, cache.n_real)
    LC.assert_model_output('%s %s x%d output' % (shape, 'BN' if batch_norm else 'LN', layers), out_i, out_n, out_32)


def test_evaluate_reaches_the_bf16_launch(monkeypatch):
    """train.evaluate(..., inference_mode=True) on a bf16-storage model over three batches: finite metrics, the loss
    within BF16_MODEL_TOL of the fp32-storage twin's"""
    import feta_tmlr_amd.transformer.models as M
    dev = torch.device('cuda:0')
    cases = [TC.build_case('zinc', dev, seed=s, bsz=16, d=64, heads=4, layers=3, batch_norm=True, mode='spectral')
             for s in range(3)]
    model32 = cases[0][0]
    IC.randomise_eval_state(model32, 3, 0.5)
    batches = [(c[1], c[2]) for c in cases]
    model = set_storage_dtype(copy.deepcopy(model32), BF16)
    crit = T.make_criterion('zinc', nb_class=1)
    calls = []
    orig = M.encoder_stack_infer
    monkeypatch.setattr(M, 'encoder_stack_infer', lambda *a, **kw: (calls.append(a[4][0].storage_dtype), orig(*a, **kw))[1])
    res_i = T.evaluate('zinc', model, crit, batches, inference_mode=True)
    assert calls == [BF16] * 3, calls
    res_n = T.evaluate('zinc', model, crit, batches, inference_mode=False)
    res_32 = T.evaluate('zinc', model32, crit, batches, inference_mode=True)
    print('bf16 inference_mode', res_i, '\nbf16 no_grad       ', res_n, '\nfp32 inference_mode', res_32)
    assert all(v == v and abs(v) != float('inf') for v in res_i.values()), res_i
    assert abs(res_i['loss'] - res_32['loss']) <= BF16_MODEL_TOL * max(1.0, abs(res_32['loss'])), (res_i, res_32)


def test_captured_replay_equals_eager():
    """encoder_stack_infer on bf16 storage captured into a graph (one stream), replayed on new inputs == eager"""
    from feta_tmlr_amd.fused_stack import encoder_stack_infer
    model, batch9, cache = _shell('zinc', True, 3, 128, None, seed=6)
    layers = set_storage_dtype(model, BF16).encoder.layers
    n, b = batch9[0].shape[1], batch9[0].shape[0]
    g = torch.Generator().manual_seed(1)
    new_inputs = lambda: (torch.randn(n, b, 64, generator=g).cuda(), (torch.rand(b, n, n, generator=g) + 0.05).cuda(),
                          (torch.rand(n * b, generator=g) + 0.5).cuda())
    sx, spe, sdeg = new_inputs()
    n_real = cache.n_real
    with torch.inference_mode():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            encoder_stack_infer(sx, spe, sdeg, n_real, layers)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = encoder_stack_infer(sx, spe, sdeg, n_real, layers)
        for _ in range(2):
            x, pe, deg = new_inputs()
            sx.copy_(x), spe.copy_(pe), sdeg.copy_(deg)
            graph.replay()
            torch.cuda.synchronize()
            eager = encoder_stack_infer(x, pe, deg, n_real, layers)
            for name, a, e in zip(('output', 'concat', 'attn'), outs, eager):
                assert torch.isfinite(a).all() and torch.equal(a, e), name
