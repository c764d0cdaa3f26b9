"""The one-launch inference stack (feta_encoder_infer, ABI 12) on the MI355X: kernel against the fp64 eval-mode reference
at the reference's shapes, model shells under torch.inference_mode() against no_grad and fp64, and a captured replay."""
import pytest
import torch

import infer_checks as IC
from feta_tmlr_amd.transformer import data as D
from feta_tmlr_amd.transformer.models import DiffGraphTransformerGenGCN

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name,bsz,n,heads,nl,ff,batch_norm', [
    ('config2', 128, 37, 4, 3, 128, True),
    ('mutag_layernorm', 32, 28, 4, 3, 128, False),
    ('molhiv_batchnorm', 1024, 64, 4, 3, 128, True),     # more graphs than workgroups: the walking loop
    ('molhiv_layernorm', 1024, 64, 4, 3, 128, False),
])
def test_encoder_infer_matches_fp64(hip, name, bsz, n, heads, nl, ff, batch_norm):
    abi, dev, stream = hip
    errs = IC.check_infer(abi, dev, stream, bsz, n, heads, nl, ff, batch_norm, seed=11, n_min=max(1, n // 4))
    print(name, errs)


def test_zinc_default_against_the_layer_by_layer_path(hip):
    """the reference's ZINC default (8 heads, d_h = 8, 10 BatchNorm layers): ten layers of eval BatchNorm with random
    running statistics amplify every rounding (|output| ~ 10^2 - 10^3), so the bar is the error today's eval path
    (DiffTransformerEncoderLayer per layer under no_grad) makes on the same case: the new path's error against fp64 is
    at most twice that, or within the 1e-5 bar"""
    abi, dev, stream = hip
    case = IC.make_case(128, 37, 128, 10, True, seed=11, n_min=9)
    x, pe, degree, n_real, layers = case
    new = IC.run_kernel(abi, dev, stream, x, pe, degree, n_real, layers, 8, True)
    old = IC.layer_by_layer(dev, x, pe, degree, n_real, layers, 8, True)
    ref = IC.reference(x, pe, degree, n_real, layers, 8, True)
    for name, a, b, r in zip(('output', 'concat', 'attn'), new, old, ref):
        e_new, e_old = IC.KC.maxdiff(a, r), IC.KC.maxdiff(b, r)
        scale = max(1.0, r.abs().max().item())
        print('%s: |new - fp64| %.3e  |no_grad - fp64| %.3e  ratio %.2f  (scale %.1f)'
              % (name, e_new, e_old, e_new / max(e_old, 1e-30), scale))
        assert torch.isfinite(a).all() and (e_new <= 2.0 * e_old or e_new <= IC.KC.TOL * scale), name


def _shell(shape, batch_norm, heads, layers, bsz, n_max, seed, stat_spread=1.0):
    torch.manual_seed(seed)
    model = DiffGraphTransformerGenGCN(28, 1, 64, heads, dim_feedforward=128, dropout=0.0, nb_layers=layers,
                                       batch_norm=batch_norm, filter_order=4, heads_share_graph=True,
                                       filter_mode='spectral')
    IC.randomise_eval_state(model, seed, stat_spread)
    ds = D.SyntheticGraphDataset(shape, bsz, in_dim=28, seed=seed, n_max=n_max)
    n_pad = max(g.num_nodes for g in ds.samples)
    batch9, cache = D.collate(ds.samples, k_eig=min(n_pad, 16), device='cuda:0')
    return model.to('cuda:0').eval(), batch9, cache


@pytest.mark.parametrize('shape,batch_norm,heads,layers,bsz,n_max,spread', [
    ('zinc', True, 8, 10, 128, None, 0.25),     # the reference's ZINC default (run_transformer_gengcn.py:35-37)
    ('molhiv', False, 4, 3, 1024, 64, 1.0),     # the molhiv bucket of N <= 64, LayerNorm
    ('molhiv', True, 4, 3, 1024, 64, 1.0),
])
def test_model_inference_mode(monkeypatch, shape, batch_norm, heads, layers, bsz, n_max, spread):
    import feta_tmlr_amd.transformer.models as M
    model, batch9, cache = _shell(shape, batch_norm, heads, layers, bsz, n_max, seed=5, stat_spread=spread)
    seen = []
    orig = M.encoder_stack_infer

    def spy(src, pe, degree_rows, n_real, layers_, need_attn=True):
        res = orig(src, pe, degree_rows, n_real, layers_, need_attn)
        seen.append((src.clone(), res))
        return res
    monkeypatch.setattr(M, 'encoder_stack_infer', spy)
    x, mask, pe, _, degree, _, edge_index, batch, fi = batch9
    run = lambda: model(x, edge_index, batch, fi, mask, pe, degree=degree, return_filter_coeff=True, graph_cache=cache)
    with torch.inference_mode():
        out_i, _, coeff_i = run()
    with torch.no_grad():
        out_n, _, coeff_n = run()
    assert len(seen) == 1, 'the one-launch stack was not taken'
    src, (y, concat, attn) = seen[0]
    IC.check_stack_against_fp64(src.device, (y, concat, attn), model.encoder, src, pe, degree, cache.n_real)
    IC.KC.assert_close('output (inference_mode vs no_grad)', out_i, out_n.double())
    IC.KC.assert_close('coefficients (inference_mode vs no_grad)', coeff_i, coeff_n.double())


def test_captured_replay_equals_eager():
    """encoder_stack_infer captured into a graph (one stream), replayed on new inputs == the eager result"""
    from feta_tmlr_amd.fused_stack import encoder_stack_infer
    model, batch9, cache = _shell('zinc', True, 4, 3, 128, None, seed=6)
    layers = model.encoder.layers
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
                assert torch.equal(a, e), name
