"""The filter stage of a forward as one autograd node (functional.FilterStageFn): gradients that a hook, retain_grad or a
second consumer reads while the backward pass is still running are finished values, on leaf inputs and on the per-layer model
path; and the launches of a step are the ones the stage made while it was three nodes.  Written once, run on the host
emulation and on the MI355X."""
import torch
import torch.nn.functional as F

import coeff_saved_checks as CS
import heads8_cat_checks as H8
import kernel_checks as KC
from feta_tmlr_amd import functional as FF
from oracle import feta_oracle as O

GRAD_TOL = 3e-5      # the project's bar for gradients (output and coefficients: KC.TOL)
PARAMS = ('gcn.weight', 'gcn.bias', 'linear.weight', 'linear.bias', 'spectral_gnns.bias', 'linear_cat.weight',
          'linear_cat.bias')


def _rel(got, ref):
    return KC.maxdiff(got, ref) / max(1.0, ref.abs().max().item())


def stage_inputs(dev, heads, seed=0):
    """the encoder of the small model (3 graphs of 9 to 32 nodes, d = 64, K = N_pad) and random stage inputs of its shapes:
    stack output rows y2 [N,B,d], per-head rows concat [N,B,d], attn [B,H,N,N] row-stochastic on the real blocks"""
    model, batch9, cache = (CS.headline_model(dev, bsz=3, layers=2) if heads == 4 else H8.model8(dev, True))
    enc, mask = model.encoder, batch9[1]
    n, bsz, d = mask.shape[1], mask.shape[0], 64
    g = torch.Generator().manual_seed(seed + 11)
    y2 = torch.randn(n, bsz, d, generator=g, dtype=torch.float64)
    concat = torch.randn(n, bsz, d, generator=g, dtype=torch.float64)
    attn, _ = KC.random_attention(bsz, heads, n, cache.n_real.cpu().long(), g)
    w = [torch.rand(n, bsz, d, generator=g, dtype=torch.float64) + 0.5 for _ in range(3)]
    return enc, mask.cpu(), cache, y2, concat, attn, w


def oracle_stage(enc, mask, cache, y2, concat, attn, w, heads):
    """fp64: (out, coeff, gradients of y2, concat and the seven parameters) of the loss run_stage takes"""
    n, bsz, d = y2.shape
    p = {k: dict(enc.named_parameters())[k].detach().cpu().double().requires_grad_(True) for k in PARAMS}
    y2r, cr = y2.clone().requires_grad_(True), concat.clone().requires_grad_(True)
    coeff = O.get_filter_coefficients_collapsed(attn, mask, p['gcn.weight'], p['gcn.bias'], p['linear.weight'],
                                                p['linear.bias'])
    oh = cr.view(n, bsz, heads, d // heads).permute(1, 0, 2, 3)
    filt = O.filter_stage_eigenbasis(oh, coeff, cache.u.cpu().double(), cache.lam.cpu().double(), mask,
                                     p['spectral_gnns.bias'], enc.order, True)
    out = F.linear(torch.cat((y2r, filt), dim=-1), p['linear_cat.weight'], p['linear_cat.bias'])
    ((out * w[0]).sum() + 0.01 * coeff.pow(2).sum() + (y2r * w[1]).sum() + (cr * w[2]).sum()).backward()
    grads = {k: v.grad for k, v in p.items()}
    grads.update(y2=y2r.grad, concat=cr.grad)
    return out.detach(), coeff.reshape(heads * bsz, -1).detach(), grads


def run_stage(abi, dev, hook, enc, cache, y2, concat, attn, w, heads, fold):
    """filter_stage on leaf inputs that carry retain_grad, a cloning hook and a second consumer each"""
    n, bsz, d = y2.shape
    for q in enc.parameters():
        q.grad = None
    y2l, cl = (t.float().to(dev).requires_grad_(True) for t in (y2, concat))
    seen = {}
    for name, t in (('y2', y2l), ('concat', cl)):
        t.retain_grad()
        t.register_hook(lambda g_, name=name: seen.setdefault(name, g_.detach().clone()))
    w32 = [t.float().to(dev) for t in w]
    with hook(), CS.Counter(abi) as c:
        out, coeff = FF.filter_stage(y2l, cl.view(n, bsz, heads, d // heads).permute(1, 0, 2, 3), enc.gcn.weight, enc.gcn.bias,
                                     enc.linear.weight, enc.linear.bias, enc.spectral_gnns.bias, enc.linear_cat.weight,
                                     enc.linear_cat.bias, attn.float().to(dev), cache.n_real, (cache.u, cache.lam), 'spec',
                                     enc.order, True, cat='fold' if fold else 'rows')
        ((out * w32[0]).sum() + 0.01 * coeff.pow(2).sum() + (y2l * w32[1]).sum() + (cl * w32[2]).sum()).backward()
    assert ('feta_spec_filter_cat_bwd' in c.calls) == fold and ('feta_rowlin_bwd_ex' in c.calls) == (not fold), c.calls
    grads = {k: dict(enc.named_parameters())[k].grad.detach().clone() for k in PARAMS}
    grads.update(y2=y2l.grad.detach().clone(), concat=cl.grad.detach().clone())
    return out.detach(), coeff.detach(), grads, seen


def check_leaf_inputs(abi, dev, hook, monkeypatch, heads):
    """C1: what a hook on an input of the stage sees is the gradient that input ends up with, bit for bit; both input
    gradients and the seven parameter gradients against fp64 at the project's bars, with the fold and without; the folded
    path's error within GUARD_FACTOR x the unfolded path's (floor GUARD_FLOOR)"""
    monkeypatch.setattr(FF, 'USE_CAT_FOLD', True)
    monkeypatch.setattr(FF, 'USE_CAT_FOLD_BWD', True)
    enc, mask, cache, y2, concat, attn, w = stage_inputs(dev, heads)
    ref = oracle_stage(enc, mask, cache, y2, concat, attn, w, heads)
    errs = {}
    for fold in (True, False):
        out, coeff, grads, seen = run_stage(abi, dev, hook, enc, cache, y2, concat, attn, w, heads, fold)
        tag = ' (%d heads, fold %s)' % (heads, 'on' if fold else 'off')
        for name in ('y2', 'concat'):
            assert torch.equal(seen[name], grads[name]), 'the hook on %s saw unfinished values%s' % (name, tag)
        KC.assert_close('stage output' + tag, out, ref[0])
        KC.assert_close('stage coefficients' + tag, coeff, ref[1])
        for k, gk in grads.items():
            KC.assert_close('stage grad %s%s' % (k, tag), gk, ref[2][k], tol=GRAD_TOL)
        errs[fold] = dict(output=_rel(out, ref[0]), coefficients=_rel(coeff, ref[1]),
                          **{k: _rel(gk, ref[2][k]) for k, gk in grads.items()})
    print('stage on leaf inputs, %d heads: ' % heads
          + ', '.join('%s %.2e / %.2e' % (k, errs[True][k], errs[False][k]) for k in errs[True]))
    for k in errs[True]:
        assert errs[True][k] <= max(KC.GUARD_FACTOR * errs[False][k], KC.GUARD_FLOOR), (k, errs[True][k], errs[False][k])
    return errs


def check_per_layer_hook(abi, dev, hook, monkeypatch):
    """C2: fused_stack = False with the fold on; a cloning hook and retain_grad on the stack output inside the encoder (the
    first operand of linear_cat) see the gradient that tensor ends up with, and the step matches the fp64 oracle"""
    monkeypatch.setattr(FF, 'USE_CAT_FOLD_BWD', True)
    model, batch9, cache = CS.headline_model(dev, bsz=3, layers=2)
    enc = model.encoder
    enc.fused_stack = False
    ref = _oracle_step4(model, batch9)
    res, hooked, errs = {}, {}, {}
    for fold in (True, False):
        monkeypatch.setattr(FF, 'USE_CAT_FOLD', fold)
        caught, seen = [], []

        def layer_hook(mod, args, result):
            caught.append(result[0])
            result[0].retain_grad()
            result[0].register_hook(lambda g_: seen.append(g_.detach().clone()))
        h = enc.layers[-1].register_forward_hook(layer_hook)
        try:
            with CS.Counter(abi) as c:
                res[fold] = CS.run_step(model, batch9, cache, hook)
        finally:
            h.remove()
        assert ('feta_spec_filter_cat_bwd' in c.calls) == fold and 'feta_bn_bwd' in c.calls, c.calls
        assert len(caught) == 1 and len(seen) == 1
        assert bool(torch.isfinite(seen[0]).all()) and torch.equal(seen[0], caught[0].grad), \
            'the hook on the stack output saw unfinished values (fold %s)' % fold
        hooked[fold] = seen[0]
        tag = ' (per-layer, fold %s)' % ('on' if fold else 'off')
        KC.assert_close('model output' + tag, res[fold][0], ref[0])
        KC.assert_close('coefficients' + tag, res[fold][1], ref[1])
        assert res[fold][2].keys() == ref[2].keys()
        for k, gk in res[fold][2].items():
            KC.assert_close('grad %s%s' % (k, tag), gk, ref[2][k], tol=GRAD_TOL)
        errs[fold] = dict(output=_rel(res[fold][0], ref[0]), coefficients=_rel(res[fold][1], ref[1]),
                          **{k: _rel(gk, ref[2][k]) for k, gk in res[fold][2].items()})
    # (the oracle does not expose the stack output: the hooked gradient is held against the unfolded path's, two fp32 results
    # of one quantity that are each held to GRAD_TOL)
    KC.assert_close('hooked gradient of the stack output, fold on / off', hooked[True], hooked[False].double(), tol=GRAD_TOL)
    for k in errs[True]:
        assert errs[True][k] <= max(KC.GUARD_FACTOR * errs[False][k], KC.GUARD_FLOOR), (k, errs[True][k], errs[False][k])


def _oracle_step4(model, batch9):
    """heads8_cat_checks.oracle_step for the 4-head model"""
    x, mask, pe, _, degree, _, edge_index, batch, fi = [None if t is None else t.cpu() for t in batch9]
    p64 = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items()
           if v.dtype.is_floating_point and 'running_' not in k}
    out_ref, coeff_ref = O.graph_transformer_gengcn(x.double(), edge_index, batch, fi, mask, pe.double(), degree.double(), p64,
                                                    num_layers=2, num_heads=4, order=4, batch_norm=True, heads_share_graph=True)
    w = torch.linspace(0.5, 1.5, out_ref.numel(), dtype=torch.float64).view_as(out_ref)
    ((out_ref * w).sum() + 0.01 * coeff_ref.pow(2).sum()).backward()
    return out_ref.detach(), coeff_ref.detach(), {k: v.grad for k, v in p64.items() if v.grad is not None}


# C3: what headline_model(bsz=3, layers=2) launches through the C ABI in one step (forward | backward), taken from the
# three-node implementation this one replaces - not from the code under test
_STACK_F = 'attn_block_fwd_sums ffn_fwd attn_block_fwd ffn_fwd_coeff'
_STACK_B = 'attn_block_bwd ffn_bwd attn_block_bwd_sums colsum_multi'
_LAYER_F = 'rowlin_fwd attn_fwd rowlin_fwd_ex bn_apply_fwd rowlin_fwd rowlin_fwd_ex bn_apply_fwd'
_LAYER_B = 'bn_bwd rowlin_bwd rowlin_bwd bn_bwd rowlin_bwd attn_bwd rowlin_bwd'
CALL_LISTS = {
    (True, True): _STACK_F + ' lin_fwd spec_filter_cat_fwd_coeff | spec_filter_cat_bwd lin_bwd ffn_bwd_coeff_saved ' + _STACK_B,
    (True, False): _STACK_F + ' lin_fwd spec_filter_fwd rowlin_fwd_ex | rowlin_bwd_ex spec_filter_bwd lin_bwd ffn_bwd_coeff '
    + _STACK_B,
    (False, True): ' '.join([_LAYER_F] * 2) + ' colsum coeff_fwd lin_fwd spec_filter_cat_fwd_coeff | spec_filter_cat_bwd lin_bwd '
    'coeff_bwd_saved ' + ' '.join([_LAYER_B] * 2),
    (False, False): ' '.join([_LAYER_F] * 2) + ' colsum coeff_fwd lin_fwd spec_filter_fwd rowlin_fwd_ex | rowlin_bwd_ex '
    'spec_filter_bwd lin_bwd coeff_bwd ' + ' '.join([_LAYER_B] * 2),
}
CALL_COUNTS = {(True, True): 13, (True, False): 15, (False, True): 35, (False, False): 37}


def check_call_list(abi, dev, hook, monkeypatch, fused, fold):
    monkeypatch.setattr(FF, 'USE_CAT_FOLD', fold)
    monkeypatch.setattr(FF, 'USE_CAT_FOLD_BWD', True)
    monkeypatch.setattr(FF, 'USE_COEFF_DSUM', True)
    model, batch9, cache = CS.headline_model(dev, bsz=3, layers=2)
    model.encoder.fused_stack = fused
    with CS.Counter(abi) as c:
        CS.run_step(model, batch9, cache, hook)
    want = ['feta_' + k for k in CALL_LISTS[(fused, fold)].split() if k != '|']
    assert len(want) == CALL_COUNTS[(fused, fold)]
    assert c.calls == want, (c.calls, want)
