"""Checks of the one-launch inference stack on bf16 storage (feta_encoder_infer_ex, dtype = FETA_BF16) - written once,
run on the host SIMT emulation (tests/test_infer_lp_emu.py) and on the MI355X (tests/test_infer_lp_gpu.py).

The bar, for each of y, concat, attn of the last layer (scale = max(1, max|ref|)):

    err_new <= BF16_TOL * scale   or   err_new <= 2 * err_today

ref: infer_checks.reference in fp64 on bf16-representable x and pe and the fp32 master weights.  today: the same layers
one by one through DiffTransformerEncoderLayer on bf16 storage under torch.no_grad() - code that does not know the new
kernel.  y and concat are compared on real rows (i < n_real[b]; nothing consumes a padded row), attn whole.  The second
branch is no blank cheque: every case carries a guard on the comparison path alone, err_today <= 2 * BF16_TOL * scale
(the bound of test_modules_emu.check_layer_attention_dropout); a case that fails it is not a usable case and fails with
that message."""
import torch

import infer_checks as IC
import kernel_checks as KC
from bench_checks import BF16_MODEL_TOL

BF16 = torch.bfloat16


def bf16_representable(t):
    return None if t is None else t.float().to(BF16).double()


def make_case(bsz, n, ff, nl, batch_norm, seed=0, **opts):
    """infer_checks.make_case with x and pe rounded to bf16, so that the path's own rounding is what is bounded"""
    x, pe, degree, n_real, layers = IC.make_case(bsz, n, ff, nl, batch_norm, seed, **opts)
    return bf16_representable(x), bf16_representable(pe), degree, n_real, layers


def run_kernel(abi, dev, stream, x, pe, degree, n_real, layers, heads, batch_norm, tie_qk=False, need_attn=True,
               in_dtype=torch.float32, dtype=BF16):
    """feta_encoder_infer_ex; x and pe travel as in_dtype; outputs are poisoned with NaN first, so every element must be
    written"""
    n, bsz, d = x.shape
    f32 = lambda t: None if t is None else t.float().contiguous().to(dev)
    tin = lambda t: None if t is None else t.float().to(in_dtype).contiguous().to(dev)
    nan = float('nan')
    y = torch.full((n, bsz, d), nan, device=dev)
    out = torch.full_like(y, nan)
    attn = torch.full((bsz, heads, n, n), nan, device=dev) if need_attn else None
    table = [dict({k: f32(v) for k, v in p.items()}, n1_eps=IC.EPS, n2_eps=IC.EPS, tie_qk=int(tie_qk)) for p in layers]
    rows = None if degree is None else f32(degree.transpose(0, 1).reshape(-1))
    abi.encoder_infer_ex(bsz, n, heads, layers[0]['w1'].shape[0], table, not batch_norm, stream, dtype=dtype, x=tin(x),
                         pe=tin(pe), n_real=n_real.to(dev), rowscale=rows, y=y, out=out, attn=attn)
    return y, out, attn


def layer_by_layer_bf16(dev, x, pe, degree, n_real, layers, heads, batch_norm, tie_qk=False):
    """today's path for a bf16-storage stack in eval(): DiffTransformerEncoderLayer.forward per layer with
    set_storage_dtype(..., bfloat16) under torch.no_grad() (the bf16 twin of infer_checks.layer_by_layer)
    -> (output, concatenated heads, attn) of the last layer"""
    from feta_tmlr_amd.transformer.layers import DiffTransformerEncoderLayer, set_storage_dtype
    n, bsz, d = x.shape
    f32 = lambda t: None if t is None else t.float().to(dev)
    out, deg, nr = f32(x).to(BF16), f32(degree), n_real.to(dev)
    pe16 = None if pe is None else f32(pe).to(BF16)
    with torch.no_grad():
        for p in layers:
            mod = DiffTransformerEncoderLayer(d, heads, p['w1'].shape[0], dropout=0.0, batch_norm=batch_norm,
                                              tie_qk=tie_qk, in_proj_bias=p['b_in'] is not None).to(dev).eval()
            a = mod.self_attn
            pairs = [(a.in_proj_weight, 'w_in'), (a.in_proj_bias, 'b_in'), (a.out_proj.weight, 'w_out'),
                     (a.out_proj.bias, 'b_out'), (mod.linear1.weight, 'w1'), (mod.linear1.bias, 'b1'),
                     (mod.linear2.weight, 'w2'), (mod.linear2.bias, 'b2')]
            for k, nm in (('n1', mod.norm1), ('n2', mod.norm2)):
                pairs += [(nm.weight, k + '_gamma'), (nm.bias, k + '_beta')]
                if batch_norm:
                    pairs += [(nm.running_mean, k + '_mean'), (nm.running_var, k + '_var')]
            for t, k in pairs:
                if t is not None:
                    t.copy_(p[k])
            set_storage_dtype(mod, BF16)
            out, attn, hd = mod(out, pe=pe16, degree=deg, need_heads=True, n_real=nr)
    return out.float(), hd.permute(1, 0, 2, 3).reshape(n, bsz, d).float(), attn.float()


def real_rows(t, n_real):
    """[N,B,d] with the rows i >= n_real[b] zeroed"""
    n = t.shape[0]
    keep = (torch.arange(n)[:, None] < n_real.long().cpu()[None, :]).unsqueeze(-1)
    return torch.where(keep, t.detach().double().cpu(), torch.zeros((), dtype=torch.float64))


def assert_bar(what, new, today, ref, n_real, need_attn=True):
    """the two-branch bar with its guard for (y, concat, attn); prints every figure before it asserts.  -> figures"""
    figures = {}
    for name, a, b, r in zip(('y', 'concat', 'attn'), new, today, ref):
        if name == 'attn':
            if not need_attn:
                continue
            a, b, r = a.detach().double().cpu(), b.detach().double().cpu(), r.double()
        else:
            a, b, r = real_rows(a, n_real), real_rows(b, n_real), real_rows(r, n_real)
        e_new, e_today = KC.maxdiff(a, r), KC.maxdiff(b, r)
        scale = max(1.0, r.abs().max().item())
        figures[name] = (e_new, e_today, scale)
        print('%s %s: err_new %.3e  err_today %.3e  scale %.2f  (new / scale %.2e, today / scale %.2e)'
              % (what, name, e_new, e_today, scale, e_new / scale, e_today / scale))
    for name, (e_new, e_today, scale) in figures.items():
        assert e_today <= 2.0 * KC.BF16_TOL * scale, \
            '%s %s: not a usable case - the comparison path itself is off by %.3e (scale %.2f)' % (what, name, e_today, scale)
    for name, a in zip(('y', 'concat', 'attn'), new):
        if a is not None:
            assert torch.isfinite(a).all(), '%s %s: not finite / not every element written' % (what, name)
    for name, (e_new, e_today, scale) in figures.items():
        assert e_new <= KC.BF16_TOL * scale or e_new <= 2.0 * e_today, \
            '%s %s: err_new %.3e against bar %.3e / twice today %.3e' % (what, name, e_new, KC.BF16_TOL * scale,
                                                                         2.0 * e_today)
    return figures


def check_infer_lp(abi, dev, stream, bsz, n, nl, ff, batch_norm, seed=0, in_dtype=torch.float32, tie_qk=False,
                   need_attn=True, heads=4, **opts):
    """bf16 kernel vs the fp64 reference under the bar above.  -> figures"""
    x, pe, degree, n_real, layers = make_case(bsz, n, ff, nl, batch_norm, seed, **opts)
    new = run_kernel(abi, dev, stream, x, pe, degree, n_real, layers, heads, batch_norm, tie_qk, need_attn, in_dtype)
    today = layer_by_layer_bf16(dev, x, pe, degree, n_real, layers, heads, batch_norm, tie_qk)
    ref = IC.reference(x, pe, degree, n_real, layers, heads, batch_norm, tie_qk)
    what = 'B=%d N=%d L=%d ff=%d %s in=%s' % (bsz, n, nl, ff, 'BN' if batch_norm else 'LN',
                                               'bf16' if in_dtype == BF16 else 'fp32')
    return assert_bar(what, new, today, ref, n_real, need_attn)


def check_stack_against_fp64_lp(dev, got, encoder, src, pe, degree, n_real):
    """what a bf16-storage model's forward got from encoder_stack_infer against the fp64 eval-mode reference, from the
    model's own parameters: the bar above.  src and pe are what the stack was given (fp32): the reference and today's
    path consume their bf16 roundings, the values the launch stages."""
    d64 = lambda t: None if t is None else t.detach().double().cpu()
    l0 = encoder.layers[0]
    heads, bn, tie = l0.self_attn.num_heads, l0.batch_norm, l0.self_attn.tie_qk
    layers = IC.model_layer_params(encoder)
    x, p, deg = bf16_representable(d64(src)), bf16_representable(d64(pe)), d64(degree)
    ref = IC.reference(x, p, deg, n_real.cpu(), layers, heads, bn, tie)
    today = layer_by_layer_bf16(dev, x, p, deg, n_real.cpu(), layers, heads, bn, tie)
    return assert_bar('stack', got, today, ref, n_real)


def assert_model_output(name, out_new, out_today, out_f32):
    """final output of a bf16-storage model under inference_mode against the SAME weights on fp32 storage under
    inference_mode: within BF16_MODEL_TOL (relative to max(1, max|out|)), or within twice the distance of today's
    bf16 no_grad output from that fp32 twin"""
    e_new, e_today = KC.maxdiff(out_new, out_f32), KC.maxdiff(out_today, out_f32)
    scale = max(1.0, out_f32.detach().abs().max().item())
    print('%s: |bf16 inference_mode - fp32| %.3e  |bf16 no_grad - fp32| %.3e  scale %.2f' % (name, e_new, e_today, scale))
    assert torch.isfinite(out_new).all(), name
    assert e_new <= BF16_MODEL_TOL * scale or e_new <= 2.0 * e_today, name
    return e_new, e_today, scale
