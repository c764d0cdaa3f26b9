"""Checks of the one-launch inference stack (feta_encoder_infer, ABI 12) against an fp64 reference of an eval-mode
encoder stack built from oracle pieces - written once, run on the host SIMT emulation (tests/test_infer_emu.py) and on
the MI355X (tests/test_infer_gpu.py)."""
import torch
import torch.nn.functional as F

import kernel_checks as KC
from oracle import feta_oracle as O

D_MODEL = 64
EPS = 1e-5


def random_layers(nl, ff, batch_norm, seed, in_proj_bias=True, d=D_MODEL):
    """fp64 parameters of nl layers (values representable in fp32).  Every zero-initialised bias is random, and so are
    the norms: gamma, beta and - BatchNorm - running_mean and running_var (positive, away from the (0, 1) defaults that
    make an eval BatchNorm nearly the identity)."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * sc).float().double()
    layers = []
    for _ in range(nl):
        p = {'w_in': rnd(3 * d, d, sc=0.5 * d ** -0.5), 'b_in': rnd(3 * d, sc=0.2) if in_proj_bias else None,
             'w_out': rnd(d, d, sc=d ** -0.5), 'b_out': rnd(d, sc=0.2),
             'w1': rnd(ff, d, sc=d ** -0.5), 'b1': rnd(ff, sc=0.2), 'w2': rnd(d, ff, sc=ff ** -0.5), 'b2': rnd(d, sc=0.2)}
        for k in ('n1', 'n2'):
            p[k + '_gamma'] = (1.0 + rnd(d, sc=0.3)).float().double()
            p[k + '_beta'] = rnd(d, sc=0.3)
            if batch_norm:
                p[k + '_mean'] = rnd(d, sc=0.7)
                p[k + '_var'] = (0.4 + 2.0 * torch.rand(d, generator=g, dtype=torch.float64)).float().double()
        layers.append(p)
    return layers


def _norm(v, p, k, batch_norm):
    if batch_norm:
        shp = v.shape
        return F.batch_norm(v.reshape(-1, shp[-1]), p[k + '_mean'], p[k + '_var'], p[k + '_gamma'], p[k + '_beta'],
                            False, 0.0, EPS).view(shp)
    return F.layer_norm(v, (v.shape[-1],), p[k + '_gamma'], p[k + '_beta'], EPS)


def reference(x, pe, degree, n_real, layers, heads, batch_norm, tie_qk=False):
    """fp64 forward of an eval-mode stack: x [N,B,d], pe [B,N,N] or None, degree [B,N] or None, n_real [B].
    -> (output [N,B,d], concatenated heads [N,B,d], attn [B,H,N,N]) of the last layer."""
    n = x.shape[0]
    mask = torch.arange(n)[None, :] >= n_real.long()[:, None]    # key padding (a suffix)
    for p in layers:
        concat, attn, _ = O.diff_attention(x, pe, mask, p['w_in'], p['b_in'], heads, tie_qk)
        src2 = F.linear(concat, p['w_out'], p['b_out'])
        if degree is not None:
            src2 = degree.transpose(0, 1).unsqueeze(-1) * src2
        x1 = _norm(x + src2, p, 'n1', batch_norm)
        y2 = x1 + F.linear(F.relu(F.linear(x1, p['w1'], p['b1'])), p['w2'], p['b2'])
        x = _norm(y2, p, 'n2', batch_norm)
    return x, concat, attn


def make_case(bsz, n, ff, nl, batch_norm, seed=0, use_pe=True, use_degree=True, in_proj_bias=True, n_min=1):
    """fp64 inputs (fp32-representable): x [N,B,d], pe, degree, n_real (graph 0 full, the others n_min .. N), layers"""
    g = torch.Generator().manual_seed(seed + 7919)
    n_real = torch.randint(min(n_min, n), n + 1, (bsz,), generator=g, dtype=torch.int32)
    n_real[0] = n
    x = torch.randn(n, bsz, D_MODEL, generator=g).double()
    pe = (torch.rand(bsz, n, n, generator=g) + 0.05).double() if use_pe else None
    degree = (torch.rand(bsz, n, generator=g) * 2 + 0.25).double() if use_degree else None
    return x, pe, degree, n_real, random_layers(nl, ff, batch_norm, seed, in_proj_bias)


def run_kernel(abi, dev, stream, x, pe, degree, n_real, layers, heads, batch_norm, tie_qk=False, need_attn=True):
    """feta_encoder_infer on fp32 copies; outputs are poisoned with NaN first, so every element must be written"""
    n, bsz, d = x.shape
    f32 = lambda t: None if t is None else t.float().contiguous().to(dev)
    nan = float('nan')
    xf = f32(x)
    y, out = torch.full_like(xf, nan), torch.full_like(xf, nan)
    attn = torch.full((bsz, heads, n, n), nan, device=dev) if need_attn else None
    table = [dict({k: f32(v) for k, v in p.items()}, n1_eps=EPS, n2_eps=EPS, tie_qk=int(tie_qk)) for p in layers]
    rows = None if degree is None else f32(degree.transpose(0, 1).reshape(-1))
    abi.encoder_infer(bsz, n, heads, layers[0]['w1'].shape[0], table, not batch_norm, stream, x=xf, pe=f32(pe),
                      n_real=n_real.to(dev), rowscale=rows, y=y, out=out, attn=attn)
    return y, out, attn


def check_infer(abi, dev, stream, bsz, n, heads, nl, ff, batch_norm, seed=0, use_pe=True, use_degree=True,
                in_proj_bias=True, tie_qk=False, need_attn=True, n_min=1, tol=KC.TOL):
    """kernel vs the fp64 reference: last layer's output, concatenated heads, attention matrix.  -> max errors"""
    x, pe, degree, n_real, layers = make_case(bsz, n, ff, nl, batch_norm, seed, use_pe, use_degree, in_proj_bias, n_min)
    y, out, attn = run_kernel(abi, dev, stream, x, pe, degree, n_real, layers, heads, batch_norm, tie_qk, need_attn)
    ry, rout, rattn = reference(x, pe, degree, n_real, layers, heads, batch_norm, tie_qk)
    errs = {'y': KC.assert_close('y', y, ry, tol), 'concat': KC.assert_close('concat', out, rout, tol)}
    if need_attn:
        errs['attn'] = KC.assert_close('attn', attn, rattn, tol)
    return errs


def model_layer_params(encoder):
    """fp64 parameter dicts (random_layers' keys) of a model's encoder layers"""
    d64 = lambda t: None if t is None else t.detach().double().cpu()
    layers = []
    for l in encoder.layers:
        a = l.self_attn
        p = {'w_in': d64(a.in_proj_weight), 'b_in': d64(a.in_proj_bias), 'w_out': d64(a.out_proj.weight),
             'b_out': d64(a.out_proj.bias), 'w1': d64(l.linear1.weight), 'b1': d64(l.linear1.bias),
             'w2': d64(l.linear2.weight), 'b2': d64(l.linear2.bias)}
        for k, nm in (('n1', l.norm1), ('n2', l.norm2)):
            p[k + '_gamma'], p[k + '_beta'] = d64(nm.weight), d64(nm.bias)
            if l.batch_norm:
                p[k + '_mean'], p[k + '_var'] = d64(nm.running_mean), d64(nm.running_var)
        layers.append(p)
    return layers


def check_stack_against_fp64(dev, got, encoder, src, pe, degree, n_real):
    """the (output, concat, attn) a model's forward got from encoder_stack_infer against the fp64 eval-mode reference:
    within the 1e-5 bar, or - where eval BatchNorm layers amplify every rounding - at most twice the error today's eval
    path (DiffTransformerEncoderLayer per layer under no_grad) makes on the same input"""
    d64 = lambda t: None if t is None else t.detach().double().cpu()
    l0 = encoder.layers[0]
    heads, bn = l0.self_attn.num_heads, l0.batch_norm
    layers = model_layer_params(encoder)
    deg = None if degree is None else d64(degree)
    ref = reference(d64(src), d64(pe), deg, n_real.cpu(), layers, heads, bn, l0.self_attn.tie_qk)
    old = layer_by_layer(dev, d64(src), d64(pe), deg, n_real.cpu(), layers, heads, bn)
    for name, a, b, r in zip(('stack output', 'stack concat', 'stack attn'), got, old, ref):
        e_new, e_old = KC.maxdiff(a, r), KC.maxdiff(b, r)
        scale = max(1.0, r.abs().max().item())
        print('%s: |new - fp64| %.3e  |no_grad - fp64| %.3e  (scale %.1f)' % (name, e_new, e_old, scale))
        assert torch.isfinite(a).all() and (e_new <= KC.TOL * scale or e_new <= 2.0 * e_old), name


def randomise_eval_state(model, seed, stat_spread=1.0):
    """non-trivial values for every zero-initialised bias and for the norms' parameters and running statistics
    (stat_spread < 1: running statistics closer to (0, 1) - deep eval BatchNorm stacks otherwise grow without bound)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for l in model.encoder.layers:
            l.self_attn.out_proj.bias.copy_(torch.randn(l.self_attn.out_proj.bias.shape, generator=g) * 0.2)
            if l.self_attn.in_proj_bias is not None:
                l.self_attn.in_proj_bias.copy_(torch.randn(l.self_attn.in_proj_bias.shape, generator=g) * 0.2)
            for nm in (l.norm1, l.norm2):
                d = nm.weight.shape[0]
                nm.weight.copy_(1.0 + 0.3 * torch.randn(d, generator=g))
                nm.bias.copy_(0.3 * torch.randn(d, generator=g))
                if isinstance(nm, torch.nn.BatchNorm1d):
                    nm.running_mean.copy_(0.7 * stat_spread * torch.randn(d, generator=g))
                    nm.running_var.copy_(1.0 + stat_spread * (2.0 * torch.rand(d, generator=g) - 0.6))
        model.encoder.spectral_gnns.bias.copy_(torch.randn(model.encoder.spectral_gnns.bias.shape, generator=g) * 0.1)
        model.encoder.gcn.bias.copy_(torch.randn(model.encoder.gcn.bias.shape, generator=g) * 0.1)


def layer_by_layer(dev, x, pe, degree, n_real, layers, heads, batch_norm):
    """the same stack through today's eval path: DiffTransformerEncoderLayer.forward per layer under torch.no_grad()
    -> (output, concatenated heads, attn) of the last layer"""
    from feta_tmlr_amd.transformer.layers import DiffTransformerEncoderLayer
    n, bsz, d = x.shape
    f32 = lambda t: None if t is None else t.float().to(dev)
    out, pe32, deg, nr = f32(x), f32(pe), f32(degree), n_real.to(dev)
    with torch.no_grad():
        for p in layers:
            mod = DiffTransformerEncoderLayer(d, heads, p['w1'].shape[0], dropout=0.0, batch_norm=batch_norm,
                                              in_proj_bias=p['b_in'] is not None).to(dev).eval()
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
            out, attn, hd = mod(out, pe=pe32, degree=deg, need_heads=True, n_real=nr)
    return out, hd.permute(1, 0, 2, 3).reshape(n, bsz, d), attn
