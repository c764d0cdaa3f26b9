"""Checks of the 8-head (d_h = 8) form of the fused attention-block kernels (ABI 13: feta_attn_block.H /
feta_attn_block_grad.H, csrc/block.hip, csrc/block_bwd.hip) - kernel_checks._ln_block_case, check_attn_block_ln,
check_attn_block_bwd_ln and check_attn_block_bwd_lp generalised to a `heads` argument.  The reference is the fp64
oracle.attention_core plus autograd, the tolerance kernel_checks.TOL; written once, run on the host emulation
(test_heads8_emu.py) and on the MI355X (test_heads8_gpu.py).  fp32 storage only: that is all the 8-head form has."""
import torch
import torch.nn.functional as F

import kernel_checks as KC
from oracle import feta_oracle as O

D_MODEL = 64


def block_case(heads, bsz, n_pad, n_min, seed, with_pe=True):
    """Inputs of one attention sub-block at d = 64: pre-norm rows x0 [N,B,64] (real values on padded rows too), pe, degree,
    weights, the affine pair of a LayerNorm and the parameter block [scale | shift | mean | rstd] of a BatchNorm in front of
    it.  Graph 0 is full (n_real = N_pad), graph 1 - where there is one - has a single real node."""
    g = torch.Generator().manual_seed(seed)
    d = D_MODEL
    n_real = torch.randint(n_min, n_pad + 1, (bsz,), generator=g)
    n_real[0] = n_pad
    if bsz > 1:
        n_real[1] = 1
    mask = torch.arange(n_pad)[None, :] >= n_real[:, None]                     # [B,N] True = pad
    x0 = (torch.randn(n_pad, bsz, d, generator=g) * 0.8 + 0.1).float().double()
    pe = None
    if with_pe:
        pe = torch.rand(bsz, n_pad, n_pad, generator=g).double() + 0.1
        pe = (pe * (~mask).unsqueeze(1) * (~mask).unsqueeze(2)).float().double()
    degree = ((torch.rand(bsz, n_pad, generator=g).double() * 0.5 + 0.5) * (~mask)).float().double()
    p = dict(w_in=torch.randn(3 * d, d, generator=g).double() / 8, b_in=torch.randn(3 * d, generator=g).double() * 0.1,
             w_out=torch.randn(d, d, generator=g).double() / 8, b_out=torch.randn(d, generator=g).double() * 0.1)
    p = {k: v.float().double() for k, v in p.items()}
    gam0 = (torch.rand(d, generator=g) + 0.5).float().double()
    bet0 = (torch.randn(d, generator=g) * 0.1).float().double()
    bn0 = torch.zeros(4, d, dtype=torch.float64)
    bn0[0] = torch.rand(d, generator=g) + 0.5
    bn0[1] = torch.randn(d, generator=g) * 0.2
    bn0[2] = torch.randn(d, generator=g) * 0.1
    bn0[3] = torch.rand(d, generator=g) + 0.5
    bn0 = bn0.float().double()
    return dict(g=g, d=d, heads=heads, n_real=n_real.to(torch.int32), mask=mask, x0=x0, pe=pe, degree=degree, p=p,
                gam0=gam0, bet0=bet0, bn0=bn0, bsz=bsz, n_pad=n_pad)


def _seen(c, norm):
    """the layer input as the kernel sees x0: through a LayerNorm ('ln'), a BatchNorm parameter block ('bn') or raw (None)"""
    if norm == 'ln':
        return F.layer_norm(c['x0'], (c['d'],), c['gam0'], c['bet0'], 1e-5)
    if norm == 'bn':
        return c['x0'] * c['bn0'][0] + c['bn0'][1]
    return c['x0']


def _norm_kw(c, norm, f32):
    if norm == 'ln':
        return dict(x_ln_gamma=f32(c['gam0']), x_ln_beta=f32(c['bet0']))
    if norm == 'bn':
        return dict(x_bn=f32(c['bn0']))
    return {}


def run_forward(abi, dev, stream, c, norm, need_attn=False, stats=False, tie_qk=False, rowscale=True):
    """feta_attn_block_fwd with H = heads on the case -> the tensors it wrote"""
    d, heads, bsz, n_pad = c['d'], c['heads'], c['bsz'], c['n_pad']
    m = n_pad * bsz
    f32 = lambda t: t.detach().float().contiguous().to(dev)
    new = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    t = dict(qkv=new(m, 3 * d), out=new(m, d), y=new(m, d), ast=new(bsz, heads, n_pad, 2),
             attn=new(bsz, heads, n_pad, n_pad) if need_attn else None,
             st=new(abi.attn_block_stat_rows(bsz, n_pad) + 1, 2, d) if stats else None)
    abi.attn_block_fwd(bsz, n_pad, float(d // heads) ** -0.5, stream, heads=heads, tie_qk=tie_qk, x=f32(c['x0']).view(m, d),
                       w_in=f32(c['p']['w_in']), b_in=f32(c['p']['b_in']), w_out=f32(c['p']['w_out']),
                       b_out=f32(c['p']['b_out']), pe=None if c['pe'] is None else f32(c['pe']), n_real=c['n_real'].to(dev),
                       rowscale=f32(c['degree'].t().reshape(m)) if rowscale else None, qkv=t['qkv'], out=t['out'],
                       attn_stats=t['ast'], attn=t['attn'], y=t['y'], y_stats=t['st'], **_norm_kw(c, norm, f32))
    return t


def check_fwd(abi, dev, stream, heads=8, bsz=3, n_pad=21, n_min=3, seed=0, with_pe=True, norm='ln', need_attn=True,
              stats=False, tie_qk=False, rowscale=True):
    """feta_attn_block_fwd, H = heads, against the fp64 oracle of in_proj -> attention -> out_proj -> degree -> residual:
    qkv (real rows), the concatenated head outputs, y, attn [B,H,N,N] and the BatchNorm partial sums of y."""
    c = block_case(heads, bsz, n_pad, n_min, seed, with_pe)
    d, m, p = c['d'], n_pad * bsz, c['p']
    t = run_forward(abi, dev, stream, c, norm, need_attn, stats, tie_qk, rowscale)
    x = _seen(c, norm)
    qkv_ref = F.linear(x, p['w_in'], p['b_in'])
    if tie_qk:       # K is Q (the K part of qkv is not written)
        qkv_ref = torch.cat([qkv_ref[..., :d], qkv_ref[..., :d], qkv_ref[..., 2 * d:]], dim=-1)
    concat, a_ref, _ = O.attention_core(qkv_ref, c['pe'], c['mask'], heads)
    deg = c['degree'].t().unsqueeze(-1) if rowscale else 1.0
    y_ref = x + deg * F.linear(concat, p['w_out'], p['b_out'])
    real = (~c['mask']).t().unsqueeze(-1)       # k / v rows of key tiles without a real node are never written
    zero = torch.zeros((), dtype=torch.float64)
    got_qkv = t['qkv'].view(n_pad, bsz, 3 * d).cpu().double()
    if tie_qk:
        got_qkv = torch.cat([got_qkv[..., :d], got_qkv[..., :d], got_qkv[..., 2 * d:]], dim=-1)
    errs = {'qkv': KC.assert_close('h%d block qkv' % heads, torch.where(real, got_qkv, zero),
                                   torch.where(real, qkv_ref, zero))}
    errs['out'] = KC.assert_close('h%d block out' % heads, t['out'].view(n_pad, bsz, d), concat)
    errs['y'] = KC.assert_close('h%d block y' % heads, t['y'].view(n_pad, bsz, d), y_ref)
    if need_attn:
        assert tuple(t['attn'].shape) == (bsz, heads, n_pad, n_pad)
        errs['attn'] = KC.assert_close('h%d block attn' % heads, t['attn'], a_ref)
    if stats:
        yr = y_ref.reshape(m, d)
        errs['sum'] = KC.assert_close('h%d block y_stats sum' % heads, t['st'][:-1, 0].sum(0), yr.sum(0))
        errs['sumsq'] = KC.assert_close('h%d block y_stats sumsq' % heads, t['st'][:-1, 1].sum(0), (yr * yr).sum(0))
    print('heads8 fwd', dict(n_pad=n_pad, bsz=bsz, norm=norm), {k: '%.2e' % v for k, v in errs.items()})
    return errs


def check_bwd(abi, dev, stream, heads=8, bsz=3, n_pad=21, n_min=3, seed=0, with_pe=True, form='ln', first_layer=False,
              split=False, with_dout2=True):
    """feta_attn_block_bwd, H = heads, on the tensors its own forward saved (qkv, out, attn_stats), against fp64 autograd of
    o1 = Norm1(x + degree * out_proj(attention(in_proj(x)))), x = x0 seen through the norm in front of the layer (none:
    first_layer).  form 'ln': LayerNorm stack (ln1_gamma / x0_ln_gamma; [dgamma1 | dbeta1] in the partial rows); form 'bn':
    BatchNorm stack (bn1 / g_sum finalized by the launch -> dgamma, dbeta; bn0 / sum_out for the previous BatchNorm).
    dx (dx + dx_b: split), dW_out, db_out, dW_in, db_in from the summed partial rows."""
    c = block_case(heads, bsz, n_pad, n_min, seed, with_pe)
    g, d, m, p, mask = c['g'], c['d'], n_pad * bsz, c['p'], c['mask']
    norm0 = None if first_layer else form
    f32 = lambda t: t.detach().float().contiguous().to(dev)
    new = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
    t = run_forward(abi, dev, stream, c, norm0, stats=(form == 'bn'))
    w = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    x = _seen(c, norm0).detach().requires_grad_(True)
    qkv_ref = F.linear(x, w['w_in'], w['b_in'])
    concat, _, _ = O.attention_core(qkv_ref, c['pe'], mask, heads, detach_max=True)
    y1 = x + c['degree'].t().unsqueeze(-1) * F.linear(concat, w['w_out'], w['b_out'])
    gam1 = (torch.rand(d, generator=g) + 0.5).float().double().requires_grad_(True)
    bet1 = (torch.randn(d, generator=g) * 0.1).float().double().requires_grad_(True)
    dy = torch.randn(n_pad, bsz, d, generator=g).float().double()
    dout2 = (torch.randn(n_pad, bsz, d, generator=g).double() * (~mask).t().unsqueeze(-1)).float().double()
    extra = (concat * dout2).sum() if with_dout2 else 0.0
    gb = abi.attn_block_bwd_blocks(bsz)
    kw = {}
    if form == 'ln':
        ((F.layer_norm(y1, (d,), gam1, bet1, 1e-5) * dy).sum() + extra).backward()
        ld = 4 * d * d + 4 * d + 2 * d
        kw = dict(y1=t['y'], ln1_gamma=f32(gam1), ln_eps=1e-5)
        if not first_layer:
            kw.update(x0_ln_gamma=f32(c['gam0']), x0_ln_beta=f32(c['bet0']))
    else:
        o1 = F.batch_norm(y1.reshape(m, d), None, None, gam1, bet1, True, 0.1, 1e-5)
        ((o1 * dy.reshape(m, d)).sum() + extra).backward()
        ld = 4 * d * d + 4 * d
        y1s = t['y'].cpu().double()                       # what the forward stored
        mean1, var1 = y1.detach().reshape(m, d).mean(0), y1.detach().reshape(m, d).var(0, unbiased=False)
        rstd1 = (var1 + 1e-5).rsqrt()
        bn1 = torch.stack([gam1.detach() * rstd1, -mean1 * gam1.detach() * rstd1, mean1, rstd1])
        dyf = dy.reshape(m, d)
        gsum = torch.stack([dyf.sum(0), (dyf * ((y1s - mean1) * rstd1)).sum(0)]).unsqueeze(0)
        kw = dict(y1=t['y'], bn1=f32(bn1), g_sum=f32(gsum), Gs=1, fin_out=new(2, d), dgamma=new(d), dbeta=new(d))
        if not first_layer:
            kw.update(bn0=f32(c['bn0']), sum_out=new(2 * gb, 2, d))
    partial = new(gb, ld)
    dx = new(m, d)
    dxb = new(m, d) if split else None
    abi.attn_block_bwd(bsz, n_pad, float(d // heads) ** -0.5, stream, heads=heads, partial=partial, dy=f32(dy).view(m, d),
                       rowscale=f32(c['degree'].t().reshape(m)), w_out=f32(p['w_out']), w_in=f32(p['w_in']), qkv=t['qkv'],
                       out=t['out'], dout2=f32(dout2).view(m, d) if with_dout2 else None,
                       pe=None if c['pe'] is None else f32(c['pe']), n_real=c['n_real'].to(dev), attn_stats=t['ast'],
                       x0=f32(c['x0']).view(m, d), dx=dx, dx_b=dxb, **kw)
    got = dx.view(n_pad, bsz, d).cpu().double()
    if split:
        got = got + dxb.view(n_pad, bsz, d).cpu().double()
    name = 'h%d %s block ' % (heads, form)
    errs = {'dx': KC.assert_close(name + 'dx', got, x.grad)}
    pw = partial.double().sum(0).cpu()
    o = 0
    refs = [('dW_out', w['w_out'].grad), ('db_out', w['b_out'].grad), ('dW_in', w['w_in'].grad), ('db_in', w['b_in'].grad)]
    if form == 'ln':
        refs += [('dgamma1', gam1.grad), ('dbeta1', bet1.grad)]
    for k, ref in refs:
        errs[k] = KC.assert_close(name + k, pw[o:o + ref.numel()].view(ref.shape), ref)
        o += ref.numel()
    if form == 'bn':
        errs['dgamma1'] = KC.assert_close(name + 'dgamma1', kw['dgamma'], gam1.grad)
        errs['dbeta1'] = KC.assert_close(name + 'dbeta1', kw['dbeta'], bet1.grad)
        if not first_layer:
            xh0 = (c['x0'] - c['bn0'][2]) * c['bn0'][3]
            so = kw['sum_out']
            errs['sum dx'] = KC.assert_close(name + 'sum dx', so[:, 0].sum(0), x.grad.reshape(m, d).sum(0))
            errs['sum dx xhat'] = KC.assert_close(name + 'sum dx xhat', so[:, 1].sum(0), (x.grad * xh0).reshape(m, d).sum(0))
    print('heads8 bwd', dict(n_pad=n_pad, bsz=bsz, form=form, split=split, first=first_layer),
          {k: '%.2e' % v for k, v in errs.items()})
    return errs


# ---- stack level ----------------------------------------------------------------------------------------------------
def model8(batch_norm, layers=2, seed=5, heads=8):
    from feta_tmlr_amd.transformer.models import DiffGraphTransformerGenGCN
    torch.manual_seed(seed)
    model = DiffGraphTransformerGenGCN(9, 1, 64, heads, dim_feedforward=128, dropout=0.0, nb_layers=layers,
                                       batch_norm=batch_norm, filter_order=2, heads_share_graph=True,
                                       filter_mode='spectral')
    with torch.no_grad():
        for l in model.encoder.layers:
            l.self_attn.out_proj.bias.normal_(0, 0.1)
            if l.self_attn.in_proj_bias is not None:
                l.self_attn.in_proj_bias.normal_(0, 0.1)
            l.norm1.weight.normal_(1.0, 0.2)
            l.norm1.bias.normal_(0, 0.1)
            l.norm2.weight.normal_(1.0, 0.2)
            l.norm2.bias.normal_(0, 0.1)
    return model


def batch_of(dev, shape='zinc', bsz=3, n_min=20, n_max=37, seed=3):
    from feta_tmlr_amd.transformer import data as D
    ds = D.SyntheticGraphDataset(shape, bsz, in_dim=9, seed=seed, pos_enc=True, n_min=n_min, n_max=n_max)
    n_pad = max(g.num_nodes for g in ds.samples)
    return D.collate(ds.samples, k_eig=n_pad, device=dev)


def check_stack_equals_three_launches(dev, hook, monkeypatch, batch_norm, shape='zinc', n_min=20, n_max=37, bsz=3):
    """an 8-head stack through the one-launch block kernels == the same stack with the attention half run as three
    launches per layer and direction (test_modules_emu.check_attn_block_equals_three_launches, built for 8 heads)"""
    import test_modules_emu as TM
    model = model8(batch_norm).to(dev)
    batch9, cache = batch_of(dev, shape, bsz, n_min, n_max)
    a = TM._stack_run(model, batch9, cache, True, monkeypatch, hook)
    b = TM._stack_run(model, batch9, cache, False, monkeypatch, hook)
    KC.assert_close('output', a[0], b[0].double(), tol=2e-6)
    KC.assert_close('coefficients', a[1], b[1].double(), tol=2e-6)
    TM.assert_close_up_to_relu_flips('dx', a[2], b[2].double(), tol=1e-5, max_rows=0)
    assert a[3].keys() == b[3].keys()
    for k in a[3]:
        KC.assert_close('grad ' + k, a[3][k], b[3][k].double(), tol=1e-5)


class counted_calls:
    """counts the calls of the named Abi methods inside the block"""

    def __init__(self, abi, names):
        self.abi, self.names, self.calls = abi, names, {}

    def __enter__(self):
        self.orig = {k: getattr(self.abi, k) for k in self.names}

        def counted(k):
            def f(*a, **kw):
                self.calls[k] = self.calls.get(k, 0) + 1
                return self.orig[k](*a, **kw)
            return f
        for k in self.names:
            setattr(self.abi, k, counted(k))
        return self.calls

    def __exit__(self, *exc):
        for k in self.names:
            setattr(self.abi, k, self.orig[k])
        return False


LAUNCH_NAMES = ('layernorm_fwd', 'layernorm_bwd', 'attn_block_fwd', 'ffn_fwd', 'ffn_bwd', 'attn_block_bwd', 'attn_fwd')


def check_launch_count(dev, hook, abi, monkeypatch, batch_norm, layers=3, bsz=4):
    """an 8-head stack of L layers runs L launches of each of the four fused kernels per step and none of feta_attn_fwd /
    feta_layernorm_fwd / feta_layernorm_bwd (the pattern of test_modules_emu.check_layernorm_on_load_launches)"""
    import test_modules_emu as TM
    model = model8(batch_norm, layers=layers, seed=11).to(dev)
    batch9, cache = batch_of(dev, 'zinc', bsz, 9, 30, seed=5)
    with counted_calls(abi, LAUNCH_NAMES) as calls:
        TM._stack_run(model, batch9, cache, True, monkeypatch, hook)
    assert all(calls.get(k, 0) == layers for k in ('attn_block_fwd', 'ffn_fwd', 'ffn_bwd', 'attn_block_bwd')), calls
    assert all(k not in calls for k in ('attn_fwd', 'layernorm_fwd', 'layernorm_bwd')), calls


def check_bf16_untouched(dev, hook, abi, monkeypatch):
    """bf16 storage has no 8-head form: lowp_stack_supported is false, and a forward of an 8-head model with bf16 storage
    does what it did before the fp32 8-head kernels existed - the layers run one by one and the bf16 attention core
    refuses d_h = 8 (ValueError from feta_attn_fwd_bf16) - without an attn_block_fwd call."""
    import pytest
    from feta_tmlr_amd import fused_stack
    from feta_tmlr_amd.transformer import layers as LY
    model = model8(True).to(dev)
    batch9, cache = batch_of(dev, 'zinc', 3, 9, 30)
    x, mask, pe, _, degree, _, edge_index, batch, fi = batch9
    assert not fused_stack.lowp_stack_supported(abi, list(model.encoder.layers), x.shape[0], x.shape[1], 64)
    LY.set_storage_dtype(model, torch.bfloat16)
    with counted_calls(abi, ('attn_block_fwd',)) as calls, hook():
        with pytest.raises(ValueError, match='head dim 8'):
            model(x, edge_index, batch, fi, mask, pe, degree=degree, graph_cache=cache)
    assert 'attn_block_fwd' not in calls


def check_bench_step_heads8(dev, run_ctx, abi, argv):
    """bench_checks.check_bench_step (what bench.py times against oracle.encoder_gengcn: output kernel_checks.TOL, gradients
    3e-5 relative) on an 8-head argv, and the step must have gone through the one-launch block kernels"""
    import bench_checks as BC
    with counted_calls(abi, ('attn_block_fwd', 'attn_block_bwd')) as calls:
        errs, used_graph = BC.check_bench_step(dev, run_ctx, argv, replays=1 if dev.type == 'cpu' else 2)
    print('heads8 bench step', argv, {k: '%.2e' % v for k, v in errs.items()})
    assert calls.get('attn_block_fwd', 0) > 0 and calls.get('attn_block_bwd', 0) > 0, calls
    return errs, used_graph
