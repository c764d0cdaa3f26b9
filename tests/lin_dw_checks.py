"""dW / db of the coefficient generator's C x C linear as a role of the first layer's attention backward
(feta_attn_block_bwd_sums_dw, csrc/feta_lin_dw.h) - at the kernel level, through the model and through every fallback of
the hand-over (functional.PendingSums.lin_dw_req).  Written once, run on the host emulation and on the MI355X."""
import pytest
import torch

import coeff_saved_checks as CS
import kernel_checks as KC
from feta_tmlr_amd import functional as FF
from feta_tmlr_amd import fused_stack as FS
from feta_tmlr_amd.transformer import data as D
from feta_tmlr_amd.transformer.models import DiffGraphTransformerGenGCN
from oracle import feta_oracle as O

NAN = float('nan')

# (R, C): one contraction chunk; two chunks (the buffer hand-over); an odd chunk count; several tile rows and columns
SHAPES = [(64, 256), (128, 256), (192, 256), (128, 512)]


class Req:
    """what Abi.attn_block_bwd takes as lin_dw (an _abi.LinDwReq without its checks: the rejections need bad ones)"""

    def __init__(self, dy, x, dw, db, rkn=None):
        self.dy, self.x, self.dw, self.db = dy, x, dw, db
        self.rkn = rkn if rkn is not None else (dy.shape[0], x.shape[1], dy.shape[1])

    def shape(self):
        return self.rkn


def block_case(abi, dev, stream, bsz=4, n_pad=37, n_min=5, seed=0):
    """Operands of one feta_attn_block_bwd launch (B graphs of n_min .. n_pad nodes, d = 64, 4 heads), saved by the launch's
    own forward kernel.  Computed once per (B, N) and shared: nothing below writes into it."""
    g, d, heads, n_real, mask, x0, pe, degree, p, _, _ = KC._ln_block_case(bsz, n_pad, n_min, seed, torch.float32)
    m = n_pad * bsz
    f32 = lambda t: t.detach().float().contiguous().to(dev)
    new = lambda *s: torch.full(s, NAN, device=dev)
    qkv, out, y = new(m, 3 * d), new(m, d), new(m, d)
    ast = torch.full((bsz, heads, n_pad, 2), NAN, device=dev)
    rows = f32(degree.t().reshape(m))
    scale = float(d // heads) ** -0.5
    w = {k: f32(v) for k, v in p.items()}
    x0d, ped, nrd = f32(x0).view(m, d), f32(pe), n_real.to(dev)
    abi.attn_block_fwd(bsz, n_pad, scale, stream, x=x0d, w_in=w['w_in'], b_in=w['b_in'], w_out=w['w_out'], b_out=w['b_out'],
                       pe=ped, n_real=nrd, rowscale=rows, qkv=qkv, out=out, attn_stats=ast, attn=None, y=y, y_stats=None)
    dy = f32(torch.randn(n_pad, bsz, d, generator=g)).view(m, d)
    dout2 = f32(torch.randn(n_pad, bsz, d, generator=g) * (~mask).t().unsqueeze(-1)).view(m, d)
    return dict(bsz=bsz, n=n_pad, m=m, d=d, scale=scale, dev=dev,
                ptrs=dict(dy=dy, rowscale=rows, w_out=w['w_out'], w_in=w['w_in'], qkv=qkv, out=out, dout2=dout2, pe=ped,
                          n_real=nrd, attn_stats=ast, x0=x0d))


def launch(abi, stream, blk, lin_dw=None, sums=(), **over):
    """one launch -> (dx, partial): everything the main workgroups write"""
    dev, d = blk['dev'], blk['d']
    dx = torch.full((blk['m'], d), NAN, device=dev)
    partial = torch.full((abi.attn_block_bwd_blocks(blk['bsz']), 4 * d * d + 4 * d), NAN, device=dev)
    ptrs = dict(blk['ptrs'], dx=dx, partial=partial)
    ptrs.update(over)
    dx, partial = ptrs['dx'], ptrs['partial']
    abi.attn_block_bwd(blk['bsz'], blk['n'], blk['scale'], stream, sums=sums, lin_dw=lin_dw, **ptrs)
    return dx, partial


def dw_case(r, c, dev, seed=0):
    """random operands of the product and its fp64 references; err_lib = the error of the library's fp32 products on the
    same operands (dW: dy^T x; db: dy^T 1), which bounds what the role is allowed"""
    g = torch.Generator().manual_seed(1000 + seed)
    dy, x = torch.randn(r, c, generator=g), torch.randn(r, c, generator=g)
    dw64, db64 = dy.double().t().mm(x.double()), dy.double().sum(0)
    dyd, xd = dy.to(dev), x.to(dev)
    lib_dw = dyd.t().mm(xd)
    lib_db = dyd.t().mm(torch.ones(r, 1, device=dev)).view(c)
    return dict(r=r, c=c, dy=dyd, x=xd, dw64=dw64, db64=db64, err_lib=(rel_err(lib_dw, dw64), rel_err(lib_db, db64)))


def rel_err(got, ref):
    return (got.detach().double().cpu() - ref).abs().max().item() / ref.abs().max().item()


def role_outputs(case):
    c, dev = case['c'], case['dy'].device
    return torch.full((c, c), NAN, device=dev), torch.full((c,), NAN, device=dev)


def assert_role_close(case, dw, db, what=''):
    """twice the library's own fp32 error against fp64: the factor covers the different summation order, nothing else"""
    e_dw, e_db = rel_err(dw, case['dw64']), rel_err(db, case['db64'])
    l_dw, l_db = case['err_lib']
    print('%s R=%d C=%d: dW role %.3e library %.3e; db role %.3e library %.3e (max abs error / max |ref|, fp64 reference)'
          % (what, case['r'], case['c'], e_dw, l_dw, e_db, l_db))
    assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
    assert e_dw <= 2.0 * l_dw, (e_dw, l_dw)
    assert e_db <= 2.0 * l_db, (e_db, l_db)


def check_kernel(abi, stream, blk, case, base, twice=False):
    """the role beside the main grid: dW / db against fp64, the main body's outputs bit-identical to the launch without it;
    twice: a second launch is bit-equal to the first, and db is optional"""
    dw, db = role_outputs(case)
    dx, partial = launch(abi, stream, blk, lin_dw=Req(case['dy'], case['x'], dw, db))
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(partial).all())
    assert torch.equal(dx, base[0]) and torch.equal(partial, base[1])
    assert_role_close(case, dw, db, 'role')
    if not twice:
        return dw, db
    dw2, db2 = role_outputs(case)
    dx2, partial2 = launch(abi, stream, blk, lin_dw=Req(case['dy'], case['x'], dw2, db2))
    assert torch.equal(dw2, dw) and torch.equal(db2, db) and torch.equal(dx2, dx) and torch.equal(partial2, partial)
    # db is optional
    dw3, _ = role_outputs(case)
    launch(abi, stream, blk, lin_dw=Req(case['dy'], case['x'], dw3, None))
    assert torch.equal(dw3, dw)
    return dw, db


def check_all_roles(abi, stream, blk, case, base):
    """main grid, dW tiles and column-sum segments (a tall and a wide one) in one launch"""
    dev = blk['dev']
    g = torch.Generator().manual_seed(7)
    segs_in = [torch.randn(40, 16, generator=g).to(dev), torch.randn(9, 4096 + 64, generator=g).to(dev)]
    outs = [torch.full((t.shape[1],), NAN, device=dev) for t in segs_in]
    dw, db = role_outputs(case)
    dx, partial = launch(abi, stream, blk, lin_dw=Req(case['dy'], case['x'], dw, db), sums=list(zip(segs_in, outs)))
    assert torch.equal(dx, base[0]) and torch.equal(partial, base[1])
    assert_role_close(case, dw, db, 'role + column sums')
    alone = [torch.full((t.shape[1],), NAN, device=dev) for t in segs_in]
    launch(abi, stream, blk, sums=list(zip(segs_in, alone)))
    for a, b, t in zip(outs, alone, segs_in):
        assert torch.equal(a, b)
        KC.assert_close('column sum', a, t.double().sum(0).cpu())
    return dw, db


def check_rounds(abi, dev, stream, case, one_round, monkeypatch):
    """more dW tiles than free workgroup slots: the role workgroups walk several tiles each.  Built from the occupancy the
    library reports: so many graphs that five slots stay free.  (Where one round holds more workgroups than the launch has
    graphs at one workgroup per graph - the emulation's two per CU - the role's grid is set directly instead.)"""
    n_pad, heads = 13, 4
    total = abi.attn_block_bwd_dw_slots(1, n_pad, heads) + 1
    tiles = (case['c'] // 128) * (case['c'] // 64)
    assert total > 5 and tiles > 5
    if abi.attn_block_bwd_blocks(total - 5) == total - 5:
        bsz = total - 5
        assert abi.attn_block_bwd_dw_slots(bsz, n_pad, heads) == 5
    else:
        bsz = 4
        monkeypatch.setenv('FETA_LIN_DW_WGS', '5')
    assert abi.attn_block_bwd_dw_supported(bsz, n_pad, heads, case['r'], case['c'], case['c'])
    blk = block_case(abi, dev, stream, bsz=bsz, n_pad=n_pad, n_min=3, seed=3)
    base = launch(abi, stream, blk)
    dw, db = role_outputs(case)
    dx, partial = launch(abi, stream, blk, lin_dw=Req(case['dy'], case['x'], dw, db))
    assert torch.equal(dx, base[0]) and torch.equal(partial, base[1])
    # the contraction order does not depend on the grid: bit-equal to the one-round launch
    assert torch.equal(dw, one_round[0]) and torch.equal(db, one_round[1])


def check_rejects(abi, dev, stream, blk):
    """each of these returns an error and launches nothing (the NaN-filled outputs stay NaN)"""
    case = dw_case(64, 256, dev)
    dy, x = case['dy'], case['x']
    flat = torch.zeros(64 * 256 + 4, device=dev)
    off = lambda t: flat[1:1 + t.numel()].view_as(t)      # 4 bytes past a 16-byte boundary
    z = lambda *s: torch.zeros(*s, device=dev)
    bad = [
        ('null dy', lambda dw, db: Req(None, x, dw, db, (64, 256, 256)), {}),
        ('null x', lambda dw, db: Req(dy, None, dw, db, (64, 256, 256)), {}),
        ('null dw', lambda dw, db: Req(dy, x, None, db), {}),
        ('misaligned dy', lambda dw, db: Req(off(dy), x, dw, db), {}),
        ('misaligned x', lambda dw, db: Req(dy, off(x), dw, db), {}),
        ('misaligned dw', lambda dw, db: Req(dy, x, torch.full((256 * 256 + 4,), NAN, device=dev)[1:1 + 256 * 256].view(256, 256), db), {}),
        ('R = 96', lambda dw, db: Req(z(96, 256), z(96, 256), dw, db), {}),
        ('K = 96', lambda dw, db: Req(z(64, 256), z(64, 96), torch.full((256, 96), NAN, device=dev), db), {}),
        ('N = 192', lambda dw, db: Req(z(64, 192), z(64, 256), torch.full((192, 256), NAN, device=dev), db[:192]), {}),
        ('SPLIT launch', lambda dw, db: Req(dy, x, dw, db), dict(dx_b=torch.full((blk['m'], blk['d']), NAN, device=dev))),
    ]
    for what, make, over in bad:
        dw, db = role_outputs(case)
        req = make(dw, db)
        # (what the main workgroups would write is allocated here, not inside launch(): it must still be NaN afterwards)
        dx = torch.full((blk['m'], blk['d']), NAN, device=dev)
        partial = torch.full((abi.attn_block_bwd_blocks(blk['bsz']), 4 * blk['d'] * blk['d'] + 4 * blk['d']), NAN, device=dev)
        with pytest.raises(ValueError):
            launch(abi, stream, blk, lin_dw=req, dx=dx, partial=partial, **over)
        for t in (req.dw, req.db, dx, partial) + tuple(over.values()):
            assert t is None or bool(torch.isnan(t).all()), what
    # bf16 storage
    dw, db = role_outputs(case)
    b16 = {k: (v.to(torch.bfloat16) if k in ('dy', 'qkv', 'out', 'dout2', 'pe', 'x0') else v) for k, v in blk['ptrs'].items()}
    dx = torch.full((blk['m'], blk['d']), NAN, device=dev).to(torch.bfloat16)
    partial = torch.full((blk['bsz'], 4 * 64 * 64 + 4 * 64), NAN, device=dev)
    with pytest.raises(ValueError):
        abi.attn_block_bwd(blk['bsz'], blk['n'], blk['scale'], stream, lin_dw=Req(dy, x, dw, db), dx=dx, partial=partial, **b16)
    for t in (dw, db, dx, partial):
        assert bool(torch.isnan(t).all())
    # the predicate: tiled shapes only, one workgroup per graph only
    assert abi.attn_block_bwd_dw_supported(4, 37, 4, 64, 256, 256) and abi.attn_block_bwd_dw_supported(4, 37, 8, 64, 256, 256)
    assert not abi.attn_block_bwd_dw_supported(4, 37, 4, 96, 256, 256)
    assert not abi.attn_block_bwd_dw_supported(4, 37, 4, 64, 96, 256)
    assert not abi.attn_block_bwd_dw_supported(4, 37, 4, 64, 256, 192)
    assert not abi.attn_block_bwd_dw_supported(4, 65, 4, 64, 256, 256) and not abi.attn_block_bwd_dw_supported(0, 37, 4, 64, 256, 256)
    assert not abi.attn_block_bwd_dw_supported(4, 37, 2, 64, 256, 256)
    assert abi.attn_block_bwd_dw_slots(100000, 37, 4) == 0


# ---- model level ------------------------------------------------------------------------------------------------------------

def small_model(dev, bsz, heads=4, order=1, layers=2, batch_norm=True, n_pad=37, seed=0):
    """d = 64, C = 256 for (4 heads, order 1) and for (8 heads, order 4); graphs of up to 37 nodes, padded to 37 as at the
    headline, on the whole eigenbasis (with all eigenvectors the filter is the oracle's; the headline's K = 16 truncates it)"""
    torch.manual_seed(seed)
    model = DiffGraphTransformerGenGCN(7, 1, 64, heads, dim_feedforward=128, dropout=0.0, nb_layers=layers,
                                       batch_norm=batch_norm, filter_order=order, heads_share_graph=True, filter_mode='spectral')
    with torch.no_grad():
        model.encoder.spectral_gnns.bias.normal_(0, 0.1)
        model.encoder.gcn.bias.normal_(0, 0.1)
    ds = D.SyntheticGraphDataset('zinc', bsz, in_dim=7, seed=seed, pos_enc=True, n_min=9, n_max=n_pad)
    batch9, cache = D.collate(ds.samples, n_pad=n_pad, k_eig=n_pad, device=dev)
    return model.to(dev), batch9, cache


LIN = ('encoder.linear.weight', 'encoder.linear.bias')


def library_linear(monkeypatch):
    """the C x C linear through the library GEMMs (at C = 256 the package would take its own csrc/lin.hip kernels)"""
    monkeypatch.setattr(FF, 'LIN_OWN_GEMM_MAX_MACS', 0)


def step_on_off(abi, model, batch9, cache, hook, monkeypatch, **kw):
    """-> (role on, role off, calls on, calls off, library GEMMs on, off)"""
    library_linear(monkeypatch)
    monkeypatch.setenv('FETA_LIN_DW_ROLE', '2')
    with CS.Counter(abi) as on_calls:
        on, mm_on = count_mm(lambda: CS.run_step(model, batch9, cache, hook, **kw))
    monkeypatch.setenv('FETA_LIN_DW_ROLE', '0')
    with CS.Counter(abi) as off_calls:
        off, mm_off = count_mm(lambda: CS.run_step(model, batch9, cache, hook, **kw))
    return on, off, on_calls.calls, off_calls.calls, mm_on, mm_off


def assert_same_but_lin(on, off):
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert on[2].keys() == off[2].keys() and all(k in on[2] for k in LIN)
    for k in on[2]:
        if k in LIN:
            KC.assert_close('on / off ' + k, on[2][k], off[2][k].double())
        else:
            assert torch.equal(on[2][k], off[2][k]), k


def count_mm(fn):
    """-> (fn(), library GEMM calls of the coefficient generator's linear: Tensor.mm / torch.mm / torch.addmm, which is how
    functional.py and _abi.LinDwReq reach the library - also from inside a backward pass)"""
    n = [0]
    saved = (torch.Tensor.mm, torch.mm, torch.addmm)

    def wrap(f):
        def g(*a, **k):
            n[0] += 1
            return f(*a, **k)
        return g
    torch.Tensor.mm, torch.mm, torch.addmm = wrap(saved[0]), wrap(saved[1]), wrap(saved[2])
    try:
        r = fn()
    finally:
        torch.Tensor.mm, torch.mm, torch.addmm = saved
    return r, n[0]


def check_model(abi, dev, hook, monkeypatch, bsz, heads=4, order=1, oracle=True, n_pad=37):
    model, batch9, cache = small_model(dev, bsz, heads=heads, order=order, n_pad=n_pad)
    assert tuple(model.encoder.linear.weight.shape) == (256, 256)
    on, off, on_calls, off_calls, mm_on, mm_off = step_on_off(abi, model, batch9, cache, hook, monkeypatch)
    assert 'feta_attn_block_bwd_sums_dw' in on_calls and 'feta_attn_block_bwd_sums_dw' not in off_calls, (on_calls, off_calls)
    assert 'feta_lin_bwd' not in on_calls + off_calls
    assert_same_but_lin(on, off)
    # one library GEMM fewer in the step (the forward's and the dX product stay), and the column sum of dcoeff with it
    assert mm_on == mm_off - 1 and mm_on == 2, (mm_on, mm_off)
    assert len(on_calls) <= len(off_calls)
    if oracle:
        oracle_grads(model, batch9, heads, order, on, off)


def oracle_grads(model, batch9, heads, order, on, off, layers=2):
    """both runs against the fp64 oracle, at the bars of the module tests"""
    x, mask, pe, _, degree, _, edge_index, batch, fi = [None if t is None else t.cpu() for t in batch9]
    p64 = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items()
           if v.dtype.is_floating_point and 'running_' not in k}
    out_ref, coeff_ref = O.graph_transformer_gengcn(x.double(), edge_index, batch, fi, mask, pe.double(), degree.double(), p64,
                                                    num_layers=layers, num_heads=heads, order=order, batch_norm=True,
                                                    heads_share_graph=True)
    w = torch.linspace(0.5, 1.5, out_ref.numel(), dtype=torch.float64).view_as(out_ref)
    ((out_ref * w).sum() + 0.01 * coeff_ref.pow(2).sum()).backward()
    for run in (on, off):
        KC.assert_close('model output', run[0], out_ref)
        for k, gk in run[2].items():
            KC.assert_close('grad ' + k, gk, p64[k].grad, tol=3e-5)


def lin_grads_ref(model, batch9, cache, hook, monkeypatch):
    """linear.weight.grad / linear.bias.grad of a plain step with the role off"""
    library_linear(monkeypatch)
    monkeypatch.setenv('FETA_LIN_DW_ROLE', '0')
    ref = CS.run_step(model, batch9, cache, hook)
    return {k: ref[2][k].double() for k in LIN}


class HandOverSpy:
    """what happens to the request, in order: 'defer' (FilterFromPooledFn.backward left it), 'run' (somebody ran it with the
    library: LinDwReq.run), bracketed by 'finish(' .. ')' while PendingSums._finish_pass is on the stack"""

    def __init__(self, monkeypatch):
        from feta_tmlr_amd import _abi
        self.events = ev = []
        defer, run, finish = FF.PendingSums.defer_lin_dw, _abi.LinDwReq.run, FF.PendingSums._finish_pass

        def spy_defer(pend, req, owners):
            ev.append('defer')
            return defer(pend, req, owners)

        def spy_run(req, abi, stream):
            ev.append('run')
            return run(req, abi, stream)

        def spy_finish(pend):
            ev.append('finish(')
            try:
                return finish(pend)
            finally:
                ev.append(')')
        monkeypatch.setattr(FF.PendingSums, 'defer_lin_dw', spy_defer)
        monkeypatch.setattr(_abi.LinDwReq, 'run', spy_run)
        monkeypatch.setattr(FF.PendingSums, '_finish_pass', spy_finish)

    def take(self):
        ev = list(self.events)
        del self.events[:]
        return ev


def check_fallbacks(abi, dev, hook, monkeypatch):
    """every way the request is NOT carried gives the same linear.weight.grad / linear.bias.grad (the smallest model that
    would take the role: 8 heads x 8 graphs = 64 rows, graphs of up to 13 nodes), and the request takes the way it should"""
    model, batch9, cache = small_model(dev, 8, heads=8, order=4, n_pad=13, layers=1)
    ref = lin_grads_ref(model, batch9, cache, hook, monkeypatch)
    spy = HandOverSpy(monkeypatch)
    monkeypatch.setenv('FETA_LIN_DW_ROLE', '2')
    lin = model.encoder.linear

    def close(got, what, factor=1.0):
        for k in LIN:
            KC.assert_close(what + ' ' + k, got[k], factor * ref[k])

    def clear_grads():
        for p in model.parameters():
            p.grad = None

    # torch.autograd.grad on the linear's parameters only: the request is left, the stack's node is pruned from the pass, and
    # the end of the pass (_finish_pass) runs the product with the library - before autograd.grad returns the tensors
    clear_grads()
    x, mask, pe, _, degree, _, edge_index, batch, fi = batch9
    with hook(), CS.Counter(abi) as c:
        out, _, coeff = model(x, edge_index, batch, fi, mask, pe, degree=degree, return_filter_coeff=True, graph_cache=cache)
        wgt = torch.linspace(0.5, 1.5, out.numel(), device=out.device).view_as(out)
        n_fwd = len(c.calls)
        (gw, gb), mms = count_mm(lambda: torch.autograd.grad((out * wgt).sum() + 0.01 * coeff.pow(2).sum(), (lin.weight, lin.bias)))
    ev = spy.take()
    assert ev == ['defer', 'finish(', 'run', ')'], ev
    bwd = c.calls[n_fwd:]
    assert 'feta_attn_block_bwd_sums_dw' not in bwd and not any('ffn_bwd' in k or 'attn_block_bwd' in k for k in bwd), bwd
    assert mms == 2, mms      # the dX product in the node, the dW product at the end of the pass
    assert lin.weight.grad is None and lin.bias.grad is None
    close({LIN[0]: gw, LIN[1]: gb}, 'autograd.grad on the linear alone')
    # the plain step of this model does carry it: left, taken by the stack's launch, never run with the library
    with CS.Counter(abi) as c:
        got = CS.run_step(model, batch9, cache, hook)
    ev = spy.take()
    assert 'feta_attn_block_bwd_sums_dw' in c.calls and 'defer' in ev and 'run' not in ev, (c.calls, ev)
    close(got[2], 'carried')
    # FETA_ATTN_BLOCK_BWD off: the stack's backward has no carrying launch - it runs the library product at its start
    monkeypatch.setattr(FS, 'USE_ATTN_BLOCK_BWD', False)
    with CS.Counter(abi) as c:
        got = CS.run_step(model, batch9, cache, hook)
    monkeypatch.setattr(FS, 'USE_ATTN_BLOCK_BWD', True)
    ev = spy.take()
    assert 'feta_attn_block_bwd_sums_dw' not in c.calls
    assert 'defer' in ev and 'run' in ev and ev.index('run') < ev.index('finish('), ev      # (by the stack, not the safety net)
    close(got[2], 'attention backward in three launches')
    # a hook on linear.weight: nothing is deferred
    seen = []
    h = lin.weight.register_hook(lambda g_: seen.append(g_.detach().clone()))
    with CS.Counter(abi) as c:
        got = CS.run_step(model, batch9, cache, hook)
    h.remove()
    assert 'feta_attn_block_bwd_sums_dw' not in c.calls and len(seen) == 1 and 'defer' not in spy.take()
    close(got[2], 'hook on linear.weight')
    KC.assert_close('what the hook saw', seen[0], ref[LIN[0]])
    # linear.weight.grad already present (the step above left it): the gradient accumulates, nothing is deferred
    assert lin.weight.grad is not None
    with CS.Counter(abi) as c:
        twice = CS.run_step(model, batch9, cache, hook, keep_grads=True)
    assert 'feta_attn_block_bwd_sums_dw' not in c.calls and 'defer' not in spy.take()
    close(twice[2], 'accumulated', 2.0)
    # a LayerNorm stack: left by the filter stage, run with the library at the start of the stack's backward
    model_ln, b9, cache_ln = small_model(dev, 8, heads=8, order=4, n_pad=13, layers=1, batch_norm=False)
    ref_ln = lin_grads_ref(model_ln, b9, cache_ln, hook, monkeypatch)
    spy.take()
    monkeypatch.setenv('FETA_LIN_DW_ROLE', '2')
    with CS.Counter(abi) as c:
        got = CS.run_step(model_ln, b9, cache_ln, hook)
    ev = spy.take()
    assert 'feta_attn_block_bwd_sums_dw' not in c.calls
    # (a LayerNorm model arms the stack only where its forward is the fused stack: either nothing was left, or the stack ran it)
    assert ('defer' not in ev and 'run' not in ev) or ev.index('run') < ev.index('finish('), ev
    for k in LIN:
        KC.assert_close('LayerNorm stack ' + k, got[2][k], ref_ln[k])


def check_two_phase(abi, dev, hook, monkeypatch):
    """keep_stack_boundary (backward_head / backward_stack): the head gradients are final when phase 1 returns"""
    model, batch9, cache = small_model(dev, 8, heads=8, order=4, n_pad=13)
    library_linear(monkeypatch)
    enc = model.encoder
    x, mask, pe, _, degree, _, edge_index, batch, fi = batch9
    src = model.embedding(x.permute(1, 0, 2)).detach()
    dout = torch.randn(src.shape, generator=torch.Generator().manual_seed(3)).to(dev)
    buffers = {k: b.clone() for k, b in enc.named_buffers()}
    names = ('linear.weight', 'linear.bias')

    def restore():
        for p in enc.parameters():
            p.grad = None
        with torch.no_grad():
            for k, b in enc.named_buffers():
                b.copy_(buffers[k])

    def fwd():
        return enc(src, pe, edge_index, fi, batch, degree=degree, src_key_padding_mask=mask, graph_cache=cache)[0]
    prm = dict(enc.named_parameters())
    with hook():
        monkeypatch.setenv('FETA_LIN_DW_ROLE', '0')
        fwd().backward(gradient=dout)
        ref = {k: prm[k].grad.detach().clone().double() for k in names}
        restore()
        monkeypatch.setenv('FETA_LIN_DW_ROLE', '2')
        enc.keep_stack_boundary = True
        try:
            with CS.Counter(abi) as c:
                enc.backward_head(fwd(), dout)
                head = {k: prm[k].grad.detach().clone() for k in names}
                enc.backward_stack()
        finally:
            enc.keep_stack_boundary = False
    assert 'feta_attn_block_bwd_sums_dw' not in c.calls
    for k in names:
        KC.assert_close('after phase 1 ' + k, head[k], ref[k])
        KC.assert_close('after phase 2 ' + k, prm[k].grad, ref[k])
    restore()
