"""The coefficient generator's backward in two parts (csrc/feta_coeff.h: feta_coeff_dsum = the tanh pass over forward data,
feta_coeff_bwd_saved = the multiply-and-column-sum that depends on dpooled), as stand-alone kernels, as roles of the filter
stage's forward launch and of the last layer's ffn_bwd, and through the model.  Written once, run on the host emulation
and on the MI355X (see kernel_checks.py)."""
import torch

import kernel_checks as KC
from feta_tmlr_amd import _abi
from feta_tmlr_amd import functional as FF
from feta_tmlr_amd.transformer import data as D
from feta_tmlr_amd.transformer.models import DiffGraphTransformerGenGCN
from oracle import feta_oracle as O

NAN = float('nan')


def coeff_case(bsz, n, h, c, seed=0, zero_diag=True, nodes=None):
    """Inputs as kernel_checks.check_coeff builds them (nodes: the first graphs' node counts, to sit on tile and padding
    edges) and the fp64 references: A / Bm [H*B, C] by autograd of the oracle's collapsed generator block by block,
    ds = gw.grad[0] and db = gb.grad of <pooled, dp>."""
    g = torch.Generator().manual_seed(seed)
    nb = torch.randint(1, n + 1, (bsz,), generator=g, dtype=torch.int32)
    nb[0] = n
    if nodes is not None:
        nb[:len(nodes)] = torch.tensor(nodes, dtype=torch.int32)
    attn, mask = KC.random_attention(bsz, h, n, nb, g, zero_diag)
    attn = attn.nan_to_num(0.0)     # (a one-node graph whose self loop was zeroed: the row is 0 / 0 - the loop is refilled with 1)
    gw = (torch.randn(c, c, generator=g, dtype=torch.float64) / c ** 0.5).requires_grad_(True)
    gb = (0.1 * torch.randn(c, generator=g, dtype=torch.float64)).requires_grad_(True)
    eye, zero = torch.eye(c, dtype=torch.float64), torch.zeros(c, dtype=torch.float64)
    pooled = O.get_filter_coefficients_collapsed(attn, mask, gw, gb, eye, zero).reshape(h * bsz, c)
    dp = torch.randn(h * bsz, c, generator=g, dtype=torch.float64)
    # pooled[blk, c] depends on column c of gw (through s[c] = sum_r gw[r, c]) and on gb[c] only: the gradient of a block's
    # row sum w.r.t. any row of gw is A[blk, :], w.r.t. gb it is Bm[blk, :]
    A, Bm = torch.empty(h * bsz, c, dtype=torch.float64), torch.empty(h * bsz, c, dtype=torch.float64)
    for blk in range(h * bsz):
        ga, gbm = torch.autograd.grad(pooled[blk].sum(), (gw, gb), retain_graph=True)
        A[blk], Bm[blk] = ga[0], gbm
    ds, db = torch.autograd.grad((pooled * dp).sum(), (gw, gb))
    return dict(bsz=bsz, n=n, h=h, c=c, nb=nb, attn=attn, gw=gw.detach(), gb=gb.detach(), dp=dp, A=A, Bm=Bm, ds=ds[0], db=db,
                dw=ds)


def device_inputs(abi, dev, stream, case):
    """s, gcn bias, cj (the forward kernel's), dpooled on the device"""
    bsz, n, h, c = case['bsz'], case['n'], case['h'], case['c']
    s = torch.empty(c, device=dev)
    abi.colsum(case['gw'].float().to(dev), s, stream)
    gb32 = case['gb'].float().to(dev)
    nbd = case['nb'].to(dev)
    cj = torch.full((h * bsz, n), NAN, device=dev)
    pooled = torch.full((h * bsz, c), NAN, device=dev)
    abi.coeff_fwd(case['attn'].float().to(dev), nbd, s, gb32, cj, pooled, stream)
    return s, gb32, nbd, cj, case['dp'].float().to(dev)


def rel_err(got, ref):
    return KC.maxdiff(got, ref) / max(1.0, ref.abs().max().item())


def check_standalone(abi, dev, stream, case):
    """feta_coeff_dsum and feta_coeff_bwd_saved against fp64, and against today's feta_coeff_bwd on the same inputs.
    -> (A, Bm, partial [G, 2, C]) of the stand-alone kernels, for the role checks"""
    bsz, n, h, c = case['bsz'], case['n'], case['h'], case['c']
    s, gb32, nbd, cj, dpd = device_inputs(abi, dev, stream, case)
    A = torch.full((h * bsz, c), NAN, device=dev)
    Bm = torch.full((h * bsz, c), NAN, device=dev)
    abi.coeff_dsum(cj, nbd, s, gb32, A, Bm, bsz, n, h, stream)
    KC.assert_close('A', A, case['A'])
    KC.assert_close('Bm', Bm, case['Bm'])
    G = abi.coeff_bwd_saved_groups(bsz, h)
    assert 1 <= G <= h * bsz
    partial = torch.full((G, 2, c), NAN, device=dev)
    ds, db = torch.full((c,), NAN, device=dev), torch.full((c,), NAN, device=dev)
    abi.coeff_bwd_saved(dpd, A, Bm, partial, ds, db, bsz, h, stream)
    KC.assert_close('ds (saved form)', ds, case['ds'])
    KC.assert_close('dgcn_bias (saved form)', db, case['db'])
    # the dense gradient of gcn.weight from the reduction launch: every row equals ds, exactly
    ds2, db2 = torch.full((c,), NAN, device=dev), torch.full((c,), NAN, device=dev)
    dw = torch.full((c + 3, c), NAN, device=dev)
    abi.coeff_bwd_saved(dpd, A, Bm, partial, ds2, db2, bsz, h, stream, dw_dense=dw)
    assert torch.equal(ds2, ds) and torch.equal(db2, db)
    assert torch.equal(dw, ds.unsqueeze(0).expand_as(dw))
    # ds == NULL: the partials only
    p2 = torch.full((G, 2, c), NAN, device=dev)
    abi.coeff_bwd_saved(dpd, A, Bm, p2, None, None, bsz, h, stream)
    assert torch.equal(p2, partial)
    # today's kernel on the same inputs: the new path's error against fp64 is at most twice its error (or the guard floor)
    g0 = abi.coeff_bwd_groups(bsz, h)
    ds0, db0 = torch.full((c,), NAN, device=dev), torch.full((c,), NAN, device=dev)
    abi.coeff_bwd(cj, nbd, s, gb32, dpd, torch.zeros(g0, 2, c, device=dev), ds0, db0, bsz, n, h, stream)
    for nme, new, old, ref in (('ds', ds, ds0, case['ds']), ('db', db, db0, case['db'])):
        e_new, e_old = rel_err(new, ref), rel_err(old, ref)
        print('%s: saved form %.3e, tanh form %.3e (relative, fp64 reference)' % (nme, e_new, e_old))
        assert e_new <= max(2.0 * e_old, KC.GUARD_FLOOR), (nme, e_new, e_old)
    return dict(s=s, gb32=gb32, nbd=nbd, cj=cj, dpd=dpd, A=A, Bm=Bm, partial=partial)


def check_empty_block(abi, dev, stream, n=37, h=2, c=80):
    """a block with n_real = 0 writes zeros (and contributes nothing)"""
    g = torch.Generator().manual_seed(3)
    bsz = 3
    nbd = torch.tensor([5, 0, n], dtype=torch.int32).to(dev)
    cj = torch.randn(h * bsz, n, generator=g).to(dev)
    s, gb = torch.randn(c, generator=g).to(dev), torch.randn(c, generator=g).to(dev)
    A, Bm = torch.full((h * bsz, c), NAN, device=dev), torch.full((h * bsz, c), NAN, device=dev)
    abi.coeff_dsum(cj, nbd, s, gb, A, Bm, bsz, n, h, stream)
    for hh in range(h):
        assert float(A[hh * bsz + 1].abs().max()) == 0.0 and float(Bm[hh * bsz + 1].abs().max()) == 0.0
    assert bool(torch.isfinite(A).all()) and bool(torch.isfinite(Bm).all())


def _filter_launch_inputs(dev, bsz=5, seed=0):
    """a feta_spec_filter_cat_fwd call of its own small shape (kernel_checks.check_spec_cat, fresh BatchNorm statistics)"""
    h, dh, order, k_eig = 4, 16, 4, 16
    d = h * dh
    x, coeff, bias, _, mask, _, _, _, cache, n = KC._filter_case(bsz, h, dh, order, seed, 'zinc', None, None, k_eig)
    g = torch.Generator().manual_seed(seed + 7)
    f32 = lambda t: t.float().contiguous().to(dev)
    y2 = torch.randn(n, bsz, d, generator=g, dtype=torch.float64) * 1.5 + 0.3
    G = 5
    parts = torch.randn(G + 1, 2, d, generator=g, dtype=torch.float64)
    parts[:G, 1] = parts[:G, 1].abs() * n * bsz + parts[:G, 0] ** 2     # (a variance that stays positive)
    args = (KC.to_view(x, True, dev), f32(cache.u.double()), f32(cache.lam.double()), f32(coeff.reshape(h * bsz, -1)), f32(bias),
            cache.n_real.to(dev))
    kw = dict(y2=KC.to_view(y2.view(n, bsz, h, dh).permute(1, 0, 2, 3), True, dev),
              w_cat=f32(torch.randn(d, 2 * d, generator=g, dtype=torch.float64) / 8),
              b_cat=f32(torch.randn(d, generator=g, dtype=torch.float64) * 0.1), y2_stats=f32(parts), Gx=G,
              gamma=f32(torch.rand(d, generator=g, dtype=torch.float64) + 0.5),
              beta=f32(torch.randn(d, generator=g, dtype=torch.float64) * 0.2))
    return args, kw, (bsz, n, h, dh, order)


def check_roles(abi, dev, stream, case, alone, monkeypatch=None):
    """Hosted forms: bit-identical to the stand-alone kernels, and the host launches' own outputs bit-identical with and
    without the role (y, out, bn_out of the filter launch; every output of ffn_bwd)."""
    bsz, n, h, c = case['bsz'], case['n'], case['h'], case['c']
    args, kw, (fb, fn, fh, fdh, order) = _filter_launch_inputs(dev)
    outs = []
    for role in (False, True):
        yv, ov = KC.token_buffers(fb, fn, fh, fdh, True, dev), KC.token_buffers(fb, fn, fh, fdh, True, dev)
        bn_out = torch.full((4, fh * fdh), NAN, device=dev)
        A, Bm = torch.full((h * bsz, c), NAN, device=dev), torch.full((h * bsz, c), NAN, device=dev)
        dsum = (alone['cj'], alone['nbd'], alone['s'], alone['gb32'], A, Bm, bsz, n, h) if role else None
        abi.spec_filter_cat_fwd(*args, yv, order, 1, stream, out=ov, bn_out=bn_out, rmean=torch.zeros(fh * fdh, device=dev),
                                rvar=torch.ones(fh * fdh, device=dev), nbt=torch.zeros((), dtype=torch.int64, device=dev),
                                dsum=dsum, **kw)
        outs.append((yv, ov, bn_out))
    assert torch.equal(A, alone['A']) and torch.equal(Bm, alone['Bm']), 'tanh pass as a role of the filter launch'
    if monkeypatch is not None and h * bsz > 3:
        # three role workgroups walk all the blocks (the headline step walks two per workgroup; the launcher reads the
        # variable at every launch): the c_j row in LDS is reused block after block - still bit-identical
        monkeypatch.setenv('FETA_COEFF_DSUM_WGS', '3')
        yv, ov = KC.token_buffers(fb, fn, fh, fdh, True, dev), KC.token_buffers(fb, fn, fh, fdh, True, dev)
        A3, Bm3 = torch.full((h * bsz, c), NAN, device=dev), torch.full((h * bsz, c), NAN, device=dev)
        abi.spec_filter_cat_fwd(*args, yv, order, 1, stream, out=ov, bn_out=torch.full((4, fh * fdh), NAN, device=dev),
                                rmean=torch.zeros(fh * fdh, device=dev), rvar=torch.ones(fh * fdh, device=dev),
                                nbt=torch.zeros((), dtype=torch.int64, device=dev),
                                dsum=(alone['cj'], alone['nbd'], alone['s'], alone['gb32'], A3, Bm3, bsz, n, h), **kw)
        monkeypatch.delenv('FETA_COEFF_DSUM_WGS')
        assert torch.equal(A3, alone['A']) and torch.equal(Bm3, alone['Bm']), 'role workgroups walking several blocks'
        assert torch.equal(yv, outs[0][0]) and torch.equal(ov, outs[0][1])
    for a, b in zip(*outs):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    m, d, ff = 70, 64, 128
    g = torch.Generator().manual_seed(5)
    rnd = lambda *sh: torch.randn(*sh, generator=g).to(dev)
    x, w1, w2, hbuf, dy = rnd(m, d), rnd(ff, d) / 8, rnd(d, ff) / 11, rnd(m, ff).relu(), rnd(m, d)
    rc = abi.ffn_bwd_chunks(m, ff)
    cols = 2 * d * ff + d + ff
    G = abi.coeff_bwd_saved_groups(bsz, h)
    res = []
    for role in (False, True):
        dx, part = torch.full((m, d), NAN, device=dev), torch.full((rc, cols), NAN, device=dev)
        partial = torch.full((G, 2, c), NAN, device=dev)
        req = _abi.CoeffSavedReq(alone['dpd'], alone['A'], alone['Bm'], partial, bsz, h) if role else None
        abi.ffn_bwd(m, ff, stream, coeff=req, partial_ptr=part.data_ptr(), partial_ld=cols, dy=dy, h=hbuf, w2=w2, w1=w1, x=x,
                    dx=dx)
        res.append((dx, part))
    assert torch.equal(partial, alone['partial']), 'saved-form backward as a role of ffn_bwd'
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def check_rejects(abi, dev, stream):
    """null and mis-shaped arguments"""
    import pytest
    c, bsz, n, h = 64, 2, 8, 2
    z = lambda *s: torch.zeros(*s, device=dev)
    nbd = torch.full((bsz,), n, dtype=torch.int32, device=dev)
    cj, s, gb, A, Bm, dp = z(h * bsz, n), z(c), z(c), z(h * bsz, c), z(h * bsz, c), z(h * bsz, c)
    part = z(abi.coeff_bwd_saved_groups(bsz, h), 2, c)
    with pytest.raises(ValueError):
        abi.coeff_dsum(cj, nbd, s, gb, None, Bm, bsz, n, h, stream)
    with pytest.raises(ValueError):
        abi.coeff_dsum(cj, nbd, s, gb, A, Bm, 0, n, h, stream)
    with pytest.raises(ValueError):
        abi.coeff_bwd_saved(dp, None, Bm, part, None, None, bsz, h, stream)
    with pytest.raises(ValueError):
        abi.coeff_bwd_saved(dp, A, Bm, part, z(c), None, bsz, h, stream)      # ds without dbias
    with pytest.raises(ValueError):
        abi.coeff_bwd_saved(dp, A, Bm, part, None, None, bsz, 0, stream)
    assert abi.coeff_bwd_saved_groups(0, 4) == 0
    # the role descriptors: a null pointer, and graphs beyond the role's 64 nodes
    args, kw, (fb, fn, fh, fdh, order) = _filter_launch_inputs(dev)
    yv, ov = KC.token_buffers(fb, fn, fh, fdh, True, dev), KC.token_buffers(fb, fn, fh, fdh, True, dev)
    common = dict(out=ov, bn_out=z(4, 64), **kw)
    with pytest.raises(ValueError):
        abi.spec_filter_cat_fwd(*args, yv, order, 1, stream, dsum=(cj, nbd, s, gb, A, None, bsz, n, h), **common)
    with pytest.raises(ValueError):
        abi.spec_filter_cat_fwd(*args, yv, order, 1, stream, dsum=(z(h * bsz, 65), nbd, s, gb, A, Bm, bsz, 65, h), **common)
    m, d, ff = 32, 64, 128
    fkw = dict(dy=z(m, d), h=z(m, ff), w2=z(d, ff), w1=z(ff, d), x=z(m, d), dx=z(m, d))
    pbuf = z(abi.ffn_bwd_chunks(m, ff), 2 * d * ff + d + ff)
    with pytest.raises(ValueError):
        abi.ffn_bwd(m, ff, stream, coeff=_abi.CoeffSavedReq(dp, A, Bm, part, 0, h), partial_ptr=pbuf.data_ptr(), **fkw)


def check_fits(abi, dev, stream):
    """The role is taken only where a role workgroup walks at most two blocks: the filter launch is on the forward's chain.
    (MI355X, K <= 16: 512 resident slots.)  B = 128 leaves 384 slots for 512 blocks; B = 448 / 500 / 511 leave 64 / 12 / 1
    for ~2000 blocks - not taken, and a launch asked to carry them anyway is rejected."""
    import pytest
    assert abi.spec_cat_fwd_coeff_fits(128, 37, 16, 512)
    assert abi.spec_cat_fwd_coeff_fits(5, 37, 16, 20) and abi.spec_cat_fwd_coeff_fits(256, 64, 16, 512)
    for b in (448, 500, 511):
        assert not abi.spec_cat_fwd_coeff_fits(b, 37, 16, 4 * b), b
    assert not abi.spec_cat_fwd_coeff_fits(128, 65, 16, 512) and not abi.spec_cat_fwd_coeff_fits(0, 37, 16, 512)
    args, kw, (fb, fn, fh, fdh, order) = _filter_launch_inputs(dev)
    rb, rn, rh, c = 300, 8, 4, 64       # 1200 blocks beside 5 graphs: more than two per free slot
    assert not abi.spec_cat_fwd_coeff_fits(fb, fn, 16, rb * rh)
    z = lambda *s: torch.zeros(*s, device=dev)
    yv, ov = KC.token_buffers(fb, fn, fh, fdh, True, dev), KC.token_buffers(fb, fn, fh, fdh, True, dev)
    with pytest.raises(ValueError):
        abi.spec_filter_cat_fwd(*args, yv, order, 1, stream, out=ov, bn_out=z(4, 64),
                                dsum=(z(rb * rh, rn), torch.full((rb,), rn, dtype=torch.int32, device=dev), z(c), z(c),
                                      z(rb * rh, c), z(rb * rh, c), rb, rn, rh), **kw)


# ---- model level ------------------------------------------------------------------------------------------------------------

def headline_model(dev, bsz=5, heads=4, n_min=9, n_max=32, layers=3, seed=0):
    """the headline's layer shape (d = 64, 4 heads, 3 layers, BatchNorm, order 4, eigenbasis filter, every head on the graph)
    at a small batch.  Graphs of up to 32 nodes on all 32 eigenvectors: the fused filter launch takes K <= 32, and with
    the whole basis the filter is the oracle's (the headline's K = 16 of 37 truncates it)."""
    torch.manual_seed(seed)
    model = DiffGraphTransformerGenGCN(7, 1, 64, heads, dim_feedforward=128, dropout=0.0, nb_layers=layers, batch_norm=True,
                                       filter_order=4, heads_share_graph=True, filter_mode='spectral')
    with torch.no_grad():
        model.encoder.spectral_gnns.bias.normal_(0, 0.1)
        model.encoder.gcn.bias.normal_(0, 0.1)
    ds = D.SyntheticGraphDataset('zinc', bsz, in_dim=7, seed=seed, pos_enc=True, n_min=n_min, n_max=n_max)
    n_pad = max(g.num_nodes for g in ds.samples)
    n_pad = (n_pad + 3) // 4 * 4
    batch9, cache = D.collate(ds.samples, n_pad=n_pad, k_eig=n_pad if n_pad <= 32 else 16, device=dev)
    return model.to(dev), batch9, cache


def run_step(model, batch9, cache, hook, keep_grads=False, create_graph=False):
    x, mask, pe, _, degree, _, edge_index, batch, fi = batch9
    for p in model.parameters():
        if not keep_grads:
            p.grad = None
    buffers = {k: b.clone() for k, b in model.named_buffers()}
    with hook():
        out, _, coeff = model(x, edge_index, batch, fi, mask, pe, degree=degree, return_filter_coeff=True, graph_cache=cache)
        w = torch.linspace(0.5, 1.5, out.numel(), device=out.device).view_as(out)
        ((out * w).sum() + 0.01 * coeff.pow(2).sum()).backward(create_graph=create_graph)
    with torch.no_grad():       # (every run starts from the same running statistics: they shift the partial sums)
        for k, b in model.named_buffers():
            b.copy_(buffers[k])
    return out.detach().clone(), coeff.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters()
                                                          if p.grad is not None}


class Counter:
    """counts what the model launches through the C ABI (every launch goes through Abi._check), by entry point"""

    def __init__(self, abi):
        self.abi, self.calls = abi, []

    def __enter__(self):
        self.orig = self.abi._check
        self.abi._check = lambda rc, name: (self.calls.append(name), self.orig(rc, name))[1]
        return self

    def __exit__(self, *exc):
        del self.abi._check


def check_model(abi, dev, hook, monkeypatch):
    """switch on against switch off and against the fp64 oracle; launch counts"""
    model, batch9, cache = headline_model(dev)
    fwd = []        # (cj, pooled) of the generator's forward role, run by run
    orig_role = FF.PendingSums.coeff_fwd_role

    def role_spy(self, *a):
        r = orig_role(self, *a)
        if r is not None:
            fwd.append(self.coeff_fwd_out)
        return r
    monkeypatch.setattr(FF.PendingSums, 'coeff_fwd_role', role_spy)
    monkeypatch.setattr(FF, 'USE_COEFF_DSUM', True)
    with Counter(abi) as on_calls:
        on = run_step(model, batch9, cache, hook)
    monkeypatch.setattr(FF, 'USE_COEFF_DSUM', False)
    with Counter(abi) as off_calls:
        off = run_step(model, batch9, cache, hook)
    # the saved form ran, hosted at both ends; the step launches as many kernels as before
    assert 'feta_spec_filter_cat_fwd_coeff' in on_calls.calls and 'feta_ffn_bwd_coeff_saved' in on_calls.calls, on_calls.calls
    assert 'feta_spec_filter_cat_fwd' in off_calls.calls and 'feta_ffn_bwd_coeff' in off_calls.calls, off_calls.calls
    for nme in ('feta_coeff_dsum', 'feta_coeff_bwd_saved', 'feta_coeff_bwd', 'feta_coeff_fwd'):
        assert nme not in on_calls.calls, nme
    assert len(on_calls.calls) == len(off_calls.calls), (on_calls.calls, off_calls.calls)
    # the forward is untouched (cj and pooled of the generator, the model's output and coefficients), and so is every
    # gradient the generator's backward does not produce
    assert len(fwd) == 2 and torch.equal(fwd[0][0], fwd[1][0]) and torch.equal(fwd[0][1], fwd[1][1])
    assert bool(torch.isfinite(fwd[0][1]).all())
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    assert on[2].keys() == off[2].keys()
    for k in on[2]:
        if k in ('encoder.gcn.weight', 'encoder.gcn.bias'):
            KC.assert_close('on / off ' + k, on[2][k], off[2][k].double())
            w = on[2]['encoder.gcn.weight']
            assert torch.equal(w, w[0:1].expand_as(w))
        else:
            assert torch.equal(on[2][k], off[2][k]), k
    # a pass that accumulates into existing .grad tensors: nothing may be deferred - the saved form runs on a launch of its own
    monkeypatch.setattr(FF, 'USE_COEFF_DSUM', True)
    run_step(model, batch9, cache, hook)
    with Counter(abi) as acc_calls:
        twice = run_step(model, batch9, cache, hook, keep_grads=True)
    assert 'feta_coeff_bwd_saved' in acc_calls.calls and 'feta_ffn_bwd_coeff_saved' not in acc_calls.calls, acc_calls.calls
    for k in ('encoder.gcn.weight', 'encoder.gcn.bias', 'encoder.linear.bias'):
        KC.assert_close('accumulated ' + k, twice[2][k], 2.0 * on[2][k].double())
    # a backward under grad mode (create_graph=True) takes the earlier form although A / Bm exist
    with Counter(abi) as cg_calls:
        cg = run_step(model, batch9, cache, hook, create_graph=True)
    for p in model.parameters():
        p.grad = None           # (breaks the parameter <-> gradient cycle create_graph leaves)
    assert 'feta_spec_filter_cat_fwd_coeff' in cg_calls.calls and 'feta_coeff_bwd' in cg_calls.calls, cg_calls.calls
    assert 'feta_coeff_bwd_saved' not in cg_calls.calls and 'feta_ffn_bwd_coeff_saved' not in cg_calls.calls, cg_calls.calls
    for k in ('encoder.gcn.weight', 'encoder.gcn.bias'):
        KC.assert_close('create_graph ' + k, cg[2][k], on[2][k].double())
    # against the oracle, at the bars of the module tests (test_fused_batchnorm_stack_matches_oracle)
    x, mask, pe, _, degree, _, edge_index, batch, fi = [None if t is None else t.cpu() for t in batch9]
    p64 = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items()
           if v.dtype.is_floating_point and 'running_' not in k}
    out_ref, coeff_ref = O.graph_transformer_gengcn(x.double(), edge_index, batch, fi, mask, pe.double(), degree.double(), p64,
                                                    num_layers=3, num_heads=4, order=4, batch_norm=True,
                                                    heads_share_graph=True)
    w = torch.linspace(0.5, 1.5, out_ref.numel(), dtype=torch.float64).view_as(out_ref)
    ((out_ref * w).sum() + 0.01 * coeff_ref.pow(2).sum()).backward()
    KC.assert_close('model output', on[0], out_ref)
    KC.assert_close('coefficients', on[1], coeff_ref)
    for k, gk in on[2].items():
        KC.assert_close('grad ' + k, gk, p64[k].grad, tol=3e-5)


def check_fallbacks(abi, dev, hook, monkeypatch):
    """no A / Bm without a pending backward, and today's path for 8 heads and for graphs beyond 64 nodes"""
    monkeypatch.setattr(FF, 'USE_COEFF_DSUM', True)
    made = []
    orig = FF.PendingSums.coeff_dsum_role

    def spy(self, *a):
        r = orig(self, *a)
        made.append(r is not None)
        return r
    monkeypatch.setattr(FF.PendingSums, 'coeff_dsum_role', spy)
    model, batch9, cache = headline_model(dev)
    x, mask, pe, _, degree, _, edge_index, batch, fi = batch9
    with hook(), Counter(abi) as c:
        with torch.inference_mode():
            model(x, edge_index, batch, fi, mask, pe, degree=degree, graph_cache=cache)
        with torch.no_grad():
            model(x, edge_index, batch, fi, mask, pe, degree=degree, graph_cache=cache)
    assert not any(made), made
    assert 'feta_spec_filter_cat_fwd_coeff' not in c.calls and 'feta_coeff_dsum' not in c.calls, c.calls
    for kw in (dict(heads=8), dict(n_min=66, n_max=70)):
        made.clear()
        model, batch9, cache = headline_model(dev, layers=2, bsz=3, **kw)
        with Counter(abi) as c:
            run_step(model, batch9, cache, hook)
        assert not any(made), (kw, made)
        assert not any(n in c.calls for n in ('feta_spec_filter_cat_fwd_coeff', 'feta_ffn_bwd_coeff_saved', 'feta_coeff_dsum',
                                               'feta_coeff_bwd_saved')), (kw, c.calls)


def check_batch_that_nearly_fills_a_round(abi, dev, hook, monkeypatch, bsz=500):
    """B = 500 leaves 12 of the filter launch's 512 slots free for 2000 blocks: the request is not taken, no A / Bm, the
    backward recomputes the tanh in ffn_bwd as before"""
    monkeypatch.setattr(FF, 'USE_COEFF_DSUM', True)
    model, batch9, cache = headline_model(dev, bsz=bsz, n_min=4, n_max=12, layers=1)
    with Counter(abi) as c:
        run_step(model, batch9, cache, hook)
    assert 'feta_spec_filter_cat_fwd' in c.calls and 'feta_ffn_bwd_coeff' in c.calls, c.calls
    assert not any(n in c.calls for n in ('feta_spec_filter_cat_fwd_coeff', 'feta_ffn_bwd_coeff_saved', 'feta_coeff_dsum',
                                           'feta_coeff_bwd_saved')), c.calls
