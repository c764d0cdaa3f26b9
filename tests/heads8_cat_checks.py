"""Checks of the 8-head (d_h = 8) form of the folded filter launches: feta_spec_filter_cat_fwd / feta_spec_filter_cat_bwd
(csrc/filter.hip, the TWO instantiations of spec_cat_fwd_graph_kernel / spec_cat_bwd_graph_kernel) - kernel_checks.check_spec_cat
and check_spec_cat_bwd with h, dh = 8, 8, head isolation, predicates and rejections, and the model through the fold.  The
reference is the fp64 oracle (oracle.spec_filter_eig per block, oracle.graph_transformer_gengcn) plus autograd, every bar
kernel_checks.assert_close at its default TOL (gradients of the model: 3e-5, the project's bar); written once, run on the
host emulation (test_heads8_cat_emu.py) and on the MI355X (test_heads8_cat_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

import kernel_checks as KC
from coeff_saved_checks import Counter, run_step
from feta_tmlr_amd import functional as FF
from feta_tmlr_amd.transformer import data as D
from feta_tmlr_amd.transformer.models import DiffGraphTransformerGenGCN
from oracle import feta_oracle as O

H, DH, ORDER = 8, 8, 4
DM = H * DH
NAN = float('nan')

# where the new code can go wrong: three ragged row tiles (N_pad ~ 37); one eigen tile half used; the MUTAG sizes; four row
# tiles and two eigen tiles; a graph of one node beside a full one of 17 (the second row tile holds one real row) at the
# smallest K; a ragged second eigen tile
ZINC = dict(bsz=5, shape='zinc', k_eig=16)
EDGE = dict(nodes=(1, 17, 9), k_eig=4)
FWD_CASES = [
    dict(ZINC, norm='bn_fresh'),
    dict(bsz=3, k_eig=8, norm='bn_block'),
    dict(shape='mutag', k_eig=8, norm='plain'),
    dict(shape='pattern', n_min=44, n_max=64, k_eig=32, bsz=2, norm='bn_fresh'),
    dict(EDGE, norm='bn_fresh'),
    dict(bsz=3, k_eig=20, norm='plain'),
    dict(bsz=3, k_eig=16, norm='bn_block', with_bias=False),
]
BWD_CASES = [dict(kw, norm=norm) for kw in FWD_CASES[:5] for norm in ('bn_block', 'plain')]


def _samples_of(nodes, seed):
    """graphs of exactly these node counts (a ZINC-like molecule each)"""
    out = []
    for i, nn_ in enumerate(nodes):
        out += D.SyntheticGraphDataset('zinc', 1, in_dim=DM, seed=seed + i, n_min=nn_, n_max=nn_).samples
    return out


def filter_case(bsz=5, shape='zinc', n_min=None, n_max=None, k_eig=16, seed=0, nodes=None):
    """kernel_checks._filter_case at h, dh = 8, 8 (nodes: a batch of exactly these node counts instead of random ones)"""
    if nodes is None:
        return KC._filter_case(bsz, H, DH, ORDER, seed, shape, n_min, n_max, k_eig)
    orig = KC.make_batch
    KC.make_batch = lambda *a, **kw: D.collate(_samples_of(nodes, seed), k_eig=k_eig)
    try:
        return KC._filter_case(len(nodes), H, DH, ORDER, seed, shape, None, None, k_eig)
    finally:
        KC.make_batch = orig


def _f32(dev):
    return lambda t: t.detach().float().contiguous().to(dev)


def _cat_operands(n, bsz, seed):
    g = torch.Generator().manual_seed(seed)
    y2 = torch.randn(n, bsz, DM, generator=g, dtype=torch.float64) * 1.5 + 0.3
    w_cat = (torch.randn(DM, 2 * DM, generator=g, dtype=torch.float64) / 8).float().double()
    b_cat = (torch.randn(DM, generator=g, dtype=torch.float64) * 0.1).float().double()
    return g, y2, w_cat, b_cat


def _bn(y2, g):
    gamma = (torch.rand(DM, generator=g, dtype=torch.float64) + 0.5).float().double()
    beta = (torch.randn(DM, generator=g, dtype=torch.float64) * 0.2).float().double()
    rows = y2.reshape(-1, DM)
    mean, var = rows.mean(0), rows.var(0, unbiased=False)
    rstd = (var + 1e-5).rsqrt()
    return gamma, beta, mean, var, rstd


def oracle_filt(x, coeff, bias, cache, n, grad=False):
    """[n, bsz, 64]: oracle.spec_filter_eig per (head, graph) block, zero rows beyond n_real"""
    u, lam = cache.u.double(), cache.lam.double()
    nb = cache.n_real.tolist()
    cols = []
    for hh in range(H):
        col = []
        for bb in range(x.shape[0]):
            k = nb[bb]
            yb = O.spec_filter_eig(x[bb, :k, hh], u[bb, :k], lam[bb], coeff[hh, bb].reshape(ORDER, DH, DH), bias)
            col.append(torch.cat([yb, torch.zeros(n - k, DH, dtype=torch.float64)], 0))
        cols.append(torch.stack(col, 1))
    return torch.cat(cols, -1)


def run_fwd(abi, dev, stream, x, coeff, bias, cache, n, y2, w_cat, b_cat, **kw):
    """feta_spec_filter_cat_fwd at 8 heads -> (filt, out) as [n, bsz, 64]"""
    bsz = x.shape[0]
    f32 = _f32(dev)
    yv = KC.token_buffers(bsz, n, H, DH, True, dev)
    ov = KC.token_buffers(bsz, n, H, DH, True, dev)
    y2v = KC.to_view(y2.view(n, bsz, H, DH).permute(1, 0, 2, 3), True, dev)
    abi.spec_filter_cat_fwd(KC.to_view(x, True, dev), f32(cache.u.double()), f32(cache.lam.double()),
                            f32(coeff.reshape(H * bsz, -1)), None if bias is None else f32(bias), cache.n_real.to(dev), yv, ORDER,
                            1, stream, y2=y2v, w_cat=f32(w_cat), b_cat=f32(b_cat), out=ov, **kw)
    return yv.permute(1, 0, 2, 3).reshape(n, bsz, DM), ov.permute(1, 0, 2, 3).reshape(n, bsz, DM)


def check_fwd(abi, dev, stream, norm='bn_fresh', with_bias=True, seed=0, **case):
    """kernel_checks.check_spec_cat at 8 heads of 8: filt, out and - norm 'bn_fresh' - the published block, the running
    statistics and num_batches_tracked"""
    x, coeff, bias, _, _, _, _, _, cache, n = filter_case(seed=seed, **case)
    if not with_bias:
        bias = None
    bsz = x.shape[0]
    m = n * bsz
    g, y2, w_cat, b_cat = _cat_operands(n, bsz, seed + 7)
    filt = oracle_filt(x, coeff, bias, cache, n)
    f32 = _f32(dev)
    kw = {}
    if norm == 'plain':
        xn = y2
    else:
        gamma, beta, mean, var, rstd = _bn(y2, g)
        xn = (y2 - mean) * rstd * gamma + beta
        block = torch.stack([gamma * rstd, beta - mean * gamma * rstd, mean, rstd])
        if norm == 'bn_block':
            kw = dict(y2_bn=f32(block))
        else:
            G = 5
            shift = (mean + 0.05 * torch.randn(DM, generator=g, dtype=torch.float64)).float().double()
            parts = torch.zeros(G + 1, 2, DM, dtype=torch.float64)
            for i, chunk in enumerate(torch.chunk(y2.reshape(m, DM) - shift, G, dim=0)):
                parts[i, 0], parts[i, 1] = chunk.sum(0), (chunk * chunk).sum(0)
            parts[G, 0] = shift
            kw = dict(y2_stats=f32(parts), Gx=G, gamma=f32(gamma), beta=f32(beta), bn_out=torch.full((4, DM), NAN, device=dev),
                      rmean=torch.zeros(DM, device=dev), rvar=torch.ones(DM, device=dev),
                      nbt=torch.zeros((), dtype=torch.int64, device=dev))
    out_ref = F.linear(torch.cat((xn, filt), dim=-1), w_cat, b_cat)
    got_filt, got_out = run_fwd(abi, dev, stream, x, coeff, bias, cache, n, y2, w_cat, b_cat, **kw)
    errs = {'filt': KC.assert_close('h8 spec_cat filt', got_filt, filt),
            'out': KC.assert_close('h8 spec_cat out', got_out, out_ref)}
    if norm == 'bn_fresh':
        errs['bn_out'] = KC.assert_close('h8 spec_cat bn block', kw['bn_out'], block)
        KC.assert_close('h8 spec_cat running mean', kw['rmean'], 0.1 * mean)
        KC.assert_close('h8 spec_cat running var', kw['rvar'], 0.9 + 0.1 * var * m / (m - 1))
        assert int(kw['nbt']) == 1
    print('heads8 cat fwd', dict(case, norm=norm, n=n), {k: '%.2e' % v for k, v in errs.items()})
    return errs


def run_bwd(abi, dev, stream, x, coeff, cache, n, filt, y2, dout, w_cat, prm, ld=None):
    """feta_spec_filter_cat_bwd at 8 heads on NaN-filled outputs -> dict of what it wrote"""
    bsz = x.shape[0]
    f32 = _f32(dev)
    tv = lambda t: KC.to_view(t.detach().view(n, bsz, H, DH).permute(1, 0, 2, 3), True, dev)
    dxv = KC.token_buffers(bsz, n, H, DH, True, dev)
    dxnv = KC.token_buffers(bsz, n, H, DH, True, dev)
    dcoeff = torch.full((H * bsz, ORDER * DH * DH), NAN, device=dev)
    dbp = torch.full((bsz * H, DH), NAN, device=dev)
    rows = abi.spec_cat_bwd_rows(bsz)
    partial = torch.full((rows, ld or DM * 2 * DM + DM), NAN, device=dev)
    gs = torch.full((rows, 2, DM), NAN, device=dev) if prm is not None else None
    abi.spec_filter_cat_bwd(KC.to_view(x, True, dev), f32(cache.u.double()), f32(cache.lam.double()), f32(coeff.reshape(H * bsz, -1)),
                            cache.n_real.to(dev), tv(filt), dxv, dcoeff, dbp, ORDER, 1, stream, dout=tv(dout), y2=tv(y2),
                            w_cat=f32(w_cat), dxn=dxnv, partial=partial, y2_bn=None if prm is None else f32(prm), gs=gs)
    return dict(dx=dxv, dcoeff=dcoeff, dbp=dbp, dxn=dxnv.permute(1, 0, 2, 3).reshape(n, bsz, DM), partial=partial, gs=gs, rows=rows)


def check_bwd(abi, dev, stream, norm='bn_block', seed=0, **case):
    """kernel_checks.check_spec_cat_bwd at 8 heads of 8: dx, dcoeff, dbias (the sum of the [item][d_h] partials), dxn, dW_cat
    and db_cat from the partial rows, gs, and nothing written beyond the partial row"""
    x, coeff, bias, _, _, _, _, _, cache, n = filter_case(seed=seed, **case)
    bsz = x.shape[0]
    g, y2, w_cat, b_cat = _cat_operands(n, bsz, seed + 11)
    dout = torch.randn(n, bsz, DM, generator=g, dtype=torch.float64)
    w_cat.requires_grad_(True)
    b_cat.requires_grad_(True)
    xr, cr, br = (t.clone().requires_grad_(True) for t in (x, coeff, bias))
    filt = oracle_filt(xr, cr, br, cache, n)
    prm = None
    if norm == 'plain':
        xn = y2.clone().requires_grad_(True)
        xhat = torch.zeros_like(y2)
    else:
        gamma, beta, mean, _, rstd = _bn(y2, g)
        prm = torch.stack([gamma * rstd, beta - mean * gamma * rstd, mean, rstd]).float().double()     # what the kernel reads
        xhat = (y2 - prm[2]) * prm[3]
        xn = (y2 * prm[0] + prm[1]).detach().requires_grad_(True)
    (F.linear(torch.cat((xn, filt), dim=-1), w_cat, b_cat) * dout).sum().backward()
    gs_ref = torch.stack([xn.grad.sum(0), (xn.grad * xhat).sum(0)], 1)     # [bsz, 2, d]
    wsz = DM * 2 * DM
    t = run_bwd(abi, dev, stream, x, coeff, cache, n, filt, y2, dout, w_cat, prm, ld=wsz + DM + 8)
    errs = {'dx': KC.assert_close('h8 spec_cat_bwd dx', t['dx'], xr.grad),
            'dcoeff': KC.assert_close('h8 spec_cat_bwd dcoeff', t['dcoeff'], cr.grad.reshape(H * bsz, -1)),
            'dbias': KC.assert_close('h8 spec_cat_bwd dbias', t['dbp'].sum(0), br.grad),
            'dxn': KC.assert_close('h8 spec_cat_bwd dxn', t['dxn'], xn.grad),
            'dW_cat': KC.assert_close('h8 spec_cat_bwd dW_cat', t['partial'][:, :wsz].sum(0).view(DM, 2 * DM), w_cat.grad),
            'db_cat': KC.assert_close('h8 spec_cat_bwd db_cat', t['partial'][:, wsz:wsz + DM].sum(0), b_cat.grad)}
    assert bool(torch.isnan(t['partial'][:, wsz + DM:]).all()), 'h8 spec_cat_bwd wrote beyond its partial row'
    if t['gs'] is not None:
        if t['rows'] == bsz:
            errs['gs'] = KC.assert_close('h8 spec_cat_bwd gs', t['gs'], gs_ref)
        else:     # a walked batch: workgroup i holds the sum over graphs i, i + rows, ...
            errs['gs'] = KC.assert_close('h8 spec_cat_bwd gs', t['gs'].sum(0), gs_ref.sum(0))
    print('heads8 cat bwd', dict(case, norm=norm, n=n), {k: '%.2e' % v for k, v in errs.items()})
    return errs


def check_head_isolation(abi, dev, stream, seed=0):
    """A wave's 16-column tile holds heads 2t and 2t + 1, and the off-diagonal 8 x 8 blocks of its W_k tile are zeros:
    replacing the coefficients and the inputs of the odd heads by other random values must not change one bit of the even
    heads' filt columns, dx columns and dcoeff blocks - and the other way round.

    Second half: NaN coefficients in head 2t + 1 leave filt of head 2t finite and equal to the oracle.  The forward's zeros
    are staged 0.0f in the W_k tile, and a NaN coefficient sits in that tile too, in the diagonal block of its own head: in
    Ytil[e][c'] = sum_c (..)[e][c] W_k[c][c'] it only meets columns c' of its own head, never a staged zero, so the half
    holds for this implementation although the zeros are not select-based.  (NaN INPUTS of the other head would meet the
    staged zeros and are not asserted.)"""
    x, coeff, bias, _, _, _, _, _, cache, n = filter_case(**ZINC, seed=seed)
    bsz = x.shape[0]
    g, y2, w_cat, b_cat = _cat_operands(n, bsz, seed + 7)
    dout = torch.randn(n, bsz, DM, generator=g, dtype=torch.float64)
    real = (torch.arange(n)[None, :] < cache.n_real[:, None]).double()[:, :, None, None]       # [B, N, 1, 1]
    heads = lambda t, par: t.reshape(*t.shape[:-1], H, DH)[..., par::2, :]      # [.., 64] -> the columns of every second head

    def run(xx, cc):
        filt, _ = run_fwd(abi, dev, stream, xx, cc, bias, cache, n, y2, w_cat, b_cat)
        t = run_bwd(abi, dev, stream, xx, cc, cache, n, filt.double().cpu(), y2, dout, w_cat, None)
        return filt, t['dx'], t['dcoeff'].view(H, bsz, -1)
    base = run(x, coeff)
    for par in (0, 1):                  # the heads that keep their values
        x2, c2 = x.clone(), coeff.clone()
        x2[:, :, 1 - par::2] = torch.randn(bsz, n, H // 2, DH, generator=g, dtype=torch.float64) * real
        c2[1 - par::2] = torch.randn(H // 2, bsz, ORDER * DH * DH, generator=g, dtype=torch.float64) / DH ** 0.5
        got = run(x2, c2)
        assert torch.equal(heads(got[0], par), heads(base[0], par)), 'filt of the untouched heads moved'
        assert torch.equal(got[1][:, :, par::2], base[1][:, :, par::2]), 'dx of the untouched heads moved'
        assert torch.equal(got[2][par::2], base[2][par::2]), 'dcoeff of the untouched heads moved'
        assert not torch.equal(heads(got[0], 1 - par), heads(base[0], 1 - par))      # (the replaced heads did change)
    c3 = coeff.clone()
    c3[1::2] = NAN
    filt, _ = run_fwd(abi, dev, stream, x, c3, bias, cache, n, y2, w_cat, b_cat)
    ref = oracle_filt(x, coeff, bias, cache, n)
    assert bool(torch.isfinite(heads(filt, 0)).all())
    KC.assert_close('h8 spec_cat filt beside NaN heads', heads(filt, 0), heads(ref, 0))
    assert bool(torch.isnan(heads(filt, 1))[:1].all())       # (row 0 is a real node of every graph)


def check_predicates(abi):
    assert abi.spec_cat_supported(37, 8, 8, 4, 16, True) and abi.spec_cat_bwd_supported(64, 8, 8, 4, 32, True)
    assert abi.spec_cat_supported(64, 8, 8, 4, 4, True) and abi.spec_cat_bwd_supported(1, 8, 8, 4, 20, True)
    for n, h, dh, p, k, share in ((65, 8, 8, 4, 16, True), (37, 8, 8, 4, 16, False), (37, 8, 8, 3, 16, True),
                                  (37, 8, 16, 4, 16, True), (37, 2, 32, 4, 16, True), (37, 8, 8, 4, 36, True),
                                  (37, 8, 8, 4, 18, True)):
        assert not abi.spec_cat_supported(n, h, dh, p, k, share), (n, h, dh, p, k, share)
        assert not abi.spec_cat_bwd_supported(n, h, dh, p, k, share), (n, h, dh, p, k, share)
    # 4 heads: unchanged (forward up to 128 nodes, backward up to 64)
    assert abi.spec_cat_supported(100, 4, 16, 4, 16, True) and not abi.spec_cat_bwd_supported(100, 4, 16, 4, 16, True)
    assert abi.spec_cat_supported(128, 4, 16, 4, 32, True) and not abi.spec_cat_supported(129, 4, 16, 4, 32, True)
    assert abi.spec_cat_bwd_supported(64, 4, 16, 4, 32, True) and not abi.spec_cat_supported(37, 4, 16, 4, 16, False)


def check_rejections(abi, dev, stream):
    """the role launch (dsum=) has no 8-head form, and 8-head graphs end at 64 nodes: both raise, with a message"""
    x, coeff, bias, _, _, _, _, _, cache, n = filter_case(bsz=2, k_eig=8)
    g, y2, w_cat, b_cat = _cat_operands(n, 2, 1)
    z = lambda *s: torch.zeros(*s, device=dev)
    c, rn = 64, 8
    dsum = (z(H * 2, rn), torch.full((2,), rn, dtype=torch.int32, device=dev), z(c), z(c), z(H * 2, c), z(H * 2, c), 2, rn, H)
    with pytest.raises(ValueError, match='4 heads x 16 only'):
        run_fwd(abi, dev, stream, x, coeff, bias, cache, n, y2, w_cat, b_cat, dsum=dsum)
    x, coeff, bias, _, _, _, _, _, cache, n = filter_case(bsz=2, shape='pattern', n_min=65, n_max=65, k_eig=16)
    assert n == 65
    g, y2, w_cat, b_cat = _cat_operands(n, 2, 1)
    with pytest.raises(ValueError, match='8 heads x 8'):
        run_fwd(abi, dev, stream, x, coeff, bias, cache, n, y2, w_cat, b_cat)
    with pytest.raises(ValueError, match='8 heads x 8'):
        run_bwd(abi, dev, stream, x, coeff, cache, n, torch.zeros(n, 2, DM, dtype=torch.float64), y2, y2, w_cat, None)


# ---- model level ------------------------------------------------------------------------------------------------------------
FOLDED = ('feta_spec_filter_cat_fwd', 'feta_spec_filter_cat_bwd')
UNFOLDED = ('feta_spec_filter_fwd', 'feta_spec_filter_bwd')
NEVER = ('feta_spec_filter_cat_fwd_coeff', 'feta_ffn_bwd_coeff_saved', 'feta_coeff_dsum', 'feta_coeff_bwd_saved')


def model8(dev, batch_norm=True, bsz=3, n_min=9, n_max=30, layers=2, seed=0):
    """coeff_saved_checks.headline_model at 8 heads of 8, BatchNorm or LayerNorm (order 4, eigenbasis filter, every head on
    the graph, the whole basis: graphs of up to 32 nodes on K = N_pad eigenvectors, where the filter is the oracle's)"""
    torch.manual_seed(seed)
    model = DiffGraphTransformerGenGCN(7, 1, DM, H, dim_feedforward=128, dropout=0.0, nb_layers=layers, batch_norm=batch_norm,
                                       filter_order=ORDER, heads_share_graph=True, filter_mode='spectral')
    with torch.no_grad():
        model.encoder.spectral_gnns.bias.normal_(0, 0.1)
        model.encoder.gcn.bias.normal_(0, 0.1)
    ds = D.SyntheticGraphDataset('zinc', bsz, in_dim=7, seed=seed, pos_enc=True, n_min=n_min, n_max=n_max)
    n_pad = (max(s.num_nodes for s in ds.samples) + 3) // 4 * 4
    assert n_pad <= 32
    batch9, cache = D.collate(ds.samples, n_pad=n_pad, k_eig=n_pad, device=dev)
    return model.to(dev), batch9, cache


def rowlin_calls(calls):
    return [c for c in calls if 'rowlin' in c]


def check_launch_names(abi, dev, hook, monkeypatch, batch_norm):
    """a training step of an 8-head model runs the filter stage as the two folded launches - no general filter launch, no
    row-linear launch for linear_cat, none of the 4-head-only role entries; with the fold switched off (FETA_CAT_FOLD=0) it
    calls what it called before the 8-head form existed"""
    monkeypatch.setattr(FF, 'USE_COEFF_DSUM', True)
    model, batch9, cache = model8(dev, batch_norm)
    monkeypatch.setattr(FF, 'USE_CAT_FOLD', True)
    monkeypatch.setattr(FF, 'USE_CAT_FOLD_BWD', True)
    with Counter(abi) as on:
        run_step(model, batch9, cache, hook)
    monkeypatch.setattr(FF, 'USE_CAT_FOLD', False)
    with Counter(abi) as off:
        run_step(model, batch9, cache, hook)
    monkeypatch.setattr(FF, 'USE_CAT_FOLD', True)
    monkeypatch.setattr(FF, 'USE_CAT_FOLD_BWD', False)
    with Counter(abi) as fwd_only:
        run_step(model, batch9, cache, hook)
    assert all(on.calls.count(k) == 1 for k in FOLDED), on.calls
    assert not any(k in on.calls for k in UNFOLDED + NEVER), on.calls
    assert all(off.calls.count(k) == 1 for k in UNFOLDED), off.calls
    assert not any(k in off.calls for k in FOLDED + NEVER), off.calls
    # linear_cat: a row-linear launch in each direction without the fold, none with it
    assert len(rowlin_calls(off.calls)) == len(rowlin_calls(on.calls)) + 2, (rowlin_calls(on.calls), rowlin_calls(off.calls))
    assert len(on.calls) < len(off.calls), (on.calls, off.calls)
    # FETA_CAT_FOLD_BWD=0: the forward fold alone
    assert 'feta_spec_filter_cat_fwd' in fwd_only.calls and 'feta_spec_filter_bwd' in fwd_only.calls, fwd_only.calls
    assert 'feta_spec_filter_cat_bwd' not in fwd_only.calls and not any(k in fwd_only.calls for k in NEVER), fwd_only.calls
    return on.calls, off.calls


def oracle_step(model, batch9, layers, batch_norm):
    x, mask, pe, _, degree, _, edge_index, batch, fi = [None if t is None else t.cpu() for t in batch9]
    p64 = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items()
           if v.dtype.is_floating_point and 'running_' not in k}
    out_ref, coeff_ref = O.graph_transformer_gengcn(x.double(), edge_index, batch, fi, mask, pe.double(), degree.double(), p64,
                                                    num_layers=layers, num_heads=H, order=ORDER, batch_norm=batch_norm,
                                                    heads_share_graph=True)
    w = torch.linspace(0.5, 1.5, out_ref.numel(), dtype=torch.float64).view_as(out_ref)
    ((out_ref * w).sum() + 0.01 * coeff_ref.pow(2).sum()).backward()
    return out_ref.detach(), coeff_ref.detach(), {k: v.grad for k, v in p64.items() if v.grad is not None}


def _rel(got, ref):
    return KC.maxdiff(got, ref) / max(1.0, ref.abs().max().item())


def check_fold_on_off(abi, dev, hook, monkeypatch, batch_norm, bsz=3, layers=2):
    """the folded and the unfolded path on the same inputs, both against the fp64 oracle at the project's bars (output and
    coefficients TOL, every parameter gradient 3e-5), and the folded path's error within GUARD_FACTOR x the unfolded
    path's (floor GUARD_FLOOR)"""
    model, batch9, cache = model8(dev, batch_norm, bsz=bsz, layers=layers)
    monkeypatch.setattr(FF, 'USE_CAT_FOLD_BWD', True)
    res = {}
    for name, sw in (('on', True), ('off', False)):
        monkeypatch.setattr(FF, 'USE_CAT_FOLD', sw)
        with Counter(abi) as c:
            res[name] = run_step(model, batch9, cache, hook)
        assert ('feta_spec_filter_cat_bwd' in c.calls) == sw, c.calls
    ref = oracle_step(model, batch9, layers, batch_norm)
    errs = {}
    for name, r in res.items():
        KC.assert_close('h8 cat model output (fold %s)' % name, r[0], ref[0])
        KC.assert_close('h8 cat model coefficients (fold %s)' % name, r[1], ref[1])
        assert r[2].keys() == ref[2].keys(), (sorted(r[2].keys() ^ ref[2].keys()))
        for k, gk in r[2].items():
            KC.assert_close('h8 cat model grad %s (fold %s)' % (k, name), gk, ref[2][k], tol=3e-5)
        errs[name] = dict(output=_rel(r[0], ref[0]), coefficients=_rel(r[1], ref[1]),
                          **{k: _rel(gk, ref[2][k]) for k, gk in r[2].items()})
    worst = max(errs['on'], key=lambda k: errs['on'][k] / max(errs['off'][k], KC.GUARD_FLOOR / KC.GUARD_FACTOR))
    print('heads8 cat fold on/off', dict(batch_norm=batch_norm, bsz=bsz), 'output %.2e / %.2e, worst ratio %s %.2e / %.2e'
          % (errs['on']['output'], errs['off']['output'], worst, errs['on'][worst], errs['off'][worst]))
    for k in errs['on']:
        assert errs['on'][k] <= max(KC.GUARD_FACTOR * errs['off'][k], KC.GUARD_FLOOR), (k, errs['on'][k], errs['off'][k])
    return errs


def check_inference(abi, dev, hook, monkeypatch, batch_norm):
    """an eval-mode forward under torch.inference_mode goes through the folded launch.  LayerNorm: against the fp64 oracle at
    TOL.  BatchNorm: the oracle normalises with batch statistics only, so the eval-mode model (running statistics moved off
    their defaults) is held against its own unfolded forward, at TOL as well."""
    model, batch9, cache = model8(dev, batch_norm)
    x, mask, pe, _, degree, _, edge_index, batch, fi = batch9
    if batch_norm:
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for k, b in model.named_buffers():
                if k.endswith('running_mean'):
                    b.copy_((torch.randn(b.shape, generator=g) * 0.1).to(dev))
                elif k.endswith('running_var'):
                    b.copy_((torch.rand(b.shape, generator=g) + 0.5).to(dev))
    model.eval()

    def forward():
        with hook(), Counter(abi) as c, torch.inference_mode():
            out, _, coeff = model(x, edge_index, batch, fi, mask, pe, degree=degree, return_filter_coeff=True, graph_cache=cache)
        return out, coeff, c.calls
    monkeypatch.setattr(FF, 'USE_CAT_FOLD', True)
    out, coeff, calls = forward()
    assert 'feta_spec_filter_cat_fwd' in calls and 'feta_spec_filter_fwd' not in calls, calls
    assert not rowlin_calls(calls) and not any(k in calls for k in NEVER), calls
    if batch_norm:
        monkeypatch.setattr(FF, 'USE_CAT_FOLD', False)
        out_ref, coeff_ref, calls = forward()
        assert 'feta_spec_filter_fwd' in calls and 'feta_spec_filter_cat_fwd' not in calls, calls
        out_ref, coeff_ref = out_ref.double().cpu(), coeff_ref.double().cpu()
    else:
        xc, maskc, pec, _, degc, _, eic, bc, fic = [None if t is None else t.cpu() for t in batch9]
        p64 = {k: v.detach().cpu().double() for k, v in model.state_dict().items() if v.dtype.is_floating_point}
        with torch.no_grad():
            out_ref, coeff_ref = O.graph_transformer_gengcn(xc.double(), eic, bc, fic, maskc, pec.double(), degc.double(), p64,
                                                            num_layers=2, num_heads=H, order=ORDER, batch_norm=False,
                                                            heads_share_graph=True)
    return {'output': KC.assert_close('h8 cat inference output', out, out_ref),
            'coefficients': KC.assert_close('h8 cat inference coefficients', coeff, coeff_ref)}


def check_bench_step(dev, run_ctx, abi, argv):
    """heads8_checks.check_bench_step_heads8 (what bench.py times against oracle.encoder_gengcn), and the captured step
    contains the two folded launches"""
    import heads8_checks as H8
    with Counter(abi) as c:
        errs, used_graph = H8.check_bench_step_heads8(dev, run_ctx, abi, argv)
    assert 'feta_spec_filter_cat_fwd' in c.calls and 'feta_spec_filter_cat_bwd' in c.calls, sorted(set(c.calls))
    assert 'feta_spec_filter_fwd' not in c.calls and 'feta_spec_filter_bwd' not in c.calls, sorted(set(c.calls))
    return errs, used_graph
