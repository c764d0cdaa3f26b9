"""Global stores with a cache policy (csrc/feta_gstore.h) on the MI355X.

The policy changes no value, so these tests aim at what a hand-chosen store instruction can break: its width, its
address, tail predicates and masked lanes.  Every device tensor the existing checkers (kernel_checks.py, lin_dw_checks.py)
allocate while a `Guard` is active - all outputs of the touched entry points among them - is a view into a larger
allocation whose 256-byte margins hold a bit pattern; the checkers compare the results with their fp64 references at
their own tolerances (they pre-fill outputs with NaN, so an element a store missed fails there), the guard then requires
every margin intact.  Shapes: the smallest at which the paths differ - B = 3 / N_pad = 17 with 17, 16 and 1 real nodes
(two row tiles, the second holding one row; a graph whose second key tile is never written), B = 2 / N_pad = 37 with 37
and 33 (NT = 3, the headline's instantiation), and B = 5 with the walking forms forced (a workgroup's first graph stores
its partial row, the later ones add to it: plain stores and adds, beside the policy stores of the other tensors).
d = 64, 4 heads."""
import contextlib

import pytest
import torch

import coeff_saved_checks as CS
import kernel_checks as KC
import lin_dw_checks as LD
from feta_tmlr_amd import train as T

pytestmark = pytest.mark.gpu

MARGIN = 256          # bytes on both sides of every guarded tensor
PATTERN = 0xA5

# (B, N_pad, n_min, seed): the seed makes the checkers' generator draw exactly the sizes named above
SHAPES = [(3, 17, 1, 99), (2, 37, 33, 10)]
SIZES = {(3, 17): [17, 16, 1], (2, 37): [37, 33]}


class Guard:
    """While active, torch.full / empty / zeros (and the *_like, Tensor.new_* forms) for a CUDA device return views into
    larger allocations with patterned margins.  check(): every margin still holds the pattern."""

    def __init__(self):
        self.allocs = []

    def _is_cuda(self, device):
        return device is not None and torch.device(device).type == 'cuda'

    def _alloc(self, shape, dtype, device, init):
        shape = tuple(int(s) for s in shape)
        dtype = dtype or torch.get_default_dtype()
        n = 1
        for s in shape:
            n *= s
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        pad = (-nbytes) % 16
        raw = self._empty((nbytes + pad + 2 * MARGIN,), dtype=torch.uint8, device=device)
        raw.fill_(PATTERN)
        t = raw[MARGIN:MARGIN + nbytes].view(dtype).view(shape)
        if init is not None:
            t.fill_(init)
        self.allocs.append((raw, nbytes))
        return t

    @staticmethod
    def _shape(args):
        if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
            return tuple(args[0])
        return tuple(args)

    def __enter__(self):
        g = self
        self.saved = (torch.full, torch.empty, torch.zeros, torch.empty_like, torch.zeros_like, torch.Tensor.new_empty,
                      torch.Tensor.new_zeros, torch.Tensor.new_full)
        full, empty, zeros, empty_like, zeros_like, new_empty, new_zeros, new_full = self.saved
        self._empty = empty

        def plain(kw):
            return set(kw) <= {'dtype', 'device'}

        def p_full(size, fill_value, **kw):
            if plain(kw) and g._is_cuda(kw.get('device')) and not isinstance(fill_value, torch.Tensor):
                return g._alloc(size, kw.get('dtype'), kw['device'], fill_value)
            return full(size, fill_value, **kw)

        def p_empty(*a, **kw):
            if plain(kw) and g._is_cuda(kw.get('device')) and all(isinstance(s, int) for s in g._shape(a)):
                return g._alloc(g._shape(a), kw.get('dtype'), kw['device'], None)
            return empty(*a, **kw)

        def p_zeros(*a, **kw):
            if plain(kw) and g._is_cuda(kw.get('device')) and all(isinstance(s, int) for s in g._shape(a)):
                return g._alloc(g._shape(a), kw.get('dtype'), kw['device'], 0)
            return zeros(*a, **kw)

        def p_empty_like(t, **kw):
            if set(kw) <= {'dtype'} and t.is_cuda and t.is_contiguous():
                return g._alloc(t.shape, kw.get('dtype', t.dtype), t.device, None)
            return empty_like(t, **kw)

        def p_zeros_like(t, **kw):
            if set(kw) <= {'dtype'} and t.is_cuda and t.is_contiguous():
                return g._alloc(t.shape, kw.get('dtype', t.dtype), t.device, 0)
            return zeros_like(t, **kw)

        def p_new_empty(t, *a, **kw):
            if set(kw) <= {'dtype'} and t.is_cuda and all(isinstance(s, int) for s in g._shape(a)):
                return g._alloc(g._shape(a), kw.get('dtype', t.dtype), t.device, None)
            return new_empty(t, *a, **kw)

        def p_new_zeros(t, *a, **kw):
            if set(kw) <= {'dtype'} and t.is_cuda and all(isinstance(s, int) for s in g._shape(a)):
                return g._alloc(g._shape(a), kw.get('dtype', t.dtype), t.device, 0)
            return new_zeros(t, *a, **kw)

        def p_new_full(t, size, fill_value, **kw):
            if set(kw) <= {'dtype'} and t.is_cuda and not isinstance(fill_value, torch.Tensor):
                return g._alloc(size, kw.get('dtype', t.dtype), t.device, fill_value)
            return new_full(t, size, fill_value, **kw)

        (torch.full, torch.empty, torch.zeros, torch.empty_like, torch.zeros_like, torch.Tensor.new_empty,
         torch.Tensor.new_zeros, torch.Tensor.new_full) = (p_full, p_empty, p_zeros, p_empty_like, p_zeros_like,
                                                           p_new_empty, p_new_zeros, p_new_full)
        return self

    def __exit__(self, *exc):
        (torch.full, torch.empty, torch.zeros, torch.empty_like, torch.zeros_like, torch.Tensor.new_empty,
         torch.Tensor.new_zeros, torch.Tensor.new_full) = self.saved

    def check(self, at_least=1):
        torch.cuda.synchronize()
        assert len(self.allocs) >= at_least, 'the guard saw %d allocations' % len(self.allocs)
        for i, (raw, nbytes) in enumerate(self.allocs):
            lo, hi = raw[:MARGIN], raw[MARGIN + nbytes:]
            assert bool((lo == PATTERN).all()), 'allocation %d (%d bytes): a store in front of the tensor' % (i, nbytes)
            assert bool((hi == PATTERN).all()), 'allocation %d (%d bytes): a store behind the tensor' % (i, nbytes)


def test_guard_sees_a_stray_store(hip):
    """the guard itself: one byte next to a tensor is found, on either side"""
    dev = hip[1]
    for off in (-1, 0):
        with Guard() as g:
            t = torch.full((5, 3), float('nan'), device=dev)
        g.check()
        raw, nbytes = g.allocs[0]
        assert t.data_ptr() == raw.data_ptr() + MARGIN and nbytes == 60
        raw[MARGIN + (nbytes if off == 0 else -1)] = 0
        with pytest.raises(AssertionError):
            g.check()


def _sizes_are(bsz, n_pad, n_min, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(n_min, n_pad + 1, (bsz,), generator=g)
    n[0] = n_pad
    assert n.tolist() == SIZES[(bsz, n_pad)], n.tolist()


@pytest.mark.parametrize('bsz,n_pad,n_min,seed', SHAPES)
def test_attn_block_bf16(hip, bsz, n_pad, n_min, seed):
    """attn_block_fwd / bwd on bf16 storage (the 8-byte and 16-byte helpers; fp32 attn, attn_stats and partial rows): qkv,
    out, attn, attn_stats, y, y_stats; dx, dx_b, sum_out and the partial rows of both backward forms"""
    abi, dev, stream = hip
    _sizes_are(bsz, n_pad, n_min, seed)
    with Guard() as g:
        r = KC.check_attn_block_lp(abi, dev, stream, bsz=bsz, n_pad=n_pad, n_min=n_min, seed=seed)
        # (the BatchNorm fold of the incoming gradient changes no store.  It is checked where the checker's bf16 tolerance
        # holds for it: at B = 2 its db_out is 1.455e-01 off on a scale of 6.01, 2.4 %, on the parent and on the host
        # emulation alike - 74 rows of bf16-rounded y1 under their own statistics)
        for split in (False, True):
            KC.check_attn_block_bwd_lp(abi, dev, stream, bsz=bsz, n_pad=n_pad, n_min=n_min, seed=seed, split=split,
                                       with_bn=bsz == 3)
    g.check(at_least=10)
    # what the contract leaves unwritten keeps its pre-filled value: K / V rows of a key tile without a real node
    qkv = r['qkv'].view(n_pad, bsz, 3, 64).float()
    for b, n in enumerate(SIZES[(bsz, n_pad)]):
        for tile in range((n_pad + 15) // 16):
            if 16 * tile >= n:
                assert bool(torch.isnan(qkv[16 * tile:16 * tile + 16, b, 1:]).all()), (b, n, tile)


@pytest.mark.parametrize('bsz,n_pad,n_min,seed', SHAPES)
def test_attn_block_fp32(hip, bsz, n_pad, n_min, seed):
    """the same launches on fp32 storage (4-byte and 16-byte stores), one workgroup per graph and SPLIT"""
    abi, dev, stream = hip
    _sizes_are(bsz, n_pad, n_min, seed)
    with Guard() as g:
        KC.check_attn_block_ln(abi, dev, stream, bsz=bsz, n_pad=n_pad, n_min=n_min, seed=seed, dtype=torch.float32)
        for split in (False, True):
            KC.check_attn_block_bwd_ln(abi, dev, stream, bsz=bsz, n_pad=n_pad, n_min=n_min, seed=seed, dtype=torch.float32,
                                       split=split)
    g.check(at_least=10)


@pytest.mark.parametrize('m', [3 * 17, 2 * 37])
def test_ffn(hip, m):
    """ffn_fwd (h, y2, y_stats) and ffn_bwd (dx, sum_out, partial rows): a last row block of 19 / 10 rows"""
    abi, dev, stream = hip
    with Guard() as g:
        KC.check_ffn_lp(abi, dev, stream, m=m)
        KC.check_ffn_bwd_lp(abi, dev, stream, m=m)
        KC.check_ffn_ln(abi, dev, stream, m=m, dtype=torch.float32)
        KC.check_ffn_bwd_ln(abi, dev, stream, m=m, dtype=torch.float32)
    g.check(at_least=8)


@pytest.mark.parametrize('bsz,n_min,n_max', [(3, 2, 17), (2, 33, 37)])
def test_spec_cat(hip, bsz, n_min, n_max):
    """spec_cat_fwd (filt, the encoder output) and spec_cat_bwd (dx, dxn, partial rows, dcoeff, dbias_part)"""
    abi, dev, stream = hip
    with Guard() as g:
        KC.check_spec_cat(abi, dev, stream, bsz=bsz, n_min=n_min, n_max=n_max)
        KC.check_spec_cat_bwd(abi, dev, stream, bsz=bsz, n_min=n_min, n_max=n_max)
    g.check(at_least=6)


def test_coeff_and_colsum(hip):
    """the coefficient generator (cj, pooled, partial sums) and the column sums, tall and wide"""
    abi, dev, stream = hip
    with Guard() as g:
        KC.check_coeff(abi, dev, stream, 3, 17, 4, 256)
        KC.check_coeff(abi, dev, stream, 2, 37, 4, 1024, faithful=False)
        KC.check_colsum(abi, dev, stream, 37, 70)
        KC.check_colsum_multi_mixed(abi, dev, stream)
    g.check(at_least=4)


def test_lin_dw_role_r64_c256(hip):
    """dW / db of the role (8-byte stores) at R = 64, C = 256 beside the main grid"""
    abi, dev, stream = hip
    with Guard() as g:
        blk = LD.block_case(abi, dev, stream)
        base = LD.launch(abi, stream, blk)
        LD.check_kernel(abi, stream, blk, LD.dw_case(64, 256, dev), base)
    g.check(at_least=6)


def _oracle_step(model, batch9, cache, layers):
    """fp64 oracle of CS.run_step's loss in the eigenbasis the kernels read (K = 16 of N_pad = 40 truncates the operator,
    the whole basis is the reference's): -> (out, parameter gradients)"""
    from oracle import feta_oracle as O
    x, mask, pe, _, degree, _, edge_index, batch, fi = [None if t is None else t.cpu() for t in batch9]
    c = cache.to(torch.device('cpu'))
    p64 = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items()
           if v.dtype.is_floating_point and 'running_' not in k}
    out, coeff = O.graph_transformer_gengcn(x.double(), edge_index, batch, fi, mask, pe.double(), degree.double(), p64,
                                            num_layers=layers, num_heads=4, order=4, batch_norm=True, heads_share_graph=True,
                                            eig=(c.u.double(), c.lam.double()))
    w = torch.linspace(0.5, 1.5, out.numel(), dtype=torch.float64).view_as(out)
    ((out * w).sum() + 0.01 * coeff.pow(2).sum()).backward()
    return out.detach(), {k: v.grad for k, v in p64.items()}


def stack_step(abi, dev, hook, bsz, n_min, n_max, guarded=True):
    """one training step of a two-layer BatchNorm stack with the filter stage and the linear_cat fold (the headline's layer
    shape), every allocation of the step guarded, against the fp64 oracle at the bars of the module tests"""
    layers = 2
    model, batch9, cache = CS.headline_model(dev, bsz=bsz, n_min=n_min, n_max=n_max, layers=layers)
    with Guard() as g, CS.Counter(abi) as c:
        run = CS.run_step(model, batch9, cache, hook)
    if guarded:
        g.check(at_least=10)
    for name in ('feta_attn_block_fwd', 'feta_ffn_fwd', 'feta_ffn_bwd', 'feta_attn_block_bwd', 'feta_spec_filter_cat_fwd',
                 'feta_spec_filter_cat_bwd'):
        assert any(k.startswith(name) for k in c.calls), (name, c.calls)
    out_ref, g_ref = _oracle_step(model, batch9, cache, layers)
    KC.assert_close('stack output', run[0], out_ref)
    assert len(run[2]) > 10
    for k, gk in run[2].items():
        KC.assert_close('stack grad ' + k, gk, g_ref[k], tol=3e-5)
    return run


@pytest.mark.parametrize('bsz,n_min,n_max', [(3, 9, 17), (2, 33, 37)])
def test_stack_step(hip, bsz, n_min, n_max):
    """N_pad = 20 on the whole eigenbasis (two row tiles) and N_pad = 40 on K = 16 (NT = 3, the headline's instantiations)"""
    stack_step(hip[0], hip[1], contextlib.nullcontext, bsz, n_min, n_max)


def test_stack_step_walking_forms(hip, monkeypatch):
    """more graphs than workgroups: the first graph of a workgroup stores its partial row, the later ones add to it"""
    monkeypatch.setenv('FETA_BLOCK_BWD_MAX_GRID', '2')
    monkeypatch.setenv('FETA_FFN_MAX_GRID', '2')
    stack_step(hip[0], hip[1], contextlib.nullcontext, 5, 33, 37)


def test_captured_step_replays_equal(hip, monkeypatch):
    """a captured step at B = 3, replayed twice from the same state: a store that lands after its launch's boundary would
    show as a gradient that differs between the replays"""
    dev = hip[1]
    model, batch9, cache = CS.headline_model(dev, bsz=3, n_min=9, n_max=17, layers=2)
    crit = T.make_criterion('zinc', nb_class=1)
    opt = T.make_optimizer('zinc', model.parameters(), lr=1e-3, capturable=True)
    graphed = T.GraphedTrainStep('zinc', model, crit, opt, batch9, cache)
    snap = graphed._snapshot()
    grads = []
    for _ in range(2):
        graphed(batch9, cache)
        torch.cuda.synchronize()
        grads.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
        graphed._restore(snap)
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 10
    for k in grads[0]:
        assert bool(torch.isfinite(grads[0][k]).all()) and torch.equal(grads[0][k], grads[1][k]), k
