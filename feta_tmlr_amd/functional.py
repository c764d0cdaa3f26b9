"""torch.autograd.Function wrappers over the C ABI (include/feta_hip.h).

Token tensors are handed to the kernels as [B, N, H, dh] *views* with explicit strides, so the
reference's seq-first [N, B, d] activations (transformer/models.py:521-527) are consumed and
produced in place: no transposes, no gathers, no scatter into zero-initialised buffers.
"""
import torch

from . import _abi, _lib
from ._abi import CoeffSavedReq, LinDwReq


def _token_view(t, batch_first, heads):
    """[N,B,d] (seq-first) or [B,N,d] (batch-first) -> [B,N,H,dh] view (no copy)."""
    d = t.shape[-1]
    v = t.view(t.shape[0], t.shape[1], heads, d // heads)
    return v if batch_first else v.permute(1, 0, 2, 3)


def _dense_like(t, batch_first):
    """grad arriving as a [B,N,H,dh]-shaped tensor -> same values in the storage order the
    kernels were given (dense (H,dh), 16-byte aligned rows)."""
    if batch_first:
        return t.contiguous()
    return t.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)


def _new_token(b, n, h, dh, batch_first, ref):
    """same storage dtype as ref (fp32, or bf16 on the bf16 storage path)"""
    if batch_first:
        return torch.empty((b, n, h, dh), dtype=ref.dtype, device=ref.device)
    return torch.empty((n, b, h, dh), dtype=ref.dtype, device=ref.device).permute(1, 0, 2, 3)


class AttentionCoreFn(torch.autograd.Function):
    """qkv (projected, [N,B,3d] or [B,N,3d]) -> (concat heads in the same token layout,
    attn [B,H,N,N] or None).  C ABI: feta_attn_fwd / feta_attn_bwd."""

    @staticmethod
    def forward(ctx, qkv, pe, n_real, num_heads, need_attn, tie_qk, batch_first, drop=None, clamp5=False):
        abi, stream = _lib.backend(qkv, pe, n_real)
        ctx.set_materialize_grads(False)   # no zero tensor for the non-differentiable attn output
        qkv = qkv.contiguous()
        l0, l1, d3 = qkv.shape
        d = d3 // 3
        dh = d // num_heads
        b, n = (l0, l1) if batch_first else (l1, l0)
        v5 = qkv.view(l0, l1, 3, num_heads, dh)
        sel = (lambda i: v5[:, :, i]) if batch_first else (lambda i: v5[:, :, i].permute(1, 0, 2, 3))
        q, k, v = sel(0), (sel(0) if tie_qk else sel(1)), sel(2)
        out = _new_token(b, n, num_heads, dh, batch_first, qkv)
        attn = torch.empty((b, num_heads, n, n), dtype=qkv.dtype, device=qkv.device) if need_attn else None
        stats = torch.empty((b, num_heads, n, 2), dtype=torch.float32, device=qkv.device)
        pe_c = None if pe is None else pe.to(qkv.dtype).contiguous()   # (bf16 storage: pe travels as bf16 too)
        scale = float(dh) ** -0.5
        abi.attn_fwd(q, k, v, pe_c, n_real, out, attn, stats, scale, stream, drop=drop, clamp5=clamp5)
        ctx.clamp5 = bool(clamp5)
        ctx.save_for_backward(qkv, pe_c, n_real, out, stats)
        ctx.cfg = (num_heads, tie_qk, batch_first, scale)
        ctx.drop = drop
        concat = (out if batch_first else out.permute(1, 0, 2, 3)).reshape(l0, l1, d)
        if attn is not None:
            ctx.mark_non_differentiable(attn)   # enters A2 detached (transformer/models.py:282)
        return concat, attn

    @staticmethod
    def backward(ctx, dconcat, _dattn):
        qkv, pe_c, n_real, out, stats = ctx.saved_tensors
        if dconcat is None:
            return (None,) * 9
        num_heads, tie_qk, batch_first, scale = ctx.cfg
        abi, stream = _lib.backend(qkv)
        l0, l1, d3 = qkv.shape
        d = d3 // 3
        dh = d // num_heads
        b, n = (l0, l1) if batch_first else (l1, l0)
        v5 = qkv.view(l0, l1, 3, num_heads, dh)
        dqkv = torch.empty_like(qkv)
        g5 = dqkv.view(l0, l1, 3, num_heads, dh)
        if batch_first:
            sel, gsel = (lambda i: v5[:, :, i]), (lambda i: g5[:, :, i])
        else:
            sel = lambda i: v5[:, :, i].permute(1, 0, 2, 3)
            gsel = lambda i: g5[:, :, i].permute(1, 0, 2, 3)
        q, k, v = sel(0), (sel(0) if tie_qk else sel(1)), sel(2)
        dout = _token_view(dconcat.to(qkv.dtype).contiguous(), batch_first, num_heads)
        delta = torch.empty((b, num_heads, n), dtype=torch.float32, device=qkv.device)
        abi.attn_bwd(q, k, v, pe_c, n_real, out, dout, stats, delta, gsel(0), gsel(1), gsel(2),
                     scale, stream, drop=ctx.drop, clamp5=ctx.clamp5)
        if tie_qk:
            dqkv[..., :d] += dqkv[..., d:2 * d]
            dqkv[..., d:2 * d] = 0
        return dqkv, None, None, None, None, None, None, None, None


def _coeff_forward(abi, stream, attn, n_real, gcn_weight, gcn_bias, pending=None):
    """The coefficient generator's forward (feta_colsum, feta_coeff_fwd) -> (pooled [H*B, C], cj, s, gcn bias) - or
    whatever of it the layer stack's launches already ran (pending: the forward hand-over of PendingSums)."""
    attn = attn.contiguous()
    b, h, n, _ = attn.shape
    c = gcn_weight.shape[1]
    dev = attn.device
    if pending is not None and pending.s is not None:
        s = pending.s                 # requested by the encoder ...
        left = pending.take_fwd()     # ... and computed inside the layer stack's first launch, or not yet
        if left:
            abi.colsum_multi(left, stream)
        pending.s = None
    else:
        s = torch.empty(c, dtype=torch.float32, device=dev)
        abi.colsum(gcn_weight.contiguous(), s, stream)
    gb = gcn_bias.contiguous()
    if pending is not None and pending.coeff_fwd_out is not None:
        cj, pooled = pending.coeff_fwd_out      # ran in the launch of the last layer's feed-forward half
        pending.coeff_fwd_out = None
    else:
        cj = torch.empty((h * b, n), dtype=torch.float32, device=dev)
        pooled = torch.empty((h * b, c), dtype=torch.float32, device=dev)
        abi.coeff_fwd(attn, n_real, s, gb, cj, pooled, stream)
    if pending is not None:
        pending.coeff_fwd_req = None
    return pooled, cj, s, gb


def _coeff_backward(abi, stream, cj, n_real, s, gb, dims, dpooled, saved=None, pending=None, params=(), waiting=(),
                    owners=()):
    """The coefficient generator's backward -> (dW, db) of the GCN parameters.  dims = (B, N, H, rows of gcn.weight).
    saved = (A, Bm): the tanh pass already ran (feta_coeff_dsum) and what is left is a multiply-and-column-sum; else the
    kernel recomputes the tanh.  waiting / owners: column sums (and the gradients they complete) that earlier steps of the
    same backward left for this step's reduction launch.  pending with the stack's backward still to come in this pass and
    params = (gcn.weight, gcn.bias) untouched: kernel and sums are left to the stack's launches."""
    b, n, h, rows = dims
    c = s.shape[0]
    dsdb = torch.empty((2, c), dtype=torch.float32, device=cj.device)   # contiguous: one reduction
    ds, db = dsdb[0], dsdb[1]
    # s = 1^T W  =>  every row of dW equals ds: the reduction launch writes the dense rows itself (an
    # expanded view would be copied into a dense .grad by autograd: one more 4 MB kernel per step)
    dw = torch.empty((rows, c), dtype=torch.float32, device=cj.device)
    dpc = dpooled.contiguous()
    if saved is not None and torch.is_grad_enabled():
        saved = None        # a backward under grad mode (create_graph=True): the recompute form, as it stands
    if saved is not None:
        A, Bm = saved
        partial = torch.empty((abi.coeff_bwd_saved_groups(b, h), 2, c), dtype=torch.float32, device=cj.device)
        req = CoeffSavedReq(dpc, A, Bm, partial, b, h)
        run = lambda ds_, db_, **kw: abi.coeff_bwd_saved(dpc, A, Bm, partial, ds_, db_, b, h, stream, **kw)
    else:
        partial = torch.empty((abi.coeff_bwd_groups(b, h), 2, c), dtype=torch.float32, device=cj.device)
        req = (cj, n_real, s, gb, dpc, partial, b, n, h)
        run = lambda ds_, db_, **kw: abi.coeff_bwd(cj, n_real, s, gb, dpc, partial, ds_, db_, b, n, h, stream, **kw)
    p2 = partial.view(-1, 2 * c)
    if pending is not None and pending.stack_armed and not pending.stack_done and PendingSums.untouched(*params):
        # the layer stack's backward comes after this node: its first launch carries the kernel in trailing workgroups
        # (feta_ffn_bwd_coeff[_saved]), its reduction launch the sums
        pending.coeff_bwd_req = req
        for item in waiting:
            pending.add(*item)
        pending.owners += owners
        pending.add(p2[:, :c], ds, dw, owners=[(params[0], dw)])
        pending.add(p2[:, c:], db, owners=[(params[1], db)])
    elif waiting:
        # ONE reduction launch for this step's partials and every column sum the steps before it left
        run(None, None)
        abi.colsum_multi([(p2[:, :c], ds, dw), (p2[:, c:], db)] + list(waiting), stream)
    else:
        run(ds, db, dw_dense=dw)
    return dw, db


class FilterCoefficientsFn(torch.autograd.Function):
    """attn [B,H,N,N] (detached) + GCN parameters -> pooled [H*B, C]
    (transformer/models.py:240-283 collapsed; C ABI: feta_colsum, feta_coeff_fwd/bwd)."""

    @staticmethod
    def forward(ctx, attn, n_real, gcn_weight, gcn_bias):
        abi, stream = _lib.backend(attn, gcn_weight)
        pooled, cj, s, gb = _coeff_forward(abi, stream, attn, n_real, gcn_weight, gcn_bias)
        ctx.save_for_backward(cj, n_real, s, gb)
        ctx.dims = (attn.shape[0], attn.shape[2], attn.shape[1], gcn_weight.shape[0])
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        cj, n_real, s, gb = ctx.saved_tensors
        abi, stream = _lib.backend(cj)
        dw, db = _coeff_backward(abi, stream, cj, n_real, s, gb, ctx.dims, dpooled)
        return None, None, dw, db

class DenseLinearFn(torch.autograd.Function):
    """y = x W^T + b for the C x C ``self.linear`` of the coefficient generator
    (transformer/models.py:284): the three GEMMs stay rocBLAS (plain library GEMMs), the bias
    gradient is one feta_colsum instead of a generic reduction kernel."""

    @staticmethod
    def forward(ctx, x, w, bias):
        ctx.save_for_backward(x, w)
        with _lib.tuned_gemm():
            return torch.addmm(bias, x, w.t())

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        abi, stream = _lib.backend(dy)
        dy = dy.contiguous()
        db = torch.empty(dy.shape[1], dtype=dy.dtype, device=dy.device)
        abi.colsum(dy, db, stream)
        with _lib.tuned_gemm():
            return dy.mm(w), dy.t().mm(x), db


def dense_linear(x, w, bias):
    return DenseLinearFn.apply(x, w, bias)


def _filter_forward(abi, stream, xs, g0, g1, cw, bias, n_real, mode, order, share, batch_first, cat=None):
    """The dynamic filter's forward launch -> y (token layout of xs).  cat: the further arguments of
    feta_spec_filter_cat_fwd - linear_cat rides in the launch (out = [xn | y] W_cat^T + b)."""
    b, n, h, dh = xs.shape
    y = _new_token(b, n, h, dh, batch_first, xs)
    if cat is not None:
        abi.spec_filter_cat_fwd(xs, g0, g1, cw, bias, n_real, y, order, share, stream, **cat)
    elif mode == 'cheb':
        abi.cheb_filter_fwd(xs, g0, cw, bias, n_real, y, order, share, stream)
    else:
        abi.spec_filter_fwd(xs, g0, g1, cw, bias, n_real, y, order, share, stream)
    return y


def _filter_backward(abi, stream, xs, g0, g1, coeff, n_real, dys, mode, order, share, batch_first, cat=None, y=None):
    """The dynamic filter's backward launch -> (dx, dcoeff, per-block partials of the bias gradient).  cat: the further
    arguments of feta_spec_filter_cat_bwd - linear_cat's backward rides in the launch, which then starts from cat['dout']
    instead of dys and needs the filter's output y."""
    b, n, h, dh = xs.shape
    dx = _new_token(b, n, h, dh, batch_first, xs)
    dcoeff = torch.empty_like(coeff)
    dbp = torch.empty((b * h, dh), dtype=torch.float32, device=xs.device)
    if cat is not None:
        abi.spec_filter_cat_bwd(xs, g0, g1, coeff, n_real, y, dx, dcoeff, dbp, order, share, stream, **cat)
    elif mode == 'cheb':
        abi.cheb_filter_bwd(xs, g0, coeff, n_real, dys, dx, dcoeff, dbp, order, share, stream)
    else:
        abi.spec_filter_bwd(xs, g0, g1, coeff, n_real, dys, dx, dcoeff, dbp, order, share, stream)
    return dx, dcoeff, dbp


class _FilterFn(torch.autograd.Function):
    """x [B,N,H,dh] view, coeff [H*B, P*dh*dh], bias [dh] -> y (same token layout as x),
    zero on padded rows.  mode 'cheb': graph = lhat [B,N,N]; mode 'spec': graph = (u, lam)."""

    @staticmethod
    def forward(ctx, x, coeff, bias, n_real, g0, g1, mode, order, share, batch_first):
        abi, stream = _lib.backend(x, coeff)
        xs = _dense_like(x, batch_first)
        coeff = coeff.contiguous()
        y = _filter_forward(abi, stream, xs, g0, g1, coeff, bias, n_real, mode, order, share, batch_first)
        ctx.save_for_backward(xs, coeff, n_real, g0, g1)
        ctx.cfg = (mode, order, share, batch_first, bias is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        xs, coeff, n_real, g0, g1 = ctx.saved_tensors
        mode, order, share, batch_first, has_bias = ctx.cfg
        abi, stream = _lib.backend(xs)
        dys = _dense_like(dy.to(xs.dtype), batch_first)
        dx, dcoeff, dbp = _filter_backward(abi, stream, xs, g0, g1, coeff, n_real, dys, mode, order, share, batch_first)
        dbias = None
        if has_bias:
            dbias = torch.empty(xs.shape[3], dtype=torch.float32, device=xs.device)
            abi.colsum(dbp, dbias, stream)
        return dx, dcoeff, dbias, None, None, None, None, None, None, None


import os as _os
# fp32 compute: above this many multiply-adds per product the C x C linear runs as library GEMMs.  Round 3 measured the
# LDS-tiled fp32 kernels of csrc/lin.hip at the BASELINE shape (2^29 MACs per product) against them: forward 15.7 vs
# 12.8 us, dX + dW (+ db + pending sums, one launch) 32.8 vs 25.8 us - the chip holds ~1.6 GHz under fp32 MFMA load, so
# the floor is 10.2 / 20.4 us and the library sits at 80 % of it; FETA_LIN_OWN_MAX_MACS=2147483648 selects ours (A/B).
# bf16 compute (bf16 storage legs) always takes the tiled kernels: 9.3 / 16.5 us, no cast launches.
LIN_OWN_GEMM_MAX_MACS = int(_os.environ.get('FETA_LIN_OWN_MAX_MACS', str(1 << 27)))
# bf16 compute (the bf16 storage legs): from this many rows H*B the three products run as LIBRARY bf16 GEMMs with fp32 output
# (torch.mm(..., out_dtype=float32) on bf16 copies of the operands - the same arithmetic as the tiled kernels of
# csrc/lin.hip: operands rounded to bf16, fp32 accumulation and result).  The tiled kernels read fp32 operands and win
# while the products are small (rows 512: 9.7 / 16.9 us against 33 / 52 us with the cast launches); at config 5's 4096
# rows they sit at 200 / 143 TFLOP/s (42.9 / 120.3 us) and the library, casts included, takes 35.5 / 60.3 us
# (tools/scratch/bf16_gemm_probe.py, eager).  Inside the captured step: 1024 rows 0.3683 vs 0.3651 ms (tiled kernels stay), 2048
# rows 0.547 vs 0.570 ms, 4096 rows (config 5) 1.08 vs 1.145 ms.
LIN_LIB_BF16_MIN_ROWS = int(_os.environ.get('FETA_LIN_LIB_BF16_MIN_ROWS', '2048'))


# The coefficient generator's kernels ride as trailing workgroups of a feed-forward launch while the batch leaves CUs idle
# there.  As a role they inherit the host kernel's two waves per SIMD; from this many (graph, head) blocks on, the stand-alone
# launches (eight waves per SIMD) are the faster form even with their launch cost: config 5 (4096 blocks) 1.040 -> 1.022 ms
# per step, the BASELINE batch (512 blocks) and config 4 (256 blocks of 128 nodes) the other way round.
COEFF_ROLE_MAX_BLOCKS = int(_os.environ.get('FETA_COEFF_ROLE_MAX', 2048))
# The tanh pass of the coefficient generator's backward (A, Bm: feta_coeff_dsum) rides in the filter stage's forward launch,
# and what stays in the stack's first backward launch is a multiply-and-column-sum (csrc/feta_coeff.h).  FETA_COEFF_DSUM=0:
# off - the backward recomputes the tanh in that launch, as before (A/B timing; EXPERIMENTS.md: 0.2579 -> 0.2535 ms at the
# headline, the last layer's ffn_bwd 19.6 -> 13.4 us, the filter launch 9.9 -> 11.0 us).
USE_COEFF_DSUM = _os.environ.get('FETA_COEFF_DSUM', '1') != '0'


# dW / db of the coefficient generator's C x C linear as a role of the first layer's attention backward - the stack's last
# launch, which leaves half the chip idle at the headline batch - instead of a library GEMM launch of its own
# (feta_attn_block_bwd_sums_dw, csrc/feta_lin_dw.h).  FETA_LIN_DW_ROLE: 0 off; 1 the default policy (the tiles fit the
# workgroup slots that launch leaves free in ONE round, and the batch is at most LIN_DW_ROLE_MAX_B graphs); 2 wherever the
# launch can carry it (tests: the role at the smallest shape it takes).  Read at every backward.
# Measured at the headline shape (C = 1024, N_pad = 37, role on against off, ms per step): B = 64 0.2173 -> 0.2121, B = 96
# 0.2408 -> 0.2310, B = 128 0.2523 -> 0.2476 (EXPERIMENTS.md); B = 32 takes csrc/lin.hip, not the library.  Nothing beyond 128
# graphs has been measured - at C = 1024 the 128 tiles no longer fit one round there anyway - so the default stops there.
LIN_DW_ROLE_MAX_B = 128


def lin_dw_role_mode():
    try:
        return int(_os.environ.get('FETA_LIN_DW_ROLE', '1'))
    except ValueError:
        return 1


def _owners(*pairs):
    """[(parameter, the gradient tensor its node returns)] without the absent ones, as second tensor objects on the same
    storage (autograd keeps a returned gradient without copying it only if nobody else holds that tensor object)"""
    return [(p, g.detach()) for p, g in pairs if p is not None and g is not None]


class PendingSums:
    """What crosses between the filter stage's autograd node (FilterStageFn) and the fused layer stack's node, one object per
    forward: every launch of a captured step costs ~4.5 us whatever its size, so work of the one rides in idle workgroups
    of the other's launches.  Forward: the stack computes s = colsum(gcn.weight) and the coefficient generator's forward.
    Backward: the stage, which runs first, leaves the generator's kernel, dW / db of the C x C linear and its column sums
    (split-K partial buffer -> gradient) to the stack's launches, iff that backward follows in the same pass (stack_armed)
    and nothing can read the gradients before it has run (untouched)."""

    def __init__(self):
        self.stack_armed = False   # the fused layer stack runs its backward in the same pass (set by the encoder), and
        self.stack_done = False    # ... has not yet: its one reduction launch takes what the stage's node leaves
        self.items = []
        self.owners = []
        self._callback_queued = False
        # forward direction: column sums of parameters that a launch of the layer stack carries in trailing workgroups
        # (s = colsum(gcn.weight) of the coefficient generator); whoever needs them first runs them if nobody did
        self.fwd_sums = []
        self.s = None
        # ... and the coefficient generator's kernels themselves: its forward shares the launch of the last layer's
        # feed-forward half (it needs that layer's attention matrix only), its backward kernel the first launch of the
        # stack's backward.  coeff_fwd_req = gcn bias (set by the encoder); coeff_fwd_out = (cj, pooled) once run;
        # coeff_bwd_req = the argument tuple of abi.coeff_bwd, or an _abi.CoeffSavedReq, left by _coeff_backward
        self.coeff_fwd_req = None
        self.coeff_fwd_out = None
        self.coeff_bwd_req = None
        # ... and dW / db of the generator's C x C linear: lin_dw_req = an _abi.LinDwReq (detached tensors only) left by
        # the stage's backward for the first layer's attention backward (fused_stack: the stack's last launch) -
        # or, if that backward has no such launch, for the library at the start of the stack's backward
        self.lin_dw_req = None

    def lin_dw_wanted(self, abi, b, n, heads, r, k, n_out):
        """May the stage's backward leave dW / db of the [n_out, k] linear (r rows) to the stack's backward for b
        graphs of n nodes?  (the stack asks the launch's own predicate again before it carries the request)"""
        mode = lin_dw_role_mode()
        if mode == 0 or not (self.stack_armed and not self.stack_done) or self.lin_dw_req is not None:
            return False
        if not abi.attn_block_bwd_dw_supported(b, n, heads, r, k, n_out):
            return False
        if mode >= 2:
            return True
        return b <= LIN_DW_ROLE_MAX_B and abi.attn_block_bwd_dw_tiles(k, n_out) <= abi.attn_block_bwd_dw_slots(b, n, heads)

    def defer_lin_dw(self, req, owners):
        self.lin_dw_req = req
        self.owners += _owners(*owners)
        self._queue_finish()

    def take_lin_dw(self):
        req, self.lin_dw_req = self.lin_dw_req, None
        return req

    def _queue_finish(self):
        if not self._callback_queued:
            # safety net: whatever no later node took (autograd pruned it from this pass) is run when the backward
            # pass ends
            torch.autograd.Variable._execution_engine.queue_callback(self._finish_pass)
            self._callback_queued = True

    def coeff_dsum_role(self, abi, req, graphs, k_eig):
        """Called by the forward that launches feta_spec_filter_cat_fwd for `graphs` graphs on k_eig eigenvectors, with
        req = (cj, n_real, s, gcn_bias, b, n, h) of the coefficient generator: -> the argument tuple of abi.coeff_dsum (A
        and Bm allocated here: the tanh pass of the generator's backward), or None if the blocks do not fit the slots that
        launch leaves free (a role workgroup walks at most two blocks: the launch is on the forward's chain)."""
        cj, n_real, s, gb, b, n, h = req
        if not abi.spec_cat_fwd_coeff_fits(graphs, n, k_eig, h * b):
            return None
        A = torch.empty((h * b, s.shape[0]), dtype=torch.float32, device=cj.device)
        Bm = torch.empty_like(A)
        return (cj, n_real, s, gb, A, Bm, b, n, h)

    @staticmethod
    def untouched(*params):
        """A gradient may be completed after its node returned only if nothing reads it before the flush: the
        parameter has no .grad to accumulate into (autograd then keeps the returned tensor itself) and no hooks."""
        # AccumulateGrad keeps the returned tensor without copying it only while grad mode is off (an ordinary
        # backward pass): under create_graph=True it accumulates a copy, and anomaly mode reads the buffer when the
        # node returns - both would see the un-reduced buffer
        if torch.is_grad_enabled() or torch.is_anomaly_enabled():
            return False
        for p in params:
            if p is None:
                continue
            if p.grad is not None or p._backward_hooks or getattr(p, '_post_accumulate_grad_hooks', None):
                return False
        return True

    def add(self, partial, out, bcast=None, owners=()):
        """owners: [(parameter, the gradient tensor its node returns)] whose storage this sum completes later: checked
        when the backward pass ends (_finish_pass) - had autograd copied the returned tensor after all (a hook on the
        AccumulateGrad node, which untouched() cannot see), the finished values are copied over that copy."""
        # (a second tensor object on the same storage: autograd keeps a returned gradient without copying it only
        # if nobody else holds a reference to that tensor object)
        self.items.append((partial, out.detach(), None if bcast is None else bcast.detach()))
        self.owners += _owners(*owners)
        self._queue_finish()

    def take(self):
        items, self.items = self.items, []
        return items

    def take_fwd(self):
        sums, self.fwd_sums = self.fwd_sums, []
        return sums

    def coeff_fwd_role(self, attn, n_real):
        """Called by the layer stack for the launch that follows the last attention: -> the argument tuple of the
        coefficient generator's forward (outputs allocated here), or None if nobody asked / s is not ready."""
        if self.coeff_fwd_req is None or self.s is None or self.fwd_sums or attn is None:
            return None
        if attn.shape[-1] > 64:      # (beyond the role's LDS tile budget the stand-alone launch is the faster form:
            return None              # csrc/feta_coeff.h - one 1024-thread workgroup per block, staged rows)
        if attn.shape[0] * attn.shape[1] > COEFF_ROLE_MAX_BLOCKS:
            return None
        gcn_bias, self.coeff_fwd_req = self.coeff_fwd_req, None
        b, h, n, _ = attn.shape
        cj = torch.empty((h * b, n), dtype=torch.float32, device=attn.device)
        pooled = torch.empty((h * b, self.s.shape[0]), dtype=torch.float32, device=attn.device)
        self.coeff_fwd_out = (cj, pooled)
        return (attn, n_real, self.s, gcn_bias.detach().contiguous(), cj, pooled)

    def take_coeff_bwd(self):
        req, self.coeff_bwd_req = self.coeff_bwd_req, None
        return req

    def _finish_pass(self):
        self._callback_queued = False
        dw_req = self.take_lin_dw()
        if dw_req is not None:      # (nobody took it: the stack's node was pruned from this pass)
            dw_req.run(*_lib.backend(dw_req.dy))
        req = self.take_coeff_bwd()
        items = self.take()
        if items:
            abi, stream = _lib.backend(items[0][0])
            if isinstance(req, CoeffSavedReq):
                req.run(abi, stream)
            elif req is not None:
                cj, n_real, s, gb, dpooled, partial, b, n, h = req
                abi.coeff_bwd(cj, n_real, s, gb, dpooled, partial, None, None, b, n, h, stream)
            abi.colsum_multi(items, stream)
        owners, self.owners = self.owners, []
        for p, g in owners:
            # .grad is None: torch.autograd.grad() handed the tensor itself to the caller - nothing to repair
            if p.grad is not None and p.grad.data_ptr() != g.data_ptr():
                with torch.no_grad():
                    p.grad.copy_(g.view_as(p.grad))


# linear_cat folded into the launches of the eigenbasis filter (FilterStageFn): forward feta_spec_filter_cat_fwd (ABI 10),
# backward feta_spec_filter_cat_bwd (ABI 11).  FETA_CAT_FOLD=0 / FETA_CAT_FOLD_BWD=0: off (A/B timing).
USE_CAT_FOLD = _os.environ.get('FETA_CAT_FOLD', '1') != '0'
USE_CAT_FOLD_BWD = _os.environ.get('FETA_CAT_FOLD_BWD', '1') != '0'


def _lin_forward(abi, stream, pooled, lin_w, lin_b, gemm_bf16):
    """coeff = pooled W_lin^T + b_lin under the one GEMM policy -> (coeff fp32, how, lp): how = 'own' (csrc/lin.hip: one
    16 x 16 tile per wave straight from L2 - where the products are launch-bound), 'lib16' (library bf16 GEMMs on the bf16
    copies lp = (pooled, W), which the backward reuses) or 'lib' (the library's fp32 GEMM - where they are compute-bound: C
    = 1024 at the BASELINE shape is 1 GFLOP each, ~12 us at half the fp32 matrix peak; lin.hip is L2-bound there, 31 us)."""
    r_, k_, n_ = pooled.shape[0], pooled.shape[1], lin_w.shape[0]
    if gemm_bf16 and r_ >= LIN_LIB_BF16_MIN_ROWS and pooled.is_cuda:
        p16, w16 = pooled.to(torch.bfloat16), lin_w.to(torch.bfloat16)
        coeff = torch.mm(p16, w16.t(), out_dtype=torch.float32)
        if lin_b is not None:
            coeff += lin_b
        return coeff, 'lib16', (p16, w16)
    if abi.lin_supported(r_, k_, n_) and (r_ * k_ * n_ <= LIN_OWN_GEMM_MAX_MACS or gemm_bf16):
        coeff = torch.empty((r_, n_), dtype=torch.float32, device=pooled.device)
        abi.lin_fwd(pooled, lin_w, lin_b, coeff, stream, bf16=gemm_bf16)
        return coeff, 'own', None
    with _lib.tuned_gemm():
        return torch.addmm(lin_b, pooled, lin_w.t()), 'lib', None


def _lin_backward(abi, stream, how, gemm_bf16, pooled, lin_w, lp, dcoeff, db_lin, sums, need_dpooled, pass_on=False,
                  dw_role=None):
    """Backward of _lin_forward -> (dpooled, dW_lin, column sums still to run); db_lin is written (or requested).
    sums: [(in, out)] column sums the steps before left.  'own': dpooled, dW_lin, db_lin and every sum in ONE launch.
    Library: dw_role(dcoeff, db_lin) may leave dW_lin / db_lin to a later launch (-> dW_lin, or None) - only the dX product
    runs here then; the sums, db_lin among them, run here in one launch unless pass_on hands them to the caller."""
    if how == 'own':
        dpooled = torch.empty_like(pooled) if need_dpooled else None
        dw_lin = torch.empty_like(lin_w)
        abi.lin_bwd(pooled, lin_w, dcoeff, dpooled, dw_lin, db_lin, stream, pairs=sums, bf16=gemm_bf16)
        return dpooled, dw_lin, []
    dw_lin = dw_role(dcoeff, db_lin) if (dw_role is not None and how == 'lib') else None
    left_dw = dw_lin is not None
    if not left_dw:
        sums = sums + [(dcoeff, db_lin)]
    if sums and not pass_on:
        abi.colsum_multi(sums, stream)
        sums = []
    if how == 'lib16':
        p16, w16 = lp
        d16 = dcoeff.to(torch.bfloat16)
        dpooled = torch.mm(d16, w16, out_dtype=torch.float32)
        dw_lin = torch.mm(d16.t(), p16, out_dtype=torch.float32)
    else:
        with _lib.tuned_gemm():
            dpooled = dcoeff.mm(lin_w)
            if not left_dw:
                dw_lin = dcoeff.t().mm(pooled)
    return dpooled, dw_lin, sums


def _filter_step_backward(abi, stream, xs, g0, g1, coeff, n_real, dys, dcoeff_ext, mode, order, share, batch_first,
                          cat=None, y=None):
    """The filter's backward as a step in front of _lin_backward -> (dx, dcoeff fp32, dbias, db_lin, [(in, out)] column
    sums to run): the filter-bias partials and dcoeff (= the gradient of b_lin) become available together, so ONE reduction
    launch takes both.  dcoeff_ext: the gradient of a regulariser on the coefficients (transformer/models.py:554-584); dys
    None (and no cat): only the coefficients were used downstream."""
    if dys is None and cat is None:
        dcoeff = dcoeff_ext.contiguous()
        return None, dcoeff, None, torch.empty(dcoeff.shape[1], dtype=torch.float32, device=xs.device), []
    dx, dcoeff, dbp = _filter_backward(abi, stream, xs, g0, g1, coeff, n_real, dys, mode, order, share, batch_first, cat, y)
    if dcoeff.dtype != torch.float32:
        dcoeff = dcoeff.float()      # the C x C linear's gradients accumulate in fp32
    if dcoeff_ext is not None:
        dcoeff += dcoeff_ext
    dh = xs.shape[3]
    both = torch.empty(dh + dcoeff.shape[1], dtype=torch.float32, device=xs.device)
    return dx, dcoeff, both[:dh], both[dh:], [(dbp, both[:dh])]


class FilterFromPooledFn(torch.autograd.Function):
    """``self.linear`` of the coefficient generator (transformer/models.py:284) and the dynamic filter
    (transformer/models.py:346-360, transformer/ChebNetDynamic.py:132-189) as ONE autograd node:
    coeff = pooled W_lin^T + b_lin, y = filter(x; coeff).  -> (y, coeff [H*B, C]).  The path of every filter stage that
    is not the one stage of its forward (FilterStageFn): last_layer_filter=False, the op-by-op bf16 path."""

    @staticmethod
    def forward(ctx, x, pooled, lin_w, lin_b, bias, n_real, g0, g1, mode, order, share, batch_first, gemm_bf16=False):
        abi, stream = _lib.backend(x, pooled)
        xs = _dense_like(x, batch_first)
        pooled, lin_w = pooled.contiguous(), lin_w.contiguous()      # fp32 master precision (also what a regulariser sees)
        coeff, how, ctx.lp = _lin_forward(abi, stream, pooled, lin_w, lin_b, bool(gemm_bf16))
        # bf16 storage path: the per-block weights the filter kernel reads are bf16 copies of them
        cw = coeff if x.dtype == torch.float32 else coeff.to(x.dtype)
        y = _filter_forward(abi, stream, xs, g0, g1, cw, bias, n_real, mode, order, share, batch_first)
        ctx.save_for_backward(xs, cw, pooled, lin_w, n_real, g0, g1)
        ctx.cfg = (mode, order, share, batch_first, bias is not None, how, bool(gemm_bf16))
        ctx.set_materialize_grads(False)
        return y, coeff

    @staticmethod
    def backward(ctx, dy, dcoeff_ext):
        xs, coeff, pooled, lin_w, n_real, g0, g1 = ctx.saved_tensors
        mode, order, share, batch_first, has_bias, how, gemm_bf16 = ctx.cfg
        abi, stream = _lib.backend(xs)
        dys = None if dy is None else _dense_like(dy.to(xs.dtype), batch_first)
        dx, dcoeff, dbias, db_lin, sums = _filter_step_backward(abi, stream, xs, g0, g1, coeff, n_real, dys, dcoeff_ext,
                                                                mode, order, share, batch_first)
        dpooled, dw_lin, _ = _lin_backward(abi, stream, how, gemm_bf16, pooled, lin_w, ctx.lp, dcoeff, db_lin, sums,
                                           ctx.needs_input_grad[1])
        return (dx, dpooled, dw_lin, db_lin, dbias if has_bias else None) + (None,) * 8


def filter_from_pooled(x, pooled, lin_w, lin_b, bias, n_real, graph, mode, order, heads_share_graph=False,
                       batch_first=False, gemm_bf16=False):
    """x [B,N,H,dh] view, pooled [H*B, C] -> (y, coeff [H*B, C]); graph = (lhat,) | (u, lam)."""
    g0, g1 = _graph_operands(graph, mode, x.dtype)
    return FilterFromPooledFn.apply(x, pooled, lin_w, lin_b, bias, n_real, g0, g1, mode, order,
                                    bool(heads_share_graph), batch_first, bool(gemm_bf16))


def _graph_operands(graph, mode, dtype):
    g0 = graph[0].contiguous()
    g1 = graph[1].contiguous() if len(graph) > 1 else None
    if dtype != torch.float32:
        if mode != 'spec':
            raise NotImplementedError("the bf16 storage path runs the eigenbasis filter (filter_mode='spectral')")
        g0 = g0.to(dtype)      # U travels as bf16; lambda and t_k(lambda) stay fp32
    return g0, g1


class RowLinearFn(torch.autograd.Function):
    """y = relu?(x W^T + b) * rowscale? + residual?  on [M, KI] rows, plus (optionally) the
    per-block partial BatchNorm statistics of y.  C ABI: feta_rowlin_fwd / feta_rowlin_bwd."""

    @staticmethod
    def forward(ctx, x, w, bias, rowscale, residual, relu, want_stats, stats_shift=None):
        abi, stream = _lib.backend(x, w)
        ctx.set_materialize_grads(False)   # no zero tensor for the non-differentiable stats output
        assert not (relu and residual is not None), 'relu mask is taken from the saved output'
        x = x.contiguous()
        w = w.contiguous()
        m, no = x.shape[0], w.shape[0]
        y = torch.empty((m, no), dtype=torch.float32, device=x.device)
        stats = None
        if want_stats:
            # shifted partial sums + the shift row (csrc/feta_rowops.h): relative to the consumer BatchNorm's running mean
            stats = torch.empty((abi.rowlin_blocks(m) + 1, 2, no), dtype=torch.float32, device=x.device)
        res = None if residual is None else residual.contiguous()
        if want_stats and stats_shift is not None:
            d = abi.rowlin_ex(m, x.shape[1], no, relu=relu, x=x, w=w, bias=bias, rowscale=rowscale, residual=res, y=y,
                              stats=stats, stats_shift=stats_shift)
            abi.rowlin_fwd_ex(d, stream)
        else:
            abi.rowlin_fwd(x, w, bias, rowscale, res, y, stats, relu, stream)
        ctx.save_for_backward(x, w, rowscale, y if relu else None)
        ctx.cfg = (bias is not None, residual is not None)
        if stats is not None:
            ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    def backward(ctx, dy, _dstats):
        x, w, rowscale, ysaved = ctx.saved_tensors
        if dy is None:
            return (None,) * 8
        has_bias, has_res = ctx.cfg
        abi, stream = _lib.backend(x)
        m, ki = x.shape
        no = w.shape[0]
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        partial = torch.empty((abi.rowlin_chunks(m), no * ki + no), dtype=torch.float32, device=x.device)
        dwdb = torch.empty(no * ki + no, dtype=torch.float32, device=x.device)
        abi.rowlin_bwd(x, w, dy, rowscale, ysaved, dx, partial, dwdb, stream)
        dw = dwdb[:no * ki].view(no, ki)
        db = dwdb[no * ki:] if has_bias else None
        return dx, dw, db, None, (dy if has_res else None), None, None, None


def _cat_forward(abi, stream, x1, x2, w, bias, tail=None):
    """y = [x1 | x2] W^T + b on [M, .] rows without materialising the concatenation (linear_cat, transformer/models.py:
    223-224).  tail (fused_stack.StackTail): x1 is the pre-norm y2 of the fused BatchNorm stack - the launch finalizes the
    statistics the stack left there (publishing tail.prm2) and normalises inside the operand loads."""
    m, k1 = x1.shape
    ki, no = k1 + x2.shape[1], w.shape[0]
    y = torch.empty((m, no), dtype=torch.float32, device=x1.device)
    d = abi.rowlin_ex(m, ki, no, x=x1, x2=x2, x_split=k1, w=w, bias=bias, y=y, **_tail_kw(tail, 'x_stats', 'x_'))
    abi.rowlin_fwd_ex(d, stream)
    return y


def _tail_kw(tail, stats, pre):
    """the arguments with which a launch finalizes the BatchNorm a StackTail describes, under that launch's names"""
    if tail is None:
        return {}
    nm = tail.norm
    return {stats: tail.st2, 'Gx': tail.G2, pre + 'gamma': tail.gamma, pre + 'beta': tail.beta, pre + 'bn_out': tail.prm2,
            pre + 'rmean': nm.running_mean, pre + 'rvar': nm.running_var, pre + 'nbt': nm.num_batches_tracked,
            'momentum': float(nm.momentum), 'eps': float(nm.eps)}


def _cat_backward(abi, stream, x1, x2, w, dy, prm2=None, reduce=True):
    """Backward of _cat_forward -> (dx1, dx2, dwdb = [dW | db] flat, split-K partial rows, gs).  prm2 (the BatchNorm
    parameter block of a StackTail): dx1 is the gradient w.r.t. the NORMALISED x1 and gs holds the partial sums its
    BatchNorm backward needs.  reduce=False: the launch leaves the partial rows for the caller's next reduction launch."""
    m, k1 = x1.shape
    ki, no = k1 + x2.shape[1], w.shape[0]
    dx1, dx2 = torch.empty_like(x1), torch.empty_like(x2)
    partial = torch.empty((abi.rowlin_chunks(m), no * ki + no), dtype=torch.float32, device=x1.device)
    dwdb = torch.empty(no * ki + no, dtype=torch.float32, device=x1.device)
    gs, kw = None, {}
    if prm2 is not None:
        gs = torch.empty((abi.rowlin_blocks(m), 2, k1), dtype=torch.float32, device=x1.device)
        kw = dict(x_bn=prm2, sum_y=x1, sum_bn=prm2, sum_out=gs)
    d = abi.rowlin_ex(m, ki, no, x=x1, x2=x2, x_split=k1, w=w, dy=dy, dx=dx1, dx2=dx2, partial=partial,
                      partial_ld=(0 if reduce else no * ki + no), **kw)
    abi.rowlin_bwd_ex(d, dwdb if reduce else None, stream)
    return dx1, dx2, dwdb, partial, gs


def _cat_grads(dwdb, w, has_bias):
    no, ki = w.shape
    return dwdb[:no * ki].view(no, ki), (dwdb[no * ki:] if has_bias else None)


class RowLinearCatFn(torch.autograd.Function):
    """linear_cat as a node of its own (_cat_forward / _cat_backward).  With tail, the StackTail contract: backward
    returns, for x1, the gradient w.r.t. the normalised tensor and leaves the BatchNorm backward partial sums in tail.gs."""

    @staticmethod
    def forward(ctx, x1, x2, w, bias, tail=None):
        abi, stream = _lib.backend(x1, x2, w)
        x1, x2, w = x1.contiguous(), x2.contiguous(), w.contiguous()
        y = _cat_forward(abi, stream, x1, x2, w, bias, tail)
        ctx.save_for_backward(x1, x2, w, None if tail is None else tail.prm2)
        ctx.tail, ctx.has_bias = tail, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x1, x2, w, prm2 = ctx.saved_tensors
        abi, stream = _lib.backend(x1)
        dx1, dx2, dwdb, _, gs = _cat_backward(abi, stream, x1, x2, w, dy.contiguous(), prm2)
        if ctx.tail is not None:
            ctx.tail.gs = gs
        return (dx1, dx2) + _cat_grads(dwdb, w, ctx.has_bias) + (None,)


class FilterStageFn(torch.autograd.Function):
    """The ONE filter stage of a forward as one autograd node: coefficient generator -> C x C linear -> dynamic filter ->
    linear_cat, each step the function the plain ops run.  (y2 [N,B,d] stack output - with tail the pre-norm rows -, x
    [B,N,H,dh] per-head rows, the seven parameters | attn, n_real, graph operands, tail, pending, cfg) -> (out [N,B,.],
    coeff [H*B, C]).  cfg = (mode, order, share, gemm_bf16, cat, grad mode): cat None - the node ends at the filter (out = the
    filtered rows, y2 unused); 'rows' - linear_cat inside; 'fold' - and riding in the filter's launches where they take it.
    Backward runs linear_cat, the filter, the linear and the generator in program order; a column sum that a later step's
    launch carries travels in a local list, and what the stack's launches carry leaves through pending (PendingSums)."""

    @staticmethod
    def forward(ctx, y2, x, gcn_w, gcn_b, lin_w, lin_b, bias, cat_w, cat_b, attn, n_real, g0, g1, tail, pending, cfg):
        mode, order, share, gemm_bf16, cat, grad_mode = cfg
        abi, stream = _lib.backend(x, attn)
        ctx.set_materialize_grads(False)
        need = [grad_mode and g for g in ctx.needs_input_grad]     # (set for a parameter also where no graph is recorded)
        coeff_live = need[2] or need[3]                                    # the generator's backward will have work
        filt_live = coeff_live or need[1] or need[4] or need[5] or need[6]     # ... the filter's and the linear's
        b, n, h, dh = x.shape
        d = h * dh
        tok = lambda t: t.view(n, b, h, dh).permute(1, 0, 2, 3)     # [N*B, d] rows -> token view
        rows = lambda t: t.permute(1, 0, 2, 3).reshape(n * b, d)    # ... and back (a view)
        pooled, cj, s, gb = _coeff_forward(abi, stream, attn, n_real, gcn_w, gcn_b, pending)
        xs = _dense_like(x, False)
        lw = lin_w.contiguous()
        coeff, how, ctx.lp = _lin_forward(abi, stream, pooled, lw, lin_b, gemm_bf16)
        y2r = cw = A = Bm = dsum = None
        if cat is not None:
            y2r, cw = y2.reshape(n * b, d).contiguous(), cat_w.contiguous()
        fold = (cat == 'fold' and USE_CAT_FOLD and mode == 'spec' and cat_w.shape == (d, 2 * d)
                and bool(abi.spec_cat_supported(n, h, dh, order, g0.shape[2], share)))
        if fold:
            if USE_COEFF_DSUM and coeff_live and n <= 64 and h == 4 and h * b <= COEFF_ROLE_MAX_BLOCKS:
                # the generator's backward will run: this launch, which leaves most of the chip idle, may compute the tanh
                # part of it (A, Bm: feta_coeff_dsum).  4 heads only: feta_spec_filter_cat_fwd_coeff has no 8-head form
                dsum = pending.coeff_dsum_role(abi, (cj, n_real, s, gb, b, n, h), b, g0.shape[2])
                if dsum is not None:
                    A, Bm = dsum[4], dsum[5]
            out = _new_token(b, n, h, dh, False, x)
            y = _filter_forward(abi, stream, xs, g0, g1, coeff, bias, n_real, mode, order, share, False,
                                cat=dict(y2=tok(y2r), w_cat=cw, b_cat=cat_b, out=out, dsum=dsum,
                                         **_tail_kw(tail, 'y2_stats', '')))
            out = rows(out)
        else:
            y = _filter_forward(abi, stream, xs, g0, g1, coeff, bias, n_real, mode, order, share, False)
            out = rows(y) if cat is None else _cat_forward(abi, stream, y2r, rows(y), cw, cat_b, tail)
        ctx.save_for_backward(xs, coeff, pooled, lw, n_real, g0, g1, cj, s, gb, y2r, cw, None if tail is None else tail.prm2,
                              y if cat is not None else None, A, Bm)
        fold_bwd = fold and bool(abi.spec_cat_bwd_supported(n, h, dh, order, g0.shape[2], share))
        ctx.cfg = (mode, order, share, gemm_bf16, cat, how, fold_bwd, coeff_live, filt_live)
        ctx.dims = (b, n, h, gcn_w.shape[0])
        ctx.params = (gcn_w, gcn_b, lin_w, lin_b, bias, cat_w, cat_b)     # (the parameters themselves: untouched())
        ctx.tail, ctx.pending = tail, pending
        return out.view(n, b, -1), coeff

    @staticmethod
    def backward(ctx, dout, dcoeff_ext):
        if dout is None and dcoeff_ext is None:
            return (None,) * 16
        xs, coeff, pooled, lw, n_real, g0, g1, cj, s, gb, y2r, cw, prm2, y, A, Bm = ctx.saved_tensors
        mode, order, share, gemm_bf16, cat, how, fold_bwd, coeff_live, filt_live = ctx.cfg
        gcn_w, gcn_b, lin_w, lin_b, bias, cat_w, cat_b = ctx.params
        pend, need = ctx.pending, ctx.needs_input_grad
        abi, stream = _lib.backend(xs)
        b, n, h, dh = xs.shape
        tok = lambda t: t.view(n, b, h, dh).permute(1, 0, 2, 3)
        sums, owners = [], []     # column sums that a later launch of this backward carries, and the gradients they complete
        dy2 = dx = dgw = dgb = dlw = dlb = dfb = dcw = dcb = dys = fold = dpooled = None
        # -- linear_cat, or its fold into the filter's launch
        if dout is not None and cat is None:
            dys = tok(dout.to(xs.dtype).contiguous())
        elif dout is not None:
            dyr = dout.reshape(n * b, -1).contiguous()
            # (the same launches as while linear_cat was a node of its own, whose gradients somebody could read before the
            # filter's launch had reduced them: its partial rows ride along only where that held)
            ride = filt_live and PendingSums.untouched(cat_w, cat_b)
            if fold_bwd and ride and USE_CAT_FOLD_BWD:
                # nothing is launched here: the filter's launch starts from dout and writes dy2, gs and the partial rows
                no, ki = cw.shape
                nb = abi.spec_cat_bwd_rows(b)
                dy2 = torch.empty_like(y2r)
                partial = torch.empty((nb, no * ki + no), dtype=torch.float32, device=xs.device)
                dwdb = torch.empty(no * ki + no, dtype=torch.float32, device=xs.device)
                gs = torch.empty((nb, 2, y2r.shape[1]), dtype=torch.float32, device=xs.device) if prm2 is not None else None
                fold = dict(dout=tok(dyr), y2=tok(y2r), w_cat=cw, dxn=tok(dy2), partial=partial, y2_bn=prm2, gs=gs)
            else:
                dy2, dx2, dwdb, partial, gs = _cat_backward(abi, stream, y2r, y.permute(1, 0, 2, 3).reshape(n * b, h * dh),
                                                            cw, dyr, prm2, reduce=not ride)
                dys = tok(dx2)
            dcw, dcb = _cat_grads(dwdb, cw, cat_b is not None)
            if ride:
                sums.append((partial, dwdb))
                owners += _owners((cat_w, dcw), (cat_b, dcb))
            if ctx.tail is not None:
                ctx.tail.gs = gs      # (StackTail contract: the stack's node runs behind this one)
        # -- the filter and the C x C linear
        if filt_live:
            dx, dcoeff, dfb, dlb, own = _filter_step_backward(abi, stream, xs, g0, g1, coeff, n_real, dys, dcoeff_ext, mode,
                                                              order, share, False, fold, y)

            def dw_role(dcoeff, db_lin):
                # dW_lin and db_lin as a role of the stack's last launch (PendingSums.lin_dw_req)
                if not (need[4] and need[5]
                        and pend.lin_dw_wanted(abi, b, n, h, dcoeff.shape[0], pooled.shape[1], dcoeff.shape[1])
                        and PendingSums.untouched(lin_w, lin_b)):
                    return None
                dw_lin = torch.empty_like(lw)
                pend.defer_lin_dw(LinDwReq(dcoeff, pooled, dw_lin, db_lin), [(lin_w, dw_lin), (lin_b, db_lin)])
                return dw_lin
            # (library GEMMs: the sums wait for the generator's reduction launch - where they did as a node's, see above)
            pass_on = coeff_live and how != 'own' and PendingSums.untouched(lin_b, bias)
            dpooled, dlw, sums = _lin_backward(abi, stream, how, gemm_bf16, pooled, lw, ctx.lp, dcoeff, dlb, own + sums,
                                               coeff_live, pass_on, dw_role)
            if sums:
                owners += _owners((lin_b, dlb), (bias, dfb))
        # -- the coefficient generator: its reduction launch, or the stack's, takes what is left
        if coeff_live and dpooled is not None:
            dgw, dgb = _coeff_backward(abi, stream, cj, n_real, s, gb, ctx.dims, dpooled, None if A is None else (A, Bm),
                                       pend, (gcn_w, gcn_b), sums, owners)
        return (None if dy2 is None else dy2.view(n, b, -1), dx, dgw, dgb, dlw, dlb, None if bias is None else dfb, dcw,
                dcb) + (None,) * 7


def filter_stage(y2, x, gcn_w, gcn_b, lin_w, lin_b, bias, cat_w, cat_b, attn, n_real, graph, mode, order,
                 heads_share_graph=False, gemm_bf16=False, cat='fold', tail=None, pending=None):
    """-> (out [N,B,.], coeff [H*B, C]) of FilterStageFn; graph = (lhat,) | (u, lam); pending: the layer stack's PendingSums"""
    g0, g1 = _graph_operands(graph, mode, x.dtype)
    return FilterStageFn.apply(y2, x, gcn_w, gcn_b, lin_w, lin_b, bias, cat_w, cat_b, attn, n_real, g0, g1, tail,
                               PendingSums() if pending is None else pending,
                               (mode, order, bool(heads_share_graph), bool(gemm_bf16), cat, torch.is_grad_enabled()))


class BatchNormTrainFn(torch.autograd.Function):
    """Training-mode BatchNorm1d over the rows of y [M, D] from per-block partial statistics.
    C ABI: feta_bn_stats (when the producer did not emit them), feta_bn_apply_fwd, feta_bn_bwd."""

    @staticmethod
    def forward(ctx, y, stats, gamma, beta, running_mean, running_var, momentum, eps, nbt=None):
        abi, stream = _lib.backend(y)
        y = y.contiguous()
        m, d = y.shape
        if stats is None:
            stats = torch.empty((abi.rowlin_blocks(m) + 1, 2, d), dtype=torch.float32, device=y.device)
            abi.bn_stats(y, stats, stream, shift=running_mean)
        out = torch.empty_like(y)
        mean_rstd = torch.empty((2, d), dtype=torch.float32, device=y.device)
        abi.bn_apply_fwd(y, stats, gamma, beta, out, mean_rstd, running_mean, running_var,
                         float(momentum), float(eps), stream, nbt=nbt)
        ctx.save_for_backward(y, mean_rstd, gamma)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, mean_rstd, gamma = ctx.saved_tensors
        abi, stream = _lib.backend(y)
        m, d = y.shape
        dout = dout.contiguous()
        partial = torch.empty((abi.rowlin_blocks(m), 2, d), dtype=torch.float32, device=y.device)
        dy = torch.empty_like(y)
        dgamma = torch.empty(d, dtype=torch.float32, device=y.device)
        dbeta = torch.empty(d, dtype=torch.float32, device=y.device)
        abi.bn_bwd(y, dout, mean_rstd, gamma, partial, dy, dgamma, dbeta, stream)
        return dy, None, dgamma, dbeta, None, None, None, None, None


ROWLIN_DIMS = (16, 32, 64, 128, 192, 256)


def row_linear_supported(ki, no, need_backward=True):
    return ki in ROWLIN_DIMS and (no in ROWLIN_DIMS if need_backward else no % 16 == 0)


def row_linear(x, w, bias=None, rowscale=None, residual=None, relu=False, want_stats=False, stats_shift=None):
    """x [M, KI] -> (y [M, NO], stats [G + 1, 2, NO] or None).  stats_shift [NO]: the running mean of the BatchNorm that
    will consume the statistics - they are sums of (y - shift) (csrc/feta_rowops.h)."""
    return RowLinearFn.apply(x, w, bias, rowscale, residual, relu, want_stats, stats_shift)


def row_linear_cat(x1, x2, w, bias=None, tail=None):
    """[x1 | x2] W^T + b on [M, .] rows; needs x1.shape[1] % 16 == 0 and supported total dims.  tail: [BN(x1) | x2], where
    BN is the last BatchNorm of the fused layer stack, never materialised (row_linear_cat_bn(y2, x2, w, bias, tail))."""
    return RowLinearCatFn.apply(x1, x2, w, bias, tail)


row_linear_cat_bn = row_linear_cat


def batch_norm_train(y, stats, gamma, beta, running_mean, running_var, momentum, eps, num_batches_tracked=None):
    return BatchNormTrainFn.apply(y, stats, gamma, beta, running_mean, running_var, momentum, eps,
                                  num_batches_tracked)


class LayerNormRowsFn(torch.autograd.Function):
    """nn.LayerNorm over the last dimension of [M, D] rows (feta_layernorm_fwd/bwd): norm1 / norm2 of
    the encoder layer when batch_norm=False."""

    @staticmethod
    def forward(ctx, y, gamma, beta, eps):
        abi, stream = _lib.backend(y, gamma)
        y = y.contiguous()
        m, d = y.shape
        out = torch.empty_like(y)
        stats = torch.empty((m, 2), dtype=torch.float32, device=y.device)
        abi.layernorm_fwd(y, gamma.contiguous(), beta.contiguous(), float(eps), out, stats, stream)
        ctx.save_for_backward(y, stats, gamma)
        return out

    @staticmethod
    def backward(ctx, dout):
        y, stats, gamma = ctx.saved_tensors
        abi, stream = _lib.backend(dout)
        m, d = y.shape
        dy = torch.empty_like(y)
        partial = torch.empty((abi.layernorm_blocks(m), 2, d), dtype=torch.float32, device=y.device)
        dgdb = torch.empty((2, d), dtype=torch.float32, device=y.device)
        abi.layernorm_bwd(dout.contiguous(), y, stats, gamma.contiguous(), dy, partial, dgdb, stream)
        return dy, dgdb[0], dgdb[1], None


def layer_norm_rows_supported(d):
    return d % 4 == 0 and 4 <= d <= 256


def layer_norm_rows(y, gamma, beta, eps):
    return LayerNormRowsFn.apply(y, gamma, beta, eps)


class DropoutState:
    """(seed, offset) of the attention-probability dropout masks: every masked forward takes the next offset, so
    masks differ between layers and steps and are reproducible from the seed (the kernels derive the mask from
    (seed, offset, b, h, query, key): include/feta_hip.h, feta_attn_fwd_drop).

    Host mode (default): (seed, offset) are Python ints handed to the kernels as arguments.
    Device mode (begin_device_mode; used by train.GraphedTrainStep): the key lives in an int64[2] DEVICE tensor which
    the kernels read when they RUN (feta_attn_*_drop_dev); call k of a step uses offset state[1] + k and the step
    itself advances state[1] by its number of masked calls (end_step, a captured in-place add) - a hipGraph replay
    therefore draws the masks the eager loop would have drawn at that step."""
    seed = None
    offset = 0
    _dev = None      # int64 [seed, offset] on the device of the captured steps (device mode), else None
    _keys = {}       # device -> THE key tensor of that device.  Captured graphs hold its raw address (the kernels read
    #                  it at run time, the captured end_step add writes it), so it is created once per device and never
    #                  replaced or freed: a second GraphedTrainStep (one per padded-size bucket) shares it - and with it
    #                  ONE offset stream, so buckets never replay each other's (seed, offset) pairs
    _calls = 0       # masked calls so far in the current step (device mode)

    @classmethod
    def manual_seed(cls, seed):
        cls.seed, cls.offset = int(seed) & (2 ** 63 - 1), 0
        cls._sync_device()

    @classmethod
    def _sync_device(cls):
        """host (seed, offset) -> every key tensor that exists (graphs captured on any device follow a re-seed)"""
        for key in cls._keys.values():
            key.copy_(torch.tensor([cls.seed, cls.offset], dtype=torch.int64))
        cls._calls = 0

    @classmethod
    def device_mode(cls):
        return cls._dev is not None

    @classmethod
    def begin_device_mode(cls, device):
        if cls.seed is None:
            cls.manual_seed(torch.initial_seed())
        device = torch.device(device)
        if device.type == 'cuda' and device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        key = cls._keys.get(device)
        if key is None:
            key = cls._keys[device] = torch.zeros(2, dtype=torch.int64, device=device)
        key.copy_(torch.tensor([cls.seed, cls.offset], dtype=torch.int64))
        cls._dev = key
        cls._calls = 0

    @classmethod
    def end_device_mode(cls):
        """Back to host-held keys.  The key tensors stay alive (graphs captured in device mode may still be replayed:
        they keep reading and advancing their device's key)."""
        cls._dev = None
        cls._calls = 0

    @classmethod
    def next(cls):
        """-> (seed, offset) as ints, or (state tensor, offset_add) in device mode"""
        if cls._dev is not None:
            cls._calls += 1
            return cls._dev, cls._calls
        if cls.seed is None:
            cls.manual_seed(torch.initial_seed())
        cls.offset += 1
        return cls.seed, cls.offset

    @classmethod
    def end_step(cls):
        """Device mode: advance the device offset by the masked calls of this step (an in-place add on the current
        stream: part of the captured step); the host mirror follows.  -> number of calls"""
        n, cls._calls = cls._calls, 0
        if cls._dev is not None and n:
            cls._dev[1:2].add_(n)
            cls.offset += n
        return n

    @classmethod
    def replayed(cls, n):
        """A captured step that made n masked calls was replayed: the host mirror follows the device offset."""
        cls.offset += n

    @classmethod
    def snapshot(cls):
        return cls.seed, cls.offset

    @classmethod
    def restore(cls, snap):
        cls.seed, cls.offset = snap
        if cls.seed is not None:
            cls._sync_device()


def attention_core(qkv, pe, n_real, num_heads, need_attn=True, tie_qk=False, batch_first=False, dropout_p=0.0,
                   stab='rowmax'):
    """dropout_p > 0: attention-probability dropout with a mask regenerated in backward (no mask tensor).  The key
    (seed, offset) is a pair of host values, or - DropoutState in device mode - a device tensor the kernels read when
    they run, which is what makes the op capturable."""
    drop = None
    if dropout_p > 0.0:
        if qkv.is_cuda and torch.cuda.is_current_stream_capturing() and not DropoutState.device_mode():
            raise RuntimeError('attention dropout inside a captured hipGraph would replay one fixed mask: capture with '
                               'the key on the device (functional.DropoutState.begin_device_mode; '
                               'train.GraphedTrainStep does)')
        drop = (float(dropout_p),) + DropoutState.next()
    if stab not in ('rowmax', 'clamp5'):
        raise ValueError("stab must be 'rowmax' or 'clamp5'")
    if stab == 'clamp5' and drop is not None:
        raise NotImplementedError('stab=clamp5 with attention dropout')
    return AttentionCoreFn.apply(qkv, pe, n_real, num_heads, need_attn, tie_qk, batch_first, drop, stab == 'clamp5')


def filter_coefficients(attn, n_real, gcn_weight, gcn_bias):
    return FilterCoefficientsFn.apply(attn, n_real, gcn_weight, gcn_bias)


def cheb_filter(x, lhat, coeff, bias, n_real, order, heads_share_graph=False, batch_first=False):
    return _FilterFn.apply(x, coeff, bias, n_real, lhat.contiguous(), None, 'cheb', order,
                           bool(heads_share_graph), batch_first)


def spec_filter(x, u, lam, coeff, bias, n_real, order, heads_share_graph=False, batch_first=False):
    return _FilterFn.apply(x, coeff, bias, n_real, u.contiguous(), lam.contiguous(), 'spec', order,
                           bool(heads_share_graph), batch_first)


def lhat_from_edges(edge_index, node_graph, node_off, num_graphs, n_pad):
    """Dense scaled Laplacian [B,N,N] of every graph of the batch (feta_lhat_from_edges)."""
    abi, stream = _lib.backend(edge_index, node_graph)
    dev = node_graph.device
    lhat = torch.zeros((num_graphs, n_pad, n_pad), dtype=torch.float32, device=dev)
    deg = torch.zeros(node_graph.shape[0], dtype=torch.float32, device=dev)
    abi.lhat_from_edges(edge_index.contiguous(), node_graph.contiguous(), node_off.contiguous(),
                        deg, lhat, stream)
    return lhat


def eigh_sym(a, n_real, shift, k=None, max_sweeps=0, tol=0.0, return_sweeps=False):
    """Batched symmetric eigendecomposition on the device (feta_eigh_sym): a [B,N,N] (lower triangle
    read, a + shift*I positive definite), n_real [B] int32 -> u [B,N,K] (ascending, zero-padded),
    lam [B,K].  Replaces the per-graph host eig of transformer/position_encoding.py:127-161."""
    abi, stream = _lib.backend(a)
    b, n, _ = a.shape
    k = n if k is None else int(k)
    if not abi.eigh_sym_supported(n):
        raise ValueError('eigh_sym: N = %d is beyond the kernels (N <= 256); decompose on the host' % n)
    u = torch.empty((b, n, k), dtype=torch.float32, device=a.device)
    lam = torch.empty((b, k), dtype=torch.float32, device=a.device)
    sweeps = torch.empty((b,), dtype=torch.int32, device=a.device) if return_sweeps else None
    abi.eigh_sym(a.contiguous(), n_real.contiguous(), float(shift), u, lam, sweeps, int(max_sweeps),
                 float(tol), stream)
    return (u, lam, sweeps) if return_sweeps else (u, lam)


SPECTRAL_MODES = {'diffusion': 0, 'pstep': 1}


def spectral_kernel(u, lam, n_real, kind='diffusion', beta=1.0, p=1, lam_offset=0.0, zero_diag=False):
    """out [B,N,N] = U f(lam + lam_offset) U^T on the real block (feta_spectral_kernel):
    'diffusion' f = exp(-beta x) (transformer/position_encoding.py:65-72), 'pstep' f = (1 - beta x)^p
    (:83-93)."""
    if kind not in SPECTRAL_MODES:
        raise ValueError('unknown spectral kernel %r' % (kind,))
    abi, stream = _lib.backend(u, lam)
    b, n, _ = u.shape
    out = torch.empty((b, n, n), dtype=torch.float32, device=u.device)
    abi.spectral_kernel(u.contiguous(), lam.contiguous(), n_real.contiguous(), SPECTRAL_MODES[kind],
                        float(beta), int(p), float(lam_offset), bool(zero_diag), out, stream)
    return out


LOSS_KINDS = {'l1': _abi.LOSS_L1, 'bce_logits': _abi.LOSS_BCE_LOGITS, 'ce': _abi.LOSS_CE}


def readout_eval(y, n_real, ids, count, labels, w1, b1, w2, b2, scores, terms, loss_kind, slope=0.0):
    """Graph-level readout of an evaluation batch in one launch (feta_readout_eval), forward only: for every slot
    b < count[0] the masked mean of the rows y[:n_real[b], b] ([N, B, 64] float32, any row strides - a view is read in
    place), Linear(w1, b1) - act - Linear(w2, b2) with act(v) = v if v > 0 else slope * v, the logits into
    scores[ids[b]] ([G, C]) and the loss / metric terms of ``loss_kind`` ('l1' | 'bce_logits' | 'ce', include/feta_hip.h)
    from labels[b] (float32 or int64) into terms[ids[b]] ([G, 4]).  ids (int32, the first B elements) and count (int32,
    one element) live on the device; slots from count[0] on write nothing.  Returns (scores, terms)."""
    if loss_kind not in LOSS_KINDS:
        raise ValueError('unknown loss_kind %r' % (loss_kind,))
    abi, stream = _lib.backend(y, n_real, ids, count, labels, w1, b1, w2, b2, scores, terms)
    if y.dim() != 3 or y.stride(2) != 1:
        raise ValueError('readout_eval: y must be [N, B, d] with dense columns, got %s with strides %s' % (tuple(y.shape), y.stride()))
    n, b, d = y.shape
    if scores.dim() != 2 or terms.dim() != 2 or terms.shape != (scores.shape[0], 4):
        raise ValueError('readout_eval: scores [G, C] and terms [G, 4], got %s and %s' % (tuple(scores.shape), tuple(terms.shape)))
    g, c = scores.shape
    if not abi.readout_eval_supported(d, c):
        raise ValueError('readout_eval: d = %d, C = %d (the kernel has d = 64 and 1 <= C <= 64)' % (d, c))
    for name, t, shape in (('n_real', n_real, (b,)), ('w1', w1, (d, d)), ('b1', b1, (d,)), ('w2', w2, (c, d)), ('b2', b2, (c,))):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError('readout_eval: %s must be contiguous %s, got %s' % (name, shape, tuple(t.shape)))
    for name, t, least in (('ids', ids, b), ('count', count, 1), ('labels', labels, b)):
        if t.numel() < least or not t.is_contiguous():
            raise ValueError('readout_eval: %s must be contiguous with at least %d elements' % (name, least))
    if not (scores.is_contiguous() and terms.is_contiguous()):
        raise ValueError('readout_eval: scores and terms must be contiguous')
    if labels.dtype not in (torch.float32, torch.int64):
        raise TypeError('readout_eval: float32 or int64 labels, got %s' % labels.dtype)
    kind = _abi.LABELS_GRAPH_F32 if labels.dtype == torch.float32 else _abi.LABELS_GRAPH_I64
    # (the stride of a size-1 dim is arbitrary and multiplies index 0 only)
    abi.readout_eval(b, n, g, c, stream, d_model=d, row_sb=y.stride(1) if b > 1 else 0, row_sn=y.stride(0) if n > 1 else 0,
                     label_kind=kind, loss_kind=LOSS_KINDS[loss_kind], slope=float(slope), y=y, n_real=n_real, ids=ids,
                     count=count, labels=labels, w1=w1, b1=b1, w2=w2, b2=b2, scores=scores, terms=terms)
    return scores, terms


def _row_strides(t):
    """(graph stride, node stride) in elements of a [N, B, d] tensor (the stride of a size-1 dim is arbitrary and multiplies
    index 0 only)"""
    return (t.stride(1) if t.shape[1] > 1 else 0), (t.stride(0) if t.shape[0] > 1 else 0)


class _ReadoutTrainFn(torch.autograd.Function):
    """readout_train below: the forward is feta_readout_train_fwd, the backward feta_readout_train_bwd on the same
    workspace; the incoming gradient of the loss stays on the device."""

    @staticmethod
    def forward(ctx, y, n_real, count, labels, w1, b1, w2, b2, loss_kind, slope):
        abi, stream = _lib.backend(y, n_real, count, labels, w1, b1, w2, b2)
        n, b, d = y.shape
        c = w2.shape[0]
        dev = y.device
        scores = torch.empty((b, c), dtype=torch.float32, device=dev)
        loss = torch.empty((2,), dtype=torch.float32, device=dev)
        ws = torch.empty((abi.readout_train_ws_floats(b, c),), dtype=torch.float32, device=dev)
        sb, sn = _row_strides(y)
        ctx.kw = dict(d_model=d, row_sb=sb, row_sn=sn, loss_kind=loss_kind, slope=slope,
                      label_kind=_abi.LABELS_GRAPH_F32 if labels.dtype == torch.float32 else _abi.LABELS_GRAPH_I64)
        abi.readout_train_fwd(b, n, c, stream, y=y, n_real=n_real, count=count, labels=labels, w1=w1, b1=b1, w2=w2, b2=b2,
                              scores=scores, loss=loss, ws=ws, **ctx.kw)
        ctx.save_for_backward(y, n_real, count, labels, w1, b1, w2, b2, scores, loss, ws)
        ctx.mark_non_differentiable(scores)
        ctx.set_materialize_grads(False)      # (no launch that zero-fills a gradient for the scores)
        return loss[0], scores

    @staticmethod
    def backward(ctx, dloss, _dscores):
        if dloss is None:
            return (None,) * 10
        y, n_real, count, labels, w1, b1, w2, b2, scores, loss, ws = ctx.saved_tensors
        abi, stream = _lib.backend(y, dloss)
        n, b, d = y.shape
        c = w2.shape[0]
        need = ctx.needs_input_grad
        new = lambda like, wanted: torch.empty(like.shape, dtype=torch.float32, device=y.device) if wanted else None
        dy, dw1, dw2 = new(y, need[0]), new(w1, need[4]), new(w2, need[6])
        db1 = new(b1, need[5]) if b1 is not None else None
        db2 = new(b2, need[7]) if b2 is not None else None
        dsb, dsn = _row_strides(dy) if dy is not None else (0, 0)
        abi.readout_train_bwd(b, n, c, stream, drow_sb=dsb, drow_sn=dsn, y=y, n_real=n_real, count=count, labels=labels,
                              w1=w1, b1=b1, w2=w2, b2=b2, scores=scores, loss=loss, ws=ws,
                              dloss=dloss.to(torch.float32).reshape(1).contiguous(), dy=dy, dw1=dw1, db1=db1, dw2=dw2, db2=db2,
                              **ctx.kw)
        return dy, None, None, None, dw1, db1, dw2, db2, None, None


def readout_train(y, n_real, count, labels, w1, b1, w2, b2, loss_kind, slope=0.0):
    """Graph-level readout of a TRAINING batch (feta_readout_train_fwd / _bwd, two launches each): for every slot
    b < count[0] the masked mean of the rows y[:n_real[b], b] ([N, B, 64] float32, any row strides), Linear(w1, b1) - act -
    Linear(w2, b2) with act(v) = v if v > 0 else slope * v, and the batch loss of train.task_loss for ``loss_kind``
    ('l1' | 'bce_logits' | 'ce') from labels[b] (float32 or int64): sum of the slots' terms over sum of their weights (a NaN
    label under 'bce_logits' has weight 0; no labelled slot at all: NaN).  count (int32, one element) lives on the device.
    -> (loss 0-d, scores [B, C]); the rows of scores from count[0] on are not written.  Differentiable in y, w1, b1, w2, b2
    through the loss (scores carry no gradient); dy is zero in the padded rows and in the slots from count[0] on.  Under
    torch.no_grad() only the forward launches run."""
    if loss_kind not in LOSS_KINDS:
        raise ValueError('unknown loss_kind %r' % (loss_kind,))
    abi, _ = _lib.backend(y, n_real, count, labels, w1, b1, w2, b2)
    if y.dim() != 3 or y.stride(2) != 1:
        raise ValueError('readout_train: y must be [N, B, d] with dense columns, got %s with strides %s' % (tuple(y.shape), y.stride()))
    n, b, d = y.shape
    if w2.dim() != 2:
        raise ValueError('readout_train: w2 must be [C, d], got %s' % (tuple(w2.shape),))
    c = w2.shape[0]
    if not abi.readout_train_supported(d, c):
        raise ValueError('readout_train: d = %d, C = %d (the kernels have d = 64 and 1 <= C <= 64)' % (d, c))
    for name, t, shape in (('n_real', n_real, (b,)), ('w1', w1, (d, d)), ('b1', b1, (d,)), ('w2', w2, (c, d)), ('b2', b2, (c,))):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous()):
            raise ValueError('readout_train: %s must be contiguous %s, got %s' % (name, shape, tuple(t.shape)))
    for name, t, least in (('count', count, 1), ('labels', labels, b)):
        if t.numel() < least or not t.is_contiguous():
            raise ValueError('readout_train: %s must be contiguous with at least %d elements' % (name, least))
    if labels.dtype not in (torch.float32, torch.int64):
        raise TypeError('readout_train: float32 or int64 labels, got %s' % labels.dtype)
    return _ReadoutTrainFn.apply(y, n_real, count, labels, w1, b1, w2, b2, LOSS_KINDS[loss_kind], float(slope))
