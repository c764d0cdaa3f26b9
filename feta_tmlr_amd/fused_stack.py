"""The whole stack of DiffTransformerEncoderLayers as ONE autograd node with a hand-scheduled forward
and backward over the C ABI: FusedEncoderStackFn (BatchNorm layers, described here) and
FusedLayerNormStackFn (LayerNorm layers, described at the class and at _ln_on_load_forward).  The two nodes and the three
LayerNorm forward forms hold the per-layer schedules only; what they share exists once: the per-call geometry (_Geom,
on ctx.geom), the forward and backward prologues and epilogues (_begin_* / _finish_*), the attention half's allocations
(_attn_alloc), the launch sequences without the fused kernels (_attn_fwd_unfused, _ffn_bwd_unfused, _attn_bwd_unfused)
and the flat gradient buffer with its slot allocator (_GradSlots).

Per layer, forward (5 launches):
    F1  qkv  = BN2_prev(y2_prev) W_in^T                       feta_rowlin_fwd_ex (finalizes BN2_prev)
    F2  concat, attn = attention core                         feta_attn_fwd
    F3  y1   = X0 + degree * (concat W_o^T + b_o), stats1     feta_rowlin_fwd_ex (residual through BN2_prev)
    F4  h    = relu(BN1(y1) W_1^T + b_1)                      feta_rowlin_fwd_ex (finalizes BN1)
    F5  y2   = BN1(y1) + h W_2^T + b_2, stats2                feta_rowlin_fwd_ex (residual through BN1)
and one feta_bn_apply_fwd_prm at the end of the stack.  BatchNorm never runs as a pass of its own:
statistics come out of the producer's epilogue, the apply happens inside the consumers' operand
loads, and normalised activations are never materialised between layers.
Backward (6 launches + the weight-gradient reductions per layer): the BatchNorm backward of the
incoming gradient is applied inside the gradient loads of feta_rowlin_bwd_ex, the residual
gradients are added in its dX epilogue, and the partial sums the next BatchNorm backward needs are
emitted there too - no stand-alone BatchNorm, add or fill kernels.

Reference semantics: DiffTransformerEncoderLayer.forward as reconstructed in
feta_tmlr_amd/transformer/layers.py (contract transformer/models.py:166-167).
"""
import os
import weakref

import torch

from . import _lib


def _views(t, l0, l1, heads, dh):
    v5 = t.view(l0, l1, 3, heads, dh)
    return [v5[:, :, i].permute(1, 0, 2, 3) for i in range(3)]


PER_LAYER = 12  # tensors per layer in the flat parameter list
# in_proj + attention + out_proj of a layer as one launch where the shape allows (csrc/block.hip);
# FETA_ATTN_BLOCK=0 keeps the three-launch sequence (A/B timing, fallback for other shapes)
USE_ATTN_BLOCK = os.environ.get('FETA_ATTN_BLOCK', '1') != '0'
USE_FFN_FUSED = os.environ.get('FETA_FFN_FUSED', '1') != '0'
# graphs beyond the one-launch block (64 < N <= 256, config 4): attention core + out_proj + degree + residual + statistics
# as one launch behind the in_proj launch (csrc/attnout.hip); 0: feta_attn_fwd -> feta_rowlin_fwd_ex
USE_ATTN_OUT = os.environ.get('FETA_ATTN_OUT', '1') != '0'
# LayerNorm of the feed-forward kernel's OUTPUT rows in its epilogue (feta_ffn.y_ln_out) where nobody downstream applies it
# on load; 0: feta_layernorm_fwd launches (A/B timing)
USE_LN_EPILOGUE = os.environ.get('FETA_LN_EPILOGUE', '1') != '0'
# backward of the FFN half (linear2 + linear1) in one launch (csrc/ffn_bwd.hip); 0: two feta_rowlin_bwd_ex launches
USE_FFN_BWD = os.environ.get('FETA_FFN_BWD', '1') != '0'
# backward of the attention sub-block (out_proj + attention + in_proj) in one launch per layer (csrc/block_bwd.hip,
# one workgroup per graph, up to 256 graphs); 0: three launches
USE_ATTN_BLOCK_BWD = os.environ.get('FETA_ATTN_BLOCK_BWD', '1') != '0'
# two workgroups per graph (one per pair of heads) where the consumer of dx is the fused FFN backward, which adds the
# two parts on load (feta_attn_block_grad.dx_b); 0: one workgroup per graph everywhere (A/B timing)
USE_ATTN_BLOCK_SPLIT = os.environ.get('FETA_ATTN_BLOCK_SPLIT', '1') != '0'
# more graphs than workgroups (B > 256): the fused attention-block backward walks several graphs per workgroup.  Until the
# lane id was laundered once per graph (csrc/block_bwd.hip: everything a lane derives from its id is invariant in the
# graph loop and was hoisted - up to 676 B of scratch per lane) that instantiation was slower than the three-launch form
# on fp32 (molhiv B = 1024, N_pad = 64: 533 k vs 649 k graphs/s); spill-free it wins: 734 k vs 663 k fp32, 901 k (777 k)
# bf16, ZINC B = 512 736 k vs 699 k.  0: three launches for fp32 stacks beyond 256 graphs (A/B timing)
USE_ATTN_BLOCK_BWD_LOOP = os.environ.get('FETA_BLOCK_BWD_LOOP', '1') != '0'


def _fused_attn_bwd(abi, b, n, d, heads, tie, dt):
    if not (USE_ATTN_BLOCK_BWD and not tie and abi.attn_block_bwd_supported(n, d, heads)):
        return False
    if heads != 4 and dt != torch.float32:   # (the 8-head form is fp32 storage only)
        return False
    gb = abi.attn_block_bwd_blocks(b)
    return gb > 0 and (gb == b or dt != torch.float32 or USE_ATTN_BLOCK_BWD_LOOP)

def layer_params(layer):
    a = layer.self_attn
    return [a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias,
            layer.norm1.weight, layer.norm1.bias, layer.linear1.weight, layer.linear1.bias,
            layer.linear2.weight, layer.linear2.bias, layer.norm2.weight, layer.norm2.bias]


# the split-K partials that are complete when the LAST launch of a stack's backward starts (every layer but the first, and
# the first layer's feed-forward half) are reduced in trailing workgroups of that launch (feta_attn_block_bwd_sums): the
# final reduction launch is left with that launch's own columns (colsum 10.5 -> 8.4 us, the launch itself 24.1 -> 25.6 us:
# 0.2749 -> 0.2735 ms per step at B = 128; at B >= 512, where that launch fills the chip, it costs 0.7 % - not taken there);
# 0: everything in the final launch (A/B timing)
USE_EARLY_COLSUM = os.environ.get('FETA_EARLY_COLSUM', '1') != '0'
USE_LN_STACK = os.environ.get('FETA_LN_STACK', '1') != '0'   # 0: LayerNorm layers run op by op (A/B timing)
# LayerNorm stacks: the CONSUMER of a pre-norm tensor applies the LayerNorm when it stages the rows (ABI 9, csrc/feta_ln.h:
# norm2 inside the next layer's attention block, norm1 inside the feed-forward kernel, their backward inside the gradient
# loads of feta_ffn_bwd / feta_attn_block_bwd) - two launches per layer and direction like the BatchNorm stack, no
# normalised tensor in HBM; 0: feta_layernorm_fwd / _bwd launches between the fused kernels (round-3 form, A/B timing)
USE_LN_ON_LOAD = os.environ.get('FETA_LN_ON_LOAD', '1') != '0'
# LayerNorm stacks on load: the FORWARD of the whole stack as ONE launch (feta_encoder_fwd_save: the kernel of
# feta_encoder_infer_ex with the stores a backward pass needs) instead of two launches per layer; the backward is
# unchanged.  Opt-in: '1' here, or one_launch_forward = True on the encoder (layers.set_one_launch_forward)
USE_LN_ONE_LAUNCH = os.environ.get('FETA_LN_ONE_LAUNCH', '0') != '0'


class StackLayers(list):
    """the layers of one fused_encoder_stack call, with the encoder's one_launch_forward (None: USE_LN_ONE_LAUNCH)"""
    one_launch = None


def ln_one_launch_supported(abi, layers, n, b, d_model, tie, dt):
    """a LayerNorm-on-load stack whose forward feta_encoder_fwd_save takes: one feed-forward width, head count and eps
    source for every layer, affine LayerNorms with a bias, and the shapes of the kernel (d_model = 64, N <= 64, ff 64 or
    128, 4 or - fp32 storage - 8 heads, up to 16 layers, no tie_qk).  Dropout and BatchNorm never get here
    (stack_supported / ln_on_load_supported)."""
    if tie or not len(layers) or dt not in (torch.float32, torch.bfloat16):
        return False
    l0 = layers[0]
    heads, ff = l0.self_attn.num_heads, l0.linear1.out_features
    for l in layers:
        if l.self_attn.num_heads != heads or l.linear1.out_features != ff or l.self_attn.tie_qk:
            return False
        if l.norm1.bias is None or l.norm2.bias is None:
            return False
    return abi.encoder_fwd_save_supported(n, d_model, heads, ff, len(layers), dt, tie)


def _fused_kernels_take(abi, layers, n, b, d_model, heads):
    """every launch of the stack is one of the four fused kernels (csrc/block.hip, ffn.hip, ffn_bwd.hip, block_bwd.hip)"""
    if not (USE_ATTN_BLOCK and USE_FFN_FUSED and USE_FFN_BWD and USE_ATTN_BLOCK_BWD):
        return False
    if not (abi.attn_block_supported(n, d_model, heads) and abi.attn_block_bwd_supported(n, d_model, heads)
            and abi.attn_block_bwd_blocks(b) > 0):
        return False
    return all(abi.ffn_supported(d_model, l.linear1.out_features) and abi.ffn_bwd_supported(d_model, l.linear1.out_features)
               for l in layers)


def ln_on_load_supported(abi, layers, n, b, d_model, tie):
    """the four fused kernels carry the LayerNorm on load: every launch of the stack has to be one of them"""
    if not USE_LN_ON_LOAD or tie:
        return False
    return _fused_kernels_take(abi, layers, n, b, d_model, layers[0].self_attn.num_heads)


def lowp_stack_supported(abi, layers, n, b, d_model):
    """bf16 storage (layers.set_storage_dtype): the stack runs iff every launch of it is one of the four fused kernels
    (the ones instantiated for bf16 tiles - and, LayerNorm stacks, feta_layernorm_*_ex)."""
    l0 = layers[0]
    heads = l0.self_attn.num_heads
    if heads != 4:   # the 8-head form of the block kernels (ABI 13) is instantiated for fp32 storage only
        return False
    if l0.self_attn.tie_qk or (not l0.batch_norm and not USE_LN_STACK):
        return False
    return _fused_kernels_take(abi, layers, n, b, d_model, heads)


def stack_supported(layers, d_model):
    """BatchNorm stack (training mode: batch statistics) or LayerNorm stack (any mode), no dropout."""
    from .functional import ROWLIN_DIMS, layer_norm_rows_supported
    if not len(layers):
        return False
    bn = layers[0].batch_norm
    for l in layers:
        if l.batch_norm != bn:
            return False
        if l.training and (l.dropout1.p > 0.0 or l.dropout.p > 0.0 or l.dropout2.p > 0.0 or l.self_attn.dropout > 0.0):
            return False
        if getattr(l.self_attn, 'stab', 'rowmax') != 'rowmax':    # (the fused kernels implement exp(s - rowmax))
            return False
        if bn:
            if not l.training or l.norm1.momentum is None or l.norm2.momentum is None:
                return False
        else:
            if not USE_LN_STACK or not isinstance(l.norm1, torch.nn.LayerNorm):
                return False
            if not (l.norm1.elementwise_affine and l.norm2.elementwise_affine and layer_norm_rows_supported(d_model)):
                return False
        ff = l.linear1.out_features
        if not all(c in ROWLIN_DIMS for c in (d_model, 3 * d_model, ff)):
            return False
    return True


# TEST HOOK (tests/bench_checks.py): a list that receives the per-layer saved tensors of every fused-stack forward (the
# relu output h among them - which side of a zero-to-rounding pre-activation the kernels took); None: off
CAPTURE_SAVED = None

# first layer of a stack -> the flat gradient buffer of its last backward (kept off the modules:
# state_dict / deepcopy / pickle of a model must not see it)
STACK_FLAT_GRAD = weakref.WeakKeyDictionary()

# every consumer workgroup re-reduces the partial statistics of its producer: beyond this many rows ONE reduction launch
# runs in front of the consumers (~5 us against ~G x G x 512 bytes of L2 reads).  Measured (round 3): 512 beats 384 and
# 1024 at the batches where it matters - molhiv B = 1024 bf16 948 k / 960 k / 955 k graphs/s, ZINC B = 512 fp32
# 745 k / 773 k / 770 k (the feed-forward kernels emit 512 rows there: not capped any more)
MAX_STAT_ROWS = int(os.environ.get('FETA_MAX_STAT_ROWS', '512'))


def _cap_partials(abi, stream, st, new, shift_row=False):
    """[G (+ 1), 2, D] partial sums -> the same if G is small, else their total as [1 (+ 1), 2, D] (one extra reduction
    launch, only at batch sizes where a step takes milliseconds anyway).  shift_row: BatchNorm STATISTICS carry one more
    row, the shift their sums are relative to (csrc/feta_rowops.h); it is not a partial and travels unchanged.
    -> (buffer, number of partial rows)"""
    g = st.shape[0] - (1 if shift_row else 0)
    if g <= MAX_STAT_ROWS:
        return st, g
    tot = new(2 if shift_row else 1, 2, st.shape[2])
    if shift_row:
        # (the shift row travels as a one-row "sum" of the same launch: no copy launch)
        abi.colsum_multi([(st[:g].view(g, -1), tot[0].view(-1)), (st[g].view(1, -1), tot[1].view(-1))], stream)
    else:
        abi.colsum(st[:g].view(g, -1), tot[0].view(-1), stream)
    return tot, 1


class StackTail:
    """Hand-over between the BatchNorm stack and the ONE consumer of its output when that consumer is linear_cat
    (transformer/models.py:223-224): the last BatchNorm is then never materialised either.  The stack returns the
    pre-norm y2 of the last layer and leaves its statistics here; linear_cat's forward kernel finalizes them and
    applies the normalisation inside its operand loads (functional._cat_forward), its backward kernel emits the
    partial sums (sum dout, sum dout * xhat) the BatchNorm backward needs from its dX epilogue.  Contract: the
    gradient that reaches the stack's first output is the gradient w.r.t. the NORMALISED tensor, with `gs` set.
    Saves the bn_apply_fwd and bn_bwd_reduce launches of a step."""

    def __init__(self):
        self.y2 = self.st2 = self.gamma = self.beta = self.norm = self.prm2 = self.gs = None
        self.G2 = 0


class _Geom:
    """Geometry of one stack call, its two allocators and the operands every launch shares.  The forward builds it
    (_begin_forward) and leaves it on ctx; the backward binds it to its own stream (_begin_backward)."""

    def __init__(self, abi, stream, src, pe, degree_rows, n_real, layers):
        a0 = layers[0].self_attn
        self.abi, self.stream = abi, stream
        self.n, self.b, self.d = src.shape
        self.m, self.nl = self.n * self.b, len(layers)
        self.heads, self.tie = a0.num_heads, a0.tie_qk
        self.dh = self.d // self.heads
        self.scale = float(self.dh) ** -0.5
        # bf16 storage (layers.set_storage_dtype; BASELINE configs 3 / 5): src and pe arrive as bf16, every token tensor
        # of the stack is bf16 (qkv, out, y1, h, y2 and the gradients in backward), the kernels run their bf16
        # instantiations (include/feta_hip.h: dtype = FETA_BF16).  Statistics, parameter blocks, attn, every parameter
        # gradient: fp32.  What LEAVES the stack is fp32 again - the last layer writes its y2 as fp32 (feta_ffn.y_f32) and
        # its per-head outputs once more as fp32 (feta_attn_block.out_f32) - so the filter stage behind it (coefficient
        # generator, spectral filter, linear_cat with the folded BatchNorm) runs unchanged and there is no cast launch.
        self.dt, self.dev = src.dtype, src.device
        self.lowp = self.dt != torch.float32
        self.pe = None if pe is None else pe.contiguous()
        self.rowscale, self.n_real = degree_rows, n_real
        self.G = 0      # BatchNorm stacks: row blocks of the row-wise kernels (rows of their statistics and sums)

    def new(self, *s):
        return torch.empty(s, dtype=torch.float32, device=self.dev)

    def newt(self, *s):
        """a token tensor: the stack's storage type"""
        return torch.empty(s, dtype=self.dt, device=self.dev)


def _begin_forward(ctx, src, pe, degree_rows, n_real, layers, pending):
    """-> (geometry, the stack's input rows [M, d])"""
    abi, stream = _lib.backend(src, pe, n_real)
    ctx.set_materialize_grads(False)   # no zero tensor for the (non-differentiable) attn output
    ctx.pending = pending
    STACK_FLAT_GRAD.pop(layers[0], None)   # the buffer of an earlier backward is stale from here on
    g = _Geom(abi, stream, src, pe, degree_rows, n_real, layers)
    if g.lowp and (pe is not None and pe.dtype != g.dt):
        raise TypeError('bf16 stack: pe must be %s as well' % g.dt)
    if g.lowp and not lowp_stack_supported(abi, layers, g.n, g.b, g.d):
        raise NotImplementedError('bf16 storage: the fused stack needs d_model = 64, 4 heads, N <= 64'
                                  + (', BatchNorm' if layers[0].batch_norm else ''))
    return g, src.contiguous().view(g.m, g.d)


def _attn_alloc(g, li, need_attn):
    """what the attention half of layer li writes -> (attn, ast, qkv, out, out32, y1); attn only where the caller wants
    the last layer's, out32 (the per-head outputs once more as fp32) only on the last layer of a bf16 stack"""
    last = li == g.nl - 1
    attn = g.new(g.b, g.heads, g.n, g.n) if (need_attn and last) else None
    ast = g.new(g.b, g.heads, g.n, 2)
    qkv = g.newt(g.m, 3 * g.d)
    out = g.newt(g.n, g.b, g.heads, g.dh)
    out32 = g.new(g.n, g.b, g.heads, g.dh) if (g.lowp and last) else None
    return attn, ast, qkv, out, out32, g.newt(g.m, g.d)


def _fwd_sums(pending, li):
    """the filter stage's forward column sums ride in the first launch of the stack that has trailing workgroups"""
    return pending.take_fwd() if (pending is not None and li == 0) else ()


def _attn_fwd_unfused(g, li, x, w_in, b_in, w_o, b_o, bufs, pending, bn_in=None, x_bn=None, y_shift=None):
    """The attention half without csrc/block.hip: F1 in_proj, then F2 + F3 in one launch, one workgroup per (graph, 32
    query rows) (csrc/attnout.hip), or F2 attention core and F3 out_proj + degree + residual.  BatchNorm stacks pass
    bn_in (the previous layer's norm2: finalized and applied on in_proj's operand load), x_bn (its parameter block, for
    the residual) and y_shift (norm1's running mean: the statistics of y1 are wanted)
    bufs: what _attn_alloc returned  -> (statistics [G1 + 1, 2, d], G1), or (None, 0) without y_shift"""
    abi, stream, n, b, d, m, heads = g.abi, g.stream, g.n, g.b, g.d, g.m, g.heads
    attn, ast, qkv, out, _, y1 = bufs
    dsc = abi.rowlin_ex(m, d, 3 * d, x=x, w=w_in, bias=b_in, y=qkv, **(bn_in or {}))
    abi.rowlin_fwd_ex(dsc, stream)
    st1, G1 = None, 0
    if USE_ATTN_OUT and not g.lowp and abi.attn_out_supported(n, d, heads):
        if y_shift is not None:
            G1 = abi.attn_out_stat_rows(b, n)
            st1 = g.new(G1 + 1, 2, d)      # (+ the shift row: the sums are relative to norm1's running mean)
        abi.attn_out_fwd(b, n, g.scale, stream, tie_qk=g.tie, x=x, x_bn=x_bn, w_out=w_o, b_out=b_o, pe=g.pe,
                         n_real=g.n_real, rowscale=g.rowscale, qkv=qkv, out=out, attn_stats=ast, attn=attn, y=y1,
                         y_stats=st1, y_shift=y_shift, sums=_fwd_sums(pending, li))
        if st1 is not None:
            st1, G1 = _cap_partials(abi, stream, st1, g.new, shift_row=True)
        return st1, G1
    q, k, v = _views(qkv, n, b, heads, g.dh)
    if g.tie:
        k = q
    abi.attn_fwd(q, k, v, g.pe, g.n_real, out.permute(1, 0, 2, 3), attn, ast, g.scale, stream)
    if y_shift is not None:
        G1 = g.G
        st1 = g.new(G1 + 1, 2, d)
    dsc = abi.rowlin_ex(m, d, d, x=out.view(m, d), w=w_o, bias=b_o, rowscale=g.rowscale, residual=x, res_bn=x_bn, y=y1,
                        stats=st1, stats_shift=y_shift)
    abi.rowlin_fwd_ex(dsc, stream)
    return st1, G1


def _finish_forward(ctx, g, layers, params, saved, final, out32, attn):
    """records what the backward needs -> the node's outputs (final, concat heads of the last layer, attn)"""
    ctx.saved_state = saved
    if CAPTURE_SAVED is not None:
        CAPTURE_SAVED.append(saved)
    ctx.geom = g
    ctx.params = params
    ctx.eps = [(float(l.norm1.eps), float(l.norm2.eps)) for l in layers]
    ctx.owner = layers[0]
    if attn is not None:
        ctx.mark_non_differentiable(attn)
    concat_last = (out32 if g.lowp else saved[-1]['out']).view(g.n, g.b, g.d)
    return final.view(g.n, g.b, g.d), concat_last, attn


class _GradSlots:
    """Split-K partial buffers of a stack backward, the flat gradient buffer and the slot allocator.  Two partial
    buffers, because their row counts differ: 'f' (linear2 / linear1 of every layer) has one row per
    feta_rowlin_chunks(M) row chunk, 'a' (out_proj / in_proj) the same or - with the fused attention-block backward -
    one row per graph.  flat = [f columns | a columns | norm tail] is ONE gradient buffer for the whole stack: every
    weight / bias gradient goes through the partial buffers and ONE deterministic multi-segment reduction at the end of
    backward (instead of one reduction launch per linear), the tail holds [tail_rows, d] per layer of dgamma / dbeta
    that come from elsewhere, and every parameter gradient (`grads`) is a view of it, so a data-parallel trainer
    all-reduces it in place (parallel.FlatBufferAllReduce)."""

    def __init__(self, g, params, fused_attn, ffn_fused, ln_f=False, ln_a=False, tail_rows=0):
        abi, d, nl = g.abi, g.d, g.nl
        ff0 = params[6].shape[0]
        rc = abi.rowlin_chunks(g.m)
        ra = abi.attn_block_bwd_blocks(g.b) if fused_attn else rc
        # the fused feed-forward backward chooses its own split-K chunk count (feta_ffn_bwd_chunks: the row-wise kernels'
        # chunks or, where that keeps its grid within one round of resident workgroups, half as many)
        if ffn_fused:
            rc = abi.ffn_bwd_chunks(g.m, ff0)
        # ln_f / ln_a (LayerNorm on load): every layer's slot is followed by [dgamma | dbeta] of the LayerNorm whose
        # backward the kernel applies on its gradient load (norm2 behind the feed-forward slot, norm1 behind the attention slot)
        self.tf = tf = nl * ((ff0 * d + ff0) + (d * ff0 + d) + (2 * d if ln_f else 0))
        self.ta = ta = nl * ((d * d + d) + (3 * d * d + 3 * d) + (2 * d if ln_a else 0))
        self.part_f, self.part_a = g.new(rc, tf), g.new(ra, ta)
        self.total = tf + ta
        self.flat = g.new(self.total + nl * tail_rows * d)
        self.tail = self.flat[self.total:].view(nl, tail_rows, d) if tail_rows else None
        self.cur = {'f': 0, 'a': 0}
        self.d, self.params = d, params
        self.grads = [None] * len(params)

    def _lin(self, idx, kind, no, ki):
        """the next [no, ki] weight + [no] bias columns of this kind go to parameters idx, idx + 1
        -> pointer to the linear's partial columns"""
        off = self.cur[kind]
        self.cur[kind] += no * ki + no
        buf, at = (self.part_f, off) if kind == 'f' else (self.part_a, self.tf + off)
        self.grads[idx] = self.flat[at:at + no * ki].view(no, ki)
        if self.params[idx + 1] is not None:
            self.grads[idx + 1] = self.flat[at + no * ki:at + no * ki + no]
        return buf.data_ptr() + 4 * off

    def _norm(self, idx, kind):
        """[dgamma | dbeta] of a LayerNorm on load follow the previous slot in the partial rows"""
        d = self.d
        at = (0 if kind == 'f' else self.tf) + self.cur[kind]
        self.cur[kind] += 2 * d
        self.grads[idx], self.grads[idx + 1] = self.flat[at:at + d], self.flat[at + d:at + 2 * d]

    def ffn(self, li, ff, ln=False):
        """the feed-forward half of layer li (, norm2 on load) -> partial pointers of linear2, linear1"""
        base = li * PER_LAYER
        pp = self._lin(base + 8, 'f', self.d, ff)
        pp1 = self._lin(base + 6, 'f', ff, self.d)
        if ln:
            self._norm(base + 10, 'f')
        return pp, pp1

    def attn(self, li, ln=False):
        """the attention half of layer li (, norm1 on load) -> partial pointers of out_proj, in_proj"""
        base = li * PER_LAYER
        ppo = self._lin(base + 2, 'a', self.d, self.d)
        ppi = self._lin(base + 0, 'a', 3 * self.d, self.d)
        if ln:
            self._norm(base + 4, 'a')
        return ppo, ppi

    def norm_tail(self, li, which):
        """dgamma, dbeta of norm1 (which = 0) / norm2 (1) of layer li in the tail"""
        dg, db = self.tail[li, 2 * which], self.tail[li, 2 * which + 1]
        idx = li * PER_LAYER + (10 if which else 4)
        self.grads[idx], self.grads[idx + 1] = dg, db
        return dg, db

    def early(self, a_done):
        """segments that are complete when the first layer's attention backward starts: 'f', and `a_done` columns of 'a'"""
        segs = [(self.part_f, self.flat[:self.tf])]
        if a_done > 0:
            segs.append((self.part_a[:, :a_done], self.flat[self.tf:self.tf + a_done]))
        return segs

    def rest(self, early_done=None):
        """segments of the final reduction: everything, or what early(early_done) left"""
        if early_done is not None:
            return [(self.part_a[:, early_done:], self.flat[self.tf + early_done:self.total])]
        return [(self.part_f, self.flat[:self.tf]), (self.part_a, self.flat[self.tf:self.total])]


def _begin_backward(ctx, d_final, fused_attn=None, lin_dw_rides=False):
    """Binds the geometry to this backward, takes what the filter stage left for it and shapes the incoming gradient.
    fused_attn None: _fused_attn_bwd decides.  lin_dw_rides: the first layer's feta_attn_block_bwd - the LAST launch -
    carries dW / db of the coefficient generator's linear where the kernel takes it; else the library runs it, here.
    -> (geometry, fused_attn, coeff_req, lin_dw, gradient rows [M, d] fp32)"""
    g, params = ctx.geom, ctx.params
    abi, stream = g.abi, g.stream = _lib.backend(ctx.saved_state[0]['qkv'])
    if fused_attn is None:
        fused_attn = _fused_attn_bwd(abi, g.b, g.n, g.d, g.heads, g.tie, g.dt)
    coeff_req = _coeff_bwd_request(ctx, abi, stream, g.d, params[(g.nl - 1) * PER_LAYER + 6].shape[0])
    carries = None
    if lin_dw_rides:
        carries = lambda rq: (fused_attn and g.dt == torch.float32
                              and abi.attn_block_bwd_dw_supported(g.b, g.n, g.heads, *rq.shape()))
    lin_dw = _lin_dw_request(ctx, abi, stream, carries)
    if d_final is None:   # only the per-head output of the last layer was used
        d_final = torch.zeros(g.n, g.b, g.d, dtype=torch.float32, device=g.dev)
    if d_final.dtype != torch.float32:
        d_final = d_final.float()      # (the stack's output is fp32: so is its gradient)
    return g, fused_attn, coeff_req, lin_dw, d_final.contiguous().view(g.m, g.d)


def _ffn_bwd_unfused(g, s, x, w2, w1, dy, dx1, pp, pp1, tf, load=None, lin1=None):
    """B1: linear2 backward, then B2: linear1 backward with the residual gradient added in its dX epilogue.  load: what
    the gradient load applies (BatchNorm stacks: the backward of norm2); lin1: the operand, residual and sum keywords of
    B2 (BatchNorm stacks: x_bn, add_* through norm2, sum_* for norm1's backward; LayerNorm: add_plain)"""
    abi, m, d = g.abi, g.m, g.d
    ff = w1.shape[0]
    dh_ = g.new(m, ff)
    dsc = abi.rowlin_ex(m, ff, d, x=s['h'], w=w2, dy=dy, dx=dh_, partial_ptr=pp, partial_ld=tf, **(load or {}))
    abi.rowlin_bwd_ex(dsc, None, g.stream)
    dsc = abi.rowlin_ex(m, d, ff, x=x, w=w1, dy=dh_, relu_y=s['h'], dx=dx1, partial_ptr=pp1, partial_ld=tf,
                        **(lin1 or {}))
    abi.rowlin_bwd_ex(dsc, None, g.stream)


def _attn_bwd_unfused(g, s, w_o, w_in, dy, d2, ppo, ppi, ta, load=None, in_proj=None):
    """B3: out_proj backward (gradient scaled by degree), B4: attention backward, B5: in_proj backward with the residual
    gradient in its dX epilogue.  d2: a second gradient into the per-head outputs (the last layer's concat) or None.
    load / in_proj: as _ffn_bwd_unfused (BatchNorm stacks: norm1's backward on B3's gradient load; x_bn, add_*, and
    sum_* for the previous layer's norm2 in B5)  -> dx0 [M, d] fp32"""
    abi, stream, n, b, d, m, heads, dh = g.abi, g.stream, g.n, g.b, g.d, g.m, g.heads, g.dh
    dconcat = g.new(m, d)
    dsc = abi.rowlin_ex(m, d, d, x=s['out'].view(m, d), w=w_o, dy=dy, rowscale=g.rowscale, dx=dconcat,
                        partial_ptr=ppo, partial_ld=ta, **(load or {}))
    abi.rowlin_bwd_ex(dsc, None, stream)
    dout2 = None
    if d2 is not None:
        if abi.attn_bwd_takes_dout2(n, dh, heads=heads):   # added inside the kernel's loads
            dout2 = d2.contiguous().view(n, b, heads, dh).permute(1, 0, 2, 3)
        else:
            dconcat = dconcat + d2.contiguous().view(m, d)
    q, k, v = _views(s['qkv'], n, b, heads, dh)
    if g.tie:
        k = q
    dqkv = g.new(m, 3 * d)
    dq, dk, dv = _views(dqkv, n, b, heads, dh)
    delta = g.new(b, heads, n)
    abi.attn_bwd(q, k, v, g.pe, g.n_real, s['out'].permute(1, 0, 2, 3), dconcat.view(n, b, heads, dh).permute(1, 0, 2, 3),
                 s['ast'], delta, dq, dk, dv, g.scale, stream, dout2=dout2)
    if g.tie:
        dqkv[:, :d] += dqkv[:, d:2 * d]
        dqkv[:, d:2 * d] = 0
    dx0 = g.new(m, d)
    dsc = abi.rowlin_ex(m, d, 3 * d, x=s['x0'], w=w_in, dy=dqkv, dx=dx0, partial_ptr=ppi, partial_ld=ta,
                        **(in_proj or {}))
    abi.rowlin_bwd_ex(dsc, None, stream)
    return dx0


def _finish_backward(ctx, g, sl, dcur, segments):
    """ONE reduction launch fills the flat gradient buffer: the given segments and whatever column sums the filter stage
    left for this launch (functional.PendingSums)  -> the node's gradients"""
    assert sl.cur == {'f': sl.tf, 'a': sl.ta}
    g.abi.colsum_multi(segments + _take_pending(ctx), g.stream)
    STACK_FLAT_GRAD[ctx.owner] = sl.flat
    return (dcur.view(g.n, g.b, g.d), None, None, None, None, None, None, None) + tuple(sl.grads)


class FusedEncoderStackFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, src, pe, degree_rows, n_real, layers, need_attn, tail, pending, *params):
        g, y_prev = _begin_forward(ctx, src, pe, degree_rows, n_real, layers, pending)
        abi, stream, new, newt = g.abi, g.stream, g.new, g.newt
        n, b, d, m, nl, heads = g.n, g.b, g.d, g.m, g.nl, g.heads
        G = g.G = abi.rowlin_blocks(m)
        block = USE_ATTN_BLOCK and abi.attn_block_supported(n, d, heads)
        saved = []
        st_prev, prm_prev = None, None
        for li, layer in enumerate(layers):
            (w_in, b_in, w_o, b_o, g1, be1, w1, bb1, w2, bb2, g2, be2) = params[li * PER_LAYER:(li + 1) * PER_LAYER]
            ff = w1.shape[0]
            bufs = attn, ast, qkv, out, out32, y1 = _attn_alloc(g, li, need_attn)
            bn_prev = {}
            if li > 0:
                pl = layers[li - 1].norm2
                prm_prev = new(4, d)
                bn_prev = dict(x_stats=st_prev, Gx=G2_prev, x_gamma=params[(li - 1) * PER_LAYER + 10],
                               x_beta=params[(li - 1) * PER_LAYER + 11], x_bn_out=prm_prev,
                               x_rmean=pl.running_mean, x_rvar=pl.running_var, x_nbt=pl.num_batches_tracked,
                               momentum=float(pl.momentum), eps=float(pl.eps))
                saved[li - 1]['prm2'] = prm_prev
            if block:
                # F1 + F2 + F3 in one launch, one or two workgroups per graph (csrc/block.hip)
                G1 = abi.attn_block_stat_rows(b, n)
                st1 = new(G1 + 1, 2, d)      # (+ the shift row: the sums are relative to norm1's running mean)
                abi.attn_block_fwd(b, n, g.scale, stream, heads=heads, tie_qk=g.tie, x=y_prev, w_in=w_in, b_in=b_in,
                                   w_out=w_o, b_out=b_o, pe=g.pe, n_real=n_real, rowscale=degree_rows, qkv=qkv, out=out,
                                   attn_stats=ast, attn=attn, y=y1, y_stats=st1, y_shift=layer.norm1.running_mean,
                                   out_f32=out32, sums=_fwd_sums(pending, li), **bn_prev)
                st1, G1 = _cap_partials(abi, stream, st1, new, shift_row=True)
            else:
                st1, G1 = _attn_fwd_unfused(g, li, y_prev, w_in, b_in, w_o, b_o, bufs, pending, bn_in=bn_prev, x_bn=prm_prev,
                                            y_shift=layer.norm1.running_mean)
            h, prm1 = newt(m, ff), new(4, d)
            n1 = layer.norm1
            bn1 = dict(x_stats=st1, Gx=G1, x_gamma=g1, x_beta=be1, x_bn_out=prm1, x_rmean=n1.running_mean,
                       x_rvar=n1.running_var, x_nbt=n1.num_batches_tracked, momentum=float(n1.momentum), eps=float(n1.eps))
            y2 = new(m, d) if li == nl - 1 else newt(m, d)    # (the stack's output is fp32 whatever the storage type)
            if USE_FFN_FUSED and abi.ffn_supported(d, ff):
                # F4 + F5 in one launch: the hidden activations stay in registers (csrc/ffn.hip)
                G2 = abi.ffn_blocks(m)
                st2 = new(G2 + 1, 2, d)
                abi.ffn_fwd(m, ff, stream, x=y1, w1=w1, b1=bb1, w2=w2, b2=bb2, h=h, y=y2, y_stats=st2,
                            y_shift=layer.norm2.running_mean,
                            coeff=_coeff_fwd_role(pending, li, nl, attn, n_real), **bn1)
                st2, G2 = _cap_partials(abi, stream, st2, new, shift_row=True)
            else:
                # F4
                dsc = abi.rowlin_ex(m, d, ff, relu=True, x=y1, w=w1, bias=bb1, y=h, **bn1)
                abi.rowlin_fwd_ex(dsc, stream)
                # F5
                G2 = G
                st2 = new(G2 + 1, 2, d)
                dsc = abi.rowlin_ex(m, ff, d, x=h, w=w2, bias=bb2, residual=y1, res_bn=prm1, y=y2, stats=st2,
                                    stats_shift=layer.norm2.running_mean)
                abi.rowlin_fwd_ex(dsc, stream)
            saved.append(dict(x0=y_prev, prm0=prm_prev, qkv=qkv, out=out, ast=ast, y1=y1, prm1=prm1, h=h, y2=y2))
            y_prev, st_prev, G2_prev = y2, st2, G2
        last = layers[-1].norm2
        prm2 = new(4, d)
        if tail is not None:
            # the consumer (linear_cat) finalizes and applies BN2 of the last layer: nothing is materialised
            tail.y2, tail.st2, tail.G2, tail.norm, tail.prm2 = y_prev, st_prev, G2_prev, last, prm2
            tail.gamma, tail.beta = params[(nl - 1) * PER_LAYER + 10], params[(nl - 1) * PER_LAYER + 11]
            tail.gs = None
            final = y_prev.view(m, d)
        else:
            # end of the stack: materialise BN2(y2) of the last layer
            final = new(m, d)
            abi.bn_apply_fwd_prm(y_prev, st_prev, params[(nl - 1) * PER_LAYER + 10], params[(nl - 1) * PER_LAYER + 11],
                                 final, prm2, last.running_mean, last.running_var, float(last.momentum),
                                 float(last.eps), stream, nbt=last.num_batches_tracked)
        ctx.tail = tail
        saved[-1]['prm2'] = prm2
        return _finish_forward(ctx, g, layers, params, saved, final, out32, attn)

    @staticmethod
    def backward(ctx, d_final, d_concat_last, _d_attn):
        saved, params = ctx.saved_state, ctx.params
        if d_final is None and d_concat_last is None:
            # nothing downstream used the stack (e.g. a loss on the filter coefficients alone: they derive from the
            # DETACHED attention matrix, transformer/models.py:282) - autograd still visits the node, with no gradient
            return (None,) * (8 + len(params))
        g, fused_attn, coeff_req, lin_dw, dcur = _begin_backward(ctx, d_final, lin_dw_rides=True)
        abi, stream, new, newt = g.abi, g.stream, g.new, g.newt
        n, b, d, m, nl, G = g.n, g.b, g.d, g.m, g.nl, g.G
        degree_rows = g.rowscale
        # the tail: dgamma, dbeta of norm1 / norm2 of every layer, written by the kernels that finalize the BatchNorm backward
        sl = _GradSlots(g, params, fused_attn, USE_FFN_BWD and abi.ffn_bwd_supported(d, params[6].shape[0]), tail_rows=4)
        tf, ta = sl.tf, sl.ta
        early_done = None     # 'a' columns already reduced by the last launch (USE_EARLY_COLSUM)
        dcur_b = None
        if ctx.tail is not None:
            # (StackTail contract) d_final is the gradient w.r.t. BN2(y2); its partial sums came with it
            gs = ctx.tail.gs
            Gs_cur = G if gs is None else gs.shape[0]     # (row blocks of linear_cat's backward, or one row per graph: the fold into the filter's launch)
            ctx.tail.gs = None
            if gs is None:
                raise RuntimeError('fused stack: the consumer of the un-normalised output did not leave the '
                                   'BatchNorm backward sums (StackTail contract)')
        else:
            gs, Gs_cur = new(G, 2, d), G
            abi.bn_bwd_reduce(saved[-1]['y2'], dcur, saved[-1]['prm2'], gs, stream)
        for li in range(nl - 1, -1, -1):
            s = saved[li]
            (w_in, b_in, w_o, b_o, g1, be1, w1, bb1, w2, bb2, g2, be2) = params[li * PER_LAYER:(li + 1) * PER_LAYER]
            ff = w1.shape[0]
            fin2 = new(2, d)
            dg2, db2 = sl.norm_tail(li, 1)
            pp, pp1 = sl.ffn(li, ff)
            dx1 = newt(m, d)
            # the gradient load applies the BatchNorm backward of norm2 to dcur
            load2 = dict(g_y=s['y2'], g_bn=s['prm2'], g_sum=gs, Gs=Gs_cur, g_fin_out=fin2, dgamma=dg2, dbeta=db2)
            if USE_FFN_BWD and abi.ffn_bwd_supported(d, ff):
                # B1 + B2 in one launch (csrc/ffn_bwd.hip): the hidden gradient never leaves the chip
                G1s = abi.ffn_bwd_blocks(m)
                gs1 = new(G1s, 2, d)
                abi.ffn_bwd(m, ff, stream, coeff=(coeff_req if li == nl - 1 else None), partial_ptr=pp, partial_ld=tf,
                            dy=dcur, dy_b=dcur_b, h=s['h'], w2=w2, w1=w1, x=s['y1'], x_bn=s['prm1'], dx=dx1, sum_out=gs1,
                            **load2)
                gs1, G1s = _cap_partials(abi, stream, gs1, new)
            else:
                assert dcur_b is None
                # B2: + residual BN2 backward, + sums for BN1 backward
                gs1, G1s = new(G, 2, d), G
                _ffn_bwd_unfused(g, s, s['y1'], w2, w1, dcur, dx1, pp, pp1, tf, load=load2,
                                 lin1=dict(x_bn=s['prm1'], add_dout=dcur, add_y=s['y2'], add_bn=s['prm2'], add_fin=fin2,
                                           sum_y=s['y1'], sum_bn=s['prm1'], sum_out=gs1))
            fin1 = new(2, d)
            dg1, db1 = sl.norm_tail(li, 0)
            a_done = sl.cur['a']      # 'a' columns of the layers behind this one: complete
            ppo, ppi = sl.attn(li)
            d2 = d_concat_last if li == nl - 1 else None      # (a second gradient into the last layer's per-head outputs)
            if fused_attn:
                # B3 + B4 + B5 in one launch, one workgroup per graph (csrc/block_bwd.hip): dconcat and dqkv stay on chip
                dx0 = newt(m, d)
                early = ()
                if li == 0 and USE_EARLY_COLSUM and b <= 160:   # (measured: a gain only while this launch leaves CUs idle)
                    # the last launch of this backward: everything but its own partial columns is reduced beside it
                    early, early_done = sl.early(a_done), a_done
                # the layer below takes the gradient in two parts iff its FFN backward is the fused kernel
                split = (USE_ATTN_BLOCK_SPLIT and li > 0 and USE_FFN_BWD and abi.attn_block_bwd_blocks(b) == b
                         and abi.ffn_bwd_supported(d, params[(li - 1) * PER_LAYER + 6].shape[0]))
                dx0b = newt(m, d) if split else None
                GB = abi.attn_block_bwd_blocks(b)
                gs_prev = new(2 * GB, 2, d) if li > 0 else None
                abi.attn_block_bwd(b, n, g.scale, stream, heads=g.heads, Gs=G1s, partial_ptr=ppo, partial_ld=ta, dy=dx1,
                                   y1=s['y1'], dx_b=dx0b, bn1=s['prm1'], g_sum=gs1, fin_out=fin1, dgamma=dg1, dbeta=db1,
                                   rowscale=degree_rows, w_out=w_o, w_in=w_in, qkv=s['qkv'], out=s['out'],
                                   dout2=None if d2 is None else d2.contiguous().view(m, d), pe=g.pe, n_real=g.n_real,
                                   attn_stats=s['ast'], x0=s['x0'], bn0=s['prm0'] if li > 0 else None, dx=dx0,
                                   sum_out=gs_prev, sums=early, lin_dw=(lin_dw if li == 0 else None))
                Gs_next = 2 * GB
                if gs_prev is not None:
                    gs_prev, Gs_next = _cap_partials(abi, stream, gs_prev, new)
                dcur, dcur_b, gs, Gs_cur = dx0, dx0b, gs_prev, Gs_next
                continue
            # B3: gradient = degree * BN1 backward of dx1; B5: + residual BN1 backward, + sums for the previous layer's BN2
            gs_prev = new(G, 2, d) if li > 0 else None
            dx0 = _attn_bwd_unfused(
                g, s, w_o, w_in, dx1, d2, ppo, ppi, ta,
                load=dict(g_y=s['y1'], g_bn=s['prm1'], g_sum=gs1, Gs=G1s, g_fin_out=fin1, dgamma=dg1, dbeta=db1),
                in_proj=dict(x_bn=s['prm0'], add_dout=dx1, add_y=s['y1'], add_bn=s['prm1'], add_fin=fin1,
                             sum_y=(s['x0'] if li > 0 else None), sum_bn=s['prm0'], sum_out=gs_prev))
            dcur, dcur_b, gs, Gs_cur = dx0, None, gs_prev, G
        assert dcur_b is None
        return _finish_backward(ctx, g, sl, dcur, sl.rest(early_done))


class FusedLayerNormStackFn(torch.autograd.Function):
    """The LayerNorm variant (batch_norm=False: the default of the reference's TU / molhiv / SBM scripts,
    experiments/run_transformer_gengcn_cv.py:56).  Three forward forms: on load (_ln_on_load_forward), on load as one
    launch (_ln_one_launch_forward) and, where a launch of the stack is not one of the four fused kernels, the
    MATERIALISED form here: LayerNorm is row-local, so the normalised activations are written (feta_layernorm_fwd after
    each sub-layer) and every kernel reads plain operands.
    Per layer, forward (4 launches where csrc/block.hip and csrc/ffn.hip take the shape, else 7):
        y1 = x0 + degree * out_proj(attention(in_proj(x0)))     feta_attn_block_fwd
        x1 = LN1(y1)                                             feta_layernorm_fwd
        y2 = x1 + linear2(relu(linear1(x1)))                     feta_ffn_fwd
        x2 = LN2(y2)                                             feta_layernorm_fwd
    backward (7 launches): LN2, linear2, linear1 (+ residual dy2 in its dX epilogue), LN1, out_proj,
    attention, in_proj (+ residual dy1); the weight / bias partials of the whole stack share one
    [chunks, total] buffer and the LayerNorm partials another: two reductions per stack, into the same
    flat gradient buffer layout as the BatchNorm stack (parallel.FlatBufferAllReduce)."""

    @staticmethod
    def forward(ctx, src, pe, degree_rows, n_real, layers, need_attn, tail, pending, *params):
        assert tail is None   # (LayerNorm is row-local: its output is materialised by feta_layernorm_fwd)
        g, x_in = _begin_forward(ctx, src, pe, degree_rows, n_real, layers, pending)
        abi, stream, new, newt = g.abi, g.stream, g.new, g.newt
        n, b, d, m, nl, heads = g.n, g.b, g.d, g.m, g.nl, g.heads
        ctx.on_load = ln_on_load_supported(abi, layers, n, b, d, g.tie)
        if ctx.on_load:
            one = getattr(layers, 'one_launch', None)
            if (USE_LN_ONE_LAUNCH if one is None else one) and ln_one_launch_supported(abi, layers, n, b, d, g.tie, g.dt):
                return _ln_one_launch_forward(ctx, g, x_in, layers, need_attn, pending, params)
            return _ln_on_load_forward(ctx, g, x_in, layers, need_attn, pending, params)
        block = USE_ATTN_BLOCK and abi.attn_block_supported(n, d, heads)
        saved = []
        for li, layer in enumerate(layers):
            (w_in, b_in, w_o, b_o, g1, be1, w1, bb1, w2, bb2, g2, be2) = params[li * PER_LAYER:(li + 1) * PER_LAYER]
            ff = w1.shape[0]
            bufs = attn, ast, qkv, out, out32, y1 = _attn_alloc(g, li, need_attn)
            if block:
                abi.attn_block_fwd(b, n, g.scale, stream, heads=heads, tie_qk=g.tie, x=x_in, w_in=w_in, b_in=b_in, w_out=w_o,
                                   b_out=b_o, pe=g.pe, n_real=n_real, rowscale=degree_rows, qkv=qkv, out=out,
                                   attn_stats=ast, attn=attn, y=y1, y_stats=new(abi.attn_block_stat_rows(b, n) + 1, 2, d),   # (statistics unused)
                                   out_f32=out32, sums=_fwd_sums(pending, li))
            else:
                _attn_fwd_unfused(g, li, x_in, w_in, b_in, w_o, b_o, bufs, pending)
            h, y2 = newt(m, ff), newt(m, d)
            # norm1 on load (ABI 9) where the feed-forward half runs as its two fused kernels: x1 is never written, the
            # backward recomputes it from y1 and takes the LayerNorm backward of norm2 on its gradient load
            ffn_on_load = (USE_LN_ON_LOAD and USE_FFN_FUSED and USE_FFN_BWD and abi.ffn_supported(d, ff)
                           and abi.ffn_bwd_supported(d, ff))
            x1 = lst1 = None
            if ffn_on_load and li == nl - 1:
                y2 = new(m, d)      # (its gradient arrives as fp32: feta_ffn_bwd wants dy and g_y of one type)
            if not ffn_on_load:
                x1, lst1 = newt(m, d), new(m, 2)
                abi.layernorm_fwd(y1, g1, be1, float(layer.norm1.eps), x1, lst1, stream)
            x2 = lst2 = None
            if ffn_on_load:
                ln_out = {}
                if USE_LN_EPILOGUE:
                    # x2 = LN2(y2) from the same launch (feta_ffn.y_ln_out): its consumers here - in_proj, the residual of
                    # feta_attn_out_fwd - are not on-load kernels, so it is materialised, but not by a launch of its own
                    x2 = new(m, d) if li == nl - 1 else newt(m, d)
                    ln_out = dict(y_ln_out=x2, y_ln_gamma=g2, y_ln_beta=be2, y_ln_eps=float(layer.norm2.eps))
                abi.ffn_fwd(m, ff, stream, eps=float(layer.norm1.eps), x=y1, x_ln_gamma=g1, x_ln_beta=be1, w1=w1, b1=bb1,
                            w2=w2, b2=bb2, h=h, y=y2, coeff=_coeff_fwd_role(pending, li, nl, attn, n_real), **ln_out)
            elif USE_FFN_FUSED and abi.ffn_supported(d, ff):
                abi.ffn_fwd(m, ff, stream, x=x1, w1=w1, b1=bb1, w2=w2, b2=bb2, h=h, y=y2,
                            coeff=_coeff_fwd_role(pending, li, nl, attn, n_real))
            else:
                dsc = abi.rowlin_ex(m, d, ff, relu=True, x=x1, w=w1, bias=bb1, y=h)
                abi.rowlin_fwd_ex(dsc, stream)
                dsc = abi.rowlin_ex(m, ff, d, x=h, w=w2, bias=bb2, residual=x1, y=y2)
                abi.rowlin_fwd_ex(dsc, stream)
            if x2 is None:
                x2, lst2 = (new(m, d) if li == nl - 1 else newt(m, d)), new(m, 2)   # (the stack's output is fp32)
                abi.layernorm_fwd(y2, g2, be2, float(layer.norm2.eps), x2, lst2, stream)
            saved.append(dict(x0=x_in, qkv=qkv, out=out, ast=ast, y1=y1, lst1=lst1, x1=x1, h=h, y2=y2, lst2=lst2,
                              ffn_on_load=ffn_on_load))
            x_in = x2
        # (a fresh tensor object for the output: the saved x2 of the last layer is not handed out)
        return _finish_forward(ctx, g, layers, params, saved, x_in, out32, attn)

    @staticmethod
    def backward(ctx, d_final, d_concat_last, _d_attn):
        saved, params = ctx.saved_state, ctx.params
        if d_final is None and d_concat_last is None:
            return (None,) * (8 + len(params))      # (see FusedEncoderStackFn.backward)
        if ctx.on_load:
            return _ln_on_load_backward(ctx, d_final, d_concat_last)
        g, fused_attn, coeff_req, _, dcur = _begin_backward(ctx, d_final)
        abi, stream, new, newt = g.abi, g.stream, g.new, g.newt
        n, b, d, m, nl = g.n, g.b, g.d, g.m, g.nl
        GL = abi.layernorm_blocks(m)
        # feed-forward half on its fused kernels with the LayerNorms on load (ABI 9): norm2's backward is taken on the
        # gradient load of feta_ffn_bwd ([dgamma2 | dbeta2] in its partial rows, behind db1), x1 = LN1(y1) on its operand
        # load; norm1's backward stays a launch (no saved statistics: recomputed from y1)
        ffn_on_load = all(s_['ffn_on_load'] for s_ in saved)     # (one feed-forward width per stack: all or none)
        lnw = 2 if ffn_on_load else 4               # LayerNorm partial columns per layer that come from feta_layernorm_bwd
        # the tail: dgamma1, dbeta1 (, dgamma2, dbeta2) per layer
        sl = _GradSlots(g, params, fused_attn, bool(ffn_on_load or (USE_FFN_BWD and abi.ffn_bwd_supported(d, params[6].shape[0]))),
                        ln_f=ffn_on_load, tail_rows=lnw)
        tf, ta = sl.tf, sl.ta
        ln_part = new(GL, nl * lnw * d)

        def ln_bwd(dout, y, stats, gamma, li, which, eps=1e-5):
            dy = newt(m, d)
            abi.layernorm_bwd(dout, y, stats, gamma, dy, None, None, stream, partial_ld=nl * lnw * d,
                              partial_ptr=ln_part.data_ptr() + 4 * (li * lnw + 2 * which) * d, eps=eps)
            sl.norm_tail(li, which)
            return dy

        for li in range(nl - 1, -1, -1):
            s = saved[li]
            (w_in, b_in, w_o, b_o, g1, be1, w1, bb1, w2, bb2, g2, be2) = params[li * PER_LAYER:(li + 1) * PER_LAYER]
            ff = w1.shape[0]
            eps1, eps2 = ctx.eps[li]
            if not ffn_on_load:
                dy2 = ln_bwd(dcur, s['y2'], s['lst2'], g2, li, 1, eps2)
            pp, pp1 = sl.ffn(li, ff, ln=ffn_on_load)
            dx1 = newt(m, d)
            if ffn_on_load:
                abi.ffn_bwd(m, ff, stream, coeff=(coeff_req if li == nl - 1 else None), partial_ptr=pp, partial_ld=tf,
                            dy=dcur, g_y=s['y2'], g_ln_gamma=g2, ln_eps=eps2, h=s['h'], w2=w2, w1=w1, x=s['y1'],
                            x_ln_gamma=g1, x_ln_beta=be1, dx=dx1)
            elif USE_FFN_BWD and abi.ffn_bwd_supported(d, ff):
                # linear2 + linear1 backward in one launch (csrc/ffn_bwd.hip), dx1 = dy2 + dh W1
                abi.ffn_bwd(m, ff, stream, coeff=(coeff_req if li == nl - 1 else None), partial_ptr=pp, partial_ld=tf,
                            dy=dy2, h=s['h'], w2=w2, w1=w1, x=s['x1'],
                            dx=dx1)
            else:
                _ffn_bwd_unfused(g, s, s['x1'], w2, w1, dy2, dx1, pp, pp1, tf, lin1=dict(add_plain=dy2))
            dy1 = ln_bwd(dx1, s['y1'], s['lst1'], g1, li, 0, eps1)     # (lst1 None: LayerNorm on load - recomputed)
            ppo, ppi = sl.attn(li)
            d2 = d_concat_last if li == nl - 1 else None      # (a second gradient into the last layer's per-head outputs)
            if fused_attn:
                # out_proj + attention + in_proj backward in one launch, one workgroup per graph (csrc/block_bwd.hip)
                dcur = newt(m, d)
                abi.attn_block_bwd(b, n, g.scale, stream, heads=g.heads, partial_ptr=ppo, partial_ld=ta, dy=dy1,
                                   rowscale=g.rowscale, w_out=w_o, w_in=w_in, qkv=s['qkv'], out=s['out'],
                                   dout2=None if d2 is None else d2.contiguous().view(m, d), pe=g.pe, n_real=g.n_real,
                                   attn_stats=s['ast'], x0=s['x0'], dx=dcur)
            else:
                dcur = _attn_bwd_unfused(g, s, w_o, w_in, dy1, d2, ppo, ppi, ta, in_proj=dict(add_plain=dy1))
        return _finish_backward(ctx, g, sl, dcur, sl.rest() + [(ln_part, sl.flat[sl.total:])])


def _ln_on_load_forward(ctx, g, x_pre, layers, need_attn, pending, params):
    """LayerNorm stack with the LayerNorm applied by the consumer of each pre-norm tensor (ABI 9).  Per layer, forward
    (2 launches):
        y1 = x0 + degree * out_proj(attention(in_proj(x0))),  x0 = LN2_prev(y2_prev) on load     feta_attn_block_fwd
        y2 = x1 + linear2(relu(linear1(x1))),                 x1 = LN1(y1) on load               feta_ffn_fwd
    and ONE feta_layernorm_fwd at the end of the stack (norm2 of the last layer: the output is handed out).  Backward
    (2 launches per layer + one reduction): feta_ffn_bwd takes the gradient w.r.t. LN2(y2) and applies the LayerNorm
    backward where it loads the gradient rows, feta_attn_block_bwd the same for LN1; [dgamma | dbeta] ride in the
    kernels' split-K partial rows.  No normalised activation is written between the kernels.
    x_pre: the pre-norm input rows of the layer (layer 0: the stack input itself)."""
    abi, stream, new, newt = g.abi, g.stream, g.new, g.newt
    n, b, d, m, nl = g.n, g.b, g.d, g.m, g.nl
    saved = []
    ln_prev = {}
    for li, layer in enumerate(layers):
        (w_in, b_in, w_o, b_o, g1, be1, w1, bb1, w2, bb2, g2, be2) = params[li * PER_LAYER:(li + 1) * PER_LAYER]
        ff = w1.shape[0]
        attn, ast, qkv, out, out32, y1 = _attn_alloc(g, li, need_attn)
        abi.attn_block_fwd(b, n, g.scale, stream, heads=g.heads, x=x_pre, w_in=w_in, b_in=b_in, w_out=w_o, b_out=b_o, pe=g.pe,
                           n_real=g.n_real, rowscale=g.rowscale, qkv=qkv, out=out, attn_stats=ast, attn=attn, y=y1,
                           y_stats=None, out_f32=out32, sums=_fwd_sums(pending, li), **ln_prev)
        h = newt(m, ff)
        y2 = new(m, d) if li == nl - 1 else newt(m, d)    # (what leaves the stack is fp32 whatever the storage type)
        # norm2 of the LAST layer is what the stack hands out: the feed-forward kernel writes it beside y2 from its epilogue
        # (feta_ffn.y_ln_out) - the stack launches no LayerNorm kernel at all
        ln_out = {}
        if li == nl - 1 and USE_LN_EPILOGUE:
            final = new(m, d)
            ln_out = dict(y_ln_out=final, y_ln_gamma=g2, y_ln_beta=be2, y_ln_eps=float(layer.norm2.eps))
        abi.ffn_fwd(m, ff, stream, eps=float(layer.norm1.eps), x=y1, x_ln_gamma=g1, x_ln_beta=be1, w1=w1, b1=bb1, w2=w2,
                    b2=bb2, h=h, y=y2, y_stats=None, coeff=_coeff_fwd_role(pending, li, nl, attn, g.n_real), **ln_out)
        saved.append(dict(x0=x_pre, qkv=qkv, out=out, ast=ast, y1=y1, h=h, y2=y2))
        x_pre = y2
        ln_prev = dict(x_ln_gamma=g2, x_ln_beta=be2, eps=float(layer.norm2.eps))
    if not USE_LN_EPILOGUE:
        # norm2 of the last layer as a launch of its own (FETA_LN_EPILOGUE=0: A/B timing)
        final = new(m, d)
        abi.layernorm_fwd(x_pre, g2, be2, float(layers[-1].norm2.eps), final, new(m, 2), stream)
    return _finish_forward(ctx, g, layers, params, saved, final, out32, attn)


def _encoder_table(layers, params, contiguous=False, running_stats=False):
    """The feta_encoder_layer table of a one-launch stack (feta_encoder_fwd_save, feta_encoder_infer[_ex]) as _abi takes
    it: one dict per layer out of the flat parameter list.  contiguous: copy what is not (the caller holds no autograd
    node that would keep the strides); running_stats: BatchNorm in eval mode - mean and variance of norm1 / norm2."""
    if contiguous:
        t = lambda p: None if p is None else p.detach().contiguous()
    else:
        t = lambda p: None if p is None else p.detach()
    table = []
    for li, l in enumerate(layers):
        (w_in, b_in, w_o, b_o, g1, be1, w1, bb1, w2, bb2, g2, be2) = params[li * PER_LAYER:(li + 1) * PER_LAYER]
        e = dict(w_in=t(w_in), b_in=t(b_in), w_out=t(w_o), b_out=t(b_o), n1_gamma=t(g1), n1_beta=t(be1),
                 w1=t(w1), b1=t(bb1), w2=t(w2), b2=t(bb2), n2_gamma=t(g2), n2_beta=t(be2),
                 n1_eps=float(l.norm1.eps), n2_eps=float(l.norm2.eps), tie_qk=int(l.self_attn.tie_qk))
        if running_stats:
            e.update(n1_mean=t(l.norm1.running_mean), n1_var=t(l.norm1.running_var),
                     n2_mean=t(l.norm2.running_mean), n2_var=t(l.norm2.running_var))
        table.append(e)
    return table


def _ln_one_launch_forward(ctx, g, x_pre, layers, need_attn, pending, params):
    """_ln_on_load_forward as ONE launch (feta_encoder_fwd_save): every layer of a graph runs in one workgroup with the
    activations in LDS, and each layer writes what _ln_on_load_backward reads - qkv, out, the softmax statistics, y1, h,
    y2 - in the layouts and storage type of feta_attn_block_fwd / feta_ffn_fwd.  The saved tensors are views of one
    [L, ...] allocation per kind; x0 of layer l > 0 is y2 of layer l - 1.  The pending forward column sums ride in trailing
    workgroups of the launch; the coefficient generator's forward does not (it reads the attention matrix this launch
    writes): pending.coeff_fwd_req stays and the filter stage (functional._coeff_forward) runs its own launch."""
    new, newt = g.new, g.newt
    n, b, d, m, nl, heads, dh, lowp = g.n, g.b, g.d, g.m, g.nl, g.heads, g.dh, g.lowp
    ff = params[6].shape[0]
    attn = new(b, heads, n, n) if need_attn else None
    qkv, out, ast = newt(nl, m, 3 * d), newt(nl, n, b, heads, dh), new(nl, b, heads, n, 2)
    y1, h, y2 = newt(nl, m, d), newt(nl, m, ff), newt(nl, m, d)
    y2_last = new(m, d) if lowp else y2[nl - 1]      # (what leaves the stack is fp32 whatever the storage type)
    out32 = new(n, b, heads, dh) if lowp else None
    final = new(m, d)
    g.abi.encoder_fwd_save(b, n, heads, ff, _encoder_table(layers, params), g.stream, dtype=g.dt, x=x_pre, pe=g.pe,
                           n_real=g.n_real, rowscale=g.rowscale, y=final, out=out32, attn=attn, qkv=qkv, out_save=out,
                           attn_stats=ast, y1=y1, h=h, y2=y2, y2_last_f32=(y2_last if lowp else None),
                           sums=(pending.take_fwd() if pending is not None else ()))
    saved = []
    for li in range(nl):
        saved.append(dict(x0=x_pre, qkv=qkv[li], out=out[li], ast=ast[li], y1=y1[li], h=h[li],
                          y2=(y2_last if li == nl - 1 else y2[li])))
        x_pre = saved[-1]['y2']
    return _finish_forward(ctx, g, layers, params, saved, final, out32, attn)


def _ln_on_load_backward(ctx, d_final, d_concat_last):
    saved, params = ctx.saved_state, ctx.params
    g, _, coeff_req, _, dcur = _begin_backward(ctx, d_final, fused_attn=True)
    abi, stream, newt = g.abi, g.stream, g.newt
    n, b, d, m, nl = g.n, g.b, g.d, g.m, g.nl
    # no tail: each slot is followed by its LayerNorm's [dgamma | dbeta]
    sl = _GradSlots(g, params, True, True, ln_f=True, ln_a=True)
    tf, ta = sl.tf, sl.ta
    dcur_b = None      # (dcur, dcur_b: gradient w.r.t. LN2(y2) of the layer at hand, in one or two parts)
    GB = abi.attn_block_bwd_blocks(b)
    for li in range(nl - 1, -1, -1):
        s = saved[li]
        (w_in, b_in, w_o, b_o, g1, be1, w1, bb1, w2, bb2, g2, be2) = params[li * PER_LAYER:(li + 1) * PER_LAYER]
        ff = w1.shape[0]
        eps1, eps2 = ctx.eps[li]
        pp, _ = sl.ffn(li, ff, ln=True)
        dx1 = newt(m, d)
        # linear2 + linear1 backward; LN2 backward on the gradient load, x1 = LN1(y1) on the operand load
        abi.ffn_bwd(m, ff, stream, coeff=(coeff_req if li == nl - 1 else None), partial_ptr=pp, partial_ld=tf,
                    dy=dcur, dy_b=dcur_b, g_y=s['y2'], g_ln_gamma=g2, ln_eps=eps2, h=s['h'], w2=w2, w1=w1, x=s['y1'],
                    x_ln_gamma=g1, x_ln_beta=be1, dx=dx1)
        ppo, _ = sl.attn(li, ln=True)
        d2 = d_concat_last if li == nl - 1 else None      # (a second gradient into the last layer's per-head outputs)
        # out_proj + attention + in_proj backward; LN1 backward on the gradient load, x0 = LN2_prev(y2_prev) on load.  The
        # layer below takes its gradient in two parts (two workgroups per graph, one per pair of heads)
        split = USE_ATTN_BLOCK_SPLIT and li > 0 and GB == b
        dx0 = newt(m, d)
        dx0b = newt(m, d) if split else None
        ln0 = {}
        if li > 0:
            ln0 = dict(x0_ln_gamma=params[(li - 1) * PER_LAYER + 10], x0_ln_beta=params[(li - 1) * PER_LAYER + 11])
        abi.attn_block_bwd(b, n, g.scale, stream, heads=g.heads, partial_ptr=ppo, partial_ld=ta, dy=dx1, y1=s['y1'],
                           ln1_gamma=g1, ln_eps=eps1, dx_b=dx0b, rowscale=g.rowscale, w_out=w_o, w_in=w_in, qkv=s['qkv'],
                           out=s['out'], dout2=None if d2 is None else d2.contiguous().view(m, d), pe=g.pe, n_real=g.n_real,
                           attn_stats=s['ast'], x0=s['x0'], dx=dx0, **ln0)
        dcur, dcur_b = dx0, dx0b
    assert dcur_b is None
    return _finish_backward(ctx, g, sl, dcur, sl.rest())


def _coeff_fwd_role(pending, li, nl, attn, n_real):
    """The coefficient generator's forward rides in the launch of the LAST layer's feed-forward half."""
    if pending is None or li != nl - 1:
        return None
    return pending.coeff_fwd_role(attn, n_real)


def _coeff_bwd_request(ctx, abi, stream, d, ff_last):
    """The coefficient generator's backward kernel, left by its autograd node for the first launch of this backward
    (the last layer's fused FFN backward); run here on its own when that launch is not the fused kernel."""
    from . import functional as F
    req = ctx.pending.take_coeff_bwd() if ctx.pending is not None else None
    if req is None:
        return None
    hosted = USE_FFN_BWD and abi.ffn_bwd_supported(d, ff_last)
    if isinstance(req, F.CoeffSavedReq):     # the saved form (A / Bm from the filter stage's forward launch)
        if not hosted:
            req.run(abi, stream)
            req = None
        return req
    if not hosted or req[6] * req[8] > F.COEFF_ROLE_MAX_BLOCKS:
        cj, n_real, s, gb, dpooled, partial, b, n, h = req
        abi.coeff_bwd(cj, n_real, s, gb, dpooled, partial, None, None, b, n, h, stream)
        req = None
    return req


def _lin_dw_request(ctx, abi, stream, carries):
    """dW / db of the coefficient generator's C x C linear (functional.PendingSums.lin_dw_req, an _abi.LinDwReq): -> the
    request if this backward's last launch - the first layer's feta_attn_block_bwd - will carry it (carries(req)), else
    None after running it with the library and a column-sum launch, as the filter stage's node would have."""
    req = ctx.pending.take_lin_dw() if ctx.pending is not None else None
    if req is None:
        return None
    if carries is None or not carries(req):
        req.run(abi, stream)
        return None
    return req


def _take_pending(ctx):
    """Column sums the filter stage handed to the stack's reduction launch; from here on its nodes reduce on their
    own (a node of the stage that autograd schedules after this one)."""
    pend = ctx.pending
    if pend is None:
        return []
    pend.stack_done = True
    return pend.take()


def fused_encoder_stack(src, pe, degree_rows, n_real, layers, need_attn=True, tail=None, pending=None, one_launch=None):
    """-> (output [N,B,d] of the last layer, concat heads of the last layer [N,B,d], attn or None).
    tail (a StackTail, BatchNorm stacks only): the output is the PRE-norm y2 of the last layer and the tail's
    consumer applies the last BatchNorm (functional.row_linear_cat_bn).
    pending (a functional.PendingSums whose stack_armed the caller set): the stack's one reduction launch also
    carries the column sums the filter stage's backward left in it.
    one_launch (LayerNorm stacks): True / False - the forward as one launch where ln_one_launch_supported says so; None:
    USE_LN_ONE_LAUNCH."""
    params = []
    for l in layers:
        params += layer_params(l)
    bn = layers[0].batch_norm
    fn = FusedEncoderStackFn if bn else FusedLayerNormStackFn
    stack = StackLayers(layers)
    stack.one_launch = one_launch
    return fn.apply(src, pe, degree_rows, n_real, stack, need_attn, tail if bn else None, pending, *params)


def infer_supported(layers, n, d):
    """The whole stack runs as ONE launch (inference: feta_encoder_infer, ABI 12, for fp32 storage and
    feta_encoder_infer_ex for bf16 storage): one norm kind for every layer (BatchNorm in eval mode with running
    statistics, or affine LayerNorm), no active dropout, exp(s - rowmax), one storage type for every layer, and the
    shapes the kernel covers (d_model = 64, 4 or 8 heads - bf16 storage: 4 -, N <= 64, ff 64 or 128, up to 16 layers)."""
    if not len(layers):
        return False
    l0 = layers[0]
    bn, heads, ff, dt = l0.batch_norm, l0.self_attn.num_heads, l0.linear1.out_features, l0.storage_dtype
    if dt not in (torch.float32, torch.bfloat16):
        return False
    for l in layers:
        a = l.self_attn
        if l.batch_norm != bn or a.num_heads != heads or l.linear1.out_features != ff:
            return False
        if l.training and (l.dropout1.p > 0.0 or l.dropout.p > 0.0 or l.dropout2.p > 0.0 or a.dropout > 0.0):
            return False
        if getattr(a, 'stab', 'rowmax') != 'rowmax' or l.storage_dtype != dt:
            return False
        for nm in (l.norm1, l.norm2):
            if bn:
                if (not isinstance(nm, torch.nn.BatchNorm1d) or nm.training or nm.running_mean is None
                        or nm.running_var is None or nm.weight is None):
                    return False
            elif (not isinstance(nm, torch.nn.LayerNorm) or not nm.elementwise_affine or nm.bias is None
                  or tuple(nm.normalized_shape) != (d,)):
                return False
    abi = _lib._TEST_ABI if _lib._TEST_ABI is not None else _lib.abi()
    if dt == torch.float32:
        return abi.encoder_infer_supported(n, d, heads, ff, len(layers))
    return abi.encoder_infer_ex_supported(n, d, heads, ff, len(layers), dt)


def encoder_stack_infer(src, pe, degree_rows, n_real, layers, need_attn=True):
    """-> (output [N,B,d] of the last layer, concat heads of the last layer [N,B,d], attn [B,H,N,N] or None), as
    fused_encoder_stack, in ONE launch (feta_encoder_infer; bf16 storage: feta_encoder_infer_ex with bf16 tiles, src and
    pe fp32 or bf16 as they arrive, fp32 outputs): forward only - nothing is saved for a backward pass and the outputs
    carry no autograd history.  The caller checks infer_supported."""
    n, b, d = src.shape
    abi, stream = _lib.backend(src)
    l0 = layers[0]
    heads, ff, bn = l0.self_attn.num_heads, l0.linear1.out_features, l0.batch_norm
    x = src.detach().contiguous()
    y = torch.empty(n, b, d, dtype=torch.float32, device=x.device)
    concat = torch.empty_like(y)
    attn = torch.empty(b, heads, n, n, dtype=torch.float32, device=x.device) if need_attn else None
    t = lambda p: None if p is None else p.detach().contiguous()
    params = []
    for l in layers:
        params += layer_params(l)
    table = _encoder_table(layers, params, contiguous=True, running_stats=bn)
    ptrs = dict(x=x, pe=t(pe), n_real=n_real.contiguous(), rowscale=t(degree_rows), y=y, out=concat, attn=attn)
    if l0.storage_dtype == torch.float32:
        abi.encoder_infer(b, n, heads, ff, table, not bn, stream, **ptrs)
    else:
        if ptrs['pe'] is not None and ptrs['pe'].dtype != x.dtype:    # one in_dtype for both
            ptrs['pe'] = ptrs['pe'].to(x.dtype)
        abi.encoder_infer_ex(b, n, heads, ff, table, not bn, stream, dtype=l0.storage_dtype, **ptrs)
    return y, concat, attn
