"""One optimisation step of the FeTA models, per task family, as the reference's training scripts
do it - the direct caller of the hot path.

    task      loss                                     optimiser                    reference
    'zinc'    L1                                       Adam(lr), warm-up schedule   experiments/run_transformer_gengcn.py:115-164,301-317
    'tu'      CrossEntropy (BCE-with-logits if 1 out)  AdamW(lr, wd=1e-4), StepLR   experiments/run_transformer_gengcn_cv.py:123-193,356-362
    'molhiv'  BCE-with-logits on non-NaN labels        AdamW                        experiments/run_transformer_gengcn_molhiv.py:136-222
    'sbm'     CrossEntropy over real nodes             AdamW                        experiments/run_transformer_gengcn_SBM_cv.py:145-218,367-373

What is not reproduced: the per-step NaN / |param|>1000 scans that drop into pdb
(run_transformer_gengcn_cv.py:161-179), the host timers and prints, the `.cuda()` copies (the
collate already emits device tensors), dataset download and CSV logging.

``GraphedTrainStep`` is the MI355X form of the loop body: forward, loss, backward and the optimiser
update captured once per padded size into a hipGraph and replayed - the reference pays ~10^3 kernel
launches and a host sync (`.cpu()` at transformer/models.py:246) per step.  ``StoreTrainStep`` feeds it from a
device-resident split, and ``StoreEvaluator`` / ``StoreEvalStep`` are the eval_epoch of the graph-level tasks in the
same form: one captured forward-only graph per bucket, one host read per split (``evaluate`` is the eager form).
``fused_head=True`` (task_loss, train_step, GraphedTrainStep, StoreTrainStep; default off) runs pooling, classifier, loss and
their backward of a graph-level shell as the four launches of ``functional.readout_train``.
"""
import torch
from torch import nn
import torch.nn.functional as F


def warmup_lr(step, lr, warmup):
    """experiments/run_transformer_gengcn.py:310-317."""
    if step < warmup:
        return 1e-6 + step * (lr - 1e-6) / warmup
    return lr * warmup ** 0.5 * step ** -0.5


def lap_signs(lap_dim, generator=None):
    """[lap_dim] float32 of +1 / -1 on the host: one draw of the reference's per-batch sign flip."""
    flip = torch.rand(lap_dim, generator=generator)
    return torch.where(flip >= 0.5, torch.ones_like(flip), -torch.ones_like(flip))


def lap_sign_flip(lap_pe, generator=None):
    """Random sign per Laplacian-PE column, one draw per batch
    (experiments/run_transformer_gengcn.py:126-131)."""
    flip = lap_signs(lap_pe.shape[-1], generator)
    return lap_pe * flip.to(lap_pe.device).unsqueeze(0)


def make_criterion(task, nb_class=1):
    if task == 'zinc':
        return nn.L1Loss()
    if task in ('tu', 'sbm'):
        return nn.BCEWithLogitsLoss() if nb_class == 1 else nn.CrossEntropyLoss()
    if task == 'molhiv':
        return nn.BCEWithLogitsLoss()
    raise ValueError('unknown task %r' % (task,))


def make_optimizer(task, params, lr, weight_decay=1e-4, capturable=False, fused=None):
    """Adam for ZINC (run_transformer_gengcn.py:302), AdamW elsewhere (..._cv.py:360).
    fused (default: with capturable, on the GPU): PyTorch's single-kernel multi-tensor update instead of
    its ~10 foreach kernels per step - the same arithmetic per element."""
    params = [p for p in params if p.requires_grad]
    if fused is None:
        fused = bool(capturable) and all(p.is_cuda for p in params)
    kw = dict(lr=lr, capturable=capturable)
    if fused:
        kw['fused'] = True
    if task == 'zinc':
        return torch.optim.Adam(params, **kw)
    return torch.optim.AdamW(params, weight_decay=weight_decay, **kw)


def pad_node_labels(labels, feature_indices, bsz, n_pad):
    """[N_tot] node labels (graph-major, transformer/data.py:456) -> [B, N_pad] with -100 on the
    padded positions (the ignore_index of cross_entropy)."""
    out = torch.full((bsz, n_pad), -100, dtype=torch.int64, device=labels.device)
    out[feature_indices[:, 0], feature_indices[:, 1]] = labels
    return out


def task_loss(task, model, criterion, batch9, graph_cache=None, padded_node_labels=False, fused_head=False, count=None):
    """forward + loss of one collated batch; returns (loss, model output).
    padded_node_labels ('sbm'): labels are [B, N_pad] from pad_node_labels and the model returns the
    logits of every position - the same mean over the real nodes as the reference's boolean gather
    (transformer/models.py:1070-1071) with static shapes and no host sync.
    fused_head: the body is ``model.encoder_rows`` and ``functional.readout_train`` - pooling, classifier and loss in two
    launches, their backward in two - for what ``_fused_head_plan`` accepts (ValueError otherwise).  The second result is then
    the scores [B, C] of the readout on EVERY task, without a gradient.  On the default path it is whatever the shell returns:
    [B, C] from the 'zinc' / 'tu' shell ([B, 1] for one output) and the SQUEEZED logits [B] (0-d for B = 1) from the molhiv
    shell, which returns ``cls_out.squeeze()``.
    count (fused_head only): int32 device tensor of one element, the number of leading slots that count for the loss and get
    a gradient (StoreTrainStep's padded batches); default: all B."""
    x, mask, pe, lap_pe, degree, labels, edge_index, batch, feature_indices = batch9
    if fused_head:
        from . import functional as FF
        from .transformer.layers import n_real_from_mask
        kind, slope = _fused_head_plan(task, model, criterion)
        rows, _ = model.encoder_rows(x, edge_index, batch, feature_indices, mask, pe, lap_pe, degree, graph_cache=graph_cache)
        n_real = graph_cache.n_real if graph_cache is not None and graph_cache.n_real is not None else n_real_from_mask(mask)
        if count is None:
            count = torch.full((1,), x.shape[0], dtype=torch.int32, device=x.device)
        labels = labels.reshape(-1)
        if labels.dtype != torch.int64:
            labels = labels.float()
        head = model.classifier
        return FF.readout_train(rows, n_real, count, labels.contiguous(), head[0].weight, head[0].bias, head[2].weight,
                                head[2].bias, kind, slope)
    extra = {'padded_logits': True} if padded_node_labels else {}
    res = model(x, edge_index, batch, feature_indices, mask, pe, lap_pe, degree,
                graph_cache=graph_cache, **extra)
    output = res[0]
    if padded_node_labels:
        if not isinstance(criterion, nn.CrossEntropyLoss):
            raise ValueError('padded node labels need a CrossEntropyLoss criterion')
        return F.cross_entropy(output.reshape(-1, output.shape[-1]), labels.reshape(-1),
                               weight=criterion.weight, ignore_index=-100), output
    if task == 'zinc':
        labels = labels.view(output.shape)          # default_collate of g.y [1] gives [B, 1]
        return criterion(output, labels), output
    if task == 'molhiv':
        labels = labels.view(-1)
        # BCE over the labeled graphs (run_transformer_gengcn_molhiv.py:177-178) without the
        # boolean gather (a host sync): NaN labels get weight 0, the mean runs over the others
        keep = ~torch.isnan(labels)
        tgt = torch.where(keep, labels, torch.zeros_like(labels)).to(output.dtype)
        w = keep.to(output.dtype)
        per = F.binary_cross_entropy_with_logits(output.view(-1), tgt, reduction='none')
        return (per * w).sum() / w.sum(), output
    labels = labels.view(-1)
    if isinstance(criterion, nn.BCEWithLogitsLoss):
        return criterion(output.view(-1), labels.to(output.dtype)), output
    return criterion(output, labels), output


def train_step(task, model, criterion, optimizer, batch9, graph_cache=None, lr=None, padded_node_labels=False,
               fused_head=False):
    """One iteration of the reference's train_epoch loop body.  -> loss (0-d tensor, no sync).
    padded_node_labels: as task_loss (batches of transformer.store.DeviceGraphStore.batch carry node labels padded).
    fused_head: as task_loss (pooling, classifier, loss and their backward in functional.readout_train)."""
    if lr is not None:
        for group in optimizer.param_groups:
            group['lr'] = lr
    optimizer.zero_grad(set_to_none=True)
    loss, _ = task_loss(task, model, criterion, batch9, graph_cache, padded_node_labels=padded_node_labels,
                        fused_head=fused_head)
    loss.backward()
    optimizer.step()
    from .functional import DropoutState
    if DropoutState.device_mode():
        DropoutState.end_step()      # (an eager step between graph replays: the shared device offset moves past its masks)
    return loss.detach()


def accuracy_SBM(scores, targets, nb_class=None):
    """experiments/run_transformer_gengcn_SBM_cv.py:126-143: mean per-class recall in percent.
    Classes are 0..max(label, prediction) as sklearn's confusion_matrix would order them (or
    nb_class when given); computed on the device, one host read at the end."""
    pred = scores.argmax(dim=1)
    if nb_class is None:
        nb_class = int(max(int(targets.max()), int(pred.max())) + 1)
    size = torch.bincount(targets, minlength=nb_class).to(torch.float64)
    hit = torch.bincount(targets[pred == targets], minlength=nb_class).to(torch.float64)
    recall = torch.where(size > 0, hit / size.clamp(min=1), torch.zeros_like(size))
    return float(100.0 * recall.sum() / nb_class)


def prepare_cache(model, batch9, graph_cache=None):
    """Graph structure in kernel layout, built outside any hipGraph: node counts / offsets from the
    mask and, for filter_mode='cheb', the dense scaled Laplacian from the edge list (the edge list
    has a different length in every batch, so it cannot be an input of a captured graph)."""
    x, mask, edge_index, batch = batch9[0], batch9[1], batch9[6], batch9[7]
    return model.encoder._graph_cache(graph_cache, edge_index, batch, mask, x.shape[1])


class GraphedTrainStep:
    """forward + loss + backward + optimiser update of one padded batch shape, captured into ONE
    hipGraph.  The fixed-shape batch tensors are copied into static buffers, so every batch
    replayed through one instance must have the [B, N_pad] of the example (one instance per bucket
    of ``data.bucket_batches``); the variable-length members of the tuple (edge_index, batch,
    feature_indices) are consumed before the graph by ``prepare_cache`` / ``pad_node_labels``.
    The learning rate lives in a device scalar (capturable optimiser), so the warm-up schedule does
    not re-capture.

    Construction does not advance training: the warm-up iterations and the capture run REAL steps on
    the example batch, so the parameters, the module buffers (BatchNorm running statistics,
    num_batches_tracked) and the optimiser state (moments and step counters) are snapshotted before
    and restored, in place, afterwards - an instance created mid-training (one per padded-size bucket)
    leaves the trajectory exactly where the reference loop would have it.

    fused_head: the step's head is functional.readout_train (task_loss); ValueError at construction for what
    ``_fused_head_plan`` refuses."""

    def __init__(self, task, model, criterion, optimizer, batch9, graph_cache=None, warmup_iters=3, fused_head=False):
        self.task, self.model, self.criterion, self.optimizer = task, model, criterion, optimizer
        self.fused_head, self.count = bool(fused_head), None
        if fused_head:
            _fused_head_plan(task, model, criterion)
            self.count = torch.full((1,), batch9[0].shape[0], dtype=torch.int32, device=batch9[0].device)
        for group in optimizer.param_groups:
            if not group.get('capturable', False):
                raise ValueError('GraphedTrainStep needs make_optimizer(..., capturable=True)')
            if not torch.is_tensor(group['lr']):
                group['lr'] = torch.tensor(float(group['lr']), device=batch9[0].device)
        clone = lambda t: None if t is None else t.clone()
        graph_cache = prepare_cache(model, batch9, graph_cache)
        self.static = tuple(clone(t) for t in self._fixed(batch9))
        self.cache = type(graph_cache)(clone(graph_cache.n_real), clone(graph_cache.node_off),
                                       graph_cache.n_pad, clone(graph_cache.u),
                                       clone(graph_cache.lam), clone(graph_cache.lhat),
                                       {k: (v.clone() if torch.is_tensor(v) else v)
                                        for k, v in graph_cache.extra.items()})
        # attention-probability dropout inside the graph: the (seed, offset) key moves to the device, every replay
        # reads it there and advances it (functional.DropoutState) - the masks of replay i are those of eager step i
        from .functional import DropoutState
        DropoutState.begin_device_mode(batch9[0].device)
        snap = self._snapshot()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup_iters):
                self._body()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = self._body()
        self._restore(snap)

    def _snapshot(self):
        """Copies of everything a step mutates; optimiser state that does not exist yet (lazily created
        by the first step) is recorded as absent and zeroed on restore."""
        tensors = list(self.model.parameters()) + list(self.model.buffers())
        opt = {}
        for p, st in self.optimizer.state.items():
            opt[p] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()}
        # ... and the random streams the warm-up steps draw from: torch's generators (nn.Dropout) and the
        # (seed, offset) of the attention-probability dropout masks
        from .functional import DropoutState
        dev = tensors[0].device if tensors else None
        rng = (torch.get_rng_state(), torch.cuda.get_rng_state(dev) if (dev is not None and dev.type == 'cuda') else None,
               DropoutState.snapshot())
        return [t.detach().clone() for t in tensors], opt, rng

    @torch.no_grad()
    def _restore(self, snap):
        """In place: the captured graph holds the addresses of these tensors."""
        saved, opt, rng = snap
        tensors = list(self.model.parameters()) + list(self.model.buffers())
        for t, s in zip(tensors, saved):
            t.copy_(s)
        from .functional import DropoutState
        torch.set_rng_state(rng[0])
        if rng[1] is not None:
            torch.cuda.set_rng_state(rng[1], tensors[0].device)
        DropoutState.restore(rng[2])
        for p, st in self.optimizer.state.items():
            before = opt.get(p)
            for k, v in st.items():
                if torch.is_tensor(v):
                    if before is not None and k in before:
                        v.copy_(before[k])
                    else:
                        v.zero_()
                elif before is not None and k in before:
                    st[k] = before[k]

    def _fixed(self, batch9):
        x, mask, pe, lap_pe, degree, labels, edge_index, batch, feature_indices = batch9
        if self.task == 'sbm':
            labels = pad_node_labels(labels, feature_indices, x.shape[0], x.shape[1])
        return (x, mask, pe, lap_pe, degree, labels, None, None, None)

    def _body(self):
        self.optimizer.zero_grad(set_to_none=True)
        loss, _ = task_loss(self.task, self.model, self.criterion, self.static, self.cache,
                            padded_node_labels=self.task == 'sbm', fused_head=self.fused_head, count=self.count)
        loss.backward()
        self.optimizer.step()
        from .functional import DropoutState
        self.drop_calls = DropoutState.end_step()     # (in-graph: the device offset moves past this step's masks)
        return loss.detach()

    def set_lr(self, lr):
        for group in self.optimizer.param_groups:
            group['lr'].fill_(lr)

    def __call__(self, batch9, graph_cache=None):
        graph_cache = prepare_cache(self.model, batch9, graph_cache)
        for dst, src in zip(self.static, self._fixed(batch9)):
            if dst is not None:
                dst.copy_(src, non_blocking=True)
        for name in ('n_real', 'node_off', 'u', 'lam', 'lhat'):
            dst, src = getattr(self.cache, name), getattr(graph_cache, name)
            if dst is not None and src is not None:
                dst.copy_(src, non_blocking=True)
        for key, dst in self.cache.extra.items():   # e.g. the per-row degree scale of this batch
            if torch.is_tensor(dst):
                dst.copy_(graph_cache.extra[key], non_blocking=True)
        self.graph.replay()
        if self.drop_calls:
            from .functional import DropoutState
            DropoutState.replayed(self.drop_calls)
        return self.loss


class StoreTrainStep(GraphedTrainStep):
    """GraphedTrainStep fed from a ``transformer.store.DeviceGraphStore``: the captured hipGraph begins with the ONE
    feta_batch_gather launch that builds the padded batch from ``batch_size`` graph ids in a static device buffer, then
    runs forward, loss, backward and the optimiser update.  A step is ``step(ids)``: a host sequence costs one copy of
    4 * batch_size bytes, a device int32 tensor (a slice of a device-side permutation) no host data at all; nothing
    else is fed - no collate, no eigendecomposition, no copies into static buffers.

    One instance per (bucket n_pad, batch_size); the same snapshot / restore contract, set_lr and DropoutState device
    mode as GraphedTrainStep (construction does not advance training: the warm-up and capture steps run on
    ``example_ids``, default the first graphs of the bucket).  Without ``fused_head`` (below) only FULL batches go through the
    captured step: the ragged last batch of a bucket goes through ``store.batch(ids)`` and
    ``train_step(..., padded_node_labels=task == 'sbm')``.
    filter_mode='spectral' reads the store's u / lam, filter_mode='cheb' its lhat (``DeviceGraphStore(..., lhat=True)``;
    the gather launch is then feta_batch_gather_ex), with either setting of heads_share_graph.
    lap_sign_flip: the reference's random sign per Laplacian-PE column (lap_sign_flip above), drawn on the host for every
    ``step(ids)`` with ``lap_signs(lap_dim, generator)`` and applied by the gather launch inside the hipGraph: one more
    host-to-device copy of 4 * lap_dim bytes per step.  Warm-up and capture run with signs of +1 and draw nothing.
    dtype: storage type of x and pe as the gather emits them; the task shells embed fp32 x, so they keep float32 (a
    bf16-storage model rounds its rows and pe itself) and torch.bfloat16 is for a model that consumes bf16 x directly.

    fused_head: the head of the captured step is functional.readout_train (task_loss), which reads the number of live slots
    on the device, so ``step(ids)`` also takes a RAGGED batch, 1 <= len(ids) <= batch_size (host sequence or device tensor),
    as StoreEvalStep does: the static id buffer holds batch_size + 1 int32, the ids and behind them the count; a short batch
    is padded with ids[0], and host ids and count travel in the one pinned copy.  The padded slots run through the encoder,
    count for nothing in the loss and get a zero gradient, and every gradient is linear in the readout's: the step equals
    an eager step on the short batch up to summation order.  NOT with a BatchNorm module in training mode, whose batch
    statistics would see the repeated graph: such a model keeps the ValueError for a short batch."""

    def __init__(self, task, model, criterion, optimizer, store, n_pad, batch_size, dtype=torch.float32,
                 example_ids=None, warmup_iters=3, lap_sign_flip=False, generator=None, fused_head=False):
        from .transformer.store import GatherBuffers
        self.task, self.model, self.criterion, self.optimizer = task, model, criterion, optimizer
        self.fused_head, self.count = bool(fused_head), None
        if fused_head:
            _fused_head_plan(task, model, criterion)
        mode = getattr(model.encoder, 'filter_mode', 'spectral')
        if mode not in ('spectral', 'cheb'):
            raise ValueError("StoreTrainStep runs filter_mode='spectral' and 'cheb' models, got %r" % (mode,))
        if mode == 'cheb' and store.lhat is None:
            raise ValueError("a filter_mode='cheb' model needs the store's Laplacians: DeviceGraphStore(..., lhat=True)")
        if lap_sign_flip and store.lap is None:
            raise ValueError('lap_sign_flip needs a store with lap_dim')
        self.store, self.generator = store, generator
        for group in optimizer.param_groups:
            if not group.get('capturable', False):
                raise ValueError('StoreTrainStep needs make_optimizer(..., capturable=True)')
            if not torch.is_tensor(group['lr']):
                group['lr'] = torch.tensor(float(group['lr']), device=store.device)
        self.bufs = GatherBuffers(store, batch_size, n_pad, dtype, lhat=mode == 'cheb', lap_sign=bool(lap_sign_flip))
        self.ids = self.bufs.ids
        if fused_head:      # one static buffer: the gather reads its front, the readout the count behind it
            self.ids = torch.zeros((self.bufs.bsz + 1,), dtype=torch.int32, device=store.device)
            self.bufs.ids, self.count = self.ids[:self.bufs.bsz], self.ids[self.bufs.bsz:]
        self._pinned, self._copied, self._turn = [None, None], [None, None], 0
        if example_ids is None:
            members = store.bucket_ids(n_pad)
            if len(members) == 0:
                raise ValueError('no graph of the store is padded to %d' % n_pad)
            example_ids = [int(members[i % len(members)]) for i in range(batch_size)]
        self._set_ids(example_ids)
        self.static, self.cache = self.bufs.batch9(), self.bufs.cache()
        # warm-up and capture as GraphedTrainStep does them (device-resident dropout key, snapshot before, restore after)
        from .functional import DropoutState
        DropoutState.begin_device_mode(store.device)
        snap = self._snapshot()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup_iters):
                self._body()
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = self._body()
        self._restore(snap)

    def _set_ids(self, ids, signs=None):
        import numpy as np
        ids = self.store.device_ids(ids) if torch.is_tensor(ids) else np.asarray(ids, np.int32)
        bsz = self.bufs.bsz
        if tuple(ids.shape) != (bsz,):
            if not self.fused_head:
                raise ValueError('this step was captured for exactly %d ids, got %s (a ragged batch goes through '
                                 'store.batch and train_step)' % (bsz, tuple(ids.shape)))
            if ids.ndim != 1 or not 1 <= ids.shape[0] <= bsz:
                raise ValueError('this step takes 1 to %d ids, got %s' % (bsz, tuple(ids.shape)))
            if any(isinstance(m, nn.modules.batchnorm._BatchNorm) and m.training for m in self.model.modules()):
                raise ValueError('this step was captured for exactly %d ids, got %s: a short batch is padded with ids[0], and '
                                 'the batch statistics of a BatchNorm module in training mode would see the repeated graph '
                                 '(a ragged batch goes through store.batch and train_step)' % (bsz, tuple(ids.shape)))
        k = ids.shape[0]
        if torch.is_tensor(ids):
            self.bufs.ids[:k].copy_(ids, non_blocking=True)
            if self.fused_head:     # (device operands only: nothing waits for the host)
                if k < bsz:
                    self.bufs.ids[k:].copy_(ids[:1].expand(bsz - k), non_blocking=True)
                self.count.fill_(k)
            if signs is None:
                return
        # one asynchronous host-to-device copy per host operand (the ids, the signs), straight into the static buffer,
        # out of one of two pinned buffer sets used alternately (BatchStager's scheme: a set is refilled only after the
        # copies enqueued from it have been read)
        turn = self._turn
        self._turn ^= 1
        if self._pinned[turn] is None:
            sign_buf = None if self.bufs.lap_sign is None else torch.empty(self.bufs.lap_sign.shape, pin_memory=True)
            self._pinned[turn] = (torch.empty(self.ids.numel(), dtype=torch.int32, pin_memory=True), sign_buf)
            self._copied[turn] = torch.cuda.Event()
        else:
            self._copied[turn].synchronize()
        id_buf, sign_buf = self._pinned[turn]
        if not torch.is_tensor(ids):
            host = id_buf.numpy()
            host[:k] = ids
            if self.fused_head:
                host[k:bsz] = ids[0]
                host[bsz] = k
            self.ids.copy_(id_buf, non_blocking=True)
        if signs is not None:
            sign_buf.copy_(signs)
            self.bufs.lap_sign.copy_(sign_buf, non_blocking=True)
        self._copied[turn].record()

    def _body(self):
        self.store.gather_into(self.bufs)
        return super()._body()

    def __call__(self, ids):
        sign = self.bufs.lap_sign
        self._set_ids(ids, None if sign is None else lap_signs(sign.shape[0], self.generator))
        self.graph.replay()
        if self.drop_calls:
            from .functional import DropoutState
            DropoutState.replayed(self.drop_calls)
        return self.loss


def rocauc(scores, labels):
    """Binary ROC-AUC over the labeled graphs (what ogb's Evaluator('ogbg-molhiv') reports,
    experiments/run_transformer_gengcn_molhiv.py:213-218): rank statistic with ties averaged."""
    keep = ~torch.isnan(labels)
    s, y = scores[keep].double().cpu(), labels[keep].double().cpu()
    pos, neg = int((y > 0.5).sum()), int((y <= 0.5).sum())
    if pos == 0 or neg == 0:
        return float('nan')
    order = torch.argsort(s)
    ranks = torch.empty_like(s)
    ranks[order] = torch.arange(1, len(s) + 1, dtype=torch.float64)
    vals, inv, counts = torch.unique(s, return_inverse=True, return_counts=True)
    sums = torch.zeros_like(vals).scatter_add_(0, inv, ranks)
    ranks = (sums / counts)[inv]                        # average rank of tied scores
    return float((ranks[y > 0.5].sum() - pos * (pos + 1) / 2.0) / (pos * neg))


def evaluate(task, model, criterion, batches, inference_mode=False):
    """The reference's eval_epoch for one split: ``batches`` yields (batch9, graph_cache).  Returns a dict:
    'loss' (sample-weighted mean, as running_loss / n_sample) plus 'mae' and 'mse' (zinc,
    run_transformer_gengcn.py:167-209), 'acc' (tu: fraction of graphs; sbm: mean per-class recall in
    percent averaged over batches, ..._SBM_cv.py:221-266) or 'rocauc' (molhiv).  The model is put in eval
    mode (BatchNorm running statistics) and restored.  Runs under torch.no_grad(), or under
    torch.inference_mode() with inference_mode=True: the encoder stack is then ONE forward-only launch where its
    shape allows (fused_stack.encoder_stack_infer)."""
    with torch.inference_mode() if inference_mode else torch.no_grad():
        return _evaluate(task, model, criterion, batches)


def _evaluate(task, model, criterion, batches):
    was_training = model.training
    model.eval()
    tot = {'loss': 0.0, 'mae': 0.0, 'mse': 0.0, 'hit': 0.0, 'acc_sum': 0.0}
    n_sample, n_batch = 0, 0
    scores, labels_all = [], []
    for batch9, cache in batches:
        loss, out = task_loss(task, model, criterion, batch9, cache)
        labels = batch9[5]
        bsz = batch9[0].shape[0]
        tot['loss'] += float(loss) * bsz
        n_sample += bsz
        n_batch += 1
        if task == 'zinc':
            lab = labels.view(out.shape)
            tot['mae'] += float(F.l1_loss(out, lab)) * bsz
            tot['mse'] += float(F.mse_loss(out, lab)) * bsz
        elif task == 'tu':
            pred = out.argmax(dim=1) if out.dim() == 2 and out.shape[1] > 1 else (out.view(-1) > 0).long()
            tot['hit'] += float((pred == labels.view(-1)).sum())
        elif task == 'sbm':
            tot['acc_sum'] += accuracy_SBM(out, labels.view(-1))
        elif task == 'molhiv':
            scores.append(out.view(-1).detach())
            labels_all.append(labels.view(-1))
    model.train(was_training)
    res = {'loss': tot['loss'] / max(n_sample, 1)}
    if task == 'zinc':
        res.update(mae=tot['mae'] / n_sample, mse=tot['mse'] / n_sample)
    elif task == 'tu':
        res['acc'] = tot['hit'] / n_sample
    elif task == 'sbm':
        res['acc'] = tot['acc_sum'] / max(n_batch, 1)
    elif task == 'molhiv':
        res['rocauc'] = rocauc(torch.cat(scores), torch.cat(labels_all))
    return res


_USE_EAGER = 'run it through store.batch and train.evaluate'


_USE_PLAIN_HEAD = 'run it with fused_head=False'


def _head_plan(task, model, criterion, instead):
    """-> (loss_kind of functional.readout_eval / readout_train, slope of the classifier's activation, d_model, nb_class) of a
    graph-level shell and its criterion: the part of _readout_plan and _fused_head_plan that looks at the model and the
    criterion only.  ValueError, ending with ``instead`` (the path to take), for what the readout kernels do not compute."""
    if task == 'sbm':
        raise ValueError("task 'sbm' has node-level logits and a per-batch confusion-matrix accuracy: " + instead)
    if task not in ('zinc', 'tu', 'molhiv'):
        raise ValueError('unknown task %r' % (task,))
    head = getattr(model, 'classifier', None)
    if (not hasattr(model, 'encoder_rows') or not isinstance(head, nn.Sequential) or len(head) != 3
            or not isinstance(head[0], nn.Linear) or not isinstance(head[2], nn.Linear)):
        raise ValueError('the model is not a graph-level shell with a Linear - activation - Linear classifier: ' + instead)
    if isinstance(head[1], nn.ReLU):
        slope = 0.0
    elif isinstance(head[1], nn.LeakyReLU):
        slope = float(head[1].negative_slope)        # (nn.LeakyReLU(True) of the molhiv shell: 1.0, the identity)
    else:
        raise ValueError('classifier activation %s: ReLU or LeakyReLU only; %s' % (type(head[1]).__name__, instead))
    d, c = head[0].in_features, head[2].out_features
    kind = 'l1' if task == 'zinc' else 'bce_logits' if (task == 'molhiv' or c == 1) else 'ce'
    if criterion is not None and task != 'molhiv':       # (task_loss does not read the criterion of 'molhiv')
        want = {'l1': nn.L1Loss, 'bce_logits': nn.BCEWithLogitsLoss, 'ce': nn.CrossEntropyLoss}[kind]
        if not isinstance(criterion, want):
            raise ValueError('task %r with %d outputs is evaluated with %s, got %s: %s'
                             % (task, c, want.__name__, type(criterion).__name__, instead))
        if (getattr(criterion, 'weight', None) is not None or getattr(criterion, 'pos_weight', None) is not None
                or getattr(criterion, 'label_smoothing', 0.0) != 0.0):
            raise ValueError('a criterion with class weights or label smoothing: ' + instead)
        if criterion.reduction != 'mean':
            raise ValueError("a criterion with reduction %r (the evaluation averages per batch: 'mean'): %s"
                             % (criterion.reduction, instead))
    return kind, slope, d, c


def _fused_head_plan(task, model, criterion):
    """-> (loss_kind, slope) of functional.readout_train for a graph-level shell that task_loss(..., fused_head=True) can run:
    a Linear - ReLU / LeakyReLU - Linear classifier with d_model = 64 and at most 64 outputs under the task's own loss with
    reduction 'mean', no class weights, pos_weight or label smoothing; ValueError otherwise."""
    kind, slope, d, c = _head_plan(task, model, criterion, _USE_PLAIN_HEAD)
    from . import _lib
    if not _lib.backend(model.classifier[0].weight)[0].readout_train_supported(d, c):
        raise ValueError('feta_readout_train has d_model = 64 and at most 64 outputs, the classifier has %d and %d: %s'
                         % (d, c, _USE_PLAIN_HEAD))
    return kind, slope


def _readout_plan(task, model, criterion, store):
    """-> (loss_kind of functional.readout_eval, slope of the classifier's activation, d_model, nb_class, filter_mode) of a
    graph-level shell whose evaluation a StoreEvalStep on ``store`` can run; ValueError where it cannot (everything that
    does not depend on the padded size)."""
    kind, slope, d, c = _head_plan(task, model, criterion, _USE_EAGER)
    from . import _lib
    if not _lib.backend(store.x)[0].readout_eval_supported(d, c):
        raise ValueError('feta_readout_eval has d_model = 64 and at most 64 outputs, the classifier has %d and %d: %s'
                         % (d, c, _USE_EAGER))
    mode = getattr(model.encoder, 'filter_mode', None)
    if mode not in ('spectral', 'cheb'):
        raise ValueError('StoreEvalStep runs the FeTA encoder (filter_mode spectral or cheb): ' + _USE_EAGER)
    if mode == 'cheb' and store.lhat is None:
        raise ValueError("a filter_mode='cheb' model needs the store's Laplacians, DeviceGraphStore(..., lhat=True); or "
                         + _USE_EAGER)
    if mode == 'spectral' and store.u is None:
        raise ValueError("a filter_mode='spectral' model needs the store's eigenpairs, DeviceGraphStore(..., k_eig=...)")
    if store.node_labels:
        raise ValueError('a store of node labels: ' + _USE_EAGER)
    return kind, slope, d, c, mode


class StoreEvalStep:
    """The evaluation of one padded batch of a ``transformer.store.DeviceGraphStore`` as ONE captured hipGraph, under
    ``torch.inference_mode()`` with the model in ``eval()``: feta_batch_gather -> embedding (+ embedding_lap_pos_enc, no
    sign flip) -> the encoder (the one-launch stack feta_encoder_infer[_ex] and the filter stage) -> feta_readout_eval,
    which leaves the logits of every graph in ``scores`` [G, C] and its loss / metric terms in ``terms`` [G, 4], both
    indexed by the graph's id in the store.  One instance per (bucket n_pad, batch_size); nothing is mutated, so
    construction needs no snapshot, and ``model.training`` is what it was afterwards.

    ``step(ids)``: 1 <= len(ids) <= batch_size host ids.  The static id buffer holds batch_size + 1 int32: the gather's
    ids and, behind them, the number of live slots, which the readout reads on the device.  A short batch is padded with
    ids[0]: the padded slots hold a real graph, so no kernel meets an empty graph, and the readout skips them.  All of it
    travels in one asynchronous copy out of alternating pinned buffers; a step does not wait for the device.

    The hipGraph holds the ADDRESSES of the parameters and of the BatchNorm running statistics; the optimiser and the
    training BatchNorm update them in place, so a step captured once reports the current model.

    ValueError (the path to use instead is store.batch + train.evaluate): task 'sbm'; a stack that
    fused_stack.infer_supported refuses at this n_pad (N_pad > 64, ...); a classifier feta_readout_eval_supported
    refuses; a criterion with class weights or another reduction than 'mean'; a filter_mode='cheb' model on a store
    without lhat.  On a CPU store - the host emulation of the tests - nothing is captured and a step runs its body."""

    def __init__(self, task, model, store, n_pad, batch_size, scores, terms, dtype=torch.float32, criterion=None,
                 warmup_iters=3):
        from .fused_stack import infer_supported
        from .transformer.store import GatherBuffers
        self.task, self.model, self.store = task, model, store
        self.loss_kind, self.slope, d, c, mode = _readout_plan(task, model, criterion, store)
        enc = model.encoder
        if tuple(scores.shape) != (store.num_graphs, c) or tuple(terms.shape) != (store.num_graphs, 4):
            raise ValueError('scores [%d, %d] and terms [%d, 4], got %s and %s'
                             % (store.num_graphs, c, store.num_graphs, tuple(scores.shape), tuple(terms.shape)))
        head = model.classifier
        self.weights = tuple(None if p is None else p.detach() for p in (head[0].weight, head[0].bias, head[2].weight, head[2].bias))
        if not all(p is None or p.is_contiguous() for p in self.weights):
            raise ValueError('the classifier parameters must be contiguous (they are read in place)')
        self.bsz, self.scores, self.terms = int(batch_size), scores, terms
        self.bufs = GatherBuffers(store, self.bsz, n_pad, dtype, lhat=mode == 'cheb')
        self.ids = torch.zeros((self.bsz + 1,), dtype=torch.int32, device=store.device)
        self.bufs.ids = self.ids[:self.bsz]          # the gather reads the front of the step's one static id buffer
        self.cache = self.bufs.cache()
        self._pinned, self._copied, self._turn = [None, None], [None, None], 0
        self.graph = None
        was_training = model.training
        model.eval()
        try:
            if not (getattr(enc, 'fused_stack', False) and enc.last_layer_filter
                    and enc.layers[0].storage_dtype == enc.storage_dtype and infer_supported(enc.layers, int(n_pad), d)):
                raise ValueError('the encoder stack has no one-launch inference form at N_pad = %d (d_model = 64, 4 or 8 '
                                 'heads, N_pad <= 64, ...): %s' % (n_pad, _USE_EAGER))
            members = store.bucket_ids(n_pad)
            if len(members) == 0:
                raise ValueError('no graph of the store is padded to %d' % n_pad)
            if store.device.type == 'cuda':
                self._send(members[:self.bsz])
                with torch.inference_mode():
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        for _ in range(warmup_iters):
                            self._body()
                    torch.cuda.current_stream().wait_stream(side)
                    self.graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.graph):
                        self._body()
        finally:
            model.train(was_training)

    def _send(self, ids):
        import numpy as np
        ids = np.asarray(ids, np.int32).reshape(-1)
        k = len(ids)
        if not 1 <= k <= self.bsz:
            raise ValueError('this step takes 1 to %d ids, got %d (StoreEvaluator cuts a split into batches)' % (self.bsz, k))
        if self.store.device.type != 'cuda':
            host = self.ids.numpy()
        else:
            # one asynchronous copy of the ids AND the count out of one of two pinned buffers used alternately
            # (StoreTrainStep._set_ids: a buffer is refilled only after the copy enqueued from it has been read)
            turn = self._turn
            self._turn ^= 1
            if self._pinned[turn] is None:
                self._pinned[turn] = torch.empty(self.bsz + 1, dtype=torch.int32, pin_memory=True)
                self._copied[turn] = torch.cuda.Event()
            else:
                self._copied[turn].synchronize()
            host = self._pinned[turn].numpy()
        host[:k] = ids
        host[k:self.bsz] = ids[0]
        host[self.bsz] = k
        if self.store.device.type == 'cuda':
            self.ids.copy_(self._pinned[turn], non_blocking=True)
            self._copied[turn].record()

    def _body(self):
        from . import functional as FF
        bufs = self.store.gather_into(self.bufs)
        rows, _ = self.model.encoder_rows(bufs.x, None, None, None, bufs.mask, bufs.pe, bufs.lap, bufs.degree,
                                          graph_cache=self.cache)
        w1, b1, w2, b2 = self.weights
        FF.readout_eval(rows, bufs.n_real, self.ids, self.ids[self.bsz:], bufs.labels, w1, b1, w2, b2, self.scores,
                        self.terms, self.loss_kind, self.slope)

    def __call__(self, ids):
        self._send(ids)
        if self.graph is not None:
            self.graph.replay()
            return
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.inference_mode():
                self._body()
        finally:
            self.model.train(was_training)

    step = __call__


class StoreEvaluator:
    """The reference's eval_epoch of a whole split out of a ``DeviceGraphStore``: one ``StoreEvalStep`` per bucket (built
    on first use), one small copy and one replay per batch - ragged tails included -, ONE device read per call.
    ``evaluate(ids=None)`` walks ``store.epoch(batch_size)`` - with ``ids`` only those graphs, in the same order - and
    returns the dict ``evaluate`` (below the training steps) returns for the same cut into batches (``batches(ids)``):
    'loss' is the sample-weighted mean of the per-batch means ('molhiv': a batch's mean runs over its labelled graphs), plus
    'mae' and 'mse' (zinc), 'acc' (tu) or 'rocauc' (molhiv, ``rocauc`` on the [G] scores and the store's labels).  The
    reductions run on the host in fp64 over the per-graph rows of ``terms``; ``scores`` [G, C] and ``terms`` [G, 4] stay on the
    device, indexed by graph id.  Raises what StoreEvalStep raises, the task and criterion checks at construction."""

    def __init__(self, task, model, criterion, store, batch_size, dtype=torch.float32):
        self.task, self.model, self.criterion, self.store = task, model, criterion, store
        self.batch_size, self.dtype = int(batch_size), dtype
        c = _readout_plan(task, model, criterion, store)[3]
        self.scores = torch.zeros((store.num_graphs, c), dtype=torch.float32, device=store.device)
        self.terms = torch.zeros((store.num_graphs, 4), dtype=torch.float32, device=store.device)
        self.labels = store.y.detach().cpu()        # (read once: what rocauc ranks the scores against)
        self.steps = {}

    def batches(self, ids=None):
        """-> [(n_pad, ids int32)]: store.epoch(batch_size), restricted to ``ids`` when given"""
        import numpy as np
        if ids is None:
            return list(self.store.epoch(self.batch_size))
        ids = np.unique(np.asarray(ids, np.int64))
        if len(ids) and (ids[0] < 0 or ids[-1] >= self.store.num_graphs):
            raise ValueError('ids outside the store of %d graphs' % self.store.num_graphs)
        cut = []
        for n_pad, members in self.store.epoch(1 << 30):
            members = members[np.isin(members, ids)]
            cut += [(n_pad, members[s:s + self.batch_size]) for s in range(0, len(members), self.batch_size)]
        return cut

    def step_for(self, n_pad):
        if n_pad not in self.steps:
            self.steps[n_pad] = StoreEvalStep(self.task, self.model, self.store, n_pad, self.batch_size, self.scores,
                                              self.terms, self.dtype, criterion=self.criterion)
        return self.steps[n_pad]

    def evaluate(self, ids=None):
        import numpy as np
        cut = self.batches(ids)
        if not cut:
            raise ValueError('nothing to evaluate')
        for n_pad, batch in cut:
            self.step_for(n_pad)(batch)
        host = torch.cat((self.scores, self.terms), dim=1).cpu().double()       # the one device read
        terms = host[:, self.scores.shape[1]:]
        walked = torch.from_numpy(np.concatenate([batch for _, batch in cut]).astype(np.int64))
        n_sample = len(walked)
        loss = 0.0
        for _, batch in cut:
            rows = terms[torch.from_numpy(batch.astype(np.int64))]
            loss += float(rows[:, 0].sum() / rows[:, 3].sum()) * len(batch)      # (weight 0: an unlabelled molhiv graph)
        res = {'loss': loss / n_sample}
        if self.task == 'zinc':
            res.update(mae=res['loss'], mse=float(terms[walked, 1].sum()) / n_sample)
        elif self.task == 'tu':
            res['acc'] = float(terms[walked, 1].sum()) / n_sample
        elif self.task == 'molhiv':
            res['rocauc'] = rocauc(host[walked, 0], self.labels[walked])
        return res
