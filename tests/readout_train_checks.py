"""Checks of the training head (feta_readout_train_fwd / _bwd, csrc/readout.hip; functional.readout_train; the fused_head
option of train.task_loss, train_step, GraphedTrainStep and StoreTrainStep).  The kernel-level reference is fp64 autograd of
masked mean pooling -> classifier -> the loss as train.task_loss writes it; the model-level reference is the same step with
fused_head=False.  Written once, run on the host emulation (test_readout_train_emu.py) and on the MI355X
(test_readout_train_gpu.py).  Bars: kernel_checks.TOL for loss and scores, 3e-5 relative for gradients (the bar of the
trajectory checks), bench_checks.BF16_MODEL_TOL for bf16-storage models."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eval_store_checks as EC
import kernel_checks as KC
import store_checks as SC
from heads8_checks import counted_calls
from feta_tmlr_amd import _abi
from feta_tmlr_amd import functional as FF
from feta_tmlr_amd import train as T
from feta_tmlr_amd.transformer import data as D
from feta_tmlr_amd.transformer.store import DeviceGraphStore

GRAD_TOL = 3e-5
PARAMS = ('w1', 'b1', 'w2', 'b2')
HEAD_CALLS = ('readout_train_fwd', 'readout_train_bwd')


def train_case(n, layout, loss, c, label_dtype, slope, dev, bsz=6, bias=True, all_nan=False):
    """eval_store_checks.readout_case at ``bsz`` slots (its y and weights), with n_real and labels of that length: slot 0 has
    n_real = N, slot 1 has n_real = 1 and, under BCE on float labels, a NaN label"""
    ops, kw = EC.readout_case(n, layout, loss, c, label_dtype, slope, dev, bsz=bsz)
    gen = torch.Generator().manual_seed(77 * n + bsz)
    n_real = torch.randint(1, n + 1, (bsz,), generator=gen).to(torch.int32)
    n_real[0], n_real[1] = n, 1
    if label_dtype == torch.int64:
        labels = torch.randint(0, max(c, 2), (bsz,), generator=gen)
    elif loss == 'bce_logits':
        labels = torch.randint(0, 2, (bsz,), generator=gen).float()
        labels[1] = float('nan')
        if all_nan:
            labels[:] = float('nan')
    else:
        labels = torch.randn(bsz, generator=gen)
    ops.update(n_real=n_real.to(dev), labels=labels.to(dev))
    del ops['ids']
    if not bias:
        ops['b1'] = ops['b2'] = None
    return ops, kw


def loss_as_task_loss(kw, out, labels):
    """the loss of train.task_loss on logits ``out`` [B, C]: 'zinc' (l1), 'molhiv' (bce_logits on float labels, NaN = no
    label), 'tu' with one output (bce_logits on int64 labels) or with C classes (ce)"""
    if kw['loss'] == 'l1':
        return F.l1_loss(out, labels.view(out.shape).to(out.dtype))
    if kw['loss'] == 'ce':
        return F.cross_entropy(out, labels)
    if labels.is_floating_point():
        keep = ~torch.isnan(labels)
        tgt = torch.where(keep, labels, torch.zeros_like(labels)).to(out.dtype)
        w = keep.to(out.dtype)
        per = F.binary_cross_entropy_with_logits(out.view(-1), tgt, reduction='none')
        return (per * w).sum() / w.sum()
    return F.binary_cross_entropy_with_logits(out.view(-1), labels.to(out.dtype))


def reference(ops, kw, count, gscale=1.0):
    """fp64 autograd on the first ``count`` slots -> dict(loss, scores [count, C], dy [N, B, 64] (zero in the slots from
    count on), w1, b1, w2, b2 gradients)"""
    o = {k: (None if v is None else v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu())
         for k, v in ops.items()}
    for k in ('y',) + PARAMS:
        if o[k] is not None:
            o[k].requires_grad_()
    n = o['y'].shape[0]
    nr = o['n_real'][:count].long()
    keep = (torch.arange(n)[:, None] < nr[None, :]).double().unsqueeze(-1)
    pooled = (o['y'][:, :count] * keep).sum(0) / keep.sum(0)
    v = F.linear(pooled, o['w1'], o['b1'])
    out = F.linear(torch.where(v > 0, v, kw['slope'] * v), o['w2'], o['b2'])
    loss = loss_as_task_loss(kw, out, o['labels'][:count])
    (gscale * loss).backward()
    res = dict(loss=loss.detach(), scores=out.detach(), dy=o['y'].grad)
    res.update({k: None if o[k] is None else o[k].grad for k in PARAMS})
    return res


def run(ops, kw, count, dev, gscale=None):
    """functional.readout_train and its backward on leaf copies of the operands -> the dict of ``reference``"""
    leaf = {k: (None if ops[k] is None else ops[k].detach().clone().requires_grad_()) for k in PARAMS}
    if ops['y'].is_contiguous():
        y = ops['y'].detach().clone().requires_grad_()
        rows = y
    else:       # a view keeps its strides: the leaf is the tensor it is cut from
        y, rows = _leaf_view(ops['y'])
    cnt = torch.tensor([count], dtype=torch.int32, device=dev)
    loss, scores = FF.readout_train(rows, ops['n_real'], cnt, ops['labels'], leaf['w1'], leaf['b1'], leaf['w2'], leaf['b2'],
                                    kw['loss'], kw['slope'])
    assert loss.dim() == 0 and tuple(scores.shape) == (rows.shape[1], kw['c']) and not scores.requires_grad
    (loss if gscale is None else gscale * loss).backward()
    dy = y.grad if rows is y else _cut_like(y.grad, ops['y'])
    res = dict(loss=loss.detach(), scores=scores.detach(), dy=dy)
    res.update({k: None if leaf[k] is None else leaf[k].grad for k in PARAMS})
    return res


def _leaf_view(view):
    """(leaf, rows): a leaf copy of the storage ``view`` is cut from and the same cut of it"""
    base = view._base if view._base is not None else view
    leaf = base.detach().clone().requires_grad_()
    off = view.storage_offset() - base.storage_offset()
    return leaf, leaf.as_strided(view.shape, view.stride(), leaf.storage_offset() + off)


def _cut_like(grad, view):
    base = view._base if view._base is not None else view
    return grad.as_strided(view.shape, view.stride(), view.storage_offset() - base.storage_offset())


def assert_matches(got, ref, count, what=''):
    KC.assert_close(what + 'loss', got['loss'].reshape(1), ref['loss'].reshape(1))
    KC.assert_close(what + 'scores', got['scores'][:count], ref['scores'])
    KC.assert_close(what + 'dy', got['dy'], ref['dy'], tol=GRAD_TOL)
    for k in PARAMS:
        assert (got[k] is None) == (ref[k] is None), k
        if ref[k] is not None:
            KC.assert_close(what + 'd' + k, got[k], ref[k], tol=GRAD_TOL)


def check_kernels(dev, run_ctx, n, layout, loss, c, label_dtype, slope, bsz=6, bias=True):
    """loss, scores, dy WHOLE (the padded rows are zero in the reference) and the four parameter gradients against fp64
    autograd; the padded rows of dy are exactly zero"""
    ops, kw = train_case(n, layout, loss, c, label_dtype, slope, dev, bsz=bsz, bias=bias)
    assert ops['y'].is_contiguous() == (layout == 'dense')
    with run_ctx():
        got = run(ops, kw, bsz, dev)
    ref = reference(ops, kw, bsz)
    assert_matches(got, ref, bsz)
    pad = torch.arange(n)[:, None] >= ops['n_real'].cpu()[None, :].long()
    assert bool(pad.any()) and float(got['dy'].cpu()[pad].abs().max()) == 0.0


def check_count(abi, dev, stream, loss, c, label_dtype):
    """count = 3 of 6, through the entry points on poisoned outputs: loss, scores and parameter gradients are those of the
    3-slot batch, dy of the slots 3..5 is exactly zero, the rows 3..5 of scores keep their bytes"""
    n, bsz, count = 16, 6, 3
    ops, kw = train_case(n, 'dense', loss, c, label_dtype, 0.01, dev, bsz=bsz)
    poisoned = lambda *shape: torch.empty(*shape, device=dev).view(torch.uint8).fill_(0xFF).view(torch.float32)
    out = dict(scores=poisoned(bsz, c), loss=poisoned(2), ws=poisoned(abi.readout_train_ws_floats(bsz, c)))
    grads = dict(dy=poisoned(n, bsz, 64), dw1=poisoned(64, 64), db1=poisoned(64), dw2=poisoned(c, 64), db2=poisoned(c))
    kind = _abi.LABELS_GRAPH_F32 if ops['labels'].dtype == torch.float32 else _abi.LABELS_GRAPH_I64
    geom = dict(row_sb=64, row_sn=bsz * 64, label_kind=kind, loss_kind=FF.LOSS_KINDS[loss], slope=0.01)
    cnt = torch.tensor([count], dtype=torch.int32, device=dev)
    abi.readout_train_fwd(bsz, n, c, stream, count=cnt, **geom, **ops, **out)
    abi.readout_train_bwd(bsz, n, c, stream, count=cnt, drow_sb=64, drow_sn=bsz * 64, dloss=torch.ones(1, device=dev),
                          **geom, **ops, **out, **grads)
    ref = reference(ops, kw, count)
    got = dict(loss=out['loss'][0], scores=out['scores'], dy=grads['dy'], w1=grads['dw1'], b1=grads['db1'], w2=grads['dw2'],
               b2=grads['db2'])
    assert_matches(got, ref, count)
    assert float(grads['dy'][:, count:].abs().max()) == 0.0
    assert EC.untouched(out['scores'][count:])
    KC.assert_close('1 / sum of the weights', out['loss'][1:], 1.0 / _weight_sum(ops, kw, count).reshape(1))


def _weight_sum(ops, kw, count):
    labels = ops['labels'][:count].cpu()
    if kw['loss'] == 'bce_logits' and labels.is_floating_point():
        return (~torch.isnan(labels)).double().sum()
    return torch.tensor(float(count), dtype=torch.float64)


def check_incoming_gradient(dev, run_ctx, captured=False):
    """(2.5 * loss).backward(): every gradient is 2.5 x the reference's.  captured (GPU): forward and backward run inside a
    torch.cuda.graph capture, where a host read of the incoming gradient or of the loss would be an error, and the gradients
    are those of the replay"""
    ops, kw = train_case(16, 'dense', 'ce', 3, torch.int64, 0.01, dev)
    ref = reference(ops, kw, 6, gscale=2.5)
    plain = reference(ops, kw, 6)
    KC.assert_close('the reference scales', ref['w1'], 2.5 * plain['w1'], tol=1e-12)
    if not captured:
        with run_ctx():
            got = run(ops, kw, 6, dev, gscale=2.5)
        assert_matches(got, ref, 6)
        return
    leaf = {k: ops[k].detach().clone().requires_grad_() for k in ('y',) + PARAMS}
    cnt = torch.tensor([6], dtype=torch.int32, device=dev)

    def body():
        loss, scores = FF.readout_train(leaf['y'], ops['n_real'], cnt, ops['labels'], leaf['w1'], leaf['b1'], leaf['w2'],
                                        leaf['b2'], kw['loss'], kw['slope'])
        (2.5 * loss).backward()
        return loss.detach(), scores
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    for t in leaf.values():
        t.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, scores = body()
    for t in leaf.values():
        t.grad.view(torch.uint8).fill_(0xFF)
    graph.replay()
    got = dict(loss=loss, scores=scores, dy=leaf['y'].grad, **{k: leaf[k].grad for k in PARAMS})
    assert_matches(got, ref, 6)


def check_deterministic(dev, run_ctx):
    """two runs on the same operands: loss, scores, dy and the four parameter gradients bit for bit"""
    ops, kw = train_case(37, 'dense', 'ce', 10, torch.int64, 0.01, dev, bsz=70)
    with run_ctx():
        a, b = run(ops, kw, 70, dev), run(ops, kw, 70, dev)
    for k in a:
        assert torch.equal(a[k].reshape(-1).view(torch.int32), b[k].reshape(-1).view(torch.int32)), k


def check_many_slots(dev, run_ctx, bsz, n=16):
    """more slots than one chunk of the parameter-gradient contraction (64) and than one lane each of the loss reduction
    (256 at B = 300 and 1024): CE with 10 classes"""
    ops, kw = train_case(n, 'dense', 'ce', 10, torch.int64, 0.01, dev, bsz=bsz)
    with run_ctx():
        got = run(ops, kw, bsz, dev)
    assert_matches(got, reference(ops, kw, bsz), bsz)


def check_all_labels_nan(dev, run_ctx):
    """no labelled graph under BCE: NaN, as task_loss gives on the same batch (0 / 0)"""
    ops, kw = train_case(16, 'dense', 'bce_logits', 1, torch.float32, 1.0, dev, all_nan=True)
    with run_ctx(), torch.no_grad():
        loss, scores = FF.readout_train(ops['y'], ops['n_real'], torch.tensor([6], dtype=torch.int32, device=dev), ops['labels'],
                                        ops['w1'], ops['b1'], ops['w2'], ops['b2'], kw['loss'], kw['slope'])
    ref = reference(ops, kw, 6)
    assert math.isnan(float(ref['loss'])) and math.isnan(float(loss))
    KC.assert_close('scores', scores, ref['scores'])


def check_no_grad_and_frozen(dev, run_ctx, abi):
    """under no_grad only the forward runs; a parameter that does not require a gradient gets None"""
    ops, kw = train_case(16, 'dense', 'l1', 1, torch.float32, 0.0, dev)
    cnt = torch.tensor([6], dtype=torch.int32, device=dev)
    args = lambda o: (o['y'], o['n_real'], cnt, o['labels'], o['w1'], o['b1'], o['w2'], o['b2'], kw['loss'], kw['slope'])
    with run_ctx():
        with counted_calls(abi, HEAD_CALLS) as calls, torch.no_grad():
            loss, _ = FF.readout_train(*args(ops))
        assert calls == {'readout_train_fwd': 1} and not loss.requires_grad
        live = dict(ops, y=ops['y'].clone().requires_grad_(), w2=ops['w2'].clone().requires_grad_())
        with counted_calls(abi, HEAD_CALLS) as calls:
            FF.readout_train(*args(live))[0].backward()
        assert calls == {'readout_train_fwd': 1, 'readout_train_bwd': 1}
    ref = reference(ops, kw, 6)
    KC.assert_close('dy', live['y'].grad, ref['dy'], tol=GRAD_TOL)
    KC.assert_close('dw2', live['w2'].grad, ref['w2'], tol=GRAD_TOL)
    assert all(ops[k].grad is None for k in ('w1', 'b1', 'b2'))


def check_arguments(dev, run_ctx):
    """the entry points and the wrapper refuse what the kernels do not cover, before any launch (the checks of
    functional.readout_eval)"""
    ops, kw = train_case(16, 'dense', 'ce', 3, torch.int64, 0.0, dev)
    cnt = torch.tensor([6], dtype=torch.int32, device=dev)

    def call(loss='ce', **o):
        o = dict(ops, **o)
        return FF.readout_train(o['y'], o['n_real'], o.get('count', cnt), o['labels'], o['w1'], o['b1'], o['w2'], o['b2'],
                                loss, 0.0)
    with run_ctx():
        call()
        with pytest.raises(ValueError, match='int64 class labels'):
            call(labels=ops['labels'].float())
        with pytest.raises(ValueError, match='dense columns'):
            call(y=ops['y'].transpose(1, 2))
        with pytest.raises(ValueError, match='w1'):
            call(w1=ops['w1'][:2])
        with pytest.raises(ValueError, match='n_real'):
            call(n_real=ops['n_real'][:3])
        with pytest.raises(ValueError, match='labels'):
            call(labels=ops['labels'][:3])
        with pytest.raises(ValueError, match='count'):
            call(count=cnt[:0])
        with pytest.raises(ValueError, match='needs C = 1'):
            call(loss='l1')
        with pytest.raises(ValueError, match='unknown loss_kind'):
            call(loss='mse')
        with pytest.raises(ValueError, match='C = 65'):
            call(w2=torch.zeros(65, 64, device=dev), b2=None)
        with pytest.raises(TypeError, match='labels'):
            call(labels=ops['labels'].to(torch.int32))


def check_struct_layout():
    """struct feta_readout_train of the header against _abi.ReadoutTrain (eval_store_checks.check_struct_layout for it)"""
    from test_abi import _header_structs
    kinds = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_int64: 'int64'}
    assert [(n, kinds[t]) for n, t in _abi.ReadoutTrain._fields_] == _header_structs()['feta_readout_train']


# ---- train_step with the fused head -------------------------------------------------------------------------------------

def step_case(task, dev, bf16=False, layers=1, bsz=2, num_graphs=12, heads=4):
    """store_checks.trajectory_case for the graph-level tasks: two models with the same weights, a store, a stager and three
    id sets.  'molhiv' embeds integer atom features, which that split does not have: its models come from trajectory_case,
    its store and id sets from eval_store_checks.molhiv_split (binary labels, some NaN) in the same way"""
    model_a, model_b, store, stager, id_sets = SC.trajectory_case(task, dev, bf16, layers=layers, bsz=bsz, num_graphs=num_graphs,
                                                                  heads=heads)
    if task == 'molhiv':
        packed = EC.molhiv_split()
        opts = dict(pos_enc='diffusion', k_eig=8)
        store = DeviceGraphStore(packed, dev, build_batch=8, **opts)
        stager = D.BatchStager(packed, bsz, 16, dev, **opts)
        members = np.random.default_rng(11).permutation(store.bucket_ids(16))
        blank = np.isnan(packed.y[members])      # one unlabelled graph leads, the other ones go last: every batch has a label
        members = np.concatenate([members[blank][:1], members[~blank], members[blank][1:]])
        id_sets = [members[0:bsz], members[bsz:2 * bsz], members[[2 * bsz, 1, 2 * bsz - 1, 0][:bsz]]]
        assert blank.any() and not any(np.isnan(packed.y[ids]).all() for ids in id_sets)
    return model_a, model_b, store, stager, id_sets


def check_train_step(task, dev, run_ctx, abi, bf16=False, **case):
    """three steps of train_step(..., fused_head=True) == the same steps with fused_head=False on a copy of the model
    (store_checks.compare_trajectories); a fused step calls readout_train_fwd and readout_train_bwd once each, and its second
    result is [B, C]"""
    crit = T.make_criterion(task, nb_class=3)
    with run_ctx():
        model_a, model_b, store, _, id_sets = step_case(task, dev, bf16, **case)
        opt_a = T.make_optimizer(task, model_a.parameters(), lr=SC.LRS[0])
        opt_b = T.make_optimizer(task, model_b.parameters(), lr=SC.LRS[0])
        losses_a, losses_b = [], []
        for ids, lr in zip(id_sets, SC.LRS):
            losses_a.append(T.train_step(task, model_a, crit, opt_a, *store.batch(ids), lr=lr).clone())
            with counted_calls(abi, HEAD_CALLS) as calls:
                losses_b.append(T.train_step(task, model_b, crit, opt_b, *store.batch(ids), lr=lr, fused_head=True).clone())
            assert calls == {'readout_train_fwd': 1, 'readout_train_bwd': 1}, calls
        with torch.no_grad():
            batch9, cache = store.batch(id_sets[0])
            loss, scores = T.task_loss(task, model_b, crit, batch9, cache, fused_head=True)
            ref_loss, ref_out = T.task_loss(task, model_b, crit, batch9, cache)
        assert tuple(scores.shape) == (len(id_sets[0]), model_b.classifier[2].out_features)
        tol = __import__('bench_checks').BF16_MODEL_TOL if bf16 else KC.TOL
        KC.assert_close(task + ' scores', scores, ref_out.reshape(scores.shape).double(), tol=tol)
        KC.assert_close(task + ' loss', loss.reshape(1), ref_loss.reshape(1).double(), tol=tol)
    SC.compare_trajectories(task, model_a, model_b, opt_a, losses_a, losses_b, SC.LRS, bf16)


def check_refused(dev, run_ctx):
    """what the fused head does not run raises ValueError and names fused_head=False"""
    from feta_tmlr_amd.transformer import models as M
    plain = 'fused_head=False'
    with run_ctx():
        model, _, store, _, id_sets = step_case('tu', dev)
        sbm, _, sbm_store, _, sbm_ids = SC.trajectory_case('sbm', dev, layers=1, bsz=2, num_graphs=12)
        batch = store.batch(id_sets[0])
        with pytest.raises(ValueError, match="'sbm'.*" + plain):
            T.task_loss('sbm', sbm, T.make_criterion('sbm', 3), *sbm_store.batch(sbm_ids[0]), padded_node_labels=True,
                        fused_head=True)
        with pytest.raises(ValueError, match='class weights.*' + plain):
            T.task_loss('tu', model, torch.nn.CrossEntropyLoss(weight=torch.ones(3, device=dev)), *batch, fused_head=True)
        with pytest.raises(ValueError, match='class weights or label smoothing.*' + plain):
            T.task_loss('tu', model, torch.nn.CrossEntropyLoss(label_smoothing=0.1), *batch, fused_head=True)
        with pytest.raises(ValueError, match='reduction.*' + plain):
            T.task_loss('tu', model, torch.nn.CrossEntropyLoss(reduction='sum'), *batch, fused_head=True)
        with pytest.raises(ValueError, match='is evaluated with CrossEntropyLoss.*' + plain):
            T.task_loss('tu', model, torch.nn.L1Loss(), *batch, fused_head=True)
        one = M.DiffGraphTransformerGenGCN(7, 1, 64, 4, dim_feedforward=128, dropout=0.0, nb_layers=1, filter_mode='spectral').to(dev)
        with pytest.raises(ValueError, match='class weights.*' + plain):
            T.task_loss('tu', one, torch.nn.BCEWithLogitsLoss(pos_weight=torch.ones(1, device=dev)), *batch, fused_head=True)
        one.classifier[1] = torch.nn.Tanh()
        with pytest.raises(ValueError, match='ReLU or LeakyReLU.*' + plain):
            T.task_loss('tu', one, torch.nn.BCEWithLogitsLoss(), *batch, fused_head=True)
        one.classifier = torch.nn.Linear(64, 1).to(dev)
        with pytest.raises(ValueError, match='Linear - activation - Linear.*' + plain):
            T.task_loss('tu', one, torch.nn.BCEWithLogitsLoss(), *batch, fused_head=True)
        many = M.DiffGraphTransformerGenGCN(7, 65, 64, 4, dim_feedforward=128, dropout=0.0, nb_layers=1, filter_mode='spectral').to(dev)
        with pytest.raises(ValueError, match='feta_readout_train.*' + plain):
            T.task_loss('tu', many, torch.nn.CrossEntropyLoss(), *batch, fused_head=True)
        narrow = M.DiffGraphTransformerGenGCN(7, 3, 32, 4, dim_feedforward=64, dropout=0.0, nb_layers=1, filter_mode='spectral').to(dev)
        with pytest.raises(ValueError, match='feta_readout_train.*' + plain):
            T.task_loss('tu', narrow, torch.nn.CrossEntropyLoss(), *batch, fused_head=True)


# ---- the captured step (GPU) --------------------------------------------------------------------------------------------

def check_store_step(task, dev, abi, bf16=False, warmup_iters=3):
    """store_checks.check_trajectory_graphed with fused_head=True: three replays of a captured StoreTrainStep == three
    steps of eager train_step on BatchStager.stage(ids); every body the construction runs makes one gather call and one
    readout_train_fwd / _bwd call each, a replay makes no call into the library from the host"""
    crit = T.make_criterion(task, nb_class=3)
    model_a, model_b, store, stager, id_sets = SC.trajectory_case(task, dev, bf16)
    opt_a, losses_a = SC.reference_steps(task, model_a, stager, id_sets, crit)
    opt_b = T.make_optimizer(task, model_b.parameters(), lr=SC.LRS[0], capturable=True)
    names = SC.FEED_NAMES + HEAD_CALLS
    try:
        with counted_calls(abi, names) as calls:
            step = T.StoreTrainStep(task, model_b, crit, opt_b, store, 16, 4, warmup_iters=warmup_iters, fused_head=True)
        bodies = warmup_iters + 1
        assert [calls.get(k) for k in ('batch_gather',) + HEAD_CALLS] == [bodies] * 3 and calls.get('attn_block_fwd', 0) > 0, calls
        losses_b = []
        with counted_calls(abi, names) as calls:
            for i, (ids, lr) in enumerate(zip(id_sets, SC.LRS)):
                step.set_lr(lr)
                losses_b.append(step(ids if i != 1 else store.device_ids(np.concatenate(id_sets))[4:8]).clone())
        assert not calls, calls
        assert len({float(l) for l in losses_b}) == 3
        SC.compare_trajectories(task, model_a, model_b, opt_a, losses_a, losses_b, SC.LRS, bf16)
        with pytest.raises(ValueError, match='1 to 4 ids'):
            step(np.concatenate(id_sets)[:5])
        with pytest.raises(ValueError, match='1 to 4 ids'):
            step([])
    finally:
        FF.DropoutState.end_device_mode()


def check_graphed_step(dev, bf16=False):
    """GraphedTrainStep(..., fused_head=True) fed by a BatchStager: three replays == three eager steps with the plain head"""
    task = 'tu'
    crit = T.make_criterion(task, nb_class=3)
    model_a, model_b, _, stager, id_sets = SC.trajectory_case(task, dev, bf16)
    opt_a, losses_a = SC.reference_steps(task, model_a, stager, id_sets, crit)
    opt_b = T.make_optimizer(task, model_b.parameters(), lr=SC.LRS[0], capturable=True)
    try:
        step = T.GraphedTrainStep(task, model_b, crit, opt_b, *stager.stage(id_sets[0]), fused_head=True)
        losses_b = []
        for ids, lr in zip(id_sets, SC.LRS):
            step.set_lr(lr)
            losses_b.append(step(*stager.stage(ids)).clone())
        SC.compare_trajectories(task, model_a, model_b, opt_a, losses_a, losses_b, SC.LRS, bf16)
    finally:
        FF.DropoutState.end_device_mode()


def check_ragged(dev, bf16=False):
    """a step captured for 4 ids, called with 3, 1 (a device tensor) and 4 ids on a LayerNorm model == eager
    train_step(..., fused_head=False) on store.batch of exactly those ids; the step does not wait for the device"""
    task = 'tu'
    crit = T.make_criterion(task, nb_class=3)
    model_a, model_b, store, _, id_sets = SC.trajectory_case(task, dev, bf16)
    assert not any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) for m in model_b.modules())
    cuts = [id_sets[0][:3], id_sets[1][2:3], id_sets[2]]
    opt_a = T.make_optimizer(task, model_a.parameters(), lr=SC.LRS[0])
    losses_a = [T.train_step(task, model_a, crit, opt_a, *store.batch(ids, 16), lr=lr).clone() for ids, lr in zip(cuts, SC.LRS)]
    opt_b = T.make_optimizer(task, model_b.parameters(), lr=SC.LRS[0], capturable=True)
    try:
        step = T.StoreTrainStep(task, model_b, crit, opt_b, store, 16, 4, fused_head=True)
        sent = [cuts[0], store.device_ids(cuts[1]), cuts[2]]
        torch.cuda.synchronize()
        losses_b = []
        torch.cuda.set_sync_debug_mode('error')
        try:
            for ids, lr in zip(sent, SC.LRS):
                step.set_lr(lr)
                losses_b.append(step(ids).clone())
        finally:
            torch.cuda.set_sync_debug_mode('default')
        assert step.ids.tolist() == [int(i) for i in cuts[2]] + [4]
        SC.compare_trajectories(task, model_a, model_b, opt_a, losses_a, losses_b, SC.LRS, bf16)
    finally:
        FF.DropoutState.end_device_mode()


def check_ragged_batchnorm_refused(dev):
    """a BatchNorm model in training mode keeps the ValueError for a short batch (its batch statistics would see the
    repeated graph), with and without the fused head; full batches run"""
    import train_checks as TC
    task = 'zinc'
    model, _, _ = TC.build_case(task, dev, d=64, heads=4, mode='spectral', batch_norm=True, layers=1)
    model.train()
    store = DeviceGraphStore(SC.packed_split('zinc', 7), dev, pos_enc='diffusion', k_eig=8)
    crit = T.make_criterion(task)
    opt = T.make_optimizer(task, model.parameters(), lr=1e-3, capturable=True)
    ids = store.bucket_ids(16)[:4]
    try:
        step = T.StoreTrainStep(task, model, crit, opt, store, 16, 4, fused_head=True)
        assert math.isfinite(float(step(ids)))
        with pytest.raises(ValueError, match='exactly 4 ids.*BatchNorm'):
            step(ids[:3])
        with pytest.raises(ValueError, match='exactly 4 ids.*BatchNorm'):
            step(store.device_ids(ids[:1]))
    finally:
        FF.DropoutState.end_device_mode()
