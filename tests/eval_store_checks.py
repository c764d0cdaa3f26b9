"""Checks of the store-fed evaluation: the readout launch (feta_readout_eval, csrc/readout.hip) against fp64 torch on the
same rows, and train.StoreEvalStep / train.StoreEvaluator against the eager model and train.evaluate on store.batch
batches of the same cut.  Written once, run on the host emulation (test_eval_store_emu.py) and on the MI355X
(test_eval_store_gpu.py); the splits are the seeded 23-graph splits of store_checks.packed_split."""
import copy
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import infer_checks as IC
import kernel_checks as KC
import store_checks as SC
from heads8_checks import counted_calls
from feta_tmlr_amd import _abi
from feta_tmlr_amd import functional as FF
from feta_tmlr_amd import train as T
from feta_tmlr_amd.transformer import models as M
from feta_tmlr_amd.transformer.store import DeviceGraphStore

D_MODEL = 64
# (loss_kind, outputs, label dtype): the three loss kinds, C in {1, 3, 10}; BCE on float labels (molhiv, one of them NaN)
# and on int64 labels (a tu model with one output)
LOSSES = [('l1', 1, torch.float32), ('bce_logits', 1, torch.float32), ('bce_logits', 1, torch.int64),
          ('ce', 3, torch.int64), ('ce', 10, torch.int64)]
SLOPES = [0.0, 1.0, 0.01]
# (N, layout of y): contiguous [N, B, 64]; the middle columns of a [N, B, 128] tensor (16-byte loads on other strides); the
# columns 1 .. 64 of a [N, B, 66] tensor (no 16-byte alignment: the element-wise loads)
LAYOUTS = [(16, 'dense'), (37, 'dense'), (37, 'view'), (16, 'unaligned')]
LAUNCHES = ('batch_gather', 'batch_gather_ex', 'encoder_infer', 'encoder_infer_ex', 'readout_eval')


def poisoned_out(g, c, dev):
    """scores [g, c] and terms [g, 4] with every byte 0xFF, as store_checks.poisoned leaves a gather's outputs"""
    scores, terms = torch.empty(g, c, device=dev), torch.empty(g, 4, device=dev)
    scores.view(torch.uint8).fill_(0xFF)
    terms.view(torch.uint8).fill_(0xFF)
    return scores, terms


def untouched(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


def readout_case(n, layout, loss, c, label_dtype, slope, dev, bsz=5, g=11, seed=0):
    """fp32 operands of one launch on ``dev``: n_real holds 1 and N, the ids are not ascending"""
    gen = torch.Generator().manual_seed(1000 * n + 10 * c + seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    width, lo = {'dense': (D_MODEL, 0), 'view': (2 * D_MODEL, 32), 'unaligned': (D_MODEL + 2, 1)}[layout]
    y = rnd(n, bsz, width).to(dev)[:, :, lo:lo + D_MODEL]
    n_real = torch.tensor([n, 1, max(1, n // 2), n - 1, 3], dtype=torch.int32)
    ids = torch.tensor([7, 2, 9, 0, 4], dtype=torch.int32)
    if label_dtype == torch.int64:
        labels = torch.randint(0, max(c, 2), (bsz,), generator=gen)
    elif loss == 'bce_logits':
        labels = torch.tensor([1.0, float('nan'), 0.0, 1.0, 0.0])
    else:
        labels = rnd(bsz)
    w = dict(w1=rnd(D_MODEL, D_MODEL) * 0.2, b1=rnd(D_MODEL) * 0.2, w2=rnd(c, D_MODEL) * 0.2, b2=rnd(c) * 0.2)
    ops = dict(y=y, n_real=n_real.to(dev), ids=ids.to(dev), labels=labels.to(dev), **{k: v.to(dev) for k, v in w.items()})
    return ops, dict(loss=loss, slope=slope, g=g, c=c)


def readout_reference(ops, kw, count):
    """fp64 torch on the same rows -> {graph id: (logits [C], terms [4])} of the first ``count`` slots"""
    o = {k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu()) for k, v in ops.items()}
    out = {}
    for b in range(count):
        n = int(o['n_real'][b])
        v = F.linear(o['y'][:n, b].mean(0), o['w1'], o['b1'])
        logits = F.linear(torch.where(v > 0, v, kw['slope'] * v), o['w2'], o['b2'])
        label = o['labels'][b]
        if kw['loss'] == 'l1':
            e = logits[0] - label
            terms = [abs(e), e * e, 0.0, 1.0]
        elif kw['loss'] == 'bce_logits':
            label = label.double()
            hit = float(bool(logits[0] > 0) == bool(label > 0.5))
            if math.isnan(float(label)):
                terms = [0.0, hit, 0.0, 0.0]
            else:
                terms = [F.binary_cross_entropy_with_logits(logits[0], label), hit, 0.0, 1.0]
        else:
            terms = [F.cross_entropy(logits[None], label[None]), float(int(logits.argmax()) == int(label)), 0.0, 1.0]
        out[int(o['ids'][b])] = (logits, torch.tensor([float(t) for t in terms], dtype=torch.float64))
    return out


def launch_readout(ops, kw, count, dev):
    scores, terms = poisoned_out(kw['g'], kw['c'], dev)
    cnt = torch.tensor([count], dtype=torch.int32, device=dev)
    FF.readout_eval(ops['y'], ops['n_real'], ops['ids'], cnt, ops['labels'], ops['w1'], ops['b1'], ops['w2'], ops['b2'],
                    scores, terms, kw['loss'], kw['slope'])
    return scores, terms


def check_readout(dev, run_ctx, n, layout, loss, c, label_dtype, slope, count=5):
    """scores and terms of the first ``count`` slots against fp64 (KC.TOL); every other row of the poisoned buffers - the
    ids of the slots from ``count`` on, the ids not in the batch - keeps its bytes"""
    ops, kw = readout_case(n, layout, loss, c, label_dtype, slope, dev)
    assert ops['y'].is_contiguous() == (layout == 'dense')
    with run_ctx():
        scores, terms = launch_readout(ops, kw, count, dev)
    ref = readout_reference(ops, kw, count)
    live = sorted(ref)
    KC.assert_close('scores', scores[live], torch.stack([ref[g][0] for g in live]))
    KC.assert_close('terms', terms[live], torch.stack([ref[g][1] for g in live]))
    rest = [g for g in range(kw['g']) if g not in ref]
    assert len(live) == count and untouched(scores[rest]) and untouched(terms[rest])


def check_readout_deterministic(dev, run_ctx):
    ops, kw = readout_case(37, 'dense', 'ce', 10, torch.int64, 0.01, dev)
    with run_ctx():
        a, b = launch_readout(ops, kw, 5, dev), launch_readout(ops, kw, 5, dev)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def check_readout_arguments(dev, run_ctx):
    """the entry point and the wrapper refuse what the kernel does not cover, before any launch"""
    ops, kw = readout_case(16, 'dense', 'ce', 3, torch.int64, 0.0, dev)
    call = lambda **o: launch_readout(dict(ops, **o), kw, 5, dev)
    with run_ctx():
        call()
        with pytest.raises(ValueError, match='int64 class labels'):
            call(labels=ops['labels'].float())
        with pytest.raises(ValueError, match='dense columns'):
            call(y=ops['y'].transpose(1, 2))
        with pytest.raises(ValueError, match='w2'):
            call(w2=ops['w2'][:2])
        with pytest.raises(ValueError, match='ids'):
            call(ids=ops['ids'][:3])
        with pytest.raises(ValueError, match='needs C = 1'):
            launch_readout(ops, dict(kw, loss='l1'), 5, dev)


def check_struct_layout():
    """struct feta_readout of the header against _abi.Readout (test_abi.test_descriptor_layouts_agree for the new one)"""
    from test_abi import _header_structs
    kinds = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_int64: 'int64'}
    assert [(n, kinds[t]) for n, t in _abi.Readout._fields_] == _header_structs()['feta_readout']


# ---- step and evaluator, end to end ----------------------------------------------------------------------------------

BUCKETS, BSZ = (16, 32, 64), 8


@functools.lru_cache(maxsize=None)
def molhiv_split():
    """the 'zinc' split with integer atom features (ogbg-molhiv wire format) and binary labels, a few of them NaN"""
    pk = copy.copy(SC.packed_split('zinc', 9))
    rng = np.random.default_rng(5)
    pk.x = np.stack([rng.integers(0, dmax, size=pk.x.shape[0]) for dmax in M.ATOM_FEATURE_DIMS], 1).astype(np.float32)
    pk.y = rng.integers(0, 2, size=pk.num_graphs).astype(np.float32)
    pk.y[[1, 6, 13, 20]] = np.nan
    return pk


@functools.lru_cache(maxsize=None)
def _store(task, dev_str):
    """the 23-graph store of a task, buckets (16, 32, 64): built once per device under whichever backend is active, then
    only read"""
    packed, opts = {'zinc': (SC.packed_split('zinc', 7), dict(k_eig=8)), 'tu': (SC.packed_split('mutag', 7), dict(lhat=True)),
                    'molhiv': (molhiv_split(), dict(k_eig=8, lap_dim=4))}[task]
    return DeviceGraphStore(packed, torch.device(dev_str), buckets=BUCKETS, pos_enc='diffusion', build_batch=8, **opts)


def eval_case(task, dev, layers=2):
    """-> (model, criterion, store) of the three graph-level tasks: zinc BatchNorm / 4 heads / spectral, tu LayerNorm / 8
    heads / cheb on a store with lhat / 3 classes, molhiv BatchNorm / 4 heads / spectral with Laplacian eigenvector features
    and NaN labels; every bias, norm parameter and running statistic randomised"""
    torch.manual_seed(3)
    kw = dict(dim_feedforward=2 * D_MODEL, dropout=0.0, nb_layers=layers, filter_order=3, heads_share_graph=True)
    if task == 'zinc':
        model = M.DiffGraphTransformerGenGCN(7, 1, D_MODEL, 4, batch_norm=True, filter_mode='spectral', **kw)
    elif task == 'tu':
        model = M.DiffGraphTransformerGenGCN(7, 3, D_MODEL, 8, batch_norm=False, filter_mode='cheb', **kw)
    else:
        model = M.DiffGraphTransformerGenGCNMolHiv(9, 1, D_MODEL, 4, batch_norm=True, filter_mode='spectral', lap_pos_enc=True,
                                                   lap_pos_enc_dim=4, **kw)
    IC.randomise_eval_state(model, seed=17, stat_spread=0.5)
    return model.to(dev), T.make_criterion(task, nb_class=3), _store(task, str(dev))


def eager_reference(task, model, crit, store, cut):
    """-> (scores [G, C], result dict) of train.evaluate(..., inference_mode=True) on the store.batch(ids, n_pad) batches of
    ``cut``: the eager model in eval() under inference_mode; the scores are what its classifier returned, batch by batch"""
    outs = []
    hook = model.classifier.register_forward_hook(lambda mod, args, out: outs.append(out.detach().clone()))
    try:
        res = T.evaluate(task, model, crit, [store.batch(ids, n_pad) for n_pad, ids in cut], inference_mode=True)
    finally:
        hook.remove()
    scores = torch.full((store.num_graphs, outs[0].shape[-1]), float('nan'), device=store.device)
    for (n_pad, ids), out in zip(cut, outs):
        scores[torch.from_numpy(ids.astype(np.int64)).to(store.device)] = out
    return scores, res


def assert_same_results(task, got, ref):
    assert sorted(got) == sorted(ref) == sorted(['loss'] + {'zinc': ['mae', 'mse'], 'tu': ['acc'], 'molhiv': ['rocauc']}[task])
    for k in ref:
        print('%s %s: evaluator %.9g  train.evaluate %.9g' % (task, k, got[k], ref[k]))
        if math.isnan(ref[k]):
            assert math.isnan(got[k]), k
        else:
            KC.assert_close(task + ' ' + k, torch.tensor(got[k], dtype=torch.float64), torch.tensor(ref[k], dtype=torch.float64))


def walked(cut, dev):
    return torch.from_numpy(np.concatenate([ids for _, ids in cut]).astype(np.int64)).to(dev)


def check_evaluator(task, dev, run_ctx, layers=2, bsz=BSZ, take=None):
    """scores and result dict of StoreEvaluator.evaluate() against the eager model and train.evaluate on the same cut -
    full batches and ragged tails of both buckets -, model.training restored; then ONE train_step moves weights and
    running statistics in place and a second evaluate() through the same steps reports the updated model.
    take (the emulation, where every lane is a host fiber): only the first take[0] graphs of the bucket of 16 and the
    first take[1] of the bucket of 32, cut into batches of ``bsz``"""
    with run_ctx():
        model, crit, store = eval_case(task, dev, layers)
        model.train()
        ev = T.StoreEvaluator(task, model, crit, store, bsz)
        ids = None if take is None else np.concatenate([store.bucket_ids(16)[:take[0]], store.bucket_ids(32)[:take[1]]])
        cut = ev.batches(ids)
        sizes = [len(b) for _, b in cut]
        assert sum(sizes) == (SC.NUM_GRAPHS if ids is None else len(ids)), cut
        assert bsz in sizes and min(sizes) < bsz and len({n for n, _ in cut}) > 1, cut
        ev.scores.view(torch.uint8).fill_(0xFF)
        ev.terms.view(torch.uint8).fill_(0xFF)
        got = ev.evaluate(ids)
        assert model.training
        first = ev.scores.clone()
        ref_scores, ref = eager_reference(task, model, crit, store, cut)
        assert model.training
        w = walked(cut, dev)
        KC.assert_close(task + ' scores', first[w], ref_scores[w].double())
        assert_same_results(task, got, ref)
        if ids is not None:      # nothing but the rows of the graphs that were walked has been written
            rest = [g for g in range(store.num_graphs) if g not in ids.tolist()]
            assert untouched(ev.scores[rest]) and untouched(ev.terms[rest])
        steps = dict(ev.steps)
        graphs = {n: s.graph for n, s in steps.items()}

        opt = T.make_optimizer(task, model.parameters(), lr=1e-2)
        full = next((n_pad, b) for n_pad, b in cut if len(b) == bsz)
        T.train_step(task, model, crit, opt, *store.batch(full[1], full[0]))
        got2 = ev.evaluate(ids)
        assert ev.steps == steps and all(s.graph is graphs[n] for n, s in ev.steps.items())
        ref_scores2, ref2 = eager_reference(task, model, crit, store, cut)
        KC.assert_close(task + ' scores after a training step', ev.scores[w], ref_scores2[w].double())
        assert_same_results(task, got2, ref2)
        assert float((ev.scores[w] - first[w]).abs().max()) > 1e-3


def check_subsets(task, dev, run_ctx, layers=2, take=(7, 4)):
    """a batch of ONE graph, a subset out of both buckets given in no order, and too many ids for a step"""
    with run_ctx():
        model, crit, store = eval_case(task, dev, layers)
        model.eval()
        ev = T.StoreEvaluator(task, model, crit, store, BSZ)
        labelled = int(np.nonzero(~np.isnan(store.y.cpu().numpy().astype(np.float64)))[0][3])
        mixed = np.concatenate([store.bucket_ids(32)[-take[1]:], store.bucket_ids(16)[-take[0]:][::-1]]).tolist()
        for ids in ([labelled], mixed):
            cut = ev.batches(ids)
            assert sorted(int(i) for _, b in cut for i in b) == sorted(ids)
            got = ev.evaluate(ids)
            ref_scores, ref = eager_reference(task, model, crit, store, cut)
            w = walked(cut, dev)
            KC.assert_close(task + ' scores of a subset', ev.scores[w], ref_scores[w].double())
            assert_same_results(task, got, ref)
        assert not model.training
        step = ev.step_for(16)
        with pytest.raises(ValueError, match='1 to 8 ids'):
            step(store.bucket_ids(16)[:9])
        with pytest.raises(ValueError, match='1 to 8 ids'):
            step([])


def check_refused(dev, run_ctx):
    """every configuration the step does not run raises ValueError and names store.batch + train.evaluate"""
    with run_ctx():
        model, crit, store = eval_case('zinc', dev, 1)
        tu_model, tu_crit, tu_store = eval_case('tu', dev, 1)
        eager = 'store.batch and train.evaluate'
        with pytest.raises(ValueError, match="'sbm'.*" + eager):
            T.StoreEvaluator('sbm', model, crit, store, BSZ)
        scores, terms = poisoned_out(store.num_graphs, 1, dev)
        with pytest.raises(ValueError, match='one-launch inference.*' + eager):       # N_pad > 64
            T.StoreEvalStep('zinc', model, store, 128, BSZ, scores, terms)
        wide = M.DiffGraphTransformerGenGCN(7, 1, D_MODEL, 4, dim_feedforward=256, dropout=0.0, nb_layers=1, batch_norm=True,
                                            filter_order=3, heads_share_graph=True, filter_mode='spectral').to(dev)
        with pytest.raises(ValueError, match='one-launch inference.*' + eager):       # a feed-forward width it does not have
            T.StoreEvalStep('zinc', wide, store, 16, BSZ, scores, terms)
        many = M.DiffGraphTransformerGenGCN(7, 65, D_MODEL, 8, dim_feedforward=128, dropout=0.0, nb_layers=1,
                                            filter_mode='cheb').to(dev)
        with pytest.raises(ValueError, match='feta_readout_eval.*' + eager):
            T.StoreEvaluator('tu', many, torch.nn.CrossEntropyLoss(), tu_store, BSZ)
        with pytest.raises(ValueError, match='class weights.*' + eager):
            T.StoreEvaluator('tu', tu_model, torch.nn.CrossEntropyLoss(weight=torch.ones(3, device=dev)), tu_store, BSZ)
        with pytest.raises(ValueError, match='reduction.*' + eager):
            T.StoreEvaluator('zinc', model, torch.nn.L1Loss(reduction='sum'), store, BSZ)
        with pytest.raises(ValueError, match='lhat=True.*' + eager):
            T.StoreEvaluator('tu', tu_model, tu_crit, store, BSZ)
        with pytest.raises(ValueError, match='scores'):
            T.StoreEvalStep('zinc', model, store, 16, BSZ, scores[:5], terms)


def check_launches(task, dev, run_ctx, abi, layers=2):
    """the body of a step is one gather call, one encoder_infer[_ex] call and one readout_eval call; a captured step runs
    the body warmup_iters + 1 times when it is built and calls nothing from the host when it is replayed"""
    with run_ctx():
        model, crit, store = eval_case(task, dev, layers)
        scores, terms = poisoned_out(store.num_graphs, model.classifier[2].out_features, dev)
        with counted_calls(abi, LAUNCHES) as calls:
            step = T.StoreEvalStep(task, model, store, 16, BSZ, scores, terms, criterion=crit)
        bodies = 0 if step.graph is None else 4
        ids = store.bucket_ids(16)[:5]
        with counted_calls(abi, LAUNCHES) as replay:
            step(ids)
        if step.graph is None:
            calls, replay, bodies = replay, {}, 1
        assert not replay, replay
        gathers = calls.get('batch_gather', 0) + calls.get('batch_gather_ex', 0)
        stacks = calls.get('encoder_infer', 0) + calls.get('encoder_infer_ex', 0)
        assert (gathers, stacks, calls.get('readout_eval', 0)) == (bodies, bodies, bodies), calls
        live = torch.from_numpy(ids.astype(np.int64)).to(dev)
        rest = [g for g in range(store.num_graphs) if g not in ids.tolist()]
        assert bool(torch.isfinite(scores[live]).all()) and bool(torch.isfinite(terms[live]).all())
        if step.graph is None:       # (a captured step has written its warm-up batch too)
            assert untouched(scores[rest]) and untouched(terms[rest])
    return step


def check_no_host_sync(task, dev):
    """GPU: step() does not wait for the device - not on the first calls, which allocate the pinned buffers, nor on the
    later ones, which reuse them"""
    step = check_launches(task, dev, __import__('contextlib').nullcontext, __import__('feta_tmlr_amd')._lib.abi())
    ids = step.store.bucket_ids(16)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for k in (8, 3, 1, 8, 5):
            step(ids[:k])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
