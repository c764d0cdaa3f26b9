"""Checks of the device-resident graph store (transformer/store.py: DeviceGraphStore), of the launch that builds a padded
batch from it (feta_batch_gather, csrc/gather.hip) and of the training step fed by it (train.StoreTrainStep).  The
reference of everything here is what the project did before: ``data.BatchStager.stage(ids)`` (+ attach_device_spectrum)
for the tensors, ``train.train_step`` on the staged batch for the trajectory.  Written once, run on the host emulation
(test_store_emu.py) and on the MI355X (test_store_gpu.py)."""
import ctypes
import functools

import numpy as np
import torch

import kernel_checks as KC
import train_checks as TC
from heads8_checks import counted_calls
from feta_tmlr_amd import _abi
from feta_tmlr_amd import train as T
from feta_tmlr_amd.transformer import data as D
from feta_tmlr_amd.transformer.store import DeviceGraphStore, GatherBuffers

NUM_GRAPHS = 23
SPECTRAL = dict(pos_enc='diffusion', k_eig=8, lap_dim=4)
FEED_NAMES = ('batch_gather', 'eigh_sym', 'lhat_from_edges', 'spectral_kernel', 'attn_block_fwd')


@functools.lru_cache(maxsize=None)
def packed_split(kind, f, num_graphs=NUM_GRAPHS, n_min=3, n_max=21):
    """-> PackedGraphs of a seeded split: 'zinc' (regression labels), 'mutag' (class labels), 'pattern' (node labels)"""
    labels = {'zinc': 'regression', 'mutag': 'class', 'pattern': 'node'}[kind]
    ds = D.SyntheticGraphDataset(kind, num_graphs, in_dim=f, seed=7, pos_enc=False, with_eig=False, n_min=n_min,
                                 n_max=n_max, labels=labels, nb_class=3)
    if kind == 'pattern':
        for g in ds.samples:
            g.y = g.y % 3
    return D.PackedGraphs(ds.samples)


def pick_ids(packed, n_pad, bsz, seed, repeat=False):
    """bsz ids of graphs that fit n_pad, in a seeded random order (not ascending); repeat: one id twice"""
    fits = np.nonzero(packed.n <= n_pad)[0]
    ids = np.random.default_rng(seed).permutation(fits)[:bsz]
    assert len(ids) == bsz
    if repeat:
        ids[-1] = ids[0]
    return ids


def poisoned(store, bsz, n_pad, dtype=torch.float32):
    """output buffers of one launch with every byte 0xFF (NaN as a float, -1 as an integer): an element the launch
    does not write fails the comparison"""
    bufs = GatherBuffers(store, bsz, n_pad, dtype)
    for t in vars(bufs).values():
        if torch.is_tensor(t) and t is not bufs.ids:
            t.view(torch.uint8).fill_(0xFF)
    return bufs


def staged_labels(packed, batch9, bsz, n_pad):
    return T.pad_node_labels(batch9[5], batch9[8], bsz, n_pad) if packed.node_labels else batch9[5]


def assert_same(name, got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, ref.dtype, got.shape, ref.shape)
    assert torch.equal(got, ref), '%s differs: %d elements' % (name, int((got != ref).sum()))


def check_gather_equals_stager(dev, run_ctx, kind, f, n_pad, bsz, repeat=False, num_graphs=NUM_GRAPHS, n_max=21):
    """x, mask, degree, degree_rows, labels, n_real and node_off of one launch into poisoned buffers == the tensors of
    BatchStager.stage(ids), bit for bit (node labels: pad_node_labels of the stager's output)"""
    packed = packed_split(kind, f, num_graphs, 3, n_max)
    ids = pick_ids(packed, n_pad, bsz, seed=bsz + n_pad, repeat=repeat)
    with run_ctx():
        store = DeviceGraphStore(packed, dev, buckets=(16, 32, 64))
        bufs = store.gather_into(poisoned(store, bsz, n_pad), store.device_ids(ids))
        ref9, refc = D.BatchStager(packed, bsz, n_pad, dev).stage(ids)
    got9, gotc = bufs.batch9(), bufs.cache()
    for name, i in (('x', 0), ('mask', 1), ('degree', 4)):
        assert_same(name, got9[i], ref9[i])
    assert got9[2] is None and got9[3] is None and got9[6] is None and got9[7] is None and got9[8] is None
    assert_same('labels', got9[5], staged_labels(packed, ref9, bsz, n_pad))
    assert_same('n_real', gotc.n_real, refc.n_real)
    assert_same('node_off', gotc.node_off, refc.node_off)
    assert_same('degree_rows', gotc.extra['degree_rows'], refc.extra['degree_rows'])
    assert gotc.n_pad == n_pad and gotc.u is None and gotc.lam is None


@functools.lru_cache(maxsize=None)
def _spectral_pair(dev_str, f):
    """(packed, store) with the spectral fields, built in chunks of 8 graphs (three chunks in the bucket of 16, one in 32);
    built once per device under whichever backend is active and then only read"""
    packed = packed_split('zinc', f)
    return packed, DeviceGraphStore(packed, torch.device(dev_str), build_batch=8, **SPECTRAL)


def check_spectral_fields(dev, run_ctx, f, n_pad, bsz=8):
    """pe, u, lam, lap (and the plain fields) of store.batch(ids) == those of BatchStager(same options).stage(ids), bit for
    bit, for ids that mix graphs of different build chunks and of both buckets.  The store staged every graph at the padded
    size of its BUCKET (16 or 32) with other neighbours than the batch under test has, at n_pad = 21 with another padded
    size too: equality holds because eigh_jacobi_kernel and spectral_fn_kernel work per graph on its n_real block (the
    emulation confirms it).  The stager leaves zeros in the padded rows and columns of pe, u, lam and lap (feta_eigh_sym and
    feta_spectral_kernel write them), so does the gather: whole tensors are compared, nothing is masked out."""
    with run_ctx():
        packed, store = _spectral_pair(str(dev), f)
        ids = pick_ids(packed, n_pad, bsz, seed=3)
        chunk = {int(g): int(np.nonzero(store.bucket_ids(int(store.bucket[g])) == g)[0][0]) // 8 for g in ids}
        assert len(set(chunk.values())) > 1 and len(set(store.bucket[ids].tolist())) > 1, 'ids of one chunk / bucket only'
        got9, gotc = store.batch(ids, n_pad=n_pad)
        ref9, refc = D.BatchStager(packed, bsz, n_pad, dev, **SPECTRAL).stage(ids)
    for name, i in (('x', 0), ('mask', 1), ('pe', 2), ('lap', 3), ('degree', 4), ('labels', 5)):
        assert_same(name, got9[i], ref9[i])
    assert_same('u', gotc.u, refc.u)
    assert_same('lam', gotc.lam, refc.lam)
    assert float(got9[2].abs().max()) > 0 and float(gotc.u.abs().max()) > 0 and float(got9[3].abs().max()) > 0


def check_bf16_output(dev, run_ctx, f, n_pad, bsz=8):
    """x and pe emitted as FETA_BF16 == .to(torch.bfloat16) (round to nearest even) of the fp32 launch; the rest unchanged"""
    with run_ctx():
        packed, store = _spectral_pair(str(dev), f)
        ids = store.device_ids(pick_ids(packed, n_pad, bsz, seed=5))
        lo = store.gather_into(poisoned(store, bsz, n_pad, torch.bfloat16), ids)
        hi = store.gather_into(poisoned(store, bsz, n_pad), ids)
    assert_same('x', lo.x, hi.x.to(torch.bfloat16))
    assert_same('pe', lo.pe, hi.pe.to(torch.bfloat16))
    for name in ('mask', 'degree', 'degree_rows', 'u', 'lam', 'lap', 'n_real', 'node_off', 'labels'):
        assert_same(name, getattr(lo, name), getattr(hi, name))


def check_invalid_ids(dev, run_ctx, kind='zinc'):
    """ids -1 and G and a graph larger than N_pad give empty graphs (n_real 0, all masked, zeros, label 0 / -100) in their
    slots, the other slots hold what a launch on the valid ids alone puts there, and every element is written.
    HOST EMULATION ONLY: an out-of-bounds read is caught there and must never be tried on a shared GPU."""
    n_pad, f = 16, 28
    with run_ctx():
        if kind == 'zinc':
            packed, store = _spectral_pair(str(dev), f)
        else:
            packed = packed_split(kind, f)
            store = DeviceGraphStore(packed, dev)
        small = np.nonzero(packed.n <= n_pad)[0]
        big = int(np.nonzero(packed.n > n_pad)[0][0])
        slots = [int(small[4]), -1, int(small[1]), store.num_graphs, big, int(small[7])]
        valid = [0, 2, 5]
        bufs = store.gather_into(poisoned(store, len(slots), n_pad), store.device_ids(slots))
        ref = store.gather_into(poisoned(store, len(valid), n_pad), store.device_ids([slots[i] for i in valid]))
    empty = [i for i in range(len(slots)) if i not in valid]
    assert bufs.n_real.tolist() == [int(packed.n[slots[i]]) if i in valid else 0 for i in range(len(slots))]
    assert_same('node_off', bufs.node_off, (torch.cumsum(bufs.n_real, 0) - bufs.n_real).to(torch.int32))
    assert bool(bufs.mask[empty].all())
    rows = bufs.degree_rows.view(n_pad, len(slots))
    assert_same('degree_rows', rows[:, valid], ref.degree_rows.view(n_pad, len(valid)))
    assert float(rows[:, empty].abs().max()) == 0.0
    for name in ('x', 'mask', 'degree', 'pe', 'u', 'lam', 'lap', 'labels'):
        t = getattr(bufs, name)
        if t is None:
            continue
        assert_same(name, t[valid], getattr(ref, name))
        if name == 'labels':
            assert bool((t[empty] == (-100 if packed.node_labels else 0)).all())
        elif name != 'mask':
            assert float(t[empty].abs().max()) == 0.0, name      # (NaN - an unwritten element - fails too)


def check_descriptor(abi, dev, stream):
    """feta_batch_gather refuses a bad descriptor with FETA_E_ARG (ValueError, with a message) before any launch"""
    import pytest
    packed = packed_split('zinc', 6)
    ids = torch.zeros(4, dtype=torch.int32, device=dev)
    n = torch.from_numpy(packed.n.astype(np.int32)).to(dev)
    off = torch.from_numpy(np.asarray(packed.node_off[:-1], np.int64)).to(dev)
    sx = torch.from_numpy(packed.x).to(dev)
    x = torch.empty(4, 21, 6, device=dev)
    u = torch.empty(4, 8, 12, device=dev)
    good = dict(s_x=sx, s_n=n, s_node_off=off, ids=ids, x=x)
    call = lambda b=4, npad=21, dtype=0, k=0, **ptrs: abi.batch_gather(len(packed.n), b, npad, stream, f=6, k=k, dtype=dtype, **ptrs)
    call(**good)       # (the descriptor the bad ones are derived from is accepted)
    for kw, msg in ((dict(good, s_n=None), 's_n'), (dict(good, ids=None), 'ids'), (dict(good, s_x=None), 's_x'),
                    (dict(good, b=0), 'B = 0'), (dict(good, b=-3), 'B = -3'), (dict(good, dtype=7), 'dtype 7'),
                    (dict(good, npad=8, k=12, u=u, s_u=sx), 'K = 12'), (dict(good, pe=x), 's_pe'),
                    (dict(good, degree=x), 's_degree'), (dict(good, labels=x), 'label')):
        with pytest.raises(ValueError, match='batch_gather.*' + msg):
            call(**kw)


def check_struct_layout():
    """struct feta_gather of the header has the same fields, in the same order and of the same kind, as _abi.Gather
    (test_abi.test_descriptor_layouts_agree for the new descriptor)"""
    from test_abi import _header_structs
    kinds = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_int64: 'int64'}
    got = [(n.rstrip('_'), kinds[t]) for n, t in _abi.Gather._fields_]
    assert got == _header_structs()['feta_gather']


# ---- the training step fed by the store -----------------------------------------------------------------------------------

def trajectory_case(task, dev, bf16=False, layers=2, bsz=4, num_graphs=NUM_GRAPHS, heads=4):
    """two models of train_checks.build_case with the same initial weights (d = 64 as 4 heads of 16 or 8 of 8: the fused stack's
    shapes; filter_mode='spectral'), a split of their input width, its store and a stager with the same options, and three
    different batches of bsz ids out of the bucket of 16 (the third reuses graphs of the first two)"""
    kind, f = ('pattern', 5) if task == 'sbm' else ('mutag', 7)
    kw = dict(d=64, heads=heads, mode='spectral', batch_norm=False, layers=layers)
    model_a, _, _ = TC.build_case(task, dev, **kw)
    model_b, _, _ = TC.build_case(task, dev, **kw)
    model_b.load_state_dict(model_a.state_dict())
    if bf16:
        from feta_tmlr_amd.transformer.layers import set_storage_dtype
        set_storage_dtype(model_a, torch.bfloat16)
        set_storage_dtype(model_b, torch.bfloat16)
    packed = packed_split(kind, f, num_graphs, 6 if task == 'sbm' else 3, 21)
    opts = dict(pos_enc='diffusion', k_eig=8)
    store = DeviceGraphStore(packed, dev, build_batch=8, **opts)
    stager = D.BatchStager(packed, bsz, 16, dev, **opts)
    members = np.random.default_rng(11).permutation(store.bucket_ids(16))
    assert len(members) > 2 * bsz
    id_sets = [members[0:bsz], members[bsz:2 * bsz], members[[2 * bsz, 1, 2 * bsz - 1, 0][:bsz]]]
    return model_a, model_b, store, stager, id_sets


def compare_trajectories(task, model_a, model_b, opt_a, losses_a, losses_b, lrs, bf16=False):
    """losses of every step and the parameters after the steps: 3e-5 relative, the bars of tests/test_train_gpu.py
    (bf16 storage: bench_checks.BF16_MODEL_TOL); elements whose gradient is rounding noise take Adam steps of arbitrary
    sign and are bounded by the step size, as there"""
    import bench_checks as BC
    tol = BC.BF16_MODEL_TOL if bf16 else 3e-5
    for i, (la, lb) in enumerate(zip(losses_a, losses_b)):
        KC.assert_close('%s loss of step %d' % (task, i), lb.float().cpu(), la.float().cpu().double(), tol=tol)
    for (k, pa), (_, pb) in zip(model_a.named_parameters(), model_b.named_parameters()):
        if pa not in opt_a.state:
            assert torch.equal(pa, pb), k
            continue
        sig = opt_a.state[pa]['exp_avg'].abs() > 1e-6
        assert float((pa.detach() - pb.detach()).abs().max()) <= len(lrs) * max(lrs) * 1.01, k
        if sig.any():
            KC.assert_close('param ' + k, pb.detach()[sig].cpu(), pa.detach()[sig].cpu().double(), tol=tol)


LRS = (1e-3, 5e-4, 2e-3)


def reference_steps(task, model_a, stager, id_sets, crit):
    opt_a = T.make_optimizer(task, model_a.parameters(), lr=LRS[0])
    losses = [T.train_step(task, model_a, crit, opt_a, *stager.stage(ids), lr=lr).clone() for ids, lr in zip(id_sets, LRS)]
    return opt_a, losses


def check_trajectory_eager(task, dev, run_ctx, abi, bf16=False):
    """three steps of train_step on store.batch(ids) == three steps of train_step on BatchStager.stage(ids); every store
    step makes exactly ONE batch_gather call, no eigh_sym / lhat_from_edges / spectral_kernel call, and its forward
    takes the fused stack (one encoder layer, batches of 2 out of 12 graphs, and on fp32 storage 8 heads of 8 - the other
    fused shape, whose coefficient generator is 16 times smaller: the emulation runs every lane as a host fiber)"""
    crit = T.make_criterion(task, nb_class=3)
    with run_ctx():
        model_a, model_b, store, stager, id_sets = trajectory_case(task, dev, bf16, layers=1, bsz=2, num_graphs=12,
                                                                    heads=4 if bf16 else 8)
        opt_a, losses_a = reference_steps(task, model_a, stager, id_sets, crit)
        opt_b = T.make_optimizer(task, model_b.parameters(), lr=LRS[0])
        losses_b = []
        for ids, lr in zip(id_sets, LRS):
            with counted_calls(abi, FEED_NAMES) as calls:
                batch9, cache = store.batch(ids)
                losses_b.append(T.train_step(task, model_b, crit, opt_b, batch9, cache, lr=lr,
                                             padded_node_labels=task == 'sbm').clone())
            assert calls.get('batch_gather') == 1 and calls.get('attn_block_fwd', 0) > 0, calls
            assert not any(k in calls for k in ('eigh_sym', 'lhat_from_edges', 'spectral_kernel')), calls
    compare_trajectories(task, model_a, model_b, opt_a, losses_a, losses_b, LRS, bf16)


def check_trajectory_graphed(task, dev, abi, bf16=False, warmup_iters=3):
    """three replays of a captured StoreTrainStep == three steps of train_step on BatchStager.stage(ids).  Every step body
    the construction runs (warm-up + capture) makes exactly one batch_gather call and none of the spectrum producers and
    takes the fused stack; a replay makes NO call into the library from the host at all: the whole step, the gather
    included, is the hipGraph, and what the host sends is the ids."""
    crit = T.make_criterion(task, nb_class=3)
    model_a, model_b, store, stager, id_sets = trajectory_case(task, dev, bf16)
    opt_a, losses_a = reference_steps(task, model_a, stager, id_sets, crit)
    opt_b = T.make_optimizer(task, model_b.parameters(), lr=LRS[0], capturable=True)
    from feta_tmlr_amd import functional as FF
    try:
        _graphed_steps(task, abi, bf16, warmup_iters, crit, model_a, model_b, store, id_sets, opt_a, losses_a, opt_b)
    finally:
        FF.DropoutState.end_device_mode()


def _graphed_steps(task, abi, bf16, warmup_iters, crit, model_a, model_b, store, id_sets, opt_a, losses_a, opt_b):
    with counted_calls(abi, FEED_NAMES) as calls:
        step = T.StoreTrainStep(task, model_b, crit, opt_b, store, 16, 4, warmup_iters=warmup_iters)
    assert calls.get('batch_gather') == warmup_iters + 1 and calls.get('attn_block_fwd', 0) > 0, calls
    assert not any(k in calls for k in ('eigh_sym', 'lhat_from_edges', 'spectral_kernel')), calls
    assert isinstance(step.graph, torch.cuda.CUDAGraph)
    losses_b = []
    with counted_calls(abi, FEED_NAMES) as calls:
        for i, (ids, lr) in enumerate(zip(id_sets, LRS)):
            step.set_lr(lr)
            # a host sequence, and a slice of a device-resident id tensor
            losses_b.append(step(ids if i != 1 else store.device_ids(np.concatenate(id_sets))[4:8]).clone())
    assert not calls, calls
    assert len({float(l) for l in losses_b}) == 3            # three different batches went through the one graph
    compare_trajectories(task, model_a, model_b, opt_a, losses_a, losses_b, LRS, bf16)
    with __import__('pytest').raises(ValueError, match='exactly 4 ids'):
        step(id_sets[0][:3])


def check_snapshot_contract(dev):
    """a StoreTrainStep built mid-training leaves parameters, buffers, optimiser state and the DropoutState key where they
    were (the contract of GraphedTrainStep, tests/test_train_gpu.py)"""
    from feta_tmlr_amd import functional as FF
    task = 'zinc'
    model, _, _ = TC.build_case(task, dev, d=64, heads=4, mode='spectral', batch_norm=True)
    for layer in model.encoder.layers:
        layer.self_attn.dropout = 0.2
    model.train()
    packed = packed_split('zinc', 7)
    store = DeviceGraphStore(packed, dev, pos_enc='diffusion', k_eig=8)
    crit = T.make_criterion(task)
    opt = T.make_optimizer(task, model.parameters(), lr=1e-3, capturable=True)
    ids = store.bucket_ids(16)[:4]
    try:
        FF.DropoutState.manual_seed(77)
        T.train_step(task, model, crit, opt, *store.batch(ids))              # mid-training: moments and counters exist
        key = FF.DropoutState.snapshot()
        start = {k: v.clone() for k, v in model.state_dict().items()}
        opt_start = {p: {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()} for p, st in opt.state.items()}
        step = T.StoreTrainStep(task, model, crit, opt, store, 16, 4)
        assert step.drop_calls == len(model.encoder.layers)
        for k, v in model.state_dict().items():
            assert torch.equal(v, start[k]), k
        assert opt.state.keys() == opt_start.keys()
        for p, st in opt.state.items():
            for k, v in st.items():
                assert torch.equal(v, opt_start[p][k]) if torch.is_tensor(v) else v == opt_start[p][k], k
        assert FF.DropoutState.snapshot() == key
        step(ids)
        assert FF.DropoutState.snapshot() == (key[0], key[1] + step.drop_calls)
        assert any(not torch.equal(v, start[k]) for k, v in model.state_dict().items())
    finally:
        FF.DropoutState.end_device_mode()
