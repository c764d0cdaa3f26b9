"""Checks of what the device-resident graph store feeds beyond the spectral mode: the dense scaled Laplacian of
filter_mode='cheb' and the per-batch sign flip of the Laplacian eigenvector features (feta_batch_gather_ex,
csrc/gather.hip; DeviceGraphStore(..., lhat=True); train.StoreTrainStep(..., lap_sign_flip=True)).  The reference is what
the project did before: ``functional.lhat_from_edges`` of ``data.BatchStager.stage(ids)``, ``train.lap_sign_flip`` of the
staged lap, ``train.train_step`` on the staged batch.  The synthetic graphs have unique, symmetrised edges, so every
entry of Lhat receives one contribution and bit equality is the bar.  Written once, run on the host emulation
(test_store_cheb_emu.py) and on the MI355X (test_store_cheb_gpu.py)."""
import contextlib
import ctypes
import functools

import numpy as np
import torch

import store_checks as SC
import train_checks as TC
from heads8_checks import counted_calls
from store_checks import LRS, assert_same, compare_trajectories, packed_split, pick_ids, poisoned
from feta_tmlr_amd import _abi
from feta_tmlr_amd import functional as FF
from feta_tmlr_amd import train as T
from feta_tmlr_amd.transformer import data as D
from feta_tmlr_amd.transformer.store import DeviceGraphStore

F_IN = 6
BIG_BUCKETS = (16, 32, 64, 128)
OUTPUTS = ('x', 'mask', 'degree', 'degree_rows', 'pe', 'u', 'lam', 'lap', 'n_real', 'node_off', 'labels')
FEED_NAMES = SC.FEED_NAMES + ('batch_gather_ex',)


def G(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _store(dev_str, kind):
    """(packed, store, stager options), built once per device under whichever backend is active and then only read:
    'lhat'      the default split, lhat alone (no eigendecomposition)
    'edge'      lhat alone on 30 graphs of 1..21 nodes: the seeded split holds a single-node graph, one of 16 nodes and
                one of 21, which the default split does not
    'big'     6 graphs of 60..72 nodes in buckets (16, 32, 64, 128): N_pad = 72 / 75 have a second 64-row chunk
    'spectral'  the default split with pe, u / lam, lap (lap_dim 4) and lhat, built 8 graphs at a time: ids mix the
                build chunks and both buckets
    'lap3'      12 graphs with lap_dim 3 (the element path of lap) and nothing else"""
    dev = torch.device(dev_str)
    if kind == 'big':
        packed = packed_split('zinc', F_IN, 6, 60, 72)
        return packed, DeviceGraphStore(packed, dev, buckets=BIG_BUCKETS, lhat=True), {}
    if kind == 'edge':
        packed = packed_split('zinc', F_IN, 30, 1, 21)
        assert {1, 16, 21} <= set(packed.n.tolist())
        return packed, DeviceGraphStore(packed, dev, lhat=True), {}
    if kind == 'lap3':
        packed = packed_split('zinc', F_IN, 12)
        return packed, DeviceGraphStore(packed, dev, lap_dim=3), dict(lap_dim=3)
    packed = packed_split('zinc', F_IN)
    if kind == 'spectral':
        return packed, DeviceGraphStore(packed, dev, build_batch=8, lhat=True, **SC.SPECTRAL), dict(SC.SPECTRAL)
    return packed, DeviceGraphStore(packed, dev, lhat=True), {}


def edge_ids(packed, n_pad, bsz, seed):
    """pick_ids with one id repeated and, where the split has them, a single-node graph and one that fills n_pad"""
    ids = pick_ids(packed, n_pad, bsz, seed, repeat=True)
    for slot, n in ((1, n_pad), (2, 1)):
        hit = np.nonzero(packed.n == n)[0]
        if len(hit) and slot < bsz - 1:
            ids[slot] = hit[0]
    return ids


def plain_launch(store, bsz, n_pad, ids):
    """feta_batch_gather of the same ids into poisoned buffers (no lhat, no signs)"""
    bufs = poisoned(store, bsz, n_pad)
    bufs.lhat = None
    return store.gather_into(bufs, ids)


def assert_outputs_same(got, ref, names=OUTPUTS):
    for name in names:
        a, b = getattr(got, name), getattr(ref, name)
        assert (a is None) == (b is None), name
        if a is not None:
            assert_same(name, a, b)


def check_lhat_equals_stager(dev, run_ctx, abi, kind, n_pad, bsz):
    """lhat of ONE batch_gather_ex launch into poisoned buffers == functional.lhat_from_edges of BatchStager.stage(ids)
    over the whole [B, N, N] tensor (the padding included), every other output == the plain launch's"""
    with run_ctx():
        packed, store, _ = _store(str(dev), kind)
        ids = edge_ids(packed, n_pad, bsz, seed=bsz + n_pad)
        assert len(set(ids.tolist())) < bsz
        ids_d = store.device_ids(ids)
        with counted_calls(abi, FEED_NAMES) as calls:
            bufs = store.gather_into(poisoned(store, bsz, n_pad), ids_d)
        assert calls == {'batch_gather_ex': 1}, calls
        plain = plain_launch(store, bsz, n_pad, ids_d)
        ref9, refc = D.BatchStager(packed, bsz, n_pad, dev).stage(ids)
        ref = FF.lhat_from_edges(ref9[6], ref9[7], refc.node_off, bsz, n_pad)
    assert bufs.lhat.dtype == torch.float32 and bufs.cache().lhat is bufs.lhat
    assert_same('lhat', bufs.lhat, ref)
    assert float(ref.abs().max()) > 0
    assert_outputs_same(bufs, plain)


def check_null_extras(dev, run_ctx, abi, n_pad, bsz=5):
    """feta_batch_gather_ex without lhat and lap_sign == feta_batch_gather on every output, bit for bit (the store with
    every field; the launch of gather_into is redirected to the _ex entry point)"""
    with run_ctx():
        packed, store, _ = _store(str(dev), 'spectral')
        ids_d = store.device_ids(edge_ids(packed, n_pad, bsz, seed=n_pad))
        plain = plain_launch(store, bsz, n_pad, ids_d)
        bufs = poisoned(store, bsz, n_pad)
        bufs.lhat = None
        orig = abi.batch_gather
        with counted_calls(abi, ('batch_gather_ex',)) as calls:
            abi.batch_gather = abi.batch_gather_ex
            try:
                store.gather_into(bufs, ids_d)
            finally:
                abi.batch_gather = orig
    assert calls == {'batch_gather_ex': 1}, calls
    assert_outputs_same(bufs, plain)


def mixed_sign_seed(lap_dim):
    """the first seed whose draw holds both signs"""
    for seed in range(64):
        if len(set(T.lap_signs(lap_dim, G(seed)).tolist())) == 2:
            return seed
    raise AssertionError('no seed with both signs')


def check_lap_sign(dev, run_ctx, kind, n_pad, bsz=5):
    """lap emitted with lap_sign = lap_signs(lap_dim, G(seed)) == train.lap_sign_flip(plain lap, G(seed)); the other outputs
    are the plain launch's.  'spectral': lap_dim 4, the vector path; 'lap3': lap_dim 3, element by element."""
    with run_ctx():
        packed, store, _ = _store(str(dev), kind)
        seed = mixed_sign_seed(store.lap_dim)
        signs = T.lap_signs(store.lap_dim, G(seed))
        assert sorted(set(signs.tolist())) == [-1.0, 1.0]
        ids_d = store.device_ids(edge_ids(packed, n_pad, bsz, seed=1 + n_pad))
        plain = plain_launch(store, bsz, n_pad, ids_d)
        bufs = poisoned(store, bsz, n_pad)
        bufs.lhat = None
        bufs.lap_sign = signs.to(dev)
        store.gather_into(bufs, ids_d)
        want = T.lap_sign_flip(plain.lap, generator=G(seed))
    assert float(plain.lap.abs().max()) > 0 and not torch.equal(want, plain.lap)
    assert_same('lap', bufs.lap, want)
    assert_outputs_same(bufs, plain, [k for k in OUTPUTS if k != 'lap'])


def check_invalid_ids(dev, run_ctx):
    """slots holding -1, G or a graph larger than N_pad get an all-zero lhat block, the other slots hold what a launch on
    the valid ids alone puts there.  HOST EMULATION ONLY (store_checks.check_invalid_ids: never tried on a shared GPU)."""
    n_pad = 16
    with run_ctx():
        packed, store, _ = _store(str(dev), 'lhat')
        small = np.nonzero(packed.n <= n_pad)[0]
        big = int(np.nonzero(packed.n > n_pad)[0][0])
        slots = [int(small[4]), -1, int(small[1]), store.num_graphs, big, int(small[7])]
        valid = [0, 2, 5]
        bufs = store.gather_into(poisoned(store, len(slots), n_pad), store.device_ids(slots))
        ref = store.gather_into(poisoned(store, len(valid), n_pad), store.device_ids([slots[i] for i in valid]))
    empty = [i for i in range(len(slots)) if i not in valid]
    assert_same('lhat', bufs.lhat[valid], ref.lhat)
    assert float(ref.lhat.abs().max()) > 0
    assert float(bufs.lhat[empty].abs().max()) == 0.0           # (NaN - an unwritten element - fails too)
    assert bufs.n_real.tolist() == [int(packed.n[slots[i]]) if i in valid else 0 for i in range(len(slots))]


def check_descriptor(abi, dev, stream):
    """feta_batch_gather_ex refuses lhat without s_lhat, lhat without s_pe_off and lap_sign without lap with FETA_E_ARG
    (ValueError, with a message) before any launch: the poisoned outputs stay as they were"""
    import pytest
    packed = packed_split('zinc', F_IN)
    g = len(packed.n)
    pitch = (packed.n + 3) & ~3
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n, off, sx = t(packed.n.astype(np.int32)), t(np.asarray(packed.node_off[:-1], np.int64)), t(packed.x)
    pe_off = t(np.concatenate([[0], np.cumsum(pitch * packed.n)])[:-1].astype(np.int64))
    s_lhat = torch.zeros(int((pitch * packed.n).sum()), device=dev)
    s_lap = torch.zeros(int(packed.n.sum()), 4, device=dev)
    ids = torch.zeros(4, dtype=torch.int32, device=dev)
    nan = lambda *shape: torch.full(shape, float('nan'), device=dev)
    x, lhat, lap, sign = nan(4, 21, F_IN), nan(4, 21, 21), nan(4, 21, 4), torch.ones(4, device=dev)
    base = dict(s_x=sx, s_n=n, s_node_off=off, ids=ids)
    call = lambda **ptrs: abi.batch_gather_ex(g, 4, 21, stream, f=F_IN, lap_dim=4, **ptrs)
    for kw, msg in ((dict(base, x=x, lhat=lhat, s_pe_off=pe_off), 'lhat needs s_lhat'),
                    (dict(base, x=x, lhat=lhat, s_lhat=s_lhat), 's_pe_off'),
                    (dict(base, x=x, lap_sign=sign, s_lap=s_lap), 'lap_sign needs lap'),
                    (dict(base, x=x, lhat=lhat, s_lhat=s_lhat, s_pe_off=pe_off, s_n=None), 's_n')):
        with pytest.raises(ValueError, match='batch_gather.*' + msg):
            call(**kw)
    assert bool(torch.isnan(x).all()) and bool(torch.isnan(lhat).all()) and bool(torch.isnan(lap).all())
    call(**dict(base, x=x, lhat=lhat, s_lhat=s_lhat, s_pe_off=pe_off, lap=lap, s_lap=s_lap, lap_sign=sign))   # accepted
    assert not bool(torch.isnan(x).any()) and float(lhat.abs().max()) == 0.0 and float(lap.abs().max()) == 0.0


def check_struct_layout():
    """struct feta_gather_ex of the header has the same fields, in the same order and of the same kind, as _abi.GatherEx,
    and begins with those of feta_gather"""
    from test_abi import _header_structs
    kinds = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_int64: 'int64'}
    got = [(n.rstrip('_'), kinds[t]) for n, t in _abi.GatherEx._fields_]
    structs = _header_structs()
    assert got == structs['feta_gather_ex']
    assert got[:-3] == structs['feta_gather'] and [n for n, _ in got[-3:]] == ['s_lhat', 'lhat', 'lap_sign']
    assert ctypes.sizeof(_abi.GatherEx) == ctypes.sizeof(_abi.Gather) + 3 * ctypes.sizeof(ctypes.c_void_p)


# ---- the training step fed by the store --------------------------------------------------------------------------------

def cheb_case(task, dev, share=1, layers=2, bsz=4, num_graphs=SC.NUM_GRAPHS, heads=4, lap_dim=0):
    """store_checks.trajectory_case with filter_mode='cheb': two models with the same weights, a split, its store (diffusion
    kernel, lhat, no eigenpairs kept) and a stager with the same options, three id sets out of the bucket of 16"""
    kind, f = ('pattern', 5) if task == 'sbm' else ('mutag', 7)
    kw = dict(d=64, heads=heads, mode='cheb', batch_norm=False, layers=layers, share=share, lap_dim=lap_dim)
    model_a, _, _ = TC.build_case(task, dev, **kw)
    model_b, _, _ = TC.build_case(task, dev, **kw)
    model_b.load_state_dict(model_a.state_dict())
    packed = packed_split(kind, f, num_graphs, 6 if task == 'sbm' else 3, 21)
    opts = dict(pos_enc='diffusion', lap_dim=lap_dim or None)
    store = DeviceGraphStore(packed, dev, build_batch=8, lhat=True, **opts)
    stager = D.BatchStager(packed, bsz, 16, dev, **opts)
    members = np.random.default_rng(11).permutation(store.bucket_ids(16))
    assert len(members) > 2 * bsz
    id_sets = [members[0:bsz], members[bsz:2 * bsz], members[[2 * bsz, 1, 2 * bsz - 1, 0][:bsz]]]
    return model_a, model_b, store, stager, id_sets


def reference_steps(task, model_a, stager, id_sets, crit, generator=None):
    """the eager loop of the reference: stage -> (lap_sign_flip of lap with ``generator``) -> train_step"""
    opt_a = T.make_optimizer(task, model_a.parameters(), lr=LRS[0])
    losses = []
    for ids, lr in zip(id_sets, LRS):
        batch9, cache = stager.stage(ids)
        if generator is not None:
            batch9 = batch9[:3] + (T.lap_sign_flip(batch9[3], generator=generator),) + batch9[4:]
        losses.append(T.train_step(task, model_a, crit, opt_a, batch9, cache, lr=lr).clone())
    return opt_a, losses


def check_trajectory_eager(task, share, dev, run_ctx, abi):
    """three train_steps on store.batch(ids) == three on BatchStager.stage(ids) for a filter_mode='cheb' model (one encoder
    layer, batches of 2 out of 12 graphs, 8 heads of 8); every store step makes ONE batch_gather_ex call, no batch_gather
    call and no lhat_from_edges call, and takes the fused stack"""
    crit = T.make_criterion(task, nb_class=3)
    with run_ctx():
        model_a, model_b, store, stager, id_sets = cheb_case(task, dev, share, layers=1, bsz=2, num_graphs=12, heads=8)
        assert model_b.encoder.filter_mode == 'cheb' and model_b.encoder.heads_share_graph == bool(share)
        opt_a, losses_a = reference_steps(task, model_a, stager, id_sets, crit)
        opt_b = T.make_optimizer(task, model_b.parameters(), lr=LRS[0])
        losses_b = []
        for ids, lr in zip(id_sets, LRS):
            with counted_calls(abi, FEED_NAMES) as calls:
                batch9, cache = store.batch(ids)
                losses_b.append(T.train_step(task, model_b, crit, opt_b, batch9, cache, lr=lr,
                                             padded_node_labels=task == 'sbm').clone())
            assert calls.get('batch_gather_ex') == 1 and calls.get('attn_block_fwd', 0) > 0, calls
            assert not any(k in calls for k in ('batch_gather', 'lhat_from_edges', 'eigh_sym', 'spectral_kernel')), calls
    compare_trajectories(task, model_a, model_b, opt_a, losses_a, losses_b, LRS)


def check_trajectory_graphed(task, share, dev, abi, lap_flip=False, warmup_iters=3):
    """three replays of a captured StoreTrainStep on a filter_mode='cheb' model == the eager reference (bucket 16, 4 ids,
    2 layers).  The construction makes one batch_gather_ex call per step body and none of batch_gather / lhat_from_edges;
    a replay makes NO library call from the host.  lap_flip: lap_dim = 4 and lap_sign_flip=True with generator G(5) against
    the eager loop that flips the staged lap with G(5); the construction leaves the generator where it was."""
    crit = T.make_criterion(task, nb_class=3)
    model_a, model_b, store, stager, id_sets = cheb_case(task, dev, share, lap_dim=4 if lap_flip else 0)
    opt_a, losses_a = reference_steps(task, model_a, stager, id_sets, crit, G(5) if lap_flip else None)
    opt_b = T.make_optimizer(task, model_b.parameters(), lr=LRS[0], capturable=True)
    gen = G(5) if lap_flip else None
    try:
        with counted_calls(abi, FEED_NAMES) as calls:
            step = T.StoreTrainStep(task, model_b, crit, opt_b, store, 16, 4, warmup_iters=warmup_iters,
                                    lap_sign_flip=lap_flip, generator=gen)
        assert calls.get('batch_gather_ex') == warmup_iters + 1 and calls.get('attn_block_fwd', 0) > 0, calls
        assert not any(k in calls for k in ('batch_gather', 'lhat_from_edges', 'eigh_sym', 'spectral_kernel')), calls
        if lap_flip:
            assert torch.equal(gen.get_state(), G(5).get_state())
            assert torch.equal(step.bufs.lap_sign.cpu(), torch.ones(4))
        losses_b = []
        with counted_calls(abi, FEED_NAMES) as calls:
            for i, (ids, lr) in enumerate(zip(id_sets, LRS)):
                step.set_lr(lr)
                # a host sequence, and a slice of a device-resident id tensor
                losses_b.append(step(ids if i != 1 else store.device_ids(np.concatenate(id_sets))[4:8]).clone())
        assert not calls, calls
        assert len({float(l) for l in losses_b}) == 3
        compare_trajectories(task, model_a, model_b, opt_a, losses_a, losses_b, LRS)
        if lap_flip:
            assert not torch.equal(gen.get_state(), G(5).get_state())
    finally:
        FF.DropoutState.end_device_mode()


def check_refusal(dev, run_ctx=contextlib.nullcontext):
    """a filter_mode='cheb' model on a store built without lhat is refused with the way out in the message; so is
    lap_sign_flip on a store without lap"""
    import pytest
    with run_ctx():
        model, _, _ = TC.build_case('tu', dev, d=64, heads=4, mode='cheb', batch_norm=False, layers=1)
        packed = packed_split('mutag', 7, 12)
        crit = T.make_criterion('tu', nb_class=3)
        opt = T.make_optimizer('tu', model.parameters(), lr=1e-3, capturable=True, fused=False)
        with pytest.raises(ValueError, match=r'lhat=True'):
            T.StoreTrainStep('tu', model, crit, opt, DeviceGraphStore(packed, dev), 16, 4)
        with pytest.raises(ValueError, match='lap_dim'):
            T.StoreTrainStep('tu', model, crit, opt, DeviceGraphStore(packed, dev, lhat=True), 16, 4, lap_sign_flip=True)
