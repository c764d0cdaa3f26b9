"""What a training loop pays per step once every step needs a NEW batch (bench.py and tools/train_bench.py time a step on
one resident batch).  On a synthetic split of 8 * B graphs and --steps distinct id sets:

    leg A   today's feed: data.BatchStager.stage(ids) (numpy gathers, ~10 host-to-device copies, the spectrum of the
            batch recomputed on the device) + train.GraphedTrainStep(batch9, cache) (~10 copies into static buffers)
    leg B   train.StoreTrainStep(ids): the ids go to the device, one hipGraph replay does the rest - the batch is
            gathered from a transformer.store.DeviceGraphStore by the first launch of the graph
    leg C   GraphedTrainStep replayed on ONE resident batch: the floor
    gather  the feta_batch_gather launch alone (50 launches per hipGraph replay, so that no host launch cost is in it)

Shape: ZINC, B = 128, N_pad = 37, k_eig = 16, diffusion kernel, the BatchNorm task shell of tools/train_bench.py
(--dtype bf16: bf16 storage).  `--filter-mode cheb` switches the model of all three legs to the Chebyshev recursion on Lhat
and the store to lhat=True without eigenpairs (the gather is then feta_batch_gather_ex; the `gather` leg also times the
same store's launch without lhat).  `--shape molhiv` (B = 1024, one N_pad = 64 bucket, atom features, lap_dim 8) exists for the
`gather` leg only: its leg A aborted on the MI355X at interpreter exit the one time it was run, the cause is not known,
and the training legs of that shape are refused until it is (EXPERIMENTS.md).  One leg per process and one JSON line per
process; `--all` runs the legs alternately in fresh child processes, --runs times each, and prints medians and raw values.
`--fused-head` builds leg B's StoreTrainStep with fused_head=True (pooling, classifier, loss and their backward in
functional.readout_train, four launches); legs A, C and gather do not change.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument('--shape', default='zinc', choices=['zinc', 'molhiv'])
ap.add_argument('--leg', default='B', choices=['A', 'B', 'C', 'gather'])
ap.add_argument('--steps', type=int, default=200)
ap.add_argument('--batch', type=int, default=0, help='default: 128 (zinc) / 1024 (molhiv)')
ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
ap.add_argument('--filter-mode', default='spectral', choices=['spectral', 'cheb'],
                help="cheb: the Chebyshev recursion on Lhat - the store keeps lhat and no eigenpairs (f32 storage only)")
ap.add_argument('--all', action='store_true', help='legs A, B, C (and gather once) in fresh processes, alternating')
ap.add_argument('--runs', type=int, default=3)
ap.add_argument('--fused-head', action='store_true', help='leg B: StoreTrainStep(..., fused_head=True)')
args = ap.parse_args()
B = args.batch or (128 if args.shape == 'zinc' else 1024)
N_PAD = 37 if args.shape == 'zinc' else 64
CHEB = args.filter_mode == 'cheb'
if args.shape == 'molhiv' and (args.all or args.leg != 'gather'):
    sys.exit('--shape molhiv runs --leg gather only (see the module docstring)')
if CHEB and args.dtype == 'bf16':
    sys.exit("bf16 storage has no filter_mode='cheb' (transformer/models.py refuses it)")

if args.all:
    raw = {'A': [], 'B': [], 'C': []}
    extra = {}
    base = [sys.executable, os.path.abspath(__file__), '--shape', args.shape, '--steps', str(args.steps), '--batch', str(B),
            '--dtype', args.dtype, '--filter-mode', args.filter_mode] + (['--fused-head'] if args.fused_head else [])
    for leg in ['gather'] + ['A', 'B', 'C'] * args.runs:
        out = subprocess.run(base + ['--leg', leg], capture_output=True, text=True, timeout=900)
        if out.returncode != 0:       # nothing more is started on the device after a failure
            sys.exit('leg %s failed (%d):\n%s\n[...]\n%s' % (leg, out.returncode, out.stderr[:3000], out.stderr[-1500:]))
        res = json.loads(out.stdout.strip().splitlines()[-1])
        print(json.dumps(res), flush=True)
        if leg == 'gather':
            extra = res
        else:
            raw[leg].append(res['ms_per_step'])
    med = {k: statistics.median(v) for k, v in raw.items()}
    print(json.dumps(dict(shape=args.shape, dtype=args.dtype, filter_mode=args.filter_mode, batch=B, n_pad=N_PAD,
                          steps=args.steps, fused_head=args.fused_head, raw_ms=raw, median_ms=med,
                          graphs_per_s={k: B / (v * 1e-3) for k, v in med.items()},
                          b_slowest_vs_a_fastest=(max(raw['B']), min(raw['A'])), b_minus_c_ms=med['B'] - med['C'],
                          c_spread_ms=max(raw['C']) - min(raw['C']), gather_us=extra.get('gather_us'),
                          gather_bf16_us=extra.get('gather_bf16_us'), gather_no_lhat_us=extra.get('gather_no_lhat_us'),
                          store_build_s=extra.get('store_build_s'),
                          store_nbytes=extra.get('store_nbytes'), store_bytes_per_graph=extra.get('store_bytes_per_graph'))))
    sys.exit(0)

import numpy as np                                                   # noqa: E402
import torch                                                         # noqa: E402

from feta_tmlr_amd import train as T                                # noqa: E402
from feta_tmlr_amd.transformer import data as D                     # noqa: E402
from feta_tmlr_amd.transformer import models as M                   # noqa: E402
from feta_tmlr_amd.transformer.store import DeviceGraphStore, GatherBuffers   # noqa: E402

dev = torch.device('cuda:0')
torch.manual_seed(0)
if args.shape == 'zinc':
    task, opts = 'zinc', dict(pos_enc='diffusion', k_eig=16)
    split = D.SyntheticGraphDataset('zinc', 8 * B, in_dim=28, seed=1, pos_enc=False, with_eig=False)
    model = M.DiffGraphTransformerGenGCN(28, 1, 64, 4, dim_feedforward=128, dropout=0.0, nb_layers=3, batch_norm=True,
                                         filter_order=4, heads_share_graph=True, filter_mode=args.filter_mode)
else:
    task, opts = 'molhiv', dict(pos_enc='diffusion', k_eig=16, lap_dim=8)
    split = D.SyntheticGraphDataset('molhiv', 8 * B, seed=1, pos_enc=False, with_eig=False, n_max=N_PAD, features='atom',
                                    labels='binary', nan_label_frac=0.1)
    model = M.DiffGraphTransformerGenGCNMolHiv(9, 1, 64, 4, dim_feedforward=128, dropout=0.0, nb_layers=3, batch_norm=False,
                                               lap_pos_enc=True, lap_pos_enc_dim=8, filter_order=4, heads_share_graph=True,
                                               filter_mode=args.filter_mode)
if CHEB:                              # the operator reads lhat: no eigenpairs are kept, the store holds the Laplacians
    opts.pop('k_eig')
model = model.to(dev)
if args.dtype == 'bf16':
    from feta_tmlr_amd.transformer.layers import set_storage_dtype
    set_storage_dtype(model, torch.bfloat16)
model.train()
crit = T.make_criterion(task)
opt = T.make_optimizer(task, model.parameters(), lr=1e-3, capturable=True)
packed = D.PackedGraphs(split.samples)
rng = np.random.default_rng(0)
WARM = 20
id_sets = [rng.choice(len(split), size=B, replace=False).astype(np.int32) for _ in range(args.steps + WARM)]


def timed(step):
    """ms per step over args.steps steps on distinct id sets, after WARM steps"""
    for ids in id_sets[:WARM]:
        step(ids)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for ids in id_sets[WARM:]:
        step(ids)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps * 1e3


res = dict(leg=args.leg, shape=args.shape, dtype=args.dtype, filter_mode=args.filter_mode, batch=B, n_pad=N_PAD,
           steps=args.steps)
if args.leg == 'B':
    res['fused_head'] = args.fused_head
if args.leg in ('A', 'C'):
    stager = D.BatchStager(packed, B, N_PAD, dev, **opts)
    batch9, cache = stager.stage(id_sets[0])
    graphed = T.GraphedTrainStep(task, model, crit, opt, batch9, cache)
    graphed.set_lr(1e-3)
    if args.leg == 'A':
        ms = timed(lambda ids: graphed(*stager.stage(ids)))
    else:
        resident = tuple(None if t is None else t.clone() for t in batch9), cache
        ms = timed(lambda ids: graphed(*resident))
else:
    store = DeviceGraphStore(packed, dev, buckets=(N_PAD,), lhat=CHEB, **opts)
    res.update(store_build_s=store.build_seconds, store_nbytes=store.nbytes,
               store_bytes_per_graph=store.nbytes / store.num_graphs)
    if args.leg == 'B':
        step = T.StoreTrainStep(task, model, crit, opt, store, N_PAD, B, fused_head=args.fused_head)
        step.set_lr(1e-3)
        ms = timed(step)
        dev_sets = [store.device_ids(ids) for ids in id_sets]
        torch.cuda.synchronize()
        host_sets, id_sets = id_sets, dev_sets
        res['ms_per_step_device_ids'] = timed(step)
        id_sets = host_sets
    else:
        per = 50
        # (cheb: the launch is feta_batch_gather_ex and emits lhat too; gather_no_lhat_us is the same store's plain launch)
        kinds = [('gather_us', torch.float32, None), ('gather_bf16_us', torch.bfloat16, None)]
        if CHEB:
            kinds.append(('gather_no_lhat_us', torch.float32, False))
        for key, dt, with_lhat in kinds:
            bufs = [GatherBuffers(store, B, N_PAD, dt, lhat=with_lhat) for _ in range(2)]
            ids_d = [store.device_ids(ids) for ids in id_sets[:per]]
            store.gather_into(bufs[0], ids_d[0])
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for i in range(per):
                    store.gather_into(bufs[i & 1], ids_d[i])
            for _ in range(3):
                graph.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                graph.replay()
            torch.cuda.synchronize()
            res[key] = (time.perf_counter() - t0) / (20 * per) * 1e6
        ms = res['gather_us'] * 1e-3
res.update(ms_per_step=ms, graphs_per_s=B / (ms * 1e-3))
print(json.dumps(res))
