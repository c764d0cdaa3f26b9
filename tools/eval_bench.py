"""What the evaluation of a whole split costs (every training script of the reference evaluates the validation and test
splits after every epoch).  On a synthetic split of --graphs graphs in one bucket, cut into batches of B with a ragged tail:

    leg eager    today's path: train.evaluate(..., inference_mode=True) over store.batch(ids) batches - one gather launch,
                 the eager model and two to four host reads per batch.  Runs code this change does not touch: the yardstick
    leg store    train.StoreEvaluator.evaluate(): one small copy and one hipGraph replay per batch (train.StoreEvalStep),
                 one device read per split
    leg readout  the feta_readout_eval launch alone (50 launches per hipGraph replay, as tools/feed_bench.py times the gather)

Both evaluation legs also time the first half of the split (whole batches only); the time of one more batch is the
difference of the two divided by the difference in batches.  Both return the same dict; each process prints its own.

Shape: ZINC, 1000 graphs, B = 128, N_pad = 37, k_eig = 16, diffusion kernel, the BatchNorm task shell of
tools/feed_bench.py in fp32 (--dtype bf16: bf16 storage; --filter-mode cheb: the Chebyshev recursion on Lhat, the store keeps
lhat and no eigenpairs).  One leg per process and one JSON line per process; `--all` runs the two evaluation legs
alternately in fresh child processes, --runs times each (and the readout leg once), and prints medians and raw values.
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
ap.add_argument('--leg', default='store', choices=['eager', 'store', 'readout'])
ap.add_argument('--graphs', type=int, default=1000)
ap.add_argument('--batch', type=int, default=128)
ap.add_argument('--reps', type=int, default=200, help='timed evaluations of the split per process')
ap.add_argument('--dtype', default='f32', choices=['f32', 'bf16'])
ap.add_argument('--filter-mode', default='spectral', choices=['spectral', 'cheb'])
ap.add_argument('--all', action='store_true', help='legs eager and store in fresh processes, alternating (readout once)')
ap.add_argument('--runs', type=int, default=3)
args = ap.parse_args()
B, N_PAD = args.batch, 37
CHEB = args.filter_mode == 'cheb'
if CHEB and args.dtype == 'bf16':
    sys.exit("bf16 storage has no filter_mode='cheb' (transformer/models.py refuses it)")

if args.all:
    raw, per_batch, extra = {'eager': [], 'store': []}, {'eager': [], 'store': []}, {}
    base = [sys.executable, os.path.abspath(__file__), '--graphs', str(args.graphs), '--batch', str(B), '--reps', str(args.reps),
            '--dtype', args.dtype, '--filter-mode', args.filter_mode]
    for leg in ['readout'] + ['eager', 'store'] * args.runs:
        out = subprocess.run(base + ['--leg', leg], capture_output=True, text=True, timeout=600)
        if out.returncode != 0:       # nothing more is started on the device after a failure
            sys.exit('leg %s failed (%d):\n%s\n[...]\n%s' % (leg, out.returncode, out.stderr[:3000], out.stderr[-1500:]))
        res = json.loads(out.stdout.strip().splitlines()[-1])
        print(json.dumps(res), flush=True)
        if leg == 'readout':
            extra = res
        else:
            raw[leg].append(res['ms_per_split'])
            per_batch[leg].append(res['ms_per_batch'])
    med = {k: statistics.median(v) for k, v in raw.items()}
    print(json.dumps(dict(dtype=args.dtype, filter_mode=args.filter_mode, graphs=args.graphs, batch=B, n_pad=N_PAD,
                          reps=args.reps, raw_ms_per_split=raw, median_ms_per_split=med,
                          median_ms_per_batch={k: statistics.median(v) for k, v in per_batch.items()},
                          store_slowest_vs_eager_fastest=(max(raw['store']), min(raw['eager'])),
                          store_leads_cleanly=max(raw['store']) < min(raw['eager']), readout_us=extra.get('readout_us'))))
    sys.exit(0)

import numpy as np                                                   # noqa: E402
import torch                                                         # noqa: E402

from feta_tmlr_amd import functional as FF                          # noqa: E402
from feta_tmlr_amd import train as T                                # noqa: E402
from feta_tmlr_amd.transformer import data as D                     # noqa: E402
from feta_tmlr_amd.transformer import models as M                   # noqa: E402
from feta_tmlr_amd.transformer.store import DeviceGraphStore        # noqa: E402

dev = torch.device('cuda:0')
torch.manual_seed(0)
task = 'zinc'
split = D.SyntheticGraphDataset('zinc', args.graphs, in_dim=28, seed=1, pos_enc=False, with_eig=False)
model = M.DiffGraphTransformerGenGCN(28, 1, 64, 4, dim_feedforward=128, dropout=0.0, nb_layers=3, batch_norm=True,
                                     filter_order=4, heads_share_graph=True, filter_mode=args.filter_mode).to(dev)
if args.dtype == 'bf16':
    from feta_tmlr_amd.transformer.layers import set_storage_dtype
    set_storage_dtype(model, torch.bfloat16)
model.train()
crit = T.make_criterion(task)
opts = dict(pos_enc='diffusion', lhat=True) if CHEB else dict(pos_enc='diffusion', k_eig=16)
store = DeviceGraphStore(D.PackedGraphs(split.samples), dev, buckets=(N_PAD,), **opts)
evaluator = T.StoreEvaluator(task, model, crit, store, B)
half_ids = np.arange((args.graphs // B // 2) * B)
cuts = {'whole': (None, evaluator.batches()), 'half': (half_ids, evaluator.batches(half_ids))}
WARM = 3


def timed(run):
    """ms per call over args.reps calls (each ends in a host read of the results), after WARM calls"""
    for _ in range(WARM):
        out = run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        out = run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.reps * 1e3, out


res = dict(leg=args.leg, dtype=args.dtype, filter_mode=args.filter_mode, graphs=args.graphs, batch=B, n_pad=N_PAD,
           reps=args.reps, batches=len(cuts['whole'][1]))
if args.leg == 'readout':
    per = 50
    n_real = store.n[:B].contiguous()
    ids = torch.arange(B + 1, dtype=torch.int32, device=dev)
    ids[B] = B
    rows = [torch.randn(N_PAD, B, 64, device=dev) for _ in range(2)]
    labels = store.y[:B].contiguous()
    head = model.classifier
    w = [p.detach() for p in (head[0].weight, head[0].bias, head[2].weight, head[2].bias)]
    launch = lambda i: FF.readout_eval(rows[i & 1], n_real, ids, ids[B:], labels, *w, evaluator.scores, evaluator.terms, 'l1', 0.0)
    launch(0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(per):
            launch(i)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        graph.replay()
    torch.cuda.synchronize()
    res['readout_us'] = (time.perf_counter() - t0) / (20 * per) * 1e6
else:
    ms = {}
    for name, (ids, cut) in cuts.items():
        if args.leg == 'eager':
            run = lambda cut=cut: T.evaluate(task, model, crit, (store.batch(b, n_pad) for n_pad, b in cut), inference_mode=True)
        else:
            run = lambda ids=ids: evaluator.evaluate(ids)
        ms[name], out = timed(run)
        res['result_' + name] = out
    extra = len(cuts['whole'][1]) - len(cuts['half'][1])
    res.update(ms_per_split=ms['whole'], ms_per_half=ms['half'], ms_per_batch=(ms['whole'] - ms['half']) / extra,
               graphs_per_s=args.graphs / (ms['whole'] * 1e-3))
print(json.dumps(res))
