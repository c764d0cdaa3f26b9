"""Eval forward per batch, eager: torch.no_grad() (the layer-by-layer / fused-training-kernel path) against
torch.inference_mode() (the encoder stack as ONE feta_encoder_infer launch) at config 2, the reference's ZINC default
(8 heads, 10 layers, BatchNorm), MUTAG with LayerNorm and the molhiv bucket (B = 1024, N = 64, BatchNorm and LayerNorm).
--dtype bf16: the same shapes on bf16 storage (layers.set_storage_dtype; inference_mode is then ONE
feta_encoder_infer_ex launch with bf16 tiles); the 8-head shape is skipped, bf16 storage has no d_h = 8 form.
--train-fwd: instead, forward + backward of the LayerNorm shapes in training mode with the one-launch forward of the stack
(feta_encoder_fwd_save, layers.set_one_launch_forward) off and on, alternating --alternations times; under
`rocprofv3 --kernel-trace --stats` that run holds the new launch beside the attn_block_fwd + ffn_fwd launches it replaces.
Prints one JSON line per shape.  Under `rocprofv3 --kernel-trace --stats -- python tools/infer_bench.py --train` the
kernel statistics also hold the training forward of config 2 (attn_block_fwd8 + ffn_fwd per layer) for comparison."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from feta_tmlr_amd.transformer import data as D                     # noqa: E402
from feta_tmlr_amd.transformer.layers import set_one_launch_forward, set_storage_dtype     # noqa: E402
from feta_tmlr_amd.transformer.models import DiffGraphTransformerGenGCN   # noqa: E402

SHAPES = {   # name: (dataset shape, B, N_pad, heads, layers, batch_norm)
    'config2': ('zinc', 128, 37, 4, 3, True),
    'zinc_default': ('zinc', 128, 37, 8, 10, True),
    'mutag_layernorm': ('mutag', 32, 28, 4, 3, False),
    'molhiv_batchnorm': ('molhiv', 1024, 64, 4, 3, True),
    'molhiv_layernorm': ('molhiv', 1024, 64, 4, 3, False),
    'config2_layernorm': ('zinc', 128, 37, 4, 3, False),          # (--train-fwd only)
    'zinc_default_layernorm': ('zinc', 128, 37, 8, 10, False),    # (--train-fwd only)
}
TRAIN_FWD = ('mutag_layernorm', 'config2_layernorm', 'zinc_default_layernorm', 'molhiv_layernorm')

ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=50)
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--shapes', default=None)
ap.add_argument('--dtype', choices=('f32', 'bf16'), default='f32', help='storage type of the model')
ap.add_argument('--train', action='store_true', help='also run training forward + backward steps at config 2')
ap.add_argument('--train-fwd', action='store_true',
                help='time training forward + backward of the LayerNorm shapes with the one-launch forward off and on')
ap.add_argument('--alternations', type=int, default=3)
args = ap.parse_args()
if args.shapes is None:
    args.shapes = ','.join(TRAIN_FWD if args.train_fwd else [k for k in SHAPES if k not in TRAIN_FWD[1:3]])
dev = torch.device('cuda:0')


def build(shape, bsz, n_pad, heads, layers, batch_norm):
    torch.manual_seed(0)
    model = DiffGraphTransformerGenGCN(28, 1, 64, heads, dim_feedforward=128, dropout=0.0, nb_layers=layers,
                                       batch_norm=batch_norm, filter_order=4, heads_share_graph=True,
                                       filter_mode='spectral').to(dev)
    if args.dtype == 'bf16':
        set_storage_dtype(model, torch.bfloat16)
    ds = D.SyntheticGraphDataset(shape, bsz, in_dim=28, seed=0, n_max=n_pad)
    batch9, cache = D.collate(ds.samples, k_eig=16, n_pad=n_pad, device=dev)
    return model, batch9, cache


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps


for name in args.shapes.split(','):
    shape, bsz, n_pad, heads, layers, bn = SHAPES[name]
    if args.dtype == 'bf16' and heads != 4:
        print(json.dumps({'shape': name, 'skipped': 'bf16 storage has no %d-head (d_h = %d) form' % (heads, 64 // heads)}),
              flush=True)
        continue
    model, batch9, cache = build(shape, bsz, n_pad, heads, layers, bn)
    x, mask, pe, _, degree, _, edge_index, batch, fi = batch9
    fwd = lambda: model(x, edge_index, batch, fi, mask, pe, degree=degree, graph_cache=cache)
    if args.train_fwd:
        model.train()

        def step():
            out, _ = fwd()
            out.sum().backward()
        res = {'shape': name, 'dtype': args.dtype, 'B': bsz, 'N': n_pad, 'heads': heads, 'layers': layers,
               'two_launch_ms': [], 'one_launch_ms': []}
        for _ in range(args.alternations):      # A/B/A/B: drift of the clocks shows as a trend within each list
            for flag, key in ((False, 'two_launch_ms'), (True, 'one_launch_ms')):
                set_one_launch_forward(model, flag)
                res[key].append(round(1e3 * timed(step), 4))
        med = lambda v: sorted(v)[len(v) // 2]
        res['speedup'] = med(res['two_launch_ms']) / med(res['one_launch_ms'])
        print(json.dumps(res), flush=True)
        continue
    if args.train and name == 'config2':
        model.train()
        def step():
            out, _ = fwd()
            out.sum().backward()
        timed(step)
    model.eval()
    res = {'shape': name, 'dtype': args.dtype, 'B': bsz, 'N': n_pad, 'heads': heads, 'layers': layers,
           'norm': 'batch' if bn else 'layer'}
    with torch.no_grad():
        res['no_grad_ms'] = 1e3 * timed(fwd)
        ref = fwd()[0]
    with torch.inference_mode():
        res['inference_mode_ms'] = 1e3 * timed(fwd)
        got = fwd()[0]
    res['speedup'] = res['no_grad_ms'] / res['inference_mode_ms']
    res['max_abs_diff'] = (got - ref).abs().max().item()
    print(json.dumps(res), flush=True)
