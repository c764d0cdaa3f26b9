"""A whole split resident on the device, its spectra computed once; a padded batch is one launch.

The reference keeps the per-graph encodings in a pickle (transformer/position_encoding.py:35-49) and builds every
batch on the host from Python lists (GraphDataset_v2.collate_fn, transformer/data.py:161-225).  ``data.BatchStager``
already replaced the lists by vectorised gathers and the pickle by device kernels, but it still runs per batch: ~20
numpy gathers, ~10 host-to-device copies and the eigendecomposition of graphs that were decomposed in every epoch
before.  ``DeviceGraphStore`` runs the stager ONCE per graph when it is built, packs what came out into flat device
arrays, and ``feta_batch_gather`` (csrc/gather.hip) then builds the padded batch of any list of graph ids in one
launch - inside a captured training step (``train.StoreTrainStep``) the host sends the ids and nothing else (with
``lap_sign_flip`` also the lap_dim signs of the batch).

Store layout (G graphs, sumN nodes):
    x [sumN, F], degree [sumN], labels [G] (float32 / int64) or [sumN] int64 node labels, n [G] int32,
    node_off [G] int64, bucket [G] int32 (host), u [sumN, K], lam [G, K], lap [sumN, lap_dim],
    pe: graph g's n x n kernel at pe_off[g] with row pitch roundup4(n) (zero columns behind n): rows start on 16 bytes.
    lhat (``lhat=True``): graph g's n x n scaled Laplacian, at the same pe_off[g] with the same pitch.

Both filter modes are fed: filter_mode='spectral' reads cache.u / cache.lam (the store needs ``k_eig``), filter_mode='cheb'
- the reference's operator and the constructor default of the models - reads cache.lhat (the store needs ``lhat=True``;
``feta_batch_gather_ex`` emits it, and applies the per-batch sign flip of the Laplacian eigenvector features when it is
given signs).  A split is evaluated from the store in captured steps too (``train.StoreEvaluator`` /
``train.StoreEvalStep``: gather, eval-mode encoder in one launch, ``feta_readout_eval``; ragged tails included, one host
read per split).  Limits: no edge list is kept, so edge_index / batch / feature_indices of the tuple are None and a cheb
model on a store without lhat has nothing to build its Laplacian from; the ragged tail batches of TRAINING go through
``store.batch`` (repeated graphs would bias BatchNorm's batch statistics), and so does the evaluation of task 'sbm' and of
stacks without a one-launch inference form (N_pad > 64); bf16 storage with filter_mode='cheb' is refused by the models, here
as everywhere.
"""
import time

import numpy as np
import torch

from .. import _abi, _lib
from .data import BUCKETS, BatchStager, GraphBatchCache


class GatherBuffers:
    """The output tensors of one feta_batch_gather launch for a [B, N_pad] batch (a StoreTrainStep keeps one set as
    the static inputs of its hipGraph).  lhat (default: when the store has it): [B, N_pad, N_pad] float32, the operand
    of filter_mode='cheb'.  lap_sign: also a [lap_dim] float32 vector of +1, the factor per column of lap that the
    launch applies (train.lap_signs).  Either one makes the launch feta_batch_gather_ex."""

    def __init__(self, store, bsz, n_pad, dtype=torch.float32, lhat=None, lap_sign=False):
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError('float32 or bfloat16 x / pe, got %s' % dtype)
        dev = store.device
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        self.bsz, self.n_pad, self.dtype = int(bsz), int(n_pad), dtype
        self.ids = torch.zeros((bsz,), dtype=torch.int32, device=dev)
        self.x = new((bsz, n_pad, store.f), dtype)
        self.mask = new((bsz, n_pad), torch.bool)
        self.degree = new((bsz, n_pad), torch.float32) if store.degree is not None else None
        self.degree_rows = new((n_pad * bsz,), torch.float32) if store.degree is not None else None
        self.pe = new((bsz, n_pad, n_pad), dtype) if store.pe is not None else None
        self.u = new((bsz, n_pad, store.k), torch.float32) if store.u is not None else None
        self.lam = new((bsz, store.k), torch.float32) if store.u is not None else None
        self.lap = new((bsz, n_pad, store.lap_dim), torch.float32) if store.lap is not None else None
        if lhat and store.lhat is None:
            raise ValueError('lhat needs DeviceGraphStore(..., lhat=True)')
        if lap_sign and store.lap is None:
            raise ValueError('lap_sign needs DeviceGraphStore(..., lap_dim=...)')
        self.lhat = new((bsz, n_pad, n_pad), torch.float32) if (store.lhat is not None and lhat is not False) else None
        self.lap_sign = torch.ones((store.lap_dim,), dtype=torch.float32, device=dev) if lap_sign else None
        self.n_real = new((bsz,), torch.int32)
        self.node_off = new((bsz,), torch.int32)
        self.labels = new((bsz, n_pad) if store.node_labels else (bsz,), store.y.dtype)

    def batch9(self):
        """the reference's 9-tuple; node labels are padded [B, N_pad] with -100 (train.pad_node_labels)"""
        return (self.x, self.mask, self.pe, self.lap, self.degree, self.labels, None, None, None)

    def cache(self):
        c = GraphBatchCache(n_real=self.n_real, node_off=self.node_off, n_pad=self.n_pad, u=self.u, lam=self.lam,
                            lhat=self.lhat)
        if self.degree_rows is not None:
            c.extra['degree_rows'] = self.degree_rows
        return c


class DeviceGraphStore:
    """``packed``: data.PackedGraphs of the split.  The other arguments are BatchStager's (pos_enc 'diffusion' | 'pstep',
    k_eig eigenpairs for filter_mode='spectral', lap_dim Laplacian eigenvector features); ``lhat=True`` also keeps every
    graph's dense scaled Laplacian for filter_mode='cheb': 4 * n * roundup4(n) bytes per graph - about 2.2 KB per ZINC
    graph on top of 6.9 KB, and as much as pe for any graph.  Every graph goes through
    ``BatchStager.stage`` once, at the padded size of its bucket and ``build_batch`` graphs at a time.  The kernels behind
    it work one workgroup per graph on the graph's own n x n block, so what is stored for a graph does not depend on the
    graphs it was staged with, and ``batch(ids)`` returns the tensors ``stage(ids)`` returns.

    ``build_seconds``: wall time of the construction (device work included); ``nbytes``: device bytes held."""

    def __init__(self, packed, device, buckets=BUCKETS, pos_enc=None, k_eig=None, lap_dim=None, beta=1.0, p=1,
                 zero_diag=False, build_batch=256, lhat=False):
        t0 = time.perf_counter()
        self.device = torch.device(device)
        dev = self.device
        ns = np.asarray(packed.n, np.int64)
        self.num_graphs, self.f = int(packed.num_graphs), int(packed.x.shape[1])
        if self.num_graphs == 0:
            raise ValueError('an empty split')
        self.buckets = tuple(sorted(int(bk) for bk in buckets))
        which = np.searchsorted(np.array(self.buckets), ns)
        if int(which.max()) >= len(self.buckets):
            g = int(np.argmax(ns))
            raise ValueError('graph %d has %d nodes, more than the largest bucket %d' % (g, int(ns[g]), self.buckets[-1]))
        self.bucket = np.array(self.buckets, np.int32)[which]             # [G] padded size of each graph's bucket (host)
        self.n_host = ns
        self.node_labels = bool(packed.node_labels)
        self.k = None if k_eig is None else int(k_eig)
        self.lap_dim = None if lap_dim is None else int(lap_dim)
        if self.k is not None and self.k > int(self.bucket.min()):
            raise ValueError('k_eig = %d is more than the smallest padded size in use, %d' % (self.k, int(self.bucket.min())))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.x = t(packed.x)
        self.degree = None if packed.degree is None else t(packed.degree)
        self.y = t(packed.y)
        self.n = t(ns.astype(np.int32))
        self.node_off = t(np.asarray(packed.node_off[:-1], np.int64))
        self.label_kind = (_abi.LABELS_NODE_I64 if self.node_labels else
                           _abi.LABELS_GRAPH_I64 if packed.y.dtype == np.int64 else _abi.LABELS_GRAPH_F32)
        sum_n = int(ns.sum())
        pitch = (ns + 3) & ~3
        sizes = pitch * ns
        self.pe = self.pe_off = self.u = self.lam = self.lap = self.lhat = None
        if pos_enc is not None or lhat:
            self.pe_off = t(np.concatenate([[0], np.cumsum(sizes)])[:-1].astype(np.int64))   # n x n block offsets
        if pos_enc is not None:
            self.pe = torch.zeros((int(sizes.sum()),), dtype=torch.float32, device=dev)
        if lhat:
            self.lhat = torch.zeros((int(sizes.sum()),), dtype=torch.float32, device=dev)
        if self.k is not None:
            self.u = torch.zeros((sum_n, self.k), dtype=torch.float32, device=dev)
            self.lam = torch.zeros((self.num_graphs, self.k), dtype=torch.float32, device=dev)
        if self.lap_dim is not None:
            self.lap = torch.zeros((sum_n, self.lap_dim), dtype=torch.float32, device=dev)
        if self.pe is not None or self.u is not None or self.lap is not None or self.lhat is not None:
            pitch_d = t(pitch)
            for n_pad in sorted(set(self.bucket.tolist())):
                members = np.nonzero(self.bucket == n_pad)[0]
                stager = BatchStager(packed, min(int(build_batch), len(members)), n_pad, dev, pos_enc=pos_enc, k_eig=k_eig,
                                     lap_dim=lap_dim, beta=beta, p=p, zero_diag=zero_diag)
                for s in range(0, len(members), int(build_batch)):
                    self._pack(stager.stage(members[s:s + int(build_batch)]), t(members[s:s + int(build_batch)]), pitch_d)
        if dev.type == 'cuda':
            torch.cuda.synchronize(dev)
        self.build_seconds = time.perf_counter() - t0

    def _pack(self, staged, gids, pitch):
        """scatter the real block of every staged graph into the flat arrays (index arithmetic on the device)"""
        batch9, cache = staged
        n_pad = cache.n_pad
        n = cache.n_real.to(torch.int64)
        r = torch.arange(n_pad, device=self.device)
        rows = r[None, :] < n[:, None]                                       # [b, N] real nodes
        dst_rows = (self.node_off[gids][:, None] + r[None, :])[rows]
        if self.pe is not None or self.lhat is not None:
            real = rows[:, :, None] & rows[:, None, :]
            dst = (self.pe_off[gids][:, None, None] + r[None, :, None] * pitch[gids][:, None, None] + r[None, None, :])[real]
        if self.pe is not None:
            self.pe[dst] = batch9[2][real]
        if self.lhat is not None:
            lhat = cache.lhat          # attach_device_spectrum left it there when the stager computed a spectrum
            if lhat is None:
                from .. import functional as FF
                lhat = FF.lhat_from_edges(batch9[6], batch9[7], cache.node_off, n.shape[0], n_pad)
            self.lhat[dst] = lhat[real]
        if self.u is not None:
            self.u[dst_rows] = cache.u[rows]
            self.lam[gids] = cache.lam
        if self.lap is not None:
            self.lap[dst_rows] = batch9[3][rows]

    @property
    def nbytes(self):
        ts = (self.x, self.degree, self.y, self.n, self.node_off, self.pe, self.pe_off, self.u, self.lam, self.lap,
              self.lhat)
        return sum(t.numel() * t.element_size() for t in ts if t is not None)

    def bucket_ids(self, n_pad):
        """graph ids of the bucket padded to n_pad, ascending"""
        return np.nonzero(self.bucket == n_pad)[0].astype(np.int32)

    def epoch(self, batch_size, rng=None, drop_last=False):
        """-> (n_pad, ids int32 [<= batch_size]) per batch, bucket by bucket as data.bucket_batches cuts them; ``rng``
        (numpy Generator) shuffles inside each bucket.  A ragged last batch of a bucket is dropped with drop_last."""
        for n_pad in sorted(set(self.bucket.tolist())):
            idx = self.bucket_ids(n_pad)
            if rng is not None:
                idx = rng.permutation(idx)
            for s in range(0, len(idx), batch_size):
                ids = idx[s:s + batch_size]
                if len(ids) == batch_size or not drop_last:
                    yield n_pad, ids

    def device_ids(self, ids):
        """int32 ids on the store's device: a device tensor is taken as it is, a host sequence costs one small copy"""
        if torch.is_tensor(ids):
            if ids.dtype != torch.int32 or ids.device != self.device:
                raise TypeError('device ids must be int32 on %s, got %s on %s' % (self.device, ids.dtype, ids.device))
            return ids.contiguous()
        return torch.from_numpy(np.ascontiguousarray(np.asarray(ids, np.int32))).to(self.device)

    def gather_into(self, bufs, ids=None):
        """one launch on the current stream: the batch of ``ids`` (default: bufs.ids) into bufs - feta_batch_gather, or
        feta_batch_gather_ex when bufs carries lhat or lap_sign"""
        ids = bufs.ids if ids is None else ids
        abi, stream = _lib.backend(self.x, ids)
        kw = dict(f=self.f, k=self.k or 0, lap_dim=self.lap_dim or 0, dtype=abi._dt_of(bufs.dtype), label_kind=self.label_kind,
                  s_x=self.x, s_degree=self.degree, s_labels=self.y, s_n=self.n, s_node_off=self.node_off,
                  s_pe=self.pe, s_pe_off=self.pe_off, s_u=self.u, s_lam=self.lam, s_lap=self.lap, ids=ids,
                  x=bufs.x, mask=bufs.mask, degree=bufs.degree, degree_rows=bufs.degree_rows, pe=bufs.pe, u=bufs.u,
                  lam=bufs.lam, lap=bufs.lap, n_real=bufs.n_real, node_off=bufs.node_off, labels=bufs.labels)
        if bufs.lhat is not None or bufs.lap_sign is not None:
            abi.batch_gather_ex(self.num_graphs, bufs.bsz, bufs.n_pad, stream, lhat=bufs.lhat, lap_sign=bufs.lap_sign,
                                s_lhat=self.lhat if bufs.lhat is not None else None, **kw)
        else:
            abi.batch_gather(self.num_graphs, bufs.bsz, bufs.n_pad, stream, **kw)
        return bufs

    def batch(self, ids, n_pad=None, dtype=torch.float32, lhat=None):
        """-> (batch9, cache) of the graphs ``ids`` in the layout of BatchStager.stage: x, mask, pe, lap, degree, labels
        and a cache with n_real, node_off, u, lam, lhat and extra['degree_rows']; edge_index, batch and feature_indices
        are None (filter_mode='spectral' with cache.u and filter_mode='cheb' with cache.lhat read none of them), node
        labels come padded [B, N_pad] with -100.  n_pad: default the largest bucket among the ids (host ids only).
        dtype: type of x and pe.  lhat: emit cache.lhat (default: whenever the store has it)."""
        if n_pad is None:
            if torch.is_tensor(ids):
                raise ValueError('n_pad is needed with device-resident ids')
            n_pad = int(self.bucket[np.asarray(ids, np.int64)].max())
        ids = self.device_ids(ids)
        if ids.dim() != 1 or ids.shape[0] == 0:
            raise ValueError('ids must be a non-empty 1-d sequence')
        bufs = self.gather_into(GatherBuffers(self, ids.shape[0], n_pad, dtype, lhat=lhat), ids)
        return bufs.batch9(), bufs.cache()
