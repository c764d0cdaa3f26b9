"""Device-resident graph store, feta_batch_gather and the store-fed training step in the host SIMT emulation
(store_checks.py; the MI355X runs the same checks in test_store_gpu.py)."""
import pytest
import torch

import store_checks as SC
from feta_tmlr_amd import _lib

CPU = torch.device('cpu')


def _ctx(emu):
    return lambda: _lib.override_for_tests(emu)


@pytest.mark.parametrize('bsz', [1, 8])
@pytest.mark.parametrize('n_pad', [21, 32])
@pytest.mark.parametrize('f', [6, 28])
@pytest.mark.parametrize('kind', ['zinc', 'mutag', 'pattern'])
def test_gather_equals_stager(emu, kind, f, n_pad, bsz):
    SC.check_gather_equals_stager(CPU, _ctx(emu), kind, f, n_pad, bsz)


@pytest.mark.parametrize('kind', ['zinc', 'pattern'])
def test_gather_with_a_repeated_id(emu, kind):
    SC.check_gather_equals_stager(CPU, _ctx(emu), kind, 6, 21, 8, repeat=True)


@pytest.mark.parametrize('n_pad', [21, 32])
@pytest.mark.parametrize('f', [6, 28])
def test_spectral_fields_equal_stager(emu, f, n_pad):
    SC.check_spectral_fields(CPU, _ctx(emu), f, n_pad)


@pytest.mark.parametrize('n_pad', [21, 32])
@pytest.mark.parametrize('f', [6, 28])
def test_bf16_output_is_the_rounded_fp32_output(emu, f, n_pad):
    SC.check_bf16_output(CPU, _ctx(emu), f, n_pad)


@pytest.mark.parametrize('kind', ['zinc', 'mutag', 'pattern'])
def test_out_of_range_and_oversized_ids_give_empty_graphs(emu, kind):
    SC.check_invalid_ids(CPU, _ctx(emu), kind)


def test_descriptor_checks(emu):
    SC.check_descriptor(emu, CPU, None)


def test_gather_descriptor_layout_agrees():
    SC.check_struct_layout()


@pytest.mark.parametrize('task,bf16', [('tu', False), ('sbm', False), ('tu', True)])
def test_store_steps_follow_the_stager_trajectory(emu, task, bf16):
    SC.check_trajectory_eager(task, CPU, _ctx(emu), emu, bf16)


def test_epoch_covers_every_graph_once_per_bucket():
    """store.epoch: every graph once, batches cut inside a bucket, ragged tails kept or dropped; nbytes counts the arrays"""
    import numpy as np
    packed = SC.packed_split('mutag', 6)
    store = SC.DeviceGraphStore(packed, CPU)
    batches = list(store.epoch(4, np.random.default_rng(0)))
    assert sorted(int(i) for _, ids in batches for i in ids) == list(range(SC.NUM_GRAPHS))
    for n_pad, ids in batches:
        assert ids.dtype == np.int32 and 0 < len(ids) <= 4 and bool((store.bucket[ids] == n_pad).all())
    full = list(store.epoch(4, None, drop_last=True))
    assert all(len(ids) == 4 for _, ids in full) and len(full) == sum(len(store.bucket_ids(b)) // 4 for b in (16, 32))
    assert store.nbytes == sum(t.numel() * t.element_size() for t in (store.x, store.degree, store.y, store.n, store.node_off))
    assert store.build_seconds >= 0.0
    with pytest.raises(ValueError, match='largest bucket'):
        SC.DeviceGraphStore(packed, CPU, buckets=(8, 16))
