"""Device-resident graph store, feta_batch_gather and train.StoreTrainStep on the MI355X (store_checks.py; the host
emulation runs the same checks in test_store_emu.py, and alone the out-of-range ids)."""
import contextlib

import pytest

import store_checks as SC

pytestmark = pytest.mark.gpu
CTX = contextlib.nullcontext


@pytest.mark.parametrize('bsz', [1, 8])
@pytest.mark.parametrize('n_pad', [21, 32])
@pytest.mark.parametrize('f', [6, 28])
@pytest.mark.parametrize('kind', ['zinc', 'mutag', 'pattern'])
def test_gather_equals_stager(hip, kind, f, n_pad, bsz):
    SC.check_gather_equals_stager(hip[1], CTX, kind, f, n_pad, bsz)


@pytest.mark.parametrize('kind', ['zinc', 'pattern'])
def test_gather_with_a_repeated_id(hip, kind):
    SC.check_gather_equals_stager(hip[1], CTX, kind, 6, 21, 8, repeat=True)


@pytest.mark.parametrize('kind,n_pad,bsz,num_graphs', [('zinc', 37, 128, 160), ('pattern', 64, 300, 320)])
def test_gather_equals_stager_at_the_bench_shapes(hip, kind, n_pad, bsz, num_graphs):
    """B = 128 / N_pad = 37 (ZINC; 37 is odd: the element-wise pe path) and B = 300 / N_pad = 64 (more graphs than CUs)"""
    SC.check_gather_equals_stager(hip[1], CTX, kind, 28, n_pad, bsz, num_graphs=num_graphs, n_max=n_pad)


@pytest.mark.parametrize('n_pad', [21, 32])
@pytest.mark.parametrize('f', [6, 28])
def test_spectral_fields_equal_stager(hip, f, n_pad):
    SC.check_spectral_fields(hip[1], CTX, f, n_pad)


@pytest.mark.parametrize('n_pad', [21, 32])
@pytest.mark.parametrize('f', [6, 28])
def test_bf16_output_is_the_rounded_fp32_output(hip, f, n_pad):
    SC.check_bf16_output(hip[1], CTX, f, n_pad)


def test_descriptor_checks(hip):
    SC.check_descriptor(hip[0], hip[1], hip[2])


@pytest.mark.parametrize('task,bf16', [('tu', False), ('sbm', False), ('tu', True)])
def test_store_train_step_follows_the_stager_trajectory(hip, task, bf16):
    SC.check_trajectory_graphed(task, hip[1], hip[0], bf16)


def test_store_train_step_keeps_the_snapshot_contract(hip):
    SC.check_snapshot_contract(hip[1])
