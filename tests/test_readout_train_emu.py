"""feta_readout_train_fwd / _bwd, functional.readout_train and the fused_head option of train_step in the host SIMT emulation
(readout_train_checks.py; the MI355X runs the same checks, and the captured step, in test_readout_train_gpu.py).  Every lane
is a host fiber here: the models have one encoder layer and batches of two graphs."""
import pytest
import torch

import eval_store_checks as EC
import readout_train_checks as RC
from feta_tmlr_amd import _lib

CPU = torch.device('cpu')
TASKS = ['zinc', 'tu', 'molhiv']


def _ctx(emu):
    return lambda: _lib.override_for_tests(emu)


@pytest.mark.parametrize('slope', EC.SLOPES)
@pytest.mark.parametrize('loss,c,label_dtype', EC.LOSSES)
@pytest.mark.parametrize('n,layout', EC.LAYOUTS)
def test_head_matches_fp64_autograd(emu, n, layout, loss, c, label_dtype, slope):
    RC.check_kernels(CPU, _ctx(emu), n, layout, loss, c, label_dtype, slope)


def test_head_without_biases(emu):
    RC.check_kernels(CPU, _ctx(emu), 37, 'dense', 'ce', 3, torch.int64, 0.01, bias=False)


@pytest.mark.parametrize('loss,c,label_dtype', EC.LOSSES)
def test_slots_behind_count_are_skipped_and_get_zero_gradient(emu, loss, c, label_dtype):
    RC.check_count(emu, CPU, None, loss, c, label_dtype)


def test_incoming_gradient_scales_every_gradient(emu):
    RC.check_incoming_gradient(CPU, _ctx(emu))


def test_two_runs_are_bit_equal(emu):
    RC.check_deterministic(CPU, _ctx(emu))


def test_slot_contraction_crosses_its_chunk(emu):
    RC.check_many_slots(CPU, _ctx(emu), 70)


def test_no_labelled_graph_gives_nan(emu):
    RC.check_all_labels_nan(CPU, _ctx(emu))


def test_no_grad_runs_the_forward_only_and_frozen_parameters_get_none(emu):
    RC.check_no_grad_and_frozen(CPU, _ctx(emu), emu)


def test_argument_checks(emu):
    RC.check_arguments(CPU, _ctx(emu))


def test_descriptor_layout_agrees():
    RC.check_struct_layout()


@pytest.mark.parametrize('task', TASKS)
def test_fused_head_step_follows_the_plain_step(emu, task):
    RC.check_train_step(task, CPU, _ctx(emu), emu, layers=1, bsz=2, num_graphs=12)


def test_refused_configurations(emu):
    RC.check_refused(CPU, _ctx(emu))
