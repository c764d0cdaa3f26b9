"""feta_readout_eval, train.StoreEvalStep and train.StoreEvaluator in the host SIMT emulation (eval_store_checks.py; the
MI355X runs the same checks, captured, in test_eval_store_gpu.py).  A step on a CPU store runs its body instead of
replaying a hipGraph.  Every lane is a host fiber here: the models have one encoder layer and the end-to-end checks walk
part of the 23-graph store - a full batch, ragged tails and a batch of one graph out of both buckets - where the GPU file
walks all of it."""
import pytest
import torch

import eval_store_checks as EC
from feta_tmlr_amd import _lib

CPU = torch.device('cpu')
TASKS = ['zinc', 'tu', 'molhiv']


def _ctx(emu):
    return lambda: _lib.override_for_tests(emu)


@pytest.mark.parametrize('slope', EC.SLOPES)
@pytest.mark.parametrize('loss,c,label_dtype', EC.LOSSES)
@pytest.mark.parametrize('n,layout', EC.LAYOUTS)
def test_readout_matches_fp64(emu, n, layout, loss, c, label_dtype, slope):
    EC.check_readout(CPU, _ctx(emu), n, layout, loss, c, label_dtype, slope)


@pytest.mark.parametrize('loss,c,label_dtype', EC.LOSSES)
def test_readout_skips_the_slots_behind_count(emu, loss, c, label_dtype):
    EC.check_readout(CPU, _ctx(emu), 37, 'dense', loss, c, label_dtype, 0.0, count=3)


def test_readout_is_bit_equal_from_launch_to_launch(emu):
    EC.check_readout_deterministic(CPU, _ctx(emu))


def test_readout_argument_checks(emu):
    EC.check_readout_arguments(CPU, _ctx(emu))


def test_readout_descriptor_layout_agrees():
    EC.check_struct_layout()


@pytest.mark.parametrize('task', TASKS)
def test_evaluator_matches_train_evaluate(emu, task):
    EC.check_evaluator(task, CPU, _ctx(emu), layers=1, bsz=4, take=(5, 2))


@pytest.mark.parametrize('task', TASKS)
def test_single_graph_subset_and_too_many_ids(emu, task):
    EC.check_subsets(task, CPU, _ctx(emu), layers=1, take=(2, 1))


def test_refused_configurations(emu):
    EC.check_refused(CPU, _ctx(emu))


@pytest.mark.parametrize('task', TASKS)
def test_step_body_is_three_calls(emu, task):
    EC.check_launches(task, CPU, _ctx(emu), emu, layers=1)
