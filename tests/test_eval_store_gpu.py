"""feta_readout_eval, train.StoreEvalStep and train.StoreEvaluator on the MI355X (eval_store_checks.py; the host emulation
runs the same checks, uncaptured, in test_eval_store_emu.py)."""
import contextlib

import pytest

import eval_store_checks as EC

pytestmark = pytest.mark.gpu
CTX = contextlib.nullcontext
TASKS = ['zinc', 'tu', 'molhiv']


@pytest.mark.parametrize('slope', EC.SLOPES)
@pytest.mark.parametrize('loss,c,label_dtype', EC.LOSSES)
@pytest.mark.parametrize('n,layout', EC.LAYOUTS)
def test_readout_matches_fp64(hip, n, layout, loss, c, label_dtype, slope):
    EC.check_readout(hip[1], CTX, n, layout, loss, c, label_dtype, slope)


@pytest.mark.parametrize('loss,c,label_dtype', EC.LOSSES)
def test_readout_skips_the_slots_behind_count(hip, loss, c, label_dtype):
    EC.check_readout(hip[1], CTX, 37, 'dense', loss, c, label_dtype, 0.0, count=3)


def test_readout_is_bit_equal_from_launch_to_launch(hip):
    EC.check_readout_deterministic(hip[1], CTX)


def test_readout_argument_checks(hip):
    EC.check_readout_arguments(hip[1], CTX)


@pytest.mark.parametrize('task', TASKS)
def test_evaluator_matches_train_evaluate(hip, task):
    EC.check_evaluator(task, hip[1], CTX)


@pytest.mark.parametrize('task', TASKS)
def test_single_graph_subset_and_too_many_ids(hip, task):
    EC.check_subsets(task, hip[1], CTX)


def test_refused_configurations(hip):
    EC.check_refused(hip[1], CTX)


@pytest.mark.parametrize('task', TASKS)
def test_step_body_is_three_calls_and_a_replay_none(hip, task):
    EC.check_launches(task, hip[1], CTX, hip[0])


@pytest.mark.parametrize('task', TASKS)
def test_step_does_not_wait_for_the_device(hip, task):
    EC.check_no_host_sync(task, hip[1])
