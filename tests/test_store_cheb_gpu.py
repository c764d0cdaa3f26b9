"""The store's feed of filter_mode='cheb' (lhat) and of the Laplacian-PE sign flip on the MI355X: feta_batch_gather_ex
through the C ABI, the eager step on store.batch and the captured train.StoreTrainStep (store_cheb_checks.py; the host
emulation runs the same checks in test_store_cheb_emu.py, and alone the out-of-range ids)."""
import contextlib

import pytest

import store_cheb_checks as CC
from test_store_cheb_emu import SHAPES

pytestmark = pytest.mark.gpu
CTX = contextlib.nullcontext


@pytest.mark.parametrize('kind,n_pad,bsz', SHAPES)
def test_lhat_equals_the_stagers(hip, kind, n_pad, bsz):
    CC.check_lhat_equals_stager(hip[1], CTX, hip[0], kind, n_pad, bsz)


@pytest.mark.parametrize('n_pad', [16, 21])
def test_null_extras_equal_the_plain_launch(hip, n_pad):
    CC.check_null_extras(hip[1], CTX, hip[0], n_pad)


@pytest.mark.parametrize('kind,n_pad', [('spectral', 16), ('spectral', 21), ('lap3', 21)])
def test_lap_sign_equals_lap_sign_flip(hip, kind, n_pad):
    CC.check_lap_sign(hip[1], CTX, kind, n_pad)


def test_descriptor_checks(hip):
    CC.check_descriptor(hip[0], hip[1], hip[2])


@pytest.mark.parametrize('task,share', [('tu', 1), ('tu', 0), ('sbm', 1)])
def test_cheb_store_steps_follow_the_stager_trajectory(hip, task, share):
    CC.check_trajectory_eager(task, share, hip[1], CTX, hip[0])


@pytest.mark.parametrize('task,share', [('tu', 1), ('tu', 0), ('sbm', 1)])
def test_cheb_store_train_step_follows_the_stager_trajectory(hip, task, share):
    CC.check_trajectory_graphed(task, share, hip[1], hip[0])


def test_store_train_step_flips_the_lap_signs_in_the_graph(hip):
    CC.check_trajectory_graphed('tu', 1, hip[1], hip[0], lap_flip=True)


def test_cheb_model_without_lhat_is_refused(hip):
    CC.check_refusal(hip[1])
