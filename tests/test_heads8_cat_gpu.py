"""The 8-head (d_h = 8) form of the folded filter launches on the MI355X: the checks of test_heads8_cat_emu.py through
libfeta_hip.so, the model at a batch that fills the chip, and what bench.py times at --heads 8 - the captured step must
contain feta_spec_filter_cat_fwd and feta_spec_filter_cat_bwd."""
import contextlib

import pytest

import heads8_cat_checks as HC

pytestmark = pytest.mark.gpu
NULL = contextlib.nullcontext


def test_predicates(hip):
    HC.check_predicates(hip[0])


def test_rejections(hip):
    HC.check_rejections(*hip)


@pytest.mark.parametrize('kw', HC.FWD_CASES)
def test_forward_kernel_matches_oracle(hip, kw):
    HC.check_fwd(*hip, **kw)


@pytest.mark.parametrize('kw', HC.BWD_CASES)
def test_backward_kernel_matches_autograd(hip, kw):
    HC.check_bwd(*hip, **kw)


def test_heads_of_a_wave_do_not_mix(hip):
    HC.check_head_isolation(*hip)


@pytest.mark.parametrize('batch_norm', [True, False])
def test_training_step_takes_the_folded_launches(hip, monkeypatch, batch_norm):
    HC.check_launch_names(hip[0], hip[1], NULL, monkeypatch, batch_norm)


@pytest.mark.parametrize('batch_norm,bsz', [(True, 3), (False, 3), (True, 128), (False, 128)])
def test_fold_on_and_off_match_oracle(hip, monkeypatch, batch_norm, bsz):
    HC.check_fold_on_off(hip[0], hip[1], NULL, monkeypatch, batch_norm, bsz=bsz)


@pytest.mark.parametrize('batch_norm', [True, False])
def test_inference_forward_takes_the_fold(hip, monkeypatch, batch_norm):
    HC.check_inference(hip[0], hip[1], NULL, monkeypatch, batch_norm)


ZINC_DEFAULT = ['--heads', '8', '--layers', '10']


@pytest.mark.parametrize('argv', [ZINC_DEFAULT, ZINC_DEFAULT + ['--layer-norm'], ['--heads', '8']])
def test_timed_configuration_runs_the_folded_launches(hip, argv):
    """what bench.py times at 8 heads against oracle.encoder_gengcn (heads8_checks.check_bench_step_heads8), with the filter
    stage as the two folded launches inside the captured step"""
    errs, used_graph = HC.check_bench_step(hip[1], NULL, hip[0], argv)
    assert used_graph
