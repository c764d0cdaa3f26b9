"""The coefficient generator's backward in two parts on the host SIMT emulation (coeff_saved_checks.py)."""
import pytest
import torch

import coeff_saved_checks as CS
from feta_tmlr_amd import _lib

CPU = torch.device('cpu')

# (bsz, n, h, c, node counts of the first graphs): stand-alone kernels on a partial channel tile (C = 80), below one tile
# (C = 64); 4 / 20 / 12 blocks against 4 / 8 / 8 groups (12 and 20 do not divide by 8); nodes on the 16-wide tile edges
# and the padding edge of N = 37; one N = 64 case
STANDALONE = [(1, 37, 2, 64, None), (5, 37, 2, 80, (37, 1, 16, 17)), (6, 37, 2, 64, (37, 16, 1, 17)), (5, 64, 2, 80, None)]
# hosted forms: h = 4, C = 1024
HOSTED = [(1, 37, 4, 1024, None), (5, 37, 4, 1024, (37, 1, 16, 17)), (3, 37, 4, 1024, (17, 37, 1)), (5, 64, 4, 1024, None)]


@pytest.fixture(scope='module')
def cases():
    """the fp64 references, computed once per shape"""
    memo = {}

    def get(key):
        if key not in memo:
            bsz, n, h, c, nodes = key
            memo[key] = CS.coeff_case(bsz, n, h, c, seed=bsz, nodes=nodes)
        return memo[key]
    return get


@pytest.mark.parametrize('key', STANDALONE)
def test_standalone_kernels(emu, cases, key):
    CS.check_standalone(emu, CPU, None, cases(key))


@pytest.mark.parametrize('key', HOSTED)
def test_hosted_roles(emu, cases, key, monkeypatch):
    case = cases(key)
    CS.check_roles(emu, CPU, None, case, CS.check_standalone(emu, CPU, None, case), monkeypatch)


def test_role_is_bounded_to_two_blocks_per_workgroup(emu):
    CS.check_fits(emu, CPU, None)


def test_empty_block_writes_zeros(emu):
    CS.check_empty_block(emu, CPU, None)


def test_bad_arguments_are_rejected(emu):
    CS.check_rejects(emu, CPU, None)


def test_groups_query(emu):
    assert emu.coeff_bwd_saved_groups(128, 4) == 8      # 4 channel tiles x 8 = the 32 slots ffn_bwd leaves free
    assert emu.coeff_bwd_saved_groups(1, 4) == 4 and emu.coeff_bwd_saved_groups(5, 4) == 8
    assert emu.coeff_bwd_saved_groups(512, 4) == 32     # a group walks at most 64 blocks


def test_model_switch_on_off_and_oracle(emu, monkeypatch):
    CS.check_model(emu, CPU, lambda: _lib.override_for_tests(emu), monkeypatch)


def test_fallbacks(emu, monkeypatch):
    CS.check_fallbacks(emu, CPU, lambda: _lib.override_for_tests(emu), monkeypatch)


@pytest.mark.parametrize('cname,pyname', [('feta_coeff_dsum_role', 'CoeffDsumRole'),
                                          ('feta_coeff_bwd_saved_role', 'CoeffBwdSavedRole')])
def test_descriptor_layouts_agree(cname, pyname):
    """the ABI mirror matches the header (as test_abi.py does for the older descriptors)"""
    import test_abi
    test_abi.test_descriptor_layouts_agree(cname, pyname)
