"""CPU tests (no GPU) of the full-batch CPO entry points for 65-128-dim observations: the spo_cpo128_* symbols are declared
in include/safepo_hip.h and bound in safepo._abi, spo_cpo128_supported is host code with the documented truth table, the
argument checks name obs_dim / act_dim, and the routing above them (ActorVCritic.kernels_supported, CPO_MAX_OBS) is unchanged."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["spo_cpo128_supported", "spo_cpo128_num_partials", "spo_cpo128_surrogate_grad", "spo_cpo128_fvp",
           "spo_cpo128_linesearch_eval"]


@pytest.fixture(scope="module")
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    return g.LIB


def test_symbols_declared_and_bound(built_lib):
    from safepo import _abi
    header = open(os.path.join(ROOT, "include", "safepo_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    lib = _abi.load(built_lib)
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name


def test_supported_truth_table(built_lib):
    from safepo import _abi
    lib = _abi.load(built_lib)
    assert [lib.spo_cpo128_supported(D, 4) for D in (64, 65, 72, 128, 129)] == [0, 1, 1, 1, 0]
    assert lib.spo_cpo128_supported(72, 17) == 0
    assert lib.spo_cpo128_supported(72, 16) == 1 and lib.spo_cpo128_supported(72, 1) == 1 and lib.spo_cpo128_supported(72, 0) == 0
    # exhaustive: 1 exactly for 65 <= obs_dim <= 128 and 1 <= act_dim <= 16
    for D in range(0, 200):
        for A in range(0, 20):
            assert lib.spo_cpo128_supported(D, A) == int(65 <= D <= 128 and 1 <= A <= 16), (D, A)


def test_partials_query(built_lib):
    from safepo import _abi
    lib = _abi.load(built_lib)
    # one partial vector per workgroup: 64-row chunks, at most 256 workgroups (as spo_cpo_num_partials)
    for rows in (1, 63, 64, 65, 3037, 64 * 256, 64 * 256 + 1, 4096 * 128):
        assert lib.spo_cpo128_num_partials(rows) == min((rows + 63) // 64, 256) == lib.spo_cpo_num_partials(rows)


def test_dims_outside_the_range_fail_with_minus_two_before_touching_the_gpu(built_lib):
    from safepo import _abi
    lib = _abi.load(built_lib)
    for D, A, word in ((64, 4, b"obs_dim"), (129, 4, b"obs_dim"), (72, 17, b"act_dim"), (72, 0, b"act_dim")):
        assert lib.spo_cpo128_surrogate_grad(None, None, None, None, None, 1.0, 64, D, A, None, None, None, None, None) == -2
        assert word in lib.spo_last_error()
        assert lib.spo_cpo128_fvp(None, None, None, 64, D, A, None, None, None, None) == -2
        assert word in lib.spo_last_error()
        assert lib.spo_cpo128_linesearch_eval(None, None, None, None, None, None, None, None, 64, D, A, None, 3, None, None) == -2
        assert word in lib.spo_last_error()
    # in range, null pointers: an argument error (-1), still without a launch
    assert lib.spo_cpo128_fvp(None, None, None, 64, 72, 2, None, None, None, None) == -1


def test_routing_above_the_primitives_is_unchanged(built_lib):
    from safepo import _abi
    from safepo.common.model import ActorVCritic
    assert _abi.CPO_MAX_OBS == 64
    for D, A in ((72, 2), (128, 16)):
        assert ActorVCritic(D, A).kernels_supported("cpo") is False
    assert ActorVCritic(60, 8).kernels_supported("cpo") is True
