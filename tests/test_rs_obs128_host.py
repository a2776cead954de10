"""CPU tests (no GPU) of the row-split update kernel's KIN = 128 form (observations of 65 .. 128 values): the new query
spo_update_rs128_supported is declared in include/safepo_hip.h, exported and bound in safepo._abi, is host code with the documented
truth table, and spo_update_rs_supported -- which also keys the data-parallel routing -- answers as before."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from safepo import _abi
    return _abi.load(g.LIB)


def test_symbol_declared_and_bound(lib):
    from safepo import _abi
    header = open(os.path.join(ROOT, "include", "safepo_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    assert "spo_update_rs128_supported" in declared
    assert "spo_update_rs128_supported" in _abi.PROTOTYPES
    assert hasattr(lib, "spo_update_rs128_supported")


def test_support_table(lib):
    f = lib.spo_update_rs128_supported
    for shape in ((65, 1, 64, 3), (72, 2, 64, 3), (128, 16, 1, 3)):
        assert f(*shape) == 1, shape
    for shape in ((64, 8, 64, 3), (129, 8, 64, 3), (72, 17, 64, 3), (72, 2, 65, 3), (72, 2, 129, 2), (72, 2, 64, 1)):
        assert f(*shape) == 0, shape
    # the critic fit's form (two networks, four row groups) lost its measurement and is not built: every n_nets == 2 shape is 0
    assert f(104, 12, 128, 2) == 0 and f(72, 2, 64, 2) == 0
    # exhaustive over the edges: 1 exactly for 65 <= obs <= 128, 1 <= act <= 16, 1 <= batch <= 64 and three networks
    for D in (0, 1, 60, 64, 65, 66, 100, 127, 128, 129, 200):
        for A in (0, 1, 8, 16, 17):
            for B in (0, 1, 32, 64, 65, 128, 129):
                for n in (0, 1, 2, 3, 4):
                    want = int(65 <= D <= 128 and 1 <= A <= 16 and n == 3 and 1 <= B <= 64)
                    assert f(D, A, B, n) == want, (D, A, B, n)


def test_the_query_up_to_64_is_unchanged(lib):
    f = lib.spo_update_rs_supported
    assert f(72, 2, 64, 3) == 0 and f(65, 8, 64, 3) == 0 and f(104, 12, 128, 2) == 0
    assert f(60, 8, 64, 3) == 1 and f(64, 16, 1, 3) == 1 and f(60, 8, 128, 2) == 1
    # the two queries never both say yes
    for D in range(1, 140):
        assert f(D, 4, 64, 3) + lib.spo_update_rs128_supported(D, 4, 64, 3) == int(D <= 128), D
