"""CPU tests (no GPU) of the host side of the row-chunk CPO kernels (spo_cpo_rows_*, csrc/cpo_rows.hip): the envelope predicate on
its corners and just outside each, the partial-count / chunk-size queries, and the refusals, which happen before any HIP call."""
import ctypes
import os
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


def _net(sizes):
    from safepo import _abi
    return _abi.MlpNet.of(sizes)


@pytest.mark.parametrize("sizes,ok", [
    ([1, 1, 1, 1], 1), ([128, 128, 128, 16], 1), ([60, 128, 128, 8], 1), ([7, 20, 36, 3], 1), ([24, 128, 16, 1], 1),
    ([129, 128, 128, 16], 0), ([128, 129, 128, 16], 0), ([128, 128, 129, 16], 0), ([128, 128, 128, 17], 0),
    ([376, 128, 128, 17], 0), ([60, 256, 256, 8], 0), ([60, 128, 8], 0), ([60, 128, 128, 128, 8], 0), ([60, 32, 32, 32, 32, 8], 0),
])
def test_supported_on_the_corners_and_just_outside(lib, sizes, ok):
    assert lib.spo_cpo_rows_supported(_net(sizes)) == ok
    assert lib.spo_cpo_rows_supported(None) == 0


def test_partials_and_chunk_rows_are_consistent(lib):
    C = lib.spo_cpo_rows_chunk_rows()
    assert C in (32, 64)
    G = lib.spo_cpo_rows_num_partials(1 << 30)
    assert 1 <= G <= 256
    last = 0
    for rows in (1, C - 1, C, C + 1, 47 * C + 29, G * C - 1, G * C, G * C + C + 29, 4096 * 128):
        n = lib.spo_cpo_rows_num_partials(rows)
        assert n == min((rows + C - 1) // C, G) and n >= last, rows
        last = n


def test_refusals_happen_on_the_host_and_name_the_dimension(lib):
    buf = (ctypes.c_double * 8)()
    ok = ctypes.cast(buf, ctypes.c_void_p)

    def calls(net, rows=64, first=ok):
        return {
            "surrogate_grad": lambda: lib.spo_cpo_rows_surrogate_grad(first, ok, ok, ok, ok, 1.0, rows, net, ok, ok, ok, ok, None),
            "fvp": lambda: lib.spo_cpo_rows_fvp(first, ok, ok, rows, net, ok, ok, ok, None),
            "linesearch_eval": lambda: lib.spo_cpo_rows_linesearch_eval(first, ok, ok, ok, ok, ok, ok, ok, rows, net, ok, 3, ok, None),
            "actor_mean": lambda: lib.spo_cpo_rows_actor_mean(first, ok, ok, rows, net, None),
        }
    for sizes, word in (([129, 128, 128, 4], b"obs_dim"), ([60, 128, 256, 4], b"hidden width"), ([60, 128, 128, 17], b"act_dim"),
                        ([60, 128, 128, 128, 4], b"hidden layers"), ([60, 128, 4], b"hidden layers")):
        for name, call in calls(_net(sizes)).items():
            assert call() == -2, (name, sizes)
            assert word in lib.spo_last_error(), (name, sizes, lib.spo_last_error())
    good = _net([60, 128, 128, 8])
    for kw in (dict(rows=0), dict(first=None)):
        for name, call in calls(good, **kw).items():
            assert call() == -1, (name, kw)
            assert b"bad args" in lib.spo_last_error(), (name, kw, lib.spo_last_error())
