"""CPU tests (no GPU) of the host side of the fused MACPO line-search candidate evaluation (spo_ma_ls_eval*, csrc/ma_ls_eval.hip):
the exported symbols, the envelope predicate inside and just outside, and the refusals, which come before any HIP call."""
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


def test_the_library_exports_the_two_entry_points(lib):
    import __graft_entry__ as g
    raw = ctypes.CDLL(g.LIB)
    for name in ("spo_ma_ls_eval_supported", "spo_ma_ls_eval"):
        assert hasattr(raw, name), name


@pytest.mark.parametrize("kw,word", [
    (dict(), None), (dict(in_dim=1, hidden=1, n_blocks=1, out_dim=1), None), (dict(in_dim=128, hidden=128, out_dim=16), None),
    (dict(hidden=65, n_blocks=1), None),
    (dict(hidden=129), b"hidden 129"), (dict(in_dim=129), b"in_dim 129"), (dict(out_dim=17), b"out_dim 17"),
    (dict(n_blocks=3), b"n_blocks 3"), (dict(is_actor=0, out_dim=1), b"is_actor"),
])
def test_envelope_and_refusals_on_the_host(lib, kw, word):
    """Inside: 1, and -1 "bad args" for null pointers.  Outside: 0, and -2 naming the dimension before a pointer is looked at
    (all of them are null here)."""
    from safepo import _abi
    net = _abi.MaNet(**dict(dict(in_dim=48, hidden=128, n_blocks=2, out_dim=6, is_actor=1), **kw))
    call = lambda rows: lib.spo_ma_ls_eval(None, net, None, 1.0, 0.5, None, None, None, None, None, None, None, rows, None, None, None, None)
    assert lib.spo_ma_ls_eval_supported(net) == (1 if word is None else 0)
    assert lib.spo_ma_ls_eval_supported(None) == 0
    if word is None:
        assert call(33) == -1 and b"bad args" in lib.spo_last_error()
    else:
        assert call(33) == -2 and word in lib.spo_last_error(), lib.spo_last_error()


def test_rows_below_one_are_bad_args(lib):
    from safepo import _abi
    net = _abi.MaNet(in_dim=48, hidden=128, n_blocks=2, out_dim=6, is_actor=1)
    one = ctypes.c_void_p(16)          # non-null and never dereferenced: the refusal comes before any HIP call
    assert lib.spo_ma_ls_eval(one, net, one, 1.0, 0.5, one, one, one, one, one, one, one, 0, one, None, one, None) == -1
    assert b"bad args" in lib.spo_last_error()
