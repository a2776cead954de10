"""CPU tests (no GPU) of the host side of the fused MACPO surrogate-gradient pair (spo_ma_trpo_grads*, csrc/ma_trpo_grads.hip): the
exported symbols, the envelope predicate at its edges, the sizes the header states, and the refusals, which come before any HIP call."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spo_ma_trpo_grads_supported", "spo_ma_trpo_grads_num_partials", "spo_ma_trpo_grads_scratch_floats", "spo_ma_trpo_grads")


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from safepo import _abi
    return _abi.load(g.LIB)


def test_the_four_symbols_are_declared_exported_and_bound(lib):
    import __graft_entry__ as g
    from safepo import _abi
    raw = ctypes.CDLL(g.LIB)
    header = open(os.path.join(ROOT, "include", "safepo_hip.h")).read()
    for name in NAMES:
        assert hasattr(raw, name) and name in _abi.PROTOTYPES and f" {name}(" in header, name


@pytest.mark.parametrize("kw,word", [
    (dict(), None), (dict(in_dim=1, hidden=1, n_blocks=1, out_dim=1), None), (dict(in_dim=128, hidden=128, out_dim=16), None),
    (dict(hidden=129), b"hidden 129"), (dict(in_dim=129), b"in_dim 129"), (dict(out_dim=17), b"out_dim 17"),
    (dict(n_blocks=3), b"n_blocks 3"), (dict(is_actor=0, out_dim=1), b"is_actor"),
])
def test_envelope_and_refusals_on_the_host(lib, kw, word):
    """Inside: 1, a positive scratch size, and -1 "bad args" for null pointers or rows < 1.  Outside: 0, scratch -1, and -2 naming
    the dimension before a pointer is looked at (all of them are null here)."""
    from safepo import _abi
    net = _abi.MaNet(**dict(dict(in_dim=48, hidden=128, n_blocks=2, out_dim=6, is_actor=1), **kw))
    call = lambda p, rows: lib.spo_ma_trpo_grads(p, net, *([p] * 7), 1.0, 0.5, rows, rows, p, p, p, p, None)
    assert lib.spo_ma_trpo_grads_supported(net) == (1 if word is None else 0) and lib.spo_ma_trpo_grads_supported(None) == 0
    if word is None:
        assert lib.spo_ma_trpo_grads_scratch_floats(net, 33) > 0 and lib.spo_ma_trpo_grads_scratch_floats(net, 0) == -1
        assert call(None, 33) == -1 and b"bad args" in lib.spo_last_error()
        assert call(ctypes.c_void_p(16), 0) == -1 and b"bad args" in lib.spo_last_error()      # never dereferenced
    else:
        assert lib.spo_ma_trpo_grads_scratch_floats(net, 33) == -1
        assert call(None, 33) == -2 and word in lib.spo_last_error(), lib.spo_last_error()


def test_partials_and_scratch_follow_the_header(lib):
    """min(ceil(rows / 32), 256) workgroups; per workgroup and gradient 17 doubles and one vector laid out like theta."""
    from safepo import _abi
    net = _abi.MaNet(in_dim=48, hidden=128, n_blocks=2, out_dim=6, is_actor=1)
    P = lib.spo_ma_param_count(net)
    rows = (1, 32, 33, 8192, 8193)
    assert [lib.spo_ma_trpo_grads_num_partials(r) for r in rows] == [1, 1, 2, 256, 256]
    assert [lib.spo_ma_trpo_grads_scratch_floats(net, r) for r in rows] == [n * 2 * (2 * 17 + P) for n in (1, 1, 2, 256, 256)]
