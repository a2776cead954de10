"""CPU tests (no GPU) of the host side of the fused multi-agent Fisher-vector product (spo_ma_fvp_*, csrc/ma_fvp.hip): the exported
symbols, the envelope predicate inside and just outside, the refusals (before any HIP call) and the two size queries."""
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


def _net(in_dim=48, hidden=128, n_blocks=2, out_dim=6, is_actor=1):
    from safepo import _abi
    return _abi.MaNet(in_dim=in_dim, hidden=hidden, n_blocks=n_blocks, out_dim=out_dim, is_actor=is_actor)


def test_the_library_exports_the_four_entry_points(lib):
    import __graft_entry__ as g
    raw = ctypes.CDLL(g.LIB)
    for name in ("spo_ma_fvp_supported", "spo_ma_fvp_num_partials", "spo_ma_fvp_scratch_floats", "spo_ma_fvp"):
        assert hasattr(raw, name), name


@pytest.mark.parametrize("kw,word", [
    (dict(), None), (dict(in_dim=1, hidden=1, n_blocks=1, out_dim=1), None), (dict(in_dim=128, hidden=128, out_dim=16), None),
    (dict(hidden=65, n_blocks=1), None),
    (dict(hidden=129), b"hidden 129"), (dict(in_dim=129), b"in_dim 129"), (dict(out_dim=17), b"out_dim 17"),
    (dict(n_blocks=3), b"n_blocks 3"), (dict(is_actor=0, out_dim=1), b"is_actor"),
])
def test_envelope_and_refusals_on_the_host(lib, kw, word):
    """Inside: 1 and a positive scratch size.  Outside: 0, scratch -1, and spo_ma_fvp answers -2 naming the dimension before it
    touches a pointer (all of them are null here)."""
    net = _net(**kw)
    assert lib.spo_ma_fvp_supported(net) == (1 if word is None else 0)
    assert lib.spo_ma_fvp_supported(None) == 0
    if word is None:
        assert lib.spo_ma_fvp_scratch_floats(net, 33) > 0
        assert lib.spo_ma_fvp_scratch_floats(net, 0) == -1
        assert lib.spo_ma_fvp(None, net, None, None, 33, 33, None, None, None, None) == -1
        assert b"bad args" in lib.spo_last_error()
    else:
        assert lib.spo_ma_fvp_scratch_floats(net, 33) == -1
        assert lib.spo_ma_fvp(None, net, None, None, 33, 33, None, None, None, None) == -2
        assert word in lib.spo_last_error(), lib.spo_last_error()


def test_num_partials_is_one_per_32_row_chunk_up_to_256(lib):
    assert [lib.spo_ma_fvp_num_partials(r) for r in (1, 32, 33, 8192, 8193)] == [1, 1, 2, 256, 256]


def test_scratch_holds_the_fold_tangent_and_one_vector_per_partial(lib):
    net = _net()
    P = lib.spo_ma_param_count(net)
    assert lib.spo_ma_fvp_scratch_floats(net, 33) == 128 * 48 + 128 + 2 * P
    assert lib.spo_ma_fvp_scratch_floats(net, 10000) == 128 * 48 + 128 + 256 * P
