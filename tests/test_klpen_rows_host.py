"""CPU tests (no GPU) of the KL-penalty form of the row-group gradient kernel (csrc/mlp_rows.hip: FOCOPS focops.py:326-347, CUP's
second stage cup.py:370-386): the four entry points are exported and bound, say which shapes they take without touching a GPU, and
refuse bad arguments before any launch."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spo_wide_kl_penalty_grad_rows_supported", "spo_wide_kl_penalty_rows_part_floats", "spo_wide_kl_penalty_grad_rows",
         "spo_wide_kl_penalty_reduce_parts")


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from safepo import _abi
    return _abi.load(g.LIB)


def _nets(dims, A):
    from safepo import _abi
    return _abi.MlpNet.of(list(dims) + [1]), _abi.MlpNet.of(list(dims) + [A])


def test_symbols_are_exported_and_bound(lib):
    from safepo import _abi
    assert set(NAMES) <= set(_abi.PROTOTYPES)
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.spo_wide_kl_penalty_rows_part_floats.restype is ctypes.c_int64


def test_shape_envelope(lib):
    from safepo import _abi
    ok = lib.spo_wide_kl_penalty_grad_rows_supported
    for A in (1, 8):
        assert ok(*_nets([60, 128, 128], A), 64) == 1 and ok(*_nets([60, 128, 128], A), 256) == 1
        assert ok(*_nets([60, 256, 256], A), 64) == 1            # the PPO launch's 157.4 KB and the old distribution behind them
    assert ok(*_nets([376, 64, 64], 17), 64) == 1
    assert ok(*_nets([60, 128, 128], 8), 22) == 1 and ok(*_nets([60, 128, 128], 8), 1) == 1
    assert ok(*_nets([60, 128, 128], 8), 257) == 0 and ok(*_nets([60, 128, 128], 8), 0) == 0
    assert ok(*_nets([60, 1024, 1024, 512], 8), 64) == 0
    assert ok(*_nets([376, 256, 256], 17), 64) == 0             # the images do not fit a CU's LDS
    assert ok(*_nets([60, 128, 128], 65), 64) == 0              # act_dim beyond SPO_WIDE_MAX_ACT
    net = _abi.MlpNet.of
    assert ok(net([60, 128, 1]), net([61, 128, 8]), 64) == 0    # the networks read the same observations
    assert ok(net([60, 128, 1]), None, 64) == 0 and ok(None, net([60, 128, 8]), 64) == 0       # (no critics-only form)
    # the PPO launch's envelope is what it was
    assert lib.spo_wide_grad_rows_supported(*_nets([60, 256, 256], 8), 64) == 1
    pf = lib.spo_wide_kl_penalty_rows_part_floats
    Pc, Pa = 60 * 128 + 128 + 128 * 128 + 128 + 128 + 1, 60 * 128 + 128 + 128 * 128 + 128 + 128 * 8 + 8
    P, ab = 2 * Pc + 8 + Pa, 2 * Pc
    sizes = [pf(P, ab, rows) for rows in (1, 16, 17, 64, 240, 256)]
    assert all(s > 0 for s in sizes) and sizes[0] == sizes[1] and sizes == sorted(sizes) and len(set(sizes)) == 5
    # a group's part holds the gradient, the actor's policy-gradient part and the row sums
    assert sizes[2] - sizes[1] >= P + (P - ab) + 5
    assert pf(0, 0, 64) < 0 and pf(-3, 0, 64) < 0 and pf(P, ab, 0) < 0 and pf(P, P + 1, 64) < 0


def test_bad_arguments_are_refused_before_any_launch(lib):
    X = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    crit, act = _nets([60, 128, 128], 8)
    grad = lib.spo_wide_kl_penalty_grad_rows
    assert grad(None, crit, act, *[None] * 10, 64, 0.02, 0.5, 0, None, None) < 0
    assert b"null pointer" in lib.spo_last_error()
    assert grad(X, crit, None, *[X] * 10, 64, 0.02, 0.5, 0, X, None) < 0 and b"null pointer" in lib.spo_last_error()
    args = [X, X, X, None, None, X, X, X, X, None]               # obs act logp_old target_r target_c adv old_mean old_std idx cursor
    assert grad(X, crit, act, *args, 64, 0.02, 0.5, 0, X, None) < 0 and b"critic targets" in lib.spo_last_error()
    args[3] = args[4] = X
    for rows in (0, 257, -1):
        assert grad(X, crit, act, *args, rows, 0.02, 0.5, 0, X, None) < 0
        assert b"rows" in lib.spo_last_error()
    for dims, A in (([60, 1024, 1024, 512], 8), ([376, 256, 256], 17), ([60, 128, 128], 65)):
        c2, a2 = _nets(dims, A)
        assert grad(X, c2, a2, *args, 64, 0.02, 0.5, 0, X, None) < 0
        assert b"outside the row-group kernel" in lib.spo_last_error()
    red = lib.spo_wide_kl_penalty_reduce_parts
    assert red(None, 64, 1000, 600, 0, 1, 0.5, None, None, None, None, None) < 0 and b"null pointer" in lib.spo_last_error()
    assert red(X, 64, 1000, 600, 0, 1, 0.5, X, None, X, X, None) < 0 and b"null pointer" in lib.spo_last_error()
    for rows, n_params, ab in ((0, 1000, 600), (257, 1000, 600), (64, 0, 0), (64, 1000, 1001), (64, 1000, -1)):
        assert red(X, rows, n_params, ab, 0, 1, 0.5, X, X, X, X, None) < 0
        assert b"bad args" in lib.spo_last_error()


def test_switch_turns_the_klpen_launch_off_with_the_row_group_kernel():
    """SPO_WIDE_ROWS=0 (read once per process: a child process)."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as g; from safepo import _abi; lib = _abi.load(g.LIB); "
            "n = _abi.MlpNet.of; print(lib.spo_wide_kl_penalty_grad_rows_supported(n([60, 128, 128, 1]), n([60, 128, 128, 8]), 64))" % ROOT)
    out = {}
    for v in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SPO_WIDE_ROWS=v), capture_output=True, text=True, check=True)
        out[v] = r.stdout.strip().splitlines()[-1]
    assert out == {"0": "0", "1": "1"}, out
