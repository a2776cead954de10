"""CPU tests (no GPU) of the full-batch CPO entry points for 129-512-dim observations and up to 32 actions (spo_cpo512_*,
csrc/cpo.hip): the symbols are declared in include/safepo_hip.h, bound in safepo._abi and exported; spo_cpo512_supported is host
code with the documented truth table and leaves its neighbours' answers alone; every entry point refuses what lies outside its
range before any device work (there is no GPU here: anything that reached HIP would fail differently); and the cases of
tests/test_gpu_cpo_obs512.py keep that file's gates meaningful (two float32 summation orders against each bound)."""
import os
import re
import sys

import numpy as np
import pytest

import cpo_obs512_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["spo_cpo512_supported", "spo_cpo512_num_partials", "spo_cpo512_surrogate_grad", "spo_cpo512_fvp",
           "spo_cpo512_linesearch_eval", "spo_cpo512_actor_mean"]


@pytest.fixture(scope="module")
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    return g.LIB


@pytest.fixture(scope="module")
def lib(built_lib):
    from safepo import _abi
    return _abi.load(built_lib)


def test_symbols_declared_bound_and_exported(built_lib, lib):
    import ctypes
    from safepo import _abi
    header = open(os.path.join(ROOT, "include", "safepo_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(built_lib)
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name
        assert hasattr(raw, name), name
    # the argument lists of the spo_cpo128_* namesakes; the mean-only entry has spo_actor_mean's
    for what in ("supported", "num_partials", "surrogate_grad", "fvp", "linesearch_eval"):
        assert _abi.PROTOTYPES["spo_cpo512_" + what] == _abi.PROTOTYPES["spo_cpo128_" + what], what
    assert _abi.PROTOTYPES["spo_cpo512_actor_mean"] == _abi.PROTOTYPES["spo_actor_mean"]


def test_supported_truth_table(lib):
    for D in (0, 64, 128, 129, 376, 512, 513):
        for A in (0, 1, 16, 17, 32, 33):
            assert lib.spo_cpo512_supported(D, A) == int(129 <= D <= 512 and 1 <= A <= 32), (D, A)
    # the neighbours at the edges 128 / 129: unchanged
    from safepo import _abi
    from safepo.common.model import ActorVCritic
    assert [lib.spo_cpo128_supported(D, 4) for D in (64, 65, 128, 129)] == [0, 1, 1, 0]
    assert lib.spo_cpo128_supported(128, 16) == 1 and lib.spo_cpo128_supported(128, 17) == 0 and lib.spo_cpo128_supported(129, 16) == 0
    assert _abi.CPO_MAX_OBS == 64 and _abi.MAX_ACT == 16
    for D, A in ((128, 16), (129, 1), (376, 17)):
        assert ActorVCritic(D, A).kernels_supported("cpo") is False
    assert ActorVCritic(64, 16).kernels_supported("cpo") is True
    # exactly one of the two ranges, or neither
    for D in (128, 129):
        for A in (1, 16):
            assert lib.spo_cpo128_supported(D, A) + lib.spo_cpo512_supported(D, A) == 1


def test_partials_query(lib):
    last = 0
    for rows in (1, 63, 64, 65, 3037, 64 * 256 - 1, 64 * 256, 64 * 256 + 1, C.ROWS_CROSS_CHUNK, C.ROWS_THREE_CHUNKS, 4096 * 128):
        n = lib.spo_cpo512_num_partials(rows)
        assert n >= 1 and n >= last, rows
        assert n == min((rows + 63) // 64, 256) == lib.spo_cpo_num_partials(rows), rows
        last = n


def _calls(lib, D, A, rows, null):
    """Every entry point with in-range placeholders (never dereferenced on the host) or, null=True, a null pointer among them."""
    import ctypes
    buf = (ctypes.c_double * 8)()
    ok = ctypes.cast(buf, ctypes.c_void_p)
    first = None if null else ok
    return {
        "surrogate_grad": lambda: lib.spo_cpo512_surrogate_grad(first, ok, ok, ok, ok, 1.0, rows, D, A, ok, ok, ok, ok, None),
        "fvp": lambda: lib.spo_cpo512_fvp(first, ok, ok, rows, D, A, ok, ok, ok, None),
        "linesearch_eval": lambda: lib.spo_cpo512_linesearch_eval(first, ok, ok, ok, ok, ok, ok, ok, rows, D, A, ok, 3, ok, None),
        "actor_mean": lambda: lib.spo_cpo512_actor_mean(first, ok, ok, rows, D, A, None),
    }


def test_refusals_happen_on_the_host(lib):
    for D, A, word in ((128, 4, b"obs_dim"), (513, 4, b"obs_dim"), (376, 33, b"act_dim")):
        for name, call in _calls(lib, D, A, 64, null=False).items():
            assert call() == -2, (name, D, A)
            assert word in lib.spo_last_error(), (name, D, A, lib.spo_last_error())
    for name, call in _calls(lib, 376, 17, 0, null=False).items():           # rows = 0
        assert call() == -1, name
        assert b"bad args" in lib.spo_last_error(), (name, lib.spo_last_error())
    for name, call in _calls(lib, 376, 17, 64, null=True).items():           # a null pointer
        assert call() == -1, name
        assert b"bad args" in lib.spo_last_error(), (name, lib.spo_last_error())


def _allclose_with_a_factor_to_spare(a, b, rtol, atol, spare=3.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= (atol + rtol * np.abs(b)) / spare).all())


@pytest.mark.parametrize("D,A,M", C.CASES)
def test_cases_keep_the_gates_meaningful(D, A, M):
    """For every (shape, rows) case of the GPU file: the float32 oracle on 1 and on 4 torch threads (two summation orders), the
    float64 oracle once.  Each assert_allclose / approx bound of the GPU test holds between the two float32 evaluations with a
    factor of 3 to spare -- a correct float32 result that sums in another order is not refused by them -- and each fp64-yardstick
    gate has a non-zero float32 distance or a non-zero floor."""
    a, b, o64 = C.oracle(D, A, M, "float32", 1), C.oracle(D, A, M, "float32", C.ORACLE_THREADS), C.oracle(D, A, M, "float64")
    tag = f"({D}, {A}, M {M})"
    for o in (a, b, o64):
        for k, val in o.items():
            assert np.isfinite(val).all(), (tag, k)
    assert o64["floor"] > 0
    for name in ("grad_r", "grad_c"):
        # np.testing.assert_allclose(g, g_ref, rtol=1e-4, atol=1e-5 * max|g_ref|)
        assert _allclose_with_a_factor_to_spare(a[name], b[name], 1e-4, 1e-5 * np.abs(b[name]).max()), (tag, name)
        assert np.abs(o64[name]).max() > 0
    for name in ("loss_r", "loss_c"):
        assert abs(b[name] - o64[name]) > 0 or o64["floor"] > 0, (tag, name)
    scale = np.abs(o64["Fv"]).max()
    assert scale > 0                                                          # 3 d_32 + 1e-6 * scale: the floor is not zero
    # np.testing.assert_allclose(hv, hv32, rtol=1e-4, atol=1e-5 * scale)
    assert _allclose_with_a_factor_to_spare(a["Fv"], b["Fv"], 1e-4, 1e-5 * scale), tag
    if not C.line_search_checked(M):
        assert "moved_kl" not in o64
        return
    # kl == pytest.approx(kl32, rel=1e-4); _gate(kl, kl32, kl64, 1e-6 * kl64)
    assert o64["moved_kl"] > 0 and abs(a["moved_kl"] - b["moved_kl"]) <= 1e-4 * abs(b["moved_kl"]) / 3.0, (tag, a["moved_kl"], b["moved_kl"])
    for name in ("moved_loss_r", "moved_loss_c"):
        assert abs(b[name] - o64[name]) > 0 or o64["floor"] > 0, (tag, name)
