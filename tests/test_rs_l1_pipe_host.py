"""CPU tests (no GPU) of the row-split kernel's unclipped fast path: spo_debug_clip_threshold is declared, exported and bound, is
host code, and the threshold it returns is one under which the joint clip's coefficient is exactly 1.0 in float32 -- so a step the
kernel's scalar test finds at or below it may skip the square root, the division and the multiplies by the coefficient."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMS = (40.0, 1.2, 0.5, 1e-2, 1e-3, 1e-6, 0.0)


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from safepo import _abi
    return _abi.load(g.LIB)


def _threshold(lib, mg):
    from safepo import _abi
    out = ctypes.c_float(float("nan"))
    rc = lib.spo_debug_clip_threshold(float(mg), ctypes.byref(out))
    assert rc == 0, (mg, lib.spo_last_error())
    return np.float32(out.value)


def _coef_f32(mg, t):
    """min(1, mg / (sqrt(t) + 1e-6)) operation by operation in float32 (clip_grad_norm_'s coefficient as the kernel forms it)."""
    mg, t = np.float32(mg), np.float32(t)
    norm = np.sqrt(t, dtype=np.float32)
    den = np.float32(norm + np.float32(1e-6))
    coef = np.float32(mg / den)
    return np.float32(1.0) if coef > np.float32(1.0) else coef


def test_symbol_declared_exported_and_bound(lib):
    from safepo import _abi
    header = open(os.path.join(ROOT, "include", "safepo_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "spo_debug_clip_threshold" in set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    assert "spo_debug_clip_threshold" in _abi.PROTOTYPES and hasattr(lib, "spo_debug_clip_threshold")


@pytest.mark.parametrize("mg", NORMS)
def test_coefficient_is_exactly_one_up_to_the_threshold(lib, mg):
    thr = _threshold(lib, mg)
    assert np.isfinite(thr)
    if thr < 0:
        assert thr == np.float32(-1.0)              # "never taken": no squared norm is <= -1
    else:
        with np.errstate(divide="ignore"):
            for t in (thr, np.nextafter(thr, np.float32(0.0)), np.float32(thr / np.float32(2.0)), np.float32(0.0)):
                c = _coef_f32(mg, t)
                assert c.dtype == np.float32 and c == np.float32(1.0), (mg, float(thr), float(t), float(c))
    if mg in (40.0, 1.2, 0.5):
        assert float(thr) >= (0.99 * mg) ** 2, (mg, float(thr))        # the fast path is not vacuous at the norms in use
        assert float(thr) <= (0.999 * float(np.float32(mg))) ** 2      # ... and is the documented one: not above (0.999 mg)^2


def test_threshold_is_the_largest_float_not_above_its_bound(lib):
    for mg in (40.0, 1.2, 0.5, 1e-2, 2e-3, 7.25, 1e4):
        thr = _threshold(lib, mg)
        lim2 = (0.999 * float(np.float32(mg))) ** 2
        assert float(thr) <= lim2 < float(np.nextafter(thr, np.float32(np.inf))), (mg, float(thr), lim2)
    assert _threshold(lib, np.nextafter(np.float32(2e-3), np.float32(0.0))) == np.float32(-1.0)
    assert _threshold(lib, float("inf")) == np.finfo(np.float32).max      # every finite squared norm is below an infinite bound
    assert _threshold(lib, 3e19) == np.finfo(np.float32).max              # (0.999 mg)^2 beyond the float range


def test_argument_errors(lib):
    out = ctypes.c_float(0.0)
    assert lib.spo_debug_clip_threshold(1.0, None) < 0 and b"null" in lib.spo_last_error()
    assert lib.spo_debug_clip_threshold(-1.0, ctypes.byref(out)) < 0 and b"max_grad_norm" in lib.spo_last_error()
    assert lib.spo_debug_clip_threshold(float("nan"), ctypes.byref(out)) < 0 and b"max_grad_norm" in lib.spo_last_error()
    assert out.value == 0.0                                               # a refused call writes nothing
