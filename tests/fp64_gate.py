"""Test helper (NOT a test module): the rule every kernel of this project is accepted by, in one place.

A blanket relative tolerance either fails on rounding noise or hides defects.  Instead the oracle is evaluated twice on the same
inputs -- in float32 (the reference's arithmetic) and in float64 (the yardstick) -- and the HIP result must be as close to
float64 as the float32 oracle is:

    |hip - f64| <= C |f32 - f64| + floor          (C = 3)

in max-norm and, unless switched off, in L2 (floor * sqrt(n)): a deviation has to be SHOWN to be rounding of the size the
reference itself has.  The floor is a fraction of the quantity's scale (1e-6 for single evaluations) or an absolute number.
Every gate computes its deviations once, prints them with the floor, asserts the inequality as written above, and returns the
ratio |hip - f64| / (C |f32 - f64| + floor) it printed from.  numpy and the standard library only."""
from __future__ import annotations

import contextlib
from typing import NamedTuple

import numpy as np

C = 3.0
REL_FLOOR = 1e-6
NORMS, MAX, L2 = ("max", "l2"), ("max",), ("l2",)
ORACLE_THREADS = 4


class Gate(NamedTuple):
    ratio: float          # worst |hip - f64| / (c |f32 - f64| + floor) over the checked norms; <= 1 passes
    d_hip: float          # max |hip - f64|
    d_32: float           # max |f32 - f64|
    scale: float          # the scale the relative floor was taken of
    ratios: np.ndarray    # per element: |hip - f64| / (c max|f32 - f64| + floor)
    what: str


def _check(dh, d32, floor, c, norms, scale, what, enforce=True, note=None, cases=None):
    """The only place the inequality is written.  dh, d32: |hip - f64|, |f32 - f64| per element."""
    assert norms and set(norms) <= set(NORMS), norms
    n = np.sqrt(dh.size)
    sides = {"max": ("max", dh.max(), d32.max(), floor), "l2": ("L2", np.linalg.norm(dh), np.linalg.norm(d32), floor * n)}
    sides = [sides[k] for k in NORMS if k in norms]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = max(a / (c * b + fl) for _, a, b, fl in sides)
        g = Gate(float(ratio), float(dh.max()), float(d32.max()), scale, dh / (c * d32.max() + floor), what)
    if note is not None:
        note(g)
    if enforce:
        head, tail = (what, "") if cases is None else (f"{what} ({cases} cases)", " (of each case's scale)")
        print(f"{head}: " + ";  ".join(f"{name} |hip-f64| {a:.3e}  |f32-f64| {b:.3e}  floor {fl:.3e}" for name, a, b, fl in sides) + tail)
        for name, a, b, fl in sides:
            assert a <= c * b + fl, \
                f"{head}: {name} |hip - f64| {a:.3e} > {c} x |f32 - f64| {b:.3e} + floor {fl:.3e} (element {int(dh.argmax())} is the furthest)"
    return g


def gate(hip, f32, f64, what="", c=C, scale=None, rel_floor=REL_FLOOR, floor=None, norms=NORMS, enforce=True, note=None):
    """One array (or scalar).  scale: None -> max|f64|; a number; or an array of per-element scales (each element is divided by
    its own and the vector gated at scale 1).  floor: an absolute floor in place of rel_floor * scale.  norms: which of "max" and
    "l2" are checked.  enforce=False measures only: no line, no inequality (the shapes and finiteness are still asserted).
    note: called with the Gate before the inequality is asserted, so that a refused gate's ratio is on record too."""
    hip, f32, f64 = (np.asarray(t, np.float64).reshape(-1) for t in (hip, f32, f64))
    assert hip.shape == f32.shape == f64.shape, (what, hip.shape, f32.shape, f64.shape)
    assert np.isfinite(hip).all(), f"{what}: non-finite HIP values"
    if np.ndim(scale) > 0:
        s = np.maximum(np.asarray(scale, np.float64).reshape(-1), 1e-30)
        hip, f32, f64, scale = hip / s, f32 / s, f64 / s, 1.0
    sc = max(float(np.abs(f64).max()) if scale is None else float(scale), 1e-30)
    fl = rel_floor * sc if floor is None else float(floor)
    return _check(np.abs(hip - f64), np.abs(f32 - f64), fl, c, norms, sc, what, enforce, note)


def gate_group(members, what="", c=C, rel_floor=REL_FLOOR, l2=True, note=None):
    """Scalars of ONE kind over several cases: a single scalar's |f32 - f64| is one draw of the reference's rounding noise -- it
    can be 0 by chance --, so the yardstick is the float32 oracle's largest deviation in the group (and, with l2, its
    root-mean-square one).  members: [(hip, f32, f64, scale)]; every member is divided by its own scale and the group gated at
    scale 1; scale None: the member's relative deviation |x - f64| / |f64|.  Gate.ratios holds every member's own ratio, Gate.d_32
    the yardstick."""
    hip, f32, f64 = (np.array([m[k] for m in members], np.float64) for k in (0, 1, 2))
    assert np.isfinite(hip).all(), f"{what}: non-finite HIP values"
    if all(m[3] is None for m in members):
        s = np.maximum(np.abs(f64), 1e-30)
        dh, d32 = np.abs(hip - f64) / s, np.abs(f32 - f64) / s
    else:
        s = np.maximum(np.abs(np.array([m[3] for m in members], np.float64)), 1e-30)
        dh, d32 = np.abs(hip / s - f64 / s), np.abs(f32 / s - f64 / s)
    return _check(dh, d32, rel_floor, c, NORMS if l2 else MAX, 1.0, what, note=note, cases=len(members))


def gate_rows(hip, f32, f64, what="", names=None, **kw):
    """Logged scalars of several steps ([steps, columns]): every COLUMN (a loss, a norm, ...) is gated over the steps with its own
    scale, so a small column is not hidden behind a large one.  -> the worst ratio."""
    hip, f32, f64 = (np.asarray(t, np.float64) for t in (hip, f32, f64))
    assert hip.shape == f32.shape == f64.shape, (what, hip.shape, f32.shape, f64.shape)
    return max(gate(hip[:, k], f32[:, k], f64[:, k], f"{what} column {names[k] if names else k}", **kw).ratio for k in range(hip.shape[1]))


def gate_blocks(hip, f32, f64, blocks, what="", **kw):
    """A flat parameter vector, every block (offset, count) with its own scale.  -> the worst ratio."""
    return max(gate(hip[o:o + n], f32[o:o + n], f64[o:o + n], f"{what} block [{o}, {o + n})", **kw).ratio for o, n in blocks if n > 0)


class Ratios(dict):
    """The worst ratio per key and the label of the gate it came from: {key: (ratio, label)}."""

    def note(self, key, ratio, label=""):
        if ratio >= self.get(key, (-1.0, ""))[0]:
            self[key] = (float(ratio), label)


@contextlib.contextmanager
def on_oracle_threads(threads=ORACLE_THREADS):
    """Context manager and decorator (@on_oracle_threads()): the oracles run on `threads` torch threads whatever the host offers
    (blocked sums round differently with the thread count), and the count is put back."""
    import torch
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        yield
    finally:
        torch.set_num_threads(before)
