"""CPU test of tests/fp64_gate.py, the rule |hip - f64| <= c |f32 - f64| + floor itself, on hand-built inputs of 1 to 8 elements
whose deviations, floors and bounds are exact in float64 (powers of two and small integers), so the boundary is met to the bit."""
import numpy as np
import pytest

import fp64_gate as G

UP = lambda x: float(np.nextafter(x, np.inf))
Z4 = np.zeros(4)
YARD = np.array([1.0, 0.0, 0.0, 0.0])          # |f32 - f64|: max 1, L2 1; with floor 0.5 the bounds are 3.5 (max) and 3 + 0.5 * 2 = 4 (L2)


def refused(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def passes(fn, *a, **k):
    try:
        fn(*a, **k)
    except AssertionError:
        return False
    return True


def test_max_norm_boundary_to_the_bit():
    for n in (1, 4):
        hip, f32 = np.zeros(n), np.zeros(n)
        hip[-1], f32[0] = 3.5, -1.0                                  # deviations of either sign, in different elements
        assert G.gate(hip, f32, np.zeros(n), "on the bound", floor=0.5, norms=G.MAX).ratio == 1.0
        hip[-1] = UP(3.5)
        refused(G.gate, hip, f32, np.zeros(n), "one ulp over", floor=0.5, norms=G.MAX)
        hip[-1] = -UP(3.5)
        refused(G.gate, hip, f32, np.zeros(n), "one ulp over, below", floor=0.5, norms=G.MAX)


def test_l2_boundary_and_the_norm_switch():
    on, over = np.array([4.0, 0, 0, 0]), np.array([UP(4.0), 0, 0, 0])
    assert G.gate(on, YARD, Z4, "L2 on the bound", floor=0.5, norms=G.L2).ratio == 1.0
    refused(G.gate, over, YARD, Z4, "L2 one ulp over", floor=0.5, norms=G.L2)
    wide = np.array([3.0, 3.0, 0, 0])                                # max 3 <= 3.5, L2 sqrt(18) = 4.24 > 4
    refused(G.gate, wide, YARD, Z4, "max passes, L2 refuses", floor=0.5)
    refused(G.gate, wide, YARD, Z4, "max passes, L2 refuses", floor=0.5, norms=G.L2)
    assert G.gate(wide, YARD, Z4, "L2 is not made", floor=0.5, norms=G.MAX).ratio == 3.0 / 3.5
    peak = np.array([3.75, 0, 0, 0])                                 # max 3.75 > 3.5, L2 3.75 <= 4
    refused(G.gate, peak, YARD, Z4, "L2 passes, max refuses", floor=0.5)
    refused(G.gate, peak, YARD, Z4, "L2 passes, max refuses", floor=0.5, norms=G.MAX)
    assert G.gate(peak, YARD, Z4, "max is not made", floor=0.5, norms=G.L2).ratio == 3.75 / 4.0
    refused(G.gate, wide, YARD, Z4, "no norm at all", floor=0.5, norms=())


def test_scales_and_floors():
    f64 = np.array([2.0, -4.0])
    # scale=None: max|f64| = 4, floor 0.25 * 4 = 1
    g = G.gate([2.0, -3.0], f64, f64, "scale None", rel_floor=0.25)
    assert (g.scale, g.d_hip, g.d_32, g.ratio) == (4.0, 1.0, 0.0, 1.0)
    refused(G.gate, [2.0, float(np.nextafter(-3.0, 0.0))], f64, f64, "scale None, one ulp over", rel_floor=0.25, norms=G.MAX)
    # a number: floor 0.25 * 8 = 2
    assert G.gate([4.0, -4.0], f64, f64, "scale 8", scale=8.0, rel_floor=0.25, norms=G.MAX).ratio == 1.0
    refused(G.gate, [UP(4.0), -4.0], f64, f64, "scale 8, one ulp over", scale=8.0, rel_floor=0.25, norms=G.MAX)
    # an array: every element over its own scale, floor 0.25 at scale 1 -> 0.5 on the first element, 2 on the second
    g = G.gate([2.5, -6.0], f64, f64, "per-element scales", scale=[2.0, 8.0], rel_floor=0.25, norms=G.MAX)
    assert (g.scale, g.d_hip, g.ratio) == (1.0, 0.25, 1.0) and list(g.ratios) == [1.0, 1.0]
    refused(G.gate, [UP(2.5), -4.0], f64, f64, "first element over its own floor", scale=[2.0, 8.0], rel_floor=0.25, norms=G.MAX)
    refused(G.gate, [2.0, -UP(6.0)], f64, f64, "second element over its own floor", scale=[2.0, 8.0], rel_floor=0.25, norms=G.MAX)
    # an absolute floor overrides the relative one, whatever the scale
    assert G.gate([2.0, -3.5], f64, f64, "absolute floor", rel_floor=0.25, floor=0.5, norms=G.MAX).ratio == 1.0
    refused(G.gate, [2.0, -3.0], f64, f64, "absolute floor", rel_floor=0.25, floor=0.5, norms=G.MAX)
    refused(G.gate, [2.0, -3.0], f64, f64, "absolute floor", scale=100.0, floor=0.5, norms=G.MAX)
    # the default: 1e-6 of the scale
    assert G.gate([2.0, -4.0 + 3e-6], f64, f64, "default floor").ratio == pytest.approx(0.75, rel=1e-9)
    refused(G.gate, [2.0, -4.0 + 5e-6], f64, f64, "default floor")


def test_zero_reference_does_not_divide_by_zero():
    with np.errstate(all="raise"):
        g = G.gate(np.zeros(3), np.zeros(3), np.zeros(3), "all zero")
        assert (g.ratio, g.scale) == (0.0, 1e-30)
        refused(G.gate, [0.0, 1e-20, 0.0], np.zeros(3), np.zeros(3), "zero reference, non-zero result")
        assert G.gate_group([(0.0, 0.0, 0.0, None)], "zero member").ratio == 0.0
        assert G.gate_group([(0.0, 0.0, 0.0, 0.0)], "zero scale").ratio == 0.0


def test_group_gate():
    lucky = (2.0, 0.0, 0.0, 1.0)                                     # its own |f32 - f64| is 0: one draw of the noise
    noisy = (0.0, 1.0, 0.0, 1.0)
    g = G.gate_group([lucky, noisy], "group", rel_floor=0.5)
    assert (g.d_hip, g.d_32, g.scale) == (2.0, 1.0, 1.0) and list(g.ratios) == [2.0 / 3.5, 0.0] and g.ratio == 2.0 / 3.5      # L2: 2 / (3 + 0.5 sqrt(2)) is smaller
    refused(G.gate_group, [lucky], "alone", rel_floor=0.5)
    # per-member scales: 8 / 4 = 2 passes where 8 would not; the yardstick is scaled too (4 / 4 = 1)
    g = G.gate_group([(8.0, 0.0, 0.0, 4.0), (0.0, -4.0, 0.0, -4.0)], "scaled", rel_floor=0.5)
    assert (g.d_hip, g.d_32) == (2.0, 1.0)
    refused(G.gate_group, [(8.0, 0.0, 0.0, 1.0), (0.0, -4.0, 0.0, 4.0)], "first member at scale 1", rel_floor=0.5)
    # scale None: each member against its own |f64|
    g = G.gate_group([(12.0, 8.0, 8.0, None), (-2.0, -2.25, -2.0, None)], "relative", rel_floor=0.125)
    assert (g.d_hip, g.d_32) == (0.5, 0.125) and g.ratios[0] == 1.0
    refused(G.gate_group, [(UP(12.0), 8.0, 8.0, None), (-2.0, -2.25, -2.0, None)], "relative, one ulp over", rel_floor=0.125, l2=False)
    # the boundary of the max-norm, and the L2 switch: max 3 <= 3.5, L2 sqrt(27) = 5.2 > 3 + 0.5 * 2
    assert G.gate_group([(3.5, 0.0, 0.0, 1.0), noisy], "on the bound", rel_floor=0.5, l2=False).ratio == 1.0
    refused(G.gate_group, [(UP(3.5), 0.0, 0.0, 1.0), noisy], "one ulp over", rel_floor=0.5, l2=False)
    three = [noisy] + [(3.0, 0.0, 0.0, 1.0)] * 3
    refused(G.gate_group, three, "L2 refuses", rel_floor=0.5)
    assert G.gate_group(three, "L2 is not made", rel_floor=0.5, l2=False).ratio == 3.0 / 3.5
    refused(G.gate_group, [(float("nan"), 0.0, 0.0, 1.0), noisy], "non-finite member")


def test_refusals_and_the_factor():
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(AssertionError, match="non-finite"):
            G.gate([0.0, bad], [0.0, 0.0], [0.0, 0.0], "non-finite", floor=1.0)
        with pytest.raises(AssertionError, match="non-finite"):
            G.gate([0.0, bad], [0.0, 0.0], [0.0, 0.0], "non-finite, measuring only", floor=1.0, enforce=False)
    refused(G.gate, [0.0, 0.0, 0.0], [0.0, 0.0], [0.0, 0.0], "shapes", floor=1.0)
    refused(G.gate, [0.0, 0.0], [0.0, 0.0], [[0.0, 0.0], [0.0, 0.0]], "shapes", floor=1.0)
    refused(G.gate_rows, np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((3, 2)), "shapes")
    assert G.C == 3.0
    assert G.gate([2.5], [1.0], [0.0], "c = 2 on the bound", c=2.0, floor=0.5).ratio == 1.0
    refused(G.gate, [3.0], [1.0], [0.0], "c = 2", c=2.0, floor=0.5)
    assert G.gate([3.0], [1.0], [0.0], "c = 3", floor=0.5).ratio == 3.0 / 3.5
    assert G.gate_group([(2.5, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 1.0)], "group, c = 2", c=2.0, rel_floor=0.5, l2=False).ratio == 1.0
    refused(G.gate_group, [(3.0, 0.0, 0.0, 1.0), (0.0, 1.0, 0.0, 1.0)], "group, c = 2", c=2.0, rel_floor=0.5, l2=False)


def test_ratio_is_the_hand_computed_one_and_tells_the_verdict(capsys):
    hip = np.array([3.0, 3.0, 0.0, 0.0])
    g = G.gate(hip, YARD, Z4, "measured", floor=0.5, enforce=False)
    assert g.ratio == max(3.0 / 3.5, np.sqrt(18.0) / 4.0) and (g.d_hip, g.d_32, g.what) == (3.0, 1.0, "measured")
    assert list(g.ratios) == [3.0 / 3.5, 3.0 / 3.5, 0.0, 0.0]
    assert capsys.readouterr().out == ""
    rng = np.random.default_rng(0)
    seen = set()
    for k in range(200):
        n = int(rng.integers(1, 9))
        f64, f32 = rng.standard_normal(n), rng.standard_normal(n) * 10.0 ** rng.integers(-8, 1)
        hip = f64 + rng.standard_normal(n) * 10.0 ** rng.integers(-8, 1)
        kw = dict(rel_floor=10.0 ** rng.integers(-7, -1), norms=(G.NORMS, G.MAX, G.L2)[k % 3])
        ok = passes(G.gate, hip, f64 + f32, f64, "random", **kw)
        assert ok == (G.gate(hip, f64 + f32, f64, "random", enforce=False, **kw).ratio <= 1.0)
        seen.add(ok)
    assert seen == {True, False}
    capsys.readouterr()
    G.gate(hip[:1] * 0 + 3.0, [1.0], [0.0], "the line", floor=0.5)
    assert capsys.readouterr().out == ("the line: max |hip-f64| 3.000e+00  |f32-f64| 1.000e+00  floor 5.000e-01;  "
                                       "L2 |hip-f64| 3.000e+00  |f32-f64| 1.000e+00  floor 5.000e-01\n")


def test_rows_and_blocks_gate_every_part_at_its_own_scale():
    f64 = np.array([[1000.0, 1.0], [-1000.0, -1.0]])
    hip = f64 + np.array([[1e-4, 0.0], [0.0, 1e-4]])                 # 1e-7 of column 0, 1e-4 of column 1
    G.gate(hip, f64, f64, "as one array: hidden behind the large column")
    refused(G.gate_rows, hip, f64, f64, "per column")
    noted = []
    assert G.gate_rows(hip, f64, f64, "per column", names=["big", "small"], rel_floor=1e-3, note=noted.append) == pytest.approx(0.1)
    assert [(g.what, g.scale) for g in noted] == [("per column column big", 1000.0), ("per column column small", 1.0)]
    flat = lambda a: a.T.reshape(-1)                                 # [big, big, small, small]
    refused(G.gate_blocks, flat(hip), flat(f64), flat(f64), [(0, 2), (2, 2)], "per block", note=noted.append)
    assert noted[-1].what == "per block block [2, 4)" and noted[-1].ratio == pytest.approx(100.0)      # noted although refused
    assert G.gate_blocks(flat(hip), flat(f64), flat(f64), [(0, 2), (2, 0), (2, 2)], "per block", rel_floor=1e-3) == pytest.approx(0.1)


def test_record_keeps_the_worst_ratio_per_key_and_its_label():
    r = G.Ratios()
    r.note("a", 0.25, "first")
    r.note("a", 0.5, "worst")
    r.note("a", 0.125, "later and smaller")
    r.note(("b", 1), 0.0, "zero is noted too")
    assert dict(r) == {"a": (0.5, "worst"), ("b", 1): (0.0, "zero is noted too")}
    r.note("a", 0.5, "the last of equals")
    assert r["a"] == (0.5, "the last of equals")
    saved = dict(r)
    r.clear()
    assert not r
    r.update(saved)
    assert r["a"][0] == 0.5


def test_oracle_threads_are_set_and_put_back():
    import torch
    before = torch.get_num_threads()
    try:
        torch.set_num_threads(3)
        seen = G.on_oracle_threads()(torch.get_num_threads)()
        assert (seen, torch.get_num_threads()) == (G.ORACLE_THREADS, 3)
        with G.on_oracle_threads(1):
            assert torch.get_num_threads() == 1
        with pytest.raises(KeyError):
            with G.on_oracle_threads():
                raise KeyError
        assert torch.get_num_threads() == 3
    finally:
        torch.set_num_threads(before)
