"""CPU companion (no GPU) of tests/test_gpu_full_batch_actor.py: the float32 and float64 oracles of every case of
tests/full_batch_actor_cases.py except the two largest row counts (16 477 and 49 169), and the conditions under which that
file's gates say something -- every value finite, the KL at moved parameters well above float32 rounding, the surrogate a
mean of O(1) terms, group yardsticks that are not zero -- and the gates themselves fed the float32 oracle in the HIP result's
place."""
import numpy as np
import pytest
import torch

import full_batch_actor_cases as C


@pytest.fixture(autouse=True)
def _leave_no_global_state():
    rng, noted = torch.get_rng_state(), dict(C.RATIOS)
    yield
    torch.set_rng_state(rng)
    C.RATIOS.clear()
    C.RATIOS.update(noted)


def test_case_tables():
    assert {C.kin(D) for D, _ in C.CPO_SHAPES} == {16, 32, 64} == {C.kin(D) for D, _ in C.CPO_FORM_SHAPES}
    assert {C.kin(D) for D, _ in C.ACTOR_SHAPES} == {16, 32, 64, 128}
    assert any(D % 4 and A % 4 for D, A in C.CPO_SHAPES) and any(D % 4 for D, _ in C.ACTOR_SHAPES)
    for D, A in C.CPO_SHAPES + C.ACTOR_SHAPES:
        assert 1 <= A <= 16 and 1 <= D <= 128
    # the launch arithmetic the row counts stand for (spo_cpo_num_partials; spo_cpo_linesearch_eval; spo_actor_kl's 768-workgroup grid)
    chunks = lambda rows: (rows + 63) // 64
    assert chunks(C.CPO_ROWS_ALL) == 48 and C.CPO_ROWS_ALL % 64 == 29
    assert chunks(C.CPO_ROWS_CROSS_CHUNK) == 256 + 2 and chunks(C.CPO_ROWS_CROSS_CHUNK - 64 - 29) == 256 and C.CPO_ROWS_CROSS_CHUNK % 64 == 29
    assert [cap // 3 for cap in C.LS_CAPPED] == [1, 2] and 2 // 3 == 0
    tiles = lambda rows: (rows + 15) // 16
    assert tiles(1000) == 63 and [-(-63 // (4 * cap)) for cap in C.KL_CAPPED] == [16, 8]
    rows = C.ACTOR_SECOND_TILE[2]
    assert tiles(rows) > 768 * 4 >= tiles(rows - 17) and rows % 16 != 0 and max(C.ACTOR_ROWS) < 768 * 64
    assert set(C.HOST_CPO_ROWS) == set(C.CPO_CASES) - {C.CPO_ROWS_CROSS_CHUNK}


@pytest.mark.parametrize("M", C.HOST_CPO_ROWS)
def test_cpo_cases_keep_the_gates_meaningful(M):
    groups = {"surrogate": [], "line search at theta_old": [], "line search at moved parameters": [], "KL at moved parameters": []}
    for D, A in C.CPO_CASES[M]:
        o32, o64 = C.cpo_oracle(D, A, M, "float32"), C.cpo_oracle(D, A, M, "float64")
        tag, s = f"({D}, {A}, M {M})", o64["adv_scale"]
        for o in (o32, o64):
            for k, val in o.items():
                assert np.isfinite(val).all(), (tag, k)
        assert s > 0
        assert o64["moved_kl"] >= 1e-5, (tag, o64["moved_kl"])
        assert o64["ratio_spread"] < 1 and o64["moved_ratio_spread"] < 1, (tag, o64["ratio_spread"], o64["moved_ratio_spread"])
        for name in ("grad_r", "grad_c", "Fv"):
            assert np.abs(o64[name]).max() > 0
            C.gate_vector("host", D, M, o32[name], o32[name], o64[name], f"{name} {tag}")
        for which in ("r", "c"):
            groups["surrogate"].append((f"{which} {tag}", D, o32["loss_" + which], o32["loss_" + which], o64["loss_" + which], s))
            groups["line search at theta_old"].append(groups["surrogate"][-1])
            k = "moved_loss_" + which
            groups["line search at moved parameters"].append((f"{which} {tag}", D, o32[k], o32[k], o64[k], s))
        groups["KL at moved parameters"].append((tag, D, o32["moved_kl"], o32["moved_kl"], o64["moved_kl"], None))
        # the symmetry tolerance of the GPU test is the float32 oracle's own asymmetry + 1e-6 |u.Fv|: the float64 one must be far below
        assert abs(o64["uFv"] - o64["vFu"]) <= 1e-10 * abs(o64["uFv"]), tag
        assert abs(o64["uFv"]) > 0
    for what, members in groups.items():
        assert C.gate_group("host", M, members, what) > 0, what


def test_gates_refuse_an_error_of_1e_4():
    """The other side of the gates: one element of a vector, or one member of a group, off by 1e-4 of the scale -- a stale row,
    a wrong lane mask -- fails, at the largest vector and at the noisiest row count (M = 1) alike.  The KL of a single row is
    the exception: 0.5 (vr + dm^2 - 1 - log vr) cancels to ~1e-4 of its terms, the float32 oracle itself is 7e-5 (relative) off
    there, and the error the gate is shown at M = 1 is 1e-2."""
    for D, A, M, kl_off in ((64, 16, C.CPO_ROWS_ALL, 1e-4), (12, 2, 1, 1e-2)):
        o32, o64 = C.cpo_oracle(D, A, M, "float32"), C.cpo_oracle(D, A, M, "float64")
        for name in ("grad_r", "Fv"):
            off = o32[name].copy()
            off[off.size // 2] += 1e-4 * np.abs(o64[name]).max()
            with pytest.raises(AssertionError):
                C.gate_vector("host", D, M, off, o32[name], o64[name], name)
        def group(key, scaled, off):
            """The float32 oracle in the HIP result's place at every shape of M, `off` added at (D, A)."""
            rows = []
            for d, a in C.CPO_CASES[M]:
                r32, r64 = C.cpo_oracle(d, a, M, "float32"), C.cpo_oracle(d, a, M, "float64")
                rows.append((f"({d}, {a})", d, r32[key] + (off if (d, a) == (D, A) else 0.0), r32[key], r64[key], r64["adv_scale"] if scaled else None))
            return rows
        with pytest.raises(AssertionError):
            C.gate_group("host", M, group("moved_loss_r", True, 1e-4 * o64["adv_scale"]), "loss")
        with pytest.raises(AssertionError):
            C.gate_group("host", M, group("moved_kl", False, kl_off * o64["moved_kl"]), "KL")


@pytest.mark.parametrize("rows", C.ACTOR_ROWS)
def test_actor_cases_keep_the_gates_meaningful(rows):
    members = []
    for D, A in C.ACTOR_SHAPES:
        o32, o64 = C.actor_oracle(D, A, rows, "float32"), C.actor_oracle(D, A, rows, "float64")
        tag = f"({D}, {A}, rows {rows})"
        assert o64["mean"].shape == (rows, A)
        assert np.isfinite(o32["mean"]).all() and np.isfinite(o64["mean"]).all() and np.isfinite([o32["kl"], o64["kl"]]).all(), tag
        assert o64["kl"] >= 1e-5, (tag, o64["kl"])
        assert np.abs(o64["mean"]).max() > 0
        C.gate_vector("host", D, rows, o32["mean"], o32["mean"], o64["mean"], f"means {tag}")
        members.append((tag, D, o32["kl"], o32["kl"], o64["kl"], None))
    assert C.gate_group("host", rows, members, "KL at moved parameters") > 0
