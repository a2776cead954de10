"""CPU companion (no GPU) of tests/test_gpu_wide_kernels.py: the float32 and float64 oracles of the cases of
tests/wide_kernel_cases.py, and the conditions under which that file's gates say something -- every value finite, every branch
class populated (>= 10 % of the rows, by the draw alone), no row within 1e-4 of a discontinuity after the redraw, float32 and
float64 in the same branch in every row, yardsticks that are not zero -- and the gates themselves: fed the float32 oracle in the HIP
result's place they pass with ratio <= 1/3, fed a deliberately wrong oracle (a one-line variant each) they refuse.  Also here:
csrc/adam.h's adam1 restated in float32 numpy, refused by the adam_v gate with the weights 1.f - beta and accepted with
(float)(1.0 - beta), and the stand-alone check of csrc/adam_host.h (tests/adam_host_check.cpp, host compiler)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import wide_kernel_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "safe-policy-optimization_amd", "csrc")


@pytest.fixture(autouse=True)
def _leave_no_global_state():
    rng, noted = torch.get_rng_state(), dict(C.RATIOS)
    yield
    torch.set_rng_state(rng)
    C.RATIOS.clear()
    C.RATIOS.update(noted)


def _finite(*oracles):
    for o in oracles:
        for k, v in o.items():
            if isinstance(v, (np.ndarray, float)):
                assert np.isfinite(v).all(), k


def _third(ratio):
    assert ratio <= 1.0 / 3.0 + 1e-12, ratio


def _refused(fn):
    with pytest.raises(AssertionError):
        fn()


def test_case_tables():
    # the launch arithmetic the row counts stand for: G = pow2ceil(act_dim) lanes per row, four waves of 64 / G rows per workgroup
    assert [C.pow2ceil(a) for a in C.ACT_DIMS] == [1, 2, 4, 16, 32, 64, 64] and [C.rpb(a) for a in C.ACT_DIMS] == [256, 128, 64, 16, 8, 4, 4]
    assert C.actor_rows(64) == [1, 3, 4, 5, 1000] and C.actor_rows(1) == [1, 255, 256, 257, 1000]
    assert C.LOSS_PAST_CAP == [(64, 1025), (1, 65537)] and C.LS_PAST_CAP == [(64, 2049), (1, 131073)]
    blocks = lambda rows, A, cap: min(-(-rows // C.rpb(A)), cap)
    assert all(blocks(r, A, C.LOSS_CAP) == C.LOSS_CAP and r == C.LOSS_CAP * C.rpb(A) + 1 for A, r in C.LOSS_PAST_CAP)
    assert all(blocks(r, A, C.LS_CAP) == C.LS_CAP and r == C.LS_CAP * C.rpb(A) + 1 for A, r in C.LS_PAST_CAP)
    assert max(blocks(1000, A, C.LOSS_CAP) for A in C.ACT_DIMS) == 250                                # 1 000 rows stay under the cap
    assert (C.ACTOR_PARTIAL, C.SPLIT_PARTIAL, C.PPO_PARTIAL) == (256 * 66, 256 * 131, 256 * 67 + 512)
    assert C.PPO_PARTIAL >= 256 * 66 + 512 + 66 and C.PPO_PARTIAL >= 256 * 19                        # what either kernel choice takes
    assert C.PPO_ROWS == [1, 255, 256, 257, 65537] and C.CRITIC_ROWS == [1, 256, 257, 65537] and 65537 > 256 * 256
    assert {a for _, a in C.SAMPLE_SHAPES} == {1, 17, 64} and {r for r, _ in C.SAMPLE_SHAPES} == {1, 256, 257}
    assert (131073, 1, True) in C.KL_CASES and 131073 > C.KL_CAP * 256
    # the GEMM forms: gemm128_kernel needs >= 192 tiles of 128 x 128, K % 4 == 0; the weight gradient takes ceil(rows / 256) slices
    tiles = lambda rows, n: -(-rows // 128) * -(-n // 128)
    assert tiles(3073, 1024) == 200 and 20 % 16 == 4 and 18 % 4 != 0
    assert -(-2049 // 256) == 9 and 2049 - 8 * 256 == 1 and -(-257 // 256) == 2 and -(-129 // 64) * 43 == 129      # 64 column-sum slices of 3 rows: 43 used
    assert sorted({c[1] for c in C.MLP_CASES}) == [129, 257, 2049, 3073] and {c[2] for c in C.MLP_CASES} == {None, "theta", "x"}
    assert {r for _, r in C.JVP_CASES} == {1, 64, 129, 3073} and {len(d) - 1 for d, _ in C.JVP_CASES} == {1, 3, 5}
    assert sorted(C.ADAM_LAYOUTS) == [3, 700, 262221] and C.ADAM_LAYOUTS[3] == (1, 2, 2) and 262221 > 1024 * 256
    assert {c["clip"] for c in C.ADAM_CONFIGS} == {"off", "below", "above3", "just_over"} and {c["t"] for c in C.ADAM_CONFIGS} == {0, 7, 9999}
    assert sum(bool(c.get("fresh")) for c in C.ADAM_CONFIGS) == 2 and {c["opts"] for c in C.ADAM_CONFIGS} == {0, 1}
    assert C.ADAM_LAYOUT_GAP[2] - C.ADAM_LAYOUT_GAP[1] == 17


# ------------------------------------------------------------------------------------------------------- the actor-side problems
@pytest.mark.parametrize("A", C.ACT_DIMS)
def test_actor_problems_keep_the_gates_meaningful(A):
    groups = {}
    for rows in C.actor_rows(A) + [r for a, r in C.LOSS_PAST_CAP if a == A]:
        pop, tag = C.actor_populations(A, rows), (A, rows)
        assert pop["near"] == 0 and pop["same_branch"] and pop["ties"] == 0, (tag, pop)
        if rows >= 1000:
            assert min(v for v in pop.values() if isinstance(v, float)) >= C.MIN_SHARE, (tag, pop)      # six surrogate classes, two KL classes
        o32, o64 = C.clip_oracle(A, rows, None, False, "float32"), C.clip_oracle(A, rows, None, False, "float64")
        s32, s64 = C.surr_oracle(A, rows, -1.0, "float32"), C.surr_oracle(A, rows, -1.0, "float64")
        _finite(o32, o64, s32, s64)
        assert o64["d_mean"].shape == (rows, A) and np.abs(o64["d_mean"]).max() > 0 or rows == 1
        _third(C.gate_actor_vectors(o32, o32, o64, f"clip {tag}"))
        _third(C.gate_actor_vectors(s32, s32, s64, f"surr {tag}"))
        if rows >= 16:
            assert np.abs(o32["d_mean"] - o64["d_mean"]).max() > 0 and np.abs(s32["d_mean"] - s64["d_mean"]).max() > 0, tag
        groups.setdefault("clip loss", []).append((o32["loss"], o32["loss"], o64["loss"], o64["scale"]))
        groups.setdefault("surr sum", []).append((s32["term_sum"], s32["term_sum"], s64["term_sum"], s64["scale"] * rows))
        if rows <= 1025:                                               # (the KL-penalty oracle is the reference's [rows, rows] broadcast)
            k32, k64 = C.klpen_oracle(A, rows, "mid", "float32"), C.klpen_oracle(A, rows, "mid", "float64")
            _finite(k32, k64)
            assert k32["count"] == k64["count"]
            for sfx in ("", "_kl", "_pg"):
                _third(C.gate_actor_vectors(k32, k32, k64, f"klpen{sfx} {tag}", sfx))
            F = k64["count"] / rows                                    # the split form adds up to the whole: g = g_KL + F g_PG
            assert np.abs(k64["d_mean"] - (k64["d_mean_kl"] + F * k64["d_mean_pg"])).max() <= 1e-12 * max(np.abs(k64["d_mean"]).max(), 1e-30)
            assert abs(k64["loss"] + k64["term_sum"] / rows) <= 1e-12 and abs(k64["loss"] - (k64["kl_sum"] - C.PG_COEF * F * k64["ra_sum"]) / rows) <= 1e-12
            groups.setdefault("klpen loss", []).append((k32["loss"], k32["loss"], k64["loss"], k64["scale"]))
        for moved in (False, True):
            l32, l64 = C.linesearch_oracle(A, rows, moved, "float32"), C.linesearch_oracle(A, rows, moved, "float64")
            _finite(l32, l64)
            assert (l64["sums"][2] == 0.0 and l32["sums"][2] == 0.0) != moved
            for k in range(3 if moved else 2):
                groups.setdefault(f"line search {k} moved {moved}", []).append((l32["sums"][k], l32["sums"][k], l64["sums"][k], l64["scales"][k]))
    for name, members in groups.items():
        assert C.gate_group(members, name) > 0, name


def test_actor_bounds_ties_and_single_row_classes():
    for A in (1, 17, 64):
        for cls in C.CLASSES:
            p = C.actor_problem(A, 1, cls)
            region, sign, _, _, near = C.actor_decisions(p)
            pop = C.actor_populations(A, 1, cls)
            assert not bool(near.any()) and pop["same_branch"] and float(sign[0]) == cls[1], (A, cls)
            assert int(region[0]) == {"below": -1, "inside": 0, "above": 1}[cls[0]], (A, cls)
            o32, o64 = C.clip_oracle(A, 1, cls, False, "float32"), C.clip_oracle(A, 1, cls, False, "float64")
            _finite(o32, o64)
            dead = (cls[0] == "above" and cls[1] > 0) or (cls[0] == "below" and cls[1] < 0)
            assert ((o64["d_mean"] == 0).all() and (o32["d_mean"] == 0).all()) == dead, (A, cls)
    # the tie: adv == 0 on every seventh row, a zero gradient there in both arithmetics, the other rows untouched by it
    p = C.actor_problem(17, 1000, None, True)
    ties = (p["adv"] == 0).numpy()
    pop = C.actor_populations(17, 1000, None, True)
    assert ties.sum() == 143 and pop["ties"] == 143 and pop["near"] == 0
    for dt in ("float32", "float64"):
        o = C.clip_oracle(17, 1000, None, True, dt)
        assert (o["d_mean"][ties] == 0).all() and np.isfinite(o["d_mean"]).all() and (np.abs(o["d_mean"][~ties]).max(-1) > 0).mean() > 0.5
    # kl_bound = +inf: every indicator is 1; a bound below every row's KL: none is, F = 0, and the mean's gradient is exactly zero
    for A in C.ACT_DIMS:
        for bound, want in (("inf", 1000.0), ("none", 0.0)):
            p = C.actor_problem(A, 1000, None, False, bound)
            assert C.actor_populations(A, 1000, None, False, bound)["same_branch"]
            k32, k64 = C.klpen_oracle(A, 1000, bound, "float32"), C.klpen_oracle(A, 1000, bound, "float64")
            assert k32["count"] == k64["count"] == want and (np.isinf(p["kl_bound"]) == (bound == "inf"))
            if bound == "none":
                assert (k64["d_mean"] == 0).all() and (k32["d_mean"] == 0).all() and k64["loss"] == 0.0
        # old_std != exp(log_std): the var_ratio - 1 term of d(log_std) is live
        p = C.actor_problem(A, 1000)
        assert float((p["old_std"].double() / torch.exp(p["log_std"].double()) - 1).abs().min()) > 1e-4


def test_exclusive_and_inclusive_clip_bounds_cannot_be_told_apart_here():
    """The clamp's bounds are inclusive (torch.clamp passes the gradient ON a bound, and so does the kernel's ratio >= lo && ratio <=
    hi).  No case can sit on a bound: the ratio is exp of a sum of act_dim terms formed in three arithmetics (float64, torch's
    float32, the kernel's lane order), which agree on no value but exp(0) -- and the float32 logp_old that makes float32's
    difference zero leaves float64's at ~1e-8.  After the redraw every row is at least 1e-4 from both bounds, so the oracle with
    exclusive bounds is the oracle, bit for bit: stated here so that nobody reads the gates as covering it.  The exact-equality
    branch the kernel does reach (s1 == s2 at adv == 0) has its own case."""
    for A, rows, tie in ((1, 1000, False), (17, 1000, True), (64, 1025, False)):
        for dt in ("float32", "float64"):
            a, b = C.clip_oracle(A, rows, None, tie, dt), C.clip_oracle(A, rows, None, tie, dt, "exclusive_clip")
            assert np.array_equal(a["d_mean"], b["d_mean"]) and np.array_equal(a["d_log_std"], b["d_log_std"]) and a["loss"] == b["loss"]


# ------------------------------------------------------------------------------------------------------------ the other kernels
def test_loss_sample_kl_and_fvp_cases():
    for rows in C.CRITIC_ROWS:
        o32, o64 = C.critic_oracle(rows, "float32"), C.critic_oracle(rows, "float64")
        _finite(o32, o64)
        _third(C.gate(o32["d_vr"], o32["d_vr"], o64["d_vr"], f"d_vr {rows}"))
        assert (o64["losses"] > 0).all()
    for A in (16, 17):
        for rows in C.PPO_ROWS:
            pop = C.actor_populations(A, rows)
            assert pop["near"] == 0 and pop["same_branch"], (A, rows)
            assert rows < 1000 or min(v for k, v in pop.items() if "/" in k) >= C.MIN_SHARE
    for rows, A in C.SAMPLE_SHAPES:
        o32, o64 = C.sample_oracle(rows, A, "float32"), C.sample_oracle(rows, A, "float64")
        _finite(o32, o64)
        assert float(C.sample_problem(rows, A)["log_std"].abs().max()) == 1.5
        _third(C.gate(o32["act"], o32["act"], o64["act"], "act"))
        _third(C.gate(o32["logp"], o32["logp"], o64["logp"], "logp", scale=o64["logp_scale"]))
        ls = C.sample_problem(rows, A)["log_std"].double()
        assert np.abs(o64["logp_det"] + float((ls + 0.5 * np.log(2 * np.pi)).sum())).max() <= 1e-12      # logp = -sum(log_std + log sqrt(2 pi))
    members = []
    for rows, A, moved in C.KL_CASES:
        o32, o64 = C.kl_oracle(rows, A, moved, "float32"), C.kl_oracle(rows, A, moved, "float64")
        assert (o64["sum"] == 0.0 and o32["sum"] == 0.0) != moved
        if moved:
            members.append((o32["sum"], o32["sum"], o64["sum"], o64["scale"]))
    assert C.gate_group(members, "KL sums") > 0
    for A, rows, total in ((1, 257, 1000), (17, 257, 1000), (64, 257, 257)):
        o32, o64 = C.fvp_oracle(A, rows, total, "float32"), C.fvp_oracle(A, rows, total, "float64")
        p = C.fvp_problem(A, rows)
        direct = (p["jv"].double() / torch.exp(p["log_std"].double()) ** 2 / (total * A)).numpy()         # (J t) / sigma^2 / (rows_total act_dim)
        assert np.abs(direct - o64["d_mean"]).max() <= 1e-12 * np.abs(direct).max()
        _third(C.gate(o32["d_mean"], o32["d_mean"], o64["d_mean"], "fvp cotangent"))


@pytest.mark.parametrize("case", C.MLP_CASES[:5:2] + [C.MLP_CASES[6], C.MLP_CASES[7]], ids=C.mlp_name)
def test_mlp_cases_keep_the_gates_meaningful(case):
    dims, rows, _ = case
    o32, o64 = C.mlp_oracle(tuple(dims), rows, "float32"), C.mlp_oracle(tuple(dims), rows, "float64")
    assert len(o64["acts"]) == len(dims) - 1 and o64["grad"].shape == (sum(c for _, c in C.mlp_blocks(dims)),) and o64["jvp"].shape == (rows, dims[-1])
    assert np.isfinite(o64["grad"]).all() and np.isfinite(o64["jvp"]).all()
    for a32, a64 in zip(o32["acts"], o64["acts"]):
        _third(C.gate(a32, a32, a64, "activations"))
        assert np.abs(a32 - a64).max() > 0
    _third(C.gate_blocks(o32["grad"], o32["grad"], o64["grad"], C.mlp_blocks(dims), "gradient"))
    _third(C.gate(o32["jvp"], o32["jvp"], o64["jvp"], "jvp", scale=o64["jvp_scale"]))
    assert (o64["jvp_scale"] >= np.abs(o64["jvp"]) * (1 - 1e-12)).all()                                  # the sum of absolute terms bounds the sum
    t = C.mlp_problem(tuple(dims), rows)["tangent"]
    assert all(float(t[o:o + c].abs().min()) > 0 for o, c in C.mlp_blocks(dims)[1::2])                  # bias tangents are non-zero


@pytest.mark.parametrize("n", [3, 700])
def test_adam_cases_keep_the_gates_meaningful(n):
    scalars = {}
    for cfg in C.ADAM_CONFIGS:
        name = C.adam_name(cfg)
        p, o32, o64 = C.adam_problem(n, name), C.adam_oracle(n, name, "float32"), C.adam_oracle(n, name, "float64")
        _finite(o32, o64)
        over = o64["scalars4"][3] / p["max_norm"]
        assert {"off": over < 1e-3, "below": abs(over - 1 / 3) < 1e-6, "above3": abs(over - 3) < 1e-5, "just_over": 1 < over < 1.001}[cfg["clip"]], (name, over)
        assert abs(o64["scalars4"][3] / p["norm64"] - 1) < 1e-12 and (o64["scalars4"][1] > 0) == bool(cfg["opts"])
        assert ((p["m"] != 0).all() and (p["v"] > 0).all()) != bool(cfg.get("fresh")) and np.abs(o64["update"]).max() > 1e-6
        assert C.adam_update_floor(n, name) < 1e-3 * C.ADAM_LR_ACTOR                                    # the floor hides no step of size lr
        C.gate_adam(o32, o32, o64, n, name, f"{name} n {n}", None, scalars)
    for nm, members in scalars.items():
        C.gate_group(members, nm)
    _third(max(r for k, (r, _) in C.RATIOS.items()))
    # the sub-ranges: nothing outside the Adam range moves, the stale gradient is rescaled only when asked, CUP's norm is the actor's
    name = "above3/t0/opts1"
    if n == 700:
        p = C.adam_problem(n, name)
        for rng, layout in (("critic_fit", None), ("cup", None), ("cup", C.ADAM_LAYOUT_GAP)):
            o = C.adam_oracle(n, name, "float64", None, rng, layout, (7, 3))
            lo, hi, norm0, rest = o["range"]
            out = np.r_[0:lo, hi:n]
            assert (o["update"][out] == 0).all() and (o["update"][lo:hi] != 0).all() and np.array_equal(o["m"][out], p["m"].double().numpy()[out])
            assert o["scalars4"][0] < 1 and (np.allclose(o["grad"][out], p["grad"].double().numpy()[out] * o["scalars4"][0], rtol=1e-12) == bool(rest))
            assert (norm0 == 0) == (o["scalars4"][1] > 0)


# -------------------------------------------------------------------------------------------- the gates refuse wrong oracles
def test_gates_refuse_deliberately_wrong_oracles():
    """Each a one-line variant of the oracle, in float32, in the HIP result's place."""
    for A in (1, 17, 64):
        for rows in (C.rpb(A) + 1, 1000):
            k32, k64 = C.klpen_oracle(A, rows, "mid", "float32"), C.klpen_oracle(A, rows, "mid", "float64")
            # KL(old || new) in place of KL(new || old): the gradient of the KL term, and which rows the indicator keeps
            w = C.klpen_oracle(A, rows, "mid", "float32", "kl_swapped")
            _refused(lambda: C.gate_actor_vectors(w, k32, k64, "kl_swapped", "_kl"))
            # F taken as 1 in the policy-gradient term
            w = C.klpen_oracle(A, rows, "mid", "float32", "F_is_one")
            _refused(lambda: C.gate_actor_vectors(w, k32, k64, "F_is_one"))
            _refused(lambda: C.gate_group([(w["loss"], k32["loss"], k64["loss"], k64["scale"])], "F_is_one loss"))
            # d(log_std) without its - 1, in all three modes
            w = C.klpen_oracle(A, rows, "mid", "float32", "minus_one_dropped")
            _refused(lambda: C.gate(w["d_log_std"], k32["d_log_std"], k64["d_log_std"], "minus_one_dropped", scale=k64["d_log_std_scale"]))
            o32, o64 = C.clip_oracle(A, rows, None, False, "float32"), C.clip_oracle(A, rows, None, False, "float64")
            w = C.clip_oracle(A, rows, None, False, "float32", "minus_one_dropped")
            _refused(lambda: C.gate(w["d_log_std"], o32["d_log_std"], o64["d_log_std"], "minus_one_dropped", scale=o64["d_log_std_scale"]))
            assert C.gate(w["d_mean"], o32["d_mean"], o64["d_mean"], "minus_one_dropped leaves d_mean alone") <= 1.0
            if rows == 1000:                                           # the pessimistic min replaced by the clipped term (a handful of rows may all agree)
                w = C.clip_oracle(A, rows, None, False, "float32", "clip_ignores_sign")
                _refused(lambda: C.gate_actor_vectors(w, o32, o64, "clip_ignores_sign"))
            s32, s64 = C.surr_oracle(A, rows, 1.0, "float32"), C.surr_oracle(A, rows, 1.0, "float64")
            w = C.surr_oracle(A, rows, 1.0, "float32", "minus_one_dropped")
            _refused(lambda: C.gate(w["d_log_std"], s32["d_log_std"], s64["d_log_std"], "minus_one_dropped", scale=s64["d_log_std_scale"]))
            # the sign of p0 forgotten
            w = C.surr_oracle(A, rows, -1.0, "float32")
            _refused(lambda: C.gate_actor_vectors(w, s32, s64, "sign"))
            l32, l64 = C.linesearch_oracle(A, rows, True, "float32"), C.linesearch_oracle(A, rows, True, "float64")
            w = C.linesearch_oracle(A, rows, True, "float32", "kl_swapped")
            _refused(lambda: C.gate_group([(w["sums"][2], l32["sums"][2], l64["sums"][2], l64["scales"][2])], "kl_swapped"))
    w, o32, o64 = (C.kl_oracle(1000, 17, True, "float32", "kl_swapped"), C.kl_oracle(1000, 17, True, "float32"), C.kl_oracle(1000, 17, True, "float64"))
    _refused(lambda: C.gate_group([(w["sum"], o32["sum"], o64["sum"], o64["scale"])], "kl_swapped"))
    # the Fisher cotangent divided by rows instead of rows_total * act_dim
    for A, rows, total in ((17, 257, 1000), (64, 257, 257), (1, 257, 1000)):
        o32, o64 = C.fvp_oracle(A, rows, total, "float32"), C.fvp_oracle(A, rows, total, "float64")
        w = C.fvp_oracle(A, rows, total, "float32", "rows_only")
        _refused(lambda: C.gate(w["d_mean"], o32["d_mean"], o64["d_mean"], "rows_only"))
    # the bias tangent dropped from the JVP
    for dims, rows in C.JVP_CASES[:6]:
        o32, o64 = C.mlp_oracle(tuple(dims), rows, "float32"), C.mlp_oracle(tuple(dims), rows, "float64")
        w = C.mlp_oracle(tuple(dims), rows, "float32", "bias_tangent_dropped")
        _refused(lambda: C.gate(w["jvp"], o32["jvp"], o64["jvp"], "bias_tangent_dropped", scale=o64["jvp_scale"]))

    def adam_variant(n, name, variant, **kw):
        a = (kw.get("rng", "all"), kw.get("layout"), kw.get("steps"))
        o32, o64 = C.adam_oracle(n, name, "float32", None, *a), C.adam_oracle(n, name, "float64", None, *a)
        w = C.adam_oracle(n, name, "float32", variant, *a)
        _refused(lambda: C.gate_adam(w, o32, o64, n, name, f"{variant} {name} n {n}", kw.get("layout")))
    for n in (3, 700):
        # the L2 gradient with factor 1; the value coefficient applied before the L2 term
        for name in ("off/t0/opts1", "above3/t0/opts1", "below/t9999/opts1"):
            adam_variant(n, name, "l2_factor_one")
            adam_variant(n, name, "value_coefficient_before_l2")
        # the clip coefficient without its 1e-6, at a norm just over the bound
        adam_variant(n, "just_over/t0/opts0", "clip_without_1e_6")
        # bias correction with t instead of t + 1 (clocks 7 / 3: by step 10 000 the corrections are 1 to 2e-5)
        for rng in ("all", "critic_fit", "cup"):
            adam_variant(n, "above3/t0/opts1", "bias_correction_t", rng=rng, steps=(7, 3))


# ------------------------------------------------------------------------------------- adam1 restated; the host header's program
def test_adam1_restated_the_old_weights_are_refused_and_the_host_formed_ones_pass():
    """csrc/adam.h's adam1 in float32 numpy (IEEE sqrt and division: the kernel's v_rcp / v_sqrt only add to the error) in the HIP
    result's place.  With the weights 1.f - beta formed from the float32 betas (1.f - 0.999f = 0.99998713e-3 against torch's
    float(1 - 0.999) = 1.00000005e-3) the adam_v gate refuses it wherever this step's (1 - beta2) g^2 is a visible share of v:
    measured ratio 10.5 to 12.3 with zero moments (v is that term alone) and 4.2 to 12.3 with moments aged over seven steps; the
    adam_m gate passes either way.  With (float)(1.0 - beta) (csrc/adam_host.h) every gate passes."""
    seen = {}
    for n in (3, 700):
        for cfg in C.ADAM_CONFIGS:
            name = C.adam_name(cfg)
            o32, o64 = C.adam_oracle(n, name, "float32"), C.adam_oracle(n, name, "float64")
            new = C.adam_oracle(n, name, "float32", "numpy_adam1_new")
            C.gate_adam(new, o32, o64, n, name, f"adam1 restated, host-formed weights {name} n {n}")
            old = C.adam_oracle(n, name, "float32", "numpy_adam1_old")
            C.gate(old["m"], o32["m"], o64["m"], f"adam_m old weights {name} n {n}")
            if cfg.get("fresh") or cfg.get("aged"):
                C.RATIOS.clear()
                _refused(lambda: C.gate(old["v"], o32["v"], o64["v"], f"adam_v old weights {name} n {n}"))
                seen[(n, name)] = max(r for r, _ in C.RATIOS.values())
    print("adam_v gate ratio with the old weights:", {k: round(v, 2) for k, v in seen.items()})
    assert len(seen) == 6 and min(seen.values()) > 4.0 and all(9.8 <= v <= 12.5 for (n, name), v in seen.items() if "fresh" in name)


ADAM_HOST_PROPERTIES = [
    "named betas give back their decimal",
    "named betas give (float)(1.0 - beta)",
    "the weight of 0.999 differs from 1.f - 0.999f",
    "sampled floats round-trip bit for bit",
    "remembered weights equal fresh ones",
    "betas outside [0, 1) are refused",
]


@pytest.fixture(scope="module")
def adam_host_output(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("adam_host") / "adam_host_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "adam_host_check.cpp"),
                            "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    return run.returncode, run.stdout.splitlines()


def test_adam_host_header_program_ends_clean(adam_host_output):
    rc, lines = adam_host_output
    assert rc == 0 and lines[-1] == "done 0", lines
    assert not [l for l in lines if l.startswith("FAIL")]
    # the header stays host-only: no HIP include, so the host compiler alone builds it
    src = open(os.path.join(CSRC, "adam_host.h")).read()
    assert "hip" not in src.split("#pragma once")[1].lower().replace("no hip", "")


@pytest.mark.parametrize("prop", ADAM_HOST_PROPERTIES)
def test_adam_host_header_property(adam_host_output, prop):
    _, lines = adam_host_output
    assert f"ok {prop}" in lines, [l for l in lines if prop in l]
