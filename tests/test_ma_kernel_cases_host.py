"""CPU companion (no GPU) of tests/test_gpu_ma_kernels.py: the float32 and float64 oracles of every case of
tests/ma_kernel_cases.py except the two row counts past the 1024 x 256 cap, and the conditions under which that file's gates say
something -- every value finite, every branch class populated, no row within 1e-4 of a discontinuity (none left out or altered
after generation), float32 and float64 in the same branch in every row, yardsticks that are not zero -- and the gates themselves:
fed the float32 oracle in the HIP result's place they pass with ratio <= 1/3, fed a deliberately wrong oracle (a one-line
variant each) they refuse, at 257 rows and at the matching one-row case."""
import numpy as np
import pytest
import torch

import ma_kernel_cases as C


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
            assert np.isfinite(v).all(), k


def _third(ratio):
    assert ratio <= 1.0 / 3.0 + 1e-12, ratio


def test_case_tables():
    # the launch arithmetic the row counts stand for: 256-thread workgroups, grid-stride, at most 1024 of them
    blocks = lambda rows: min((rows + C.WG - 1) // C.WG, C.WG_CAP)
    passes = lambda rows, wg: len(range(wg * C.WG, rows, blocks(rows) * C.WG))          # trips of workgroup wg's thread 0 through the loop
    assert [blocks(r) for r in C.ROWS] == [1, 1, 1, 1, 1, 2, 4] and [r % C.WG for r in C.ROWS] == [1, 63, 65, 255, 0, 1, 232]
    assert max(C.ROWS) < C.CAP_ROWS == 262144 and all(passes(r, 0) == 1 for r in C.ROWS)
    one, full = C.ROWS_PAST_CAP
    assert (one, full) == (262145, 262401) and blocks(one) == blocks(full) == C.WG_CAP
    assert passes(one, 0) == 2 and passes(one, 1) == 1 and one - C.CAP_ROWS == 1                     # one row of workgroup 0's second pass
    assert passes(full, 0) == 2 and passes(full, 1) == 2 and passes(full, 2) == 1 and full - C.CAP_ROWS == C.WG + 1
    assert C.ACT_DIMS[0] == 1 and C.ACT_DIMS[-1] == C.MAX_ACT == 16 and C.ACTOR_PARTIAL_DOUBLES == 1024 * 20
    assert set(C.PAST_CAP_ACT_DIM) == set(C.ACTOR_FORMS) and {1, 16} <= set(C.PAST_CAP_ACT_DIM.values()) <= set(C.ACT_DIMS)
    assert {f for f, _ in C.ACTOR_FORMS} == set(C.FORMS) and all(("macpo" == f) or (f, 1) in C.ACTOR_FORMS for f, _ in C.ACTOR_FORMS)
    assert C.FORMS["macpo"]["clip"] == float(np.float32(3e38)) and C.FORMS["macpo"]["ent"] == 0 and C.FORMS["mappo"]["per_dim"] == 1
    assert blocks(C.SHARD_ROWS) == 2 and C.SHARD_ROWS in C.ROWS
    assert C.ADAM_N[-1] == full and {c["clip"] for c in C.ADAM_CONFIGS} == {"off", "below", "above3", "just_over"}
    assert sum(bool(c.get("fresh")) for c in C.ADAM_CONFIGS) == 1 and {(c["wd"] > 0, c["step"]) for c in C.ADAM_CONFIGS} == {(False, 0), (False, 9999), (True, 0), (True, 9999)}
    assert sorted(r * a for r, a in C.SAMPLE_SHAPES[:3]) == [255, 256, 257] and {a for _, a in C.SAMPLE_SHAPES[3:]} == {1, 5, 16}
    assert len(C.POPART_ALL) == 12 and set(C.POPART_FEW) <= set(C.POPART_ALL) and {c[0] for c in C.POPART_FEW} == {0, 1}
    assert C.GAE_T == [1, 7, 9] and C.GAE_N == [1, 255, 257]


# ------------------------------------------------------------------------------------------------------- spo_ma_actor_loss
@pytest.mark.parametrize("rows", C.ROWS[1:] + [2 * C.SHARD_ROWS, 2])
def test_actor_cases_keep_the_gates_meaningful(rows):
    groups = {}
    for form, masks in C.ACTOR_FORMS:
        for A in (C.ACT_DIMS if rows in C.ROWS else [5]):
            o32, o64 = C.actor_oracle(form, masks, A, rows, None, "float32"), C.actor_oracle(form, masks, A, rows, None, "float64")
            pop, tag = C.actor_populations(form, masks, A, rows), (form, masks, A, rows)
            _finite(o32, o64)
            assert pop["near"] == 0 and pop["same_branch"], (tag, pop)
            assert o64["dmean"].shape == (rows, A) and o64["scalars"][4] == float(C.actor_problem(form, masks, A, rows)["active"].sum())
            if rows >= 63:
                classes = ("adv_pos", "adv_neg") if form == "macpo" else ("below", "inside", "above", "adv_pos", "adv_neg")
                assert min(pop[k] for k in classes) >= C.MIN_SHARE, (tag, pop)
                assert 0.05 <= 1 - o64["scalars"][4] / rows <= 0.35, tag        # ~20 % inactive: Binomial(63, 0.2) +- 3 sd of 0.05
                assert np.abs(o32["dmean"] - o64["dmean"]).max() > 0 and np.abs(o64["dmean"]).max() > 0, tag
            C.gate_actor(f"{form}/masks{masks}", A, rows, o32, o32, o64, groups, entry="host")
    for name, members in groups.items():
        yard = C.gate_group("host", members, name)
        assert yard > 0 or name in ("sum(active)", "mean(imp * cost_adv)"), name
    assert any(m[6] > 0 for m in groups["mean(imp * cost_adv)"])
    _third(max(r for (e, *_), (r, _) in C.RATIOS.items() if e == "host"))


@pytest.mark.parametrize("form,masks", C.ACTOR_FORMS)
def test_actor_single_row_cases_sit_in_their_branch(form, masks):
    want = {"below": -1, "inside": 0, "above": 1}
    for A in C.ACT_DIMS:
        for cls in C.ACTOR_CLASSES:
            p = C.actor_problem(form, masks, A, 1, cls)
            region, sign, near = C.actor_decisions(p, form)
            pop = C.actor_populations(form, masks, A, 1, cls)
            assert not bool(near.any()) and pop["same_branch"] and float(sign[0]) == cls[1], (form, A, cls)
            assert form == "macpo" or bool((region == want[cls[0]]).all()), (form, A, cls)
            o32, o64 = C.actor_oracle(form, masks, A, 1, cls, "float32"), C.actor_oracle(form, masks, A, 1, cls, "float64")
            _finite(o32, o64)
            # a ratio outside the clip range on the side the advantage pushes to: the surrogate's gradient is exactly zero
            dead = form != "macpo" and ((cls[0] == "above" and cls[1] > 0) or (cls[0] == "below" and cls[1] < 0))
            if dead:
                assert (o64["dmean"] == 0).all() and (o32["dmean"] == 0).all(), (form, A, cls)
            else:
                assert np.abs(o64["dmean"]).max() > 0, (form, A, cls)
            C.gate_actor(f"{form}/masks{masks}", A, 1, o32, o32, o64, entry="host")


# ------------------------------------------------------------------------------------------------------- spo_ma_value_loss
@pytest.mark.parametrize("rows", C.ROWS[1:] + [2 * C.SHARD_ROWS, 2])
def test_value_cases_keep_the_gates_meaningful(rows):
    losses = []
    for active in C.VALUE_FORMS:
        for cls in ((None, "on_bound") if rows == C.SHARD_ROWS else (None,)):
            o32, o64 = C.value_oracle(active, rows, cls, "float32"), C.value_oracle(active, rows, cls, "float64")
            pop = C.value_populations(active, rows, cls)
            _finite(o32, o64)
            assert pop["near"] == 0 and pop["same_branch"], (active, rows, cls, pop)
            if rows >= 63:
                assert min(v for v in pop.values() if isinstance(v, float)) >= C.MIN_SHARE, (active, rows, cls, pop)
                assert pop["neg_orig"] >= C.MIN_SHARE and pop["neg_clip"] >= C.MIN_SHARE                    # the reference's empty e < -delta branch
                assert np.abs(o32["dvalues"] - o64["dvalues"]).max() > 0 and o64["loss"] > 0
            if cls == "on_bound":
                p = C.value_problem(active, rows, cls)
                on = (p["values"] - p["value_preds"]).abs() == C.CLIP
                assert int(on.sum()) == (rows + 3) // 4 and bool((p["value_preds"][on] == 0).all())
            C.gate_value(f"active{active}/{cls}", rows, o32, o32, o64, losses, entry="host")
    assert C.gate_group("host", losses, "value loss") > 0 or rows == 2
    _third(max(r for (e, *_), (r, _) in C.RATIOS.items() if e == "host"))


@pytest.mark.parametrize("active", C.VALUE_FORMS)
def test_value_single_row_cases_sit_in_their_branch(active):
    for cls in C.VALUE_CLASSES + ["on_bound"]:
        p = C.value_problem(active, 1, cls)
        i, bo, bc, pk, near = C.value_decisions(p)
        assert not bool(near.any()) and C.value_populations(active, 1, cls)["same_branch"], cls
        if cls in C._VALUE_CLASS:
            assert bool(C._VALUE_CLASS[cls](i, bo, bc, pk).all()), cls
        else:
            assert float(p["values"][0]) == C.CLIP and float(p["value_preds"][0]) == 0.0 and int(pk[0]) == 1
        o32, o64 = C.value_oracle(active, 1, cls, "float32"), C.value_oracle(active, 1, cls, "float64")
        _finite(o32, o64)
        if cls == "neg":
            assert o64["loss"] == 0.0 and o64["dvalues"][0] == 0.0 and o32["loss"] == 0.0
        if cls in ("clipped", "neg"):
            assert o64["dvalues"][0] == 0.0
        if cls in ("quad", "unclipped", "max_orig", "max_clip", "on_bound"):
            assert o64["dvalues"][0] != 0.0, cls
        C.gate_value(f"active{active}/{cls}", 1, o32, o32, o64, entry="host")


# ----------------------------------------------------------------------------------------------------------- the other kernels
@pytest.mark.parametrize("rows", C.ROWS + [2 * C.SHARD_ROWS])
def test_popart_cases_keep_the_gates_meaningful(rows):
    for cfg in (C.POPART_ALL if rows == C.SHARD_ROWS else C.POPART_FEW[:2] if rows == 2 * C.SHARD_ROWS else C.POPART_FEW):
        o32, o64 = C.popart_oracle(cfg, rows, "float32"), C.popart_oracle(cfg, rows, "float64")
        _finite(o32, o64)
        train, state, inp, beta = cfg
        # the variance before its clamp is far from 1e-2 on either side, in both arithmetics
        for o in (o32, o64):
            assert (o["var_raw"] < 5e-3) == (inp == "narrow" or state == "fresh" and (rows == 1 or not train)) and abs(o["var_raw"] - 1e-2) > 5e-3, (cfg, rows, o["var_raw"])
        if state == "fresh":
            assert o64["state3"][2] == (0.0 if not train else pytest.approx(1 - beta, rel=1e-9))   # <= epsilon: the debiasing clamp is in force
            # one update at beta 0.99999 leaves 1 - beta = the float32 epsilon to 3e-8: the clamp sits at the value it guards
            assert abs(o64["state3"][2] - C.POPART_EPS) <= 1e-7 * C.POPART_EPS or beta == 0.9 or not train
        if train:
            _third(C.gate("host", C.popart_name(cfg), None, rows, o32["state3"], o32["state3"], o64["state3"], "state", scale=o64["state_scales"]))
        _third(C.gate("host", C.popart_name(cfg), None, rows, o32["out"], o32["out"], o64["out"], "normalised rows"))


@pytest.mark.parametrize("n", C.ADAM_N[:-1])
def test_adam_cases_keep_the_gates_meaningful(n):
    norms = []
    for cfg in C.ADAM_CONFIGS:
        name = C.adam_name(cfg)
        p, o32, o64 = C.adam_problem(n, name), C.adam_oracle(n, name, "float32"), C.adam_oracle(n, name, "float64")
        _finite(o32, o64)
        over = o64["norm"] / p["max_norm"]
        assert {"off": True, "below": abs(over - 1 / 3) < 1e-6, "above3": abs(over - 3) < 1e-5, "just_over": 1 < over < 1.001}[cfg["clip"]], (name, over)
        assert ((p["m"] != 0).all() and (p["v"] > 0).all()) != bool(cfg.get("fresh")) and np.abs(o64["update"]).max() > 1e-6
        assert C.adam_update_floor(n, name) < 1e-3 * C.ADAM_LR                                     # the floor hides no step of size lr
        C.gate_adam(name, n, o32, o32, o64, norms, entry="host")
    assert C.gate_group("host", norms, "norm") >= 0
    _third(max(r for (e, *_), (r, _) in C.RATIOS.items() if e == "host"))


def test_lamda_sample_and_gae_cases():
    sides = set()
    for case in C.LAMDA_CASES:
        (w32, _, _), (w64, scale, pre) = C.lamda_oracle(case, "float32"), C.lamda_oracle(case, "float64")
        assert np.isfinite([w32, w64, scale]).all() and abs(pre) > 1e-3 and (w64 == 0) == (pre < 0) == (w32 == 0)
        sides.add(pre < 0)
    assert sides == {True, False}
    for rows, A in C.SAMPLE_SHAPES:
        for coefs in C.SAMPLE_COEFS:
            o32, o64 = C.sample_oracle(rows, A, coefs, "float32"), C.sample_oracle(rows, A, coefs, "float64")
            _finite(o32, o64)
            ls = C.sample_problem(rows, A, coefs)["log_std"]
            assert float(ls.abs().max()) == 4.0 and ls.numel() == A
            for key in o64:
                assert o64[key].shape == (rows, A)
                _third(C.gate("host", key, A, rows, o32[key], o32[key], o64[key], f"{key} {rows} x {A}"))
    for T in C.GAE_T:
        for N in C.GAE_N:
            p = C.gae_problem(T, N)
            assert p["want_r"].shape == (T + 1, N, 1) and bool(torch.isfinite(p["want_r"][:T]).all()) and bool(torch.isfinite(p["want_c"][:T]).all())
            assert 0 < float(p["masks"].mean()) < 1 or N == 1
            assert (p["sd_r"], p["mu_r"]) != (p["sd_c"], p["mu_c"]) and p["sd_r"] != 1.0 and p["mu_r"] != 0.0


# -------------------------------------------------------------------------------------------- the gates refuse wrong oracles
def _refused(fn):
    with pytest.raises(AssertionError):
        fn()


def _actor_variant(form, masks, A, rows, cls, variant):
    o32, o64 = C.actor_oracle(form, masks, A, rows, cls, "float32"), C.actor_oracle(form, masks, A, rows, cls, "float64")
    wrong = C.actor_oracle(form, masks, A, rows, cls, "float32", variant)
    _refused(lambda: C.gate_actor(f"{form}/{variant}", A, rows, wrong, o32, o64, entry="host"))


def _value_variant(active, rows, cls, variant):
    o32, o64 = C.value_oracle(active, rows, cls, "float32"), C.value_oracle(active, rows, cls, "float64")
    wrong = C.value_oracle(active, rows, cls, "float32", variant)
    _refused(lambda: C.gate_value(f"active{active}/{variant}", rows, wrong, o32, o64, entry="host"))


def _adam_variant(n, name, variant):
    o32, o64 = C.adam_oracle(n, name, "float32"), C.adam_oracle(n, name, "float64")
    _refused(lambda: C.gate_adam(name, n, C.adam_oracle(n, name, "float32", variant), o32, o64, entry="host"))


def test_gates_refuse_deliberately_wrong_oracles():
    """Each a one-line variant of the oracle, in float32, in the HIP result's place: at 257 rows and at one row in the branch
    the variant touches (a two-shard batch of 2 x 257 and 2 x 1 rows for the rows_global variant)."""
    R = C.SHARD_ROWS
    # a symmetric Huber -- the e < -delta branch "repaired"
    for active in C.VALUE_FORMS:
        for rows in (63, R, 1000):
            _value_variant(active, rows, None, "symmetric_huber")
        _value_variant(active, 1, "neg", "symmetric_huber")
        # clip bounds exclusive instead of inclusive: seen on the rows that sit on the bound
        _value_variant(active, R, "on_bound", "exclusive_clip")
        _value_variant(active, 1, "on_bound", "exclusive_clip")
        # rows in place of rows_global in a mean
        _value_variant(active, 2 * R, None, "rows_for_rows_global")
        _value_variant(active, 2, None, "rows_for_rows_global")
        # the last row of the input left stale
        _value_variant(active, R, None, "stale_last_row")
        _value_variant(active, 1, "quad", "stale_last_row")
    for form, masks in C.ACTOR_FORMS:
        _actor_variant(form, masks, 5, 2 * R, None, "rows_for_rows_global")
        _actor_variant(form, masks, 5, 2, None, "rows_for_rows_global")
        for A in (1, 16):
            _actor_variant(form, masks, A, R, None, "stale_last_row")
            _actor_variant(form, masks, A, 1, ("inside", 1.0), "stale_last_row")
    # entropy weight ignoring the active mask
    for form in ("mappolag", "happo", "mappo"):
        _actor_variant(form, 1, 5, R, None, "entropy_ignores_mask")
        _actor_variant(form, 1, 5, 1, ("inside", -1.0), "entropy_ignores_mask")
    # factor applied in the per-dimension form
    for masks in (0, 1):
        for A in (1, 16):
            _actor_variant("mappo", masks, A, R, None, "factor_in_per_dim")
            _actor_variant("mappo", masks, A, 1, ("inside", 1.0), "factor_in_per_dim")
    for n in (R, 1):
        # Adam without its bias correction, at step 1 (by step 10 000 the corrections are 1 to 2e-5)
        for cfg in (c for c in C.ADAM_CONFIGS[:12] if c["step"] == 0):
            _adam_variant(n, C.adam_name(cfg), "no_bias_correction")
        # clip coefficient without the 1e-6, at a norm just over the bound
        _adam_variant(n, "just_over/wd0e+00/t0", "clip_without_1e_6")
        _adam_variant(n, C.adam_name(C.ADAM_CONFIGS[5]), "stale_last_row")
    # 1 - beta2 taken in float32 (1.3e-5 off torch's): the kernel's own former arithmetic, which the one-element cases exposed; from
    # zero moments v = (1 - beta2) g^2 shows it at every size
    _adam_variant(1, "below/wd1e-02/t0", "one_minus_beta_in_float32")
    for n in C.ADAM_N[:-1]:
        _adam_variant(n, "off/wd0e+00/t0/fresh", "one_minus_beta_in_float32")
    for rows, A in ((R, 1), (1, 16)):
        for coefs in C.SAMPLE_COEFS:
            o32, o64 = C.sample_oracle(rows, A, coefs, "float32"), C.sample_oracle(rows, A, coefs, "float64")
            wrong = C.sample_oracle(rows, A, coefs, "float32", "stale_last_row")
            for key in ("act", "logp", "logp_given"):
                _refused(lambda: C.gate("host", key, A, rows, wrong[key], o32[key], o64[key], key))
    for rows in (R, 1):
        cfg = C.POPART_FEW[1]
        o32, o64 = C.popart_oracle(cfg, rows, "float32"), C.popart_oracle(cfg, rows, "float64")
        wrong = C.popart_oracle(cfg, rows, "float32", "stale_last_row")
        _refused(lambda: C.gate("host", "popart", None, rows, wrong["out"], o32["out"], o64["out"], "normalised rows"))
        _refused(lambda: C.gate("host", "popart", None, rows, wrong["state3"], o32["state3"], o64["state3"], "state", scale=o64["state_scales"]))
