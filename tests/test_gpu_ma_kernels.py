"""GPU tests of the multi-agent trainer kernels by direct ABI calls, branch by branch, under the float64 yardstick:
spo_ma_actor_loss, spo_ma_value_loss, spo_ma_popart_stats / spo_ma_popart_forward, spo_ma_clip_adam, spo_ma_lamda_update,
spo_ma_sample / spo_ma_log_probs (csrc/ma_net.hip) and spo_ma_gae (csrc/multi_agent.hip).

The reference is the same operation in plain torch float64 on the CPU (oracle/ma_restatement.py, autograd, clip_grad_norm_,
torch.optim.Adam), the yardstick the same oracle in float32, and a HIP result passes when |hip - f64| <= 3 |f32 - f64| + floor in
max-norm and L2 (tests/ma_yardstick.gate), floor = 1e-6 of the quantity's scale.  Shapes: act_dim 1 .. 16 (= SPO_MAX_ACT), row
counts with a ragged last workgroup, more than one workgroup, and 262 145 / 262 401 rows -- a second grid-stride pass under the
1024-workgroup cap; every branch of the clipped surrogate and of the clipped Huber loss holds at least 10 % of the rows, no row
lies within 1e-4 of a discontinuity, and one-row cases come once per branch.  A data-parallel share is called once per shard
with rows_global / denom_host of the whole batch and the shards' outputs are summed.  Every output and every partial_ws has
exactly the documented size and is followed by a guard of NaNs that must be untouched.  The cases, their oracles and the gates
are in tests/ma_kernel_cases.py (tests/test_ma_kernel_cases_host.py shows on the CPU that the gates refuse wrong oracles); after
the last test the worst ratio |hip - f64| / (3 |f32 - f64| + floor) per (entry point, form, act_dim, rows) is printed
(profiles/ma_trainer_kernels/gate_ratios.txt)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ma_kernel_cases as C  # noqa: E402

GUARD = 64
NAN = float("nan")


@pytest.fixture(autouse=True)
def _leave_no_global_state():
    threads, rng = torch.get_num_threads(), torch.get_rng_state()
    yield
    torch.set_num_threads(threads)
    torch.set_rng_state(rng)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    C.RATIOS.clear()
    yield torch.device("cuda:0")
    print("\n==== worst gate ratios (<= 1 passes) ====\n" + C.ratio_table() + "\n==== end of gate ratios ====")


class Guarded:
    """Device buffers of exactly n elements followed by GUARD NaNs.  out(): a result the call must fill; ws(): a workspace."""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def _new(self, n, dtype, full, init=None):
        buf = torch.full((n + GUARD,), NAN, dtype=dtype, device=self.dev)
        if init is not None:
            buf[:n] = init.to(self.dev)
        self.items.append((buf, n, full))
        return buf

    def out(self, n, dtype=torch.float32):
        return self._new(n, dtype, True)

    def ws(self, n):
        return self._new(n, torch.float64, False)

    def inout(self, init):
        return self._new(init.numel(), init.dtype, True, init.reshape(-1))

    def check(self, what):
        torch.cuda.synchronize()
        for buf, n, full in self.items:
            assert bool(torch.isnan(buf[n:]).all()), f"{what}: written past the end of a buffer of {n}"
            assert not full or bool(torch.isfinite(buf[:n]).all()), f"{what}: an output of {n} is not filled"

    def untouched(self, what):
        torch.cuda.synchronize()
        for buf, n, full in self.items:
            assert bool(torch.isnan(buf).all()), f"{what}: a refused call wrote to a buffer"


def _lib():
    from safepo import _abi
    return _abi.load(), _abi.ptr, _abi.stream_ptr()


def _host(buf, n):
    return buf[:n].double().cpu().numpy()


# ------------------------------------------------------------------------------------------------------- spo_ma_actor_loss
def _hip_actor(dev, form, masks, A, rows, cls=None, shards=1):
    """spo_ma_actor_loss over case (form, masks, A, rows, cls) in `shards` equal shares -> dmean [rows, A], dlogstd [A], scalars [5]
    (float64 numpy; sums over the shares, the entropy -- no sum over rows -- asserted equal on every share)."""
    from safepo import _abi
    lib, ptr, st = _lib()
    p, f = C.actor_problem(form, masks, A, rows, cls), C.FORMS[form]
    denom = float(p["active"].sum()) if masks else float(rows)
    cfg = _abi.MaLossCfg(f["clip"], f["ent"], C.STD_COEFS[0], C.STD_COEFS[1], masks, f["per_dim"])
    per = rows // shards
    assert per * shards == rows
    dmean, dls, scal, ents = [], np.zeros(A), np.zeros(5), []
    log_std, lamda = p["log_std"].to(dev), torch.tensor([f["lamda"]], dtype=torch.float32, device=dev)
    for k in range(shards):
        put = lambda key: p[key][k * per:(k + 1) * per].contiguous().to(dev)
        t = {key: put(key) for key in ("mean", "act", "old_logp", "adv", "cost_adv", "factor", "active")}
        G = Guarded(dev)
        dm, dl, sc, ws = G.out(per * A), G.out(A), G.out(5), G.ws(C.ACTOR_PARTIAL_DOUBLES)
        _abi.check(lib.spo_ma_actor_loss(ptr(t["mean"]), ptr(log_std), ptr(t["act"]), ptr(t["old_logp"]), ptr(t["adv"]), ptr(t["cost_adv"]),
                                         ptr(t["factor"]), ptr(t["active"]), ptr(lamda), cfg, per, A, denom, rows, ptr(dm), ptr(dl), ptr(sc),
                                         ptr(ws), st), "spo_ma_actor_loss")
        G.check(f"spo_ma_actor_loss {form} masks {masks} A {A} rows {per}")
        blocks = min((per + C.WG - 1) // C.WG, C.WG_CAP)
        parts = ws[:C.ACTOR_PARTIAL_DOUBLES].view(C.WG_CAP, C.AL_NS + C.MAX_ACT)
        assert bool(torch.isfinite(parts[:blocks, :C.AL_NS + A]).all()) and bool(torch.isnan(parts[blocks:]).all())
        assert bool(torch.isnan(parts[:, C.AL_NS + A:]).all())           # one row of partials per launched workgroup, act_dim wide
        dmean.append(_host(dm, per * A).reshape(per, A))
        dls += _host(dl, A)
        s = _host(sc, 5)
        ents.append(s[1])
        scal += s
    assert all(e == ents[0] for e in ents)
    scal[1] = ents[0]
    return np.concatenate(dmean), dls, scal


def _gate_actor_case(groups, dev, form, masks, A, rows, cls=None, shards=1):
    """dmean and dlogstd of one case through the gates; its five scalars are appended to `groups` (gated per kind by the caller).
    One-row cases (cls): the caller gates the vectors too."""
    label = f"{form}/masks{masks}" + ("/2shards" if shards > 1 else "")
    dm, dl, sc = _hip_actor(dev, form, masks, A, rows, cls, shards)
    hip = {"dmean": dm, "dlogstd": dl, "scalars": sc}
    o32, o64 = C.actor_oracle(form, masks, A, rows, cls, "float32"), C.actor_oracle(form, masks, A, rows, cls, "float64")
    C.gate_actor(label, A, rows, hip, o32, o64, groups, vectors=cls is None)
    return dm, dl, o32, o64


def _gate_groups(entry, groups, what):
    for name, members in groups.items():
        C.gate_group(entry, members, f"{what}: {name}")


@pytest.mark.parametrize("rows", C.ROWS[1:])
def test_actor_loss_vs_fp64_oracle(dev, rows):
    """Every form (MAPPO-L with lamda 0.7, HAPPO, MAPPO's per-dimension ratios -- each with and without the active mask -- and
    MACPO's unclipped configuration) at every act_dim: dmean per element, dlogstd (entropy term included) against the sum of the
    absolute per-row terms, the five scalars per kind over all cases of this row count."""
    groups = {}
    for form, masks in C.ACTOR_FORMS:
        for A in C.ACT_DIMS:
            _gate_actor_case(groups, dev, form, masks, A, rows)
    _gate_groups("spo_ma_actor_loss", groups, f"rows {rows}")


@pytest.mark.parametrize("form,masks", C.ACTOR_FORMS)
def test_actor_loss_single_row_in_every_branch(dev, form, masks):
    """rows = 1, once per (ratio below / inside / above the clip range) x (hybrid advantage positive / negative).  One element's
    |f32 - f64| is a single draw of rounding noise, so the six one-row results of an act_dim are gated as one vector."""
    groups = {}
    for A in C.ACT_DIMS:
        parts = [_gate_actor_case(groups, dev, form, masks, A, 1, cls) for cls in C.ACTOR_CLASSES]
        label, cat = f"{form}/masks{masks}", lambda k, key=None: np.concatenate([(q[k] if key is None else q[k][key]).reshape(-1) for q in parts])
        C.gate("spo_ma_actor_loss", label, A, 1, cat(0), cat(2, "dmean"), cat(3, "dmean"), f"dmean {label} A {A}, six one-row cases")
        C.gate("spo_ma_actor_loss", label, A, 1, cat(1), cat(2, "dlogstd"), cat(3, "dlogstd"), f"dlogstd {label} A {A}, six one-row cases",
               scale=cat(3, "dlogstd_scale"))
    _gate_groups("spo_ma_actor_loss", groups, f"{form}/masks{masks} one row")


@pytest.mark.parametrize("rows", [2 * C.SHARD_ROWS, 2])
def test_actor_loss_two_shards(dev, rows):
    """rows_global = 2 x rows in one process: every form called once per half with denom_host / rows_global of the whole batch, the
    halves' sums added, against the oracle on the concatenated batch."""
    groups = {}
    for form, masks in C.ACTOR_FORMS:
        _gate_actor_case(groups, dev, form, masks, 5, rows, shards=2)
    _gate_groups("spo_ma_actor_loss", groups, f"two shards of {rows // 2}")


@pytest.mark.parametrize("form,masks", C.ACTOR_FORMS)
@pytest.mark.parametrize("rows", C.ROWS_PAST_CAP)
def test_actor_loss_second_pass_under_the_cap(dev, rows, form, masks):
    """262 145 rows: one row in workgroup 0's second grid-stride pass; 262 401: a full second pass of workgroup 0, one row of
    workgroup 1.  One act_dim per form."""
    groups = {}
    _gate_actor_case(groups, dev, form, masks, C.PAST_CAP_ACT_DIM[(form, masks)], rows)
    _gate_groups("spo_ma_actor_loss", groups, f"{form}/masks{masks} rows {rows}")


# ------------------------------------------------------------------------------------------------------- spo_ma_value_loss
def _hip_value(dev, active, rows, cls=None, shards=1):
    from safepo import _abi
    lib, ptr, st = _lib()
    p = C.value_problem(active, rows, cls)
    denom = float(p["active"].sum()) if active else float(rows)
    per = rows // shards
    assert per * shards == rows
    dvalues, loss = [], 0.0
    for k in range(shards):
        t = {key: p[key][k * per:(k + 1) * per].contiguous().to(dev) for key in ("values", "value_preds", "ret_c", "ret_o", "active")}
        G = Guarded(dev)
        dv, lo, ws = G.out(per), G.out(1), G.ws(C.VALUE_PARTIAL_DOUBLES)
        _abi.check(lib.spo_ma_value_loss(ptr(t["values"]), ptr(t["value_preds"]), ptr(t["ret_c"]), ptr(t["ret_o"]),
                                         ptr(t["active"]) if active else None, denom, C.CLIP, C.HUBER_DELTA, C.VALUE_LOSS_COEF, per, rows,
                                         ptr(dv), ptr(lo), ptr(ws), st), "spo_ma_value_loss")
        G.check(f"spo_ma_value_loss active {active} rows {per}")
        blocks = min((per + C.WG - 1) // C.WG, C.WG_CAP)
        assert bool(torch.isfinite(ws[:blocks]).all()) and bool(torch.isnan(ws[blocks:]).all())
        dvalues.append(_host(dv, per))
        loss += float(_host(lo, 1)[0])
    return np.concatenate(dvalues), loss


def _gate_value_case(losses, dev, active, rows, cls=None, shards=1):
    label = f"active{active}" + ("/2shards" if shards > 1 else "") + (f"/{cls}" if cls == "on_bound" else "")
    dv, loss = _hip_value(dev, active, rows, cls, shards)
    o32, o64 = C.value_oracle(active, rows, cls, "float32"), C.value_oracle(active, rows, cls, "float64")
    if rows > 1:
        pop = C.value_populations(active, rows, cls)
        print(f"value loss {label} rows {rows}: " + "  ".join(f"{k} {v:.2f}" for k, v in pop.items() if isinstance(v, float)))
    C.gate_value(label, rows, {"dvalues": dv, "loss": loss}, o32, o64, losses, vector=rows > 1)
    return dv, o32, o64


@pytest.mark.parametrize("rows", C.ROWS[1:])
def test_value_loss_vs_fp64_oracle(dev, rows):
    """clip_param 0.2, huber_delta 0.7, with the active pointer and without: the quadratic branch, e > delta and the reference's
    empty e < -delta branch, clipped and unclipped values - value_preds, max taking either error -- each on >= 10 % of the rows
    (printed).  At 257 rows also the rows ON the inclusive clip bound and two shards of 257 with rows_global = 514."""
    losses = []
    for active in C.VALUE_FORMS:
        _gate_value_case(losses, dev, active, rows)
        if rows == C.SHARD_ROWS:
            _gate_value_case(losses, dev, active, rows, "on_bound")
            _gate_value_case(losses, dev, active, 2 * rows, shards=2)
            _gate_value_case(losses, dev, active, 2, shards=2)
    C.gate_group("spo_ma_value_loss", losses, f"value loss, rows {rows}")


@pytest.mark.parametrize("active", C.VALUE_FORMS)
def test_value_loss_single_row_in_every_branch(dev, active):
    """rows = 1 once per branch class (and once on the clip bound), plus two shards of one row; the one-row gradients are gated as one vector."""
    losses, parts = [], []
    for cls in C.VALUE_CLASSES + ["on_bound"]:
        parts.append(_gate_value_case(losses, dev, active, 1, cls))
    cat = lambda k, key=None: np.concatenate([(q[k] if key is None else q[k][key]).reshape(-1) for q in parts])
    C.gate("spo_ma_value_loss", f"active{active}", None, 1, cat(0), cat(1, "dvalues"), cat(2, "dvalues"), f"dvalues active{active}, one-row cases")
    C.gate_group("spo_ma_value_loss", losses, f"value loss active{active}, one-row cases")


@pytest.mark.parametrize("rows", C.ROWS_PAST_CAP)
def test_value_loss_second_pass_under_the_cap(dev, rows):
    losses = []
    for active in C.VALUE_FORMS:
        _gate_value_case(losses, dev, active, rows)
    C.gate_group("spo_ma_value_loss", losses, f"value loss, rows {rows}")


# ------------------------------------------------------------------------------------------------------------ spo_ma_popart_*
def _hip_popart(dev, cfg, rows, shards=1):
    """spo_ma_popart_stats per share, the sums added, spo_ma_popart_forward per share from a copy of the state (every rank of a
    data-parallel job holds one) -> normalised rows, state3, sums2."""
    from safepo import _abi
    lib, ptr, st = _lib()
    train, _, _, beta = cfg
    p = C.popart_problem(cfg, rows)
    per = rows // shards
    assert per * shards == rows
    xs = [p["x"][k * per:(k + 1) * per].contiguous().to(dev) for k in range(shards)]
    total = torch.zeros(2, dtype=torch.float64, device=dev)
    for x in xs:
        G = Guarded(dev)
        sums, ws = G.out(2, torch.float64), G.ws(C.POPART_PARTIAL_DOUBLES)
        _abi.check(lib.spo_ma_popart_stats(ptr(x), per, ptr(sums), ptr(ws), st), "spo_ma_popart_stats")
        G.check(f"spo_ma_popart_stats rows {per}")
        blocks = min((per + C.WG - 1) // C.WG, C.WG_CAP)
        assert bool(torch.isfinite(ws[:2 * blocks]).all()) and bool(torch.isnan(ws[2 * blocks:]).all())
        total += sums[:2]
    outs, states = [], []
    for x in xs:
        G = Guarded(dev)
        state, out = G.inout(p["state3"]), G.out(per)
        _abi.check(lib.spo_ma_popart_forward(ptr(x), per, ptr(state), beta, C.POPART_EPS, train, ptr(total) if train else None, rows, ptr(out),
                                             st), "spo_ma_popart_forward")
        G.check(f"spo_ma_popart_forward rows {per}")
        outs.append(_host(out, per))
        states.append(_host(state, 3))
    assert all((s == states[0]).all() for s in states)
    return np.concatenate(outs), states[0], total.cpu().numpy()


def _gate_popart_case(dev, cfg, rows, shards=1):
    label = C.popart_name(cfg) + ("/2shards" if shards > 1 else "")
    out, state, sums = _hip_popart(dev, cfg, rows, shards)
    o32, o64 = C.popart_oracle(cfg, rows, "float32"), C.popart_oracle(cfg, rows, "float64")
    x64 = C.popart_problem(cfg, rows)["x"].double()
    # the kernel sums in double: at most rows roundings of 2^-53 relative to the sum of the absolute terms
    for k, terms in enumerate((x64.abs().sum(), (x64 ** 2).sum())):
        assert abs(sums[k] - o64["sums"][k]) <= rows * 2.0 ** -53 * float(terms), (label, rows, k, sums[k], o64["sums"][k])
    if cfg[0]:
        C.gate("spo_ma_popart_forward", label, None, rows, state, o32["state3"], o64["state3"], f"PopArt state {label} rows {rows}",
               scale=o64["state_scales"])
    else:
        assert (state == C.popart_problem(cfg, rows)["state3"].double().numpy()).all(), (label, rows)
    # one fresh-state training row: m = (x * (1 - beta)) / (1 - beta) carries two float32 roundings of |x| -- at most one ulp of |x|
    # together --, the float64 output is exactly 0 and max|f64| no scale: the floor there is that ulp over sqrt(var) (= 0.1: var is clamped)
    floor = float(np.spacing(np.float32(abs(float(x64[0]))))) / 0.1 if (rows == 1 and cfg[0] and cfg[1] == "fresh") else None
    C.gate("spo_ma_popart_forward", label, None, rows, out, o32["out"], o64["out"], f"normalised rows {label} rows {rows}", floor=floor)


@pytest.mark.parametrize("rows", C.ROWS + C.ROWS_PAST_CAP)
def test_popart_vs_fp64_oracle(dev, rows):
    """train 1 and 0; a fresh state of zeros (the debiasing clamp sits at epsilon) and one after many updates; an input whose
    variance falls under the 1e-2 clamp and one well above; beta 0.99999 and 0.9 -- all combinations at 257 rows, four of them at
    the other counts; at 257 rows also two shards with rows_global = 514 and the sums taken over both."""
    for cfg in (C.POPART_ALL if rows == C.SHARD_ROWS else C.POPART_FEW):
        _gate_popart_case(dev, cfg, rows)
    if rows == C.SHARD_ROWS:
        for cfg in C.POPART_FEW[:2]:
            _gate_popart_case(dev, cfg, 2 * rows, shards=2)


# ------------------------------------------------------------------------------------------------------------ spo_ma_clip_adam
def _hip_adam(dev, n, name):
    from safepo import _abi
    lib, ptr, st = _lib()
    p = C.adam_problem(n, name)
    G = Guarded(dev)
    theta, m, v, norm, ws = G.inout(p["theta"]), G.inout(p["m"]), G.inout(p["v"]), G.out(1), G.ws(C.ADAM_PARTIAL_DOUBLES)
    grad = p["grad"].to(dev)
    _abi.check(lib.spo_ma_clip_adam(ptr(theta), ptr(grad), ptr(m), ptr(v), n, p["step"], C.ADAM_LR, C.ADAM_EPS, p["wd"], p["max_norm"],
                                    p["use_clip"], ptr(norm), ptr(ws), st), "spo_ma_clip_adam")
    G.check(f"spo_ma_clip_adam n {n} {name}")
    assert torch.equal(grad.cpu(), p["grad"])                                    # the gradient is only read
    return {"norm": float(_host(norm, 1)[0]), "m": _host(m, n), "v": _host(v, n), "update": _host(theta, n) - p["theta"].double().numpy()}


@pytest.mark.parametrize("n", C.ADAM_N)
def test_clip_adam_vs_fp64_oracle(dev, n):
    """clip off / on under the bound / on a factor 3 over it / 0.05 % over it at a norm of 1e-3, weight_decay 0 and 1e-2, Adam
    steps 1 and 10 000, from non-zero moments, and a new optimiser's first step from zero moments: the returned norm, both moments, and the UPDATE theta_after - theta_before against
    3 |f32 - f64| + half an ulp of max|theta| (a 1e-6 floor on the O(1) parameter would hide a wrong step of size lr)."""
    norms = []
    for cfg in (C.ADAM_CONFIGS if n <= 1000 else C.ADAM_BIG_CONFIGS):
        name = C.adam_name(cfg)
        C.gate_adam(name, n, _hip_adam(dev, n, name), C.adam_oracle(n, name, "float32"), C.adam_oracle(n, name, "float64"), norms)
    C.gate_group("spo_ma_clip_adam", norms, f"gradient norm, n {n}")


# --------------------------------------------------------------------------------------------------------- spo_ma_lamda_update
def test_lamda_update_both_sides_of_the_relu(dev):
    from safepo import _abi
    lib, ptr, st = _lib()
    members = []
    for k, case in enumerate(C.LAMDA_CASES):
        lam, s3, aver, limit, rate = case
        G = Guarded(dev)
        lamda = G.inout(torch.tensor([lam], dtype=torch.float32))
        scalars = torch.tensor([NAN, NAN, NAN, s3, NAN], dtype=torch.float32, device=dev)       # only mean(imp * cost_adv) may be read
        _abi.check(lib.spo_ma_lamda_update(ptr(lamda), ptr(scalars), aver, limit, C.GAMMA32, rate, st), "spo_ma_lamda_update")
        G.check("spo_ma_lamda_update")
        (w32, _, _), (w64, scale, pre) = C.lamda_oracle(case, "float32"), C.lamda_oracle(case, "float64")
        hip = float(_host(lamda, 1)[0])
        assert (hip == 0.0) == (pre < 0), (case, hip, pre)
        members.append((f"case{k}", None, 1, hip, w32, w64, scale))
    assert {m[5] == 0.0 for m in members} == {True, False}
    C.gate_group("spo_ma_lamda_update", members, "multiplier after the update")


# ------------------------------------------------------------------------------------------- spo_ma_sample / spo_ma_log_probs
def _hip_sample(dev, rows, A, coefs):
    from safepo import _abi
    lib, ptr, st = _lib()
    p = {k: v.to(dev) for k, v in C.sample_problem(rows, A, coefs).items()}
    n, res = rows * A, {}
    for det in (0, 1):
        G = Guarded(dev)
        act, logp = G.out(n), G.out(n)
        _abi.check(lib.spo_ma_sample(ptr(p["mean"]), ptr(p["log_std"]), None if det else ptr(p["eps"]), coefs[0], coefs[1], det, ptr(act),
                                     ptr(logp), rows, A, st), "spo_ma_sample")
        G.check(f"spo_ma_sample rows {rows} A {A}")
        if det:
            assert torch.equal(act[:n].cpu(), p["mean"].reshape(-1).cpu())
            res["logp_det"] = _host(logp, n)
        else:
            res["act"], res["logp"] = _host(act, n), _host(logp, n)
    G = Guarded(dev)
    logp = G.out(n)
    _abi.check(lib.spo_ma_log_probs(ptr(p["mean"]), ptr(p["log_std"]), ptr(p["act"]), coefs[0], coefs[1], ptr(logp), rows, A, st), "spo_ma_log_probs")
    G.check(f"spo_ma_log_probs rows {rows} A {A}")
    res["logp_given"] = _host(logp, n)
    return res


@pytest.mark.parametrize("rows", sorted({r for r, _ in C.SAMPLE_SHAPES}))
def test_sample_and_log_probs_vs_fp64_oracle(dev, rows):
    """Sampled (act = mean + std * eps and its log-probabilities) and deterministic (act == mean bit for bit), and the
    log-probabilities of given actions; log_std over [-4, 4], std coefficients (1, 0.5) and (2, 1.5).  At one row the act_dims
    are gated as one vector."""
    entry = {"act": "spo_ma_sample", "logp": "spo_ma_sample", "logp_det": "spo_ma_sample", "logp_given": "spo_ma_log_probs"}
    for coefs in C.SAMPLE_COEFS:
        shapes = [A for r, A in C.SAMPLE_SHAPES if r == rows]
        res = [(A, _hip_sample(dev, rows, A, coefs), C.sample_oracle(rows, A, coefs, "float32"), C.sample_oracle(rows, A, coefs, "float64")) for A in shapes]
        if rows == 1:
            cat = lambda k, key: np.concatenate([q[k][key].reshape(-1) for q in res])
            res = [(None, {k: cat(1, k) for k in entry}, {k: cat(2, k) for k in entry}, {k: cat(3, k) for k in entry})]
        for A, hip, o32, o64 in res:
            for key, ent in entry.items():
                C.gate(ent, f"{key}/coefs{coefs}", A, rows, hip[key], o32[key], o64[key], f"{key} rows {rows} A {A} coefs {coefs}")


# ------------------------------------------------------------------------------------------------------------------ spo_ma_gae
@pytest.mark.parametrize("T", C.GAE_T)
def test_gae_bit_identical_to_the_restatement(dev, T):
    """T below, around and past the kernel's unroll of 8 x N of one lane, a ragged workgroup and two workgroups; random masks, two
    different PopArt de-normalisations: bit-identical to MR.masked_gae in float32, row T and the guard untouched."""
    from safepo import _abi
    lib, ptr, st = _lib()
    for N in C.GAE_N:
        p = C.gae_problem(T, N)
        t = {k: p[k].to(dev) for k in ("rewards", "costs", "value_preds", "cost_preds", "masks")}
        G = Guarded(dev)
        ret, cret = G._new((T + 1) * N, torch.float32, False), G._new((T + 1) * N, torch.float32, False)
        _abi.check(lib.spo_ma_gae(ptr(t["rewards"]), ptr(t["costs"]), ptr(t["value_preds"]), ptr(t["cost_preds"]), ptr(t["masks"]), ptr(ret),
                                  ptr(cret), T, N, p["gamma"], p["gae_lambda"], p["sd_r"], p["mu_r"], p["sd_c"], p["mu_c"], st), "spo_ma_gae")
        G.check(f"spo_ma_gae T {T} N {N}")
        for buf, want in ((ret, p["want_r"]), (cret, p["want_c"])):
            assert bool(torch.isnan(buf[T * N:]).all())                                # row T is not written, as in the reference
            assert np.array_equal(buf[:T * N].cpu().numpy().view(np.uint32), want[:T].reshape(-1).numpy().view(np.uint32)), (T, N)


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_entry_points_refuse_bad_arguments_before_launching(dev):
    """rows = 0, act_dim = 17, denom_host = 0, rows_global < rows and a null pointer: non-zero return, every output untouched.  All
    other arguments are valid, and every buffer is large enough for act_dim 17."""
    from safepo import _abi
    lib, ptr, st = _lib()
    rows, A = 8, 4
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    one = lambda *s: torch.ones(*s, dtype=torch.float32, device=dev)
    cfg = _abi.MaLossCfg(C.CLIP, 0.01, 1.0, 0.5, 1, 0)
    G = Guarded(dev)
    big = rows * 17
    o = {k: G.out(big) for k in ("a", "b", "c")}
    wsd = G.ws(C.ACTOR_PARTIAL_DOUBLES)
    mean, ls, act, old = z(rows, 17), z(17), z(rows, 17), z(rows, 17)
    vec, lam = one(rows), z(1)
    refused = []

    def actor(rows=rows, A=A, denom=float(rows), rows_global=rows, mean_p=ptr(mean), out_p=ptr(o["a"])):
        return lib.spo_ma_actor_loss(mean_p, ptr(ls), ptr(act), ptr(old), ptr(vec), ptr(vec), ptr(vec), ptr(vec), ptr(lam), cfg, rows, A, denom,
                                     rows_global, out_p, ptr(o["b"]), ptr(o["c"]), ptr(wsd), st)
    refused += [("actor rows 0", actor(rows=0)), ("actor act_dim 17", actor(A=17)), ("actor act_dim 0", actor(A=0)), ("actor denom 0", actor(denom=0.0)),
                ("actor rows_global < rows", actor(rows_global=rows - 1)), ("actor null input", actor(mean_p=None)), ("actor null output", actor(out_p=None))]

    def value(rows=rows, denom=float(rows), rows_global=rows, v_p=ptr(vec), out_p=ptr(o["a"])):
        return lib.spo_ma_value_loss(v_p, ptr(vec), ptr(vec), ptr(vec), None, denom, C.CLIP, C.HUBER_DELTA, 1.0, rows, rows_global, out_p, ptr(o["b"]),
                                     ptr(wsd), st)
    refused += [("value rows 0", value(rows=0)), ("value denom 0", value(denom=0.0)), ("value rows_global < rows", value(rows_global=rows - 1)),
                ("value null input", value(v_p=None)), ("value null output", value(out_p=None))]

    def sample(rows=rows, A=A, det=0, eps_p=ptr(act), out_p=ptr(o["a"])):
        return lib.spo_ma_sample(ptr(mean), ptr(ls), eps_p, 1.0, 0.5, det, out_p, ptr(o["b"]), rows, A, st)
    refused += [("sample rows 0", sample(rows=0)), ("sample act_dim 17", sample(A=17)), ("sample null eps", sample(eps_p=None)),
                ("sample null output", sample(out_p=None))]

    def logp(rows=rows, A=A, act_p=ptr(act)):
        return lib.spo_ma_log_probs(ptr(mean), ptr(ls), act_p, 1.0, 0.5, ptr(o["a"]), rows, A, st)
    refused += [("log_probs rows 0", logp(rows=0)), ("log_probs act_dim 17", logp(A=17)), ("log_probs null input", logp(act_p=None))]
    sums = G.out(2, torch.float64)
    refused += [("popart_stats rows 0", lib.spo_ma_popart_stats(ptr(vec), 0, ptr(sums), ptr(wsd), st)),
                ("popart_stats null", lib.spo_ma_popart_stats(None, rows, ptr(sums), ptr(wsd), st))]
    good = torch.zeros(2, dtype=torch.float64, device=dev)

    def forward(rows=rows, train=1, sums_p=ptr(good), rows_global=rows, state_p=ptr(o["c"])):
        return lib.spo_ma_popart_forward(ptr(vec), rows, state_p, 0.9, C.POPART_EPS, train, sums_p, rows_global, ptr(o["a"]), st)
    refused += [("popart_forward rows 0", forward(rows=0)), ("popart_forward rows_global < rows", forward(rows_global=rows - 1)),
                ("popart_forward train without sums", forward(sums_p=None)), ("popart_forward null state", forward(state_p=None, train=0))]

    def adam(n=rows, step=0, grad_p=ptr(vec), norm_p=ptr(o["c"])):
        return lib.spo_ma_clip_adam(ptr(o["a"]), grad_p, ptr(o["b"]), ptr(o["b"]), n, step, C.ADAM_LR, C.ADAM_EPS, 0.0, 10.0, 1, norm_p, ptr(wsd), st)
    refused += [("clip_adam n 0", adam(n=0)), ("clip_adam step -1", adam(step=-1)), ("clip_adam null gradient", adam(grad_p=None)),
                ("clip_adam null norm", adam(norm_p=None))]
    refused += [("lamda_update null scalars", lib.spo_ma_lamda_update(ptr(o["a"]), None, 1.0, 1.0, 0.99, 0.1, st)),
                ("lamda_update null multiplier", lib.spo_ma_lamda_update(None, ptr(vec), 1.0, 1.0, 0.99, 0.1, st)),
                ("gae null", lib.spo_ma_gae(None, ptr(vec), ptr(vec), ptr(vec), ptr(vec), ptr(o["a"]), ptr(o["b"]), 1, 4, 0.99, 0.95, 1.0, 0.0, 1.0, 0.0, st)),
                ("gae negative T", lib.spo_ma_gae(ptr(vec), ptr(vec), ptr(vec), ptr(vec), ptr(vec), ptr(o["a"]), ptr(o["b"]), -1, 4, 0.99, 0.95, 1.0, 0.0,
                                                  1.0, 0.0, st))]
    for what, rc in refused:
        assert rc != 0, what
        assert lib.spo_last_error(), what
    G.untouched("refusals")
    # the same calls with nothing wrong go through (so the refusals above were about the one bad argument)
    for what, rc in (("actor", actor()), ("value", value()), ("sample", sample()), ("log_probs", logp()), ("popart_stats",
                     lib.spo_ma_popart_stats(ptr(vec), rows, ptr(sums), ptr(wsd), st))):
        _abi.check(rc, what)
    torch.cuda.synchronize()
