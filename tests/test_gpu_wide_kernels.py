"""GPU tests of the wide-network kernels by direct ABI calls, path by path and branch by branch, under the float64 yardstick:
spo_wide_actor_loss (three modes), spo_wide_kl_penalty_split / _combine, spo_wide_linesearch_sums, spo_wide_ppo_loss,
spo_wide_critic_loss, spo_wide_fvp_cotangent, spo_gauss_sample, spo_gauss_kl_sum, spo_gather_rows / _at, spo_mlp_forward /
_backward / _jvp above 128 rows and their _multi forms, and the four spo_wide_clip_adam* entries with
spo_wide_rows_clip_adam_dev_log (csrc/wide.hip, csrc/gemm_f32.hip, the optimiser pass of csrc/mlp_rows.hip).

The reference is the same operation in plain torch float64 on the CPU (autograd, torch.distributions, clip_grad_norm_,
torch.optim.Adam, torch.func.jvp), the yardstick the same oracle in float32, and a HIP result passes when
|hip - f64| <= 3 |f32 - f64| + floor in max-norm and L2 (tests/ma_yardstick.gate), floor = 1e-6 of the quantity's scale; pure data
movement is compared bit for bit.  Shapes: act_dim 1 .. 64 with ragged lanes inside a row's lane group, row counts around one
workgroup's rows and past every capped grid, the GEMM forms by size and alignment.  Every output and every partial_ws has exactly
the documented size and is followed by a guard of NaNs that must be untouched.  The cases, their oracles and the gates are in
tests/wide_kernel_cases.py (tests/test_wide_kernel_cases_host.py shows on the CPU that the gates refuse wrong oracles); after the
last test the worst ratio |hip - f64| / (3 |f32 - f64| + floor) per test is printed (profiles/wide_kernels/gate_ratios.txt)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wide_kernel_cases as C  # noqa: E402

GUARD = 64
NAN = float("nan")
INT_GUARD = -(2 ** 62) - 12345


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
    """Device buffers of exactly n elements followed by GUARD NaNs.  out(): a result the call must fill; ws(): a workspace;
    inout(): a buffer with given contents."""

    def __init__(self, dev):
        self.dev, self.items, self.ints = dev, [], []

    def _new(self, n, dtype, full, init=None):
        if not dtype.is_floating_point:                                # (an int64 cursor: a sentinel stands in for the NaNs)
            buf = torch.full((n + GUARD,), INT_GUARD, dtype=dtype, device=self.dev)
            buf[:n] = init.reshape(-1).to(self.dev)
            self.ints.append((buf, n))
            return buf
        buf = torch.full((n + GUARD,), NAN, dtype=dtype, device=self.dev)
        if init is not None:
            buf[:n] = init.reshape(-1).to(self.dev)
        self.items.append((buf, n, full))
        return buf

    def out(self, n, dtype=torch.float32):
        return self._new(n, dtype, True)

    def ws(self, n, dtype=torch.float64):
        return self._new(n, dtype, False)

    def inout(self, init):
        return self._new(init.numel(), init.dtype, True, init)

    def check(self, what):
        torch.cuda.synchronize()
        for buf, n, full in self.items:
            assert bool(torch.isnan(buf[n:]).all()), f"{what}: written past the end of a buffer of {n}"
            assert not full or bool(torch.isfinite(buf[:n]).all()), f"{what}: an output of {n} is not filled"
        for buf, n in self.ints:
            assert bool((buf[n:] == INT_GUARD).all()), f"{what}: written past the end of an integer buffer of {n}"

    def untouched(self, what):
        torch.cuda.synchronize()
        for buf, n, full in self.items:
            assert bool(torch.isnan(buf).all()), f"{what}: a refused call wrote to a buffer"


def _lib():
    from safepo import _abi
    return _abi.load(), _abi.ptr, _abi.stream_ptr()


def _ok(rc, what):
    from safepo import _abi
    _abi.check(rc, what)


def _host(buf, n=None):
    return (buf if n is None else buf[:n]).double().cpu().numpy()


PER_ROW = {"mean", "act", "logp_old", "adv", "adv_b", "old_mean", "mean_new", "mean_old", "adv_a"}


def _up(p, dev, keys, lo=0, hi=None):
    return {k: (p[k][lo:hi] if k in PER_ROW else p[k]).contiguous().to(dev) for k in keys}


def _gate_groups(groups, what):
    for name, members in groups.items():
        C.gate_group(members, f"{what}: {name}")


# ------------------------------------------------------------------------------------------------------- spo_wide_actor_loss
ACTOR_KEYS = ("mean", "log_std", "act", "logp_old", "adv", "old_mean", "old_std")


def _hip_actor(dev, mode, p, p0, p1, chunks=None, prime=None, float_outs=True):
    """spo_wide_actor_loss over the problem `p` in row chunks [(lo, hi)] (None: one call) -> d_mean [rows, A], sums [2 + A]
    (double, accumulated over the chunks), loss_out and d_log_std_out of the LAST call.  prime: what sums_inout holds before the
    first call (which runs with accumulate = 0)."""
    lib, ptr, st = _lib()
    rows, A = p["mean"].shape
    chunks = chunks or [(0, rows)]
    G = Guarded(dev)
    sums = G.inout(torch.full((2 + A,), 1e30, dtype=torch.float64) if prime is None else prime)
    dmean, loss, dls = [], None, None
    for k, (lo, hi) in enumerate(chunks):
        t = _up(p, dev, ACTOR_KEYS, lo, hi)
        dm, ws = G.out((hi - lo) * A), G.ws(C.ACTOR_PARTIAL)
        loss, dls = (G.out(1), G.out(A)) if float_outs else (None, None)
        _ok(lib.spo_wide_actor_loss(mode, ptr(t["mean"]), ptr(t["log_std"]), ptr(t["act"]), ptr(t["logp_old"]), ptr(t["adv"]), ptr(t["old_mean"]),
                                    ptr(t["old_std"]), hi - lo, rows, A, p0, p1, ptr(dm), ptr(sums), 1 if k else 0, ptr(loss), ptr(dls), ptr(ws),
                                    C.ACTOR_PARTIAL, st), "spo_wide_actor_loss")
        G.check(f"spo_wide_actor_loss mode {mode} A {A} rows {hi - lo} of {rows}")
        blocks = min(-(-(hi - lo) // C.rpb(A)), C.LOSS_CAP)
        parts = ws[:C.ACTOR_PARTIAL].view(C.LOSS_CAP, 2 + C.MAX_ACT)
        assert bool(torch.isfinite(parts[:blocks, :2 + A]).all()) and bool(torch.isnan(parts[blocks:]).all()) and bool(torch.isnan(parts[:, 2 + A:]).all())
        dmean.append(_host(dm, (hi - lo) * A).reshape(hi - lo, A))
    out = {"d_mean": np.concatenate(dmean), "sums": _host(sums, 2 + A)}
    if float_outs:
        out.update({"loss": float(loss[0]), "d_log_std_out": _host(dls, A)})
    out["d_log_std"] = out["sums"][2:]
    return out


def _gate_loss_case(hip, o32, o64, what, groups, sign=1.0):
    """Vectors through the gates; the two scalars into `groups`.  d_log_std_out is the float copy of the double sums."""
    C.gate_actor_vectors(hip, o32, o64, what)
    n = o64["rows_total"]
    if "d_log_std_out" in hip:
        assert np.array_equal(hip["d_log_std_out"], hip["sums"][2:].astype(np.float32).astype(np.float64)), what
        groups.setdefault("loss_out", []).append((hip["loss"], sign * o32["loss"], sign * o64["loss"], o64["scale"]))
    groups.setdefault("sums[0]", []).append((hip["sums"][0], o32["term_sum"], o64["term_sum"], o64["scale"] * n))


@pytest.mark.parametrize("A", C.ACT_DIMS)
def test_actor_loss_clipped_surrogate(dev, A):
    """Mode 0 at every lane-group width, around one workgroup's rows (rpb - 1, rpb, rpb + 1), at one row and at 1 000: d_mean, the
    double sums, loss_out, d_log_std_out."""
    groups = {}
    for rows in C.actor_rows(A):
        p = C.actor_problem(A, rows)
        hip = _hip_actor(dev, 0, p, C.CLIP, 0.0)
        _gate_loss_case(hip, C.clip_oracle(A, rows, None, False, "float32"), C.clip_oracle(A, rows, None, False, "float64"), f"clip A {A} rows {rows}", groups)
        assert hip["sums"][1] == 0.0
    _gate_groups(groups, f"clip A {A}")


@pytest.mark.parametrize("A", [1, 17, 64])
def test_actor_loss_clipped_surrogate_one_row_per_class(dev, A):
    """One row in each of the six classes (ratio below / inside / above the clip range x sign of the advantage); the six d_mean and
    d_log_std vectors are gated as one vector, each divided by its case's scale.  Above with adv > 0 and below with adv < 0 are
    clipped: the gradient is exactly zero."""
    vec, groups = {"hip": [], "f32": [], "f64": []}, {}
    for cls in C.CLASSES:
        p = C.actor_problem(A, 1, cls)
        hip = _hip_actor(dev, 0, p, C.CLIP, 0.0)
        o32, o64 = C.clip_oracle(A, 1, cls, False, "float32"), C.clip_oracle(A, 1, cls, False, "float64")
        dead = (cls[0] == "above" and cls[1] > 0) or (cls[0] == "below" and cls[1] < 0)
        assert (o64["d_mean"] == 0).all() == dead
        if dead:
            assert (hip["d_mean"] == 0).all() and (hip["d_log_std"] == 0).all(), cls
        else:
            for key in ("d_mean", "d_log_std"):
                s = np.abs(o64[key]).max()
                for nm, o in (("hip", hip), ("f32", o32), ("f64", o64)):
                    vec[nm].append(o[key].reshape(-1) / s)
        groups.setdefault("loss_out", []).append((hip["loss"], o32["loss"], o64["loss"], o64["scale"]))
        groups.setdefault("sums[0]", []).append((hip["sums"][0], o32["term_sum"], o64["term_sum"], o64["scale"]))
    C.gate(*(np.concatenate(vec[k]) for k in ("hip", "f32", "f64")), f"clip one-row classes A {A}: gradients", scale=1.0)
    _gate_groups(groups, f"clip one-row classes A {A}")


def test_actor_loss_clipped_surrogate_exact_tie(dev):
    """Rows with adv == 0: both surrogates are equal (s1 == s2), torch.min's backward splits the gradient of a zero -- d_mean is
    exactly 0 and finite there, and the rest of the batch passes the gates."""
    A, rows, groups = 17, 1000, {}
    p = C.actor_problem(A, rows, None, True)
    ties = (p["adv"] == 0).numpy()
    assert ties.sum() == 143
    hip = _hip_actor(dev, 0, p, C.CLIP, 0.0)
    assert np.isfinite(hip["d_mean"]).all() and (hip["d_mean"][ties] == 0).all() and (hip["d_mean"][~ties] != 0).any()
    _gate_loss_case(hip, C.clip_oracle(A, rows, None, True, "float32"), C.clip_oracle(A, rows, None, True, "float64"), "clip tie", groups)
    _gate_groups(groups, "clip tie")


@pytest.mark.parametrize("A", C.ACT_DIMS)
def test_actor_loss_plain_surrogate(dev, A):
    """Mode 1 with both signs of p0; at act_dim 3 / 17 also in three chunks and a ragged tail (accumulate, rows_total > rows)
    against the oracle of the whole batch.  The first call stores (accumulate = 0) into sums primed with garbage."""
    groups = {}
    for rows in C.actor_rows(A):
        p = C.actor_problem(A, rows)
        for sign in (1.0, -1.0):
            hip = _hip_actor(dev, 1, p, sign, 0.0)
            _gate_loss_case(hip, C.surr_oracle(A, rows, sign, "float32"), C.surr_oracle(A, rows, sign, "float64"), f"surr A {A} rows {rows} sign {sign}", groups)
    if A in (3, 17):
        rows = 1000
        p = C.actor_problem(A, rows)
        chunks = [(0, 300), (300, 600), (600, 900), (900, 1000)]
        hip = _hip_actor(dev, 1, p, -1.0, 0.0, chunks)
        o32, o64 = C.surr_oracle(A, rows, -1.0, "float32"), C.surr_oracle(A, rows, -1.0, "float64")
        # (the float outputs of the last chunk's call are formed from the running sums: the whole batch's)
        _gate_loss_case(hip, o32, o64, f"surr A {A} chunked", groups)
    _gate_groups(groups, f"surr A {A}")


def _gate_klpen_case(hip, o32, o64, what, groups, rows):
    C.gate_actor_vectors(hip, o32, o64, what)
    assert hip["sums"][1] == o64["count"], (what, hip["sums"][1], o64["count"])
    groups.setdefault("loss_out", []).append((hip["loss"], o32["loss"], o64["loss"], o64["scale"]))
    groups.setdefault("sums[0]", []).append((hip["sums"][0], o32["term_sum"], o64["term_sum"], o64["scale"] * rows))


@pytest.mark.parametrize("A", C.ACT_DIMS)
def test_actor_loss_kl_penalty(dev, A):
    """Mode 2 (FOCOPS; CUP's second stage with kl_bound = +inf): old_std != exp(log_std), so the var_ratio - 1 term of d(log_std) is
    live; both indicator classes hold about half the rows.  A bound below every row's KL: F = 0 and d_mean is exactly 0."""
    groups = {}
    for rows, bound in [(r, "mid") for r in C.actor_rows(A)] + [(1000, "inf"), (1000, "none")]:
        p = C.actor_problem(A, rows, None, False, bound)
        hip = _hip_actor(dev, 2, p, p["kl_bound"], C.PG_COEF)
        o32, o64 = C.klpen_oracle(A, rows, bound, "float32"), C.klpen_oracle(A, rows, bound, "float64")
        if bound == "none":
            assert o64["count"] == 0 and (hip["d_mean"] == 0).all() and (hip["sums"] == 0).all() and hip["loss"] == 0
            continue
        assert bound != "inf" or o64["count"] == rows
        _gate_klpen_case(hip, o32, o64, f"klpen A {A} rows {rows} {bound}", groups, rows)
    _gate_groups(groups, f"klpen A {A}")


# ------------------------------------------------------------------------------- spo_wide_kl_penalty_split / _combine
def _hip_split(dev, p):
    lib, ptr, st = _lib()
    rows, A = p["mean"].shape
    t, G = _up(p, dev, ACTOR_KEYS), Guarded(dev)
    dk, dp, lk, lp, sums, ws = G.out(rows * A), G.out(rows * A), G.out(A), G.out(A), G.ws(8, torch.float32), G.ws(C.SPLIT_PARTIAL)
    _ok(lib.spo_wide_kl_penalty_split(ptr(t["mean"]), ptr(t["log_std"]), ptr(t["act"]), ptr(t["logp_old"]), ptr(t["adv"]), ptr(t["old_mean"]),
                                      ptr(t["old_std"]), rows, A, p["kl_bound"], C.PG_COEF, ptr(dk), ptr(dp), ptr(lk), ptr(lp), ptr(sums), ptr(ws),
                                      C.SPLIT_PARTIAL, st), "spo_wide_kl_penalty_split")
    G.check(f"spo_wide_kl_penalty_split A {A} rows {rows}")
    assert bool(torch.isfinite(sums[:6]).all()) and bool(torch.isnan(sums[6:8]).all())          # six of SPO_KLPEN_SUMS = 8 floats are this entry's
    return {"d_mean_kl": _host(dk, rows * A).reshape(rows, A), "d_mean_pg": _host(dp, rows * A).reshape(rows, A), "d_log_std_kl": _host(lk, A),
            "d_log_std_pg": _host(lp, A), "sums": _host(sums, 6), "dev": (dk, dp, lk, lp, sums)}


def _combine(dev, grad, pg, sums, begin, actor_begin, scale, want_loss=True):
    lib, ptr, st = _lib()
    G = Guarded(dev)
    g, loss = G.inout(grad), (G.out(1) if want_loss else None)
    _ok(lib.spo_wide_kl_penalty_combine(ptr(g), ptr(pg), ptr(sums), grad.numel(), begin, actor_begin, scale, C.PG_COEF, ptr(loss), st),
        "spo_wide_kl_penalty_combine")
    G.check("spo_wide_kl_penalty_combine")
    return g[:grad.numel()].clone(), (float(loss[0]) if want_loss else None)


@pytest.mark.parametrize("A", C.ACT_DIMS)
def test_kl_penalty_split_then_combine(dev, A):
    """The split form's two cotangents, its two d(log_std) parts and its row sums against the gradients of mean(ind * kl) and of
    -pg_coef * mean(ratio * adv); then spo_wide_kl_penalty_combine at grad_scale 1 and 0.5 over [critic filler | d_mean | d_log_std]
    against mode 2's oracle and its loss."""
    groups = {}
    for rows, bound in [(r, "mid") for r in C.actor_rows(A)] + [(1000, "inf")]:
        p = C.actor_problem(A, rows, None, False, bound)
        hip = _hip_split(dev, p)
        o32, o64 = C.klpen_oracle(A, rows, bound, "float32"), C.klpen_oracle(A, rows, bound, "float64")
        what = f"split A {A} rows {rows} {bound}"
        for sfx in ("_kl", "_pg"):
            C.gate_actor_vectors(hip, o32, o64, what, sfx)
        s = hip["sums"]
        assert s[0] == 0 and s[1] == 0 and s[2] == o64["count"] and s[5] == rows, (what, s)
        groups.setdefault("sum ind*KL", []).append((s[3], o32["kl_sum"], o64["kl_sum"], max(o64["kl_sum"], 1e-30)))
        groups.setdefault("sum ratio*adv", []).append((s[4], o32["ra_sum"], o64["ra_sum"], o64["ra_scale"]))
        if rows != 1000:
            continue
        dk, dp, lk, lp, sums = hip["dev"]
        filler = torch.linspace(-1.0, 1.0, 37, device=dev)
        n = rows * A
        grad = torch.cat([filler, dk[:n], lk[:A]])
        pg = torch.cat([torch.full((37,), NAN, device=dev), dp[:n], lp[:A]])          # below actor_begin pg_grad is not read
        for scale in (1.0, 0.5):
            g, loss = _combine(dev, grad, pg, sums, 0, 37, scale)
            assert torch.equal(g[:37], filler * scale)
            got = {"d_mean": _host(g[37:37 + n]).reshape(rows, A), "d_log_std": _host(g[37 + n:])}
            sc = lambda o: {k: (v * scale if isinstance(v, np.ndarray) else v) for k, v in o.items()}
            C.gate_actor_vectors(got, sc(o32), sc(o64), f"{what} combined x {scale}")
            groups.setdefault("combined loss", []).append((loss, o32["loss"], o64["loss"], o64["scale"]))
    _gate_groups(groups, f"split A {A}")


@pytest.mark.parametrize("begin_is_actor", [0, 1])
def test_kl_penalty_combine_past_the_capped_grid(dev, begin_is_actor):
    """More than 1 024 x 256 elements behind `begin`: grad[begin, n) = (grad + F pg [from actor_begin on]) * scale, nothing below
    begin is touched.  Against the same expression in float32 / float64 torch."""
    n, ab = 1024 * 256 + 300 + 77, 77
    begin = ab if begin_is_actor else 0
    g = torch.Generator().manual_seed(5 + begin_is_actor)
    grad, pg = torch.randn(n, generator=g), torch.randn(n, generator=g)
    sums = torch.tensor([0.0, 0.0, 487.0, 21.5, -15.9, 1000.0, NAN, NAN])
    got, loss = _combine(dev, grad.to(dev), pg.to(dev), sums.to(dev), begin, ab, 0.5)
    assert torch.equal(got[:begin].cpu(), grad[:begin])

    def want(dt):
        F = sums[2].to(dt) / sums[5].to(dt)
        w = grad.to(dt).clone()
        w[ab:] += F * pg.to(dt)[ab:]
        w[begin:] *= 0.5
        return w.double().numpy(), float((sums[3].to(dt) - C.PG_COEF * F * sums[4].to(dt)) / sums[5].to(dt))
    (w32, l32), (w64, l64) = want(torch.float32), want(torch.float64)
    C.gate(_host(got)[begin:], w32[begin:], w64[begin:], f"combine begin {begin}")
    C.gate_group([(loss, l32, l64, 21.5 / 1000 + C.PG_COEF * 0.487 * 15.9 / 1000)], "combine loss")


# ------------------------------------------------------------------------------------------------ past the capped grids
@pytest.mark.parametrize("A,rows", C.LOSS_PAST_CAP)
def test_actor_loss_kernels_past_the_capped_grid(dev, A, rows):
    """256 x rpb + 1 rows: workgroup 0's first wave takes a second grid-stride pass of one row.  All three modes and the split form."""
    groups = {}
    p = C.actor_problem(A, rows)
    _gate_loss_case(_hip_actor(dev, 0, p, C.CLIP, 0.0), C.clip_oracle(A, rows, None, False, "float32"), C.clip_oracle(A, rows, None, False, "float64"),
                    f"clip A {A} rows {rows}", groups)
    _gate_groups(groups, "clip past cap")
    groups = {}
    _gate_loss_case(_hip_actor(dev, 1, p, -1.0, 0.0), C.surr_oracle(A, rows, -1.0, "float32"), C.surr_oracle(A, rows, -1.0, "float64"),
                    f"surr A {A} rows {rows}", groups)
    _gate_groups(groups, "surr past cap")
    # the KL-penalty oracle is the reference's [rows, rows] broadcast: kept to the 1 025-row case
    if rows <= 2048:
        groups = {}
        o32, o64 = C.klpen_oracle(A, rows, "mid", "float32"), C.klpen_oracle(A, rows, "mid", "float64")
        _gate_klpen_case(_hip_actor(dev, 2, p, p["kl_bound"], C.PG_COEF), o32, o64, f"klpen A {A} rows {rows}", groups, rows)
        hip = _hip_split(dev, p)
        for sfx in ("_kl", "_pg"):
            C.gate_actor_vectors(hip, o32, o64, f"split A {A} rows {rows}", sfx)
        assert hip["sums"][2] == o64["count"]
        _gate_groups(groups, "klpen past cap")


# --------------------------------------------------------------------------------------------------- spo_wide_linesearch_sums
def _hip_linesearch(dev, q, chunks=None, capacity=None):
    lib, ptr, st = _lib()
    rows, A = q["mean_new"].shape
    chunks = chunks or [(0, rows)]
    G = Guarded(dev)
    sums = G.inout(torch.full((3,), 1e30, dtype=torch.float64))
    for k, (lo, hi) in enumerate(chunks):
        t = _up(q, dev, q.keys(), lo, hi)
        blocks = min(-(-(hi - lo) // C.rpb(A)), C.LS_CAP)
        cap = capacity or 3 * blocks
        ws = G.ws(cap)
        _ok(lib.spo_wide_linesearch_sums(ptr(t["mean_new"]), ptr(t["log_std_new"]), ptr(t["act"]), ptr(t["logp_old"]), ptr(t["adv_a"]), ptr(t["adv_b"]),
                                         ptr(t["mean_old"]), ptr(t["log_std_old"]), hi - lo, A, ptr(ws), cap, ptr(sums), 1 if k else 0, st),
            "spo_wide_linesearch_sums")
        G.check(f"spo_wide_linesearch_sums A {A} rows {hi - lo}")
        assert bool(torch.isfinite(ws[:3 * min(blocks, cap // 3)]).all())
    return _host(sums, 3)


def _gate_linesearch(groups, hip, o32, o64):
    for k, nm in enumerate(("sum ratio*adv_a", "sum ratio*adv_b", "sum KL")):
        groups.setdefault(nm, []).append((hip[k], o32["sums"][k], o64["sums"][k], o64["scales"][k]))


@pytest.mark.parametrize("kind", range(5))
def test_linesearch_sums(dev, kind):
    """Row kind 0 .. 4 = 1, rpb - 1, rpb, rpb + 1, 1 000 rows at every act_dim.  At unchanged parameters the KL sum is exactly 0; at
    moved means and a moved log_std all three sums are gated; at 1 000 rows also accumulated over chunks and with partial_capacity =
    3, which clamps the grid to one workgroup.  A sum over a handful of rows carries the rounding of log-probabilities of size
    ~1.4 act_dim under an exp -- one draw of it per case in the float32 oracle as well -- so the scalars of one kind are gated as a
    group over the act_dims (tests/ma_kernel_cases.py::gate_group; tests/test_gpu_ma_kernels.py groups the same way)."""
    groups = {}
    for A in C.ACT_DIMS:
        rows = [1, C.rpb(A) - 1, C.rpb(A), C.rpb(A) + 1, 1000][kind]
        if rows < 1 or (kind and rows == 1):
            continue
        same = _hip_linesearch(dev, C.linesearch_problem(A, rows, False))
        assert same[2] == 0.0, (A, rows, same)
        o32, o64 = C.linesearch_oracle(A, rows, False, "float32"), C.linesearch_oracle(A, rows, False, "float64")
        assert o64["sums"][2] == 0.0
        for k, nm in enumerate(("sum ratio*adv_a", "sum ratio*adv_b")):
            groups.setdefault(nm + " (unchanged)", []).append((same[k], o32["sums"][k], o64["sums"][k], o64["scales"][k]))
        q, o32, o64 = C.linesearch_problem(A, rows, True), C.linesearch_oracle(A, rows, True, "float32"), C.linesearch_oracle(A, rows, True, "float64")
        _gate_linesearch(groups, _hip_linesearch(dev, q), o32, o64)
        if rows == 1000:
            _gate_linesearch(groups, _hip_linesearch(dev, q, [(0, 300), (300, 600), (600, 900), (900, 1000)]), o32, o64)
            _gate_linesearch(groups, _hip_linesearch(dev, q, capacity=3), o32, o64)
    _gate_groups(groups, f"line search row kind {kind}")


@pytest.mark.parametrize("A,rows", C.LS_PAST_CAP)
def test_linesearch_sums_past_the_capped_grid(dev, A, rows):
    groups = {}
    _gate_linesearch(groups, _hip_linesearch(dev, C.linesearch_problem(A, rows, True)), C.linesearch_oracle(A, rows, True, "float32"),
                     C.linesearch_oracle(A, rows, True, "float64"))
    assert _hip_linesearch(dev, C.linesearch_problem(A, rows, False))[2] == 0.0
    _gate_groups(groups, f"line search A {A} rows {rows}")


# -------------------------------------------------------------------------------- spo_wide_ppo_loss, spo_wide_critic_loss
def _hip_critic(dev, rows):
    lib, ptr, st = _lib()
    c = {k: v.to(dev) for k, v in C.critic_problem(rows).items()}
    G = Guarded(dev)
    dvr, dvc, l2, ws = G.out(rows), G.out(rows), G.out(2), G.ws(C.CRITIC_PARTIAL)
    _ok(lib.spo_wide_critic_loss(ptr(c["v_r"]), ptr(c["v_c"]), ptr(c["tgt_r"]), ptr(c["tgt_c"]), rows, ptr(dvr), ptr(dvc), ptr(l2), ptr(ws),
                                 C.CRITIC_PARTIAL, st), "spo_wide_critic_loss")
    G.check(f"spo_wide_critic_loss rows {rows}")
    return {"d_vr": _host(dvr, rows), "d_vc": _host(dvc, rows), "losses": _host(l2, 2)}


def test_critic_loss(dev):
    """One workgroup finishing its own sums (<= 256 rows) against the finish kernel (257), and 65 537 rows past the 256-workgroup cap."""
    groups = {}
    for rows in C.CRITIC_ROWS:
        hip, o32, o64 = _hip_critic(dev, rows), C.critic_oracle(rows, "float32"), C.critic_oracle(rows, "float64")
        for key in ("d_vr", "d_vc"):
            C.gate(hip[key], o32[key], o64[key], f"critic {key} rows {rows}")
        for k in range(2):
            groups.setdefault(f"losses2[{k}]", []).append((hip["losses"][k], o32["losses"][k], o64["losses"][k], o64["losses"][k]))
    _gate_groups(groups, "critic loss")


@pytest.mark.parametrize("A", [16, 17])
def test_ppo_loss_on_both_sides_of_the_kernel_switch(dev, A):
    """act_dim 16: the one-thread-per-row kernel; 17: the critic kernel + the lanes-per-row actor kernel.  The same problem class on
    both; one workgroup finishing its own sums (1, 255, 256 rows) against the finish kernel (257), 65 537 rows past the cap; the
    workspace has exactly the documented size."""
    lib, ptr, st = _lib()
    groups = {}
    for rows in C.PPO_ROWS:
        p, c = C.actor_problem(A, rows), {k: v.to(dev) for k, v in C.critic_problem(rows).items()}
        t, G = _up(p, dev, ACTOR_KEYS), Guarded(dev)
        dvr, dvc, dm, dls, l3, ws = G.out(rows), G.out(rows), G.out(rows * A), G.out(A), G.out(3), G.ws(C.PPO_PARTIAL)
        _ok(lib.spo_wide_ppo_loss(ptr(c["v_r"]), ptr(c["v_c"]), ptr(t["mean"]), ptr(t["log_std"]), ptr(t["act"]), ptr(t["logp_old"]), ptr(t["adv"]),
                                  ptr(c["tgt_r"]), ptr(c["tgt_c"]), rows, A, C.CLIP, ptr(dvr), ptr(dvc), ptr(dm), ptr(dls), ptr(l3), ptr(ws),
                                  C.PPO_PARTIAL, st), "spo_wide_ppo_loss")
        G.check(f"spo_wide_ppo_loss A {A} rows {rows}")
        a32, a64 = C.clip_oracle(A, rows, None, False, "float32"), C.clip_oracle(A, rows, None, False, "float64")
        c32, c64 = C.critic_oracle(rows, "float32"), C.critic_oracle(rows, "float64")
        what = f"ppo loss A {A} rows {rows}"
        C.gate_actor_vectors({"d_mean": _host(dm, rows * A).reshape(rows, A), "d_log_std": _host(dls, A)}, a32, a64, what)
        C.gate(_host(dvr, rows), c32["d_vr"], c64["d_vr"], f"d_vr {what}")
        C.gate(_host(dvc, rows), c32["d_vc"], c64["d_vc"], f"d_vc {what}")
        l = _host(l3, 3)
        for k in range(2):
            groups.setdefault(f"losses3[{k}]", []).append((l[k], c32["losses"][k], c64["losses"][k], c64["losses"][k]))
        groups.setdefault("losses3[2]", []).append((l[2], a32["loss"], a64["loss"], a64["scale"]))
    _gate_groups(groups, f"ppo loss A {A}")


# ----------------------------------------------------------------------------------------------------- spo_wide_fvp_cotangent
@pytest.mark.parametrize("A,rows,rows_total", [(1, 257, 1000), (17, 257, 1000), (64, 257, 257), (64, 16385, 20000)])
def test_fvp_cotangent(dev, A, rows, rows_total):
    """(J t) / sigma^2 / (rows_total * act_dim) with rows_total > rows; 16 385 x 64 elements are past the 4 096-workgroup cap."""
    lib, ptr, st = _lib()
    p, G = C.fvp_problem(A, rows), Guarded(dev)
    jv, ls, dm = p["jv"].to(dev), p["log_std"].to(dev), G.out(rows * A)
    _ok(lib.spo_wide_fvp_cotangent(ptr(jv), ptr(ls), rows, rows_total, A, ptr(dm), st), "spo_wide_fvp_cotangent")
    G.check("spo_wide_fvp_cotangent")
    C.gate(_host(dm, rows * A), C.fvp_oracle(A, rows, rows_total, "float32")["d_mean"], C.fvp_oracle(A, rows, rows_total, "float64")["d_mean"],
           f"fvp cotangent A {A} rows {rows} of {rows_total}")


# ------------------------------------------------------------------------------------------ spo_gauss_sample, spo_gauss_kl_sum
@pytest.mark.parametrize("rows,A", C.SAMPLE_SHAPES)
def test_gauss_sample(dev, rows, A):
    """eps NULL: the action is the mean bit for bit and logp = -sum(log_std + log sqrt(2 pi)); with eps: rsample and its
    log-probability, log_std in +-1.5."""
    lib, ptr, st = _lib()
    p = C.sample_problem(rows, A)
    mean, ls, eps = (p[k].to(dev) for k in ("mean", "log_std", "eps"))
    o32, o64 = C.sample_oracle(rows, A, "float32"), C.sample_oracle(rows, A, "float64")
    G = Guarded(dev)
    act, logp = G.out(rows * A), G.out(rows)
    _ok(lib.spo_gauss_sample(ptr(mean), ptr(ls), None, ptr(act), ptr(logp), rows, A, st), "spo_gauss_sample")
    G.check("spo_gauss_sample deterministic")
    assert torch.equal(act[:rows * A].view(rows, A), mean)
    det_scale = float((p["log_std"].double().abs() + 0.5 * np.log(2 * np.pi)).sum())
    C.gate(_host(logp, rows), o32["logp_det"], o64["logp_det"], f"deterministic logp {rows} x {A}", scale=det_scale)
    G = Guarded(dev)
    act, logp = G.out(rows * A), G.out(rows)
    _ok(lib.spo_gauss_sample(ptr(mean), ptr(ls), ptr(eps), ptr(act), ptr(logp), rows, A, st), "spo_gauss_sample")
    G.check("spo_gauss_sample")
    C.gate(_host(act, rows * A), o32["act"], o64["act"], f"sampled action {rows} x {A}")
    C.gate(_host(logp, rows), o32["logp"], o64["logp"], f"sampled logp {rows} x {A}", scale=o64["logp_scale"])


def test_gauss_kl_sum(dev):
    """Equal distributions give exactly 0; moved ones are gated; accumulate adds to the running sum; 131 073 rows are past the
    512-workgroup cap; partial_capacity = 3 clamps the grid at 1 000 rows."""
    lib, ptr, st = _lib()
    members = []

    def call(rows, A, moved, capacity, sum_in=None, accumulate=0):
        t = {k: v.to(dev) for k, v in C.kl_problem(rows, A, moved).items()}
        G = Guarded(dev)
        s, ws = G.inout(torch.tensor([1e30 if sum_in is None else sum_in], dtype=torch.float64)), G.ws(capacity)
        _ok(lib.spo_gauss_kl_sum(ptr(t["mean_old"]), ptr(t["log_std_old"]), ptr(t["mean_new"]), ptr(t["log_std_new"]), rows, A, ptr(ws), capacity,
                                 ptr(s), accumulate, st), "spo_gauss_kl_sum")
        G.check(f"spo_gauss_kl_sum rows {rows} A {A}")
        return float(s[0])
    for rows, A, moved in C.KL_CASES:
        cap = min(-(-rows // 256), C.KL_CAP) if (rows, A) != (1000, 3) else 3
        got, o32, o64 = call(rows, A, moved, cap), C.kl_oracle(rows, A, moved, "float32"), C.kl_oracle(rows, A, moved, "float64")
        if not moved:
            assert got == 0.0 and o64["sum"] == 0.0
        else:
            members.append((got, o32["sum"], o64["sum"], o64["scale"]))
    o32, o64 = C.kl_oracle(1000, 17, True, "float32"), C.kl_oracle(1000, 17, True, "float64")
    members.append((call(1000, 17, True, 4, sum_in=2.5, accumulate=1) - 2.5, o32["sum"], o64["sum"], o64["scale"]))
    C.gate_group(members, "gauss KL sum")


# ---------------------------------------------------------------------------------------------------- spo_gather_rows / _at
def _gather(dev, widths, n_src, idx, n, cursor=None):
    lib, ptr, st = _lib()
    k = len(widths)
    g = torch.Generator().manual_seed(17 + k + n)
    srcs = [torch.randn(n_src, w, generator=g).to(dev) for w in widths]
    G = Guarded(dev)
    dsts = [G.out(n * w) for w in widths]
    vp = ctypes.c_void_p * k
    idx_d = idx.to(dev)
    cur = None if cursor is None else torch.tensor([cursor], dtype=torch.int64, device=dev)
    args = (k, vp(*[ptr(s) for s in srcs]), (ctypes.c_int * k)(*widths), vp(*[ptr(d) for d in dsts]), ptr(idx_d))
    if cursor is None:
        _ok(lib.spo_gather_rows(*args, n, st), "spo_gather_rows")
    else:
        _ok(lib.spo_gather_rows_at(*args, ptr(cur), n, st), "spo_gather_rows_at")
    G.check(f"spo_gather_rows widths {widths} n {n}")
    window = idx_d[(cursor or 0):(cursor or 0) + n]
    for s, d, w in zip(srcs, dsts, widths):
        assert torch.equal(d[:n * w].view(n, w), s[window]), (widths, n, w)
    assert cur is None or int(cur[0]) == cursor


def test_gather_rows_is_exact(dev):
    """Count 1 and 8, widths 1 / 3 / 376 in one call, repeated indices, 700 rows at width 376 (more than 1 024 x 256 elements: the
    capped grid), the cursor window with a non-zero device cursor; NaN guards behind every destination."""
    g = torch.Generator().manual_seed(3)
    M = 1500
    perm = torch.randperm(M, generator=g)
    _gather(dev, [5], M, perm, 1)
    _gather(dev, [1, 3, 376], M, perm, 257)
    _gather(dev, [1, 3, 376, 17, 2, 1, 64, 8], M, perm, 64)
    _gather(dev, [1, 3, 376], M, torch.randint(0, 9, (300,), generator=g), 300)          # repeated indices
    _gather(dev, [376, 1], M, perm, 700)
    _gather(dev, [1, 3, 376], M, perm, 257, cursor=1000)
    _gather(dev, [376], M, perm, 700, cursor=800)


# ---------------------------------------------------------------------------------- spo_mlp_forward / _backward above 128 rows
def _net(dims):
    from safepo import _abi
    return _abi.MlpNet.of(dims)


def _offset_view(t, dev, misaligned):
    """The tensor on the device, 16-byte aligned, or as a view one float into a buffer (4 bytes past a 16-byte boundary)."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()] if misaligned else buf[:t.numel()]
    v.copy_(t.reshape(-1))
    assert (v.data_ptr() % 16 != 0) == bool(misaligned)
    return v.view(t.shape)


def _hip_mlp(dev, dims, rows, misalign=None, jvp=False, backward=True):
    lib, ptr, st = _lib()
    net, p = _net(dims), C.mlp_problem(tuple(dims), rows)
    theta, x = _offset_view(p["theta"], dev, misalign == "theta"), _offset_view(p["x"], dev, misalign == "x")
    d_out, tangent = p["d_out"].to(dev), p["tangent"].to(dev)
    P = int(lib.spo_mlp_param_count(net))
    assert P == p["theta"].numel()
    G = Guarded(dev)
    ws = G.out(int(lib.spo_mlp_workspace_floats(net, rows)))
    _ok(lib.spo_mlp_forward(ptr(theta), net, ptr(x), rows, ptr(ws), st), "spo_mlp_forward")
    out, o = {"acts": []}, 0
    for d in dims[1:]:
        out["acts"].append(_host(ws[o:o + rows * d]).reshape(rows, d))
        o += rows * d
    if backward:
        grad, scratch = G.out(P), G.ws(int(lib.spo_mlp_backward_scratch_floats(net, rows)), torch.float32)
        _ok(lib.spo_mlp_backward(ptr(theta), net, ptr(x), rows, ptr(ws), ptr(d_out), ptr(grad), ptr(scratch), st), "spo_mlp_backward")
        out["grad"] = _host(grad, P)
    if jvp:
        dout, scratch = G.out(rows * dims[-1]), G.ws(int(lib.spo_mlp_jvp_scratch_floats(net, rows)), torch.float32)
        _ok(lib.spo_mlp_jvp(ptr(theta), net, ptr(tangent), ptr(x), rows, ptr(ws), ptr(dout), ptr(scratch), st), "spo_mlp_jvp")
        out["jvp"] = _host(dout, rows * dims[-1]).reshape(rows, dims[-1])
    G.check(f"mlp {dims} rows {rows}")
    assert torch.equal(theta.cpu(), p["theta"]) and torch.equal(x.cpu(), p["x"])
    return out


@pytest.mark.parametrize("case", C.MLP_CASES, ids=C.mlp_name)
def test_mlp_forward_backward_above_128_rows(dev, case):
    """The GEMM-launch-per-layer path: every layer's activations and the flat gradient per parameter block.  [61, 100, 1] and
    [33, 256, 96, 5] run the 64-tile GEMM (column sums at 129 rows leave trailing slices empty; 257 rows: two weight-gradient
    slices); [20, 1024, 32, 3] at 3 073 rows runs gemm128_kernel in both forms (plain with K = 20, a ragged last chunk; dH with
    tanh' fused) -- with theta one float off alignment its scalar-load branch -- and [18, 1024, 32, 3] (K % 4 != 0) falls back;
    [20, 64, 3] at 2 049 rows: nine weight-gradient slices, the last of one row, in the vector form and (x one float off) the scalar one."""
    dims, rows, misalign = case
    hip = _hip_mlp(dev, dims, rows, misalign)
    o32, o64 = C.mlp_oracle(tuple(dims), rows, "float32"), C.mlp_oracle(tuple(dims), rows, "float64")
    for l, (a, b, c) in enumerate(zip(hip["acts"], o32["acts"], o64["acts"])):
        C.gate(a, b, c, f"mlp {C.mlp_name(case)} activations of layer {l}")
    C.gate_blocks(hip["grad"], o32["grad"], o64["grad"], C.mlp_blocks(dims), f"mlp {C.mlp_name(case)} gradient")


@pytest.mark.parametrize("case", C.JVP_CASES, ids=C.mlp_name)
def test_mlp_jvp_vs_forward_mode_autograd(dev, case):
    """spo_mlp_jvp against torch.func.jvp in float64: one-layer and five-layer networks, 1 / 64 / 129 / 3 073 rows, a tangent whose
    bias entries are non-zero."""
    dims, rows = case
    hip = _hip_mlp(dev, dims, rows, jvp=True, backward=False)
    o32, o64 = C.mlp_oracle(tuple(dims), rows, "float32"), C.mlp_oracle(tuple(dims), rows, "float64")
    C.gate(hip["jvp"], o32["jvp"], o64["jvp"], f"jvp {C.mlp_name(case)}", scale=o64["jvp_scale"])


@pytest.mark.parametrize("wide_at", [None, 1])
def test_mlp_multi_forms_equal_the_single_calls(dev, wide_at):
    """spo_mlp_forward_multi / spo_mlp_backward_multi for 1 to 4 networks: bit for bit the single calls, with every network inside
    the one-launch kernel's envelope and (wide_at) with one network too wide for it -- the per-network fallback."""
    lib, ptr, st = _lib()
    rows = C.MULTI_ROWS
    all_dims = [list(d) for d in C.MULTI_SMALL]
    if wide_at is not None:
        all_dims[wide_at] = list(C.MULTI_WIDE)
    single = []
    for dims in all_dims:
        net, p = _net(dims), C.mlp_problem(tuple(dims), rows)
        t = {k: v.to(dev) for k, v in p.items()}
        ws = torch.full((int(lib.spo_mlp_workspace_floats(net, rows)),), NAN, device=dev)
        grad = torch.full((p["theta"].numel(),), NAN, device=dev)
        scratch = torch.zeros(int(lib.spo_mlp_backward_scratch_floats(net, rows)), device=dev)
        _ok(lib.spo_mlp_forward(ptr(t["theta"]), net, ptr(t["x"]), rows, ptr(ws), st), "spo_mlp_forward")
        _ok(lib.spo_mlp_backward(ptr(t["theta"]), net, ptr(t["x"]), rows, ptr(ws), ptr(t["d_out"]), ptr(grad), ptr(scratch), st), "spo_mlp_backward")
        torch.cuda.synchronize()
        assert bool(torch.isfinite(ws).all()) and bool(torch.isfinite(grad).all())
        single.append((net, t, ws, grad, scratch))
    from safepo import _abi
    for count in range(1, 5):
        if wide_at is not None and count <= wide_at:
            continue
        G = Guarded(dev)
        wss = [G.out(s[2].numel()) for s in single[:count]]
        grads = [G.out(s[3].numel()) for s in single[:count]]
        vp = ctypes.c_void_p * count
        nets = (ctypes.POINTER(_abi.MlpNet) * count)(*[ctypes.pointer(s[0]) for s in single[:count]])
        thetas, xs = vp(*[ptr(s[1]["theta"]) for s in single[:count]]), vp(*[ptr(s[1]["x"]) for s in single[:count]])
        _ok(lib.spo_mlp_forward_multi(count, thetas, nets, xs, rows, vp(*[ptr(w) for w in wss]), st), "spo_mlp_forward_multi")
        _ok(lib.spo_mlp_backward_multi(count, thetas, nets, xs, rows, vp(*[ptr(w) for w in wss]), vp(*[ptr(s[1]["d_out"]) for s in single[:count]]),
                                       vp(*[ptr(g) for g in grads]), vp(*[ptr(s[4]) for s in single[:count]]), st), "spo_mlp_backward_multi")
        G.check(f"mlp multi count {count}")
        for k in range(count):
            assert torch.equal(wss[k][:single[k][2].numel()], single[k][2]), (count, k, "activations")
            assert torch.equal(grads[k][:single[k][3].numel()], single[k][3]), (count, k, "gradient")


# ------------------------------------------------------------------------------------------------------ spo_wide_clip_adam*
def _ppo_cfg(p, A=3):
    from safepo import _abi
    return _abi.PpoCfg(obs_dim=7, act_dim=A, batch=64, use_critic_norm=p["opts"], use_value_coefficient=p["opts"], clip=0.2,
                       max_grad_norm=p["max_norm"], lr_actor=C.ADAM_LR_ACTOR, lr_critic=C.ADAM_LR_CRITIC, beta1=C.BETA1, beta2=C.BETA2,
                       adam_eps=C.ADAM_EPS, l2_coef=C.ADAM_L2)


def _hip_adam(dev, n, name, form, rng="all", layout=None, steps=None, lr_override=(-1.0, -1.0), log=False):
    """One call of spo_wide_clip_adam (form "plain"), _ex, _dev or _dev_log -> every output as float64 numpy; dev forms also pow4
    (before, after) and, with the log, the loss-log rows and the cursor."""
    lib, ptr, st = _lib()
    p = C.adam_problem(n, name, layout)
    r_end, c_end, ab = p["layout"]
    lo, hi, norm0, rest = C.ADAM_RANGES[rng](c_end, ab, n)
    t_c, t_a = steps or (p["t"], p["t"])
    cfg = _ppo_cfg(p)
    b1, b2 = C.BETA1, C.BETA2                                       # the betas as the library's clocks see them: the decimals the caller meant
    G = Guarded(dev)
    th, gr, m, v = (G.inout(p[k]) for k in ("theta", "grad", "m", "v"))
    l3, s4, ws = G.inout(p["losses3"]), G.out(4), G.ws(C.ADAM_PARTIAL)
    head = (ptr(th), ptr(gr), ptr(m), ptr(v), n, r_end, c_end, ab, ctypes.byref(cfg))
    tail = (ptr(l3), ptr(s4), ptr(ws), C.ADAM_PARTIAL)
    out = {}
    if form == "plain":
        assert rng == "all" and t_c == t_a
        _ok(lib.spo_wide_clip_adam(*head, t_c, *tail, st), form)
    elif form == "ex":
        _ok(lib.spo_wide_clip_adam_ex(*head, t_c, t_a, lo, hi, norm0, rest, *tail, st), form)
    else:
        pow4_0 = [b1 ** t_c, b2 ** t_c, b1 ** t_a, b2 ** t_a, lr_override[0], lr_override[1]]
        pow4 = G.inout(torch.tensor(pow4_0, dtype=torch.float64))
        if form == "dev":
            _ok(lib.spo_wide_clip_adam_dev(*head, ptr(pow4), lo, hi, norm0, rest, *tail, st), form)
        else:
            step = 64
            log_buf, cursor = G.ws(3 * 5, torch.float32), G.inout(torch.tensor([3 * step], dtype=torch.int64))
            _ok(lib.spo_wide_clip_adam_dev_log(*head, ptr(pow4), lo, hi, norm0, rest, *tail, ptr(log_buf), ptr(l3), ptr(cursor), step, st), form)
            torch.cuda.synchronize()
            out.update({"log": log_buf[:15].cpu().view(5, 3), "cursor": int(cursor[0]), "cursor_step": step})
        out.update({"pow4_before": np.array(pow4_0), "pow4": _host(pow4, 6), "b": (b1, b2)})
    G.check(f"{form} n {n} {name} {rng}")
    blocks = min(-(-n // 256), 1024)
    assert bool(torch.isfinite(ws[:3 * blocks]).all()) and bool(torch.isnan(ws[3 * blocks:]).all())
    out.update({"theta": _host(th, n), "m": _host(m, n), "v": _host(v, n), "grad": _host(gr, n), "scalars4": _host(s4, 4), "losses3": _host(l3, 3)})
    out["update"] = out["theta"] - p["theta"].double().numpy()
    return out


def _gate_adam_case(dev, n, name, form, scalars, **kw):
    okw = {k: v for k, v in kw.items() if k in ("rng", "layout", "steps")}
    if kw.get("lr_override"):
        okw["lr_override"] = kw["lr_override"]
    args = (n, name)
    o32 = C.adam_oracle(*args, "float32", None, okw.get("rng", "all"), okw.get("layout"), okw.get("steps"), okw.get("lr_override"))
    o64 = C.adam_oracle(*args, "float64", None, okw.get("rng", "all"), okw.get("layout"), okw.get("steps"), okw.get("lr_override"))
    hip = _hip_adam(dev, n, name, form, **{k: v for k, v in kw.items() if k != "lr_override" or v})
    lo, hi, _, _ = o64["range"]
    outside = np.r_[0:lo, hi:n]
    p = C.adam_problem(n, name, kw.get("layout"))
    for key in ("theta", "m", "v"):                                    # outside the Adam range nothing moves
        assert np.array_equal(hip[key][outside], p[key].double().numpy()[outside]), (name, form, key)
    C.gate_adam(hip, o32, o64, n, name, f"{form} n {n} {name} {kw.get('rng', 'all')}", kw.get("layout"), scalars)
    return hip, o64


@pytest.mark.parametrize("n", [3, 700])
def test_clip_adam_every_configuration(dev, n):
    """spo_wide_clip_adam against clip_grad_norm_ + three torch.optim.Adam: clip off / below / 3 x above / 0.05 % over a 1e-3 norm,
    t = 0 and 9 999, fresh optimisers (v = (1 - beta2) g^2 bare), both options on and off; 3 parameters (one per range) and 700."""
    scalars = {}
    for cfg in C.ADAM_CONFIGS:
        hip, o64 = _gate_adam_case(dev, n, C.adam_name(cfg), "plain", scalars)
        assert (hip["scalars4"][0] < 1.0) == (cfg["clip"] in ("above3", "just_over")) == (o64["scalars4"][0] < 1.0)
    _gate_groups(scalars, f"clip + Adam n {n}")


def test_clip_adam_past_the_capped_grid(dev):
    """262 221 parameters: the grid-stride loops and the coefficient kernel's 64-lane sum take several trips."""
    n, scalars = 262144 + 77, {}
    for k in C.ADAM_BIG:
        _gate_adam_case(dev, n, C.adam_name(C.ADAM_CONFIGS[k]), "plain", scalars)
    _gate_groups(scalars, f"clip + Adam n {n}")


@pytest.mark.parametrize("form", ["ex", "dev"])
def test_clip_adam_sub_ranges_and_clocks(dev, form):
    """The critic fit (Adam below the actor, the actor's stale gradient rescaled), CUP's second stage (norm and Adam over the actor
    only; with log_std counted below actor_begin: norm_begin = actor_begin - act_dim) and the full range, with different clocks
    for the critics' and the actor's optimisers."""
    scalars = {}
    for name in ("above3/t0/opts1", "below/t9999/opts1", "off/t0/opts1/fresh"):
        for rng in ("all", "critic_fit", "cup"):
            _gate_adam_case(dev, 700, name, form, scalars, rng=rng, steps=(7, 3))
        _gate_adam_case(dev, 700, name, form, scalars, rng="cup", steps=(7, 3), layout=C.ADAM_LAYOUT_GAP)
    _gate_adam_case(dev, 262144 + 77, "above3/t0/opts1", form, scalars, rng="critic_fit", steps=(7, 3))
    _gate_groups(scalars, f"clip + Adam {form} sub-ranges")


def test_clip_adam_device_clocks_rates_and_log(dev):
    """The device form: pow4[0..3] after the call are beta^(t + 1) (beta: the decimal the cfg's float32 value stands for) to 1e-15 relative for the
    optimisers inside the Adam range and untouched for the others; a learning-rate override of exactly 0 is honoured (theta
    unchanged bit for bit in that range while the moments advance), a negative one takes the cfg's; the loss-log row and the cursor."""
    name, n = "above3/t0/opts1", 700
    for rng, adv_c, adv_a in (("all", 1, 1), ("critic_fit", 1, 0), ("cup", 0, 1)):
        hip = _hip_adam(dev, n, name, "dev", rng=rng, steps=(7, 3))
        b1, b2 = hip["b"]
        want = [b1 ** 8 if adv_c else b1 ** 7, b2 ** 8 if adv_c else b2 ** 7, b1 ** 4 if adv_a else b1 ** 3, b2 ** 4 if adv_a else b2 ** 3]
        assert np.abs(hip["pow4"][:4] / np.array(want) - 1).max() <= 1e-15, (rng, hip["pow4"], want)
        for k, adv in enumerate((adv_c, adv_c, adv_a, adv_a)):
            assert adv or hip["pow4"][k] == hip["pow4_before"][k]
        assert np.array_equal(hip["pow4"][4:], [-1.0, -1.0])
    scalars = {}
    r_end, c_end, ab = C.ADAM_LAYOUTS[n]
    p = C.adam_problem(n, name)
    for over in ((0.0, -1.0), (-1.0, 0.0), (f32v_(1e-2), f32v_(5e-3))):
        hip, _ = _gate_adam_case(dev, n, name, "dev", scalars, steps=(7, 3), lr_override=over)
        frozen = slice(ab, n) if over[0] == 0.0 else slice(0, ab) if over[1] == 0.0 else None
        if frozen is not None:
            assert np.array_equal(hip["theta"][frozen], p["theta"].double().numpy()[frozen])
            assert (hip["m"][frozen] != p["m"].double().numpy()[frozen]).all() and (hip["v"][frozen] != p["v"].double().numpy()[frozen]).all()
        assert np.array_equal(hip["pow4"][4:], list(over))
    hip, _ = _gate_adam_case(dev, n, name, "dev_log", scalars, steps=(7, 3))
    _gate_groups(scalars, "clip + Adam device form")
    log = hip["log"]
    assert hip["cursor"] == 4 * hip["cursor_step"] and bool(torch.isnan(log[[0, 1, 2, 4]]).all())
    assert np.array_equal(log[3].double().numpy(), hip["losses3"])


def f32v_(x):
    return float(np.float32(x))


def test_rows_clip_adam_equals_reduce_parts_then_clip_adam(dev):
    """spo_wide_rows_clip_adam_dev_log fed by one spo_wide_ppo_grad_rows, bit for bit spo_wide_reduce_parts +
    spo_wide_clip_adam_dev_log on a copy of the same state (both Adam kernels take the host-formed weights)."""
    from safepo import _abi
    lib, ptr, st = _lib()
    D, A, hidden, rows = 9, 3, [20], 37
    net_c, net_a = _abi.MlpNet.of([D] + hidden + [1]), _abi.MlpNet.of([D] + hidden + [A])
    if not lib.spo_wide_grad_rows_supported(net_c, net_a, rows):
        pytest.fail("the row-group kernel refuses a 37-row minibatch of [9, 20, .] networks")
    Pc, Pa = int(lib.spo_mlp_param_count(net_c)), int(lib.spo_mlp_param_count(net_a))
    P = 2 * Pc + A + Pa
    g = torch.Generator().manual_seed(23)
    theta = 0.2 * torch.randn(P, generator=g)
    theta[2 * Pc:2 * Pc + A] = -0.5 + 0.1 * torch.randn(A, generator=g)
    state = {"theta": theta, "m": 0.01 * torch.randn(P, generator=g), "v": 1e-4 * torch.rand(P, generator=g)}
    data = {"obs": torch.randn(rows, D, generator=g), "act": torch.randn(rows, A, generator=g), "logp": -0.5 * A + 0.3 * torch.randn(rows, generator=g),
            "tgt_r": torch.randn(rows, generator=g), "tgt_c": torch.randn(rows, generator=g), "adv": torch.randn(rows, generator=g)}
    d = {k: v.to(dev) for k, v in data.items()}
    cfg = _abi.PpoCfg(obs_dim=D, act_dim=A, batch=rows, use_critic_norm=1, use_value_coefficient=1, clip=0.2, max_grad_norm=0.5, lr_actor=3e-4,
                      lr_critic=1e-3, beta1=0.9, beta2=0.999, adam_eps=1e-8, l2_coef=0.001)
    b1, b2 = 0.9, 0.999
    results = []
    for fused in (0, 1):
        G = Guarded(dev)
        th, m, v = (G.inout(state[k]) for k in ("theta", "m", "v"))
        grad, l3, s4, ws = G.out(P), G.out(3), G.out(4), G.ws(C.ADAM_PARTIAL)
        parts = G.ws(int(lib.spo_wide_grad_rows_part_floats(P, rows)), torch.float32)
        pow4 = G.inout(torch.tensor([b1 ** 5, b2 ** 5, b1 ** 5, b2 ** 5, -1.0, -1.0], dtype=torch.float64))
        log_buf, cursor = G.ws(6, torch.float32), G.inout(torch.tensor([rows], dtype=torch.int64))
        _ok(lib.spo_wide_ppo_grad_rows(ptr(th), net_c, net_a, ptr(d["obs"]), ptr(d["act"]), ptr(d["logp"]), ptr(d["tgt_r"]), ptr(d["tgt_c"]),
                                       ptr(d["adv"]), None, None, rows, 0.2, ptr(parts), st), "spo_wide_ppo_grad_rows")
        if fused:
            _ok(lib.spo_wide_rows_clip_adam_dev_log(ptr(parts), rows, ptr(th), ptr(grad), ptr(m), ptr(v), P, Pc, 2 * Pc, 2 * Pc, cfg, ptr(pow4), ptr(l3),
                                                    ptr(s4), ptr(ws), C.ADAM_PARTIAL, ptr(log_buf), ptr(cursor), rows, st), "spo_wide_rows_clip_adam_dev_log")
        else:
            _ok(lib.spo_wide_reduce_parts(ptr(parts), rows, P, 3, ptr(grad), ptr(l3), st), "spo_wide_reduce_parts")
            _ok(lib.spo_wide_clip_adam_dev_log(ptr(th), ptr(grad), ptr(m), ptr(v), P, Pc, 2 * Pc, 2 * Pc, ctypes.byref(cfg), ptr(pow4), 0, P, 0, 0,
                                               ptr(l3), ptr(s4), ptr(ws), C.ADAM_PARTIAL, ptr(log_buf), ptr(l3), ptr(cursor), rows, st),
                "spo_wide_clip_adam_dev_log")
        G.check(f"rows step fused {fused}")
        assert float(s4[0]) < 1.0                                      # the step clips
        results.append({"theta": th[:P].clone(), "m": m[:P].clone(), "v": v[:P].clone(), "grad": grad[:P].clone(), "l3": l3[:3].clone(),
                        "s4": s4[:4].clone(), "pow4": pow4[:6].clone(), "log": log_buf[3:6].clone(), "cursor": cursor[:1].clone()})
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), k
    assert not torch.equal(results[0]["theta"].cpu(), theta)


# ------------------------------------------------------------------------------------------------------------------ refusals
def _refused(rc, G, what):
    lib, _, _ = _lib()
    assert rc != 0, f"{what}: accepted"
    msg = lib.spo_last_error()
    assert msg and len(msg) > 0, f"{what}: no message"
    G.untouched(what)


def test_refusals_leave_outputs_untouched(dev):
    """Every entry point refuses act_dim 0 and 65, mode 3, a chunked or accumulating mode 2, a workspace one double too small, null
    pointers, gather count 9 and width 0, ranges out of order, n_layers 0 and 6 and betas outside [0, 1): non-zero, a message in
    spo_last_error, NaN-primed outputs untouched."""
    from safepo import _abi
    lib, ptr, st = _lib()
    A, rows = 17, 40
    p = C.actor_problem(A, rows)
    t = _up(p, dev, ACTOR_KEYS)
    inp = [ptr(t[k]) for k in ACTOR_KEYS]

    def fresh():
        G = Guarded(dev)
        return G, [G.ws(n, torch.float32) for n in (rows * A, rows * A, A, A, 8, rows, rows, 3)], G.ws(C.SPLIT_PARTIAL), G.ws(2 + A)
    # spo_wide_actor_loss
    for what, kw in (("act_dim 0", dict(A=0)), ("act_dim 65", dict(A=65)), ("mode 3", dict(mode=3)), ("mode 2 chunked", dict(mode=2, total=rows + 1)),
                     ("mode 2 accumulating", dict(mode=2, acc=1)), ("workspace too small", dict(cap=-(-rows // C.rpb(A)) * (2 + C.MAX_ACT) - 1)),
                     ("null mean", dict(null=0)), ("null sums", dict(null_sums=1)), ("mode 2 without old_mean", dict(mode=2, null=5)), ("rows 0", dict(rows=0))):
        G, (dm, _, dls, _, _, _, _, loss), ws, sums = fresh()
        a = list(inp)
        if "null" in kw:
            a[kw["null"]] = None
        rc = lib.spo_wide_actor_loss(kw.get("mode", 0), *a, kw.get("rows", rows), kw.get("total", rows), kw.get("A", A), C.CLIP, 0.0, ptr(dm),
                                     None if kw.get("null_sums") else ptr(sums), kw.get("acc", 0), ptr(loss), ptr(dls), ptr(ws), kw.get("cap", C.ACTOR_PARTIAL), st)
        _refused(rc, G, f"spo_wide_actor_loss {what}")
    # spo_wide_kl_penalty_split / _combine
    for what, kw in (("act_dim 0", dict(A=0)), ("act_dim 65", dict(A=65)), ("workspace too small", dict(cap=-(-rows // C.rpb(A)) * (3 + 2 * C.MAX_ACT) - 1)),
                     ("null old_std", dict(null=6)), ("rows 0", dict(rows=0))):
        G, (dk, dp, lk, lp, sums, _, _, _), ws, _ = fresh()
        a = list(inp)
        if "null" in kw:
            a[kw["null"]] = None
        rc = lib.spo_wide_kl_penalty_split(*a, kw.get("rows", rows), kw.get("A", A), 0.02, C.PG_COEF, ptr(dk), ptr(dp), ptr(lk), ptr(lp), ptr(sums), ptr(ws),
                                           kw.get("cap", C.SPLIT_PARTIAL), st)
        _refused(rc, G, f"spo_wide_kl_penalty_split {what}")
    for what, (n, begin, ab, null) in (("begin past actor_begin", (100, 50, 40, 0)), ("actor_begin == n_params", (100, 0, 100, 0)), ("negative begin", (100, -1, 40, 0)),
                                       ("null sums", (100, 0, 40, 1))):
        G = Guarded(dev)
        g, pg, loss = G.ws(100, torch.float32), G.ws(100, torch.float32), G.ws(1, torch.float32)
        rc = lib.spo_wide_kl_penalty_combine(ptr(g), ptr(pg), None if null else ptr(t["adv"]), n, begin, ab, 1.0, C.PG_COEF, ptr(loss), st)
        _refused(rc, G, f"spo_wide_kl_penalty_combine {what}")
    # spo_wide_linesearch_sums, spo_wide_ppo_loss, spo_wide_critic_loss, spo_wide_fvp_cotangent, spo_gauss_sample, spo_gauss_kl_sum
    ls_in = [ptr(t["mean"]), ptr(t["log_std"]), ptr(t["act"]), ptr(t["logp_old"]), ptr(t["adv"]), ptr(t["adv"]), ptr(t["mean"]), ptr(t["log_std"])]
    for what, kw in (("act_dim 0", dict(A=0)), ("act_dim 65", dict(A=65)), ("capacity 2", dict(cap=2)), ("null act", dict(null=2)), ("rows 0", dict(rows=0))):
        G = Guarded(dev)
        ws, s3 = G.ws(64), G.ws(3)
        a = list(ls_in)
        if "null" in kw:
            a[kw["null"]] = None
        _refused(lib.spo_wide_linesearch_sums(*a, kw.get("rows", rows), kw.get("A", A), ptr(ws), kw.get("cap", 64), ptr(s3), 0, st), G, f"spo_wide_linesearch_sums {what}")
    c = {k: v.to(dev) for k, v in C.critic_problem(rows).items()}
    for what, kw in (("act_dim 0", dict(A=0)), ("act_dim 65", dict(A=65)), ("workspace too small", dict(cap=256 * (2 + C.MAX_ACT) + 512 + 2 + C.MAX_ACT - 1)),
                     ("workspace too small at act_dim 16", dict(A=16, cap=18)), ("null adv", dict(null=1)), ("rows 0", dict(rows=0))):
        G, (dm, _, dls, _, _, dvr, dvc, l3), ws, _ = fresh()
        rc = lib.spo_wide_ppo_loss(ptr(c["v_r"]), ptr(c["v_c"]), ptr(t["mean"]), ptr(t["log_std"]), ptr(t["act"]), ptr(t["logp_old"]),
                                   None if kw.get("null") else ptr(t["adv"]), ptr(c["tgt_r"]), ptr(c["tgt_c"]), kw.get("rows", rows), kw.get("A", A), C.CLIP,
                                   ptr(dvr), ptr(dvc), ptr(dm), ptr(dls), ptr(l3), ptr(ws), kw.get("cap", C.PPO_PARTIAL), st)
        _refused(rc, G, f"spo_wide_ppo_loss {what}")
    for what, kw in (("workspace too small", dict(cap=1)), ("null target", dict(null=1)), ("rows 0", dict(rows=0))):
        G, (_, _, _, _, _, dvr, dvc, l3), ws, _ = fresh()
        rc = lib.spo_wide_critic_loss(ptr(c["v_r"]), ptr(c["v_c"]), None if kw.get("null") else ptr(c["tgt_r"]), ptr(c["tgt_c"]), kw.get("rows", rows), ptr(dvr),
                                      ptr(dvc), ptr(l3), ptr(ws), kw.get("cap", C.CRITIC_PARTIAL), st)
        _refused(rc, G, f"spo_wide_critic_loss {what}")
    for what, kw in (("act_dim 0", dict(A=0)), ("act_dim 65", dict(A=65)), ("rows_total < rows", dict(total=rows - 1)), ("null jv", dict(null=1))):
        G, (dm, *_), _, _ = fresh()
        rc = lib.spo_wide_fvp_cotangent(None if kw.get("null") else ptr(t["mean"]), ptr(t["log_std"]), rows, kw.get("total", rows), kw.get("A", A), ptr(dm), st)
        _refused(rc, G, f"spo_wide_fvp_cotangent {what}")
    for what, kw in (("act_dim 0", dict(A=0)), ("act_dim 65", dict(A=65)), ("null log_std", dict(null=1)), ("rows 0", dict(rows=0))):
        G, (act, *_, logp, _, _), _, _ = fresh()
        rc = lib.spo_gauss_sample(ptr(t["mean"]), None if kw.get("null") else ptr(t["log_std"]), ptr(t["act"]), ptr(act), ptr(logp), kw.get("rows", rows),
                                  kw.get("A", A), st)
        _refused(rc, G, f"spo_gauss_sample {what}")
        G = Guarded(dev)
        ws, s1 = G.ws(8), G.ws(1)
        rc = lib.spo_gauss_kl_sum(ptr(t["mean"]), None if kw.get("null") else ptr(t["log_std"]), ptr(t["mean"]), ptr(t["log_std"]), kw.get("rows", rows),
                                  kw.get("A", A), ptr(ws), 8, ptr(s1), 0, st)
        _refused(rc, G, f"spo_gauss_kl_sum {what}")
    G = Guarded(dev)
    ws, s1 = G.ws(8), G.ws(1)
    _refused(lib.spo_gauss_kl_sum(ptr(t["mean"]), ptr(t["log_std"]), ptr(t["mean"]), ptr(t["log_std"]), rows, A, ptr(ws), 0, ptr(s1), 0, st), G,
             "spo_gauss_kl_sum capacity 0")
    # spo_gather_rows / _at
    idx = torch.arange(rows, device=dev)
    for what, count, widths, null in (("count 9", 9, [1] * 9, False), ("count 0", 0, [1], False), ("width 0", 2, [3, 0], False), ("null source", 2, [3, 1], True)):
        G = Guarded(dev)
        k = len(widths)
        dsts = [G.ws(rows * max(w, 1), torch.float32) for w in widths]
        vp = ctypes.c_void_p * k
        srcs = vp(*[None if (null and j == 1) else ptr(t["mean"]) for j in range(k)])
        rc = lib.spo_gather_rows(count, srcs, (ctypes.c_int * k)(*widths), vp(*[ptr(d) for d in dsts]), ptr(idx), rows, st)
        _refused(rc, G, f"spo_gather_rows {what}")
        rc = lib.spo_gather_rows_at(count, srcs, (ctypes.c_int * k)(*widths), vp(*[ptr(d) for d in dsts]), ptr(idx), None, rows, st)
        _refused(rc, G, f"spo_gather_rows_at {what}")
    # the MLP entry points: n_layers 0 and 6, a zero width, null pointers
    dims = [7, 20, 3]
    mp = {k: v.to(dev) for k, v in C.mlp_problem(tuple(dims), rows).items()}
    good = _abi.MlpNet.of(dims)
    bad_nets = [("n_layers 0", _abi.MlpNet(0, (ctypes.c_int32 * 6)(7, 0, 0, 0, 0, 0))), ("n_layers 6", _abi.MlpNet(6, (ctypes.c_int32 * 6)(7, 8, 8, 8, 8, 8))),
                ("a zero width", _abi.MlpNet(2, (ctypes.c_int32 * 6)(7, 0, 3, 0, 0, 0)))]
    for what, net in bad_nets:
        assert lib.spo_mlp_param_count(net) == -1 and lib.spo_mlp_workspace_floats(net, rows) == -1 and lib.spo_mlp_backward_scratch_floats(net, rows) == -1
        assert lib.spo_mlp_jvp_scratch_floats(net, rows) == -1
    for what, net, null in [(w, nt, False) for w, nt in bad_nets] + [("null x", good, True)]:
        G = Guarded(dev)
        ws, grad, scratch, dout = G.ws(rows * 23, torch.float32), G.ws(mp["theta"].numel(), torch.float32), G.ws(4096, torch.float32), G.ws(rows * 3, torch.float32)
        x = None if null else ptr(mp["x"])
        _refused(lib.spo_mlp_forward(ptr(mp["theta"]), net, x, rows, ptr(ws), st), G, f"spo_mlp_forward {what}")
        _refused(lib.spo_mlp_backward(ptr(mp["theta"]), net, x, rows, ptr(mp["x"]), ptr(mp["d_out"]), ptr(grad), ptr(scratch), st), G, f"spo_mlp_backward {what}")
        _refused(lib.spo_mlp_jvp(ptr(mp["theta"]), net, ptr(mp["tangent"]), x, rows, ptr(mp["x"]), ptr(dout), ptr(scratch), st), G, f"spo_mlp_jvp {what}")
        vp = ctypes.c_void_p * 1
        nets = (ctypes.POINTER(_abi.MlpNet) * 1)(ctypes.pointer(net))
        _refused(lib.spo_mlp_forward_multi(1, vp(ptr(mp["theta"])), nets, vp(x), rows, vp(ptr(ws)), st), G, f"spo_mlp_forward_multi {what}")
        _refused(lib.spo_mlp_backward_multi(1, vp(ptr(mp["theta"])), nets, vp(x), rows, vp(ptr(mp["x"])), vp(ptr(mp["d_out"])), vp(ptr(grad)), vp(ptr(scratch)), st),
                 G, f"spo_mlp_backward_multi {what}")
    vp = ctypes.c_void_p * 5
    nets5 = (ctypes.POINTER(_abi.MlpNet) * 5)(*[ctypes.pointer(good)] * 5)
    G = Guarded(dev)
    ws = G.ws(rows * 23, torch.float32)
    _refused(lib.spo_mlp_forward_multi(5, vp(*[ptr(mp["theta"])] * 5), nets5, vp(*[ptr(mp["x"])] * 5), rows, vp(*[ptr(ws)] * 5), st), G, "spo_mlp_forward_multi count 5")
    # the four clip + Adam entries and the fused one
    n, name = 700, "above3/t0/opts1"
    ap = C.adam_problem(n, name)
    for what, kw in (("ranges out of order", dict(layout=(400, 200, 400))), ("actor_begin past n_params", dict(layout=(200, 400, 701))),
                     ("optimiser range out of order", dict(adam=(500, 400))), ("adam_end past n_params", dict(adam=(0, 701))), ("norm_begin negative", dict(norm0=-1)),
                     ("workspace too small", dict(cap=8)), ("null theta", dict(null=1)), ("n_params 0", dict(n=0)), ("beta2 = 1", dict(beta2=1.0)),
                     ("beta1 negative", dict(beta1=-0.1)), ("negative step", dict(step=-1))):
        for form in ("plain", "ex", "dev", "dev_log"):
            if form == "plain" and ("adam" in kw or "norm0" in kw):
                continue
            if form in ("dev", "dev_log") and "step" in kw:
                continue
            G = Guarded(dev)
            th, gr, m, v = (G.ws(n, torch.float32) for _ in range(4))
            l3, s4, ws, pow4 = G.ws(3, torch.float32), G.ws(4, torch.float32), G.ws(C.ADAM_PARTIAL), G.ws(6)
            log_buf, cursor = G.ws(15, torch.float32), G.ws(1, torch.float32)
            cfg = _ppo_cfg(ap)
            cfg.beta1, cfg.beta2 = kw.get("beta1", C.BETA1), kw.get("beta2", C.BETA2)
            r_end, c_end, ab = kw.get("layout", ap["layout"])
            lo, hi = kw.get("adam", (0, n))
            head = (None if kw.get("null") else ptr(th), ptr(gr), ptr(m), ptr(v), kw.get("n", n), r_end, c_end, ab, ctypes.byref(cfg))
            tail = (ptr(l3), ptr(s4), ptr(ws), kw.get("cap", C.ADAM_PARTIAL))
            t0 = kw.get("step", 0)
            if form == "plain":
                rc = lib.spo_wide_clip_adam(*head, t0, *tail, st)
            elif form == "ex":
                rc = lib.spo_wide_clip_adam_ex(*head, t0, 0, lo, hi, kw.get("norm0", 0), 0, *tail, st)
            elif form == "dev":
                rc = lib.spo_wide_clip_adam_dev(*head, ptr(pow4), lo, hi, kw.get("norm0", 0), 0, *tail, st)
            else:
                rc = lib.spo_wide_clip_adam_dev_log(*head, ptr(pow4), lo, hi, kw.get("norm0", 0), 0, *tail, ptr(log_buf), ptr(l3), None, 0, st)
            _refused(rc, G, f"spo_wide_clip_adam {form} {what}")
    for form in ("dev", "dev_log"):                                    # no clocks; a cursor without a step
        G = Guarded(dev)
        th, gr, m, v = (G.ws(n, torch.float32) for _ in range(4))
        l3, s4, ws, pow4, cursor = G.ws(3, torch.float32), G.ws(4, torch.float32), G.ws(C.ADAM_PARTIAL), G.ws(6), G.ws(1)
        cfg = _ppo_cfg(ap)
        head = (ptr(th), ptr(gr), ptr(m), ptr(v), n, *ap["layout"], ctypes.byref(cfg))
        tail = (ptr(l3), ptr(s4), ptr(ws), C.ADAM_PARTIAL)
        if form == "dev":
            rc = lib.spo_wide_clip_adam_dev(*head, None, 0, n, 0, 0, *tail, st)
        else:
            rc = lib.spo_wide_clip_adam_dev_log(*head, ptr(pow4), 0, n, 0, 0, *tail, None, None, ptr(cursor), 0, st)
        _refused(rc, G, f"spo_wide_clip_adam {form} without clocks / cursor step")
    for what, kw in (("ranges out of order", dict(layout=(400, 200, 400))), ("workspace too small", dict(cap=8)), ("beta2 = 1", dict(beta2=1.0)),
                     ("null parts", dict(null=1)), ("rows 0", dict(rows=0)), ("rows 257", dict(rows=257))):
        G = Guarded(dev)
        th, gr, m, v, parts = (G.ws(n, torch.float32) for _ in range(5))
        l3, s4, ws, pow4 = G.ws(3, torch.float32), G.ws(4, torch.float32), G.ws(C.ADAM_PARTIAL), G.ws(6)
        cfg = _ppo_cfg(ap)
        cfg.beta2 = kw.get("beta2", C.BETA2)
        rc = lib.spo_wide_rows_clip_adam_dev_log(None if kw.get("null") else ptr(parts), kw.get("rows", 16), ptr(th), ptr(gr), ptr(m), ptr(v), n,
                                                 *kw.get("layout", ap["layout"]), cfg, ptr(pow4), ptr(l3), ptr(s4), ptr(ws), kw.get("cap", C.ADAM_PARTIAL), None, None, 0, st)
        _refused(rc, G, f"spo_wide_rows_clip_adam_dev_log {what}")
