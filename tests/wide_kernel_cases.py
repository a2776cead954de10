"""The cases of tests/test_gpu_wide_kernels.py (no test in here): the wide-network kernels of csrc/wide.hip, the GEMMs of
csrc/gemm_f32.hip they call and the optimiser pass of csrc/mlp_rows.hip, reached by direct ABI calls.  Here are the case tables,
every problem built on the CPU from seeds, each operation in plain torch (autograd, torch.distributions, clip_grad_norm_,
torch.optim.Adam, torch.func.jvp) in float32 -- the yardstick -- and float64 -- the reference --, and the gates.
tests/test_wide_kernel_cases_host.py checks on the CPU that the problems keep the gates meaningful and that the gates refuse
deliberately wrong oracles (the `variant` argument of the oracles).

Discontinuities: the clipped surrogate at ratio = 1 +- clip, the sign of the advantage, the KL indicator at kl = kl_bound.  Every
problem is drawn in float32, its decision quantities are evaluated in float64, and every row within MARGIN (relative) of a
boundary is drawn again -- the whole row -- until none is left, so the float32 and the float64 oracle (and a correct kernel) take
the same branch in every row.  One tie on purpose: rows with adv == 0 (`tie`), where both surrogates are equal and the gradient
is exactly zero.

Every oracle result is computed once per process (functools.lru_cache) and shared; callers do not modify what they get.  The
oracles run on fp64_gate.ORACLE_THREADS torch threads whatever the host offers and put the count back."""
import functools
import os

import numpy as np
import torch

from ma_kernel_cases import _redraw_until_clear, _seed, f32v, MARGIN, MIN_SHARE  # noqa: F401  (sets sys.path)
import fp64_gate as G

Normal = torch.distributions.Normal
kl_divergence = torch.distributions.kl_divergence
n64 = lambda x: x.detach().double().numpy().copy()

# ---- launch arithmetic of the actor-side loss kernels: G = pow2ceil(act_dim) lanes per row, 4 waves of 64 / G rows per workgroup
MAX_ACT, PPO_ROW_KERNEL_MAX_ACT = 64, 16                          # SPO_WIDE_MAX_ACT; SPO_MAX_ACT (spo_wide_ppo_loss's one-thread-per-row kernel)
ACT_DIMS = [1, 2, 3, 16, 17, 33, 64]
LOSS_CAP, LS_CAP, KL_CAP = 256, 512, 512                          # workgroup caps: losses, line search, spo_gauss_kl_sum


def pow2ceil(a):
    g = 1
    while g < a:
        g <<= 1
    return g


def rpb(A):
    return 4 * (64 // pow2ceil(A))


def actor_rows(A):
    return sorted({1, rpb(A) - 1, rpb(A), rpb(A) + 1, 1000} - {0})


LOSS_PAST_CAP = [(64, LOSS_CAP * rpb(64) + 1), (1, LOSS_CAP * rpb(1) + 1)]      # (act_dim, rows): 1 025 and 65 537
LS_PAST_CAP = [(64, LS_CAP * rpb(64) + 1), (1, LS_CAP * rpb(1) + 1)]            # 2 049 and 131 073
ACTOR_PARTIAL = LOSS_CAP * (2 + MAX_ACT)                          # documented partial_ws sizes, in doubles (include/safepo_hip.h)
SPLIT_PARTIAL = LOSS_CAP * (3 + 2 * MAX_ACT)
PPO_PARTIAL = LOSS_CAP * (3 + MAX_ACT) + 512
CRITIC_PARTIAL = 512
ADAM_PARTIAL = 3 * 1024
CLIP = f32v(0.2)
LOG_RATIO_STD = 0.46                                              # P(|N(0, 0.46)| < 0.2) ~ 1/3: a third of the ratios in each region
CLASSES = [(r, s) for r in ("below", "inside", "above") for s in (1.0, -1.0)]
LOG_RATIO = {"below": (-0.7, -0.3), "inside": (-0.15, 0.15), "above": (0.25, 0.7)}
PG_COEF = f32v(1.0 / 1.5)                                         # FOCOPS: 1 / lam
KL_HALF_WIDTH = 0.02                                              # the rows' KL is uniform within +- this of the bound ("mid")
PPO_ROWS = [1, 255, 256, 257, 65537]
CRITIC_ROWS = [1, 256, 257, 65537]


# ------------------------------------------------------------------------------------------------------------------- problems
def _logp(mean, std, act):
    return Normal(mean, std).log_prob(act).sum(-1)


def _logp_of(mean, ls_rows, act, variant=None):
    if variant == "minus_one_dropped":                                # log_prob whose - log(std) term is a constant: d(log_std) loses its - 1
        return (-((act - mean) ** 2) / (2 * torch.exp(ls_rows) ** 2) - ls_rows.detach() - 0.5 * float(np.log(2 * np.pi))).sum(-1)
    return _logp(mean, torch.exp(ls_rows), act)


def actor_decisions(p, dtype=torch.float64):
    """region -1 / 0 / +1 (ratio below / inside, bounds inclusive / above the clip range), sign of adv, the KL indicator at the
    problem's kl_bound, the KL itself, and `near` [rows]: within MARGIN of a discontinuity (adv == 0 exactly is the tie, not near)."""
    t = {k: v.to(dtype) for k, v in p.items() if torch.is_tensor(v) and v.is_floating_point()}
    std = torch.exp(t["log_std"])
    ratio = torch.exp(_logp(t["mean"], std, t["act"]) - t["logp_old"])
    lo, hi = 1.0 - CLIP, 1.0 + CLIP
    region = (ratio > hi).long() - (ratio < lo).long()
    kl = kl_divergence(Normal(t["mean"], std), Normal(t["old_mean"], t["old_std"])).sum(-1)
    bound = p["kl_bound"]
    near = ((ratio - lo).abs() <= MARGIN * lo) | ((ratio - hi).abs() <= MARGIN * hi) | ((t["adv"].abs() <= MARGIN) & (t["adv"] != 0))
    near = near | ((t["adv_b"].abs() <= MARGIN) & (t["adv_b"] != 0))
    if np.isfinite(bound):
        near = near | ((kl - bound).abs() <= MARGIN * bound)
    return region, torch.sign(t["adv"]), (kl <= bound), kl, near


@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def actor_problem(A, rows, cls=None, tie=False, bound="mid"):
    """float32 inputs of every actor-side loss kernel on ONE draw: mean, log_std, act, adv (adv_b: the line search's second
    advantage), logp_old = the float64 log-probability of the actions minus a log ratio ~ N(0, LOG_RATIO_STD), rounded once (cls =
    (region, sign): the log ratio inside LOG_RATIO[region], the advantage of that sign); the old distribution of the KL-penalty
    loss: old_std = exp(log_std + N(0, 0.05)) (so var_ratio != 1) and old_mean such that KL(new || old) is uniform within
    +- KL_HALF_WIDTH of kl_bound ("mid"; "inf": +inf, CUP; "none": half the smallest KL, no row inside).  tie: every seventh row
    has adv == 0."""
    g = torch.Generator().manual_seed(_seed("wide-actor", A, rows, str(cls), int(tie), bound))
    log_std = (0.5 * torch.randn(A, generator=g)).clamp(-1.0, 1.0)
    std64 = torch.exp(log_std.double())
    old_std = torch.exp(log_std.double() + 0.05 * torch.randn(A, generator=g).double()).float()
    vrat = (std64 / old_std.double()) ** 2
    c0 = float((0.5 * (vrat - 1 - torch.log(vrat))).sum())
    kl_mid = f32v(c0 + 1.5 * KL_HALF_WIDTH)

    def draw(n):
        r = lambda *s: torch.randn(*s, generator=g)
        mean = 0.5 * r(n, A)
        act = (mean.double() + std64 * r(n, A).double()).float()
        if cls is None:
            lr, adv = LOG_RATIO_STD * r(n).double(), r(n)
        else:
            lo, hi = LOG_RATIO[cls[0]]
            lr = lo + (hi - lo) * torch.rand(n, generator=g).double()
            adv = cls[1] * (0.2 + r(n).abs())
        logp_old = (_logp(mean.double(), std64, act.double()) - lr).float()
        z = r(n, A).double()
        u = 0.5 * KL_HALF_WIDTH + 2 * KL_HALF_WIDTH * torch.rand(n, 1, generator=g).double()      # 0.5 sum dm^2 in [0.5, 2.5] half widths
        dm = torch.sqrt(2 * u) * z / z.norm(dim=-1, keepdim=True)
        old_mean = (mean.double() - dm * old_std.double()).float()
        return {"mean": mean, "act": act, "logp_old": logp_old, "adv": adv, "adv_b": 0.5 * r(n) + 0.1, "old_mean": old_mean}

    fixed = {"log_std": log_std, "old_std": old_std, "kl_bound": kl_mid}

    def bad_rows(p):
        region, sign, ind, kl, near = actor_decisions(dict(p, **fixed))
        if cls is not None:
            near = near | (region != {"below": -1, "inside": 0, "above": 1}[cls[0]]) | (sign != cls[1])
        return near
    p, again = _redraw_until_clear(draw, bad_rows, rows, f"wide actor {A} {rows} {cls}")
    p.update(fixed)
    if tie:
        p["adv"][::7] = 0.0
    if bound != "mid":
        kl = actor_decisions(p)[3]
        p["kl_bound"] = float("inf") if bound == "inf" else f32v(0.5 * float(kl.min()))
    p["drawn_again"] = again
    return p


def actor_populations(A, rows, cls=None, tie=False, bound="mid"):
    p = actor_problem(A, rows, cls, tie, bound)
    r64, s64, i64, _, near = actor_decisions(p)
    r32, s32, i32, _, _ = actor_decisions(p, torch.float32)
    share = lambda m: float(m.double().mean())
    out = {f"{nm}/{'+' if s > 0 else '-'}": share((r64 == k) & (s64 == s)) for nm, k in (("below", -1), ("inside", 0), ("above", 1)) for s in (1.0, -1.0)}
    out.update({"kl_in": share(i64), "kl_out": share(~i64), "near": int(near.sum()), "ties": int((p["adv"] == 0).sum()),
                "same_branch": bool(torch.equal(r32, r64) and torch.equal(s32.double(), s64) and torch.equal(i32, i64))})
    return out


def _leaves(p, dtype, rows_total=None):
    t = {k: v.to(dtype) for k, v in p.items() if torch.is_tensor(v)}
    rows, A = t["mean"].shape
    mean = t["mean"].clone().requires_grad_(True)
    ls_rows = t["log_std"].expand(rows, A).clone().requires_grad_(True)      # a per-row copy: its gradient's rows are the summed terms
    return t, mean, ls_rows, rows, A


def _grads(loss, mean, ls_rows):
    gm, gl = torch.autograd.grad(loss, (mean, ls_rows), allow_unused=True, retain_graph=True)
    gm = torch.zeros_like(mean) if gm is None else gm
    gl = torch.zeros_like(ls_rows) if gl is None else gl
    return n64(gm), n64(gl.sum(0)), n64(gl.abs().sum(0))


# ------------------------------------------------------------------------------------------- spo_wide_actor_loss, mode 0 and 1
@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def clip_oracle(A, rows, cls, tie, dtype_name, variant=None, rows_total=None):
    """-mean(min(ratio * adv, clamp(ratio, 1 - clip, 1 + clip) * adv)) (ppo_lag.py:316-319) over rows_total rows (the problem's
    own when None) -> d_mean, d_log_std (+ the sum of its absolute per-row terms), term_sum = sum of the min terms, loss,
    scale = mean |adv|."""
    t, mean, ls_rows, rows, _ = _leaves(actor_problem(A, rows, cls, tie), getattr(torch, dtype_name))
    n = rows_total or rows
    ratio = torch.exp(_logp_of(mean, ls_rows, t["act"], variant) - t["logp_old"])
    if variant == "exclusive_clip":                                   # bounds exclusive: rows ON a bound lose their gradient (none are)
        rc = torch.where((ratio > 1 - CLIP) & (ratio < 1 + CLIP), ratio, ratio.detach().clamp(1 - CLIP, 1 + CLIP))
    else:
        rc = torch.clamp(ratio, 1 - CLIP, 1 + CLIP)
    if variant == "clip_ignores_sign":                                # the pessimistic min replaced by the clipped term
        terms = rc * t["adv"]
    else:
        terms = torch.min(ratio * t["adv"], rc * t["adv"])
    loss = -terms.sum() / n
    dm, dl, dl_abs = _grads(loss, mean, ls_rows)
    return {"d_mean": dm, "d_log_std": dl, "d_log_std_scale": dl_abs, "term_sum": float(terms.sum().detach()), "loss": float(loss.detach()),
            "scale": float(t["adv"].abs().sum() / n), "rows_total": n}


@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def surr_oracle(A, rows, sign, dtype_name, variant=None):
    """sign * mean(ratio * adv) (cpo.py:356-381) -> as clip_oracle; term_sum = sum ratio * adv, loss = its plain mean (what the
    kernel's loss_out holds: the caller applies the sign)."""
    t, mean, ls_rows, rows, _ = _leaves(actor_problem(A, rows), getattr(torch, dtype_name))
    ratio = torch.exp(_logp_of(mean, ls_rows, t["act"], variant) - t["logp_old"])
    terms = ratio * t["adv"]
    loss = sign * terms.mean()
    dm, dl, dl_abs = _grads(loss, mean, ls_rows)
    return {"d_mean": dm, "d_log_std": dl, "d_log_std_scale": dl_abs, "term_sum": float(terms.sum().detach()),
            "loss": float(terms.mean().detach()), "scale": float(t["adv"].abs().mean()), "rows_total": rows}


# ------------------------------------------------------------- spo_wide_actor_loss mode 2, spo_wide_kl_penalty_split / _combine
@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def klpen_oracle(A, rows, bound, dtype_name, variant=None, pg_coef=PG_COEF):
    """The KL-penalty loss of FOCOPS / CUP's second stage as the reference writes it (focops.py:326-333): temp_kl [rows, 1] and
    ratio * adv [rows] broadcast to [rows, rows], so the loss is mean(ind * kl) - pg_coef * mean(ind) * mean(ratio * adv).  ->
    the whole loss and its gradients (mode 2), and the split form's parts: the gradients of mean(ind * kl) and of
    -pg_coef * mean(ratio * adv) (F taken as 1), count = sum ind, kl_sum = sum ind * kl, ra_sum = sum ratio * adv."""
    dtype = getattr(torch, dtype_name)
    p = actor_problem(A, rows, None, False, bound)
    t, mean, ls_rows, rows, _ = _leaves(p, dtype)
    std = torch.exp(ls_rows)
    ratio = torch.exp(_logp_of(mean, ls_rows, t["act"], variant) - t["logp_old"])
    new, old = Normal(mean, std), Normal(t["old_mean"], t["old_std"].expand(rows, A))
    kl = (kl_divergence(old, new) if variant == "kl_swapped" else kl_divergence(new, old)).sum(-1, keepdim=True)
    ind = (kl.detach() <= p["kl_bound"]).to(dtype)
    ra = ratio * t["adv"]
    if variant == "F_is_one":                                         # per-row indicator on the policy-gradient term too ... with F = 1
        loss = (ind * kl).mean() - pg_coef * ra.mean()
    else:
        loss = ((kl - pg_coef * ra) * ind).mean()                     # [rows, 1] x [rows] -> [rows, rows]: the reference's broadcast
    l_kl, l_pg = (ind * kl).sum() / rows, -pg_coef * ra.sum() / rows
    out = {"loss": float(loss.detach()), "count": float(ind.sum()), "kl_sum": float((ind * kl).sum().detach()), "ra_sum": float(ra.sum().detach()),
           "scale": float((ind * kl).abs().mean().detach() + pg_coef * t["adv"].abs().mean()), "ra_scale": float(t["adv"].abs().sum()),
           "term_sum": float((pg_coef * ind.mean() * ra - ind[:, 0] * kl[:, 0]).sum().detach())}
    for nm, l in (("", loss), ("_kl", l_kl), ("_pg", l_pg)):
        dm, dl, dl_abs = _grads(l, mean, ls_rows)
        out.update({f"d_mean{nm}": dm, f"d_log_std{nm}": dl, f"d_log_std{nm}_scale": dl_abs})
    # a row's KL term of d(log_std) is var_ratio - 1: itself a difference of two O(1) numbers, each rounded in float32 (var_ratio
    # comes out of an exp and a division), and the same for every row.  The scale of that sum is the sum of the absolute values of
    # ITS terms, mean(ind) * (var_ratio + 1), not |var_ratio - 1| (1e-3 where old_std happens to be close to exp(log_std))
    vr = n64((torch.exp(t["log_std"]) / t["old_std"]) ** 2).astype(np.float64)
    F = out["count"] / rows
    out["d_log_std_kl_scale"] = F * (vr + 1)
    out["d_log_std_scale"] = out["d_log_std_kl_scale"] + F * out["d_log_std_pg_scale"]
    return out


# --------------------------------------------------------------------------------------------------- spo_wide_linesearch_sums
@functools.lru_cache(maxsize=None)
def linesearch_problem(A, rows, moved):
    """The old distribution is the actor problem's (mean, log_std), logp_old its log-probability of the actions (float64, rounded
    once); the new one is the same (moved = False: KL exactly 0) or moved by N(0, 0.05) in the means and N(0, 0.03) in log_std."""
    p = actor_problem(A, rows)
    g = torch.Generator().manual_seed(_seed("wide-ls", A, rows, int(moved)))
    q = {"mean_old": p["mean"], "log_std_old": p["log_std"], "act": p["act"], "adv_a": p["adv"], "adv_b": p["adv_b"]}
    q["logp_old"] = _logp(p["mean"].double(), torch.exp(p["log_std"].double()), p["act"].double()).float()
    q["mean_new"] = p["mean"] + 0.05 * torch.randn(rows, A, generator=g) if moved else p["mean"].clone()
    q["log_std_new"] = p["log_std"] + 0.03 * torch.randn(A, generator=g) if moved else p["log_std"].clone()
    return q


@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def linesearch_oracle(A, rows, moved, dtype_name, variant=None):
    """cpo.py:473-491 -> sums [3] = {sum ratio * adv_a, sum ratio * adv_b, sum over rows and dims of KL(old || new)}, scales [3]."""
    t = {k: v.to(getattr(torch, dtype_name)) for k, v in linesearch_problem(A, rows, moved).items()}
    new, old = Normal(t["mean_new"], torch.exp(t["log_std_new"])), Normal(t["mean_old"], torch.exp(t["log_std_old"]))
    ratio = torch.exp(new.log_prob(t["act"]).sum(-1) - t["logp_old"])
    kl = kl_divergence(new, old) if variant == "kl_swapped" else kl_divergence(old, new)
    return {"sums": np.array([float((ratio * t["adv_a"]).sum()), float((ratio * t["adv_b"]).sum()), float(kl.sum())]),
            "scales": np.array([float(t["adv_a"].abs().sum()), float(t["adv_b"].abs().sum()), max(float(kl.abs().sum()), 1e-30)])}


# ------------------------------------------------------------------------------------ spo_wide_ppo_loss, spo_wide_critic_loss
@functools.lru_cache(maxsize=None)
def critic_problem(rows, seed=0):
    g = torch.Generator().manual_seed(_seed("wide-critic", rows, seed))
    r = lambda: torch.randn(rows, generator=g)
    return {"v_r": r(), "v_c": 0.5 * r().abs(), "tgt_r": 0.3 + 1.2 * r(), "tgt_c": 0.7 * r().abs()}


@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def critic_oracle(rows, dtype_name, seed=0):
    """F.mse_loss of both critics and the gradients at their outputs -> d_vr, d_vc [rows], losses [2]."""
    t = {k: v.to(getattr(torch, dtype_name)) for k, v in critic_problem(rows, seed).items()}
    vr, vc = t["v_r"].clone().requires_grad_(True), t["v_c"].clone().requires_grad_(True)
    lr_, lc_ = torch.nn.functional.mse_loss(vr, t["tgt_r"]), torch.nn.functional.mse_loss(vc, t["tgt_c"])
    (lr_ + lc_).backward()
    return {"d_vr": n64(vr.grad), "d_vc": n64(vc.grad), "losses": np.array([float(lr_.detach()), float(lc_.detach())])}


# ----------------------------------------------------------------------------------------------------- spo_wide_fvp_cotangent
@functools.lru_cache(maxsize=None)
def fvp_problem(A, rows):
    g = torch.Generator().manual_seed(_seed("wide-fvp", A, rows))
    return {"jv": torch.randn(rows, A, generator=g), "log_std": torch.linspace(-1.5, 1.5, A) if A > 1 else torch.tensor([-1.5])}


@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def fvp_oracle(A, rows, rows_total, dtype_name, variant=None):
    """The cotangent of the Fisher-vector product: the gradient at `mean` of mean over rows_total rows AND act_dim dims of
    KL(old || new) has the Jacobian-vector product (J t) / sigma^2 / (rows_total * act_dim) (cpo.py:132-157, differentiated twice
    at new == old): autograd of 0.5 * sum(jv_detached * ((m - m0) / sigma)^2 ...) written directly."""
    t = {k: v.to(getattr(torch, dtype_name)) for k, v in fvp_problem(A, rows).items()}
    m = torch.zeros_like(t["jv"]).requires_grad_(True)
    old, new = Normal(torch.zeros_like(m), torch.exp(t["log_std"]).expand(rows, A)), Normal(m, torch.exp(t["log_std"]).expand(rows, A))
    denom = rows if variant == "rows_only" else rows_total * A
    kl = kl_divergence(old, new).sum() / denom
    (gm,) = torch.autograd.grad(kl, m, create_graph=True)
    (hv,) = torch.autograd.grad((gm * t["jv"]).sum(), m)
    return {"d_mean": n64(hv)}


# ------------------------------------------------------------------------------------------ spo_gauss_sample, spo_gauss_kl_sum
SAMPLE_SHAPES = [(r, a) for a in (1, 17, 64) for r in (1, 256, 257)]


@functools.lru_cache(maxsize=None)
def sample_problem(rows, A):
    g = torch.Generator().manual_seed(_seed("wide-sample", rows, A))
    return {"mean": 0.5 * torch.randn(rows, A, generator=g), "eps": torch.randn(rows, A, generator=g),
            "log_std": torch.linspace(-1.5, 1.5, A) if A > 1 else torch.tensor([-1.5 if rows % 2 else 1.5])}


@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def sample_oracle(rows, A, dtype_name):
    """model.py:149-170: act = mean + std * eps (rsample), logp = Normal.log_prob(act).sum(-1); logp_det: of the mean itself."""
    t = {k: v.to(getattr(torch, dtype_name)) for k, v in sample_problem(rows, A).items()}
    d = Normal(t["mean"], torch.exp(t["log_std"]))
    act = t["mean"] + d.stddev * t["eps"]
    return {"act": n64(act), "logp": n64(d.log_prob(act).sum(-1)), "logp_det": n64(d.log_prob(t["mean"]).sum(-1)),
            "logp_scale": n64(d.log_prob(act).abs().sum(-1))}


KL_CASES = [(1, 1, True), (1000, 17, True), (1000, 64, False), (KL_CAP * 256 + 1, 1, True), (1000, 3, True)]      # (rows, act_dim, moved)


@functools.lru_cache(maxsize=None)
def kl_problem(rows, A, moved):
    g = torch.Generator().manual_seed(_seed("wide-kl", rows, A, int(moved)))
    mo, lo = 0.5 * torch.randn(rows, A, generator=g), (0.5 * torch.randn(A, generator=g)).clamp(-1, 1)
    if not moved:
        return {"mean_old": mo, "log_std_old": lo, "mean_new": mo.clone(), "log_std_new": lo.clone()}
    return {"mean_old": mo, "log_std_old": lo, "mean_new": mo + 0.1 * torch.randn(rows, A, generator=g), "log_std_new": lo + 0.05 * torch.randn(A, generator=g)}


@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def kl_oracle(rows, A, moved, dtype_name, variant=None):
    t = {k: v.to(getattr(torch, dtype_name)) for k, v in kl_problem(rows, A, moved).items()}
    old, new = Normal(t["mean_old"], torch.exp(t["log_std_old"])), Normal(t["mean_new"], torch.exp(t["log_std_new"]))
    kl = kl_divergence(new, old) if variant == "kl_swapped" else kl_divergence(old, new)
    return {"sum": float(kl.sum()), "scale": max(float(kl.abs().sum()), 1e-30)}


# ---------------------------------------------------------------------------------- spo_mlp_forward / _backward / _jvp / _multi
# (dims, rows, misalign): misalign "theta" / "x": that operand is a view one float into its buffer (scalar-load forms)
MLP_CASES = [([61, 100, 1], 129, None), ([61, 100, 1], 257, None), ([33, 256, 96, 5], 129, None), ([33, 256, 96, 5], 257, None),
             ([20, 1024, 32, 3], 3073, None), ([20, 1024, 32, 3], 3073, "theta"), ([18, 1024, 32, 3], 3073, None),
             ([20, 64, 3], 2049, None), ([20, 64, 3], 2049, "x")]
JVP_CASES = [([7, 3], r) for r in (1, 64, 129)] + [([12, 20, 24, 28, 32, 2], r) for r in (1, 64, 129)] + [([20, 1024, 32, 3], 3073), ([7, 3], 3073)]
MULTI_SMALL = [[7, 32, 1], [7, 32, 1], [7, 20, 24, 3], [12, 64, 64, 5]]     # every one inside csrc/mlp_small.hip's envelope
MULTI_WIDE = [33, 256, 256, 5]                                             # too wide for it at 100 rows: the per-network fallback
MULTI_ROWS = 100
mlp_name = lambda c: "x".join(str(d) for d in c[0]) + f"@{c[1]}" + (f"/{c[2]}-offset" if len(c) > 2 and c[2] else "")


def mlp_blocks(dims):
    """(offset, count) of every parameter block W_0, b_0, W_1, ... in the flat vector."""
    out, o = [], 0
    for l in range(len(dims) - 1):
        for cnt in (dims[l + 1] * dims[l], dims[l + 1]):
            out.append((o, cnt))
            o += cnt
    return out


@functools.lru_cache(maxsize=None)
def mlp_problem(dims, rows):
    """theta (flat, nn.Linear order: W ~ N(0, 1 / fan_in), b ~ N(0, 0.01)), x, d_out, and a tangent laid out like theta whose
    bias entries are non-zero."""
    dims = list(dims)
    g = torch.Generator().manual_seed(_seed("wide-mlp", sum(dims), len(dims), rows))
    parts = []
    for l in range(len(dims) - 1):
        parts += [torch.randn(dims[l + 1], dims[l], generator=g).reshape(-1) / dims[l] ** 0.5, 0.1 * torch.randn(dims[l + 1], generator=g)]
    theta = torch.cat(parts)
    tangent = torch.randn(theta.numel(), generator=g) * (theta.abs() + 0.05)
    return {"theta": theta, "x": torch.randn(rows, dims[0], generator=g), "d_out": torch.randn(rows, dims[-1], generator=g), "tangent": tangent}


def _mlp_forward(parts, x, n):
    h, acts = x, []
    for l in range(n):
        h = h @ parts[2 * l].T + parts[2 * l + 1]
        if l + 1 < n:
            h = torch.tanh(h)
        acts.append(h)
    return acts


def _split(flat, dims):
    return [flat[o:o + c].reshape(dims[k // 2 + 1], dims[k // 2]) if k % 2 == 0 else flat[o:o + c] for k, (o, c) in enumerate(mlp_blocks(dims))]


@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def mlp_oracle(dims, rows, dtype_name, variant=None):
    """The tanh MLP of model.py:30-48 -> every layer's activations, the flat gradient of sum(out * d_out) (autograd), the
    forward-mode tangent of the output along `tangent` (torch.func.jvp) and its per-element scale."""
    dims, dtype = list(dims), getattr(torch, dtype_name)
    n = len(dims) - 1
    t = {k: v.to(dtype) for k, v in mlp_problem(tuple(dims), rows).items()}
    parts = [q.clone().requires_grad_(True) for q in _split(t["theta"], dims)]
    acts = _mlp_forward(parts, t["x"], n)
    (acts[-1] * t["d_out"]).sum().backward()
    grad = torch.cat([q.grad.reshape(-1) for q in parts])
    tang = _split(t["tangent"], dims)
    if variant == "bias_tangent_dropped":
        tang = [q if k % 2 == 0 else torch.zeros_like(q) for k, q in enumerate(tang)]
    prim = tuple(q.detach() for q in _split(t["theta"], dims))
    _, jv = torch.func.jvp(lambda *ps: _mlp_forward(ps, t["x"], n)[-1], prim, tuple(tang))
    # an element of the tangent output is the sum h tW^T + dh W^T + tb of the last layer, with cancellation: its scale is the sum of
    # the absolute values of those terms (h, dh: the last hidden layer's activations and their tangent; the observations' is zero)
    if n > 1:
        h, dh = torch.func.jvp(lambda *ps: _mlp_forward(ps, t["x"], n)[-2], prim, tuple(tang))
    else:
        h, dh = t["x"], torch.zeros_like(t["x"])
    scale = h.abs() @ tang[-2].abs().T + dh.abs() @ prim[-2].abs().T + tang[-1].abs()
    return {"acts": [n64(a) for a in acts], "grad": n64(grad), "jvp": n64(jv), "jvp_scale": n64(scale)}


# ------------------------------------------------------------------------------------------------------ spo_wide_clip_adam*
ADAM_LR_ACTOR, ADAM_LR_CRITIC, ADAM_EPS, ADAM_L2 = f32v(3e-4), f32v(1e-3), f32v(1e-8), f32v(1e-3)
BETA1, BETA2 = 0.9, 0.999                                           # what the caller means; the cfg carries their float32 values
ADAM_LAYOUTS = {3: (1, 2, 2), 700: (200, 400, 400), 262144 + 77: (100003, 200006, 200006)}      # n_params -> r_end, c_end, actor_begin
ADAM_LAYOUT_GAP = (200, 400, 417)                                   # 700 parameters, 17 (log_std) between the critics and actor_begin
# clip: "off" / "below" / "above3" / "just_over" (norm 1.0005e-3 against max_norm 1e-3: the 1e-6 of the coefficient shows)
ADAM_CONFIGS = [dict(clip=c, t=t, opts=o) for c, t, o in (("off", 0, 1), ("off", 9999, 0), ("below", 0, 0), ("below", 9999, 1),
                                                          ("above3", 0, 1), ("above3", 9999, 0), ("above3", 0, 0), ("off", 9999, 1))]
ADAM_CONFIGS.append(dict(clip="just_over", t=0, opts=0))
ADAM_CONFIGS.append(dict(clip="off", t=0, opts=1, fresh=True))     # a new optimiser: zero moments, so v = (1 - beta2) g^2 bare
ADAM_CONFIGS.append(dict(clip="off", t=0, opts=0, fresh=True))
ADAM_CONFIGS.append(dict(clip="off", t=7, opts=0, aged=True))      # moments aged over seven steps from zero: this step's (1 - beta2) g^2 is ~1/8 of v
ADAM_BIG = [0, 5, 8, 9]
# sub-ranges (form "ex" / "dev"): name -> (adam range, norm_begin, scale_rest) as functions of (c_end, actor_begin, P)
ADAM_RANGES = {"all": lambda c, ab, P: (0, P, 0, 0), "critic_fit": lambda c, ab, P: (0, ab, 0, 1), "cup": lambda c, ab, P: (c, P, c, 0)}
adam_name = lambda c: f"{c['clip']}/t{c['t']}/opts{c['opts']}" + ("/fresh" if c.get("fresh") else "") + ("/aged" if c.get("aged") else "")


@functools.lru_cache(maxsize=None)
def adam_problem(n, name, layout=None):
    cfg = next(c for c in ADAM_CONFIGS if adam_name(c) == name)
    g = torch.Generator().manual_seed(_seed("wide-adam", n, name))
    r = lambda: torch.randn(n, generator=g)
    theta, grad = r(), 0.1 * r()
    m0, v0 = 0.05 * r(), (0.05 * r()) ** 2 + 1e-4
    if cfg["clip"] == "just_over":                                     # (opts 0: no L2 term, the norm is the given gradient's)
        grad = (grad.double() * (1.0005e-3 / float(grad.double().norm()))).float()
        gs = 1e-3 / n ** 0.5
        m0, v0 = m0 * (10 * gs), v0 * (10 * gs) ** 2                  # moments of the gradient's size: a coefficient 1e-3 off shows in them
    if cfg.get("fresh"):
        m0, v0 = torch.zeros(n), torch.zeros(n)
    if cfg.get("aged"):
        m64, v64 = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
        for _ in range(cfg["t"]):
            gk = 0.1 * r().double()
            m64, v64 = BETA1 * m64 + (1 - BETA1) * gk, BETA2 * v64 + (1 - BETA2) * gk * gk
        m0, v0 = m64.float(), v64.float()
    r_end, c_end, ab = layout or ADAM_LAYOUTS[n]
    g64 = grad.double().clone()
    if cfg["opts"]:
        g64[:c_end] += 2 * ADAM_L2 * theta.double()[:c_end]
        g64[:r_end] *= 2
    norm64 = float(g64.norm())
    max_norm = {"off": f32v(1e6), "below": f32v(3 * norm64), "above3": f32v(norm64 / 3), "just_over": f32v(1e-3)}[cfg["clip"]]
    return {"theta": theta, "grad": grad, "m": m0, "v": v0, "max_norm": max_norm, "opts": cfg["opts"], "t": cfg["t"], "norm64": norm64,
            "layout": (r_end, c_end, ab), "losses3": torch.tensor([0.5, 0.25, 0.125])}


def _adam1_numpy(p, g, m, v, w1, w2, b2, eps, step_size, inv_bc2_sqrt):
    """csrc/adam.h's adam1 in float32 numpy with IEEE sqrt and division (the kernel's v_rcp / v_sqrt only add to the error); fmaf
    through float64 (exact product, one rounding of the sum to float32 up to double rounding)."""
    f = np.float32
    fma = lambda a, b, c: (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(f) if np.ndim(a) else \
        (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(f)
    m2 = fma(g - m, f(w1), m)
    v2 = fma(v, f(b2), (f(w2) * g) * g)
    denom = fma(np.sqrt(v2), f(inv_bc2_sqrt), np.full_like(v2, f(eps)))
    p2 = fma(m2 * (f(1) / denom), -f(step_size), p)
    return p2, m2, v2


@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def adam_oracle(n, name, dtype_name, variant=None, rng="all", layout=None, steps=None, lr_override=None):
    """ppo_lag.py:310-329 on given gradients: the critics' L2 term l2 * sum p^2 added to their losses (autograd: 2 * l2 * p), the
    reward critic's loss doubled under use_value_coefficient, clip_grad_norm_ over [norm_begin, P), one torch.optim.Adam step per
    parameter group inside the Adam range (reward critic, cost critic and the gap below actor_begin: lr_critic, the critics'
    clock; actor: lr_actor, its clock), from the given moments.  Outside the Adam range nothing moves; the gradient there is
    rescaled by clip_grad_norm_ when it belongs to the clipped set (scale_rest).  steps: (t critics, t actor), default the
    config's t for both.  lr_override: (actor, critic), negative = the cfg's.
    -> theta, update = theta - theta_before, m, v, grad (the buffer as the call leaves it),
    scalars4 = {coefficient, L2 term reward critic, cost critic, norm}, losses3.
    numpy_adam1_old / numpy_adam1_new (float32 only): the Adam step is csrc/adam.h's adam1 restated in numpy with the weights
    1.f - beta (old) or (float)(1.0 - beta) (csrc/adam_host.h)."""
    dtype = getattr(torch, dtype_name)
    p = adam_problem(n, name, layout)
    r_end, c_end, ab = p["layout"]
    lo, hi, norm0, rest = ADAM_RANGES[rng](c_end, ab, n)
    t_c, t_a = steps or (p["t"], p["t"])
    lr_a, lr_c = ADAM_LR_ACTOR, ADAM_LR_CRITIC
    if lr_override:
        lr_a, lr_c = (lr_override[0] if lr_override[0] >= 0 else lr_a), (lr_override[1] if lr_override[1] >= 0 else lr_c)
    l2 = ADAM_L2 if (p["opts"] and norm0 == 0) else 0.0
    vcoef = 2.0 if (p["opts"] and norm0 == 0) else 1.0
    groups = [(0, r_end, lr_c, t_c), (r_end, c_end, lr_c, t_c), (c_end, ab, lr_c, t_c), (ab, n, lr_a, t_a)]
    groups = [gr for gr in groups if gr[1] > gr[0]]
    theta0, gin = p["theta"].to(dtype), p["grad"].to(dtype)
    params, l2_terms = [], [0.0, 0.0]
    for k, (a, b, lr, t) in enumerate(groups):
        q = torch.nn.Parameter(theta0[a:b].clone())
        loss = (q * gin[a:b]).sum()                                   # a loss whose gradient is the given one
        if b <= c_end and l2:
            reg = q.pow(2).sum() * l2
            l2_terms[0 if b <= r_end else 1] = float(reg.detach())
            if variant == "l2_factor_one":
                reg = reg / 2
            if variant == "value_coefficient_before_l2":
                loss = loss * (vcoef if b <= r_end else 1.0) + reg
            else:
                loss = (loss + reg) * (vcoef if b <= r_end else 1.0)
        loss.backward()
        params.append(q)
    grad_pre = torch.cat([q.grad.detach().clone() for q in params])
    clipped = [q for q, gr in zip(params, groups) if gr[0] >= norm0]
    if variant == "clip_without_1e_6":
        norm = torch.cat([q.grad.reshape(-1) for q in clipped]).norm()
        for q in clipped:
            q.grad.mul_(torch.clamp(p["max_norm"] / norm, max=1.0))
    else:
        norm = torch.nn.utils.clip_grad_norm_(clipped, p["max_norm"])
    coef = min(1.0, p["max_norm"] / (float(norm) + 1e-6))
    grad_post = torch.cat([q.grad.detach().clone() for q in params])
    m, v = p["m"].to(dtype).clone(), p["v"].to(dtype).clone()
    for q, (a, b, lr, t) in zip(params, groups):
        if not (a >= lo and b <= hi):
            continue
        if variant in ("numpy_adam1_old", "numpy_adam1_new"):
            assert dtype == torch.float32
            one = np.float32(1)
            w1, w2 = (one - np.float32(BETA1), one - np.float32(BETA2)) if variant.endswith("old") else (np.float32(1.0 - BETA1), np.float32(1.0 - BETA2))
            bc1, bc2 = 1.0 - BETA1 ** (t + 1), 1.0 - BETA2 ** (t + 1)
            p2, m2, v2 = _adam1_numpy(q.detach().numpy(), q.grad.numpy(), m[a:b].numpy(), v[a:b].numpy(), w1, w2, np.float32(BETA2), ADAM_EPS,
                                      np.float32(lr / bc1), np.float32(1.0 / bc2 ** 0.5))
            with torch.no_grad():
                q.copy_(torch.from_numpy(p2)); m[a:b] = torch.from_numpy(m2); v[a:b] = torch.from_numpy(v2)
            continue
        opt = torch.optim.Adam([q], lr=lr, betas=(BETA1, BETA2), eps=ADAM_EPS)
        assert variant != "bias_correction_t" or t > 0                # (1 - beta^0 = 0: the variant needs a running clock)
        opt.state[q] = {"step": torch.tensor(float(t if variant != "bias_correction_t" else t - 1), dtype=torch.float32),
                        "exp_avg": m[a:b], "exp_avg_sq": v[a:b]}     # (views: the step writes the moments in place)
        opt.step()
    theta = torch.cat([q.detach() for q in params])
    losses3 = p["losses3"].to(dtype).clone()
    if norm0 == 0:
        losses3[0] += l2_terms[0]
        losses3[1] += l2_terms[1]
    # the gradient buffer after the call: inside the Adam range the L2 term / value coefficient were added in place (before the clip);
    # outside it the stale gradient was rescaled by the clip coefficient (scale_rest) or left alone
    inside = (torch.arange(n) >= lo) & (torch.arange(n) < hi)
    grad = torch.where(inside | (not rest), grad_pre, grad_post)
    return {"theta": n64(theta), "update": n64(theta) - n64(theta0), "m": n64(m), "v": n64(v), "grad": n64(grad),
            "scalars4": np.array([coef, l2_terms[0], l2_terms[1], float(norm)]), "losses3": n64(losses3), "range": (lo, hi, norm0, rest)}


def adam_update_floor(n, name, layout=None):
    """Half an ulp of max|theta|: the rounding of the stored parameter, which the kernel and the float32 oracle share."""
    return float(np.spacing(np.float32(adam_problem(n, name, layout)["theta"].abs().max()))) / 2


# ----------------------------------------------------------------------------------------------------------------------- gates
# |hip - f64| <= 3 |f32 - f64| + floor in max-norm and L2 (tests/fp64_gate.py), floor = 1e-6 of the quantity's scale: single
# evaluations from identical state.  Scale: max|f64| of a vector; for a sum with cancellation the float64 sum / mean of the absolute
# values of its terms (surrogate means: mean |adv|, as tests/test_gpu_wide_dims.py takes it).  Every gate prints both
# deviations and the floor before it asserts and notes its ratio |hip - f64| / (3 |f32 - f64| + floor) under the running test.
RATIOS = G.Ratios()


def _note(g):
    """Notes a fp64_gate.Gate under the running test."""
    RATIOS.note(os.environ.get("PYTEST_CURRENT_TEST", "?").split("::")[-1].split(" (")[0], g.ratio, g.what)


def gate(hip, f32, f64, what, scale=None, floor=None):
    """fp64_gate.gate on one array (or scalar).  scale: None -> max|f64|; a number; or an array of per-element scales.  floor: an
    absolute floor in place of 1e-6 x scale.  -> the ratio."""
    return G.gate(hip, f32, f64, what, scale=scale, floor=floor, note=_note).ratio


def gate_group(members, what):
    """fp64_gate.gate_group (max-norm and L2) on scalars of ONE kind over several cases: members = [(hip, f32, f64, scale)].
    -> the yardstick's max."""
    return G.gate_group(members, what, note=_note).d_32


def gate_blocks(hip, f32, f64, blocks, what):
    """fp64_gate.gate_blocks: a flat parameter vector, every block (offset, count) with its own scale.  -> the worst ratio."""
    return G.gate_blocks(hip, f32, f64, blocks, what, note=_note)


def gate_actor_vectors(hip, o32, o64, what, sfx=""):
    """d_mean per element and d_log_std against the sum of the absolute values of its per-row terms."""
    r1 = gate(hip[f"d_mean{sfx}"], o32[f"d_mean{sfx}"], o64[f"d_mean{sfx}"], f"d_mean{sfx} {what}")
    r2 = gate(hip[f"d_log_std{sfx}"], o32[f"d_log_std{sfx}"], o64[f"d_log_std{sfx}"], f"d_log_std{sfx} {what}", scale=o64[f"d_log_std{sfx}_scale"])
    return max(r1, r2)


def gate_adam(hip, o32, o64, n, name, what, layout=None, scalars=None):
    """Every output of one clip + Adam call: theta, both moments and the gradient per parameter range with its own scale, the
    update theta - theta_before against half an ulp of max|theta|, scalars4 and losses3 (appended to `scalars` for a group gate
    when given: single scalars)."""
    r_end, c_end, ab = layout or ADAM_LAYOUTS[n]
    blocks = [(0, r_end), (r_end, c_end - r_end), (c_end, ab - c_end), (ab, n - ab)]
    for key in ("theta", "m", "v"):
        gate_blocks(hip[key], o32[key], o64[key], blocks, f"adam {key} {what}")
    gate(hip["update"], o32["update"], o64["update"], f"adam update {what}", floor=adam_update_floor(n, name, layout))
    gate_blocks(hip["grad"], o32["grad"], o64["grad"], blocks, f"adam gradient {what}")
    names = ("clip coefficient", "L2 term reward critic", "L2 term cost critic", "norm")
    members = [(f"scalars4 {names[k]}", hip["scalars4"][k], o32["scalars4"][k], o64["scalars4"][k], max(abs(o64["scalars4"][k]), 1e-30)) for k in range(4)]
    members += [(f"losses3[{k}]", hip["losses3"][k], o32["losses3"][k], o64["losses3"][k], abs(o64["losses3"][k])) for k in range(3)]
    for nm, h, a, b, s in members:
        if b == 0.0:
            assert h == 0.0, (what, nm, h)
        elif scalars is None:
            gate_group([(h, a, b, s)], f"{nm} {what}")
        else:
            scalars.setdefault(nm, []).append((h, a, b, s))


def ratio_table():
    """RATIOS as text: the worst ratio per test and the gate it came from."""
    lines = [f"{'test':<100} worst |hip-f64| / (3 |f32-f64| + floor)"]
    for key, (r, what) in sorted(RATIOS.items()):
        lines.append(f"{key:<100} {r:.3f}   ({what})")
    worst = max(RATIOS.items(), key=lambda kv: kv[1][0]) if RATIOS else ("-", (0.0, ""))
    return "\n".join([f"worst of all: {worst[1][0]:.3f} in {worst[0]} ({worst[1][1]})", ""] + lines)
