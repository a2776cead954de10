"""The cases of tests/test_gpu_full_batch_actor.py (no test in here): the shape and row tables of the full-batch actor kernels
(spo_cpo_surrogate_grad / spo_cpo_fvp / spo_cpo_linesearch_eval of csrc/cpo.hip at KIN 16 / 32 / 64; spo_actor_mean / spo_actor_kl
of csrc/policy.hip at KIN 16 / 32 / 64 / 128), every problem built on the CPU from seeds, and the same operation in plain torch
(oracle/restatement.py, autograd, torch.distributions.kl_divergence) in float32 -- the yardstick -- and float64 -- the reference.
tests/test_full_batch_actor_cases_host.py checks on the CPU that the problems keep the gates of the GPU test meaningful.

Every oracle result is computed once per process (functools.lru_cache) and shared; callers do not modify what they get.  The
oracles run on fp64_gate.ORACLE_THREADS torch threads whatever the host offers (blocked sums round differently with the thread count, and
the float32 oracle's rounding is the yardstick), and put the count back."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "safe-policy-optimization_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fp64_gate as G  # noqa: E402
from oracle import restatement as R  # noqa: E402
from test_gpu_parity import _synthetic_update_problem  # noqa: E402  (its tests carry the gpu marker; the builder needs no GPU)

# ---- csrc/cpo.hip through CPOEngine: both sides of each KIN boundary, act_dim / obs_dim that are no multiple of 4
CPO_SHAPES = [(1, 1), (12, 2), (16, 4), (17, 5), (32, 16), (33, 3), (60, 8), (64, 16)]
CPO_FORM_SHAPES = [(12, 2), (17, 5), (64, 16)]                   # one per KIN form
CPO_ROWS_ALL = 3037                                               # 47 full 64-row chunks + a 29-row tail, one chunk per workgroup
CPO_ROWS_CROSS_CHUNK = 256 * 64 + 64 + 29                        # 16 477: 258 chunks over the 256-partial cap -> workgroups 0 and 1
#                                                                  walk two chunks, workgroup 1's second one is the 29-row tail
CPO_CASES = {CPO_ROWS_ALL: CPO_SHAPES, 1: CPO_FORM_SHAPES, 63: CPO_FORM_SHAPES, CPO_ROWS_CROSS_CHUNK: CPO_FORM_SHAPES}
# line search: theta_actor += CPO_MOVE * randn.  test_cpo128_primitives_vs_oracle moves by 0.02 * randn; on these problems that
# takes max|ratio - 1| of the float64 oracle to 1.2 .. 3.4 at every shape of M = 3037 (KL 2e-3 .. 4e-3).  At 0.005 it stays
# below 0.7 there (0.98 at (64, 16) with 16 477 rows) and the KL is 5e-5 .. 3e-4, above the 1e-5 the CPU companion asks for.
CPO_MOVE = 0.005
LS_CAPPED = [3, 7]                                                # partial_capacity of the direct calls: 1 and 2 workgroups

# ---- csrc/policy.hip by direct ABI calls
ACTOR_SHAPES = [(1, 1), (16, 4), (17, 5), (33, 3), (60, 8), (64, 16), (65, 1), (100, 13), (128, 16)]
ACTOR_ROWS = [1, 15, 16, 17, 63, 65, 1000]
ACTOR_MOVE = 0.01                                                 # theta += ACTOR_MOVE * randn (tests/test_gpu_parity.py::test_actor_kl_vs_oracle)
ACTOR_SECOND_TILE = (6, 2, 768 * 64 + 17)                         # 49 169 rows: 3 074 tiles over 768 x 4 waves -> waves 0 and 1 of
#                                                                   workgroup 0 take a second tile, wave 1's has a single row
KL_CAPPED = [1, 2]                                                # kl_partials_capacity at 1000 rows: 63 tiles over 4 / 8 waves

# the CPU companion leaves out the two largest row counts
HOST_CPO_ROWS = [CPO_ROWS_ALL, 1, 63]


def kin(D):
    """The KIN form both files pick for obs_dim D (pick_kin; cpo.hip's own stops at 64)."""
    return 16 if D <= 16 else 32 if D <= 32 else 64 if D <= 64 else 128


def _seeded_policy_state(D, A, seed):
    """state_dict of ActorVCritic(D, A) initialised under `seed`, log_std = 0.2 * randn; torch's generator is left as found."""
    from safepo.common.model import ActorVCritic
    rng = torch.get_rng_state()
    torch.manual_seed(seed)
    pol = ActorVCritic(D, A)
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    torch.set_rng_state(rng)
    return {k: v.detach().clone() for k, v in pol.state_dict().items()}


def oracle_policy(state_dict, D, A, dtype):
    ref = R.OraclePolicy(D, A)
    assert list(ref.state_dict()) == list(state_dict)
    ref.load_state_dict({k: v.clone() for k, v in state_dict.items()})
    return ref.to(dtype)


# ------------------------------------------------------------------------------------------------------------- csrc/cpo.hip
@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def cpo_problem(D, A, M):
    """Parameters, batch and directions of case (D, A, M), all float32 on the CPU.  The batch is _synthetic_update_problem's with
    one change: that builder's log_prob assumes a standard-normal policy, and against an initialised actor with log_std != 0 its
    ratios reach e^2.  Here log_prob is the float64 oracle's log-probability of the actions at these parameters plus the
    builder's own 0.1 * N(0, 1) noise, so every ratio lies within (0.6, 1.6): the surrogate is then a mean of O(1) terms and
    mean|adv| is its scale."""
    seed = 100003 * D + 101 * A + M
    sd = _seeded_policy_state(D, A, seed)
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=seed + 1)
    noise = logp.double() + A * 0.9 + 0.5 * (act.double() ** 2).sum(-1)
    with torch.no_grad():
        logp = (oracle_policy(sd, D, A, torch.float64).actor(obs.double()).log_prob(act.double()).sum(-1) + noise).float()
    Pa = A + 64 * D + 64 + 64 * 64 + 64 + A * 64 + A
    draw = lambda s: torch.randn(Pa, generator=torch.Generator().manual_seed(s))
    return {"state_dict": sd, "Pa": Pa, "v": draw(3), "u": draw(4), "delta": CPO_MOVE * draw(5),
            "data": {"obs": obs, "act": act, "log_prob": logp, "adv_r": adv, "adv_c": adv.flip(0) * 0.5 + 0.1}}


@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def cpo_oracle(D, A, M, dtype_name):
    """Everything CPOEngine's three primitives return for case (D, A, M), from the oracle in `dtype_name`: float64 numpy vectors
    and python floats."""
    dtype = getattr(torch, dtype_name)
    p = cpo_problem(D, A, M)
    ref = oracle_policy(p["state_dict"], D, A, dtype)
    data = {k: v.to(dtype) for k, v in p["data"].items()}
    assert R.actor_flat_params(ref.actor).numel() == p["Pa"]
    out = {"adv_scale": float(p["data"]["adv_r"].abs().mean())}
    for which in ("r", "c"):
        ref.actor.zero_grad()
        loss = R.cpo_surrogate(ref, data, which)
        loss.backward()
        out["grad_" + which] = R.actor_flat_grads(ref.actor).double().numpy().copy()
        out["loss_" + which] = float(loss.detach())
    for name in ("v", "u"):
        out["F" + name] = R.cpo_fvp(p[name].to(dtype), ref, data["obs"]).detach().double().numpy().copy()
    v64, u64 = p["v"].double().numpy(), p["u"].double().numpy()
    out["uFv"], out["vFu"] = float(u64 @ out["Fv"]), float(v64 @ out["Fu"])

    def ratio_spread():
        lp = ref.actor(data["obs"]).log_prob(data["act"]).sum(-1)
        return float((torch.exp(lp - data["log_prob"]) - 1).abs().max())
    with torch.no_grad():
        out["ratio_spread"] = ratio_spread()
        old = ref.actor(data["obs"])
        old_mean, old_std = old.mean.clone(), old.stddev.clone()
        R.actor_set_flat_params(ref.actor, R.actor_flat_params(ref.actor) + p["delta"].to(dtype))
        out["moved_kl"] = float(torch.distributions.kl_divergence(torch.distributions.Normal(old_mean, old_std), ref.actor(data["obs"])).mean())
        out["moved_loss_r"] = float(R.cpo_surrogate(ref, data, "r"))
        out["moved_loss_c"] = float(R.cpo_surrogate(ref, data, "c"))
        out["moved_ratio_spread"] = ratio_spread()
    return out


# ---------------------------------------------------------------------------------------------------------- csrc/policy.hip
@functools.lru_cache(maxsize=None)
def actor_problem(D, A, rows):
    """theta (as the state_dict of ActorVCritic(D, A)), observations and the perturbation of the whole flat vector (critics and
    log_std included), float32 on the CPU."""
    seed = 200003 * D + 103 * A + rows
    sd = _seeded_policy_state(D, A, seed)
    g = torch.Generator().manual_seed(seed + 1)
    obs = torch.randn(rows, D, generator=g)
    P = sum(v.numel() for v in sd.values())
    return {"state_dict": sd, "obs": obs, "delta": ACTOR_MOVE * torch.randn(P, generator=g)}


@functools.lru_cache(maxsize=None)
@G.on_oracle_threads()
def actor_oracle(D, A, rows, dtype_name):
    """-> {"mean": [rows, A] float64 numpy, "kl": KL(old || moved).sum(-1).mean() with old = this dtype's own forward}."""
    dtype = getattr(torch, dtype_name)
    p = actor_problem(D, A, rows)
    ref = oracle_policy(p["state_dict"], D, A, dtype)
    obs = p["obs"].to(dtype)
    with torch.no_grad():
        old = ref.actor(obs)
        old_mean, old_std = old.mean.clone(), old.stddev.clone()
        off = 0
        for prm in ref.parameters():                      # parameters() order == the flat theta's (asserted on the keys above)
            n = prm.numel()
            prm.add_(p["delta"][off:off + n].view(prm.shape).to(dtype))
            off += n
        assert off == p["delta"].numel()
    return {"mean": old_mean.double().numpy().copy(), "kl": R.actor_kl(ref, obs, old_mean, old_std)}


# ------------------------------------------------------------------------------------------------------------------- gates
# |hip - f64| <= 3 |f32 - f64| + floor with the floors of tests/test_gpu_cpo_obs128.py::test_cpo128_primitives_vs_oracle:
# 1e-6 * mean|adv_r| (surrogate means, line-search sums), 1e-6 * max|f64| (vectors), 1e-6 * kl64 (KL).  Every gate prints both
# deviations and the floor before it asserts, and notes its ratio |hip - f64| / (3 |f32 - f64| + floor) under
# (entry point, KIN form, rows) in RATIOS.
RATIOS = G.Ratios()


def gate_vector(entry, D, rows, hip, f32, f64, what):
    """fp64_gate.gate (max-norm and L2, floor 1e-6 * max|f64|)."""
    G.gate(hip, f32, f64, what, note=lambda g: RATIOS.note((entry, kin(D), rows), g.ratio, what))


def gate_group(entry, rows, members, what):
    """fp64_gate.gate_group (max-norm) over the scalars of ONE kind of all shapes of one row count.  members: [(name, D, hip, f32,
    f64, scale)]; scale = the case's mean|adv_r| for a surrogate loss (each member is measured against ITS OWN case's scale),
    None for a KL (measured against |f64|).  The yardstick is the largest such deviation of the float32 oracle in the group.
    Returns it."""
    def note(g):
        for (name, D, *_), ratio in zip(members, g.ratios):
            RATIOS.note((entry, kin(D), rows), ratio, f"{what} / {name}")
    return G.gate_group([m[2:] for m in members], what, l2=False, note=note).d_32


def ratio_table():
    """RATIOS as text: one line per (entry point, KIN form, rows)."""
    lines = [f"{'entry point':<28} {'KIN':>4} {'rows':>6}  worst |hip-f64| / (3 |f32-f64| + floor)"]
    for (entry, k, rows), (r, _) in sorted(RATIOS.items()):
        lines.append(f"{entry:<28} {k:>4} {rows:>6}  {r:.3f}")
    return "\n".join(lines)
