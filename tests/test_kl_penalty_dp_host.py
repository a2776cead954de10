"""CPU tests (no GPU) of the data-parallel FOCOPS / CUP step: the split KL-penalty entry points refuse bad arguments before
any launch, and the decomposition they implement -- g = g_KL + F * g_PG with the GLOBAL indicator fraction F -- is the
gradient of the reference's loss on the union of the ranks' rows (focops.py:326-337)."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    return g.LIB


def _cfg(**over):
    from safepo import _abi
    c = dict(obs_dim=60, act_dim=8, batch=32, use_critic_norm=1, use_value_coefficient=0, clip=0.2, max_grad_norm=40.0,
             lr_actor=3e-4, lr_critic=3e-4, beta1=0.9, beta2=0.999, adam_eps=1e-8, l2_coef=0.001)
    c.update(over)
    return _abi.PpoCfg(**c)


def test_split_kl_penalty_entry_points_refuse_bad_arguments(built_lib):
    from safepo import _abi
    lib = _abi.load(built_lib)
    assert {"spo_kl_penalty_grad", "spo_clip_adam_ex", "spo_clip_adam_ex_then_kl_grad"} <= set(_abi.PROTOTYPES)
    cfg = _cfg()
    nn = [None] * 8
    X = ctypes.c_void_p(256)          # never dereferenced: every call below fails its checks before a launch
    # spo_kl_penalty_grad
    assert lib.spo_kl_penalty_grad(*nn, 32, ctypes.byref(cfg), None, None, 0.02, 0.5, 0, None, None, None, None) < 0
    assert b"null pointer" in lib.spo_last_error()
    args = [X] * 8
    for n_idx in (0, 33):
        assert lib.spo_kl_penalty_grad(*args, n_idx, ctypes.byref(cfg), X, X, 0.02, 0.5, 0, X, X, X, None) < 0
        assert b"bad n_idx" in lib.spo_last_error()
    crit = [X] * 4 + [None, None] + [X] * 2            # no critic targets: only with actor_only
    assert lib.spo_kl_penalty_grad(*crit, 32, ctypes.byref(cfg), X, X, 0.02, 0.5, 0, X, X, X, None) < 0
    assert b"critic targets" in lib.spo_last_error()
    bad = _cfg(obs_dim=500)
    assert lib.spo_kl_penalty_grad(*args, 32, ctypes.byref(bad), X, X, 0.02, 0.5, 0, X, X, X, None) < 0
    assert b"obs_dim 500" in lib.spo_last_error()
    # spo_clip_adam_ex
    assert lib.spo_clip_adam_ex(None, None, None, None, None, None, 0, 0, 1.0, 0.0, 0, ctypes.byref(cfg), None, None) < 0
    assert b"null pointer" in lib.spo_last_error()
    assert lib.spo_clip_adam_ex(X, X, X, X, None, None, -1, 0, 1.0, 0.0, 0, ctypes.byref(cfg), None, None) < 0
    assert b"step counts" in lib.spo_last_error()
    assert lib.spo_clip_adam_ex(X, X, X, X, X, None, 0, 0, 1.0, 0.0, 0, ctypes.byref(cfg), None, None) < 0
    assert b"needs the sums" in lib.spo_last_error()
    assert lib.spo_clip_adam_ex(X, X, X, X, None, None, 0, 0, 1.0, 0.0, 0, ctypes.byref(cfg), X, None) < 0
    assert b"losses3 needs the sums" in lib.spo_last_error()
    # the folded entry refuses through the optimiser's checks first
    assert lib.spo_clip_adam_ex_then_kl_grad(None, None, None, None, None, None, 0, 0, 1.0, *nn, 0.02, 0.5, 0, None, 0,
                                             ctypes.byref(cfg), None, None) < 0
    assert b"clip_adam_ex" in lib.spo_last_error()
    assert lib.spo_kl_penalty_grad(*args, 32, None, X, X, 0.02, 0.5, 0, X, X, X, None) < 0
    assert b"cfg is NULL" in lib.spo_last_error()


def _shard(policy, n, kl_rows, seed, D, A):
    """n rows whose KL(new || old) is kl_rows[i] per row (the old mean is offset from the policy's mean)."""
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(n, D, generator=g, dtype=torch.float64)
    act = torch.randn(n, A, generator=g, dtype=torch.float64)
    logp = -A * 0.9 - 0.5 * (act ** 2).sum(-1) + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    adv = torch.randn(n, generator=g, dtype=torch.float64)
    with torch.no_grad():
        dist = policy.actor(obs)
        mu, std = dist.mean, dist.stddev
    # KL(N(mu, s) || N(mu + d, s)) summed over A dims = 0.5 * A * (d / s)^2 with the same d / s in every dim
    delta = std * torch.sqrt(2.0 * torch.as_tensor(kl_rows, dtype=torch.float64) / A)[:, None]
    return obs, act, logp, adv, (mu + delta).detach(), std[0].detach()


def _grad(policy, loss):
    params = list(policy.actor.parameters())
    gs = torch.autograd.grad(loss, params, retain_graph=True)
    return torch.cat([x.reshape(-1) for x in gs])


def test_split_kl_penalty_gradient_equals_union_gradient_float64():
    """The spec the data-parallel kernels implement: with two shards whose indicator fractions differ (none over target_kl on
    one, about half on the other), the mean over the shards of g_KL + F_global * g_PG -- every part a local mean, as
    spo_kl_penalty_grad emits them -- is the float64 autograd gradient of focops_actor_loss on the union; with each shard's
    own F it is not (so a GPU test on such data separates the two)."""
    sys.path.insert(0, ROOT)
    from oracle import restatement as R
    torch.manual_seed(3)
    D, A, n, target_kl = 12, 3, 32, 0.05
    pol = R.OraclePolicy(D, A, hidden_sizes=(64, 64)).double()
    kl0 = torch.full((n,), 0.2 * target_kl, dtype=torch.float64)                          # F = 1
    kl1 = torch.where(torch.arange(n) % 2 == 0, torch.tensor(3.0 * target_kl, dtype=torch.float64),
                      torch.tensor(0.3 * target_kl, dtype=torch.float64))                 # F = 1 / 2
    shards = [_shard(pol, n, kl0, 11, D, A), _shard(pol, n, kl1, 12, D, A)]
    c = 1.0 / R.FOCOPS_LAM
    union = [torch.cat([s[i] for s in shards], 0) for i in range(5)] + [shards[0][5]]
    assert torch.allclose(shards[0][5], shards[1][5])          # state-independent std
    g_union = _grad(pol, R.focops_actor_loss(pol, *union, target_kl))

    parts, counts = [], []
    for obs, act, logp, adv, om, os_ in shards:
        dist = pol.actor(obs)
        old = torch.distributions.Normal(om, os_)
        kl = torch.distributions.kl_divergence(dist, old).sum(-1)
        ind = (kl.detach() <= target_kl).to(torch.float64)
        ratio = torch.exp(dist.log_prob(act).sum(-1) - logp)
        g_kl = _grad(pol, (ind * kl).mean())
        g_pg = _grad(pol, -c * (ratio * adv).mean())
        parts.append((g_kl, g_pg))
        counts.append(float(ind.sum()))
    F_local = [cnt / n for cnt in counts]
    F_global = sum(counts) / (2 * n)
    assert F_local[0] == 1.0 and 0.3 < F_local[1] < 0.7 and F_global != F_local[1]
    g_split = sum(gk + F_global * gp for gk, gp in parts) / 2
    scale = float(g_union.abs().max())
    assert float((g_split - g_union).abs().max()) <= 1e-12 * scale
    g_local = sum(gk + F * gp for (gk, gp), F in zip(parts, F_local)) / 2
    assert float((g_local - g_union).abs().max()) > 1e-3 * scale


def test_wide_split_entry_points_refuse_bad_arguments(built_lib):
    from safepo import _abi
    lib = _abi.load(built_lib)
    X = ctypes.c_void_p(256)          # never dereferenced
    assert lib.spo_wide_kl_penalty_split(*[None] * 7, 32, 17, 0.02, 0.5, *[None] * 6, 0, None) < 0
    assert b"null pointer" in lib.spo_last_error()
    assert lib.spo_wide_kl_penalty_split(*[X] * 7, 32, 65, 0.02, 0.5, *[X] * 6, 1 << 20, None) < 0
    assert b"act_dim 65" in lib.spo_last_error()
    assert lib.spo_wide_kl_penalty_split(*[X] * 7, 512, 17, 0.02, 0.5, *[X] * 6, 10, None) < 0
    assert b"partial workspace too small" in lib.spo_last_error()
    assert lib.spo_wide_kl_penalty_combine(X, None, X, 100, 0, 50, 0.5, 0.5, None, None) < 0
    assert b"null pointer" in lib.spo_last_error()
    assert lib.spo_wide_kl_penalty_combine(X, X, X, 100, 60, 50, 0.5, 0.5, None, None) < 0
    assert b"bad ranges" in lib.spo_last_error()
    cfg = _cfg()
    assert lib.spo_clip_adam_ex_then_grad(None, None, None, None, 0, 0, 1.0, 0, *[None] * 7, 0, ctypes.byref(cfg), None, None) < 0
    assert b"clip_adam_ex" in lib.spo_last_error()
