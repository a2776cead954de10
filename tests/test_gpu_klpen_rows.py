"""GPU tests of the KL-penalty form of the row-group gradient kernel (csrc/mlp_rows.hip): FOCOPS's minibatch step
(focops.py:312-347) and CUP's actor-only second stage (cup.py:370-386) for hidden_sizes other than [64, 64] in one gradient launch
split over 16-row groups, CUP's first stage on the same kernel's clipped-surrogate form, and the data-parallel split step.
Oracle: oracle/restatement.py (OraclePolicy, KLPenaltyUpdater: the reference's own torch calls); gates: tests/envelope.py."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

from oracle import restatement as R  # noqa: E402  (checker only)
from test_gpu_parity import _synthetic_update_problem, _wide_pair  # noqa: E402

CUP_COEF = (1 - 0.99 * 0.95) / (1 - 0.99)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _problem(D, A, hidden, M, batch, actor_only, dev):
    """Engine, oracle policy and inputs of test_gpu_wide_dims.py::test_wide_kl_penalty_minibatch_steps_vs_oracle (same seeds: the
    networks from M + D, the rows from M, old_mean / old_std drawn after them, kl_bound the 0.55 quantile of the rows' KL)."""
    from safepo.common.engine import WidePPOLagEngine
    pol, ref = _wide_pair(D, A, hidden, dev, seed=M + D)
    problem = _synthetic_update_problem(M, D, A, seed=M)
    obs = problem[0]
    with torch.no_grad():
        dist = ref.actor(obs)
        old_mean = dist.mean + 0.05 * torch.randn(M, A)
        old_std = dist.stddev[0] * torch.exp(0.05 * torch.randn(A))
        kl0 = torch.distributions.kl_divergence(dist, torch.distributions.Normal(old_mean, old_std.expand(M, A))).sum(-1)
    kl_bound = float(kl0.quantile(0.55)) if not actor_only else float("inf")
    pg_coef = 1 / 1.5 if not actor_only else -0.37
    cfg = {"hidden_sizes": hidden, "gamma": 0.99, "target_kl": 1e9, "batch_size": batch, "learning_iters": 1, "max_grad_norm": 40.0}
    eng = WidePPOLagEngine(pol, 1, M, cfg, dev)
    obs, act, logp, tgt_r, tgt_c, adv = problem
    b = eng.buffer
    b.data["obs"].copy_(obs.view(1, M, D)); b.data["act"].copy_(act.view(1, M, A)); b.data["log_prob"].copy_(logp.view(1, M))
    b.data["target_value_r"].copy_(tgt_r.view(1, M)); b.data["target_value_c"].copy_(tgt_c.view(1, M)); b.adv_mix.copy_(adv.view(1, M))
    eng.mean_old.copy_(old_mean); eng.std_old.copy_(old_std)
    return pol, ref, eng, problem, old_mean, old_std, kl_bound, pg_coef


def _oracle_grad(rp, dtype, rows, om, os_, kl_bound, actor_only):
    """Flat autograd gradient of the step's loss WITHOUT the critics' L2 terms (the optimiser entry points add them), the data
    losses [r, c, pi], the number of rows inside the bound and the smallest |KL_i - bound|."""
    o_, a_, lp_, tr_, tc_, ad_ = (t.to(dtype) for t in rows)
    om, os_ = om.to(dtype), os_.to(dtype).expand_as(om)
    rp.zero_grad()
    with torch.no_grad():
        kl_i = torch.distributions.kl_divergence(rp.actor(o_), torch.distributions.Normal(om, os_)).sum(-1)
    count = int((kl_i <= kl_bound).sum())
    margin = float((kl_i - kl_bound).abs().min()) if np.isfinite(kl_bound) else float("inf")
    if actor_only:
        loss_pi = R.cup_second_stage_loss(rp, o_, a_, lp_, ad_, om, os_, 0.37 / CUP_COEF, 0.99)
        loss_pi.backward()
        g = torch.cat([p.grad.reshape(-1) for p in rp.actor.parameters()])
        return g.double().numpy(), [np.nan, np.nan, loss_pi.item()], count, margin
    loss_r = torch.nn.functional.mse_loss(rp.reward_critic(o_), tr_)
    loss_c = torch.nn.functional.mse_loss(rp.cost_critic(o_), tc_)
    loss_pi = R.focops_actor_loss(rp, o_, a_, lp_, ad_, om, os_, kl_bound)
    (loss_pi + loss_r + loss_c).backward()
    return R.flat_grads(rp).double().numpy(), [loss_r.item(), loss_c.item(), loss_pi.item()], count, margin


def _launch(eng, idx, kl_bound, pg_coef, actor_only, combine, window=None, adv=None):
    """spo_wide_kl_penalty_grad_rows + spo_wide_kl_penalty_reduce_parts through the C ABI into fresh NaN-filled outputs:
    (grad, pg_grad, sums, losses).  idx: device int64 indices, None (the rows themselves: `window` = their number), or with
    `window` = (PermWindow, rows) the window at its device cursor."""
    from safepo import _abi
    lib, w, dev = eng.lib, eng.wide, eng.dev
    d, M, D, A = eng.buffer.data, eng.M, eng.D, eng.A
    if isinstance(window, tuple):
        win, n = window
        p_idx, p_cur = _abi.ptr(win.perm), _abi.ptr(win.cursor)
    elif idx is None:
        n, p_idx, p_cur = int(window), None, None
    else:
        n, p_idx, p_cur = idx.numel(), _abi.ptr(idx), None
    parts = torch.full((int(lib.spo_wide_kl_penalty_rows_part_floats(w.P, w.off_ls, n)),), float("nan"), device=dev)
    adv = eng.buffer.adv_mix if adv is None else adv
    _abi.check(lib.spo_wide_kl_penalty_grad_rows(
        _abi.ptr(eng.policy.theta), w.net_c, w.net_a, _abi.ptr(d["obs"]), _abi.ptr(d["act"]), _abi.ptr(d["log_prob"]),
        None if actor_only else _abi.ptr(d["target_value_r"]), None if actor_only else _abi.ptr(d["target_value_c"]), _abi.ptr(adv),
        _abi.ptr(eng.mean_old), _abi.ptr(eng.std_old), p_idx, p_cur, n, float(kl_bound), float(pg_coef), int(actor_only),
        _abi.ptr(parts), _abi.stream_ptr()), "spo_wide_kl_penalty_grad_rows")
    g = torch.full((w.P,), float("nan"), device=dev)
    pg = torch.full((w.P,), float("nan"), device=dev)
    sums = torch.full((_abi.KLPEN_SUMS,), float("nan"), device=dev)
    l3 = torch.full((3,), float("nan"), device=dev)
    _abi.check(lib.spo_wide_kl_penalty_reduce_parts(_abi.ptr(parts), n, w.P, w.off_ls, int(actor_only), int(combine), float(pg_coef),
                                                    _abi.ptr(g), _abi.ptr(pg), _abi.ptr(sums), _abi.ptr(l3), _abi.stream_ptr()),
               "spo_wide_kl_penalty_reduce_parts")
    torch.cuda.synchronize()
    return g, pg, sums, l3


# (first row, rows, how the rows are named): 64 = four full groups, 22 = a ragged second group, 50, 256 = all sixteen groups
CASES = [(0, 64, "idx"), (64, 22, "idx"), (86, 50, "window"), (136, 256, "idx"), (0, 50, "null"), (400, 64, "window"), (392, 22, "idx")]


@pytest.mark.parametrize("actor_only", [False, True])
@pytest.mark.parametrize("D,A,hidden", [(60, 8, [128, 128]), (33, 3, [256, 96])])
def test_klpen_row_group_gradient_vs_autograd(dev, D, A, hidden, actor_only):
    """1. The gradient launch + the group sum (combine = 1) of ONE minibatch against torch autograd of the oracle's loss in float32
    and float64: the flat gradient under E.gate_array(rel_floor=1e-6), the losses at rtol 1e-5 / atol 2e-6, the count of rows
    inside the bound EQUAL to the oracle's (float32 and float64 oracle agree on it, no row within 1e-6 of the bound).  theta is
    not written; with actor_only the critics' block of the gradient is not written."""
    import envelope as E
    from safepo.common.wide import PermWindow
    M = 700
    pol, ref, eng, problem, old_mean, old_std, kl_bound, pg_coef = _problem(D, A, hidden, M, 64, actor_only, dev)
    w = eng.wide
    assert w.klpen_rows_ok(64) and w.klpen_rows_ok(256) and not w.klpen_rows_ok(257)
    ref64 = copy.deepcopy(ref).double()
    theta0 = pol.theta.clone()
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(6))
    for lo, n, form in CASES:
        if form == "null":
            idx = torch.arange(n)
            g, pg, sums, l3 = _launch(eng, None, kl_bound, pg_coef, actor_only, 1, window=n)
        elif form == "window":
            idx = perm[lo:lo + n]
            win = PermWindow(M, n, dev)
            win.load(perm.to(dev))
            win.cursor.fill_(lo)
            g, pg, sums, l3 = _launch(eng, None, kl_bound, pg_coef, actor_only, 1, window=(win, n))
        else:
            idx = perm[lo:lo + n]
            g, pg, sums, l3 = _launch(eng, idx.to(dev), kl_bound, pg_coef, actor_only, 1)
        rows = [t[idx] for t in problem]
        g32, l32, c32, margin = _oracle_grad(ref, torch.float32, rows, old_mean[idx], old_std, kl_bound, actor_only)
        g64, l64, c64, _ = _oracle_grad(ref64, torch.float64, rows, old_mean[idx], old_std, kl_bound, actor_only)
        assert c32 == c64 and margin > 1e-6, (lo, n, c32, c64, margin)               # no row sits ON the bound
        if not actor_only:
            assert 0 < c32 < n, (lo, n, c32)
        s = sums.cpu().numpy()
        assert s[2] == c32 and s[5] == n and s[0] == 0 and s[1] == 0, (lo, n, form, s, c32)
        got = g.cpu().numpy().astype(np.float64)
        off = w.off_ls
        if actor_only:
            assert np.isnan(got[:off]).all(), "actor_only wrote the critics' block"
            got = got[off:]
        assert np.isfinite(got).all(), f"{int(np.isnan(got).sum())} gradient elements never written (rows {n}, {form})"
        print(f"klpen rows {D}x{A} {hidden} actor_only={actor_only} rows {n} ({form}): count {c32}, max|hip-f64| / max|f64| = "
              f"{np.abs(got - g64).max() / np.abs(g64).max():.2e}, oracle f32 {np.abs(g32 - g64).max() / np.abs(g64).max():.2e}")
        E.gate_array(got, g32, g64, f"KL-penalty row-group gradient, rows {n} ({form})", rel_floor=1e-6)
        np.testing.assert_allclose(l3.cpu().numpy(), l32, rtol=1e-5, atol=2e-6, equal_nan=True)
        # the policy-gradient part is there on its own too: pg_coef * (sum ratio*adv) / rows is its loss term at F = 1
        assert torch.isfinite(pg[off:]).all() and np.isfinite(s[3]) and np.isfinite(s[4])
    assert torch.equal(pol.theta, theta0)


@pytest.mark.parametrize("D,A,hidden", [(60, 8, [128, 128]), (33, 3, [256, 96]), (17, 2, [32])])
def test_klpen_split_identity_and_determinism(dev, D, A, hidden):
    """2. combine = 0 followed by spo_wide_kl_penalty_combine(grad_scale = 1) is bit-equal to combine = 1 (gradient and actor loss);
    with actor_only the critics' block of grad is not written.  3. Two launches on the same inputs give bit-equal outputs."""
    from safepo import _abi
    M = 300
    for actor_only in (False, True):
        pol, ref, eng, problem, old_mean, old_std, kl_bound, pg_coef = _problem(D, A, hidden, M, 64, actor_only, dev)
        w, lib = eng.wide, eng.lib
        perm = torch.randperm(M, generator=torch.Generator().manual_seed(8)).to(dev)
        for lo, n in ((0, 64), (64, 22), (86, 200)):
            idx = perm[lo:lo + n].contiguous()
            g1, pg1, s1, l1 = _launch(eng, idx, kl_bound, pg_coef, actor_only, 1)
            g0, pg0, s0, l0 = _launch(eng, idx, kl_bound, pg_coef, actor_only, 0)
            g0b, pg0b, s0b, l0b = _launch(eng, idx, kl_bound, pg_coef, actor_only, 0)
            for a, b in ((g0, g0b), (pg0, pg0b), (s0, s0b), (l0, l0b)):          # determinism (NaN = not written, in both)
                assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
            assert torch.equal(s0, s1) and torch.equal(pg0[w.off_ls:], pg1[w.off_ls:])
            assert torch.isnan(l0[2]) and torch.isfinite(l1[2])
            lo_p = w.off_ls if actor_only else 0
            assert torch.isnan(pg0[:w.off_ls]).all()
            if actor_only:
                assert torch.isnan(g0[:lo_p]).all() and torch.isnan(g1[:lo_p]).all() and torch.isnan(l1[:2]).all()
            else:
                assert torch.equal(l0[:2], l1[:2]) and torch.isfinite(l1[:2]).all()
                assert torch.equal(g0[:w.off_ls], g1[:w.off_ls])
            assert not torch.equal(g0[w.off_ls:], g1[w.off_ls:])                  # (F g_PG is not 0)
            _abi.check(lib.spo_wide_kl_penalty_combine(_abi.ptr(g0), _abi.ptr(pg0), _abi.ptr(s0), w.P, lo_p, w.off_ls, 1.0, float(pg_coef),
                                                       _abi.ptr(l0[2:]), _abi.stream_ptr()), "spo_wide_kl_penalty_combine")
            torch.cuda.synchronize()
            assert torch.equal(g0[lo_p:], g1[lo_p:]) and torch.equal(l0[2], l1[2])


# D, A, hidden, actor_only, M, batch: the inputs whose indicator margins were checked on the CPU oracle (see the table below)
TRAJECTORIES = [(60, 8, [128, 128], False, 214, 64), (60, 8, [256, 256], False, 214, 64), (72, 2, [128, 128], False, 214, 64),
                (104, 12, [128, 128], False, 214, 64), (33, 3, [256, 96], False, 214, 64), (33, 3, [256, 96], True, 214, 64),
                (17, 2, [32], False, 250, 100), (60, 8, [128, 128], False, 600, 256)]


@pytest.mark.parametrize("D,A,hidden,actor_only,M,batch", TRAJECTORIES)
def test_klpen_row_group_minibatch_steps_vs_oracle(dev, D, A, hidden, actor_only, M, batch):
    """4. The protocol of test_gpu_wide_dims.py::test_wide_kl_penalty_minibatch_steps_vs_oracle, unchanged, through
    WidePPOLagEngine.learning_iter_ex on the row-group path (asserted): indicator active on part of every minibatch, the actor's
    optimiser clock 5 steps ahead, a ragged last minibatch (the graph-replayed steps read the window's device cursor, the last one
    runs eagerly), first step at 1e-5, losses and parameters inside the rounding envelope around the float64 trajectory; with
    actor_only the critics bit-untouched and the clocks checked.  33 inputs: the scalar weight loads; [32]: a one-hidden-layer
    actor; 256 rows: all sixteen row groups.  Rows outside the bound per minibatch and the smallest |KL - bound| of any step, on
    the CPU oracle's own trajectory (float32 and float64 agree on every count; the test prints them and asserts the condition):
      60, 8, [128, 128]   26, 34, 33, 7    1.9e-5 (bound 1.97e-2)      60, 8, [256, 256]   24, 30, 38, 13   1.6e-5 (1.35e-2)
      72, 2, [128, 128]   34, 20, 30, 13   6.3e-6 (3.3e-3)             104, 12, [128, 128] 24, 31, 26, 12   7.9e-6 (5.0e-2)
      33, 3, [256, 96]    28, 26, 34, 10   8.5e-6 (1.6e-2)             17, 2, [32] (250 / 100)  45, 42, 23  6.4e-6 (3.9e-3)
      60, 8, [128, 128] (600 / 256)  113, 114, 45   3.1e-6 (3.3e-2)"""
    import envelope as E
    from safepo import _abi
    pol, ref, eng, problem, old_mean, old_std, kl_bound, pg_coef = _problem(D, A, hidden, M, batch, actor_only, dev)
    obs, act, logp, tgt_r, tgt_c, adv = problem
    assert not eng._feature_split_kernel_ok(eng._cfg_struct())
    assert eng._row_group_step_ok(batch, _abi.ACTOR_LOSS_KL_PENALTY, actor_only) is True
    assert eng._row_group_step_ok(M % batch, _abi.ACTOR_LOSS_KL_PENALTY, actor_only) is True
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(3))
    eng.adam_step_actor_extra = 5
    theta0 = pol.theta.clone()
    ref64 = copy.deepcopy(ref).double()

    def oracle(rp, dtype):
        upd = R.KLPenaltyUpdater(rp)
        for _ in range(5):                          # the actor's Adam clock runs 5 steps ahead (zero gradients: moments stay 0)
            upd.opt_a.zero_grad()
            for prm in rp.actor.parameters():
                prm.grad = torch.zeros_like(prm)
            upd.opt_a.step()
        o_, a_, lp_, tr_, tc_, ad_, om_ = (t.to(dtype) for t in (obs, act, logp, tgt_r, tgt_c, adv, old_mean))
        os_full = old_std.expand(M, A).to(dtype)
        out, masked, margin = [], [], float("inf")
        for s0 in range(0, M, batch):
            idx = perm[s0:s0 + batch]
            with torch.no_grad():
                kl_i = torch.distributions.kl_divergence(rp.actor(o_[idx]), torch.distributions.Normal(om_[idx], os_full[idx])).sum(-1)
                masked.append(int((kl_i > kl_bound).sum()))
                margin = min(margin, float((kl_i - kl_bound).abs().min()))
            if actor_only:
                l = upd.cup_second_stage_step(o_[idx], a_[idx], lp_[idx], ad_[idx], om_[idx], os_full[idx], 0.37 / CUP_COEF, 0.99)
                out.append([np.nan, np.nan, l])
            else:
                out.append(list(upd.focops_step(o_[idx], a_[idx], lp_[idx], tr_[idx], tc_[idx], ad_[idx], om_[idx], os_full[idx], kl_bound)))
        return np.asarray(out, np.float64), R.flat_params(rp).double().numpy(), masked, margin
    ref_losses, th32, masked, margin = oracle(ref, torch.float32)
    l64, th64, masked64, _ = oracle(ref64, torch.float64)
    n_steps = (M + batch - 1) // batch
    print(f"klpen trajectory {D}x{A} {hidden} actor_only={actor_only}: rows outside the bound {masked}, min |KL - bound| {margin:.2e}, "
          f"bound {kl_bound:.3e}")
    if not actor_only:
        assert all(0 < m < min(batch, M - k * batch) for k, m in enumerate(masked)), masked      # active on part of EVERY minibatch
        assert masked == masked64 and margin > 1e-6, (masked, masked64, margin)                  # no sample sits ON the bound
    losses = eng.learning_iter_ex(perm.to(torch.int32).to(dev), adv.to(dev).contiguous(), _abi.ACTOR_LOSS_KL_PENALTY, kl_bound,
                                  pg_coef, actor_only)
    got = losses.cpu().numpy()
    np.testing.assert_allclose(got[0], ref_losses[0], rtol=1e-5, atol=2e-6, equal_nan=True)      # first step: 1e-5
    cols = [2] if actor_only else [0, 1, 2]
    E.assert_loss_envelope(got[:, cols], ref_losses[:, cols], l64[:, cols], "KL-penalty pass on the row groups: losses", window=n_steps,
                           floor_rel=3e-6)
    E.assert_theta_envelope(pol.theta.cpu().numpy(), th32, th64, "KL-penalty pass on the row groups: theta",
                            floor_abs_max=E.theta_floor(3e-4, n_steps))
    if actor_only:
        off = pol.log_std_offset
        assert torch.equal(pol.theta[:off], theta0[:off])
        assert eng.adam_step == 0 and eng.adam_step_actor_extra == 5 + n_steps
    else:
        assert eng.adam_step == n_steps and eng.adam_step_actor_extra == 5


def test_klpen_row_group_path_is_chosen_from_the_shape(dev):
    """Outside the kernel's envelope the launch-per-network step stays: [1024, 1024, 512], more than 256 rows."""
    from safepo import _abi
    from safepo.common.engine import WidePPOLagEngine
    KL, CLIP = _abi.ACTOR_LOSS_KL_PENALTY, _abi.ACTOR_LOSS_CLIP
    for hidden, want in (([1024, 1024, 512], False), ([128, 128], True)):
        pol, _ = _wide_pair(60, 8, hidden, dev, seed=1)
        cfg = {"hidden_sizes": hidden, "gamma": 0.99, "target_kl": 1e9, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 40.0}
        eng = WidePPOLagEngine(pol, 1, 128, cfg, dev)
        for ao in (False, True):
            assert eng._row_group_step_ok(64, KL, ao) is want and eng._row_group_step_ok(257, KL, ao) is False
        assert eng._row_group_step_ok(64, CLIP, False) is want and eng._row_group_step_ok(64, CLIP, True) is False


def test_cup_first_stage_on_the_row_groups_vs_oracle(dev):
    """5. CUP's first stage (cup.py:300-351: the clipped surrogate on the reward advantage, all three networks) at [128, 128] takes
    the row-group path and matches KLPenaltyUpdater.minibatch_step under the envelopes of the KL-penalty trajectory test (the
    actor's clock 5 steps ahead, ragged last minibatch)."""
    import envelope as E
    from safepo import _abi
    D, A, hidden, M, batch = 60, 8, [128, 128], 214, 64
    pol, ref, eng, problem, *_ = _problem(D, A, hidden, M, batch, False, dev)
    obs, act, logp, tgt_r, tgt_c, _ = problem
    adv = torch.randn(M, generator=torch.Generator().manual_seed(41))             # (its own advantage array, not the buffer's)
    assert eng._row_group_step_ok(batch, _abi.ACTOR_LOSS_CLIP, False) is True
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(3))
    eng.adam_step_actor_extra = 5
    ref64 = copy.deepcopy(ref).double()

    def oracle(rp, dtype):
        upd = R.KLPenaltyUpdater(rp)
        for prm in rp.actor.parameters():
            upd.opt_a.state[prm] = {"step": torch.tensor(5.0), "exp_avg": torch.zeros_like(prm), "exp_avg_sq": torch.zeros_like(prm)}
        cols = [t.to(dtype) for t in (obs, act, logp, tgt_r, tgt_c, adv)]
        out = [upd.minibatch_step(*(t[perm[s0:s0 + batch]] for t in cols)) for s0 in range(0, M, batch)]
        return np.asarray(out, np.float64), R.flat_params(rp).double().numpy()
    ref_losses, th32 = oracle(ref, torch.float32)
    l64, th64 = oracle(ref64, torch.float64)
    losses = eng.learning_iter_ex(perm.to(torch.int32).to(dev), adv.to(dev).contiguous(), _abi.ACTOR_LOSS_CLIP)
    got = losses.cpu().numpy()
    n_steps = (M + batch - 1) // batch
    np.testing.assert_allclose(got[0], ref_losses[0], rtol=1e-5, atol=2e-6)
    E.assert_loss_envelope(got, ref_losses, l64, "CUP first stage on the row groups: losses", window=n_steps, floor_rel=3e-6)
    E.assert_theta_envelope(pol.theta.cpu().numpy(), th32, th64, "CUP first stage on the row groups: theta",
                            floor_abs_max=E.theta_floor(3e-4, n_steps))
    assert eng.adam_step == n_steps and eng.adam_step_actor_extra == 5


def _dp_shape_on_row_groups(dev, shape, rows):
    from safepo import _abi
    from safepo.common.engine import WidePPOLagEngine
    dims = [int(v) for v in shape.split(",")]
    pol, _ = _wide_pair(dims[0], dims[1], dims[2:], dev, seed=1)
    cfg = {"hidden_sizes": dims[2:], "gamma": 0.99, "target_kl": 1e9, "batch_size": rows, "learning_iters": 1, "max_grad_norm": 40.0}
    eng = WidePPOLagEngine(pol, 1, 4 * rows, cfg, dev)
    return all(eng._row_group_step_ok(rows, _abi.ACTOR_LOSS_KL_PENALTY, ao) for ao in (False, True)) and \
        eng._row_group_step_ok(rows, _abi.ACTOR_LOSS_CLIP, False)


def test_dp_cup_both_stages_on_the_row_groups(dev, tmp_path):
    """6. Two ranks on one GPU at 60 / 8, [128, 128] (tests/kl_penalty_dp_worker.py as it is): CUP's first stage on the clipped
    row-group launch with the all-reduce behind its group sum, the second stage on the KL-penalty launch with combine = 0, the
    all-reduce of [g | g_PG | sums] and spo_wide_kl_penalty_combine.  (The thresholds of _check_trajectory hold for this case on
    the launch-per-network step too: measured there at loss 2.4e-5, theta 5.4e-7.)"""
    from test_gpu_dp_kl_penalty import _check_trajectory, _run_worker
    shape = "60,8,128,128"
    assert _dp_shape_on_row_groups(dev, shape, 32)
    res = _run_worker(tmp_path, "0", shape, "cup")
    assert res["engine"] == "WidePPOLagEngine", res
    assert res["clocks"] == [[16, 5], [16, 21]], res
    assert res["critics_unchanged_stage2"], res
    assert res["stage1_theta_max_abs_diff"] < 1e-5, res
    _check_trajectory(res)


def test_dp_focops_shapes_take_the_row_groups(dev):
    """6. FOCOPS under two ranks on the KL-penalty launch is gated by the existing
    test_gpu_dp_kl_penalty.py::test_dp_focops_global_batch_equals_reference_minibatches: its three wide shapes take the row-group
    path at the 32 rows per rank it runs (asserted here).  A dp_batch = local case at 60 / 8, [128, 128] with 64 rows per rank is
    NOT added: _check_trajectory's fixed element-wise loss threshold (1e-4) has never been run at that case and the launch-per-network
    step misses it as well (actor loss column 1.37e-4 where the loss passes near 0, 1.4e-6 of the column's size; the row-group step
    1.08e-4), so it says nothing about this path."""
    for shape in ("100,20,64,64", "60,8,128,128", "376,17,64,64"):
        assert _dp_shape_on_row_groups(dev, shape, 32), shape
