"""GPU tests of the seed-batched feature-split update: S independent runs at HumanoidVelocity-class dims whose minibatch steps
share one launch of the feature-split kernel (spo_update_iter_ex_ks_multi, csrc/update_ks.hip; PPOLagEngineGroup of
WidePPOLagEngines; the scripts' --batch-wide-obs).  The reference throughout is the one-run-per-launch path on the same machine --
spo_update_iter_ex_ks through WidePPOLagEngine.learning_iter_ex, the engine's update / update_focops / update_cup, the scripts'
`--seed` -- and the comparison is bit for bit: a run of a group IS the stand-alone run.  No tolerances; the single launch itself is
gated against the fp64 yardstick by the existing suites.  No test provokes a timeout of the exchange.

The inputs of tests 1-3 are tests/ks_batch_problem.py's: per (shape, mode) a max_grad_norm fixed from the float32 CPU oracle so
that between a quarter and three quarters of the steps clip and none lies within 1e-3 (relative) of the bound, and, for FOCOPS, a
kl_bound under which the indicator fraction lies strictly between 0 and 1 on every step (the counts are stated there)."""
import argparse
import csv
import ctypes
import faulthandler
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import ks_batch_problem as P  # noqa: E402

TIME_LIMIT_S = 180
CFG = {"hidden_sizes": [64, 64], "gamma": P.GAMMA, "target_kl": 1e9, "learning_iters": 1}
HUMANOID = (376, 17, 64)


@pytest.fixture(autouse=True)
def _time_limit_and_global_state():
    threads, rng = torch.get_num_threads(), torch.get_rng_state()
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()
    torch.set_num_threads(threads)
    torch.set_rng_state(rng)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_routing(monkeypatch):
    monkeypatch.delenv("SPO_KS_SAFE", raising=False)
    assert os.environ.get("SPO_WIDE_KS", "1") != "0", "SPO_WIDE_KS=0 takes the feature-split kernel away in this process: unset it"


def _counters(lib, reset=1):
    """{launches enqueued, runs that took part, of those: runs on write-through stores} since the last reset."""
    from safepo import _abi
    c3 = (ctypes.c_ulonglong * 3)()
    _abi.check(lib.spo_debug_update_ks_multi_counters(c3, reset), "update_ks multi counters")
    return [int(x) for x in c3]


class _Run:
    """Run r of a (shape, mode) on the device: engine, its two shuffles, its advantage and the arguments of learning_iter_ex."""

    def __init__(self, shape, mode, r, dev):
        from safepo.common.engine import WidePPOLagEngine
        D, A, batch = shape
        p = P.make_run(shape, mode, r)
        M = p["M"]
        eng = WidePPOLagEngine(p["policy"].to(dev), 1, M, dict(CFG, batch_size=batch, max_grad_norm=p["max_grad_norm"]), dev)
        assert eng._feature_split_kernel_ok(eng._cfg_struct())
        b = eng.buffer
        b.data["obs"].view(-1, D).copy_(p["obs"]); b.data["act"].view(-1, A).copy_(p["act"])
        b.data["log_prob"].view(-1).copy_(p["logp"]); b.data["target_value_r"].view(-1).copy_(p["tgt_r"])
        b.data["target_value_c"].view(-1).copy_(p["tgt_c"])
        eng.mean_old.copy_(p["old_mean"]); eng.std_old.copy_(p["old_std"])
        eng.lr_factor, eng.adam_step, eng.adam_step_actor_extra = p["lr_factor"], p["step_c"], p["step_a_extra"]
        self.eng, self.adv = eng, p["adv"].to(dev).contiguous()
        self.perms = [x.to(torch.int32).to(dev) for x in p["perms"]]
        self.actor_loss, self.actor_only = P.MODES[mode]
        self.kl_bound, self.pg_coef = p["kl_bound"], p["pg_coef"]
        self.step_c, self.step_a_extra = p["step_c"], p["step_a_extra"]

    def single(self, launch):
        """spo_update_iter_ex_ks: the stand-alone launch."""
        return self.eng.learning_iter_ex(self.perms[launch], self.adv, self.actor_loss, self.kl_bound, self.pg_coef, self.actor_only)

    def clocks(self):
        return self.eng.adam_step, self.eng.adam_step_actor_extra

    def want_clocks(self, launches, nst):
        return (self.step_c, self.step_a_extra + launches * nst) if self.actor_only else (self.step_c + launches * nst, self.step_a_extra)


def _state(eng):
    return eng.policy.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone()


def _same_bits(x, y):
    """torch.equal on the bit patterns (an actor-only launch leaves NaN in the critics' loss columns)."""
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _assert_same(got, want, what):
    for name, x, y in zip(("theta", "adam_m", "adam_v"), got, want):
        assert _same_bits(x, y), f"{what}: {name} differs in {int((x != y).sum())} of {x.numel()} entries, max |d| {float((x - y).abs().max())}"


_REFERENCE = {}


def _reference(shape, mode, dev, n=None, safe=False):
    """Per run r < n (default: as many as a launch takes at this shape) of a (shape, mode): (theta, m, v) after the first and after
    the second single launch, and the two loss logs -- spo_update_iter_ex_ks, one run after the other.  Computed once per case and
    left alone; a run does not depend on the number of runs beside it."""
    n = P.max_runs(shape) if n is None else n
    key = (shape, mode, safe)
    ref = _REFERENCE.setdefault(key, [])
    for r in range(len(ref), n):
        run = _Run(shape, mode, r, dev)
        s_init = _state(run.eng)
        l0 = run.single(0).clone()
        s0 = _state(run.eng)
        l1 = run.single(1).clone()
        run.eng.check_sync_error()
        cols = [2] if P.MODES[mode][1] else [0, 1, 2]
        assert all(torch.isfinite(t).all() for t in _state(run.eng)) and all(torch.isfinite(t[:, cols]).all() for t in (l0, l1))
        assert not torch.equal(s_init[0], s0[0])
        ref.append({"after1": s0, "after2": _state(run.eng), "losses": (l0, l1)})
    # the runs differ from each other (the comparisons below are not between copies of one run)
    if n > 1:
        assert not torch.equal(ref[0]["after2"][0], ref[1]["after2"][0]) and not _same_bits(ref[0]["losses"][0], ref[1]["losses"][0])
    return ref


def _batched_against_single(dev, shape, mode, S, safe=False):
    from safepo import _abi
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    D, A, batch = shape
    actor_loss, actor_only = P.MODES[mode]
    assert lib.spo_update_ks_multi_supported(D, A, batch, S) == 1
    ref = _reference(shape, mode, dev, S, safe)
    nst = P.n_steps(shape)
    runs = [_Run(shape, mode, r, dev) for r in range(S)]
    group = PPOLagEngineGroup([x.eng for x in runs])
    assert group.batched_ex(actor_loss) and group.batched()
    for launch in range(2):
        _counters(lib)
        losses = group.learning_iter_ex_all([x.perms[launch] for x in runs], [x.adv for x in runs], actor_loss,
                                            [x.kl_bound for x in runs], [x.pg_coef for x in runs], actor_only)
        group.check_sync_error()                                        # no error word is set
        assert all(int(x.eng.sync_ws[8].item()) == 0 for x in runs)
        # ONE launch of S runs, not S launches; write-through stores only where SPO_KS_SAFE asks for them
        assert _counters(lib) == [1, S, S if safe else 0]
        for r, x in enumerate(runs):
            assert x.clocks() == x.want_clocks(launch + 1, nst)
            assert _same_bits(losses[r], ref[r]["losses"][launch]), f"run {r} of {S}, launch {launch}: loss log"
            _assert_same(_state(x.eng), ref[r]["after1" if launch == 0 else "after2"], f"run {r} of {S}, launch {launch}")


# ------------------------------------------------------------------------------------------------ 1. bit-exact against the single launch
# every (shape, mode) at 1, 3 and 8 runs, and at 9 and 16 where a launch takes that many (up to 256 observations)
BIT_EXACT_CASES = [(shape, mode, S) for shape, mode in P.CASES for S in P.REPLICAS if S <= P.max_runs(shape)]


@pytest.mark.parametrize("shape,mode,S", BIT_EXACT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_batched_launch_is_bit_exact_against_single_launches(dev, shape, mode, S):
    _batched_against_single(dev, shape, mode, S)


@pytest.mark.parametrize("mode", ["clip", "focops", "cup2"])
def test_batched_launch_is_bit_exact_under_write_through_stores(dev, monkeypatch, mode):
    """SPO_KS_SAFE=1 (read at every launch): the exchange on write-through stores, single launches under the same setting; every
    run of the batched launch reports the write-through path."""
    monkeypatch.setenv("SPO_KS_SAFE", "1")
    _batched_against_single(dev, HUMANOID, mode, 3, safe=True)


# ------------------------------------------------------------------------------------------------ 2. inactive runs
GUARD = 64              # floats (or words) of guard pattern on either side


def _guarded(t, pattern):
    """A copy of t in the middle of a buffer filled with `pattern` -> (the whole buffer, the view that holds the copy)."""
    buf = torch.full((t.numel() + 2 * GUARD,), pattern, dtype=t.dtype, device=t.device)
    inner = buf[GUARD:GUARD + t.numel()].view(t.shape)
    inner.copy_(t)
    return buf, inner


def _fill(t, x, e, perm, losses, theta=None, adam_m=None, adam_v=None, sync_ws=None, active=1):
    from safepo import _abi
    d = e.buffer.data
    t.theta = _abi.ptr(e.policy.theta if theta is None else theta)
    t.adam_m, t.adam_v = _abi.ptr(e.adam_m if adam_m is None else adam_m), _abi.ptr(e.adam_v if adam_v is None else adam_v)
    t.adam_step_critics, t.adam_step_actor = e.adam_step, e.adam_step + e.adam_step_actor_extra
    t.obs, t.act, t.logp_old = _abi.ptr(d["obs"]), _abi.ptr(d["act"]), _abi.ptr(d["log_prob"])
    t.target_r, t.target_c, t.adv = _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(x.adv)
    t.perm, t.old_mean, t.old_std = _abi.ptr(perm), _abi.ptr(e.mean_old), _abi.ptr(e.std_old)
    t.kl_bound, t.pg_coef, t.losses_out = x.kl_bound, x.pg_coef, _abi.ptr(losses)
    t.sync_ws = _abi.ptr(e.sync_ws if sync_ws is None else sync_ws)
    t.cfg, t.active = e._cfg_struct(), active


@pytest.mark.parametrize("mode", ["clip", "focops", "cup2"])
def test_inactive_runs_are_untouched(dev, mode):
    from safepo import _abi
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    shape, S, off = HUMANOID, 3, 1
    actor_loss, actor_only = P.MODES[mode]
    M, nst = P.rows(shape), P.n_steps(shape)
    ref = _reference(shape, mode, dev, S)
    runs = [_Run(shape, mode, r, dev) for r in range(S)]
    # the run that sits out: its parameters, moments, loss log and sync_ws in guarded buffers of our own
    e = runs[off].eng
    g_theta, g_m, g_v = _guarded(e.policy.theta, -3.5), _guarded(e.adam_m, -4.5), _guarded(e.adam_v, -5.5)
    g_loss = _guarded(torch.full((nst, 3), -77.0, device=dev), -6.5)
    ws = torch.arange(1, 33, device=dev) * 0x0101010101
    ws[8] = 0
    g_ws = _guarded(ws, 0x7E7E7E7E7E7E)
    kept = [b.clone() for b, _ in (g_theta, g_m, g_v, g_loss, g_ws)]
    logs = [torch.full((nst, 3), -77.0, device=dev) for _ in range(S)]
    reps = (_abi.UpdateExReplica * S)()
    for r, x in enumerate(runs):
        if r == off:
            _fill(reps[r], x, x.eng, x.perms[0], g_loss[1], g_theta[1], g_m[1], g_v[1], g_ws[1], active=0)
        else:
            _fill(reps[r], x, x.eng, x.perms[0], logs[r])
    _counters(lib)
    _abi.check(lib.spo_update_iter_ex_ks_multi(reps, S, M, actor_loss, int(actor_only), _abi.stream_ptr()), "spo_update_iter_ex_ks_multi")
    torch.cuda.synchronize()
    assert _counters(lib) == [1, S - 1, 0]
    for (buf, _), k, what in zip((g_theta, g_m, g_v, g_loss, g_ws), kept, ("theta", "adam_m", "adam_v", "loss log", "sync_ws")):
        assert _same_bits(buf.view(-1), k.view(-1)) if buf.dtype == torch.float32 else torch.equal(buf, k), f"inactive run: {what} or its guards written"
    cols = [2] if actor_only else [0, 1, 2]
    for r, x in enumerate(runs):
        if r == off:
            continue
        assert int(x.eng.sync_ws[8].item()) == 0
        _assert_same(_state(x.eng), ref[r]["after1"], f"active run {r}")
        assert torch.equal(logs[r][:, cols], ref[r]["losses"][0][:, cols])
        if actor_only:
            x.eng.adam_step_actor_extra += nst
        else:
            x.eng.adam_step += nst
    # the second launch through the group, the same run sitting out
    before = _state(runs[off].eng)
    ws_before = runs[off].eng.sync_ws.clone()
    group = PPOLagEngineGroup([x.eng for x in runs])
    active = [r != off for r in range(S)]
    losses = group.learning_iter_ex_all([x.perms[1] for x in runs], [x.adv for x in runs], actor_loss, [x.kl_bound for x in runs],
                                        [x.pg_coef for x in runs], actor_only, active)
    group.check_sync_error()
    for r, x in enumerate(runs):
        if r == off:
            assert losses[r] is None and x.clocks() == x.want_clocks(0, nst)
            _assert_same(_state(x.eng), before, "inactive run, second launch")
            assert torch.equal(x.eng.sync_ws, ws_before)
        else:
            assert x.clocks() == x.want_clocks(2, nst) and _same_bits(losses[r], ref[r]["losses"][1])
            _assert_same(_state(x.eng), ref[r]["after2"], f"active run {r}, second launch")


# ------------------------------------------------------------------------------------------------ 3. refused and all-inactive tables
def test_all_inactive_and_refused_tables(dev):
    """Checked before device work: the runs' state and a sentinel buffer (their loss logs) stay untouched, the launch counter too."""
    from safepo import _abi
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    shape, mode = HUMANOID, "focops"
    runs = [_Run(shape, mode, r, dev) for r in range(2)]
    before = [_state(x.eng) for x in runs]
    group = PPOLagEngineGroup([x.eng for x in runs])
    args = ([x.perms[0] for x in runs], [x.adv for x in runs], 1, [x.kl_bound for x in runs], [x.pg_coef for x in runs], False)
    _counters(lib)
    assert group.learning_iter_ex_all(*args, [False, False]) == [None, None]
    torch.cuda.synchronize()
    assert _counters(lib, 0) == [0, 0, 0]
    M, nst = P.rows(shape), P.n_steps(shape)
    sentinel = [torch.full((nst, 3), -77.0, device=dev) for _ in runs]

    def table(n=2, obs_dim=None):
        """n entries; those beyond the two real runs repeat them (such tables are refused before a pointer is looked at)."""
        reps = (_abi.UpdateExReplica * n)()
        for r in range(n):
            x = runs[r % 2]
            _fill(reps[r], x, x.eng, x.perms[0], sentinel[r % 2])
            if obs_dim is not None:
                reps[r].cfg.obs_dim = obs_dim
        return reps

    f, st = lib.spo_update_iter_ex_ks_multi, _abi.stream_ptr()
    err = lambda: lib.spo_last_error().decode()          # noqa: E731
    t = table(); t[0].active = t[1].active = 0
    assert f(t, 2, M, 1, 0, st) == 0                                           # all runs inactive: nothing enqueued
    assert f(table(9), 9, M, 1, 0, st) != 0 and "at most 8 runs" in err()       # 9 runs at 376 observations
    assert f(table(17, 192), 17, M, 1, 0, st) != 0 and "17 replicas outside [1, 16]" in err()      # 17 at 192
    t = table(); t[1].cfg.obs_dim = 192
    assert f(t, 2, M, 1, 0, st) != 0 and "replica 1 has obs_dim" in err()       # unequal shapes
    t = table(); t[1].theta = t[0].theta
    assert f(t, 2, M, 1, 0, st) != 0 and "share theta" in err()
    t = table(); t[1].sync_ws = t[0].sync_ws
    assert f(t, 2, M, 1, 0, st) != 0 and "share theta or sync_ws" in err()
    t = table(); t[1].old_mean = None
    assert f(t, 2, M, 1, 0, st) != 0 and "old distribution is NULL" in err()    # the KL penalty needs the old distribution
    t = table(); t[0].target_c = None
    assert f(t, 2, M, 1, 0, st) != 0 and "critic targets are NULL" in err()     # without actor_only the critics need targets
    # a stream under capture (captured, never replayed)
    torch.cuda.synchronize()
    x = torch.zeros(8, device=dev)
    graph = torch.cuda.CUDAGraph()
    t = table()
    with torch.cuda.graph(graph):
        x.add_(1.0)
        rc = f(t, 2, M, 1, 0, _abi.stream_ptr())
        msg = err()
    torch.cuda.synchronize()
    assert rc != 0 and "under capture" in msg, (rc, msg)
    assert _counters(lib) == [0, 0, 0]
    for x_, b, s in zip(runs, before, sentinel):
        _assert_same(_state(x_.eng), b, "refused tables")
        assert bool((s == -77.0).all()) and int(x_.eng.sync_ws[8].item()) == 0
    # ... and through the group: two runs on one parameter vector
    runs[1].eng.policy.theta = runs[0].eng.policy.theta
    with pytest.raises(_abi.SpoError, match="share theta"):
        group.learning_iter_ex_all(*args)
    assert _counters(lib) == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ 4. the group's updates
D_H, A_H = 376, 17
LAMS = [0.0, 0.3, 1.1]
ITERS = [4, 3, 2]                # learning_iters per run; runs 0 and 1 additionally get a target_kl that can stop them early


def _rollout_engine(i, dev, target_kl, learning_iters):
    """Run i of test 4: 16 envs x 16 steps of the synthetic device env behind a WidePPOLagEngine, ready for an update."""
    from safepo.common.engine import WidePPOLagEngine
    from safepo.common.env import SynthDeviceEnv
    from safepo.common.model import ActorVCritic
    N, T = 16, 16
    torch.manual_seed(300 + i)
    pol = ActorVCritic(D_H, A_H).to(dev)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": target_kl, "batch_size": 64, "learning_iters": learning_iters,
           "max_grad_norm": 40.0}
    eng = WidePPOLagEngine(pol, N, T, cfg, dev)
    env = SynthDeviceEnv(N, D_H, A_H, seed=7 + i, p_term=0.02, p_cost=0.1, trunc_len=10, device=dev, normalize_obs=True,
                         obs_scale=2.0, obs_shift=0.5)
    rms = env.fuse_normalize(True)
    obs, _ = env.reset()
    eng.rollout_epoch(env, obs, rms=rms)
    eng.drain_episode_events(None)
    g = torch.Generator().manual_seed(900 + i)
    perms = [torch.randperm(N * T, generator=g).to(torch.int32).to(dev) for _ in range(2 * 4 + 1)]
    return eng, (lambda it: perms[it])


def _pass_kls(update, i, dev):
    """The KL after every pass of stand-alone run i with its learning_iters and no KL stop."""
    eng, perm_fn = _rollout_engine(i, dev, 1e9, ITERS[i])
    kls, read = [], eng.kl_read
    eng.kl_read = lambda: kls.append(read()) or kls[-1]
    update(eng, LAMS[i], perm_fn)
    return kls


def _compare_group_update(name, dev, targets):
    from safepo import _abi
    from safepo.common.engine import WidePPOLagEngine
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    update = getattr(WidePPOLagEngine, name)
    alone = []
    for i in range(3):
        eng, perm_fn = _rollout_engine(i, dev, targets[i], ITERS[i])
        out = update(eng, LAMS[i], perm_fn)
        alone.append((out, _state(eng), (eng.adam_step, eng.adam_step_actor_extra)))
    built = [_rollout_engine(i, dev, targets[i], ITERS[i]) for i in range(3)]
    group = PPOLagEngineGroup([e for e, _ in built])
    assert group.batched() and group.batched_ex(0) and group.batched_ex(1)
    _counters(lib)
    outs = getattr(group, name)(LAMS, [f for _, f in built])
    c3 = _counters(lib)
    stages = [("stop_iter", "losses")] + ([("second_stage_stop_iter", "second_stage_losses")] if name == "update_cup" else [])
    # one launch per pass of every stage, a run taking part in as many as it has passes
    want = [sum(max(a[0][k] for a in alone) for k, _ in stages), sum(a[0][k] for a in alone for k, _ in stages), 0]
    assert c3 == want, (c3, want)
    for i, ((eng, _), out, (aout, astate, aclocks)) in enumerate(zip(built, outs, alone)):
        assert set(out) == set(aout)
        for k in ("kl", "loss_r", "loss_c", "loss_pi") + (("kl_first_stage",) if name == "update_cup" else ()):
            assert out[k] == aout[k] or (out[k] != out[k] and aout[k] != aout[k]), (i, k, out[k], aout[k])
        for k_stop, k_loss in stages:
            assert out[k_stop] == aout[k_stop], (i, k_stop, out[k_stop], aout[k_stop])
            assert len(out[k_loss]) == out[k_stop] and all(_same_bits(x, y) for x, y in zip(out[k_loss], aout[k_loss])), (i, k_loss)
        assert (eng.adam_step, eng.adam_step_actor_extra) == aclocks and eng.buffer.ptr == 0
        _assert_same(_state(eng), astate, f"group {name}, run {i}")
    assert not torch.equal(alone[0][1][0], alone[1][1][0])
    return [a[0] for a in alone]


def _staggered_targets(name, dev):
    """Run 0 gets half its first pass's unstopped KL (it stops after one pass), run 1 the middle of its first two; run 2 never
    stops on the KL and runs its 2 passes."""
    from safepo.common.engine import WidePPOLagEngine
    k0, k1 = (_pass_kls(getattr(WidePPOLagEngine, name), i, dev) for i in (0, 1))
    assert k0[0] > 0 and k1[0] > 0, (k0, k1)
    return [0.5 * k0[0], 0.5 * (k1[0] + k1[1]), 1e9], (k0, k1)


def test_group_update_ppo_with_staggered_early_stops(dev):
    targets, kls = _staggered_targets("update", dev)
    alone = _compare_group_update("update", dev, targets)
    stops = [o["stop_iter"] for o in alone]
    print(f"PPO-Lagrangian at {D_H} / {A_H}: unstopped KLs {kls}, targets {targets[:2]}, stops {stops}")
    assert stops[0] == 1 and stops[2] == 2 and len(set(stops)) >= 2            # the runs stop at different passes


def test_group_update_focops_with_staggered_early_stops(dev):
    # (target_kl is also FOCOPS's per-row KL bound, so a run's KLs depend on it: the stops are where the stand-alone runs stop)
    targets, kls = _staggered_targets("update_focops", dev)
    alone = _compare_group_update("update_focops", dev, targets)
    stops = [o["stop_iter"] for o in alone]
    print(f"FOCOPS at {D_H} / {A_H}: unbounded KLs {kls}, targets {targets[:2]}, stops {stops}")
    assert stops[2] == 2 and len(set(stops)) >= 2


def test_group_update_cup_with_staggered_early_stops(dev):
    """Both stages of CUP are one launch per pass at these dims (the stand-alone run has no other kernel for either)."""
    targets, kls = _staggered_targets("update_cup", dev)
    alone = _compare_group_update("update_cup", dev, targets)
    stops = [(o["stop_iter"], o["second_stage_stop_iter"]) for o in alone]
    print(f"CUP at {D_H} / {A_H}: first-stage KLs {kls}, targets {targets[:2]}, stops {stops}")
    assert stops[0][0] == 1 and stops[2] == (2, 2) and len({s[0] for s in stops}) >= 2


# ------------------------------------------------------------------------------------------------ 5. the scripts
SEEDS = [0, 1000, 2000]


def _args(log_dir, **kw):
    a = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=16, experiment="t", log_dir=str(log_dir), device="cuda",
                           device_id=0, write_terminal=True, headless=False, total_steps=2 * 16 * 64, steps_per_epoch=16 * 64,
                           randomize=False, cost_limit=25.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035,
                           cfg_override={"learning_iters": 3}, env_kwargs={"obs_dim": D_H, "act_dim": A_H, "trunc_len": 16},
                           batch_update=False, batch_wide_obs=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _run_record(log_dir):
    rows = list(csv.DictReader(open(os.path.join(log_dir, "progress.csv"))))
    assert len(rows) == 2
    cols = [{k: v for k, v in row.items() if not k.startswith("Time/")} for row in rows]
    sd = torch.load(os.path.join(log_dir, "torch_save", "model0.pt"))
    return cols, sd


def _assert_same_run(a, b, what):
    assert a[0] == b[0], f"{what}: progress.csv differs: " + str([(k, x[k], y[k]) for x, y in zip(a[0], b[0]) for k in x if x[k] != y.get(k)][:6])
    assert set(a[1]) == set(b[1]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1]), f"{what}: saved actor differs"


@pytest.mark.parametrize("algo", ["ppo_lag", "focops", "cup"])
def test_scripts_with_seeds_equal_the_stand_alone_runs(dev, tmp_path, algo, capsys):
    import importlib
    from safepo import _abi
    lib = _abi.load()
    mod = importlib.import_module(f"safepo.single_agent.{algo}")
    klpen = algo != "ppo_lag"
    alone = {}
    for tag, seed in (("a", 0), ("b", 1000), ("c", 2000)):
        d = tmp_path / f"alone_{tag}"
        mod.main(_args(d, seed=seed), {})
        alone[tag] = _run_record(d)
    dirs = [str(tmp_path / f"group_{s}") for s in SEEDS]
    with pytest.raises(SystemExit, match="wide-network"):                # without --batch-wide-obs True: today's refusal
        mod.main(_args(tmp_path / "unused", seeds=list(SEEDS), log_dirs=dirs, batch_update=klpen), {})
    assert not any(os.path.exists(d) for d in dirs)
    _counters(lib)
    mod.main(_args(tmp_path / "unused", seeds=list(SEEDS), log_dirs=dirs, batch_update=klpen, batch_wide_obs=True), {})
    c3 = _counters(lib)
    assert c3[0] >= 2 and c3[1] > c3[0] and c3[2] == 0, c3                # the updates ran as shared launches
    for d, tag, seed in zip(dirs, ("a", "b", "c"), SEEDS):
        rec = _run_record(d)
        _assert_same_run(rec, alone[tag], f"{algo} --seeds {SEEDS} --batch-wide-obs True: seed {seed}")
        assert ("Train/SeconStageStopIter" in rec[0][0]) == (algo == "cup")
    capsys.readouterr()
    # the runs differ from each other (the comparison above is not between three copies of one run)
    assert alone["a"][0] != alone["b"][0] and alone["b"][0] != alone["c"][0]


def test_refusals(dev, tmp_path):
    from safepo.single_agent import focops, ppo_lag
    # hidden sizes other than [64, 64] stay refused, flag or no flag
    a = _args(tmp_path / "x", seeds=[0, 1], batch_wide_obs=True, cfg_override={"learning_iters": 1, "hidden_sizes": [96, 96]})
    with pytest.raises(SystemExit, match="wide-network"):
        ppo_lag.main(a, {})
    # nine seeds at 376 observations: more than a launch takes there, refused before any log directory is written
    seeds = [1000 * i for i in range(9)]
    dirs = [str(tmp_path / f"nine_{s}") for s in seeds]
    with pytest.raises(SystemExit, match="at most 8 seeds"):
        ppo_lag.main(_args(tmp_path / "nine", seeds=seeds, log_dirs=dirs, batch_wide_obs=True), {})
    assert not any(os.path.exists(d) for d in dirs) and not os.path.exists(tmp_path / "nine")
    # focops / cup: the flag widens --batch-update True
    with pytest.raises(SystemExit, match="give both"):
        focops.main(_args(tmp_path / "y", seeds=[0, 1], batch_wide_obs=True), {})
    assert not os.path.exists(tmp_path / "y")
