"""GPU tests of the seed-batched FOCOPS / CUP path: S independent runs whose minibatch steps share one persistent launch of the
four-wave kernel (spo_update_iter_ex_multi, csrc/update.hip; PPOLagEngineGroup.learning_iter_ex_all / update_focops / update_cup).
The reference throughout is today's one-run-per-launch path on the same machine -- PPOLagEngine.learning_iter_ex / update_focops /
update_cup / the scripts' `--seed` -- and the comparison is bit for bit: a run of a group IS the stand-alone run.  No test
provokes a timeout of the exchange.

The inputs of tests 1-3 are tests/klpen_batch_problem.py's: per (shape, mode) a max_grad_norm fixed from the float32 CPU oracle so
that between a quarter and three quarters of the steps clip and none lies within 1e-3 (relative) of the bound -- the speculative
Adam and the redone one are both compared -- and, for FOCOPS, a kl_bound and old means under which the indicator fraction lies
strictly between 0 and 1 on every step (the counts are stated there, entry by entry)."""
import argparse
import csv
import ctypes
import faulthandler
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import klpen_batch_problem as P  # noqa: E402

TIME_LIMIT_S = 180
CFG = {"hidden_sizes": [64, 64], "gamma": P.GAMMA, "target_kl": 1e9, "learning_iters": 1}
S_MAX = P.S_MAX


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
    monkeypatch.delenv("SPO_FORCE_DP", raising=False)
    assert int(os.environ.get("SPO_UPDATE_FORM", "3")) >= 3, "SPO_UPDATE_FORM selects an older form in this process: unset it"


def _multi_counters(lib, reset=1):
    from safepo import _abi
    c2 = (ctypes.c_ulonglong * 2)()
    _abi.check(lib.spo_debug_update_ex_multi_counters(c2, reset), "update_ex multi counters")
    return [int(x) for x in c2]


class _Run:
    """Run r of a (shape, mode) on the device: engine, its two shuffles, its advantage and the arguments of learning_iter_ex."""

    def __init__(self, shape, mode, r, dev):
        from safepo.common.engine import PPOLagEngine
        D, A, batch = shape
        p = P.make_run(shape, mode, r)
        M = p["M"]
        eng = PPOLagEngine(p["policy"].to(dev), 1, M, dict(CFG, batch_size=batch, max_grad_norm=p["max_grad_norm"]), dev)
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
        assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} of {x.numel()} entries, max |d| {float((x - y).abs().max())}"


_REFERENCE = {}


def _reference(shape, mode, dev):
    """Per run r < S_MAX of a (shape, mode): (theta, m, v) after the first and after the second single launch, and the two loss
    logs -- today's learning_iter_ex, one run after the other.  Computed once per case and left alone; a run does not depend on S."""
    key = (shape, mode)
    if key in _REFERENCE:
        return _REFERENCE[key]
    ref, moved = [], 0
    for r in range(S_MAX):
        run = _Run(shape, mode, r, dev)
        s_init = _state(run.eng)
        l0 = run.single(0).clone()
        s0 = _state(run.eng)
        l1 = run.single(1).clone()
        run.eng.check_sync_error()
        ref.append({"after1": s0, "after2": _state(run.eng), "losses": (l0, l1)})
        moved += int(not torch.equal(s_init[0], s0[0]))
    for x in ref:
        cols = [2] if P.MODES[mode][1] else [0, 1, 2]
        assert all(torch.isfinite(t).all() for t in x["after2"]) and all(torch.isfinite(t[:, cols]).all() for t in x["losses"])
    assert moved == S_MAX
    # the runs differ from each other (the comparisons below are not between copies of one run)
    assert not torch.equal(ref[0]["after2"][0], ref[1]["after2"][0]) and not _same_bits(ref[0]["losses"][0], ref[1]["losses"][0])
    _REFERENCE[key] = ref
    return ref


# ------------------------------------------------------------------------------------------------ 1. bit-exact against the single launch
@pytest.mark.parametrize("S", [1, 3, 9, 17])
@pytest.mark.parametrize("shape,mode", P.CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_batched_launch_is_bit_exact_against_single_launches(dev, shape, mode, S):
    from safepo import _abi
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    D, A, batch = shape
    actor_loss, actor_only = P.MODES[mode]
    assert lib.spo_update_ex_multi_supported(D, A, batch, actor_loss, S) == 1
    assert lib.spo_update_ex_multi_matches_single(D, A, batch, actor_loss) == 1
    ref = _reference(shape, mode, dev)
    nst = P.n_steps(shape)
    runs = [_Run(shape, mode, r, dev) for r in range(S)]
    group = PPOLagEngineGroup([x.eng for x in runs])
    assert group.batched_ex(actor_loss)
    for launch in range(2):
        _multi_counters(lib)
        losses = group.learning_iter_ex_all([x.perms[launch] for x in runs], [x.adv for x in runs], actor_loss,
                                            [x.kl_bound for x in runs], [x.pg_coef for x in runs], actor_only)
        group.check_sync_error()
        assert _multi_counters(lib) == [1, S]                       # ONE launch of S runs, not S launches
        for r, x in enumerate(runs):
            assert x.clocks() == x.want_clocks(launch + 1, nst)
            assert _same_bits(losses[r], ref[r]["losses"][launch]), f"run {r} of {S}, launch {launch}: loss log"
            _assert_same(_state(x.eng), ref[r]["after1" if launch == 0 else "after2"], f"run {r} of {S}, launch {launch}")


# ------------------------------------------------------------------------------------------------ 2. inactive runs
@pytest.mark.parametrize("mode", ["focops", "cup2"])
def test_inactive_runs_are_untouched(dev, mode):
    from safepo import _abi
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    shape, S, off = (60, 8, 64), 9, (1, 8)
    actor_loss, actor_only = P.MODES[mode]
    M, nst = P.rows(shape), P.n_steps(shape)
    ref = _reference(shape, mode, dev)
    runs = [_Run(shape, mode, r, dev) for r in range(S)]
    for r in off:                                                   # a pattern in the sitting-out runs' sync_ws (error word: 0)
        runs[r].eng.sync_ws.copy_(torch.arange(1, 33, device=dev) * 0x0101010101)
        runs[r].eng.sync_ws[8] = 0
    before = [_state(x.eng) for x in runs]
    ws_before = [x.eng.sync_ws.clone() for x in runs]
    # through the C entry, with loss logs of our own: the inactive runs' stay as they were
    logs = [torch.full((nst, 3), -77.0, device=dev) for _ in range(S)]
    reps = (_abi.UpdateExReplica * S)()
    for r, x in enumerate(runs):
        e, d, t = x.eng, x.eng.buffer.data, reps[r]
        t.theta, t.adam_m, t.adam_v = _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v)
        t.adam_step_critics, t.adam_step_actor = e.adam_step, e.adam_step + e.adam_step_actor_extra
        t.obs, t.act, t.logp_old = _abi.ptr(d["obs"]), _abi.ptr(d["act"]), _abi.ptr(d["log_prob"])
        t.target_r, t.target_c, t.adv = _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(x.adv)
        t.perm, t.old_mean, t.old_std = _abi.ptr(x.perms[0]), _abi.ptr(e.mean_old), _abi.ptr(e.std_old)
        t.kl_bound, t.pg_coef, t.losses_out, t.sync_ws = x.kl_bound, x.pg_coef, _abi.ptr(logs[r]), _abi.ptr(e.sync_ws)
        t.cfg, t.active = e._cfg_struct(), int(r not in off)
    _multi_counters(lib)
    _abi.check(lib.spo_update_iter_ex_multi(reps, S, M, actor_loss, int(actor_only), _abi.stream_ptr()), "spo_update_iter_ex_multi")
    torch.cuda.synchronize()
    assert _multi_counters(lib) == [1, S - len(off)]
    cols = [2] if actor_only else [0, 1, 2]
    for r, x in enumerate(runs):
        assert int(x.eng.sync_ws[8].item()) == 0
        if r in off:
            _assert_same(_state(x.eng), before[r], f"inactive run {r}")
            assert torch.equal(x.eng.sync_ws, ws_before[r]), f"inactive run {r}: sync_ws written"
            assert bool((logs[r] == -77.0).all()), f"inactive run {r}: loss log written"
        else:
            _assert_same(_state(x.eng), ref[r]["after1"], f"active run {r}")
            assert torch.equal(logs[r][:, cols], ref[r]["losses"][0][:, cols])
            if actor_only:
                x.eng.adam_step_actor_extra += nst
            else:
                x.eng.adam_step += nst
    # the second launch through the group, same runs sitting out
    group = PPOLagEngineGroup([x.eng for x in runs])
    active = [r not in off for r in range(S)]
    losses = group.learning_iter_ex_all([x.perms[1] for x in runs], [x.adv for x in runs], actor_loss, [x.kl_bound for x in runs],
                                        [x.pg_coef for x in runs], actor_only, active)
    group.check_sync_error()
    for r, x in enumerate(runs):
        if r in off:
            assert losses[r] is None and x.clocks() == x.want_clocks(0, nst)
            _assert_same(_state(x.eng), before[r], f"inactive run {r}, second launch")
            assert torch.equal(x.eng.sync_ws, ws_before[r])
        else:
            assert x.clocks() == x.want_clocks(2, nst) and _same_bits(losses[r], ref[r]["losses"][1])
            _assert_same(_state(x.eng), ref[r]["after2"], f"active run {r}, second launch")


# ------------------------------------------------------------------------------------------------ 3. refused and all-inactive tables
def test_all_inactive_and_refused_tables(dev):
    """Checked before device work: the runs' state and a sentinel buffer (their loss logs) stay untouched, the counters at zero."""
    from safepo import _abi
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    shape, mode = (12, 2, 64), "focops"
    runs = [_Run(shape, mode, r, dev) for r in range(2)]
    before = [_state(x.eng) for x in runs]
    group = PPOLagEngineGroup([x.eng for x in runs])
    args = ([x.perms[0] for x in runs], [x.adv for x in runs], 1, [x.kl_bound for x in runs], [x.pg_coef for x in runs], False)
    _multi_counters(lib)
    assert group.learning_iter_ex_all(*args, [False, False]) == [None, None]
    torch.cuda.synchronize()
    assert _multi_counters(lib, 0) == [0, 0]
    # through the C entry: a table that is refused touches neither the runs nor their loss logs
    M, nst = P.rows(shape), P.n_steps(shape)
    sentinel = [torch.full((nst, 3), -77.0, device=dev) for _ in runs]

    def table():
        reps = (_abi.UpdateExReplica * 2)()
        for r, x in enumerate(runs):
            e, d, t = x.eng, x.eng.buffer.data, reps[r]
            t.theta, t.adam_m, t.adam_v = _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v)
            t.adam_step_critics, t.adam_step_actor = e.adam_step, e.adam_step + e.adam_step_actor_extra
            t.obs, t.act, t.logp_old = _abi.ptr(d["obs"]), _abi.ptr(d["act"]), _abi.ptr(d["log_prob"])
            t.target_r, t.target_c, t.adv = _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(x.adv)
            t.perm, t.old_mean, t.old_std = _abi.ptr(x.perms[0]), _abi.ptr(e.mean_old), _abi.ptr(e.std_old)
            t.kl_bound, t.pg_coef, t.losses_out, t.sync_ws = x.kl_bound, x.pg_coef, _abi.ptr(sentinel[r]), _abi.ptr(e.sync_ws)
            t.cfg, t.active = e._cfg_struct(), 1
        return reps

    f, st = lib.spo_update_iter_ex_multi, _abi.stream_ptr()
    t = table(); t[1].theta = t[0].theta
    assert f(t, 2, M, 1, 0, st) < 0 and "share theta" in lib.spo_last_error().decode()
    t = table(); t[1].sync_ws = t[0].sync_ws
    assert f(t, 2, M, 1, 0, st) < 0 and "share" in lib.spo_last_error().decode()
    t = table(); t[1].old_mean = None
    assert f(t, 2, M, 1, 0, st) < 0 and "old distribution" in lib.spo_last_error().decode()
    t = table(); t[0].target_c = None
    assert f(t, 2, M, 1, 0, st) < 0 and "critic targets" in lib.spo_last_error().decode()
    t = table(); t[1].cfg.batch = 32
    assert f(t, 2, M, 1, 0, st) < 0 and "replica 1" in lib.spo_last_error().decode()
    t = table(); t[0].cfg.batch = t[1].cfg.batch = 65
    assert f(t, 2, M, 1, 0, st) < 0 and "> 64" in lib.spo_last_error().decode()
    assert f(table(), 0, M, 1, 0, st) < 0 and f(table(), 33, M, 1, 0, st) < 0 and f(table(), 2, M, 7, 0, st) < 0
    t = table(); t[0].active = t[1].active = 0
    assert f(t, 2, M, 1, 0, st) == 0
    torch.cuda.synchronize()
    assert _multi_counters(lib) == [0, 0]
    for x, b, s in zip(runs, before, sentinel):
        _assert_same(_state(x.eng), b, "refused tables")
        assert bool((s == -77.0).all()) and int(x.eng.sync_ws[8].item()) == 0
    # ... and through the group: two runs on one parameter vector
    runs[1].eng.policy.theta = runs[0].eng.policy.theta
    with pytest.raises(_abi.SpoError, match="share theta"):
        group.learning_iter_ex_all(*args)
    assert _multi_counters(lib) == [0, 0]


# ------------------------------------------------------------------------------------------------ 4. the group's updates
def _rollout_engine(i, D, A, dev, target_kl, learning_iters):
    """Run i of test 4: 3 envs x 64 steps of the synthetic device env behind it, ready for update_focops / update_cup."""
    from safepo.common.engine import PPOLagEngine
    from safepo.common.env import SynthDeviceEnv
    from safepo.common.model import ActorVCritic
    N, T = 3, 64
    torch.manual_seed(300 + i)
    pol = ActorVCritic(D, A).to(dev)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": target_kl, "batch_size": 64, "learning_iters": learning_iters,
           "max_grad_norm": 40.0}
    eng = PPOLagEngine(pol, N, T, cfg, dev)
    env = SynthDeviceEnv(N, D, A, seed=7 + i, p_term=0.02, p_cost=0.1, trunc_len=10, device=dev, normalize_obs=True,
                         obs_scale=2.0, obs_shift=0.5)
    rms = env.fuse_normalize(True)
    obs, _ = env.reset()
    eng.rollout_epoch(env, obs, rms=rms)
    eng.drain_episode_events(None)
    g = torch.Generator().manual_seed(900 + i)
    perms = [torch.randperm(N * T, generator=g).to(torch.int32).to(dev) for _ in range(2 * 4 + 1)]
    return eng, (lambda it: perms[it])


LAMS = [0.0, 0.3, 1.1, 0.6]
ITERS = [4, 3, 4, 1]             # learning_iters per run; runs 0 and 1 additionally get a target_kl that stops them early


def _pass_kls(update, i, D, A, dev):
    """The KL after every pass of stand-alone run i with its learning_iters and no KL stop."""
    eng, perm_fn = _rollout_engine(i, D, A, dev, 1e9, ITERS[i])
    kls, read = [], eng.kl_read
    eng.kl_read = lambda: kls.append(read()) or kls[-1]
    update(eng, LAMS[i], perm_fn)
    return kls


def _compare_group_update(name, D, A, dev, targets, expect_batched):
    from safepo import _abi
    from safepo.common.engine import PPOLagEngine
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    update = getattr(PPOLagEngine, name)
    alone = []
    for i in range(4):
        eng, perm_fn = _rollout_engine(i, D, A, dev, targets[i], ITERS[i])
        out = update(eng, LAMS[i], perm_fn)
        alone.append((out, _state(eng), (eng.adam_step, eng.adam_step_actor_extra)))
    built = [_rollout_engine(i, D, A, dev, targets[i], ITERS[i]) for i in range(4)]
    group = PPOLagEngineGroup([e for e, _ in built])
    _multi_counters(lib)
    outs = getattr(group, name)(LAMS, [f for _, f in built])
    c2 = _multi_counters(lib)
    stages = [("stop_iter", "losses")] + ([("second_stage_stop_iter", "second_stage_losses")] if name == "update_cup" else [])
    # one launch per pass of every batched stage, a run taking part in as many as it has passes
    want = [sum(max(a[0][k] for a in alone) for (k, _), b in zip(stages, expect_batched) if b),
            sum(a[0][k] for a in alone for (k, _), b in zip(stages, expect_batched) if b)]
    assert c2 == want, (c2, want)
    for i, ((eng, _), out, (aout, astate, aclocks)) in enumerate(zip(built, outs, alone)):
        assert set(out) == set(aout)
        for k in ("kl", "loss_r", "loss_c", "loss_pi") + (("kl_first_stage",) if name == "update_cup" else ()):
            assert out[k] == aout[k] or (out[k] != out[k] and aout[k] != aout[k]), (i, k, out[k], aout[k])
        for k_stop, k_loss in stages:
            assert out[k_stop] == aout[k_stop], (i, k_stop, out[k_stop], aout[k_stop])
            assert len(out[k_loss]) == out[k_stop] and all(_same_bits(x, y) for x, y in zip(out[k_loss], aout[k_loss])), (i, k_loss)
        assert (eng.adam_step, eng.adam_step_actor_extra) == aclocks and eng.buffer.ptr == 0
        _assert_same(_state(eng), astate, f"group {name}, run {i}")
    return [a[0] for a in alone]


def test_group_update_focops_with_staggered_early_stops(dev):
    from safepo.common.engine import PPOLagEngine
    D, A = 60, 8
    # target_kl is also FOCOPS's per-row KL bound, so a run's KLs depend on it: run 0 gets half its first pass's unbounded KL,
    # run 1 the middle of its first two; runs 2 and 3 never stop on the KL and run their 4 passes / 1 pass
    k0, k1 = (_pass_kls(PPOLagEngine.update_focops, i, D, A, dev) for i in (0, 1))
    targets = [0.5 * k0[0], 0.5 * (k1[0] + k1[1]), 1e9, 1e9]
    alone = _compare_group_update("update_focops", D, A, dev, targets, [True])
    stops = [o["stop_iter"] for o in alone]
    print(f"FOCOPS: unbounded KLs {k0} / {k1}, targets {targets[:2]}, stops {stops}")
    assert stops[2:] == [4, 1] and len(set(stops)) >= 2               # the runs stop at different passes


@pytest.mark.parametrize("D,A,first_stage_batched", [(72, 2, True), (60, 8, False)])
def test_group_update_cup_with_staggered_early_stops(dev, D, A, first_stage_batched):
    """At 72 observations both stages are one launch per pass; at 60 the stand-alone first stage runs the main + helper kernel,
    so the group runs that stage engine by engine and batches the second."""
    from safepo import _abi
    from safepo.common.engine import PPOLagEngine
    assert bool(_abi.load().spo_update_ex_multi_matches_single(D, A, 64, 0)) == first_stage_batched
    # CUP's target_kl only stops: the first stage's KLs are those of the run without a stop up to the pass that stops
    k0, k1 = (_pass_kls(PPOLagEngine.update_cup, i, D, A, dev) for i in (0, 1))
    assert k0[0] > 0 and k1[0] < k1[1], (k0, k1)
    targets = [0.5 * k0[0], 0.5 * (k1[0] + k1[1]), 1e9, 1e9]
    alone = _compare_group_update("update_cup", D, A, dev, targets, [first_stage_batched, True])
    stops = [(o["stop_iter"], o["second_stage_stop_iter"]) for o in alone]
    print(f"CUP at {D} / {A}: first-stage KLs {k0[:ITERS[0]]} / {k1[:ITERS[1]]}, targets {targets[:2]}, stops {stops}")
    assert [s[0] for s in stops] == [1, 2, 4, 1]                       # staggered in the first stage ...
    assert stops[2][1] == 4 and stops[3][1] == 1                       # ... and in the second (runs 0 and 1: where their KL says)


# ------------------------------------------------------------------------------------------------ 5. the scripts
SEEDS = [0, 1000, 2000]


def _args(log_dir, **kw):
    a = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=16, experiment="t", log_dir=str(log_dir), device="cuda",
                           device_id=0, write_terminal=True, headless=False, total_steps=2 * 16 * 64, steps_per_epoch=16 * 64,
                           randomize=False, cost_limit=25.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035,
                           cfg_override={"learning_iters": 3}, env_kwargs={"trunc_len": 16}, batch_update=False)
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


@pytest.mark.parametrize("algo", ["focops", "cup"])
def test_scripts_with_seeds_equal_the_stand_alone_runs(dev, tmp_path, algo, capsys):
    import importlib
    mod = importlib.import_module(f"safepo.single_agent.{algo}")
    alone = {}
    for tag, seed in (("a", 0), ("b", 1000), ("c", 2000)):
        d = tmp_path / f"alone_{tag}"
        mod.main(_args(d, seed=seed), {})
        alone[tag] = _run_record(d)
    dirs = [str(tmp_path / f"group_{s}") for s in SEEDS]
    with pytest.raises(SystemExit, match="--batch-update True"):        # without the flag: today's refusal
        mod.main(_args(tmp_path / "unused", seeds=list(SEEDS), log_dirs=dirs), {})
    mod.main(_args(tmp_path / "unused", seeds=list(SEEDS), log_dirs=dirs, batch_update=True), {})
    for d, tag, seed in zip(dirs, ("a", "b", "c"), SEEDS):
        rec = _run_record(d)
        _assert_same_run(rec, alone[tag], f"{algo} --seeds {SEEDS} --batch-update True: seed {seed}")
        assert ("Train/SeconStageStopIter" in rec[0][0]) == (algo == "cup")
    capsys.readouterr()
    # the runs differ from each other (the comparison above is not between three copies of one run)
    assert alone["a"][0] != alone["b"][0] and alone["b"][0] != alone["c"][0]


def test_seeds_are_refused_for_wide_shapes(dev, tmp_path):
    from safepo.single_agent import focops
    a = _args(tmp_path / "x", seeds=[0, 1], batch_update=True, cfg_override={"learning_iters": 1, "hidden_sizes": [96, 96]})
    with pytest.raises(SystemExit, match="wide-network"):
        focops.main(a, {})
