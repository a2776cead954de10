"""GPU tests of the seed-batched PPO-Lagrangian path: S independent runs whose minibatch steps share one persistent launch of
the row-split kernel (spo_ppo_lag_update_iter_multi, csrc/update_rs.hip; safepo.common.engine_group).  The reference throughout
is today's one-run-per-launch path on the same machine -- PPOLagEngine.learning_iter / PPOLagEngine.update / the scripts'
`--seed` -- and the comparison is bit for bit: a run of a group IS the stand-alone run.  No test provokes a timeout of the
exchange."""
import argparse
import csv
import ctypes
import faulthandler
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_parity import _synthetic_update_problem, _fill_update_problem  # noqa: E402

TIME_LIMIT_S = 180
CFG = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "learning_iters": 1}
SHAPES = [(60, 8, 64), (12, 2, 64), (72, 2, 64), (5, 1, 20)]          # KIN 64 / 16 / 128, and a second row group without rows
S_MAX = 17
MAX_GRAD_NORM = 1.2
# The value targets and advantages of _synthetic_update_problem (N(0, 1), U(0, 1), N(0, 1)) times this.  As they come, the joint
# gradient norm of these six-step launches never gets under 1.2 at 60 / 8 and 72 / 2 (float32 oracle: 1.31 .. 7.4 and 1.27 .. 10.5
# over the 17 runs; none of 80 other seed triples at 60 / 8 has a step under the bound), so every step would be clipped and the
# unclipped path would go uncompared.  At 0.6 the oracle has 138 / 63 / 64 / 115 of the 204 / 204 / 204 / 170 steps of the four
# shapes above the bound, none within 9e-4 of it (relative): both kinds of step at every shape, already among the first three runs.
TARGET_SCALE = 0.6


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
    for k in ("SPO_RS_OBS128", "SPO_RS_SAFE", "SPO_FORCE_DP"):
        monkeypatch.delenv(k, raising=False)
    assert int(os.environ.get("SPO_UPDATE_FORM", "3")) >= 3, "SPO_UPDATE_FORM selects an older form in this process: unset it"


def _counters(lib, reset=1):
    from safepo import _abi
    c4 = (ctypes.c_ulonglong * 4)()
    _abi.check(lib.spo_debug_update_counters(c4, reset), "counters")
    return [int(x) for x in c4]


def _multi_counters(lib, reset=1):
    from safepo import _abi
    c2 = (ctypes.c_ulonglong * 2)()
    _abi.check(lib.spo_debug_rs_multi_counters(c2, reset), "multi counters")
    return [int(x) for x in c2]


def _rows(D, A, batch):
    return 100 if batch == 20 else 64 * 5 + 19                       # the final minibatch is ragged


def _engine(D, A, batch, r, dev):
    """Run r of a shape: its own initialisation, update problem and two shuffles."""
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    M = _rows(D, A, batch)
    torch.manual_seed(100 + r)
    pol = ActorVCritic(D, A).to(dev)
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    eng = PPOLagEngine(pol, 1, M, dict(CFG, batch_size=batch, max_grad_norm=MAX_GRAD_NORM), dev)
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=1000 + r)
    _fill_update_problem(eng, (obs, act, logp, TARGET_SCALE * tgt_r, TARGET_SCALE * tgt_c, TARGET_SCALE * adv))
    g = torch.Generator().manual_seed(50 + r)
    perms = [torch.randperm(M, generator=g).to(torch.int32).to(dev) for _ in range(2)]
    return eng, perms


def _state(eng):
    return eng.policy.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone()


_REFERENCE = {}


def _reference(shape, dev):
    """Per run r < S_MAX of a shape: (theta, m, v) after the first and after the second single launch, and the two loss logs --
    today's learning_iter, one run after the other.  Computed once per shape and left alone; a run does not depend on S."""
    if shape in _REFERENCE:
        return _REFERENCE[shape]
    from safepo import _abi
    lib = _abi.load()
    D, A, batch = shape
    nst = (_rows(*shape) + batch - 1) // batch
    _counters(lib)
    ref = []
    for r in range(S_MAX):
        eng, perms = _engine(D, A, batch, r, dev)
        l0 = eng.learning_iter(perms[0]).clone()
        s0 = _state(eng)
        l1 = eng.learning_iter(perms[1]).clone()
        eng.check_sync_error()
        ref.append({"after1": s0, "after2": _state(eng), "losses": (l0, l1)})
    c4 = _counters(lib)
    print(f"single launches at {shape}: steps {c4[0]}, clipped {c4[1]}")
    assert c4[0] == 2 * S_MAX * nst, (c4, nst)
    assert 0 < c4[1] < c4[0], c4                                    # the clip is active on part of the steps, at every shape
    for x in ref:
        assert all(torch.isfinite(t).all() for t in x["after2"]) and all(torch.isfinite(t).all() for t in x["losses"])
    _REFERENCE[shape] = ref
    return ref


def _assert_same(got, want, what):
    for name, x, y in zip(("theta", "adam_m", "adam_v"), got, want):
        assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} of {x.numel()} entries, max |d| {float((x - y).abs().max())}"


# ------------------------------------------------------------------------------------------------ 1. bit-exact against the single launch
@pytest.mark.parametrize("S", [1, 3, 9, 17])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batched_launch_is_bit_exact_against_single_launches(dev, shape, S):
    from safepo import _abi
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    D, A, batch = shape
    assert lib.spo_update_rs_multi_supported(D, A, batch, S) == 1
    ref = _reference(shape, dev)
    nst = (_rows(*shape) + batch - 1) // batch
    built = [_engine(D, A, batch, r, dev) for r in range(S)]
    group = PPOLagEngineGroup([e for e, _ in built])
    assert group.batched()
    for launch in range(2):
        _counters(lib); _multi_counters(lib)
        losses = group.learning_iter_all([p[launch] for _, p in built])
        group.check_sync_error()
        c4, c2 = _counters(lib), _multi_counters(lib)
        assert c4[0] == S * nst, (c4, S, nst)                       # the step counter sums over the runs
        assert c2[0] == S, c2                                       # ... and it was ONE launch of S runs, not S launches
        for r, (eng, _) in enumerate(built):
            assert eng.adam_step == (launch + 1) * nst
            assert torch.equal(losses[r], ref[r]["losses"][launch]), f"run {r} of {S}, launch {launch}: loss log"
            _assert_same(_state(eng), ref[r]["after1" if launch == 0 else "after2"], f"run {r} of {S}, launch {launch}")


def test_write_through_exchange_gives_the_same_bits(dev, monkeypatch):
    from safepo import _abi
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    shape, S = (60, 8, 64), 9
    ref = _reference(shape, dev)
    monkeypatch.setenv("SPO_RS_SAFE", "1")
    built = [_engine(*shape, r, dev) for r in range(S)]
    group = PPOLagEngineGroup([e for e, _ in built])
    _multi_counters(lib)
    for launch in range(2):
        losses = group.learning_iter_all([p[launch] for _, p in built])
        for r in range(S):
            assert torch.equal(losses[r], ref[r]["losses"][launch])
    group.check_sync_error()
    assert _multi_counters(lib) == [2 * S, 2 * S]                   # every run of both launches on the write-through path
    for r, (eng, _) in enumerate(built):
        _assert_same(_state(eng), ref[r]["after2"], f"SPO_RS_SAFE=1, run {r}")


# ------------------------------------------------------------------------------------------------ 2. inactive runs
def test_inactive_runs_are_untouched(dev):
    from safepo import _abi
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    shape, S, off = (60, 8, 64), 9, (1, 8)
    D, A, batch = shape
    M = _rows(*shape)
    nst = (M + batch - 1) // batch
    ref = _reference(shape, dev)
    built = [_engine(D, A, batch, r, dev) for r in range(S)]
    before = [_state(e) for e, _ in built]
    # through the C entry, with loss logs of our own: the inactive runs' stay as they were
    logs = [torch.full((nst, 3), -77.0, device=dev) for _ in range(S)]
    reps = (_abi.UpdateReplica * S)()
    for r, (e, perms) in enumerate(built):
        d, x = e.buffer.data, reps[r]
        x.theta, x.adam_m, x.adam_v, x.adam_step = _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v), 0
        x.obs, x.act, x.logp_old = _abi.ptr(d["obs"]), _abi.ptr(d["act"]), _abi.ptr(d["log_prob"])
        x.target_r, x.target_c, x.adv = _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(e.buffer.adv_mix)
        x.perm, x.losses_out, x.sync_ws = _abi.ptr(perms[0]), _abi.ptr(logs[r]), _abi.ptr(e.sync_ws)
        x.cfg, x.active = e._cfg_struct(), int(r not in off)
    _counters(lib); _multi_counters(lib)
    _abi.check(lib.spo_ppo_lag_update_iter_multi(reps, S, M, _abi.stream_ptr()), "spo_ppo_lag_update_iter_multi")
    torch.cuda.synchronize()
    assert _counters(lib)[0] == (S - len(off)) * nst and _multi_counters(lib)[0] == S - len(off)
    for r, (e, _) in enumerate(built):
        assert int(e.sync_ws[8].item()) == 0
        if r in off:
            _assert_same(_state(e), before[r], f"inactive run {r}")
            assert bool((logs[r] == -77.0).all()), f"inactive run {r}: loss log written"
        else:
            e.adam_step += nst
            _assert_same(_state(e), ref[r]["after1"], f"active run {r}")
            assert torch.equal(logs[r], ref[r]["losses"][0])
    # the second launch through the group, same runs sitting out
    group = PPOLagEngineGroup([e for e, _ in built])
    active = [r not in off for r in range(S)]
    losses = group.learning_iter_all([p[1] for _, p in built], active)
    group.check_sync_error()
    for r, (e, _) in enumerate(built):
        if r in off:
            assert losses[r] is None and e.adam_step == 0
            _assert_same(_state(e), before[r], f"inactive run {r}, second launch")
        else:
            assert e.adam_step == 2 * nst and torch.equal(losses[r], ref[r]["losses"][1])
            _assert_same(_state(e), ref[r]["after2"], f"active run {r}, second launch")


def test_all_inactive_and_refused_tables(dev):
    from safepo import _abi
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    built = [_engine(12, 2, 64, r, dev) for r in range(2)]
    before = [_state(e) for e, _ in built]
    group = PPOLagEngineGroup([e for e, _ in built])
    _counters(lib)
    assert group.learning_iter_all([p[0] for _, p in built], [False, False]) == [None, None]
    torch.cuda.synchronize()
    assert _counters(lib)[0] == 0
    for (e, _), b in zip(built, before):
        _assert_same(_state(e), b, "nothing active")
    # two runs on one parameter vector: refused, nothing launched
    built[1][0].policy.theta = built[0][0].policy.theta
    with pytest.raises(_abi.SpoError, match="share theta"):
        group.learning_iter_all([p[0] for _, p in built])
    assert _counters(lib)[0] == 0


# ------------------------------------------------------------------------------------------------ 3. the group's update
def _rollout_engine(i, dev, target_kl, learning_iters=4):
    """Run i of test 3: 3 envs x 64 steps of the synthetic device env behind it, ready for update()."""
    from safepo.common.engine import PPOLagEngine
    from safepo.common.env import SynthDeviceEnv
    from safepo.common.model import ActorVCritic
    D, A, N, T = 60, 8, 3, 64
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
    perms = [torch.randperm(N * T, generator=g).to(torch.int32).to(dev) for _ in range(learning_iters + 1)]
    return eng, (lambda it: perms[it])


def test_group_update_with_staggered_early_stops(dev):
    from safepo.common.engine_group import PPOLagEngineGroup
    lams, stops = [0.0, 0.3, 1.1], [1, 2, 4]
    # the KL after every pass of each stand-alone run, without early stopping
    targets = []
    for i in range(3):
        eng, perm_fn = _rollout_engine(i, dev, float("inf"))
        kls, read = [], eng.kl_read
        eng.kl_read = lambda: kls.append(read()) or kls[-1]
        out = eng.update(lams[i], perm_fn)
        assert out["stop_iter"] == 4 and len(kls) == 4
        print(f"run {i}: KL per pass {kls}")
        k = stops[i]
        lo = max(kls[:k - 1]) if k > 1 else 0.0
        assert lo < kls[k - 1], (i, kls)                            # (the pass that is to stop has the largest KL so far)
        targets.append(0.5 * (lo + kls[k - 1]))
    alone = []
    for i in range(3):
        eng, perm_fn = _rollout_engine(i, dev, targets[i])
        out = eng.update(lams[i], perm_fn)
        assert out["stop_iter"] == stops[i], (i, out["stop_iter"], targets[i])
        alone.append((out, _state(eng), eng.adam_step))
    built = [_rollout_engine(i, dev, targets[i]) for i in range(3)]
    group = PPOLagEngineGroup([e for e, _ in built])
    assert group.batched()
    outs = group.update(lams, [f for _, f in built])
    for i, ((eng, _), out, (aout, astate, astep)) in enumerate(zip(built, outs, alone)):
        assert out["stop_iter"] == aout["stop_iter"] == stops[i]
        assert out["kl"] == aout["kl"], (i, out["kl"], aout["kl"])
        assert (out["loss_r"], out["loss_c"], out["loss_pi"]) == (aout["loss_r"], aout["loss_c"], aout["loss_pi"])
        assert len(out["losses"]) == stops[i] and all(torch.equal(x, y) for x, y in zip(out["losses"], aout["losses"]))
        assert eng.adam_step == astep and eng.buffer.ptr == 0
        _assert_same(_state(eng), astate, f"group update, run {i}")


# ------------------------------------------------------------------------------------------------ 4. the scripts
SEEDS = [0, 1000, 2000]


def _args(log_dir, **kw):
    a = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=16, experiment="t", log_dir=str(log_dir), device="cuda",
                           device_id=0, write_terminal=True, headless=False, total_steps=3 * 16 * 64, steps_per_epoch=16 * 64,
                           randomize=False, cost_limit=25.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035,
                           cfg_override={"learning_iters": 3}, env_kwargs={"trunc_len": 16})
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _run_record(log_dir):
    rows = list(csv.DictReader(open(os.path.join(log_dir, "progress.csv"))))
    assert len(rows) == 3
    cols = [{k: v for k, v in row.items() if not k.startswith("Time/")} for row in rows]
    sd = torch.load(os.path.join(log_dir, "torch_save", "model0.pt"))
    return cols, sd


def _assert_same_run(a, b, what):
    assert a[0] == b[0], f"{what}: progress.csv differs: " + str([(k, x[k], y[k]) for x, y in zip(a[0], b[0]) for k in x if x[k] != y.get(k)][:6])
    assert set(a[1]) == set(b[1]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1]), f"{what}: saved actor differs"


@pytest.mark.parametrize("algo", ["ppo_lag", "pg"])
def test_scripts_with_seeds_equal_the_stand_alone_runs(dev, tmp_path, algo, capsys):
    import importlib
    mod = importlib.import_module(f"safepo.single_agent.{algo}")
    alone = {}
    for tag, seed in (("a", 0), ("again", 0), ("b", 1000), ("c", 2000)):
        d = tmp_path / f"alone_{tag}"
        mod.main(_args(d, seed=seed), {})
        alone[tag] = _run_record(d)
    _assert_same_run(alone["a"], alone["again"], "two stand-alone runs of seed 0")
    dirs = [str(tmp_path / f"group_{s}") for s in SEEDS]
    mod.main(_args(tmp_path / "unused", seeds=list(SEEDS), log_dirs=dirs), {})
    for d, tag, seed in zip(dirs, ("a", "b", "c"), SEEDS):
        _assert_same_run(_run_record(d), alone[tag], f"{algo} --seeds {SEEDS}: seed {seed}")
    capsys.readouterr()
    # the runs differ from each other (the comparison above is not between three copies of one run)
    assert alone["a"][0] != alone["b"][0] and alone["b"][0] != alone["c"][0]


def test_seeds_are_refused_for_wide_shapes(dev, tmp_path):
    from safepo.single_agent import ppo_lag
    a = _args(tmp_path / "x", seeds=[0, 1], cfg_override={"learning_iters": 1, "hidden_sizes": [96, 96]})
    with pytest.raises(SystemExit, match="wide-network"):
        ppo_lag.main(a, {})
