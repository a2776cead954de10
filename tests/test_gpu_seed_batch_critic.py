"""GPU tests of the seed-batched critic fit: S independent critic fits (the second-order scripts' cpo.py:534-571 loop) whose
minibatch steps share one persistent launch of the four-row-group row-split kernel (spo_critic_fit_iter_multi,
csrc/update_rs.hip; safepo.common.engine_group.CPOEngineGroup).  The reference throughout is today's one-run-per-launch path on
the same machine -- spo_critic_fit_iter / CPOEngine.critic_fit / the scripts' `--seed` -- on copies of the same state, and the
comparison is bit for bit: parameters, both Adam moments, stale_sq_io and the [n_mb, 3] loss log.  No tolerance anywhere.  No
test provokes a timeout of the exchange."""
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
CFG = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 0.01, "learning_iters": 1}
# (D, A, batch, M): the smallest shapes at which the four-row-group form can go wrong --
#   KIN 64, the tail minibatch (70 rows) leaves row group 2 with 6 rows and group 3 empty;
#   KIN 16, 100-row minibatches: group 3 has 4 rows;
#   KIN 32, 65-row minibatches: group 2 has one row, group 3 none; the tail is 3 rows.
SHAPES = [(60, 8, 128, 3 * 128 + 70), (12, 2, 100, 3 * 100), (20, 1, 65, 3 * 65 + 3)]
S_MAX = 17
# So that some steps clip and some do not: the float32 oracle (oracle/restatement.CriticFitter on these very problems, the 17
# runs, two passes) has joint norms of 0.71 .. 1.58 / 0.67 .. 1.72 / 0.45 .. 3.76 at the three shapes with 54 of 136 / 39 of 102 /
# 80 of 136 steps above this bound, both kinds already among the first three runs.  The stale actor gradient (||.||^2 = 0.5 at
# the start) is part of that norm, and every clipped step rescales it: the joint clip's write to stale_sq_io is exercised.
MAX_GRAD_NORM = 1.0
TARGET_SCALE = 0.6                  # the value targets of _synthetic_update_problem times this, as in test_gpu_seed_batch.py
STALE_SQ0 = 0.5
SENTINEL = -77.0


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
    for k in ("SPO_RS_SAFE", "SPO_CPO_SPLIT", "SPO_RS_ROWS"):
        monkeypatch.delenv(k, raising=False)
    assert int(os.environ.get("SPO_UPDATE_FORM", "3")) >= 3, "SPO_UPDATE_FORM selects an older form in this process: unset it"


def _counters(lib, reset=1):
    from safepo import _abi
    c4 = (ctypes.c_ulonglong * 4)()
    _abi.check(lib.spo_debug_update_counters(c4, reset), "counters")
    return [int(x) for x in c4]


def _critic_counters(lib, reset=1):
    from safepo import _abi
    c2 = (ctypes.c_ulonglong * 2)()
    _abi.check(lib.spo_debug_rs_critic_multi_counters(c2, reset), "critic multi counters")
    return [int(x) for x in c2]


def _ppo_multi_counters(lib, reset=0):
    from safepo import _abi
    c2 = (ctypes.c_ulonglong * 2)()
    _abi.check(lib.spo_debug_rs_multi_counters(c2, reset), "multi counters")
    return [int(x) for x in c2]


def _engine(shape, r, dev, learning_iters=1):
    """Run r of a shape: its own initialisation, critic-fit problem, stale actor-gradient norm and two shuffles."""
    from safepo.common.model import ActorVCritic
    from safepo.single_agent.cpo import CPOEngine
    D, A, batch, M = shape
    torch.manual_seed(100 + r)
    pol = ActorVCritic(D, A).to(dev)
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    eng = CPOEngine(pol, 1, M, dict(CFG, batch_size=batch, max_grad_norm=MAX_GRAD_NORM, learning_iters=learning_iters), dev)
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=1000 + r)
    _fill_update_problem(eng, (obs, act, logp, TARGET_SCALE * tgt_r, TARGET_SCALE * tgt_c, adv))
    eng.stale_sq.fill_(STALE_SQ0 + 0.01 * r)
    g = torch.Generator().manual_seed(50 + r)
    perms = [torch.randperm(M, generator=g).to(torch.int32).to(dev) for _ in range(max(2, learning_iters))]
    return eng, perms


def _state(eng):
    return eng.policy.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.stale_sq.clone()


def _n_mb(shape):
    return (shape[3] + shape[2] - 1) // shape[2]


def _single_iter(lib, eng, perm, shape):
    """One spo_critic_fit_iter launch -- today's path -- with a sentinel-filled [n_mb, 3] log."""
    from safepo import _abi
    d = eng.buffer.data
    log = torch.full((_n_mb(shape), 3), SENTINEL, device=eng.dev)
    _abi.check(lib.spo_critic_fit_iter(
        _abi.ptr(eng.policy.theta), _abi.ptr(eng.adam_m), _abi.ptr(eng.adam_v), eng.adam_step, _abi.ptr(d["obs"]),
        _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(perm), eng.M, eng._cfg_struct(),
        _abi.ptr(eng.stale_sq), _abi.ptr(log), _abi.ptr(eng.sync_ws), _abi.stream_ptr()), "spo_critic_fit_iter")
    eng.adam_step += _n_mb(shape)
    return log


def _table(engs, perms, logs, active=None):
    from safepo import _abi
    S = len(engs)
    reps = (_abi.CriticFitReplica * S)()
    for r, e in enumerate(engs):
        d, x = e.buffer.data, reps[r]
        x.theta, x.adam_m, x.adam_v, x.adam_step = _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v), e.adam_step
        x.obs, x.target_r, x.target_c = _abi.ptr(d["obs"]), _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"])
        x.perm, x.losses_out, x.stale_sq_io = _abi.ptr(perms[r]), _abi.ptr(logs[r]), _abi.ptr(e.stale_sq)
        x.sync_ws, x.cfg, x.active = _abi.ptr(e.sync_ws), e._cfg_struct(), int(active is None or active[r])
    return reps


def _multi_iter(lib, engs, perms, shape, active=None):
    """One spo_critic_fit_iter_multi launch with sentinel-filled logs."""
    from safepo import _abi
    logs = [torch.full((_n_mb(shape), 3), SENTINEL, device=e.dev) for e in engs]
    _abi.check(lib.spo_critic_fit_iter_multi(_table(engs, perms, logs, active), len(engs), engs[0].M, _abi.stream_ptr()),
               "spo_critic_fit_iter_multi")
    for r, e in enumerate(engs):
        if active is None or active[r]:
            e.adam_step += _n_mb(shape)
    return logs


_REFERENCE = {}


def _reference(shape, dev):
    """Per run r < S_MAX of a shape: the state after the first and after the second single launch and the two loss logs.
    Computed once per shape and left alone; a run does not depend on S."""
    if shape in _REFERENCE:
        return _REFERENCE[shape]
    from safepo import _abi
    lib = _abi.load()
    assert lib.spo_critic_fit_multi_matches_single(*shape[:3]) == 1     # the single launch IS the four-row-group form here
    _counters(lib)
    ref = []
    for r in range(S_MAX):
        eng, perms = _engine(shape, r, dev)
        stale0 = eng.stale_sq.clone()
        l0 = _single_iter(lib, eng, perms[0], shape)
        s0 = _state(eng)
        l1 = _single_iter(lib, eng, perms[1], shape)
        eng.check_sync_error()
        ref.append({"stale0": stale0, "after1": s0, "after2": _state(eng), "losses": (l0, l1)})
    c4 = _counters(lib)
    print(f"single launches at {shape}: steps {c4[0]}, clipped {c4[1]}")
    assert c4[0] == 2 * S_MAX * _n_mb(shape), (c4, shape)
    assert 0 < c4[1] < c4[0], c4                                    # the clip is active on part of the steps, at every shape
    for x in ref:
        assert all(torch.isfinite(t).all() for t in x["after2"])
        assert all(torch.isfinite(t[:, :2]).all() and bool((t[:, 2] == SENTINEL).all()) for t in x["losses"])
    # the clip rescaled the stale norm (stale_sq_io is written, not only read), and not in every run alike
    assert any(not torch.equal(x["after2"][3], x["stale0"]) for x in ref)
    assert len({float(x["after2"][3]) / float(x["stale0"]) for x in ref}) > 1
    _REFERENCE[shape] = ref
    return ref


def _assert_same(got, want, what):
    for name, x, y in zip(("theta", "adam_m", "adam_v", "stale_sq"), got, want):
        assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} of {x.numel()} entries, max |d| {float((x - y).abs().max())}"


# ------------------------------------------------------------------------------------------------ 1. bit-exact against the single launch
@pytest.mark.parametrize("S", [1, 3, 9, 17])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batched_launch_is_bit_exact_against_single_launches(dev, shape, S):
    from safepo import _abi
    lib = _abi.load()
    assert lib.spo_critic_fit_multi_supported(*shape[:3], S) == 1
    ref = _reference(shape, dev)
    nst = _n_mb(shape)
    built = [_engine(shape, r, dev) for r in range(S)]
    engs = [e for e, _ in built]
    ppo_before = _ppo_multi_counters(lib)
    for launch in range(2):
        _counters(lib); _critic_counters(lib)
        logs = _multi_iter(lib, engs, [p[launch] for _, p in built], shape)
        torch.cuda.synchronize()
        c4, c2 = _counters(lib), _critic_counters(lib)
        print(f"{shape} S {S} launch {launch}: runs {c2[0]}, on the write-through path {c2[1]}")      # (reported, not asserted)
        assert c4[0] == S * nst, (c4, S, nst)                       # the step counter sums over the runs
        assert c2[0] == S, c2                                       # ... and it was ONE launch of S runs
        for r, e in enumerate(engs):
            assert int(e.sync_ws[8].item()) == 0, f"run {r}: error word set"
            assert torch.equal(logs[r], ref[r]["losses"][launch]), f"run {r} of {S}, launch {launch}: loss log"
            _assert_same(_state(e), ref[r]["after1" if launch == 0 else "after2"], f"run {r} of {S}, launch {launch}")
    assert _ppo_multi_counters(lib) == ppo_before                   # the PPO form's counters do not see these launches


def test_write_through_exchange_gives_the_same_bits(dev, monkeypatch):
    from safepo import _abi
    lib = _abi.load()
    shape, S = SHAPES[0], 9
    ref = _reference(shape, dev)
    monkeypatch.setenv("SPO_RS_SAFE", "1")                           # (read at every launch)
    built = [_engine(shape, r, dev) for r in range(S)]
    engs = [e for e, _ in built]
    _critic_counters(lib)
    for launch in range(2):
        logs = _multi_iter(lib, engs, [p[launch] for _, p in built], shape)
        for r in range(S):
            assert torch.equal(logs[r], ref[r]["losses"][launch])
    torch.cuda.synchronize()
    assert _critic_counters(lib) == [2 * S, 2 * S]                  # every run of both launches on the write-through path
    for r, e in enumerate(engs):
        assert int(e.sync_ws[8].item()) == 0
        _assert_same(_state(e), ref[r]["after2"], f"SPO_RS_SAFE=1, run {r}")


# ------------------------------------------------------------------------------------------------ 2. inactive runs, refusals
def test_inactive_runs_are_untouched(dev):
    from safepo import _abi
    lib = _abi.load()
    shape, S, off = SHAPES[0], 9, (1, 8)
    ref = _reference(shape, dev)
    built = [_engine(shape, r, dev) for r in range(S)]
    engs = [e for e, _ in built]
    for r in off:                                                   # sentinel-filled state: must stay sentinel
        e = engs[r]
        for t in (e.policy.theta, e.adam_m, e.adam_v, e.stale_sq):
            t.fill_(SENTINEL)
        e.sync_ws.fill_(0x5A5A5A5A)
    active = [r not in off for r in range(S)]
    _counters(lib); _critic_counters(lib)
    logs = _multi_iter(lib, engs, [p[0] if a else None for (_, p), a in zip(built, active)], shape, active)
    torch.cuda.synchronize()
    assert _counters(lib)[0] == (S - len(off)) * _n_mb(shape) and _critic_counters(lib)[0] == S - len(off)
    for r, e in enumerate(engs):
        if r in off:
            assert all(bool((t == SENTINEL).all()) for t in _state(e)), f"inactive run {r}: state written"
            assert bool((e.sync_ws == 0x5A5A5A5A).all()), f"inactive run {r}: sync_ws written"
            assert bool((logs[r] == SENTINEL).all()) and e.adam_step == 0
        else:
            assert int(e.sync_ws[8].item()) == 0
            _assert_same(_state(e), ref[r]["after1"], f"active run {r}")
            assert torch.equal(logs[r], ref[r]["losses"][0])


def test_all_inactive_and_refused_tables(dev):
    from safepo import _abi
    lib = _abi.load()
    shape = SHAPES[1]
    built = [_engine(shape, r, dev) for r in range(3)]
    engs, perms = [e for e, _ in built], [p[0] for _, p in built]
    before = [_state(e) for e in engs]
    logs = [torch.full((_n_mb(shape), 3), SENTINEL, device=dev) for _ in engs]
    f = lib.spo_critic_fit_iter_multi
    _counters(lib); _critic_counters(lib)

    def refused(table, n, match):
        assert f(table, n, engs[0].M, _abi.stream_ptr()) < 0
        assert match in lib.spo_last_error().decode(), lib.spo_last_error().decode()

    assert f(_table(engs, perms, logs, [False] * 3), 3, engs[0].M, _abi.stream_ptr()) == 0          # nothing active: nothing enqueued
    refused(_table(engs, perms, logs), 0, "replicas outside")
    t = (_abi.CriticFitReplica * 25)(*([_table(engs, perms, logs)[0]] * 25))
    refused(t, 25, "replicas outside")
    for field in ("theta", "sync_ws", "stale_sq_io"):
        t = _table(engs, perms, logs)
        setattr(t[2], field, getattr(t[1], field))
        refused(t, 3, "replicas 1 and 2 share theta, sync_ws or stale_sq_io")
    t = _table(engs, perms, logs)
    t[1].cfg.batch = 128
    refused(t, 3, "replica 1 has obs_dim / act_dim / batch")
    t = _table(engs, perms, logs)
    for x in t:
        x.cfg.batch = 64                                            # two row groups in the single launch: not batched here
    refused(t, 3, "no replica-batched form")
    t = _table(engs, perms, logs)
    t[0].losses_out = None
    refused(t, 3, "null pointer in replica 0")
    torch.cuda.synchronize()
    assert _counters(lib)[0] == 0 and _critic_counters(lib) == [0, 0]                                # no launch left behind
    for e, b, log in zip(engs, before, logs):
        _assert_same(_state(e), b, "refused tables")
        assert bool((log == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ 3. the group
def test_group_critic_fit_all_against_per_engine_critic_fit(dev):
    from safepo import _abi
    from safepo.common.engine_group import CPOEngineGroup
    lib = _abi.load()
    shape, n_its = SHAPES[0], (1, 3, 2, 3)
    alone = []
    for r, n in enumerate(n_its):
        eng, perms = _engine(shape, r, dev, learning_iters=n)
        out = eng.critic_fit(lambda it, p=perms: p[it])
        alone.append((out, _state(eng), eng.adam_step))
    built = [_engine(shape, r, dev, learning_iters=n) for r, n in enumerate(n_its)]
    group = CPOEngineGroup([e for e, _ in built])
    assert group.batched()
    _critic_counters(lib)
    outs = group.critic_fit_all([(lambda it, p=perms: p[it]) for _, perms in built])
    torch.cuda.synchronize()
    assert _critic_counters(lib)[0] == sum(n_its)                   # max(n_its) launches, a finished run sitting out
    for r, ((eng, _), out, (aout, astate, astep)) in enumerate(zip(built, outs, alone)):
        assert (out["loss_r"], out["loss_c"]) == (aout["loss_r"], aout["loss_c"]), r
        assert len(out["losses"]) == n_its[r] and all(torch.equal(x, y) for x, y in zip(out["losses"], aout["losses"]))
        assert eng.adam_step == astep == n_its[r] * _n_mb(shape)
        _assert_same(_state(eng), astate, f"critic_fit_all, run {r}")
    # minibatches up to 64 rows run two row groups in the single launch: not batched, every engine fits on its own
    assert not CPOEngineGroup([_engine((60, 8, 64, 128), r, dev)[0] for r in range(2)]).batched()


def test_group_leaves_the_split_form_to_the_engines(dev, monkeypatch):
    """SPO_CPO_SPLIT=force: the engines take their two-replica split form, so the group fits them one by one -- the same
    results as each engine's own critic_fit under that setting."""
    from safepo import _abi
    from safepo.common.engine_group import CPOEngineGroup
    lib = _abi.load()
    shape = (60, 8, 128, 256)
    assert CPOEngineGroup([_engine(shape, r, dev)[0] for r in range(2)]).batched()                   # (default routing: batched)
    monkeypatch.setenv("SPO_CPO_SPLIT", "force")
    alone = []
    for r in range(2):
        eng, perms = _engine(shape, r, dev, learning_iters=2)
        out = eng.critic_fit(lambda it, p=perms: p[it])
        alone.append((out, _state(eng)))
    built = [_engine(shape, r, dev, learning_iters=2) for r in range(2)]
    group = CPOEngineGroup([e for e, _ in built])
    assert not group.batched()
    _critic_counters(lib)
    outs = group.critic_fit_all([(lambda it, p=p: p[it]) for _, p in built])
    torch.cuda.synchronize()
    assert _critic_counters(lib) == [0, 0]                          # no batched launch
    for r, ((eng, _), out, (aout, astate)) in enumerate(zip(built, outs, alone)):
        assert (out["loss_r"], out["loss_c"]) == (aout["loss_r"], aout["loss_c"]) and len(out["losses"]) == 2
        _assert_same(_state(eng), astate, f"split form, run {r}")


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


@pytest.mark.parametrize("algo", ["cpo", "trpo_lag"])
def test_scripts_with_seeds_equal_the_stand_alone_runs(dev, tmp_path, algo, capsys):
    import importlib
    from safepo import _abi
    lib = _abi.load()
    mod = importlib.import_module(f"safepo.single_agent.{algo}")
    alone = {}
    for tag, seed in (("a", 0), ("b", 1000), ("c", 2000)):
        d = tmp_path / f"alone_{tag}"
        mod.main(_args(d, seed=seed), {})
        alone[tag] = _run_record(d)
    dirs = [str(tmp_path / f"group_{s}") for s in SEEDS]
    _critic_counters(lib)
    mod.main(_args(tmp_path / "unused", seeds=list(SEEDS), log_dirs=dirs, batch_critic_fit=True), {})
    assert _critic_counters(lib)[0] == 3 * 3 * 3                    # seeds x epochs x iterations went through the batched launch
    for d, tag, seed in zip(dirs, ("a", "b", "c"), SEEDS):
        _assert_same_run(_run_record(d), alone[tag], f"{algo} --seeds {SEEDS} --batch-critic-fit True: seed {seed}")
    capsys.readouterr()
    # the runs differ from each other (the comparison above is not between three copies of one run)
    assert alone["a"][0] != alone["b"][0] and alone["b"][0] != alone["c"][0]
    # without the flag: refused as before
    with pytest.raises(SystemExit, match="second-order"):
        mod.main(_args(tmp_path / "unused2", seeds=list(SEEDS)), {})


def test_seeds_are_refused_for_wide_shapes(dev, tmp_path):
    from safepo.single_agent import cpo, trpo_lag
    a = _args(tmp_path / "x", seeds=[0, 1], batch_critic_fit=True, env_kwargs={"trunc_len": 16, "obs_dim": 72})
    with pytest.raises(SystemExit, match="wide-network"):
        cpo.main(a, {})
    a = _args(tmp_path / "y", seeds=[0, 1], batch_critic_fit=True, cfg_override={"learning_iters": 1, "hidden_sizes": [96, 96]})
    with pytest.raises(SystemExit, match="wide-network"):
        trpo_lag.main(a, {})
