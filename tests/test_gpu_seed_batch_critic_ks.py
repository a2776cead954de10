"""GPU tests of the seed-batched feature-split critic fit: S independent runs of the second-order scripts at 129-512
observations whose critic fits share one launch of the feature-split kernel per iteration (spo_critic_fit_iter_ks_multi,
csrc/update_ks.hip; CPOEngineGroup(ks_form=True) of WideCPOEngines; the scripts' --batch-critic-fit-feature-split).  The reference
throughout is the one-run-per-launch path on the same machine -- spo_critic_fit_iter_ks from the same start,
WideCPOEngine.critic_fit, the scripts' `--seed` -- and every comparison is torch.equal: a run of a batched launch IS the
stand-alone run.  No tolerances; the single launch itself is gated against the fp64 yardstick by the existing suites.  No test
provokes a timeout of the exchange (the error path of the group is tested on the CPU with a stand-in).

The inputs are tests/critic_ks_batch_problem.py's: rows M = 5 * batch + 7 (a ragged last minibatch), per-run learning rates and
max_grad_norm such that run 0 clips and run 1 never does (asserted here on stale_sq_io, and with the float32 oracle on the CPU in
test_seed_batch_critic_ks_host.py)."""
import argparse
import csv
import ctypes
import faulthandler
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import critic_ks_batch_problem as P  # noqa: E402

TIME_LIMIT_S = 180
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
    monkeypatch.delenv("SPO_KS_SAFE", raising=False)
    assert os.environ.get("SPO_WIDE_KS", "1") != "0", "SPO_WIDE_KS=0 takes the feature-split kernel away in this process: unset it"


def _counters(lib, reset=1):
    """{launches enqueued, runs that took part, of those: runs on write-through stores} since the last reset."""
    from safepo import _abi
    c3 = (ctypes.c_ulonglong * 3)()
    _abi.check(lib.spo_debug_critic_fit_ks_multi_counters(c3, reset), "critic_fit_ks multi counters")
    return [int(x) for x in c3]


def _first_order_counters(lib):
    from safepo import _abi
    c3 = (ctypes.c_ulonglong * 3)()
    _abi.check(lib.spo_debug_update_ks_multi_counters(c3, 0), "update_ks multi counters")
    return [int(x) for x in c3]


_CPU = {}


def _cpu_problem(shape, r, batch):
    """Run r's start on the CPU, built once per (shape, r, batch) and left alone."""
    key = (shape, r, batch)
    if key not in _CPU:
        pol = P.make_policy(shape, r)
        theta = pol.theta.detach().clone()
        g = torch.Generator().manual_seed(7000 + r)
        # (moments of a fit under way: non-zero, the second one positive)
        m = 1e-3 * torch.randn(theta.numel(), generator=g)
        v = 1e-5 * torch.rand(theta.numel(), generator=g)
        _CPU[key] = (theta, m, v, pol.log_std_offset, P.make_rows(shape, r, batch), P.make_perms(r, batch))
    return _CPU[key]


class _Run:
    """Run r of a (shape, batch) on the device: parameters, moments, rows, shuffles, stale norm, clock, cfg, sync_ws."""

    def __init__(self, shape, batch, r, dev):
        from safepo import _abi
        D, A = shape
        theta, m, v, ls_off, (obs, tgt_r, tgt_c), perms = _cpu_problem(shape, r, batch)
        self.theta, self.m, self.v = theta.to(dev), m.to(dev), v.to(dev)
        self.theta0, self.ls_off = self.theta.clone(), ls_off
        self.obs, self.tgt_r, self.tgt_c = obs.to(dev), tgt_r.to(dev), tgt_c.to(dev)
        self.perms = [p.to(dev) for p in perms]
        self.stale = torch.full((1,), P.stale_sq0(r), dtype=torch.float32, device=dev)
        self.adam_step, self.M, self.n_mb = P.adam_step0(r), P.rows(batch), P.n_steps(batch)
        self.sync_ws = torch.zeros(32, dtype=torch.int64, device=dev)
        self.cfg = _abi.PpoCfg(obs_dim=D, act_dim=A, batch=batch, use_critic_norm=1, use_value_coefficient=0, clip=0.2,
                               max_grad_norm=P.max_grad_norm(r), lr_actor=3e-4, lr_critic=P.lr_critic(r), beta1=0.9, beta2=0.999,
                               adam_eps=1e-8, l2_coef=0.001)

    def state(self):
        return self.theta.clone(), self.m.clone(), self.v.clone(), self.stale.clone()

    def single(self, lib, launch):
        """spo_critic_fit_iter_ks: the stand-alone launch."""
        from safepo import _abi
        losses = torch.full((self.n_mb, 3), SENTINEL, device=self.theta.device)
        _abi.check(lib.spo_critic_fit_iter_ks(
            _abi.ptr(self.theta), _abi.ptr(self.m), _abi.ptr(self.v), self.adam_step, _abi.ptr(self.obs), _abi.ptr(self.tgt_r),
            _abi.ptr(self.tgt_c), _abi.ptr(self.perms[launch]), self.M, self.cfg, _abi.ptr(self.stale), _abi.ptr(losses),
            _abi.ptr(self.sync_ws), _abi.stream_ptr()), "spo_critic_fit_iter_ks")
        self.adam_step += self.n_mb
        return losses

    def fill(self, t, perm, losses, active=1, **over):
        from safepo import _abi
        g = lambda k: over.get(k, getattr(self, k))     # noqa: E731
        t.theta, t.adam_m, t.adam_v, t.adam_step = _abi.ptr(g("theta")), _abi.ptr(g("m")), _abi.ptr(g("v")), self.adam_step
        t.obs, t.target_r, t.target_c = _abi.ptr(self.obs), _abi.ptr(self.tgt_r), _abi.ptr(self.tgt_c)
        t.perm, t.losses_out, t.stale_sq_io = _abi.ptr(perm), _abi.ptr(losses), _abi.ptr(g("stale"))
        t.sync_ws, t.cfg, t.active = _abi.ptr(g("sync_ws")), self.cfg, active


STATE_NAMES = ("theta", "adam_m", "adam_v", "stale_sq")


def _assert_same(got, want, what):
    for name, x, y in zip(STATE_NAMES, got, want):
        assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} of {x.numel()} entries, max |d| {float((x - y).abs().max())}"


def _multi(lib, runs, launch, active=None):
    """One spo_critic_fit_iter_ks_multi launch with sentinel-filled logs; advances every active run's clock."""
    from safepo import _abi
    S = len(runs)
    logs = [torch.full((x.n_mb, 3), SENTINEL, device=x.theta.device) for x in runs]
    reps = (_abi.CriticFitReplica * S)()
    for r, x in enumerate(runs):
        x.fill(reps[r], x.perms[launch], logs[r], int(active is None or active[r]))
    _abi.check(lib.spo_critic_fit_iter_ks_multi(reps, S, runs[0].M, _abi.stream_ptr()), "spo_critic_fit_iter_ks_multi")
    torch.cuda.synchronize()
    for r, x in enumerate(runs):
        if active is None or active[r]:
            x.adam_step += x.n_mb
    return logs


_REFERENCE = {}


def _reference(lib, shape, batch, dev, n, safe=False):
    """Per run r < n of a (shape, batch): (theta, m, v, stale_sq) after the first and after the second single launch and the two
    loss logs -- spo_critic_fit_iter_ks, one run after the other, adam_step carried.  Computed once per case and left alone; a run
    does not depend on the number of runs beside it."""
    ref = _REFERENCE.setdefault((shape, batch, safe), [])
    for r in range(len(ref), n):
        x = _Run(shape, batch, r, dev)
        init = x.state()
        l0 = x.single(lib, 0)
        s0 = x.state()
        l1 = x.single(lib, 1)
        s1 = x.state()
        assert int(x.sync_ws[8].item()) == 0
        assert all(torch.isfinite(t).all() for t in s1) and all(torch.isfinite(t[:, :2]).all() for t in (l0, l1))
        assert not torch.equal(init[0][:x.ls_off], s0[0][:x.ls_off]) and not torch.equal(s0[0], s1[0])
        assert torch.equal(s1[0][x.ls_off:], init[0][x.ls_off:])                  # the actor's block is not the critic fit's
        assert bool((l0[:, 2] == SENTINEL).all())                                # column 2 of the log is not written
        ref.append({"init": init, "after1": s0, "after2": s1, "losses": (l0, l1)})
    if n > 1:
        # the runs differ from each other (the comparisons below are not between copies of one run) ...
        assert not torch.equal(ref[0]["after2"][0], ref[1]["after2"][0]) and not torch.equal(ref[0]["losses"][0], ref[1]["losses"][0])
        # ... and both kinds of step occurred within the launch: run 0 (max_grad_norm 0.6 under a stale norm above 0.707) clipped
        # -- every clip rescales stale_sq_io -- and run 1 (max_grad_norm 1000) never did: its stale norm comes back bit for bit
        assert float(ref[0]["after1"][3]) < float(ref[0]["init"][3]), "run 0 did not clip"
        assert torch.equal(ref[1]["after2"][3], ref[1]["init"][3]), "run 1 clipped"
    return ref


def _batched_against_single(dev, shape, batch, S, safe=False):
    from safepo import _abi
    lib = _abi.load()
    D, _ = shape
    assert lib.spo_critic_fit_ks_multi_supported(D, batch, S) == 1
    ref = _reference(lib, shape, batch, dev, S, safe)
    runs = [_Run(shape, batch, r, dev) for r in range(S)]
    before_first_order = _first_order_counters(lib)
    for launch in range(2):
        _counters(lib)
        logs = _multi(lib, runs, launch)
        assert all(int(x.sync_ws[8].item()) == 0 for x in runs)                  # no error word is set
        c3 = _counters(lib)
        assert c3[:2] == [1, S], c3                                              # ONE launch of S runs, not S launches
        if safe:
            assert c3[2] == S, c3                                                # every run reports the write-through path
        elif c3[2] != 0:
            print(f"{shape} batch {batch}, {S} runs, launch {launch}: the placement census chose write-through stores for "
                  f"{c3[2]} of {S} runs (their workgroups were not on one XCD); results are compared all the same")
        for r, x in enumerate(runs):
            what = f"run {r} of {S}, launch {launch}"
            assert x.adam_step == P.adam_step0(r) + (launch + 1) * x.n_mb
            assert torch.equal(logs[r], ref[r]["losses"][launch]), f"{what}: loss log"
            _assert_same(x.state(), ref[r]["after1" if launch == 0 else "after2"], what)
            assert torch.equal(x.theta[x.ls_off:], x.theta0[x.ls_off:]), f"{what}: the actor's block of theta changed"
    assert _first_order_counters(lib) == before_first_order                      # the first-order launches' counters do not move


# ------------------------------------------------------------------------------------------------ 1. bit-exact against the single launch
# every shape x batch at 1, 3 and 8 runs, and at 9 and 16 where a launch takes that many (up to 384 observations: runs r and r + 8
# share an XCD label there)
BIT_EXACT_CASES = [(shape, batch, S) for shape in P.SHAPES for batch in P.BATCHES for S in P.REPLICAS if S <= P.max_runs(shape[0])]


@pytest.mark.parametrize("shape,batch,S", BIT_EXACT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_batched_launch_is_bit_exact_against_single_launches(dev, shape, batch, S):
    _batched_against_single(dev, shape, batch, S)


@pytest.mark.parametrize("batch", [128, 65])
def test_batched_launch_is_bit_exact_under_write_through_stores(dev, monkeypatch, batch):
    """SPO_KS_SAFE=1 (read at every launch): the exchange on write-through stores, single launches under the same setting; every
    run of the batched launch reports the write-through path."""
    monkeypatch.setenv("SPO_KS_SAFE", "1")
    _batched_against_single(dev, P.HUMANOID, batch, 3, safe=True)


# ------------------------------------------------------------------------------------------------ 2. inactive runs
GUARD = 64              # floats (or words) of guard pattern on either side


def _guarded(t, pattern):
    """A copy of t in the middle of a buffer filled with `pattern` -> (the whole buffer, the view that holds the copy)."""
    buf = torch.full((t.numel() + 2 * GUARD,), pattern, dtype=t.dtype, device=t.device)
    inner = buf[GUARD:GUARD + t.numel()].view(t.shape)
    inner.copy_(t)
    return buf, inner


def test_inactive_runs_are_untouched(dev):
    from safepo import _abi
    lib = _abi.load()
    shape, batch, S, off = P.HUMANOID, 128, 3, 1
    ref = _reference(lib, shape, batch, dev, S)
    runs = [_Run(shape, batch, r, dev) for r in range(S)]
    x = runs[off]
    # the run that sits out: its parameters, moments, stale norm and sync_ws in sentinel-guarded buffers of our own, themselves
    # filled with sentinels; perm and losses_out NULL
    g_theta, g_m, g_v = _guarded(torch.full_like(x.theta, -3.5), -3.25), _guarded(torch.full_like(x.m, -4.5), -4.25), \
        _guarded(torch.full_like(x.v, -5.5), -5.25)
    g_stale = _guarded(torch.full_like(x.stale, -6.5), -6.25)
    ws = torch.arange(1, 33, device=dev) * 0x0101010101
    g_ws = _guarded(ws, 0x7E7E7E7E7E7E)
    kept = [b.clone() for b, _ in (g_theta, g_m, g_v, g_stale, g_ws)]
    logs = [torch.full((y.n_mb, 3), SENTINEL, device=dev) for y in runs]
    reps = (_abi.CriticFitReplica * S)()
    for r, y in enumerate(runs):
        if r == off:
            y.fill(reps[r], None, None, 0, theta=g_theta[1], m=g_m[1], v=g_v[1], stale=g_stale[1], sync_ws=g_ws[1])
        else:
            y.fill(reps[r], y.perms[0], logs[r])
    _counters(lib)
    _abi.check(lib.spo_critic_fit_iter_ks_multi(reps, S, x.M, _abi.stream_ptr()), "spo_critic_fit_iter_ks_multi")
    torch.cuda.synchronize()
    assert _counters(lib)[:2] == [1, S - 1]
    for (buf, _), k, what in zip((g_theta, g_m, g_v, g_stale, g_ws), kept, ("theta", "adam_m", "adam_v", "stale_sq", "sync_ws")):
        assert torch.equal(buf, k), f"inactive run: {what} or its guards written"
    assert bool((logs[off] == SENTINEL).all())
    for r, y in enumerate(runs):
        if r == off:
            continue
        y.adam_step += y.n_mb
        assert int(y.sync_ws[8].item()) == 0
        _assert_same(y.state(), ref[r]["after1"], f"active run {r}")
        assert torch.equal(logs[r], ref[r]["losses"][0])
    # the second launch, the same run (now with its real arrays) sitting out
    before = x.state()
    logs = _multi(lib, runs, 1, [r != off for r in range(S)])
    for r, y in enumerate(runs):
        if r == off:
            _assert_same(y.state(), before, "inactive run, second launch")
            assert bool((logs[r] == SENTINEL).all()) and y.adam_step == P.adam_step0(r) and not bool(y.sync_ws.any())
        else:
            _assert_same(y.state(), ref[r]["after2"], f"active run {r}, second launch")
            assert torch.equal(logs[r], ref[r]["losses"][1])
    # every run sitting out: nothing enqueued
    _counters(lib)
    _multi(lib, runs, 1, [False] * S)
    assert _counters(lib) == [0, 0, 0]


def test_refused_tables_touch_nothing(dev):
    """Refused before device work -- a stream under capture among them (captured, never replayed): the runs' state, their logs and
    the launch counter stay what they were."""
    from safepo import _abi
    lib = _abi.load()
    shape, batch = P.HUMANOID, 128
    runs = [_Run(shape, batch, r, dev) for r in range(2)]
    before = [x.state() for x in runs]
    logs = [torch.full((x.n_mb, 3), SENTINEL, device=dev) for x in runs]

    def table():
        reps = (_abi.CriticFitReplica * 2)()
        for r, x in enumerate(runs):
            x.fill(reps[r], x.perms[0], logs[r])
        return reps

    f, M = lib.spo_critic_fit_iter_ks_multi, runs[0].M
    err = lambda: lib.spo_last_error().decode()          # noqa: E731
    _counters(lib)
    t = table(); t[1].stale_sq_io = t[0].stale_sq_io
    assert f(t, 2, M, _abi.stream_ptr()) != 0 and "share theta, sync_ws or stale_sq_io" in err()
    t = table(); t[1].cfg.batch = 64
    assert f(t, 2, M, _abi.stream_ptr()) != 0 and "replica 1 has obs_dim" in err()
    torch.cuda.synchronize()
    x = torch.zeros(8, device=dev)
    graph = torch.cuda.CUDAGraph()
    t = table()
    with torch.cuda.graph(graph):
        x.add_(1.0)
        rc = f(t, 2, M, _abi.stream_ptr())
        msg = err()
    torch.cuda.synchronize()
    assert rc != 0 and "under capture" in msg, (rc, msg)
    assert _counters(lib) == [0, 0, 0]
    for y, b, log in zip(runs, before, logs):
        _assert_same(y.state(), b, "refused tables")
        assert bool((log == SENTINEL).all()) and not bool(y.sync_ws.any())


# ------------------------------------------------------------------------------------------------ 3. the group
D_H, A_H = P.HUMANOID
ITERS = [3, 1, 2]                # learning_iters per run


def _engine(r, dev, batch=128):
    """Run r on the engine the scripts build for it (make_engine: WideCPOEngine, critic fit on the feature-split kernel), with a
    stale actor gradient in flat_grad's tail."""
    from safepo.single_agent.cpo import WideCPOEngine, make_engine
    pol = P.make_policy(P.HUMANOID, r).to(dev)
    M = P.rows(batch)
    eng = make_engine(pol, 1, M, dict(P.CFG, batch_size=batch, max_grad_norm=P.max_grad_norm(r), learning_iters=ITERS[r]), dev)
    assert type(eng) is WideCPOEngine and not eng._critics_on_persistent_kernel and eng._feature_split_critic_fit_ok(eng._cfg_struct())
    obs, tgt_r, tgt_c = P.make_rows(P.HUMANOID, r, batch)
    b = eng.buffer
    b.data["obs"].view(-1, D_H).copy_(obs); b.data["target_value_r"].view(-1).copy_(tgt_r); b.data["target_value_c"].view(-1).copy_(tgt_c)
    eng.lr_critic = P.lr_critic(r)
    g = torch.Generator().manual_seed(400 + r)
    vec = torch.randn(eng.Pa, generator=g)
    eng._set_stale_actor_grad((vec * (P.stale_sq0(r) ** 0.5 / float(vec.norm()))).to(dev))
    perms = [p.to(dev) for p in P.make_perms(r, batch, max(ITERS))]
    return eng, (lambda it: perms[it])


def _engine_state(eng):
    return tuple(t.clone() for t in (eng.policy.theta, eng.adam_m, eng.adam_v, eng.stale_sq, eng.flat_grad[eng.ls_off:]))


def test_group_critic_fit_with_staggered_learning_iters(dev, monkeypatch):
    from safepo import _abi
    from safepo.common.engine_group import CPOEngineGroup
    lib = _abi.load()
    alone = []
    for r in range(3):
        eng, perm_fn = _engine(r, dev)
        tail0 = eng.flat_grad[eng.ls_off:].clone()
        out = eng.critic_fit(perm_fn)
        alone.append((out, _engine_state(eng), eng.adam_step, tail0))
    # run 0 clipped, so its stale vector was rescaled; run 1 never did, so its vector is what it was
    assert not torch.equal(alone[0][1][4], alone[0][3]) and torch.equal(alone[1][1][4], alone[1][3])
    built = [_engine(r, dev) for r in range(3)]
    with pytest.raises(_abi.SpoError, match="WideCPOEngine"):                    # without the switch: refused as before
        CPOEngineGroup([e for e, _ in built])
    group = CPOEngineGroup([e for e, _ in built], ks_form=True)
    assert group.batched_ks() and not group.batched() and not group.batched_split()
    _counters(lib)
    outs = group.critic_fit_all([f for _, f in built])
    c3 = _counters(lib)
    assert c3[:2] == [max(ITERS), sum(ITERS)], c3                                # one launch per iteration, a run in as many as it has
    for r, ((eng, _), out, (aout, astate, astep, _t)) in enumerate(zip(built, outs, alone)):
        assert (out["loss_r"], out["loss_c"]) == (aout["loss_r"], aout["loss_c"]) and len(out["losses"]) == ITERS[r]
        assert all(torch.equal(x, y) for x, y in zip(out["losses"], aout["losses"]))
        assert eng.adam_step == astep and int(eng.sync_ws[8].item()) == 0
        for name, x, y in zip(STATE_NAMES + ("flat_grad tail",), _engine_state(eng), astate):
            assert torch.equal(x, y), f"group run {r}: {name}"
    # where the group does not batch (SPO_WIDE_KS=0 takes the kernel away from the engines too): each engine's own critic_fit
    monkeypatch.setenv("SPO_WIDE_KS", "0")
    assert not group.batched_ks()


# ------------------------------------------------------------------------------------------------ 4. the scripts
SEEDS = [0, 1000]


def _args(log_dir, **kw):
    a = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=16, experiment="t", log_dir=str(log_dir), device="cuda",
                           device_id=0, write_terminal=True, headless=False, total_steps=2 * 16 * 64, steps_per_epoch=16 * 64,
                           randomize=False, cost_limit=25.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035,
                           cfg_override={"learning_iters": 3}, env_kwargs={"obs_dim": D_H, "act_dim": A_H, "trunc_len": 16})
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


@pytest.mark.parametrize("algo", ["cpo", "trpo_lag"])
def test_scripts_with_seeds_equal_the_stand_alone_runs(dev, tmp_path, algo, capsys):
    import importlib
    from safepo import _abi
    lib = _abi.load()
    mod = importlib.import_module(f"safepo.single_agent.{algo}")
    alone = {}
    for seed in SEEDS:
        d = tmp_path / f"alone_{seed}"
        mod.main(_args(d, seed=seed), {})
        alone[seed] = _run_record(d)
    dirs = [str(tmp_path / f"group_{s}") for s in SEEDS]
    with pytest.raises(SystemExit, match="wide-network"):                # without the new flag: today's refusal
        mod.main(_args(tmp_path / "unused", seeds=list(SEEDS), log_dirs=dirs, batch_critic_fit=True), {})
    assert not any(os.path.exists(d) for d in dirs)
    _counters(lib)
    mod.main(_args(tmp_path / "unused", seeds=list(SEEDS), log_dirs=dirs, batch_critic_fit=True, batch_critic_fit_feature_split=True), {})
    c3 = _counters(lib)
    assert c3[:2] == [2 * 3, 2 * 3 * 2], c3                          # epochs x iterations launches of two runs each
    for d, seed in zip(dirs, SEEDS):
        _assert_same_run(_run_record(d), alone[seed], f"{algo} --seeds {SEEDS} --batch-critic-fit-feature-split True: seed {seed}")
    capsys.readouterr()
    # the runs differ from each other (the comparison above is not between two copies of one run)
    assert alone[0][0] != alone[1000][0]


def test_seed_cap_is_checked_before_any_log_directory(dev, tmp_path):
    from safepo.single_agent import cpo
    seeds = [1000 * i for i in range(9)]
    dirs = [str(tmp_path / f"nine_{s}") for s in seeds]
    kw = {"obs_dim": 448, "act_dim": 8, "trunc_len": 16}                  # S = 7: eight runs at the most
    with pytest.raises(SystemExit, match="at most 8 seeds"):
        cpo.main(_args(tmp_path / "nine", seeds=seeds, log_dirs=dirs, batch_critic_fit=True, batch_critic_fit_feature_split=True,
                       env_kwargs=kw), {})
    assert not any(os.path.exists(d) for d in dirs) and not os.path.exists(tmp_path / "nine")
