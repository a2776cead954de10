"""GPU tests of the seed-batched split critic fit: the two-replica split critic fits (65-128 observations: WideCPOEngine on the
persistent two-critic kernel) of S independent runs in one persistent launch per iteration (spo_critic_fit_iter_split_multi,
csrc/update.hip; safepo.common.engine_group.CPOEngineGroup(split_form=True)).  The reference throughout is today's path on the
same machine -- spo_critic_fit_iter_split / WideCPOEngine.critic_fit / the scripts' `--seed` -- on copies of the same state, and
the comparison is bit for bit: both replicas' parameters, both Adam moments, both stale_sq_io and both loss logs.  No tolerance
anywhere.  No test provokes a timeout of the exchange."""
import argparse
import csv
import ctypes
import faulthandler
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_parity import _fill_update_problem  # noqa: E402
import seed_batch_critic_split_cases as C  # noqa: E402

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
    for k in ("SPO_CPO_SPLIT", "SPO_RS_ROWS", "SPO_CPO_SPLIT_FORM"):
        monkeypatch.delenv(k, raising=False)
    assert int(os.environ.get("SPO_UPDATE_FORM", "3")) >= 3, "SPO_UPDATE_FORM selects an older form in this process: unset it"


def _counters(lib, reset=1):
    from safepo import _abi
    c3 = (ctypes.c_ulonglong * 3)()
    _abi.check(lib.spo_debug_critic_fit_split_multi_counters(c3, reset), "split multi counters")
    return [int(x) for x in c3]


def _engine(shape, r, dev, learning_iters=1):
    """Run r of a shape: its own initialisation, critic-fit problem, stale actor-gradient norm and shuffles -- on the engine the
    scripts build for it (make_engine: WideCPOEngine, critics on the persistent kernel) with its split state."""
    from safepo.single_agent.cpo import WideCPOEngine, make_engine
    pol = C.make_policy(shape, r).to(dev)
    eng = make_engine(pol, 1, C.M, dict(C.CFG, batch_size=C.BATCH, max_grad_norm=C.MAX_GRAD_NORM, learning_iters=learning_iters), dev)
    assert type(eng) is WideCPOEngine and eng._critics_on_persistent_kernel
    _fill_update_problem(eng, C.make_problem(shape, r))
    eng.stale_sq.fill_(C.stale_sq0(r))
    assert eng._split_setup() is not None, "the stand-alone critic fit does not take the split form here"
    return eng, [p.to(dev) for p in C.make_perms(r, max(2, learning_iters))]


def _cfg64(eng):
    """What WideCPOEngine.critic_fit hands spo_critic_fit_iter_split."""
    eng._in_persistent_critic_fit = True
    try:
        cfg = eng._cfg_struct()
    finally:
        eng._in_persistent_critic_fit = False
    cfg.batch = 64
    return cfg


def _start(eng):
    """The start of a critic fit: the second replica is a copy of the first."""
    st = eng._split_setup()
    st["theta1"].copy_(eng.policy.theta); st["m1"].copy_(eng.adam_m); st["v1"].copy_(eng.adam_v); st["stale1"].copy_(eng.stale_sq)


def _state(eng):
    st = eng._split_setup()
    return tuple(t.clone() for t in (eng.policy.theta, eng.adam_m, eng.adam_v, eng.stale_sq, st["theta1"], st["m1"], st["v1"], st["stale1"]))


STATE_NAMES = ("theta0", "adam_m0", "adam_v0", "stale_sq0", "theta1", "adam_m1", "adam_v1", "stale_sq1")


def _halves(perm):
    p = perm.view(C.N_MB, 128)
    return p[:, :64].contiguous().view(-1), p[:, 64:].contiguous().view(-1)


def _single_iter(lib, eng, perm):
    """One spo_critic_fit_iter_split launch -- today's path -- with sentinel-filled logs; continues the run's step tag."""
    from safepo import _abi
    st, d = eng._split_setup(), eng.buffer.data
    p0, p1 = _halves(perm)
    l0, l1 = (torch.full((C.N_MB, 3), SENTINEL, device=eng.dev) for _ in range(2))
    _abi.check(lib.spo_critic_fit_iter_split(
        _abi.ptr(eng.policy.theta), _abi.ptr(eng.adam_m), _abi.ptr(eng.adam_v), _abi.ptr(st["theta1"]), _abi.ptr(st["m1"]),
        _abi.ptr(st["v1"]), eng.adam_step, _abi.ptr(d["obs"]), _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]),
        _abi.ptr(p0), _abi.ptr(p1), C.M // 2, _cfg64(eng), _abi.ptr(eng.stale_sq), _abi.ptr(st["stale1"]), _abi.ptr(l0), _abi.ptr(l1),
        _abi.ptr(eng.sync_ws), _abi.ptr(st["sync_ws"]), st["regions"], st["step"] & 0xFFFFFFFF, _abi.stream_ptr()),
        "spo_critic_fit_iter_split")
    st["step"] += C.N_MB
    eng.adam_step += C.N_MB
    return l0, l1


def _table(engs, perms, logs, active=None):
    from safepo import _abi
    S = len(engs)
    reps = (_abi.CriticFitSplitReplica * S)()
    keep = []
    for r, e in enumerate(engs):
        st, d, x = e._split_setup(), e.buffer.data, reps[r]
        x.cfg, x.active = _cfg64(e), int(active is None or active[r])
        x.theta0, x.adam_m0, x.adam_v0 = _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v)
        x.theta1, x.adam_m1, x.adam_v1 = _abi.ptr(st["theta1"]), _abi.ptr(st["m1"]), _abi.ptr(st["v1"])
        x.adam_step = e.adam_step
        x.obs, x.target_r, x.target_c = _abi.ptr(d["obs"]), _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"])
        if perms[r] is not None:
            p0, p1 = _halves(perms[r])
            keep.append((p0, p1))
            x.perm0, x.perm1 = _abi.ptr(p0), _abi.ptr(p1)
        x.stale_sq_io0, x.stale_sq_io1 = _abi.ptr(e.stale_sq), _abi.ptr(st["stale1"])
        x.losses0, x.losses1 = _abi.ptr(logs[r][0]), _abi.ptr(logs[r][1])
        x.sync_ws0, x.sync_ws1 = _abi.ptr(e.sync_ws), _abi.ptr(st["sync_ws"])
        x.regions2[0], x.regions2[1] = st["regions"][0], st["regions"][1]
        x.step0 = st["step"] & 0xFFFFFFFF
    return reps, keep


def _new_logs(engs):
    return [tuple(torch.full((C.N_MB, 3), SENTINEL, device=e.dev) for _ in range(2)) for e in engs]


def _multi_iter(lib, engs, perms, active=None):
    """One spo_critic_fit_iter_split_multi launch with sentinel-filled logs; continues every active run's step tag."""
    from safepo import _abi
    logs = _new_logs(engs)
    reps, keep = _table(engs, perms, logs, active)
    _abi.check(lib.spo_critic_fit_iter_split_multi(reps, len(engs), C.M // 2, _abi.stream_ptr()), "spo_critic_fit_iter_split_multi")
    for r, e in enumerate(engs):
        if active is None or active[r]:
            e._split_setup()["step"] += C.N_MB
            e.adam_step += C.N_MB
    return logs


_REFERENCE = {}


def _reference(shape, dev):
    """Per run r < S_MAX of a shape: the state (both replicas) after the first and after the second single launch and the loss
    logs.  Computed once per shape and left alone; a run does not depend on S."""
    if shape in _REFERENCE:
        return _REFERENCE[shape]
    from safepo import _abi
    lib = _abi.load()
    ref = []
    for r in range(C.S_MAX):
        eng, perms = _engine(shape, r, dev)
        stale0 = eng.stale_sq.clone()
        _start(eng)
        la = _single_iter(lib, eng, perms[0])
        s0 = _state(eng)
        lb = _single_iter(lib, eng, perms[1])
        torch.cuda.synchronize()
        assert int(eng.sync_ws[8].item()) == 0 and int(eng._split_setup()["sync_ws"][8].item()) == 0
        ref.append({"stale0": stale0, "after1": s0, "after2": _state(eng), "losses": (la, lb)})
    for x in ref:
        assert all(torch.isfinite(t).all() for t in x["after2"])
        for pair in x["losses"]:
            assert all(torch.isfinite(t[:, :2]).all() and bool((t[:, 2] == SENTINEL).all()) for t in pair)
        # the two replicas of a run end on the same bits (each reduces the same exchanged sum)
        assert all(torch.equal(x["after2"][k], x["after2"][k + 4]) for k in range(4))
    # the clip rescaled the stale norm in some runs (stale_sq_io is written, not only read) and not in every run alike
    assert any(not torch.equal(x["after2"][3], x["stale0"]) for x in ref)
    assert len({float(x["after2"][3]) / float(x["stale0"]) for x in ref}) > 1
    _REFERENCE[shape] = ref
    return ref


def _assert_same(got, want, what):
    for name, x, y in zip(STATE_NAMES, got, want):
        assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} of {x.numel()} entries, max |d| {float((x - y).abs().max())}"


# ------------------------------------------------------------------------------------------------ 1. bit-exact against the single launch
@pytest.mark.parametrize("S", [1, 3, 9, 17])
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_batched_launch_is_bit_exact_against_single_launches(dev, shape, S):
    from safepo import _abi
    lib = _abi.load()
    assert lib.spo_critic_fit_split_multi_supported(shape[0], 64, S) == 1
    ref = _reference(shape, dev)
    built = [_engine(shape, r, dev) for r in range(S)]
    engs = [e for e, _ in built]
    for e in engs:
        _start(e)
    for launch in range(2):                                         # the second continues step0, the tags and adam_step
        _counters(lib)
        logs = _multi_iter(lib, engs, [p[launch] for _, p in built])
        torch.cuda.synchronize()
        c3 = _counters(lib)
        print(f"{shape} S {S} launch {launch}: launches {c3[0]}, runs {c3[1]}, on the shared-L2 body {c3[2]}")   # (third: reported)
        assert c3[:2] == [1, S] and 0 <= c3[2] <= S, c3             # ONE launch of S runs
        for r, e in enumerate(engs):
            assert int(e.sync_ws[8].item()) == 0 and int(e._split_setup()["sync_ws"][8].item()) == 0, f"run {r}: error word set"
            for h in range(2):
                assert torch.equal(logs[r][h], ref[r]["losses"][launch][h]), f"run {r} of {S}, launch {launch}: loss log {h}"
            _assert_same(_state(e), ref[r]["after1" if launch == 0 else "after2"], f"run {r} of {S}, launch {launch}")


def test_uncached_exchange_gives_the_same_bits(dev):
    """SPO_CPO_SPLIT_L2=0 (read once per process, hence a child process): every run of the batched launch takes the uncached
    body -- the third counter stays 0 -- and equals its single launches under the same setting bit for bit."""
    import json
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    S, shape = 9, C.SHAPES[0]
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "seed_batch_critic_split_worker.py"), str(S), str(shape[0]), str(shape[1])],
                       env=dict(os.environ, SPO_CPO_SPLIT_L2="0"), capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    res = json.loads([line for line in r.stdout.splitlines() if line.startswith("RESULT ")][-1][7:])
    assert res["l2"] == "0" and res["bad"] == [], res
    assert res["counters"] == [2, 2 * S, 0], res                    # two launches of S runs, none on the shared-L2 body


# ------------------------------------------------------------------------------------------------ 2. inactive runs, refusals
def test_inactive_runs_are_untouched(dev):
    from safepo import _abi
    lib = _abi.load()
    shape, S, off = C.SHAPES[0], 9, (1, 8)
    ref = _reference(shape, dev)
    built = [_engine(shape, r, dev) for r in range(S)]
    engs = [e for e, _ in built]
    for e in engs:
        _start(e)
    for r in off:                                                   # sentinel-filled state: must stay sentinel
        e, st = engs[r], engs[r]._split_setup()
        for t in (e.policy.theta, e.adam_m, e.adam_v, e.stale_sq, st["theta1"], st["m1"], st["v1"], st["stale1"]):
            t.fill_(SENTINEL)
        e.sync_ws.fill_(0x5A5A5A5A)
        st["sync_ws"].fill_(0x5A5A5A5A)
    active = [r not in off for r in range(S)]
    steps_before = [e._split_setup()["step"] for e in engs]
    _counters(lib)
    logs = _multi_iter(lib, engs, [p[0] if a else None for (_, p), a in zip(built, active)], active)
    torch.cuda.synchronize()
    assert _counters(lib)[:2] == [1, S - len(off)]
    for r, e in enumerate(engs):
        st = e._split_setup()
        if r in off:
            assert all(bool((t == SENTINEL).all()) for t in _state(e)), f"inactive run {r}: state written"
            assert bool((e.sync_ws == 0x5A5A5A5A).all()) and bool((st["sync_ws"] == 0x5A5A5A5A).all()), f"inactive run {r}: sync_ws written"
            assert all(bool((t == SENTINEL).all()) for t in logs[r]) and e.adam_step == 0 and st["step"] == steps_before[r]
        else:
            assert int(e.sync_ws[8].item()) == 0 and int(st["sync_ws"][8].item()) == 0
            _assert_same(_state(e), ref[r]["after1"], f"active run {r}")
            assert all(torch.equal(logs[r][h], ref[r]["losses"][0][h]) for h in range(2))


def test_all_inactive_and_refused_tables(dev):
    from safepo import _abi
    lib = _abi.load()
    shape = C.SHAPES[1]
    built = [_engine(shape, r, dev) for r in range(3)]
    engs, perms = [e for e, _ in built], [p[0] for _, p in built]
    for e in engs:
        _start(e)
    before = [_state(e) for e in engs]
    logs = _new_logs(engs)
    f = lib.spo_critic_fit_iter_split_multi
    _counters(lib)

    def refused(table, n, match, m_half=C.M // 2):
        assert f(table[0], n, m_half, _abi.stream_ptr()) < 0
        assert match in lib.spo_last_error().decode(), lib.spo_last_error().decode()

    assert f(_table(engs, perms, logs, [False] * 3)[0], 3, C.M // 2, _abi.stream_ptr()) == 0       # nothing active: nothing enqueued
    refused(_table(engs, perms, logs), 0, "replicas outside")
    refused(_table(engs, perms, logs), 3, "bad sizes", m_half=0)
    for field in ("theta0", "sync_ws1"):
        t = _table(engs, perms, logs)
        setattr(t[0][2], field, getattr(t[0][1], field))
        refused(t, 3, "replicas 1 and 2 share theta or sync_ws")
    t = _table(engs, perms, logs)
    t[0][1].theta1 = t[0][1].theta0
    refused(t, 3, "replica 1: the two halves need separate replicas")
    t = _table(engs, perms, logs)
    t[0][1].cfg.batch = 32
    refused(t, 3, "replica 1 has obs_dim / act_dim / batch")
    t = _table(engs, perms, logs)
    for x in t[0]:
        x.cfg.batch = 65
    refused(t, 3, "no seed-batched split form")
    t = _table(engs, perms, logs)
    t[0][0].losses1 = None
    refused(t, 3, "null pointer in replica 0")
    t = _table(engs, perms, logs)
    t[0][2].adam_step = -1
    refused(t, 3, "negative adam_step")
    torch.cuda.synchronize()
    assert _counters(lib) == [0, 0, 0]                                 # no launch left behind
    for e, b, pair in zip(engs, before, logs):
        _assert_same(_state(e), b, "refused tables")
        assert all(bool((t == SENTINEL).all()) for t in pair)


def test_launch_is_refused_under_stream_capture(dev):
    from safepo import _abi
    lib = _abi.load()
    shape = C.SHAPES[0]
    built = [_engine(shape, r, dev) for r in range(2)]
    engs, perms = [e for e, _ in built], [p[0] for _, p in built]
    for e in engs:
        _start(e)
    before = [_state(e) for e in engs]
    logs = _new_logs(engs)
    reps, keep = _table(engs, perms, logs)
    torch.cuda.synchronize()
    x = torch.zeros(8, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # (captured, never replayed)
        x.add_(1.0)
        rc = lib.spo_critic_fit_iter_split_multi(reps, 2, C.M // 2, _abi.stream_ptr())
        msg = lib.spo_last_error().decode()
    torch.cuda.synchronize()
    assert rc < 0 and "under capture" in msg, (rc, msg)
    for e, b in zip(engs, before):
        _assert_same(_state(e), b, "refused under capture")


# ------------------------------------------------------------------------------------------------ 3. the group
def test_group_critic_fit_all_against_per_engine_critic_fit(dev):
    from safepo import _abi
    from safepo.common.engine_group import CPOEngineGroup
    lib = _abi.load()
    shape, n_its = C.SHAPES[0], (1, 3, 2, 3)
    alone = []
    for r, n in enumerate(n_its):
        eng, perms = _engine(shape, r, dev, learning_iters=n)
        out = eng.critic_fit(lambda it, p=perms: p[it])
        alone.append((out, _state(eng), eng.adam_step, eng._split_setup()["step"]))
    built = [_engine(shape, r, dev, learning_iters=n) for r, n in enumerate(n_its)]
    with pytest.raises(_abi.SpoError, match="WideCPOEngine"):       # without the switch: refused as ever
        CPOEngineGroup([e for e, _ in built])
    group = CPOEngineGroup([e for e, _ in built], split_form=True)
    assert group.batched_split() and not group.batched()
    _counters(lib)
    outs = group.critic_fit_all([(lambda it, p=perms: p[it]) for _, perms in built])
    torch.cuda.synchronize()
    c3 = _counters(lib)
    assert c3[0] == max(n_its) and c3[1] == sum(n_its), c3          # one launch per iteration of the longest run, finished runs sit out
    for r, ((eng, _), out, (aout, astate, astep, atag)) in enumerate(zip(built, outs, alone)):
        assert (out["loss_r"], out["loss_c"]) == (aout["loss_r"], aout["loss_c"]), r
        assert len(out["losses"]) == n_its[r] and all(torch.equal(x, y) for x, y in zip(out["losses"], aout["losses"]))
        assert eng.adam_step == astep == n_its[r] * C.N_MB and eng._split_setup()["step"] == atag
        _assert_same(_state(eng), astate, f"critic_fit_all, run {r}")
    # minibatches other than 128 rows: no split form in the engines, every engine fits on its own
    from safepo.single_agent.cpo import make_engine
    odd = [make_engine(C.make_policy(shape, r).to(dev), 1, 128, dict(C.CFG, batch_size=64, max_grad_norm=1.0), dev) for r in range(2)]
    assert not CPOEngineGroup(odd, split_form=True).batched_split()


# ------------------------------------------------------------------------------------------------ 4. the scripts
SEEDS = [0, 1000, 2000]


def _args(log_dir, **kw):
    a = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=16, experiment="t", log_dir=str(log_dir), device="cuda",
                           device_id=0, write_terminal=True, headless=False, total_steps=3 * 16 * 64, steps_per_epoch=16 * 64,
                           randomize=False, cost_limit=25.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035,
                           cfg_override={"learning_iters": 3}, env_kwargs={"trunc_len": 16, "obs_dim": 72})
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
    _counters(lib)
    mod.main(_args(tmp_path / "unused", seeds=list(SEEDS), log_dirs=dirs, batch_critic_fit=True, batch_critic_fit_split=True), {})
    c3 = _counters(lib)
    assert c3[:2] == [3 * 3, 3 * 3 * 3], c3                         # epochs x iterations launches of three runs each
    for d, tag, seed in zip(dirs, ("a", "b", "c"), SEEDS):
        _assert_same_run(_run_record(d), alone[tag], f"{algo} --seeds {SEEDS} --batch-critic-fit-split True: seed {seed}")
    capsys.readouterr()
    # the runs differ from each other (the comparison above is not between three copies of one run)
    assert alone["a"][0] != alone["b"][0] and alone["b"][0] != alone["c"][0]
    # without the new flag: refused as before
    with pytest.raises(SystemExit, match="wide-network"):
        mod.main(_args(tmp_path / "unused2", seeds=list(SEEDS), batch_critic_fit=True), {})
