"""CPU tests (no GPU) of the seed-batched critic fit of the second-order scripts: the entry points are declared, exported and
bound; the block -> (run, workgroup) mapping of the critic-batched launch (the function the kernel itself uses); the support
and routing tables at their edges; what the launch refuses on the host; CPOEngineGroup's loop on recording stand-in engines;
the opt-in flag of the scripts and of the sweep launcher."""
import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("spo_critic_fit_iter_multi", "spo_critic_fit_multi_supported", "spo_critic_fit_multi_matches_single",
               "spo_rs_critic_multi_block_map", "spo_debug_rs_critic_multi_counters")
S_CAP = 24


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from safepo import _abi
    return _abi.load(g.LIB)


@pytest.fixture(autouse=True)
def _global_rng_state_is_put_back():
    st = random.getstate(), np.random.get_state(), torch.get_rng_state()
    yield
    random.setstate(st[0]); np.random.set_state(st[1]); torch.set_rng_state(st[2])


# ------------------------------------------------------------------------------------------------ symbols, struct
def test_symbols_declared_exported_and_bound(lib):
    from safepo import _abi
    header = open(os.path.join(ROOT, "include", "safepo_hip.h")).read()
    assert "SPO_RS_CRITIC_MAX_REPLICAS 24" in header and _abi.RS_CRITIC_MAX_REPLICAS == S_CAP
    assert "SPO_RS_MAX_REPLICAS 32" in header and _abi.RS_MAX_REPLICAS == 32          # the PPO form's cap stays
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name
    body = re.search(r"typedef struct \{([^}]*)\} spo_critic_fit_replica;", header, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert [n for n, _ in _abi.CriticFitReplica._fields_] == names, names
    assert names == ["theta", "adam_m", "adam_v", "adam_step", "obs", "target_r", "target_c", "perm", "losses_out", "stale_sq_io",
                     "sync_ws", "cfg", "active"]


# ------------------------------------------------------------------------------------------------ block mapping
def _walk(fn, S, blocks):
    out = []
    for b in blocks:
        rep, wg = ctypes.c_int(-1), ctypes.c_int(-1)
        out.append((b, fn(b, S, ctypes.byref(rep), ctypes.byref(wg)), rep.value, wg.value))
    return out


@pytest.mark.parametrize("S", range(1, S_CAP + 1))
def test_critic_block_mapping(lib, S):
    f = lib.spo_rs_critic_multi_block_map
    grid = 64 * ((S + 7) // 8)
    seen, label_of, per_label = {}, {}, [0] * 8
    for b, work, rep, wg in _walk(f, S, range(grid)):
        x, k = b & 7, b >> 3
        want_rep, want_wg = 8 * (k // 8) + x, k % 8
        if want_rep >= S:
            assert work == 0, (S, b)
            continue
        assert work == 1 and (rep, wg) == (want_rep, want_wg), (S, b, rep, wg)
        assert 0 <= rep < S and 0 <= wg < 8                          # every working block serves a run < S
        assert (rep, wg) not in seen, (S, b, seen[(rep, wg)])
        seen[(rep, wg)] = b
        assert label_of.setdefault(rep, x) == x                      # the eight blocks of a run share a label (an XCD)
        per_label[x] += 1
    assert len(seen) == 8 * S                                        # each run gets workgroups 0..7 exactly once
    assert all(label_of[r] == (r & 7) for r in range(S))             # ... all on label run & 7
    assert max(per_label) <= 24                                      # at most three runs = 24 one-CU blocks on an XCD's 32 CUs
    for _b, work, _r, _w in _walk(f, S, (-1, grid, grid + 5, 64 * 3)):
        assert work == 0                                             # outside the grid (64 ceil(S / 8) blocks)
    if S % 8 == 0:
        assert f(grid - 1, S, None, None) == 1
    assert f(grid, S, None, None) == 0


def test_critic_block_mapping_refuses_run_counts_outside_the_cap(lib):
    f = lib.spo_rs_critic_multi_block_map
    assert f(0, 0, None, None) == 0 and f(0, S_CAP + 1, None, None) == 0 and f(0, -3, None, None) == 0
    assert f(0, 1, None, None) == 1 and f(0, S_CAP, None, None) == 1


def test_ppo_block_mapping_keeps_its_results(lib):
    """The generalised mapping with six workgroups per run: what spo_rs_multi_block_map documented before."""
    for S in (1, 8, 9, 32):
        grid = 48 * ((S + 7) // 8)
        for b, work, rep, wg in _walk(lib.spo_rs_multi_block_map, S, range(-1, grid + 2)):
            want_rep, want_wg = 8 * ((b >> 3) // 6) + (b & 7), (b >> 3) % 6
            ok = 0 <= b < grid and want_rep < S
            assert work == int(ok), (S, b)
            if ok:
                assert (rep, wg) == (want_rep, want_wg)
    assert lib.spo_rs_multi_block_map(0, 33, None, None) == 0 and lib.spo_rs_multi_block_map(0, 25, None, None) == 1


# ------------------------------------------------------------------------------------------------ support and routing tables
def test_supported_table(lib):
    f = lib.spo_critic_fit_multi_supported
    for D in (0, 1, 16, 17, 60, 64, 65, 128):
        for A in (0, 1, 8, 16, 17):
            for B in (0, 1, 64, 65, 100, 128, 129):
                single = bool(lib.spo_update_rs_supported(D, A, B, 2))
                for S in (0, 1, 8, 24, 25, 32):
                    assert f(D, A, B, S) == int(single and 65 <= B <= 128 and 1 <= S <= S_CAP), (D, A, B, S)
    # the edges by name: 64 / 65 observations, 64 / 65 / 128 / 129 rows
    assert [f(64, 8, B, 3) for B in (64, 65, 128, 129)] == [0, 1, 1, 0]
    assert [f(65, 8, B, 3) for B in (64, 65, 128, 129)] == [0, 0, 0, 0]


def test_routing_query_follows_the_single_launch(lib):
    g = lib.spo_critic_fit_multi_matches_single
    form = os.environ.get("SPO_UPDATE_FORM")
    default = not form and not os.environ.get("SPO_RS_ROWS")
    for D in (1, 16, 17, 60, 64, 65, 128):
        for A in (1, 8, 16, 17):
            for B in (1, 64, 65, 128, 129):
                sup = lib.spo_critic_fit_multi_supported(D, A, B, 1)
                assert g(D, A, B) in (0, 1) and g(D, A, B) <= sup, (D, A, B)
                if default:
                    assert g(D, A, B) == sup, (D, A, B)
                if form is not None and int(form) < 3:
                    assert g(D, A, B) == 0


# ------------------------------------------------------------------------------------------------ host refusals
def _table(S, D=60, A=8, batch=128):
    from safepo import _abi
    reps = (_abi.CriticFitReplica * max(S, 1))()
    for i in range(S):
        base = 0x10000 * (i + 1)
        r = reps[i]
        for k, name in enumerate(("theta", "adam_m", "adam_v", "obs", "target_r", "target_c", "perm", "losses_out", "stale_sq_io",
                                  "sync_ws")):
            setattr(r, name, base + 256 * k)
        r.cfg = _abi.PpoCfg(obs_dim=D, act_dim=A, batch=batch)
        r.active = 1
    return reps


def test_host_validation_happens_before_any_device_work(lib):
    """No GPU here: anything that reached HIP would fail with a HIP error instead of these messages."""
    f = lib.spo_critic_fit_iter_multi

    def err():
        return lib.spo_last_error().decode()

    assert f(None, 2, 256, None) < 0 and "null replica table" in err()
    assert f(_table(1), 0, 256, None) < 0 and "replicas" in err()
    assert f(_table(25), 25, 256, None) < 0 and "replicas" in err()
    assert f(_table(2), 2, 0, None) < 0 and "bad sizes" in err()
    assert f(_table(2, D=65), 2, 256, None) < 0 and "no replica-batched form" in err()
    assert f(_table(2, batch=64), 2, 256, None) < 0 and "no replica-batched form" in err()
    assert f(_table(2, batch=129), 2, 256, None) < 0 and "no replica-batched form" in err()
    t = _table(3)
    t[2].cfg.batch = 100
    assert f(t, 3, 256, None) < 0 and "replica 2" in err()
    for field in ("theta", "sync_ws", "stale_sq_io"):
        t = _table(3)
        setattr(t[2], field, getattr(t[0], field))
        assert f(t, 3, 256, None) < 0 and "share" in err() and "0 and 2" in err(), field
    for field in ("theta", "adam_m", "adam_v", "obs", "target_r", "target_c", "stale_sq_io", "sync_ws", "perm", "losses_out"):
        t = _table(2)
        setattr(t[1], field, None)
        assert f(t, 2, 256, None) < 0 and "null pointer in replica 1" in err(), field
    t = _table(2)
    t[0].adam_step = -1
    assert f(t, 2, 256, None) < 0 and "negative adam_step" in err()
    # perm / losses_out may be null in a run that sits out -- and with every run sitting out nothing is enqueued (no HIP call:
    # this returns 0 on a machine without a GPU)
    t = _table(3)
    for r in t:
        r.active, r.perm, r.losses_out = 0, None, None
    assert f(t, 3, 256, None) == 0


# ------------------------------------------------------------------------------------------------ CPOEngineGroup on stand-ins
class _StubComm:
    world_size = 1


class _StubEngine:
    """Records what the group asks of an engine; critic_fit is CPOEngine.critic_fit's loop without the launch."""
    D, A, M, dev = 4, 2, 12, torch.device("cpu")

    def __init__(self, learning_iters):
        self.log, self.cfg, self.comm = [], {"learning_iters": learning_iters}, _StubComm()

    def critic_fit(self, perm_fn=None):
        ls = []
        for it in range(self.cfg["learning_iters"]):
            self.log.append(("launch", it, perm_fn(it)))
            ls.append(torch.full((3, 2), float(10 * it + len(self.log))))
        self.log.append(("check",))
        means = torch.cat(ls, 0).mean(0).tolist() if ls else [float("nan")] * 2
        return {"loss_r": means[0], "loss_c": means[1], "losses": ls}

    def check_sync_error(self):
        self.log.append(("check",))

    def perm_fn(self, it):
        self.log.append(("perm", it))
        return ("perm", it)


def test_group_falls_back_to_per_engine_critic_fit():
    from safepo.common.engine_group import CPOEngineGroup
    es = [_StubEngine(n) for n in (1, 3, 2)]
    group = CPOEngineGroup(es)
    assert len(group) == 3 and not group.batched()
    outs = group.critic_fit_all([e.perm_fn for e in es])
    alone = [_StubEngine(n) for n in (1, 3, 2)]
    alone_out = [e.critic_fit(e.perm_fn) for e in alone]
    for e, a, o, ao in zip(es, alone, outs, alone_out):
        assert e.log == a.log
        assert (o["loss_r"], o["loss_c"]) == (ao["loss_r"], ao["loss_c"]) and len(o["losses"]) == len(ao["losses"])


def test_group_fallback_draws_default_shuffles_under_the_runs_generators():
    from safepo.common.engine_group import CPOEngineGroup, ReplicaRNG
    seeds = (5, 77)
    es = [_StubEngine(2) for _ in seeds]
    outer = torch.get_rng_state().clone()
    CPOEngineGroup(es, rngs=[ReplicaRNG(s) for s in seeds]).critic_fit_all()
    assert torch.equal(torch.get_rng_state(), outer)               # nothing drawn from the process-wide state
    for e, s in zip(es, seeds):
        torch.manual_seed(s)
        want = [torch.randperm(e.M).to(torch.int32) for _ in range(2)]
        got = [x[2] for x in e.log if x[0] == "launch"]
        assert len(got) == 2 and all(g.dtype == torch.int32 and torch.equal(g, w) for g, w in zip(got, want))


def test_group_batched_loop_order_with_recorded_launches():
    """The batched loop itself (the launch replaced by a recorder): per run, iteration it's shuffle is drawn before launch it
    and after launch it - 1, as CPOEngine.critic_fit draws it; a run with fewer learning_iters sits out the later launches."""
    from safepo.common.engine_group import CPOEngineGroup
    n_its = (1, 3, 2)
    es = [_StubEngine(n) for n in n_its]
    group = CPOEngineGroup(es)
    group.batched = lambda cfgs=None: True
    launches = []

    def fit_iter_all(perms, active=None):
        launches.append((list(perms), list(active)))
        out = []
        for i, e in enumerate(es):
            if active[i]:
                e.log.append(("launch", len(launches) - 1, perms[i]))
                out.append(torch.tensor([[1.0 + i, 2.0 * len(launches), -1.0]] * 3))
            else:
                out.append(None)
        return out

    group.fit_iter_all = fit_iter_all
    outs = group.critic_fit_all([e.perm_fn for e in es])
    assert [a for _, a in launches] == [[True, True, True], [False, True, True], [False, True, False]]
    for (perms, active) in launches:
        assert all((p is None) == (not a) for p, a in zip(perms, active))
    for i, (e, n) in enumerate(zip(es, n_its)):
        want = [x for it in range(n) for x in (("perm", it), ("launch", it, ("perm", it)))] + [("check",)]
        assert e.log == want, (i, e.log)
        ls = outs[i]["losses"]
        assert len(ls) == n and all(x.shape == (3, 2) for x in ls)            # the [n_mb, 2] views critic_fit returns
        means = torch.cat(ls, 0).mean(0).tolist()
        assert (outs[i]["loss_r"], outs[i]["loss_c"]) == (means[0], means[1])
    # no learning iterations at all: nothing launched, NaN means
    es0 = [_StubEngine(0), _StubEngine(0)]
    g0 = CPOEngineGroup(es0)
    g0.batched = lambda cfgs=None: True
    g0.fit_iter_all = lambda perms, active=None: pytest.fail("launched")
    o = g0.critic_fit_all()
    assert all(np.isnan(x["loss_r"]) and x["losses"] == [] for x in o)


def test_group_check_sync_error_names_the_run():
    from safepo import _abi
    from safepo.common.engine_group import CPOEngineGroup
    es = [_StubEngine(1) for _ in range(3)]

    def bad():
        raise _abi.SpoError("exchange timed out")

    es[1].check_sync_error = bad
    with pytest.raises(_abi.SpoError, match="replica 1 of 3: exchange timed out"):
        CPOEngineGroup(es).check_sync_error()


def test_group_argument_checks():
    from safepo import _abi
    from safepo.common.engine_group import CPOEngineGroup, ReplicaRNG
    from safepo.single_agent.cpo import CPOEngine, WideCPOEngine
    with pytest.raises(ValueError, match="no engines"):
        CPOEngineGroup([])
    with pytest.raises(ValueError, match="one ReplicaRNG per engine"):
        CPOEngineGroup([_StubEngine(1), _StubEngine(1)], rngs=[ReplicaRNG(0)])
    with pytest.raises(ValueError, match="one perm_fn"):
        CPOEngineGroup([_StubEngine(1), _StubEngine(1)]).critic_fit_all([None])
    odd = _StubEngine(1)
    odd.M = 13
    with pytest.raises(_abi.SpoError, match="engine 1 has obs / act / rows"):
        CPOEngineGroup([_StubEngine(1), odd])
    with pytest.raises(_abi.SpoError, match="at most 24"):
        CPOEngineGroup([_StubEngine(1) for _ in range(25)])
    wide = object.__new__(WideCPOEngine)
    with pytest.raises(_abi.SpoError, match="WideCPOEngine"):
        CPOEngineGroup([wide])
    dp = object.__new__(CPOEngine)
    dp.comm = type("C", (), {"world_size": 2})()
    dp.D, dp.A, dp.M, dp.dev = 4, 2, 12, torch.device("cpu")
    with pytest.raises(_abi.SpoError, match="world size 1 only"):
        CPOEngineGroup([dp])
    group = CPOEngineGroup([_StubEngine(1), _StubEngine(1)])
    group.batched = lambda cfgs=None: True
    with pytest.raises(ValueError, match="one perm and one active flag"):
        CPOEngineGroup.fit_iter_all(group, [None], [True, True])


# ------------------------------------------------------------------------------------------------ the flag
def test_flag_default_and_refusal_without_it():
    from safepo.utils import config
    args, _ = config.single_agent_args([])
    assert args.batch_critic_fit is False and config.critic_seed_batch(args) is False
    args, _ = config.single_agent_args(["--seeds", "3", "--batch-critic-fit", "True"])
    assert args.batch_critic_fit is True and config.critic_seed_batch(args) is False        # one seed stays --seed
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "2000"])
    for name in ("cpo", "pcpo", "trpo_lag", "rcpo", "trpo", "natural_pg"):
        mod = __import__(f"safepo.single_agent.{name}", fromlist=["main"])
        with pytest.raises(SystemExit, match="second-order") as ei:
            mod.main(args, {})
        assert "--batch-critic-fit" in str(ei.value)                # the refusal names the flag
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "--batch-critic-fit", "True"])
    assert config.critic_seed_batch(args) is True
    # a namespace built by hand without the attribute (tests, notebooks): off
    import argparse
    assert pytest.raises(SystemExit, config.critic_seed_batch, argparse.Namespace(seed=0, seeds=[1, 2]))
    # focops / cup keep their own refusal, without the flag's sentence
    with pytest.raises(SystemExit, match="focops and cup") as ei:
        config.refuse_seed_batch(args, "focops and cup")
    assert "--batch-critic-fit" not in str(ei.value)


def test_flag_refusals_before_any_device_work(monkeypatch):
    from safepo.single_agent import cpo, trpo_lag
    from safepo.utils import config
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "--batch-critic-fit", "True"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    for mod in (cpo, trpo_lag):
        with pytest.raises(SystemExit, match="torchrun"):
            mod.main(args, {})
    monkeypatch.delenv("WORLD_SIZE")
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "4", "4", "--batch-critic-fit", "True"])
    with pytest.raises(SystemExit, match="same seed twice"):
        cpo.main(args, {})
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--batch-critic-fit", "True", "--seeds"] + [str(s) for s in range(25)])
    with pytest.raises(SystemExit, match="at most 24"):
        trpo_lag.main(args, {})


def test_help_text_names_the_flag_and_its_measurement(capsys):
    from safepo.single_agent import benchmark
    from safepo.utils import config
    for parse, flag in ((config.single_agent_args, "--batch-critic-fit"), (benchmark.parse_args, "--batch-second-order")):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            parse(["--help"])
        text = " ".join(capsys.readouterr().out.split())
        assert flag in text and "profiles/seed_batch_critic/step_times.txt" in text, flag


def _cmd(algo, task, seeds, gpu, extra=()):
    from safepo.single_agent import benchmark
    import shlex
    head = [shlex.quote(sys.executable), shlex.quote(os.path.join(benchmark.HERE, f"{algo}.py")), "--task", task, "--seed", str(seeds[0])]
    if len(seeds) > 1:
        head += ["--seeds"] + [str(s) for s in seeds]
    return " ".join(head + list(extra) + ["--write-terminal", "False", "--experiment", "benchmark", "--total-steps", "10000000",
                                            "--num-envs", "10", "--steps-per-epoch", "20000", "--device-id", str(gpu)])


def test_launcher_without_the_flag_prints_what_it_prints_today(capsys, monkeypatch):
    from safepo.single_agent import benchmark
    monkeypatch.setattr(benchmark, "visible_gpus", lambda: 1)
    base = ["--workers", "0", "--tasks", "SynthSafe-v0", "--algo", "ppo_lag", "cpo", "trpo_lag", "--num-seeds", "3", "--seeds-per-run", "3"]
    capsys.readouterr()
    got = benchmark.main(base)
    out = capsys.readouterr().out
    want = [_cmd("ppo_lag", "SynthSafe-v0", [0, 1000, 2000], 0)] + [_cmd(a, "SynthSafe-v0", [s], 0) for a in ("cpo", "trpo_lag")
                                                                     for s in (0, 1000, 2000)]
    assert got == want
    assert out == "======= commands to run:\n" + "".join(c + "\n" for c in want) + \
        "not running the experiments because --workers is set to 0; just printing the commands to run\n"
    assert "--batch-critic-fit" not in out


def test_launcher_with_the_flag_groups_the_second_order_scripts(monkeypatch):
    from safepo.single_agent import benchmark
    monkeypatch.setattr(benchmark, "visible_gpus", lambda: 1)
    flag = ("--batch-critic-fit", "True")
    tasks = ["SynthSafe-v0", "SafetyAntVelocity-v1", "SafetyCarGoal1-v0", "SafetyHumanoidVelocity-v1"]
    got = benchmark.main(["--workers", "0", "--tasks"] + tasks + ["--algo", "ppo_lag", "cpo", "focops", "--num-seeds", "3",
                                                                  "--seeds-per-run", "3", "--batch-second-order"])
    seeds = [0, 1000, 2000]
    want = []
    for t in tasks:
        want.append(_cmd("ppo_lag", t, seeds, 0)) if "Humanoid" not in t else want.extend(_cmd("ppo_lag", t, [s], 0) for s in seeds)
        if t in ("SynthSafe-v0", "SafetyAntVelocity-v1"):           # observations up to 64: CPOEngine
            want.append(_cmd("cpo", t, seeds, 0, flag))
        else:
            want.extend(_cmd("cpo", t, [s], 0) for s in seeds)
        want.extend(_cmd("focops", t, [s], 0) for s in seeds)
    assert got == want
    # every script of the family, and the cap of 24 per command
    got = benchmark.main(["--workers", "0", "--tasks", "SynthSafe-v0", "--algo", "cpo", "pcpo", "rcpo", "trpo_lag", "trpo", "natural_pg",
                          "ppo_lag", "--num-seeds", "30", "--seeds-per-run", "30", "--batch-second-order"])
    s30 = [1000 * k for k in range(30)]
    want = [c for a in ("cpo", "pcpo", "rcpo", "trpo_lag", "trpo", "natural_pg")
            for c in (_cmd(a, "SynthSafe-v0", s30[:24], 0, flag), _cmd(a, "SynthSafe-v0", s30[24:], 0, flag))]
    assert got == want + [_cmd("ppo_lag", "SynthSafe-v0", s30, 0)]
    # --seeds-per-run 1: the flag alone changes nothing
    base = ["--workers", "0", "--tasks", "SynthSafe-v0", "--algo", "cpo", "--num-seeds", "2"]
    assert benchmark.main(base + ["--batch-second-order"]) == benchmark.main(base)
