"""CPU tests (no GPU) of the seed-batched split critic fit (65-128 observations): the entry points are declared, exported and
bound; the support table at its edges; the block -> (run, workgroup) mapping of the launch (the function the kernel itself uses);
what the launch refuses on the host; CPOEngineGroup(split_form=True)'s loop on recording stand-in engines, its fallback and its
error path; the opt-in flags of the scripts and of the sweep launcher; and the clip condition of the GPU tests' problems (both
clipped and unclipped steps occur on the very initialisations test_gpu_seed_batch_critic_split.py uses)."""
import ctypes
import os
import random
import re
import shlex
import sys

import numpy as np
import pytest
import torch

import seed_batch_critic_split_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("spo_critic_fit_iter_split_multi", "spo_critic_fit_split_multi_supported", "spo_critic_fit_split_multi_block_map",
               "spo_debug_critic_fit_split_multi_counters")
S_CAP = 32


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
    assert "SPO_CRITIC_SPLIT_MAX_REPLICAS 32" in header and _abi.CRITIC_SPLIT_MAX_REPLICAS == S_CAP
    assert "SPO_RS_CRITIC_MAX_REPLICAS 24" in header and _abi.RS_CRITIC_MAX_REPLICAS == 24         # the row-split group's cap stays
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name
    body = re.search(r"typedef struct \{([^}]*)\} spo_critic_fit_split_replica;", header, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
    assert [n for n, _ in _abi.CriticFitSplitReplica._fields_] == names, names
    assert names == ["theta0", "adam_m0", "adam_v0", "theta1", "adam_m1", "adam_v1", "adam_step", "obs", "target_r", "target_c",
                     "perm0", "perm1", "stale_sq_io0", "stale_sq_io1", "losses0", "losses1", "sync_ws0", "sync_ws1", "regions2",
                     "step0", "cfg", "active"]
    # the layout the C side reads: 17 pointers and an int64 (144 bytes), two region pointers, step0, the cfg, active
    f = _abi.CriticFitSplitReplica
    assert f.regions2.offset == 18 * 8 and f.step0.offset == 20 * 8 and f.cfg.offset == 20 * 8 + 4
    assert f.active.offset == f.cfg.offset + ctypes.sizeof(_abi.PpoCfg) and ctypes.sizeof(f) % 8 == 0


def test_counters_without_a_launch_need_no_device(lib):
    c3 = (ctypes.c_ulonglong * 3)(7, 7, 7)
    assert lib.spo_debug_critic_fit_split_multi_counters(c3, 0) == 0 and list(c3) == [0, 0, 0]
    assert lib.spo_debug_critic_fit_split_multi_counters(None, 0) < 0


# ------------------------------------------------------------------------------------------------ support table
def test_supported_table(lib):
    f = lib.spo_critic_fit_split_multi_supported
    for D in (0, 1, 60, 64, 65, 72, 128, 129, 512):
        for B in (0, 1, 63, 64, 65, 128):
            for S in (0, 1, 8, 24, 25, 32, 33):
                assert f(D, B, S) == int(65 <= D <= 128 and 1 <= B <= 64 and 1 <= S <= S_CAP), (D, B, S)
    # the edges by name: 64 / 65 and 128 / 129 observations, 64 / 65 rows per half, 32 / 33 runs
    assert [f(D, 64, 3) for D in (64, 65, 128, 129)] == [0, 1, 1, 0]
    assert [f(72, B, 3) for B in (64, 65)] == [1, 0]
    assert [f(72, 64, S) for S in (32, 33)] == [1, 0]


# ------------------------------------------------------------------------------------------------ block mapping
def _walk(fn, S, blocks):
    out = []
    for b in blocks:
        rep, wg = ctypes.c_int(-1), ctypes.c_int(-1)
        out.append((b, fn(b, S, ctypes.byref(rep), ctypes.byref(wg)), rep.value, wg.value))
    return out


@pytest.mark.parametrize("S", [1, 8, 9, 17, 32])
def test_block_mapping(lib, S):
    f = lib.spo_critic_fit_split_multi_block_map
    grid = 32 * ((S + 7) // 8)
    seen, label_of, per_label = {}, {}, [0] * 8
    for b, work, rep, wg in _walk(f, S, range(grid)):
        x, k = b & 7, b >> 3
        want_rep, want_wg = 8 * (k // 4) + x, k % 4
        if want_rep >= S:
            assert work == 0, (S, b)
            continue
        assert work == 1 and (rep, wg) == (want_rep, want_wg), (S, b, rep, wg)
        assert 0 <= rep < S and 0 <= wg < 4
        assert (rep, wg) not in seen, (S, b, seen[(rep, wg)])       # every block serves at most one (run, workgroup)
        seen[(rep, wg)] = b
        assert label_of.setdefault(rep, x) == x                      # the four blocks of a run share a label (an XCD)
        per_label[x] += 1
    assert len(seen) == 4 * S                                        # each run gets workgroups 0..3 exactly once
    assert all(label_of[r] == (r & 7) for r in range(S))             # ... all on label run & 7
    assert max(per_label) <= 16                                      # at most four runs = 16 one-CU blocks on an XCD's 32 CUs
    for _b, work, _r, _w in _walk(f, S, (-1, grid, grid + 5, 32 * 4)):
        assert work == 0                                             # outside the grid (32 ceil(S / 8) blocks)
    assert f(0, S, None, None) == 0                                  # (no place to put the answer)


def test_block_mapping_refuses_run_counts_outside_the_cap(lib):
    rep, wg = ctypes.c_int(-1), ctypes.c_int(-1)
    f = lambda b, S: lib.spo_critic_fit_split_multi_block_map(b, S, ctypes.byref(rep), ctypes.byref(wg))
    assert f(0, 0) == 0 and f(0, S_CAP + 1) == 0 and f(0, -3) == 0
    assert f(0, 1) == 1 and f(0, S_CAP) == 1 and f(127, S_CAP) == 1 and (rep.value, wg.value) == (31, 3)


# ------------------------------------------------------------------------------------------------ host refusals
POINTERS = ("theta0", "adam_m0", "adam_v0", "theta1", "adam_m1", "adam_v1", "obs", "target_r", "target_c", "perm0", "perm1",
            "stale_sq_io0", "stale_sq_io1", "losses0", "losses1", "sync_ws0", "sync_ws1")


def _table(S, D=72, A=2, batch=64):
    from safepo import _abi
    reps = (_abi.CriticFitSplitReplica * max(S, 1))()
    for i in range(S):
        base = 0x100000 * (i + 1)
        r = reps[i]
        for k, name in enumerate(POINTERS):
            setattr(r, name, base + 256 * k)
        r.regions2[0], r.regions2[1] = base + 0x10000, base + 0x20000
        r.cfg = _abi.PpoCfg(obs_dim=D, act_dim=A, batch=batch)
        r.active = 1
    return reps


def test_host_validation_happens_before_any_device_work(lib):
    """No GPU here: anything that reached HIP would fail with a HIP error instead of these messages."""
    f = lib.spo_critic_fit_iter_split_multi

    def err():
        return lib.spo_last_error().decode()

    assert f(None, 2, 192, None) < 0 and "null replica table" in err()
    assert f(_table(1), 0, 192, None) < 0 and "replicas" in err()
    assert f(_table(33), 33, 192, None) < 0 and "replicas" in err()
    assert f(_table(2), 2, 0, None) < 0 and "bad sizes" in err()
    assert f(_table(2), 2, -64, None) < 0 and "bad sizes" in err()
    for kw in ({"D": 64}, {"D": 129}, {"batch": 65}, {"batch": 128}):
        assert f(_table(2, **kw), 2, 192, None) < 0 and ("no seed-batched split form" in err() or "obs_dim" in err()), kw
    assert f(_table(2, D=64), 2, 192, None) < 0 and "no seed-batched split form" in err()
    for field, value in (("obs_dim", 80), ("act_dim", 3), ("batch", 32)):
        t = _table(3)
        setattr(t[2].cfg, field, value)
        assert f(t, 3, 192, None) < 0 and "replica 2 has obs_dim / act_dim / batch" in err(), field
    for field in POINTERS:
        t = _table(2)
        setattr(t[1], field, None)
        assert f(t, 2, 192, None) < 0 and "null pointer in replica 1" in err(), field
    for k in range(2):
        t = _table(2)
        t[1].regions2[k] = None
        assert f(t, 2, 192, None) < 0 and "null pointer in replica 1" in err()
    for a, b in (("theta0", "theta0"), ("theta1", "theta0"), ("theta0", "theta1"), ("sync_ws0", "sync_ws0"), ("sync_ws1", "sync_ws0"),
                 ("sync_ws1", "sync_ws1")):
        t = _table(3)
        setattr(t[2], a, getattr(t[0], b))
        assert f(t, 3, 192, None) < 0 and "share theta or sync_ws" in err() and "0 and 2" in err(), (a, b)
    for a, b in (("theta1", "theta0"), ("adam_m1", "adam_m0"), ("adam_v1", "adam_v0"), ("sync_ws1", "sync_ws0"), ("losses1", "losses0"),
                 ("stale_sq_io1", "stale_sq_io0")):
        t = _table(2)
        setattr(t[1], a, getattr(t[1], b))
        assert f(t, 2, 192, None) < 0 and "replica 1: the two halves need separate replicas" in err(), a
    t = _table(2)
    t[0].adam_step = -1
    assert f(t, 2, 192, None) < 0 and "negative adam_step" in err()
    # a run that sits out may leave its pointers null -- and with every run sitting out nothing is enqueued (no HIP call: this
    # returns 0 on a machine without a GPU)
    t = _table(3)
    for r in t:
        r.active = 0
        for name in POINTERS:
            setattr(r, name, None)
    assert f(t, 3, 192, None) == 0
    t = _table(3)
    for r in t:
        r.active = 0
    assert f(t, 3, 192, None) == 0


# ------------------------------------------------------------------------------------------------ CPOEngineGroup on stand-ins
class _StubComm:
    world_size = 1


class _StubPolicy:
    def __init__(self, v):
        self.theta = torch.full((6,), float(v))


class _StubEngine:
    """Records what the group asks of an engine; critic_fit is CPOEngine.critic_fit's loop without the launch.  Holds the state
    the split loop reads and restores (parameters, moments, stale norm, step counts, both error words)."""
    D, A, M, dev = 72, 2, 256, torch.device("cpu")

    def __init__(self, learning_iters, v=1.0):
        self.log, self.cfg, self.comm = [], {"learning_iters": learning_iters, "batch_size": 128}, _StubComm()
        self.policy, self.adam_m, self.adam_v = _StubPolicy(v), torch.full((6,), v + 0.25), torch.full((6,), v + 0.5)
        self.stale_sq, self.adam_step = torch.tensor([v + 0.75]), 7
        self.sync_ws = torch.zeros(32, dtype=torch.int64)
        self._st = {"theta1": torch.zeros(6), "m1": torch.zeros(6), "v1": torch.zeros(6), "stale1": torch.zeros(1),
                    "sync_ws": torch.zeros(32, dtype=torch.int64), "step": 64}

    def _split_setup(self):
        return self._st

    def critic_fit(self, perm_fn=None):
        ls = []
        for it in range(self.cfg["learning_iters"]):
            self.log.append(("launch", it, perm_fn(it)))
            ls.append(torch.full((2, 2), float(10 * it + len(self.log))))
        self.log.append(("check",))
        means = torch.cat(ls, 0).mean(0).tolist() if ls else [float("nan")] * 2
        return {"loss_r": means[0], "loss_c": means[1], "losses": ls}

    def check_sync_error(self):
        self.log.append(("check",))

    def perm_fn(self, it):
        self.log.append(("perm", it))
        return ("perm", it)


def _recording_group(es, on_launch=None):
    """A split_form group whose launch is replaced by a recorder that moves the state the way the launch would."""
    from safepo.common.engine_group import CPOEngineGroup
    group = CPOEngineGroup(es, split_form=True)
    group.batched_split = lambda: True
    launches = []

    def fit_iter_split_all(perms, active=None):
        launches.append((list(perms), list(active)))
        out = []
        for i, e in enumerate(es):
            if not active[i]:
                out.append(None)
                continue
            e.log.append(("launch", len(launches) - 1, perms[i]))
            assert torch.equal(e._st["theta1"], e.policy.theta) or len(launches) > 1      # copied before the first launch
            e.policy.theta += 1.0; e.adam_m += 1.0; e.adam_v += 1.0; e.stale_sq *= 0.5
            e.adam_step += 2
            e._st["step"] += 2
            out.append(torch.tensor([[1.0 + i, 2.0 * len(launches), -1.0]] * 2))
        if on_launch is not None:
            on_launch(len(launches) - 1)
        return out

    group.fit_iter_split_all = fit_iter_split_all
    return group, launches


def test_group_falls_back_to_per_engine_critic_fit_where_not_batched_split():
    from safepo.common.engine_group import CPOEngineGroup
    es = [_StubEngine(n) for n in (1, 3, 2)]
    group = CPOEngineGroup(es, split_form=True)
    assert len(group) == 3 and not group.batched_split() and not group.batched()      # (stand-ins: no library behind them)
    outs = group.critic_fit_all([e.perm_fn for e in es])
    alone = [_StubEngine(n) for n in (1, 3, 2)]
    alone_out = [e.critic_fit(e.perm_fn) for e in alone]
    for e, a, o, ao in zip(es, alone, outs, alone_out):
        assert e.log == a.log
        assert (o["loss_r"], o["loss_c"]) == (ao["loss_r"], ao["loss_c"]) and len(o["losses"]) == len(ao["losses"])
    # without the switch batched_split() is never true, whatever the engines
    g = CPOEngineGroup([_StubEngine(1)])
    assert g.split_form is False and not g.batched_split()


def test_group_split_loop_order_with_recorded_launches():
    """The split loop itself (the launch replaced by a recorder): the second replica is a copy of the first before the first
    launch; per run, iteration it's shuffle is drawn before launch it and after launch it - 1, as _critic_fit_split draws it; a
    run with fewer learning_iters sits out the later launches; the error words are read once, after the last launch."""
    n_its = (1, 3, 2)
    es = [_StubEngine(n, v=1.0 + i) for i, n in enumerate(n_its)]
    group, launches = _recording_group(es)
    outs = group.critic_fit_all([e.perm_fn for e in es])
    assert [a for _, a in launches] == [[True, True, True], [False, True, True], [False, True, False]]
    for (perms, active) in launches:
        assert all((p is None) == (not a) for p, a in zip(perms, active))
    for i, (e, n) in enumerate(zip(es, n_its)):
        want = [x for it in range(n) for x in (("perm", it), ("launch", it, ("perm", it)))]
        assert e.log == want, (i, e.log)                             # (no per-engine check: the group reads the words itself)
        ls = outs[i]["losses"]
        assert len(ls) == n and all(x.shape == (2, 2) for x in ls)   # the [n_mb, 2] views critic_fit returns
        means = torch.cat(ls, 0).mean(0).tolist()
        assert (outs[i]["loss_r"], outs[i]["loss_c"]) == (means[0], means[1])
        assert e.adam_step == 7 + 2 * n and e._st["step"] == 64 + 2 * n
    # no learning iterations at all: nothing launched, NaN means
    es0 = [_StubEngine(0), _StubEngine(0)]
    g0, l0 = _recording_group(es0)
    o = g0.critic_fit_all()
    assert l0 == [] and all(np.isnan(x["loss_r"]) and x["losses"] == [] for x in o)


def test_group_split_loop_draws_default_shuffles_under_the_runs_generators():
    from safepo.common.engine_group import ReplicaRNG
    seeds = (5, 77)
    es = [_StubEngine(2) for _ in seeds]
    group, launches = _recording_group(es)
    group.rngs = [ReplicaRNG(s) for s in seeds]
    outer = torch.get_rng_state().clone()
    group.critic_fit_all()
    assert torch.equal(torch.get_rng_state(), outer)               # nothing drawn from the process-wide state
    for e, s in zip(es, seeds):
        torch.manual_seed(s)
        want = [torch.randperm(e.M).to(torch.int32) for _ in range(2)]
        got = [x[2] for x in e.log if x[0] == "launch"]
        assert len(got) == 2 and all(g.dtype == torch.int32 and torch.equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("word", ["first", "second"])
def test_group_split_error_restores_every_run_and_names_the_run(word):
    from safepo import _abi
    es = [_StubEngine(2, v=1.0 + i) for i in range(3)]
    before = [(e.policy.theta.clone(), e.adam_m.clone(), e.adam_v.clone(), e.stale_sq.clone(), e.adam_step) for e in es]

    def on_launch(k):
        if k == 1:                                                  # the exchange of run 1 gave up during the second launch
            (es[1].sync_ws if word == "first" else es[1]._st["sync_ws"])[8] = 2

    group, launches = _recording_group(es, on_launch)
    with pytest.raises(_abi.SpoError, match=r"replica 1 of 3: split critic fit: exchange error 2"):
        group.critic_fit_all([e.perm_fn for e in es])
    assert len(launches) == 2
    for e, b in zip(es, before):
        assert torch.equal(e.policy.theta, b[0]) and torch.equal(e.adam_m, b[1]) and torch.equal(e.adam_v, b[2])
        assert torch.equal(e.stale_sq, b[3]) and e.adam_step == b[4]
        assert int(e.sync_ws[8]) == 0 and int(e._st["sync_ws"][8]) == 0          # the words are cleared


def test_group_argument_checks():
    from safepo import _abi
    from safepo.common.engine_group import CPOEngineGroup
    from safepo.single_agent.cpo import WideCPOEngine

    def wide(D, persistent=True):
        w = object.__new__(WideCPOEngine)
        w.D, w.A, w.M, w.dev, w.comm = D, 2, 256, torch.device("cpu"), _StubComm()
        w._critics_on_persistent_kernel = persistent
        return w

    with pytest.raises(_abi.SpoError, match="WideCPOEngine"):       # today's behaviour without the switch
        CPOEngineGroup([wide(72)])
    for bad in (wide(64), wide(129), wide(72, persistent=False)):   # outside 65-128 observations / critics on the wide kernels
        with pytest.raises(_abi.SpoError, match="WideCPOEngine"):
            CPOEngineGroup([bad], split_form=True)
    dp = wide(72)
    dp.comm = type("C", (), {"world_size": 2})()
    with pytest.raises(_abi.SpoError, match="world size 1 only"):
        CPOEngineGroup([dp], split_form=True)
    with pytest.raises(_abi.SpoError, match="at most 32"):
        CPOEngineGroup([wide(72) for _ in range(33)], split_form=True)
    with pytest.raises(_abi.SpoError, match="at most 24"):          # stand-ins and CPOEngines keep the cap of 24, switch or not
        CPOEngineGroup([_StubEngine(1) for _ in range(25)], split_form=True)
    with pytest.raises(_abi.SpoError, match="at most 24"):
        CPOEngineGroup([wide(72) for _ in range(25)])
    group = CPOEngineGroup([_StubEngine(1), _StubEngine(1)], split_form=True)
    with pytest.raises(ValueError, match="one perm and one active flag"):
        CPOEngineGroup.fit_iter_split_all(group, [None], [True, True])


# ------------------------------------------------------------------------------------------------ the flags
def test_flag_default_and_refusal_without_the_flag_it_widens():
    from safepo.utils import config
    args, _ = config.single_agent_args([])
    assert args.batch_critic_fit_split is False and args.batch_critic_fit is False
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "--batch-critic-fit-split", "True"])
    assert args.batch_critic_fit_split is True
    for name in ("cpo", "pcpo", "trpo_lag", "rcpo", "trpo", "natural_pg"):
        mod = __import__(f"safepo.single_agent.{name}", fromlist=["main"])
        with pytest.raises(SystemExit, match="--batch-critic-fit True"):
            mod.main(args, {})
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "--batch-critic-fit", "True",
                                        "--batch-critic-fit-split", "True"])
    assert config.critic_seed_batch(args) is True
    args, _ = config.single_agent_args(["--seeds", "3", "--batch-critic-fit", "True", "--batch-critic-fit-split", "True"])
    assert config.critic_seed_batch(args) is False                  # one seed stays --seed


def test_flag_refusals_before_any_device_work(monkeypatch):
    from safepo.single_agent import cpo, trpo_lag
    from safepo.utils import config
    both = ["--batch-critic-fit", "True", "--batch-critic-fit-split", "True"]
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000"] + both)
    monkeypatch.setenv("WORLD_SIZE", "2")
    for mod in (cpo, trpo_lag):
        with pytest.raises(SystemExit, match="torchrun"):
            mod.main(args, {})
    monkeypatch.delenv("WORLD_SIZE")
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "4", "4"] + both)
    with pytest.raises(SystemExit, match="same seed twice"):
        cpo.main(args, {})
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds"] + [str(s) for s in range(33)] + both)
    with pytest.raises(SystemExit, match="at most 32"):
        trpo_lag.main(args, {})
    # without the new flag the cap of 24 holds
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--batch-critic-fit", "True", "--seeds"] + [str(s) for s in range(25)])
    with pytest.raises(SystemExit, match="at most 24"):
        trpo_lag.main(args, {})


def test_help_text_names_the_flags_and_their_measurement(capsys):
    from safepo.single_agent import benchmark
    from safepo.utils import config
    for parse, flag in ((config.single_agent_args, "--batch-critic-fit-split"), (benchmark.parse_args, "--batch-second-order-wide-obs")):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            parse(["--help"])
        text = " ".join(capsys.readouterr().out.split())
        assert flag in text and "profiles/seed_batch_critic_split/step_times.txt" in text, flag
    assert os.path.exists(os.path.join(ROOT, "profiles", "seed_batch_critic_split", "step_times.txt"))


def _cmd(algo, task, seeds, gpu, extra=(), doggo=False):
    from safepo.single_agent import benchmark
    head = [shlex.quote(sys.executable), shlex.quote(os.path.join(benchmark.HERE, f"{algo}.py")), "--task", task, "--seed", str(seeds[0])]
    if len(seeds) > 1:
        head += ["--seeds"] + [str(s) for s in seeds]
    budget = ["100000000", "20", "200000"] if doggo else ["10000000", "10", "20000"]
    return " ".join(head + list(extra) + ["--write-terminal", "False", "--experiment", "benchmark", "--total-steps", budget[0],
                                            "--num-envs", budget[1], "--steps-per-epoch", budget[2], "--device-id", str(gpu)])


TASKS = ["SynthSafe-v0", "SafetyAntVelocity-v1", "SafetyCarGoal1-v0", "SafetyAntButton2-v0", "SafetyDoggoPush1-v0",
         "SafetyRacecarCircle2-v0", "SafetyPointGoal1-v0", "SafetyHumanoidVelocity-v1"]


def test_launcher_without_the_new_flag_prints_what_it_prints_today(monkeypatch):
    from safepo.single_agent import benchmark
    monkeypatch.setattr(benchmark, "visible_gpus", lambda: 1)
    flag = ("--batch-critic-fit", "True")
    got = benchmark.main(["--workers", "0", "--tasks"] + TASKS + ["--algo", "cpo", "--num-seeds", "3", "--seeds-per-run", "3",
                                                                  "--batch-second-order"])
    seeds = [0, 1000, 2000]
    want = []
    for t in TASKS:
        if t in ("SynthSafe-v0", "SafetyAntVelocity-v1", "SafetyPointGoal1-v0"):      # observations up to 64: CPOEngine
            want.append(_cmd("cpo", t, seeds, 0, flag))
        else:                                                        # Car / Ant / Doggo / Racecar navigation, Humanoid: one per seed
            want.extend(_cmd("cpo", t, [s], 0, doggo="Doggo" in t) for s in seeds)
    assert got == want
    assert not any("--batch-critic-fit-split" in c for c in got)
    with pytest.raises(SystemExit, match="--batch-second-order"):  # the new flag needs the one it widens
        benchmark.main(["--workers", "0", "--tasks", "SafetyCarGoal1-v0", "--algo", "cpo", "--seeds-per-run", "3",
                        "--batch-second-order-wide-obs"])


def test_launcher_with_the_new_flag_groups_the_wide_observation_tasks(monkeypatch):
    from safepo.single_agent import benchmark
    monkeypatch.setattr(benchmark, "visible_gpus", lambda: 1)
    flag, both = ("--batch-critic-fit", "True"), ("--batch-critic-fit", "True", "--batch-critic-fit-split", "True")
    got = benchmark.main(["--workers", "0", "--tasks"] + TASKS + ["--algo", "ppo_lag", "cpo", "focops", "--num-seeds", "3",
                                                                  "--seeds-per-run", "3", "--batch-second-order",
                                                                  "--batch-second-order-wide-obs"])
    seeds = [0, 1000, 2000]
    want = []
    for t in TASKS:
        dg = "Doggo" in t
        want.append(_cmd("ppo_lag", t, seeds, 0, doggo=dg)) if "Humanoid" not in t else want.extend(_cmd("ppo_lag", t, [s], 0) for s in seeds)
        if t in ("SynthSafe-v0", "SafetyAntVelocity-v1", "SafetyPointGoal1-v0"):
            want.append(_cmd("cpo", t, seeds, 0, flag))
        elif "Humanoid" in t:                                        # 376 observations: the feature-split critic fit, not batched
            want.extend(_cmd("cpo", t, [s], 0) for s in seeds)
        else:
            want.append(_cmd("cpo", t, seeds, 0, both, doggo=dg))
        want.extend(_cmd("focops", t, [s], 0, doggo=dg) for s in seeds)
    assert got == want
    # every script of the family, and the cap of 32 per command on those tasks (24 stays where it was)
    s40 = [1000 * k for k in range(40)]
    got = benchmark.main(["--workers", "0", "--tasks", "SafetyCarGoal1-v0", "SynthSafe-v0", "--algo", "cpo", "pcpo", "rcpo", "trpo_lag",
                          "trpo", "natural_pg", "--num-seeds", "40", "--seeds-per-run", "32", "--batch-second-order",
                          "--batch-second-order-wide-obs"])
    algos = ("cpo", "pcpo", "rcpo", "trpo_lag", "trpo", "natural_pg")
    want = []
    for group in (s40[:32], s40[32:]):
        for t in ("SafetyCarGoal1-v0", "SynthSafe-v0"):
            for a in algos:
                if t == "SynthSafe-v0":
                    want.extend(_cmd(a, t, group[i:i + 24], 0, flag) for i in range(0, len(group), 24))
                else:
                    want.append(_cmd(a, t, group, 0, both))
    assert got == want
    # --seeds-per-run 1: the flags alone change nothing
    base = ["--workers", "0", "--tasks", "SafetyCarGoal1-v0", "--algo", "cpo", "--num-seeds", "2"]
    assert benchmark.main(base + ["--batch-second-order", "--batch-second-order-wide-obs"]) == benchmark.main(base)


# ------------------------------------------------------------------------------------------------ the clip condition
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_clip_condition_on_the_tests_own_initialisation(shape, monkeypatch):
    """Both clipped and unclipped steps occur among runs 0-2 of the GPU tests' problems: the float32 oracle (CriticFitter,
    cpo.py:541-571) on ActorVCritic's own initialisation has at least one step whose joint gradient norm is above 1.05
    (max_grad_norm 1.0: clipped, stale_sq_io rescaled) and at least one below 0.95 (not clipped)."""
    from oracle import restatement as R
    norms = []
    orig = torch.nn.utils.clip_grad_norm_

    def recording(params, max_norm, *a, **kw):
        n = orig(params, max_norm, *a, **kw)
        norms.append(float(n))
        return n

    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", recording)
    D, A = shape
    for r in range(3):
        pol = C.make_policy(shape, r)
        ref = R.OraclePolicy(D, A)
        ref.load_state_dict({k: v.detach().clone() for k, v in pol.state_dict().items()})
        n_act = sum(p.numel() for p in ref.actor.parameters())
        for p in ref.actor.parameters():                            # any vector of that norm: only its norm enters the clip
            p.grad = torch.full_like(p, float(np.sqrt(C.stale_sq0(r) / n_act)))
        fitter = R.CriticFitter(ref, max_grad_norm=C.MAX_GRAD_NORM)
        obs, _, _, tgt_r, tgt_c, _ = C.make_problem(shape, r)
        for perm in C.make_perms(r):
            for k in range(C.N_MB):
                idx = perm[k * C.BATCH:(k + 1) * C.BATCH].long()
                fitter.minibatch_step(obs[idx], tgt_r[idx], tgt_c[idx])
    assert len(norms) == 3 * 2 * C.N_MB
    print(f"{shape}: joint norms {min(norms):.3f} .. {max(norms):.3f}, {sum(n > 1.0 for n in norms)} of {len(norms)} above 1.0")
    assert max(norms) > 1.05 and min(norms) < 0.95, norms
