"""CPU tests (no GPU) of the seed-batched PPO-Lagrangian path: the new entry points are declared, exported and bound; the
support query's truth table; the launch's block -> (run, workgroup) mapping (the function the kernel itself uses); the group's
KL-stopped loop on recording stand-in engines against PPOLagEngine.update's own loop; the per-run generator states; the sweep
launcher's --seeds-per-run."""
import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("spo_ppo_lag_update_iter_multi", "spo_update_rs_multi_supported", "spo_rs_multi_block_map",
               "spo_debug_rs_multi_counters", "spo_update_rs_multi_matches_single")


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


# ------------------------------------------------------------------------------------------------ symbols, truth table
def test_symbols_declared_exported_and_bound(lib):
    from safepo import _abi
    header = open(os.path.join(ROOT, "include", "safepo_hip.h")).read()
    assert "SPO_RS_MAX_REPLICAS 32" in header and _abi.RS_MAX_REPLICAS == 32
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert "spo_update_replica" in header
    # the struct's binding has the header's fields in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} spo_update_replica;", header, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert [n for n, _ in _abi.UpdateReplica._fields_] == names, names


def test_support_truth_table(lib):
    f = lib.spo_update_rs_multi_supported
    for D in (0, 1, 60, 64, 65, 66, 100, 127, 128, 129, 200):
        for A in (0, 1, 8, 16, 17):
            for B in (0, 1, 32, 64, 65, 128, 129):
                single = bool(lib.spo_update_rs_supported(D, A, B, 3) or lib.spo_update_rs128_supported(D, A, B, 3))
                for S in (0, 1, 8, 9, 32, 33):
                    assert f(D, A, B, S) == int(single and 1 <= S <= 32), (D, A, B, S)
    assert f(60, 8, 64, 3) == 1 and f(72, 2, 64, 17) == 1 and f(5, 1, 20, 9) == 1


def test_routing_query_follows_the_single_launch(lib):
    """spo_update_rs_multi_matches_single: the library's own answer to "would the stand-alone launch run the two-row-group
    row-split form here" -- under the default routing, every shape the batched form supports; never a shape it does not."""
    g = lib.spo_update_rs_multi_matches_single
    default = not any(os.environ.get(k) for k in ("SPO_UPDATE_FORM", "SPO_RS_ROWS", "SPO_RS_OBS128"))
    for D in (0, 1, 16, 17, 60, 64, 65, 128, 129):
        for A in (0, 1, 8, 16, 17):
            for B in (0, 1, 20, 64, 65, 128):
                sup = lib.spo_update_rs_multi_supported(D, A, B, 1)
                assert g(D, A, B) in (0, 1) and g(D, A, B) <= sup, (D, A, B)
                if default:
                    assert g(D, A, B) == sup, (D, A, B)


def test_host_validation_happens_before_any_device_work(lib):
    """Refused on the host (no GPU here: anything that reached HIP would fail differently): the replica count, a shape outside
    the form, unequal shapes, a shared theta."""
    from safepo import _abi
    f = lib.spo_ppo_lag_update_iter_multi

    def table(S, D=60, A=8, batch=64):
        reps = (_abi.UpdateReplica * max(S, 1))()
        for i in range(S):
            base = 0x1000 * (i + 1)
            r = reps[i]
            for k, name in enumerate(("theta", "adam_m", "adam_v", "obs", "act", "logp_old", "target_r", "target_c", "adv", "perm",
                                      "losses_out", "sync_ws")):
                setattr(r, name, base + 64 * k)
            r.cfg = _abi.PpoCfg(obs_dim=D, act_dim=A, batch=batch)
            r.active = 1
        return reps

    def err():
        return lib.spo_last_error().decode()

    assert f(table(1), 0, 128, None) < 0 and "replicas" in err()
    assert f(table(33), 33, 128, None) < 0 and "replicas" in err()
    assert f(table(2), 2, 0, None) < 0
    assert f(table(2, D=129), 2, 128, None) < 0 and "no replica-batched form" in err()
    assert f(table(2, batch=65), 2, 128, None) < 0 and "no replica-batched form" in err()
    t = table(3)
    t[2].cfg.act_dim = 4
    assert f(t, 3, 128, None) < 0 and "replica 2" in err()
    t = table(3)
    t[2].theta = t[0].theta
    assert f(t, 3, 128, None) < 0 and "share" in err()
    t = table(3)
    t[1].sync_ws = t[0].sync_ws
    assert f(t, 3, 128, None) < 0 and "share" in err()
    t = table(2)
    t[1].adv = None
    assert f(t, 2, 128, None) < 0 and "null pointer in replica 1" in err()


# ------------------------------------------------------------------------------------------------ block mapping
def _walk(lib, S, blocks):
    out = []
    for b in blocks:
        rep, wg = ctypes.c_int(-1), ctypes.c_int(-1)
        out.append((b, lib.spo_rs_multi_block_map(b, S, ctypes.byref(rep), ctypes.byref(wg)), rep.value, wg.value))
    return out


@pytest.mark.parametrize("S", range(1, 33))
def test_block_mapping(lib, S):
    grid = 8 * 6 * ((S + 7) // 8)
    seen, label_of, per_label = {}, {}, [0] * 8
    for b, work, rep, wg in _walk(lib, S, range(grid)):
        want_rep, want_wg = 8 * ((b >> 3) // 6) + (b & 7), (b >> 3) % 6
        if want_rep >= S:
            assert work == 0, (S, b)                   # blocks beyond S report no work
            continue
        assert work == 1 and (rep, wg) == (want_rep, want_wg), (S, b, rep, wg)
        assert 0 <= rep < S and 0 <= wg < 6
        assert (rep, wg) not in seen, (S, b, seen[(rep, wg)])
        seen[(rep, wg)] = b
        assert label_of.setdefault(rep, b & 7) == (b & 7)          # the six blocks of a run share a label (an XCD)
        per_label[b & 7] += 1
    assert len(seen) == 6 * S                                      # every (run, workgroup) exactly once
    assert max(per_label) <= 6 * ((S + 7) // 8)
    assert all(label_of[r] == (r & 7) for r in range(S))           # runs r, r + 8, ... share one
    for _b, work, _r, _w in _walk(lib, S, (-1, grid, grid + 5, 8 * 6 * 4)):
        assert work == 0
    assert lib.spo_rs_multi_block_map(0, 0, None, None) == 0 and lib.spo_rs_multi_block_map(0, 33, None, None) == 0


# ------------------------------------------------------------------------------------------------ the group's KL-stopped loop
class _StubBuffer:
    def __init__(self, log):
        self.log = log

    def compute_gae(self, lam, comm):
        self.log.append(("gae", lam))

    def reset(self):
        self.log.append(("reset",))


class _StubComm:
    world_size = 1


class _StubEngine:
    """Records what the update loop asks of an engine; KL values come from a script."""
    D, A, M, dev = 4, 2, 12, torch.device("cpu")

    def __init__(self, kls, learning_iters, target_kl):
        self.log, self.kls = [], list(kls)
        self.cfg = {"learning_iters": learning_iters, "target_kl": target_kl}
        self.comm, self.buffer = _StubComm(), _StubBuffer(self.log)

    def snapshot_old_distribution(self):
        self.log.append(("snapshot",))

    def learning_iter(self, perm):
        self.log.append(("iter", perm))
        return torch.full((2, 3), float(len(self.log)))

    def kl_launch(self):
        self.log.append(("kl_launch",))

    def kl_read(self):
        self.log.append(("kl_read",))
        return self.kls.pop(0)

    def check_sync_error(self):
        self.log.append(("check",))

    def perm_fn(self, it):
        self.log.append(("perm", it))
        return ("perm", it)


SCRIPTS = [([0.9], 1), ([0.1, 0.9], 2), ([0.1, 0.2, 0.3, 0.4], 4)]       # (KL after every pass, passes until the stop)


def test_group_kl_loop_with_stub_engines():
    from safepo.common.engine import PPOLagEngine
    from safepo.common.engine_group import PPOLagEngineGroup
    # the stand-alone loop itself, on the same stand-ins
    alone = [_StubEngine(kls, 4, 0.5) for kls, _ in SCRIPTS]
    alone_out = [PPOLagEngine.update(e, 0.25 * i, e.perm_fn) for i, e in enumerate(alone)]
    assert [o["stop_iter"] for o in alone_out] == [n for _, n in SCRIPTS]
    es = [_StubEngine(kls, 4, 0.5) for kls, _ in SCRIPTS]
    group = PPOLagEngineGroup(es)
    seen_active = []
    inner = group.learning_iter_all

    def recording(perms, active=None):
        seen_active.append(list(active))
        return inner(perms, active)

    group.learning_iter_all = recording
    outs = group.update([0.25 * i for i in range(3)], [e.perm_fn for e in es])
    assert seen_active == [[True, True, True], [False, True, True], [False, False, True], [False, False, True]]
    for e, a, (_, n) in zip(es, alone, SCRIPTS):
        assert sum(1 for x in e.log if x[0] == "iter") == n
        assert e.log == a.log                     # per run: the same calls in the same order, shuffle draws and KL reads included
    for o, ao in zip(outs, alone_out):
        assert o["stop_iter"] == ao["stop_iter"] and o["kl"] == ao["kl"]
        assert (o["loss_r"], o["loss_c"], o["loss_pi"]) == (ao["loss_r"], ao["loss_c"], ao["loss_pi"])
        assert len(o["losses"]) == len(ao["losses"]) and all(torch.equal(x, y) for x, y in zip(o["losses"], ao["losses"]))


def test_group_loop_with_no_learning_iterations():
    from safepo.common.engine_group import PPOLagEngineGroup
    es = [_StubEngine([], 0, 0.5), _StubEngine([0.9], 3, 0.5)]
    outs = PPOLagEngineGroup(es).update([0.0, 0.0], [e.perm_fn for e in es])
    assert outs[0]["stop_iter"] == 0 and outs[0]["kl"] == 1.0 and np.isnan(outs[0]["loss_r"]) and outs[0]["losses"] == []
    assert outs[1]["stop_iter"] == 1 and not any(x[0] == "iter" for x in es[0].log)


# ------------------------------------------------------------------------------------------------ per-run generator states
def test_replica_rng_context():
    from safepo.common.engine_group import ReplicaRNG
    a, b = 11, 2000
    torch.manual_seed(777); np.random.seed(777); random.seed(777)
    outer_before = torch.get_rng_state().clone()
    ra, rb = ReplicaRNG(a), ReplicaRNG(b)
    got = {a: [], b: []}
    with ra:
        got[a].append(torch.randn(3)); got[a].append(np.random.rand(2)); got[a].append(random.random())
    with rb:
        got[b].append(torch.randperm(7)); got[b].append(torch.randn(2, 2))
    with ra:
        got[a].append(torch.randperm(5))
    with rb:
        got[b].append(np.random.rand(3)); got[b].append(random.random()); got[b].append(torch.randn(1))
    with ra:
        got[a].append(torch.randn(4))
    assert torch.equal(torch.get_rng_state(), outer_before)          # nothing was drawn from the process-wide state
    outside = torch.randn(2)
    # every run's sequence is the one after a plain seeding of its seed
    random.seed(a); np.random.seed(a); torch.manual_seed(a)
    want_a = [torch.randn(3), np.random.rand(2), random.random(), torch.randperm(5), torch.randn(4)]
    random.seed(b); np.random.seed(b); torch.manual_seed(b)
    want_b = [torch.randperm(7), torch.randn(2, 2), np.random.rand(3), random.random(), torch.randn(1)]
    for g, w in ((got[a], want_a), (got[b], want_b)):
        assert len(g) == len(w)
        for x, y in zip(g, w):
            assert torch.equal(x, y) if torch.is_tensor(x) else np.array_equal(x, y)
    torch.manual_seed(777)
    assert torch.equal(torch.randn(2), outside)


# ------------------------------------------------------------------------------------------------ launcher, flags
def test_launcher_seeds_per_run(capsys):
    from safepo.single_agent import benchmark
    base = ["--workers", "0", "--tasks", "SynthSafe-v0", "SafetyDoggoGoal1-v0", "--algo", "ppo_lag", "cppo_pid", "--num-seeds", "3"]
    plain = benchmark.main(base)
    assert benchmark.main(base + ["--seeds-per-run", "1"]) == plain and len(plain) == 3 * 2 * 2
    capsys.readouterr()
    benchmark.main(base)
    out_plain = capsys.readouterr().out
    benchmark.main(base + ["--seeds-per-run", "1"])
    assert capsys.readouterr().out == out_plain                    # byte for byte what is printed today
    three = benchmark.main(base + ["--seeds-per-run", "3"])
    assert len(three) == 2 * 2                                     # one command per (task, algorithm)
    for c in three:
        assert "--seed 0 --seeds 0 1000 2000 " in c
    assert {(c.split("--task ")[1].split()[0], os.path.basename(c.split()[1])) for c in three} == \
        {(t, a + ".py") for t in ("SynthSafe-v0", "SafetyDoggoGoal1-v0") for a in ("ppo_lag", "cppo_pid")}
    # algorithms (and tasks) without a seed-batched form keep one command per seed inside a grouped sweep
    mixed = benchmark.main(["--workers", "0", "--tasks", "SynthSafe-v0", "SafetyHumanoidVelocity-v1", "--algo", "ppo_lag", "focops", "cpo",
                            "--num-seeds", "3", "--seeds-per-run", "3"])
    with_seeds = [c for c in mixed if "--seeds" in c]
    assert len(with_seeds) == 1 and "ppo_lag.py --task SynthSafe-v0 --seed 0 --seeds 0 1000 2000 " in with_seeds[0]
    assert len(mixed) == 1 + 5 * 3
    for algo, task in (("focops", "SynthSafe-v0"), ("cpo", "SynthSafe-v0"), ("ppo_lag", "SafetyHumanoidVelocity-v1")):
        assert sorted(int(c.split("--seed ")[1].split()[0]) for c in mixed if f"{algo}.py --task {task} " in c) == [0, 1000, 2000]
    two = benchmark.main(base + ["--seeds-per-run", "2", "--start-seed", "5"])
    assert len(two) == 2 * 2 * 2
    assert sum("--seeds 5 1005 " in c for c in two) == 4 and sum("--seed 2005 --write-terminal" in c for c in two) == 4


def test_seeds_flag_and_refusals():
    from safepo.utils import config
    args, _ = config.single_agent_args([])
    assert args.seeds is None and config.seed_list(args) == [0]
    assert config.seed_list(config.build_parser().parse_args([])) == [0]       # (a namespace without the flag: [--seed])
    args, _ = config.single_agent_args(["--seed", "7"])
    assert config.seed_list(args) == [7]
    config.refuse_seed_batch(args, "x")                             # one seed: nothing to refuse
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "2000"])
    assert config.seed_list(args) == [0, 1000, 2000]
    with pytest.raises(SystemExit, match="focops and cup"):
        from safepo.single_agent import focops
        focops.main(args, {})
    with pytest.raises(SystemExit, match="second-order"):
        from safepo.single_agent import trpo_lag
        trpo_lag.main(args, {})
    with pytest.raises(SystemExit, match="second-order"):
        from safepo.single_agent import cpo
        cpo.main(args, {})
