"""CPU tests (no GPU) of the seed-batched feature-split update (spo_update_iter_ex_ks_multi, csrc/update_ks.hip;
PPOLagEngineGroup of WidePPOLagEngines; --batch-wide-obs): the support rule and the launch's block -> (run, workgroup) mapping (the
function the kernel itself uses) against Python restatements; the entry points are declared, exported and bound; tables refused on
the host; the scripts' new flag and its refusals; the sweep launcher's command lists."""
import argparse
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("spo_update_iter_ex_ks_multi", "spo_update_ks_multi_supported", "spo_update_ks_multi_block_map",
               "spo_debug_update_ks_multi_counters")


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from safepo import _abi
    return _abi.load(g.LIB)


@pytest.fixture(autouse=True)
def _global_rng_state_is_put_back():
    import random
    import numpy as np
    st = random.getstate(), np.random.get_state(), torch.get_rng_state()
    yield
    random.setstate(st[0]); np.random.set_state(st[1]); torch.set_rng_state(st[2])


def _err(lib):
    return lib.spo_last_error().decode()


def _cap(obs_dim):
    """The rule, restated: at most 24 working blocks per XCD label at 3 S blocks a run, 16 runs at the most."""
    S = (obs_dim + 63) // 64
    return min(16, 8 * (8 // S))


# ------------------------------------------------------------------------------------------------ symbols, the struct
def test_symbols_declared_exported_and_bound(lib):
    from safepo import _abi
    header = open(os.path.join(ROOT, "include", "safepo_hip.h")).read()
    assert "#define SPO_KS_MAX_REPLICAS 16" in header and _abi.KS_MAX_REPLICAS == 16
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name
    c_int, P = ctypes.c_int, ctypes.c_void_p
    assert _abi.PROTOTYPES["spo_update_iter_ex_ks_multi"] == (c_int, [ctypes.POINTER(_abi.UpdateExReplica), c_int, ctypes.c_int64, c_int,
                                                                      c_int, P])
    assert lib.spo_update_iter_ex_ks_multi.argtypes == _abi.PROTOTYPES["spo_update_iter_ex_ks_multi"][1]
    assert _abi.PROTOTYPES["spo_update_ks_multi_supported"] == (c_int, [c_int] * 4)
    assert _abi.PROTOTYPES["spo_update_ks_multi_block_map"] == (c_int, [c_int] * 4 + [ctypes.POINTER(c_int)] * 2)
    assert _abi.PROTOTYPES["spo_debug_update_ks_multi_counters"] == (c_int, [P, c_int])
    # the entry reuses spo_update_ex_replica unchanged: the binding has the header's fields in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} spo_update_ex_replica;", header, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert [n for n, _ in _abi.UpdateExReplica._fields_] == names, names


# ------------------------------------------------------------------------------------------------ the support rule
OBS_DIMS = sorted({0, 1, 513} | {64 * k + d for k in range(0, 9) for d in (-1, 0, 1) if 1 <= 64 * k + d <= 513})


def test_support_rule(lib):
    f = lib.spo_update_ks_multi_supported
    assert _cap(64) == _cap(256) == 16 and _cap(257) == _cap(376) == _cap(512) == 8 and _cap(129) == 16
    for D in OBS_DIMS:
        for A in (1, 32, 33):
            for B in (1, 64, 65):
                single = 1 <= D <= 512 and 1 <= A <= 32 and 1 <= B <= 64
                assert lib.spo_ks_supported(D, A, B) == int(single), (D, A, B)
                for n in range(0, 18):
                    assert f(D, A, B, n) == int(single and 1 <= n <= _cap(D)), (D, A, B, n)
    assert f(376, 17, 64, 8) == 1 and f(376, 17, 64, 9) == 0 and f(192, 8, 64, 16) == 1 and f(192, 8, 64, 17) == 0
    assert f(376, 0, 64, 1) == 0 and f(376, 17, 0, 1) == 0 and f(-5, 17, 64, 1) == 0


# ------------------------------------------------------------------------------------------------ block mapping
def _walk(lib, D, n, actor_only, blocks):
    out = []
    for b in blocks:
        rep, wg = ctypes.c_int(-1), ctypes.c_int(-1)
        out.append((b, lib.spo_update_ks_multi_block_map(b, D, n, actor_only, ctypes.byref(rep), ctypes.byref(wg)), rep.value, wg.value))
    return out


@pytest.mark.parametrize("actor_only", [0, 1])
@pytest.mark.parametrize("S", range(1, 9))
def test_block_mapping(lib, S, actor_only):
    D = 64 * S - 8                                                     # (any obs_dim of the slice count)
    assert (D + 63) // 64 == S
    wgs = (1 if actor_only else 3) * S
    for n in range(1, _cap(D) + 1):
        grid = 8 * wgs * ((n + 7) // 8)
        seen, label_of, per_label = {}, {}, [0] * 8
        for b, work, rep, wg in _walk(lib, D, n, actor_only, range(grid)):
            want_rep, want_wg = 8 * ((b >> 3) // wgs) + (b & 7), (b >> 3) % wgs
            if want_rep >= n:
                assert work == 0 and (rep, wg) == (-1, -1), (S, n, b)      # blocks beyond n report no work and fill nothing
                continue
            assert work == 1 and (rep, wg) == (want_rep, want_wg), (S, n, b, rep, wg)
            assert 0 <= rep < n and 0 <= wg < wgs
            assert (rep, wg) not in seen, (S, n, b, seen[(rep, wg)])
            seen[(rep, wg)] = b
            assert label_of.setdefault(rep, b & 7) == (b & 7)              # a run's blocks share one label (an XCD)
            per_label[b & 7] += 1
        assert len(seen) == wgs * n                                        # every (run, workgroup) exactly once
        assert all(label_of[r] == r % 8 for r in range(n))                 # run r on label r mod 8
        assert max(per_label) <= 24                                        # at most 24 working blocks carry any one label
        for _b, work, _r, _w in _walk(lib, D, n, actor_only, (-1, grid, grid + 5, 8 * 24 * 2)):
            assert work == 0                                               # no work outside the grid
    for n in (0, -1, _cap(D) + 1, 17):
        assert lib.spo_update_ks_multi_block_map(0, D, n, actor_only, None, None) == 0
    assert lib.spo_update_ks_multi_block_map(0, 0, 1, actor_only, None, None) == 0
    assert lib.spo_update_ks_multi_block_map(0, 513, 1, actor_only, None, None) == 0
    assert lib.spo_update_ks_multi_block_map(0, D, 1, actor_only, None, None) == 1     # (the outputs are optional)


# ------------------------------------------------------------------------------------------------ refused tables
PTRS = ("theta", "adam_m", "adam_v", "obs", "act", "logp_old", "target_r", "target_c", "adv", "perm", "old_mean", "old_std", "losses_out",
        "sync_ws")


def _table(S, D=376, A=17, batch=64, active=1):
    from safepo import _abi
    reps = (_abi.UpdateExReplica * max(S, 1))()
    for i in range(S):
        base = 0x10000 * (i + 1)
        r = reps[i]
        for k, name in enumerate(PTRS):
            setattr(r, name, base + 256 * k)
        r.kl_bound, r.pg_coef = 0.02, 0.5
        r.cfg = _abi.PpoCfg(obs_dim=D, act_dim=A, batch=batch, beta1=0.9, beta2=0.999)
        r.active = active
    return reps


def test_host_validation_happens_before_any_device_work(lib):
    """Refused on the host (no GPU here: anything that reached HIP would fail differently, and the fake pointers are never
    touched), and an all-inactive table returns 0."""
    f = lib.spo_update_iter_ex_ks_multi
    assert f(None, 1, 128, 1, 0, None) < 0 and "null replica table" in _err(lib)
    assert f(_table(1), 0, 128, 1, 0, None) < 0 and "replicas" in _err(lib)
    assert f(_table(17, D=192), 17, 128, 1, 0, None) < 0 and "replicas" in _err(lib)
    assert f(_table(9), 9, 128, 1, 0, None) < 0 and "at most 8 runs" in _err(lib) and "obs_dim 376" in _err(lib)
    assert f(_table(2), 2, 0, 1, 0, None) < 0 and "bad sizes" in _err(lib)
    assert f(_table(2), 2, 128, 2, 0, None) < 0 and "unknown actor_loss" in _err(lib)
    assert f(_table(2, D=513), 2, 128, 1, 0, None) < 0 and "obs_dim 513" in _err(lib)
    assert f(_table(2, A=33), 2, 128, 0, 0, None) < 0 and "act_dim 33" in _err(lib)
    assert f(_table(2, batch=65), 2, 128, 1, 0, None) < 0 and "batch 65" in _err(lib)
    assert f(_table(2), 2, 64 << 30, 1, 0, None) < 0 and "too many minibatch steps" in _err(lib)
    t = _table(3)
    t[2].cfg.act_dim = 4
    assert f(t, 3, 128, 1, 0, None) < 0 and "replica 2" in _err(lib)
    t = _table(3)
    t[1].cfg.batch = 32
    assert f(t, 3, 128, 0, 0, None) < 0 and "replica 1" in _err(lib)
    for shared in ("theta", "sync_ws"):
        t = _table(3)
        setattr(t[2], shared, getattr(t[0], shared))
        assert f(t, 3, 128, 1, 0, None) < 0 and "replicas 0 and 2 share" in _err(lib)
    for name in ("theta", "adam_m", "adam_v", "obs", "act", "logp_old", "adv", "perm", "losses_out", "sync_ws"):
        t = _table(2)
        setattr(t[1], name, None)
        assert f(t, 2, 128, 1, 0, None) < 0 and "null pointer in replica 1" in _err(lib), name
    for name in ("old_mean", "old_std"):                      # needed by the KL-penalty loss only
        t = _table(2)
        setattr(t[0], name, None)
        assert f(t, 2, 128, 1, 0, None) < 0 and "old distribution is NULL in replica 0" in _err(lib)
    for name in ("target_r", "target_c"):                     # not needed with actor_only
        t = _table(2)
        setattr(t[1], name, None)
        assert f(t, 2, 128, 1, 0, None) < 0 and "critic targets are NULL in replica 1" in _err(lib)
    for clock in ("adam_step_critics", "adam_step_actor"):
        t = _table(2)
        setattr(t[1], clock, -1)
        assert f(t, 2, 128, 1, 0, None) < 0 and "negative adam_step" in _err(lib)
    # all runs inactive: nothing to do -- also with the pointers a sitting-out run may leave NULL, and what the loss does not need
    t = _table(3, active=0)
    for r in t:
        r.perm, r.losses_out = None, None
    assert f(t, 3, 128, 1, 0, None) == 0
    t = _table(2, active=0)
    t[0].old_mean, t[0].old_std, t[1].target_r, t[1].target_c = None, None, None, None
    assert f(t, 2, 128, 0, 1, None) == 0
    assert lib.spo_debug_update_ks_multi_counters(None, 0) < 0


# ------------------------------------------------------------------------------------------------ the scripts' flag
def test_batch_wide_obs_flag_and_refusals(monkeypatch):
    from safepo.single_agent import _first_order, cup, focops, ppo_lag
    from safepo.utils import config
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000"])
    assert args.batch_wide_obs is False and args.batch_update is False
    called = []
    monkeypatch.setattr(_first_order, "run_seed_batch", lambda *a, **k: called.append((a, k)) or "batched")
    # without the flag: as ever (focops / cup refuse several seeds, with today's text)
    for mod in (focops, cup):
        with pytest.raises(SystemExit) as ei:
            mod.main(args, {})
        assert "--seeds with more than one seed is not available for focops and cup" in str(ei.value) and "--batch-wide-obs" not in str(ei.value)
    # focops / cup: the new flag widens --batch-update True and is refused without it -- with several seeds or one
    for argv in (["--seeds", "0", "1000"], ["--seed", "3"]):
        args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--batch-wide-obs", "True"] + argv)
        assert args.batch_wide_obs is True
        for mod in (focops, cup):
            with pytest.raises(SystemExit, match="give both"):
                mod.main(args, {})
    assert called == []
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "--batch-wide-obs", "True", "--batch-update", "True"])
    for mod, variant in ((focops, "focops"), (cup, "cup")):
        assert mod.main(args, {}) == "batched"
        a, k = called.pop()
        assert not called and variant in a[5:] + tuple(k.values()) and a[0].batch_wide_obs is True
    # the PPO family needs the one flag only
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "--batch-wide-obs", "True"])
    assert ppo_lag.main(args, {}) == "batched" and called.pop()[0][0].batch_wide_obs is True and not called


def test_too_many_seeds_are_refused_before_anything_is_built(monkeypatch, tmp_path):
    """More seeds than any shape of the feature-split launch takes: refused before an environment, a policy or a log directory."""
    from safepo.single_agent import _first_order
    built = []
    monkeypatch.setattr(_first_order, "make_sa_mujoco_env", lambda *a, **k: built.append(1))
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    a = argparse.Namespace(seed=0, seeds=[1000 * i for i in range(17)], device="cuda", device_id=0, task="SynthSafe-v0", batch_wide_obs=True,
                           log_dir=str(tmp_path / "runs"), num_envs=4, steps_per_epoch=64, total_steps=128, use_eval=False)
    with pytest.raises(SystemExit, match="at most 16 seeds"):
        _first_order.run_seed_batch(a, {}, {"hidden_sizes": [64, 64]}, "adam", 0.2, "ppo")
    assert built == [] and not os.path.exists(tmp_path / "runs")


# ------------------------------------------------------------------------------------------------ the sweep launcher
def test_benchmark_commands(capsys):
    from safepo.single_agent import benchmark
    algos = ["focops", "cup", "ppo_lag", "ppo", "pg", "cppo_pid", "cpo"]
    base = ["--workers", "0", "--tasks", "SynthSafe-v0", "SafetyHumanoidVelocity-v1", "--algo"] + algos + ["--num-seeds", "3",
                                                                                                         "--seeds-per-run", "3"]
    hum = "--task SafetyHumanoidVelocity-v1 "
    plain, klpen = benchmark.main(base), benchmark.main(base + ["--batch-focops-cup"])
    # without --batch-wide-obs: HumanoidVelocity is one subprocess per seed for every script, and no command names the flag
    # (the lists the existing launcher tests expect: tests/test_seed_batch_host.py, tests/test_seed_batch_klpen_host.py)
    for cmds in (plain, klpen):
        assert not any("--batch-wide-obs" in c for c in cmds)
        for algo in algos:
            mine = [c for c in cmds if f"{algo}.py {hum}" in c]
            assert len(mine) == 3 and not any("--seeds" in c for c in mine), algo
    wide = benchmark.main(base + ["--batch-wide-obs"])
    for algo in ("ppo_lag", "ppo", "pg", "cppo_pid"):                       # grouped, the one flag appended
        mine = [c for c in wide if f"{algo}.py {hum}" in c]
        assert len(mine) == 1 and "--seed 0 --seeds 0 1000 2000 --batch-wide-obs True --write-terminal False" in mine[0], mine
    for algo in ("focops", "cup", "cpo"):                                   # focops / cup need --batch-focops-cup as well
        mine = [c for c in wide if f"{algo}.py {hum}" in c]
        assert len(mine) == 3 and not any("--seeds" in c or "--batch-wide-obs" in c for c in mine), algo
    # every other command is the one of the list without the flag, in the same order
    assert [c for c in wide if hum not in c] == [c for c in plain if hum not in c]
    both = benchmark.main(base + ["--batch-wide-obs", "--batch-focops-cup"])
    for algo in ("focops", "cup"):
        mine = [c for c in both if f"{algo}.py {hum}" in c]
        assert len(mine) == 1 and "--seeds 0 1000 2000 --batch-update True --batch-wide-obs True --write-terminal False" in mine[0], mine
    assert len([c for c in both if f"cpo.py {hum}" in c]) == 3
    assert [c for c in both if hum not in c] == [c for c in klpen if hum not in c]
    # groups of at most 8 seeds: K = 12 is chunked into 8 + 4
    big = benchmark.main(["--workers", "0", "--tasks", "SafetyHumanoidVelocity-v1", "--algo", "ppo_lag", "focops", "--num-seeds", "12",
                          "--seeds-per-run", "12", "--batch-wide-obs", "--batch-focops-cup"])
    s8, s4 = " ".join(str(1000 * i) for i in range(8)), " ".join(str(1000 * i) for i in range(8, 12))
    for algo, extra in (("ppo_lag", ""), ("focops", " --batch-update True")):
        mine = [c for c in big if f"{algo}.py {hum}" in c]
        assert len(mine) == 2, mine
        assert f"--seed 0 --seeds {s8}{extra} --batch-wide-obs True " in mine[0] and f"--seed 8000 --seeds {s4}{extra} --batch-wide-obs True " in mine[1]
    # one seed per run: the flag changes nothing
    assert benchmark.main(base[:-2] + ["--batch-wide-obs", "--batch-focops-cup"]) == benchmark.main(base[:-2])
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------ the group's admission rule
def test_group_refuses_mixed_and_other_wide_engines(monkeypatch):
    """Admission needs no device: a group is all PPOLagEngines, or all WidePPOLagEngines on the feature-split kernel."""
    from safepo import _abi
    from safepo.common import engine
    from safepo.common.engine_group import PPOLagEngineGroup

    class _Comm:
        world_size = 1

    def fake(cls, ok=True, D=376, world=1):
        e = object.__new__(cls)
        e.D, e.A, e.M, e.dev, e.comm = D, 17, 128, torch.device("cpu"), _Comm()
        e.comm.world_size = world
        e._cfg_struct = lambda: _abi.PpoCfg(obs_dim=D, act_dim=17, batch=64)
        e._feature_split_kernel_ok = lambda cfg: ok
        return e

    W, Pe = engine.WidePPOLagEngine, engine.PPOLagEngine
    g = PPOLagEngineGroup([fake(W), fake(W)])
    assert g._ks and g.batched() and g.batched_ex(0) and g.batched_ex(1)
    with pytest.raises(_abi.SpoError, match="outside the feature-split kernel"):
        PPOLagEngineGroup([fake(W), fake(W, ok=False)])
    with pytest.raises(_abi.SpoError, match="WidePPOLagEngine"):               # mixed: refused as ever
        PPOLagEngineGroup([fake(Pe), fake(W)])
    with pytest.raises(_abi.SpoError, match="world size 1"):
        PPOLagEngineGroup([fake(W), fake(W, world=2)])
    with pytest.raises(_abi.SpoError, match="engine 1 has obs"):
        PPOLagEngineGroup([fake(W), fake(W, D=192)])
    # more runs than the launch takes at this shape, or unequal minibatch sizes: stepped engine by engine
    assert not PPOLagEngineGroup([fake(W) for _ in range(9)]).batched()
    g = PPOLagEngineGroup([fake(W), fake(W)])
    g.engines[1]._cfg_struct = lambda: _abi.PpoCfg(obs_dim=376, act_dim=17, batch=32)
    assert not g.batched() and not g.batched_ex(1)
