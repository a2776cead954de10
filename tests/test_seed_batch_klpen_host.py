"""CPU tests (no GPU) of the seed-batched FOCOPS / CUP path (spo_update_iter_ex_multi, csrc/update.hip; PPOLagEngineGroup's
update_focops / update_cup): the entry points are declared, exported and bound and the replica struct has the header's size; the
launch's block -> (run, workgroup) mapping (the function the kernel itself uses); the support and routing queries; refused tables;
--batch-update and the sweep launcher's --batch-focops-cup; the group's loops on recording stand-in engines against the engine's
own update_focops / update_cup."""
import argparse
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("spo_update_iter_ex_multi", "spo_update_ex_multi_supported", "spo_update_ex_multi_matches_single",
               "spo_update_ex_multi_block_map", "spo_debug_update_ex_multi_counters")


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


# ------------------------------------------------------------------------------------------------ symbols, the struct
def test_symbols_declared_exported_and_bound(lib):
    from safepo import _abi
    header = open(os.path.join(ROOT, "include", "safepo_hip.h")).read()
    assert "SPO_UPDATE_EX_MAX_REPLICAS 32" in header and _abi.UPDATE_EX_MAX_REPLICAS == 32
    assert "#define SPO_ABI_VERSION 2" in header and lib.spo_abi_version() == 2
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name
    # the struct's binding has the header's fields in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} spo_update_ex_replica;", header, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert [n for n, _ in _abi.UpdateExReplica._fields_] == names, names


def test_struct_size_against_the_header(tmp_path):
    """sizeof(spo_update_ex_replica) as the host compiler lays the header's struct out == ctypes' size of the binding."""
    from safepo import _abi
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "safepo_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(spo_update_ex_replica), offsetof(spo_update_ex_replica, kl_bound),\n'
                   '                        offsetof(spo_update_ex_replica, cfg), offsetof(spo_update_ex_replica, active)); return 0; }\n')
    exe = tmp_path / "size"
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if subprocess.run(
        ["sh", "-c", f"command -v {c}"], capture_output=True).returncode == 0), None)
    assert cc is not None, "no C compiler for the header"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    R = _abi.UpdateExReplica
    assert got == [ctypes.sizeof(R), R.kl_bound.offset, R.cfg.offset, R.active.offset], got


# ------------------------------------------------------------------------------------------------ block mapping
def _walk(lib, S, actor_only, blocks):
    out = []
    for b in blocks:
        rep, wg = ctypes.c_int(-1), ctypes.c_int(-1)
        out.append((b, lib.spo_update_ex_multi_block_map(b, S, actor_only, ctypes.byref(rep), ctypes.byref(wg)), rep.value, wg.value))
    return out


@pytest.mark.parametrize("actor_only", [0, 1])
@pytest.mark.parametrize("S", range(1, 33))
def test_block_mapping(lib, S, actor_only):
    wgs = 1 if actor_only else 3
    grid = 8 * wgs * ((S + 7) // 8)
    seen, label_of, per_label = {}, {}, [0] * 8
    for b, work, rep, wg in _walk(lib, S, actor_only, range(grid)):
        want_rep, want_wg = 8 * ((b >> 3) // wgs) + (b & 7), (b >> 3) % wgs
        if want_rep >= S:
            assert work == 0 and (rep, wg) == (-1, -1), (S, b)     # blocks beyond S report no work and fill nothing
            continue
        assert work == 1 and (rep, wg) == (want_rep, want_wg), (S, b, rep, wg)
        assert 0 <= rep < S and 0 <= wg < wgs
        assert (rep, wg) not in seen, (S, b, seen[(rep, wg)])
        seen[(rep, wg)] = b
        assert label_of.setdefault(rep, b & 7) == (b & 7)          # the blocks of a run share a label (an XCD)
        per_label[b & 7] += 1
    assert len(seen) == wgs * S                                    # every (run, workgroup) exactly once
    assert max(per_label) <= wgs * ((S + 7) // 8) <= 12            # at most 12 working blocks per XCD
    assert all(label_of[r] == (r & 7) for r in range(S))           # run r on label r mod 8: runs r, r + 8, ... share one
    for _b, work, _r, _w in _walk(lib, S, actor_only, (-1, grid, grid + 5, 8 * 3 * 4)):
        assert work == 0                                           # no work outside the grid
    assert lib.spo_update_ex_multi_block_map(0, 0, actor_only, None, None) == 0
    assert lib.spo_update_ex_multi_block_map(0, 33, actor_only, None, None) == 0


# ------------------------------------------------------------------------------------------------ support and routing
def test_support_truth_table(lib):
    f = lib.spo_update_ex_multi_supported
    for D in (0, 1, 16, 17, 64, 65, 128, 129):
        for A in (0, 1, 16, 17):
            for B in (0, 1, 20, 64, 65, 128):
                for loss in (0, 1, 2, -1):
                    single = 1 <= D <= 128 and 1 <= A <= 16 and B >= 1 and (loss == 0 or (loss == 1 and B <= 64))
                    for S in (0, 1, 8, 32, 33):
                        assert f(D, A, B, loss, S) == int(single and 1 <= S <= 32), (D, A, B, loss, S)


def test_routing_query_follows_the_single_launch(lib):
    """spo_update_ex_multi_matches_single: the KL-penalty loss always runs the four-wave kernel; the clipped surrogate only
    where the main + helper kernel does not take the stand-alone launch (SPO_UPDATE_FORM is read once per process: the table
    follows the value this process has)."""
    g = lib.spo_update_ex_multi_matches_single
    form = int(os.environ.get("SPO_UPDATE_FORM", "3"))
    for D in (0, 1, 16, 17, 60, 64, 65, 72, 128, 129):
        for A in (0, 1, 8, 16, 17):
            for B in (0, 1, 20, 64, 65, 128):
                for loss in (0, 1):
                    sup = lib.spo_update_ex_multi_supported(D, A, B, loss, 1)
                    want = sup and (loss == 1 or D > 64 or B > 64 or form < 2)
                    assert g(D, A, B, loss) == int(bool(want)), (D, A, B, loss, form)
    assert g(60, 8, 64, 2) == 0


def test_routing_query_under_the_four_wave_form():
    """In a process with SPO_UPDATE_FORM=0 every supported clipped-surrogate shape matches too."""
    code = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as g; from safepo import _abi; lib = _abi.load(g.LIB); "
            "print(lib.spo_update_ex_multi_matches_single(60, 8, 64, 0), lib.spo_update_ex_multi_matches_single(60, 8, 64, 1), "
            "lib.spo_update_ex_multi_matches_single(129, 8, 64, 0))" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SPO_UPDATE_FORM="0"), check=True, capture_output=True, text=True)
    assert out.stdout.split() == ["1", "1", "0"], out.stdout


# ------------------------------------------------------------------------------------------------ refused tables
PTRS = ("theta", "adam_m", "adam_v", "obs", "act", "logp_old", "target_r", "target_c", "adv", "perm", "old_mean", "old_std", "losses_out",
        "sync_ws")


def _table(S, D=60, A=8, batch=64, active=1):
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
    touched), and an all-inactive table returns 0; the counters stay at zero throughout."""
    f = lib.spo_update_iter_ex_multi
    c2 = (ctypes.c_ulonglong * 2)()
    assert lib.spo_debug_update_ex_multi_counters(c2, 1) == 0
    assert f(None, 1, 128, 1, 0, None) < 0 and "null replica table" in _err(lib)
    assert f(_table(1), 0, 128, 1, 0, None) < 0 and "replicas" in _err(lib)
    assert f(_table(33), 33, 128, 1, 0, None) < 0 and "replicas" in _err(lib)
    assert f(_table(2), 2, 0, 1, 0, None) < 0 and "bad sizes" in _err(lib)
    assert f(_table(2), 2, 128, 2, 0, None) < 0 and "unknown actor_loss" in _err(lib)
    assert f(_table(2, D=129), 2, 128, 1, 0, None) < 0 and "obs_dim" in _err(lib)
    assert f(_table(2, A=17), 2, 128, 0, 0, None) < 0 and "act_dim" in _err(lib)
    assert f(_table(2, batch=65), 2, 128, 1, 0, None) < 0 and "batch_size 65 > 64" in _err(lib)
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
    # the old distribution: needed by the KL-penalty loss only; the targets: not with actor_only
    for name in ("old_mean", "old_std"):
        t = _table(2)
        setattr(t[0], name, None)
        assert f(t, 2, 128, 1, 0, None) < 0 and "old distribution is NULL in replica 0" in _err(lib)
    for name in ("target_r", "target_c"):
        t = _table(2)
        setattr(t[1], name, None)
        assert f(t, 2, 128, 1, 0, None) < 0 and "critic targets are NULL in replica 1" in _err(lib)
    t = _table(2)
    t[1].adam_step_actor = -1
    assert f(t, 2, 128, 1, 0, None) < 0 and "negative adam_step" in _err(lib)
    # all runs inactive: nothing to do -- also with the pointers a sitting-out run may leave NULL, and what the loss does not need
    t = _table(3, active=0)
    for r in t:
        r.perm, r.losses_out = None, None
    assert f(t, 3, 128, 1, 0, None) == 0
    t = _table(2, active=0)
    t[0].old_mean, t[0].old_std, t[1].target_r, t[1].target_c = None, None, None, None
    assert f(t, 2, 128, 0, 1, None) == 0
    assert lib.spo_debug_update_ex_multi_counters(c2, 0) == 0 and list(c2) == [0, 0]
    assert lib.spo_debug_update_ex_multi_counters(None, 0) < 0


# ------------------------------------------------------------------------------------------------ flags, launcher
def test_batch_update_flag_and_refusal(monkeypatch):
    from safepo.single_agent import _first_order, cup, focops
    from safepo.utils import config
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "2000"])
    assert args.batch_update is False
    called = []
    monkeypatch.setattr(_first_order, "run_seed_batch", lambda *a, **k: called.append((a, k)) or "batched")
    for mod in (focops, cup):
        with pytest.raises(SystemExit) as ei:
            mod.main(args, {})
        msg = str(ei.value)
        # today's message, then the hint
        assert "--seeds with more than one seed is not available for focops and cup: the seed-batched update exists for the" in msg
        assert "run one process per seed" in msg and msg.rstrip().endswith("launch.)") and "--batch-update True" in msg
    assert called == []
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "2000", "--batch-update", "True"])
    assert args.batch_update is True
    for mod, variant in ((focops, "focops"), (cup, "cup")):
        assert mod.main(args, {}) == "batched"
        a, k = called.pop()
        assert not called and variant in a[5:] + tuple(k.values()), (a, k)
    # one seed: the ordinary run, whatever the flag says (run() goes on past the seed-batch branch to the device check)
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "7", "--batch-update", "True", "--device", "cpu"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        focops.main(args, {})
    assert called == [] and args.seed == 7


def test_seed_batch_refusals_hold_for_focops_and_cup(monkeypatch):
    """run_seed_batch's own refusals do not depend on the variant: torchrun, a seed twice, the CPU."""
    from safepo.single_agent import _first_order
    a = argparse.Namespace(seed=0, seeds=[0, 1], device="cuda", device_id=0, task="SynthSafe-v0", batch_update=True)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="torchrun"):
        _first_order.run_seed_batch(a, {}, {}, "adam", 0.2, "focops")
    monkeypatch.delenv("WORLD_SIZE")
    a.seeds = [3, 3]
    with pytest.raises(SystemExit, match="same seed twice"):
        _first_order.run_seed_batch(a, {}, {}, "adam", 0.2, "cup")
    a.seeds, a.device = [0, 1], "cpu"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _first_order.run_seed_batch(a, {}, {}, "adam", 0.2, "cup")


def test_benchmark_commands(capsys):
    from safepo.single_agent import benchmark
    base = ["--workers", "0", "--tasks", "SynthSafe-v0", "SafetyHumanoidVelocity-v1", "--algo", "focops", "cup", "ppo_lag", "--num-seeds", "3",
            "--seeds-per-run", "3"]
    plain = benchmark.main(base)
    # without the flag: focops / cup keep one command per seed, none carries --batch-update
    assert not any("--batch-update" in c for c in plain)
    for algo in ("focops", "cup"):
        for task in ("SynthSafe-v0", "SafetyHumanoidVelocity-v1"):
            mine = [c for c in plain if f"{algo}.py --task {task} " in c]
            assert len(mine) == 3 and not any("--seeds" in c for c in mine)
    on = benchmark.main(base + ["--batch-focops-cup"])
    for algo in ("focops", "cup"):
        mine = [c for c in on if f"{algo}.py --task SynthSafe-v0 " in c]
        assert len(mine) == 1 and "--seed 0 --seeds 0 1000 2000 --batch-update True --write-terminal False" in mine[0]
        hum = [c for c in on if f"{algo}.py --task SafetyHumanoidVelocity-v1 " in c]         # HumanoidVelocity excepted
        assert len(hum) == 3 and not any("--seeds" in c or "--batch-update" in c for c in hum)
    # ppo_lag is grouped either way and never carries the flag
    for cmds in (plain, on):
        lag = [c for c in cmds if "ppo_lag.py --task SynthSafe-v0 " in c]
        assert len(lag) == 1 and "--seeds 0 1000 2000" in lag[0] and "--batch-update" not in lag[0]
    assert len(plain) == 2 * 3 * 2 + 1 + 3 and len(on) == 2 * 1 + 2 * 3 + 1 + 3
    # one seed per run: the flag changes nothing
    assert benchmark.main(base[:-2] + ["--batch-focops-cup"]) == benchmark.main(base[:-2])
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------ the group's loops
class _StubBuffer:
    def __init__(self, log):
        self.log, self.adv_mix, self.data = log, "adv_mix", {"adv_c": "adv_c"}

    def compute_gae(self, lam, comm):
        self.log.append(("gae", lam))

    def reset(self):
        self.log.append(("reset",))


class _StubComm:
    world_size = 1


class _StubEngine:
    """Records what the update asks of an engine; the KL after every pass comes from a script (first stage, then second)."""
    D, A, M, dev = 4, 2, 12, torch.device("cpu")

    def __init__(self, kls, learning_iters, target_kl):
        self.log, self.kls = [], list(kls)
        self.cfg = {"learning_iters": learning_iters, "target_kl": target_kl, "gamma": 0.99}
        self.comm, self.buffer = _StubComm(), _StubBuffer(self.log)

    def snapshot_old_distribution(self):
        self.log.append(("snapshot",))

    def learning_iter_ex(self, perm, adv, actor_loss=0, kl_bound=float("inf"), pg_coef=0.0, actor_only=False):
        self.log.append(("iter_ex", perm, adv, actor_loss, kl_bound, pg_coef, actor_only))
        return torch.full((2, 3), float(len(self.log)))

    def kl_launch(self):
        self.log.append(("kl_launch",))

    def kl_read(self):
        self.log.append(("kl_read",))
        return self.kls.pop(0)

    def kl_to_old(self):
        self.kl_launch()
        return self.kl_read()

    def check_sync_error(self):
        self.log.append(("check",))

    def perm_fn(self, it):
        self.log.append(("perm", it))
        return ("perm", it)


def _bind(e):
    """The engine's own loop and updates on a stand-in."""
    from safepo.common.engine import PPOLagEngine
    e._kl_stopped_loop = lambda *a: PPOLagEngine._kl_stopped_loop(e, *a)
    return e


def _record_actives(group):
    seen, inner = [], group.learning_iter_ex_all

    def recording(perms, advs, actor_loss=0, kl_bounds=None, pg_coefs=None, actor_only=False, active=None):
        seen.append((actor_loss, bool(actor_only), list(active)))
        return inner(perms, advs, actor_loss, kl_bounds, pg_coefs, actor_only, active)

    group.learning_iter_ex_all = recording
    return seen


FOCOPS_SCRIPTS = [([0.9], 4, 1), ([0.1, 0.9], 4, 2), ([0.1, 0.2, 0.3, 0.4], 4, 4), ([0.1, 0.1], 2, 2)]   # (KLs, learning_iters, passes)


def test_group_focops_loop_with_stub_engines():
    from safepo.common.engine import PPOLagEngine
    from safepo.common.engine_group import PPOLagEngineGroup
    lams = [0.25 * i for i in range(4)]
    alone = [_bind(_StubEngine(kls, n, 0.5)) for kls, n, _ in FOCOPS_SCRIPTS]
    alone_out = [PPOLagEngine.update_focops(e, lams[i], e.perm_fn, focops_lam=1.5) for i, e in enumerate(alone)]
    assert [o["stop_iter"] for o in alone_out] == [p for _, _, p in FOCOPS_SCRIPTS]
    es = [_StubEngine(kls, n, 0.5) for kls, n, _ in FOCOPS_SCRIPTS]
    group = PPOLagEngineGroup(es)
    assert not group.batched_ex(1)                                   # (stand-ins are stepped one by one)
    seen = _record_actives(group)
    outs = group.update_focops(lams, [e.perm_fn for e in es], focops_lam=1.5)
    # one launch per pass; a run that stopped -- by its KL or by its learning_iters -- sits out the later ones
    assert seen == [(1, False, a) for a in ([True] * 4, [False, True, True, True], [False, False, True, False], [False, False, True, False])]
    for e, a, (_, _, p) in zip(es, alone, FOCOPS_SCRIPTS):
        assert sum(1 for x in e.log if x[0] == "iter_ex") == p
        # per run the same calls with the same arguments in the same order: a pass's shuffle is drawn at the start of that pass,
        # none after the stop
        assert e.log == a.log
        assert [x[1] for x in e.log if x[0] == "perm"] == list(range(p))
    for o, ao in zip(outs, alone_out):
        assert set(o) == set(ao) and o["stop_iter"] == ao["stop_iter"] and o["kl"] == ao["kl"]
        assert (o["loss_r"], o["loss_c"], o["loss_pi"]) == (ao["loss_r"], ao["loss_c"], ao["loss_pi"])
        assert len(o["losses"]) == len(ao["losses"]) and all(torch.equal(x, y) for x, y in zip(o["losses"], ao["losses"]))


# (first-stage KLs + second-stage KLs, learning_iters, first-stage passes, second-stage passes)
CUP_SCRIPTS = [([0.9] + [0.1, 0.1, 0.9], 4, 1, 3), ([0.1, 0.9] + [0.9], 4, 2, 1), ([0.1, 0.2, 0.3, 0.4] + [0.1, 0.2, 0.3, 0.4], 4, 4, 4),
               ([0.1, 0.1] + [0.1, 0.9], 2, 2, 2)]


def test_group_cup_loop_with_stub_engines():
    from safepo.common.engine import PPOLagEngine
    from safepo.common.engine_group import PPOLagEngineGroup
    lams = [0.1 + 0.25 * i for i in range(4)]
    alone = [_bind(_StubEngine(kls, n, 0.5)) for kls, n, _, _ in CUP_SCRIPTS]
    alone_out = [PPOLagEngine.update_cup(e, lams[i], e.perm_fn, cup_lambda=0.95) for i, e in enumerate(alone)]
    assert [(o["stop_iter"], o["second_stage_stop_iter"]) for o in alone_out] == [(a, b) for _, _, a, b in CUP_SCRIPTS]
    es = [_StubEngine(kls, n, 0.5) for kls, n, _, _ in CUP_SCRIPTS]
    group = PPOLagEngineGroup(es)
    seen = _record_actives(group)
    outs = group.update_cup(lams, [e.perm_fn for e in es], cup_lambda=0.95)
    T, F = True, False
    assert seen == [(0, False, a) for a in ([T, T, T, T], [F, T, T, T], [F, F, T, F], [F, F, T, F])] + \
                   [(1, True, a) for a in ([T, T, T, T], [T, F, T, T], [T, F, T, F], [F, F, T, F])]
    for e, a, (_, _, p1, p2) in zip(es, alone, CUP_SCRIPTS):
        assert e.log == a.log
        # run i's second-stage shuffle index goes on from its own first-stage stop_iter
        assert [x[1] for x in e.log if x[0] == "perm"] == list(range(p1)) + list(range(p1, p1 + p2))
        assert [x[0] for x in e.log].count("snapshot") == 2 and e.log[-2:] == [("check",), ("reset",)]
    for o, ao in zip(outs, alone_out):
        assert set(o) == set(ao)
        for k in ("stop_iter", "second_stage_stop_iter", "kl", "kl_first_stage", "loss_r", "loss_c", "loss_pi"):
            assert o[k] == ao[k], k
        for k in ("losses", "second_stage_losses"):
            assert len(o[k]) == len(ao[k]) and all(torch.equal(x, y) for x, y in zip(o[k], ao[k]))


def test_learning_iter_ex_all_argument_checks():
    from safepo.common.engine_group import PPOLagEngineGroup
    es = [_StubEngine([], 1, 0.5) for _ in range(2)]
    group = PPOLagEngineGroup(es)
    with pytest.raises(ValueError, match="one perm"):
        group.learning_iter_ex_all(["p"], ["a", "b"])
    with pytest.raises(ValueError, match="one multiplier"):
        group.update_focops([0.0])
    with pytest.raises(ValueError, match="one multiplier"):
        group.update_cup([0.0, 0.0, 0.0])
    out = group.learning_iter_ex_all(["p0", "p1"], ["a0", "a1"], 1, [0.02, 0.03], [0.5, 0.6], False, [False, True])
    assert out[0] is None and es[0].log == [] and es[1].log == [("iter_ex", "p1", "a1", 1, 0.03, 0.6, False)]
