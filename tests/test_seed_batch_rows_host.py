"""CPU tests (no GPU) of the seed-batched row-group step (spo_wide_rows_multi_upload / spo_wide_rows_step_multi, csrc/mlp_rows.hip;
PPOLagEngineGroup of WidePPOLagEngines on the row-group kernel; --hidden-sizes, --batch-wide-rows): the entry points are declared,
exported and bound; the support rule against a Python restatement; malformed tables refused on the host, with their texts and
their order; the scripts' new flags and refusals; the sweep launcher's command lists; the group's admission rule."""
import argparse
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("spo_wide_rows_multi_supported", "spo_wide_rows_multi_table_bytes", "spo_wide_rows_multi_upload",
               "spo_wide_rows_step_multi")


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
    assert "#define SPO_WIDE_ROWS_MAX_REPLICAS 32" in header and _abi.WIDE_ROWS_MAX_REPLICAS == 32
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name][1]
    c_int, c_int64, P, N = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(_abi.MlpNet)
    assert _abi.PROTOTYPES["spo_wide_rows_multi_supported"] == (c_int, [N, N, c_int64, c_int])
    assert _abi.PROTOTYPES["spo_wide_rows_multi_table_bytes"] == (c_int64, [c_int])
    assert _abi.PROTOTYPES["spo_wide_rows_multi_upload"] == (c_int, [P, ctypes.POINTER(_abi.WideRowsReplica), c_int, N, N, c_int64, c_int64, P])
    assert _abi.PROTOTYPES["spo_wide_rows_step_multi"] == (c_int, [P, c_int, N, N, c_int64, P])
    # the binding has the header's fields in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} spo_wide_rows_replica;", header, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert [n for n, _ in _abi.WideRowsReplica._fields_] == names, names
    assert lib.spo_wide_rows_multi_table_bytes(0) == -1 and lib.spo_wide_rows_multi_table_bytes(33) == -1
    one = lib.spo_wide_rows_multi_table_bytes(1)
    assert one > 0 and lib.spo_wide_rows_multi_table_bytes(32) == 32 * one


# ------------------------------------------------------------------------------------------------ the support rule
def _up16(v):
    return (v + 15) & ~15


def _lds_floats(dims, A):
    """csrc/mlp_rows.hip's LDS map of a 16-row group, restated: per level a row image [16][w + 4] and (below the output) a
    transposed one [w][20], two dZ row images and two transposed ones at the widest layer output, the per-row scalars."""
    n = len(dims) - 1
    off = 0
    for u in range(n + 1):
        off += 16 * (_up16(dims[u]) + 4)
        if u < n:
            off += _up16(dims[u]) * 20
    pz = max([16] + [_up16(d) for d in dims[1:]])
    ap = 4 if A < 1 else (A + 3) & ~3
    return off + 2 * 16 * (pz + 4) + 2 * pz * 20 + 112 + 2 * ap + 32 * ap


def _supported(D, A, hidden, rows, n):
    return (1 <= rows <= 256 and 1 <= len(hidden) + 1 <= 5 and 1 <= A <= 64 and 1 <= n <= 32
            and all(4 * _lds_floats([D] + hidden + [out], A) <= 160 * 1024 for out in (1, A)))


def test_support_rule(lib):
    from safepo import _abi
    f = lib.spo_wide_rows_multi_supported
    too_big = 0
    for D in (7, 60, 600):
        for A in (1, 8, 17, 64, 65):
            for width in (20, 64, 128, 256, 384):
                for depth in (1, 2, 3, 4):
                    hidden = [width] * depth
                    nc, na = _abi.MlpNet.of([D] + hidden + [1]), _abi.MlpNet.of([D] + hidden + [A])
                    over = 4 * _lds_floats([D] + hidden + [A], A) > 160 * 1024
                    too_big += over
                    for rows in (0, 1, 20, 64, 256, 257):
                        single = lib.spo_wide_grad_rows_supported(nc, na, rows)
                        assert single == int(_supported(D, A, hidden, rows, 1)), (D, A, hidden, rows)
                        for n in (0, 1, 9, 32, 33):
                            assert f(nc, na, rows, n) == int(_supported(D, A, hidden, rows, n)), (D, A, hidden, rows, n)
                            assert f(nc, na, rows, n) == int(bool(single) and 1 <= n <= 32)
    assert too_big > 0                                                    # the grid holds shapes beyond one CU's 160 KB
    nc, na = _abi.MlpNet.of([60, 256, 256, 1]), _abi.MlpNet.of([60, 256, 256, 8])
    assert 4 * _lds_floats([60, 256, 256, 8], 8) <= 160 * 1024 and f(nc, na, 64, 32) == 1        # (157.4 KB: fits)
    nc, na = _abi.MlpNet.of([300, 256, 256, 1]), _abi.MlpNet.of([300, 256, 256, 8])
    assert 4 * _lds_floats([300, 256, 256, 8], 8) > 160 * 1024 and f(nc, na, 64, 1) == 0
    assert f(nc, None, 64, 1) == 0                                        # an actor is needed (the critic fit is not batched)


# ------------------------------------------------------------------------------------------------ refused tables
PTRS = ("theta", "adam_m", "adam_v", "grad", "parts", "obs", "act", "logp_old", "target_r", "target_c", "adv", "perm", "cursor_dev",
        "pow4_dev", "losses3_out", "scalars4_out", "partial_ws", "loss_log_dev")
NETS = ([60, 128, 128, 1], [60, 128, 128, 8])


def _table(S, active=1, capacity=3 * 1024):
    from safepo import _abi
    reps = (_abi.WideRowsReplica * max(S, 1))()
    for i in range(S):
        r = reps[i]
        for k, name in enumerate(PTRS):
            setattr(r, name, 0x100000 * (i + 1) + 4096 * k)
        r.partial_capacity = capacity
        r.cfg = _abi.PpoCfg(obs_dim=60, act_dim=8, batch=64, clip=0.2, max_grad_norm=40.0, beta1=0.9, beta2=0.999, adam_eps=1e-8)
        r.active = active
    return reps


def test_upload_refusals_come_before_any_device_work_in_order(lib):
    """No GPU here: a call that reached HIP would fail differently, and the fake pointers are never touched."""
    from safepo import _abi
    f = lib.spo_wide_rows_multi_upload
    nc, na = (_abi.MlpNet.of(d) for d in NETS)
    TAB = 0x7000000
    assert f(None, _table(2), 2, nc, na, 64, 64, None) < 0 and _err(lib) == "wide_rows_multi_upload: null table"
    assert f(TAB, None, 2, nc, na, 64, 64, None) < 0 and _err(lib) == "wide_rows_multi_upload: null table"
    for n in (0, -1, 33):
        assert f(TAB, _table(2), n, nc, na, 64, 64, None) < 0 and _err(lib) == f"wide_rows_multi_upload: n_replicas {n} outside [1,32]"
    assert f(None, _table(2), 0, nc, na, 64, 64, None) < 0 and "null table" in _err(lib)                 # (the table first)
    for rows in (0, 257):
        assert f(TAB, _table(2), 2, nc, na, rows, 64, None) < 0 and "wide_rows_multi_upload: shape outside the row-group kernel" in _err(lib)
    assert f(TAB, _table(2), 2, nc, None, 64, 64, None) < 0 and "shape outside the row-group kernel" in _err(lib)
    big_c, big_a = _abi.MlpNet.of([300, 256, 256, 1]), _abi.MlpNet.of([300, 256, 256, 8])
    assert f(TAB, _table(2), 2, big_c, big_a, 64, 64, None) < 0 and "shape outside the row-group kernel" in _err(lib)
    for name in PTRS:
        t = _table(3)
        setattr(t[1], name, None)
        rc = f(TAB, t, 3, nc, na, 64, 0, None)                                    # (cursor_step bad too: the later refusal)
        if name == "loss_log_dev":                                                # optional, as in the stand-alone entry
            assert rc < 0 and _err(lib) == "wide_rows_multi_upload: cursor_step must be > 0"
        else:
            assert rc < 0 and _err(lib) == "wide_rows_multi_upload: replica 1: null pointer", name
    for shared in ("theta", "parts", "cursor_dev"):
        t = _table(3, capacity=1)                                                 # (workspace too small as well: the later refusal)
        setattr(t[2], shared, getattr(t[0], shared))
        assert f(TAB, t, 3, nc, na, 64, 64, None) < 0 and _err(lib) == f"wide_rows_multi_upload: replicas 0 and 2 share {shared}"
    t = _table(3)
    t[0].theta = None                                                             # a null pointer is named before a shared one
    t[2].parts = t[1].parts
    assert f(TAB, t, 3, nc, na, 64, 64, None) < 0 and "replica 0: null pointer" in _err(lib)
    # 2 * 24 449 + 8 + 25 352 parameters: 291 blocks of 256 -> 873 doubles
    t = _table(2)
    t[1].partial_capacity = 872
    assert f(TAB, t, 2, nc, na, 64, 0, None) < 0 and _err(lib) == "wide_rows_multi_upload: partial workspace too small"
    t[1].partial_capacity = 873
    for step in (0, -64):
        assert f(TAB, t, 2, nc, na, 64, step, None) < 0 and _err(lib) == "wide_rows_multi_upload: cursor_step must be > 0"
    # an inactive run is not looked at: NULL pointers, a shared theta, no workspace
    t = _table(3)
    t[1].active = 0
    for name in PTRS:
        setattr(t[1], name, None)
    t[1].partial_capacity = 0
    assert f(TAB, t, 3, nc, na, 64, 0, None) < 0 and _err(lib) == "wide_rows_multi_upload: cursor_step must be > 0"
    t[1].theta = t[0].theta
    assert f(TAB, t, 3, nc, na, 64, 0, None) < 0 and _err(lib) == "wide_rows_multi_upload: cursor_step must be > 0"
    # the launch entry's own refusals
    g = lib.spo_wide_rows_step_multi
    assert g(None, 2, nc, na, 64, None) < 0 and _err(lib) == "wide_rows_step_multi: null table"
    assert g(TAB, 33, nc, na, 64, None) < 0 and _err(lib) == "wide_rows_step_multi: n_replicas 33 outside [1,32]"
    assert g(TAB, 2, nc, na, 257, None) < 0 and "wide_rows_step_multi: shape outside the row-group kernel" in _err(lib)
    # the stand-alone entry keeps its texts (the checks are shared code now)
    h = lib.spo_wide_rows_clip_adam_dev_log
    cfg = _abi.PpoCfg(obs_dim=60, act_dim=8, batch=64)
    a = [TAB, 64, TAB, TAB, TAB, TAB, 1000, 100, 200, 200, cfg, TAB, TAB, TAB, TAB, 3 * 1024, None, TAB, 64, None]
    bad = list(a); bad[7], bad[8] = 300, 200
    assert h(*bad) < 0 and _err(lib) == "wide_rows_clip_adam: parameter ranges out of order"
    bad = list(a); bad[18] = 0; bad[15] = 1
    assert h(*bad) < 0 and _err(lib) == "wide_rows_clip_adam: cursor_step must be > 0"
    bad = list(a); bad[15] = 11
    assert h(*bad) < 0 and _err(lib) == "wide_rows_clip_adam: partial workspace too small"


# ------------------------------------------------------------------------------------------------ the scripts' flags
def test_hidden_sizes_parse_and_reach_the_config():
    from safepo.utils import config
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0"])
    assert args.hidden_sizes is None and args.batch_wide_rows is False
    assert config.fold_overrides({"hidden_sizes": [64, 64], "x": 1}, args) == {"hidden_sizes": [64, 64], "x": 1}
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--hidden-sizes", "128", "96", "32", "--batch-wide-rows", "True"])
    assert args.hidden_sizes == [128, 96, 32] and args.batch_wide_rows is True
    assert config.fold_overrides({"hidden_sizes": [64, 64], "x": 1}, args) == {"hidden_sizes": [128, 96, 32], "x": 1}
    args.cfg_override = {"hidden_sizes": [256, 256], "x": 2}                    # an explicit override still wins
    assert config.fold_overrides({"hidden_sizes": [64, 64], "x": 1}, args) == {"hidden_sizes": [256, 256], "x": 2}
    # a Namespace built by hand (no such attribute) folds as ever
    assert config.fold_overrides({"hidden_sizes": [64, 64]}, argparse.Namespace(cfg_override={"y": 3})) == {"hidden_sizes": [64, 64], "y": 3}


@pytest.mark.parametrize("algo", ["ppo_lag", "ppo", "pg", "cppo_pid", "focops", "cup", "cpo", "pcpo", "rcpo", "trpo_lag", "trpo", "natural_pg"])
def test_hidden_sizes_reach_every_scripts_config(monkeypatch, algo):
    """Every script folds --hidden-sizes where it folds cfg_override: the config its run builds has the widths."""
    import importlib
    from safepo.single_agent import _first_order, _second_order, cpo
    from safepo.utils import config
    seen = []

    def spy(cfg, args):
        out = config.fold_overrides(cfg, args)
        seen.append(list(out["hidden_sizes"]))
        raise SystemExit("stop here")

    for mod in (_first_order, _second_order, cpo):
        monkeypatch.setattr(mod, "fold_overrides", spy)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    mod = importlib.import_module(f"safepo.single_agent.{algo}")
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--hidden-sizes", "128", "128"])
    with pytest.raises(SystemExit, match="stop here"):
        mod.main(args, {})
    assert seen == [[128, 128]]


def test_batch_wide_rows_flag_and_refusals(monkeypatch):
    from safepo.single_agent import _first_order, cpo, focops, ppo_lag
    from safepo.utils import config
    called = []
    monkeypatch.setattr(_first_order, "run_seed_batch", lambda *a, **k: called.append((a, k)) or "batched")
    # focops / cup and the second-order scripts refuse the flag: those forms are not built -- several seeds or one
    for argv in (["--seeds", "0", "1000"], ["--seed", "3"]):
        args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--hidden-sizes", "128", "128", "--batch-wide-rows", "True"] + argv)
        with pytest.raises(SystemExit, match="--batch-wide-rows True is not available for focops and cup.*no such form"):
            focops.main(args, {})
        with pytest.raises(SystemExit, match="--batch-wide-rows True is not available for the second-order scripts.*no such form"):
            cpo.main(args, {})
    assert called == []
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "--hidden-sizes", "128", "128",
                                        "--batch-wide-rows", "True"])
    assert ppo_lag.main(args, {}) == "batched" and called.pop()[0][0].batch_wide_rows is True and not called


def test_without_the_flag_the_refusal_is_todays(monkeypatch, tmp_path):
    """hidden_sizes [128, 128] with two seeds and no --batch-wide-rows: the refusal text of before, word for word; with the flag
    a seed count or a shape that does not fit is refused before anything is logged, naming the limit."""
    from safepo.single_agent import _first_order

    class _Space:
        shape = (60,)

    class _ASpace:
        shape = (8,)

    monkeypatch.setattr(_first_order, "make_sa_mujoco_env", lambda *a, **k: (object(), _Space(), _ASpace()))
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    from safepo.common import engine_group

    class _NoRNG:
        def __init__(self, seed, device=None):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

    monkeypatch.setattr(engine_group, "ReplicaRNG", _NoRNG)
    monkeypatch.setattr(_first_order, "ActorVCritic", lambda **k: type("P", (), {"to": lambda self, d: self, "kernels_supported": lambda self, *a: False})())

    def ns(**kw):
        a = argparse.Namespace(seed=0, seeds=[0, 1000], device="cuda", device_id=0, task="SynthSafe-v0", log_dir=str(tmp_path / "runs"),
                               num_envs=4, steps_per_epoch=1024, total_steps=2048, use_eval=False)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    cfg = {"hidden_sizes": [128, 128], "batch_size": 64}
    with pytest.raises(SystemExit) as ei:
        _first_order.run_seed_batch(ns(), {}, cfg, "adam", 0.2, "ppo")
    assert str(ei.value) == ("--seeds with more than one seed needs the persistent kernels' shapes (hidden_sizes [64, 64], obs_dim <= "
                             "128, act_dim <= 16); SynthSafe-v0 with hidden_sizes [128, 128] runs on the wide-network "
                             "kernels: one process per seed")
    with pytest.raises(SystemExit, match="at most 32 seeds share the row-group step's launches"):
        _first_order.run_seed_batch(ns(seeds=list(range(33)), batch_wide_rows=True), {}, cfg, "adam", 0.2, "ppo")
    with pytest.raises(SystemExit, match="does not fit the row-group kernel"):
        _first_order.run_seed_batch(ns(batch_wide_rows=True), {}, {"hidden_sizes": [512, 512], "batch_size": 64}, "adam", 0.2, "ppo")
    with pytest.raises(SystemExit, match="does not fit the row-group kernel"):
        _first_order.run_seed_batch(ns(batch_wide_rows=True), {}, {"hidden_sizes": [128, 128], "batch_size": 512}, "adam", 0.2, "ppo")
    with pytest.raises(SystemExit, match="not a graph-replayed pass"):
        _first_order.run_seed_batch(ns(batch_wide_rows=True, steps_per_epoch=128), {}, cfg, "adam", 0.2, "ppo")
    assert not os.path.exists(tmp_path / "runs")


# ------------------------------------------------------------------------------------------------ the sweep launcher
def test_benchmark_commands(capsys):
    from safepo.single_agent import benchmark
    algos = ["ppo_lag", "ppo", "pg", "cppo_pid", "focops", "cup", "cpo"]
    base = ["--workers", "0", "--tasks", "SynthSafe-v0", "--algo"] + algos + ["--num-seeds", "3", "--seeds-per-run", "3"]
    plain = benchmark.main(base)
    assert not any("--hidden-sizes" in c or "--batch-wide-rows" in c for c in plain)
    # --batch-wide-rows without other widths changes nothing
    assert benchmark.main(base + ["--batch-wide-rows"]) == plain
    # other widths without the flag: every command names them, one subprocess per seed for every script
    wide = benchmark.main(base + ["--hidden-sizes", "128", "128", "--batch-focops-cup", "--batch-second-order"])
    assert len(wide) == 3 * len(algos) and all("--hidden-sizes 128 128 --write-terminal" in c and "--seeds" not in c for c in wide)
    rows = benchmark.main(base + ["--hidden-sizes", "128", "128", "--batch-wide-rows"])
    for algo in ("ppo_lag", "ppo", "pg", "cppo_pid"):
        mine = [c for c in rows if f"{algo}.py " in c]
        assert len(mine) == 1 and "--seed 0 --seeds 0 1000 2000 --hidden-sizes 128 128 --batch-wide-rows True --write-terminal False" in mine[0]
    for algo in ("focops", "cup", "cpo"):
        mine = [c for c in rows if f"{algo}.py " in c]
        assert len(mine) == 3 and not any("--seeds" in c or "--batch-wide-rows" in c for c in mine)
    # --hidden-sizes 64 64 is the default shape: grouped as without it, the widths passed on
    same = benchmark.main(base + ["--hidden-sizes", "64", "64"])
    assert [c.replace(" --hidden-sizes 64 64", "") for c in same] == plain
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------ the group's admission rule
def test_group_takes_wide_engines_outside_the_feature_split_kernel(monkeypatch):
    """Admission needs no device: a group of WidePPOLagEngines none of which is on the feature-split kernel is the row-group kind;
    _rows_batched follows the engine's own conditions for the graph-replayed fused step."""
    from safepo import _abi
    from safepo.common import engine
    from safepo.common.engine_group import PPOLagEngineGroup

    class _Comm:
        def __init__(self, world):
            self.world_size = world

    class _Wide:
        net_c, net_a = _abi.MlpNet.of(NETS[0]), _abi.MlpNet.of(NETS[1])

        def __init__(self, ok):
            self.ok = ok

        def rows_grad_ok(self, rows):
            return self.ok

    class _Pol:
        def __init__(self, hs):
            self.hidden_sizes = hs

    def fake(ks=False, world=1, rows_ok=True, M=64 * 5 + 7, batch=64, hs=(128, 128), graph_max=2048):
        e = object.__new__(engine.WidePPOLagEngine)
        e.D, e.A, e.M, e.dev, e.comm = 60, 8, M, torch.device("cpu"), _Comm(world)
        e._cfg_struct = lambda: _abi.PpoCfg(obs_dim=60, act_dim=8, batch=batch)
        e._feature_split_kernel_ok = lambda cfg: ks
        e.wide, e.policy, e.graph_max_batch = _Wide(rows_ok), _Pol(list(hs)), graph_max
        return e

    g = PPOLagEngineGroup([fake(), fake(), fake()])
    assert g._rows and not g._ks and g.batched() and not g.batched_ex(0) and not g.batched_ex(1)
    assert PPOLagEngineGroup([fake() for _ in range(32)]).batched() and not PPOLagEngineGroup([fake() for _ in range(33)]).batched()
    assert not PPOLagEngineGroup([fake(), fake(rows_ok=False)]).batched()           # a shape the row-group kernel does not take
    assert not PPOLagEngineGroup([fake(M=128), fake(M=128)]).batched()              # two minibatches: not graph-replayed stand-alone
    assert not PPOLagEngineGroup([fake(graph_max=0), fake()]).batched()
    monkeypatch.setenv("SPO_WIDE_ROWS_FUSED", "0")
    assert not g.batched()
    monkeypatch.delenv("SPO_WIDE_ROWS_FUSED")
    assert g.batched()
    with pytest.raises(_abi.SpoError, match="world size 1"):
        PPOLagEngineGroup([fake(), fake(world=2)])
    with pytest.raises(_abi.SpoError, match="hidden_sizes"):
        PPOLagEngineGroup([fake(), fake(hs=(128, 64))])
    with pytest.raises(_abi.SpoError, match="outside the feature-split kernel"):    # mixed kinds: refused as ever
        PPOLagEngineGroup([fake(ks=True), fake()])
