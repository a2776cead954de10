"""CPU tests (no GPU) of the seed-batched row-group step of FOCOPS / CUP (spo_wide_rows_ex_multi_upload /
spo_wide_rows_ex_step_multi, csrc/mlp_rows.hip + csrc/wide.hip; PPOLagEngineGroup(..., klpen_rows=True); --batch-klpen-rows): the
entry points are declared, exported and bound; the table size and the support answers; malformed tables refused on the host, with
their texts and their order; the scripts' new flag and refusals; the sweep launcher's command lists; the group's admission rule."""
import argparse
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("spo_wide_rows_ex_multi_supported", "spo_wide_rows_ex_multi_table_bytes", "spo_wide_rows_ex_multi_upload",
               "spo_wide_rows_ex_step_multi")
CLIP, KLPEN = 0, 1


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
    assert "#define SPO_ABI_VERSION 2" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _abi.PROTOTYPES[name][1]
    c_int, c_int64, P, N = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(_abi.MlpNet)
    assert _abi.PROTOTYPES["spo_wide_rows_ex_multi_supported"] == (c_int, [N, N, c_int64, c_int, c_int, c_int])
    assert _abi.PROTOTYPES["spo_wide_rows_ex_multi_table_bytes"] == (c_int64, [c_int])
    assert _abi.PROTOTYPES["spo_wide_rows_ex_multi_upload"] == (c_int, [P, ctypes.POINTER(_abi.WideRowsExReplica), c_int, N, N, c_int64,
                                                                        c_int64, c_int, c_int, P])
    assert _abi.PROTOTYPES["spo_wide_rows_ex_step_multi"] == (c_int, [P, c_int, N, N, c_int64, c_int, c_int, P])
    # the binding has the header's fields in the header's order: spo_wide_rows_replica's, then the old distribution and the loss options
    body = re.search(r"typedef struct \{([^}]*)\} spo_wide_rows_ex_replica;", header, flags=re.S).group(1)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert [n for n, _ in _abi.WideRowsExReplica._fields_] == names, names
    assert names == [n for n, _ in _abi.WideRowsReplica._fields_] + ["old_mean", "old_std", "kl_bound", "pg_coef"]


# ------------------------------------------------------------------------------------------------ table size, support
NETS = ([60, 128, 128, 1], [60, 128, 128, 8])


def test_table_bytes_and_supported_answers(lib):
    from safepo import _abi
    tb, f = lib.spo_wide_rows_ex_multi_table_bytes, lib.spo_wide_rows_ex_multi_supported
    assert tb(0) == -1 and tb(33) == -1 and tb(-1) == -1
    sizes = [tb(n) for n in range(1, 33)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    nc, na = (_abi.MlpNet.of(d) for d in NETS)
    for loss, only in ((KLPEN, 0), (KLPEN, 1), (CLIP, 0)):
        assert f(nc, na, 64, loss, only, 1) == 1 and f(nc, na, 64, loss, only, 32) == 1 and f(nc, na, 256, loss, only, 3) == 1
        assert f(nc, na, 64, loss, only, 0) == 0 and f(nc, na, 64, loss, only, 33) == 0          # 0 and 33 replicas
        assert f(nc, na, 257, loss, only, 3) == 0 and f(nc, na, 0, loss, only, 3) == 0           # 257 rows
        assert f(nc, None, 64, loss, only, 3) == 0                                                # an actor is needed
    assert f(nc, na, 64, CLIP, 1, 3) == 0                                 # no actor-only step with the clipped surrogate
    assert f(nc, na, 64, 2, 0, 3) == 0 and f(nc, na, 64, -1, 0, 3) == 0   # not a loss
    # a shape the clipped surrogate's launch holds and the KL-penalty one (the rows' old distribution behind the actor's images)
    # does not: found by scanning the width through the two host functions
    found = None
    for width in range(200, 400, 4):
        c, a = _abi.MlpNet.of([60, width, width, 1]), _abi.MlpNet.of([60, width, width, 64])
        if lib.spo_wide_grad_rows_supported(c, a, 64) and not lib.spo_wide_kl_penalty_grad_rows_supported(c, a, 64):
            found = (width, c, a)
            break
    assert found is not None
    width, c, a = found
    assert f(c, a, 64, CLIP, 0, 2) == 1 and f(c, a, 64, KLPEN, 0, 2) == 0 and f(c, a, 64, KLPEN, 1, 2) == 0, width


# ------------------------------------------------------------------------------------------------ refused tables
PTRS = ("theta", "adam_m", "adam_v", "grad", "parts", "obs", "act", "logp_old", "target_r", "target_c", "adv", "perm", "cursor_dev",
        "pow4_dev", "losses3_out", "scalars4_out", "partial_ws", "loss_log_dev", "old_mean", "old_std")


def _table(S, active=1, capacity=3 * 1024, **cfg_kw):
    from safepo import _abi
    reps = (_abi.WideRowsExReplica * max(S, 1))()
    cfg = dict(obs_dim=60, act_dim=8, batch=64, clip=0.2, max_grad_norm=40.0, beta1=0.9, beta2=0.999, adam_eps=1e-8)
    cfg.update(cfg_kw)
    for i in range(S):
        r = reps[i]
        for k, name in enumerate(PTRS):
            setattr(r, name, 0x100000 * (i + 1) + 4096 * k)
        r.partial_capacity = capacity
        r.cfg = _abi.PpoCfg(**cfg)
        r.kl_bound, r.pg_coef, r.active = 0.02, 0.5, active
    return reps


@pytest.mark.parametrize("loss,only", [(KLPEN, 0), (KLPEN, 1), (CLIP, 0)])
def test_upload_refusals_come_before_any_device_work_in_order(lib, loss, only):
    """No GPU here: a call that reached HIP would fail differently, and the fake pointers are never touched."""
    from safepo import _abi
    f = lib.spo_wide_rows_ex_multi_upload
    nc, na = (_abi.MlpNet.of(d) for d in NETS)
    TAB, W = 0x7000000, "wide_rows_ex_multi_upload: "
    assert f(None, _table(2), 2, nc, na, 64, 64, loss, only, None) < 0 and _err(lib) == W + "null table"
    assert f(TAB, None, 2, nc, na, 64, 64, loss, only, None) < 0 and _err(lib) == W + "null table"
    for n in (0, -1, 33):
        assert f(TAB, _table(2), n, nc, na, 64, 64, loss, only, None) < 0 and _err(lib) == W + f"n_replicas {n} outside [1,32]"
    assert f(None, _table(2), 0, nc, na, 64, 64, loss, only, None) < 0 and "null table" in _err(lib)                 # (the table first)
    assert f(TAB, _table(2), 2, nc, na, 257, 64, 7, only, None) < 0 and _err(lib).startswith(W + "actor_loss 7 is neither")
    assert f(TAB, _table(2), 2, nc, na, 257, 64, CLIP, 1, None) < 0 and _err(lib).startswith(W + "actor_only needs the KL-penalty loss")
    form = "KL-penalty" if loss == KLPEN else "clipped-surrogate"
    for rows in (0, 257):
        assert f(TAB, _table(2), 2, nc, na, rows, 64, loss, only, None) < 0 and W + f"shape outside the row-group kernel's {form} form" in _err(lib)
    assert f(TAB, _table(2), 2, nc, None, 64, 64, loss, only, None) < 0 and "shape outside the row-group kernel" in _err(lib)
    big_c, big_a = _abi.MlpNet.of([300, 256, 256, 1]), _abi.MlpNet.of([300, 256, 256, 8])
    assert f(TAB, _table(2), 2, big_c, big_a, 64, 64, loss, only, None) < 0 and "shape outside the row-group kernel" in _err(lib)
    for name in PTRS:
        t = _table(3)
        setattr(t[1], name, None)
        rc = f(TAB, t, 3, nc, na, 64, 0, loss, only, None)                           # (cursor_step bad too: the later refusal)
        if name == "loss_log_dev" or (only and name in ("target_r", "target_c")) or (loss == CLIP and name in ("old_mean", "old_std")):
            assert rc < 0 and _err(lib) == W + "cursor_step must be > 0", name       # optional, as in the stand-alone entries
        elif name in ("target_r", "target_c"):
            assert rc < 0 and _err(lib) == W + "replica 1: critic targets are NULL", name
        elif name in ("old_mean", "old_std"):
            assert rc < 0 and _err(lib) == W + "replica 1: the KL-penalty loss needs old_mean / old_std", name
        else:
            assert rc < 0 and _err(lib) == W + "replica 1: null pointer", name
    for shared in ("theta", "parts", "cursor_dev"):
        t = _table(3, capacity=1)                                                    # (workspace too small as well: the later refusal)
        setattr(t[2], shared, getattr(t[0], shared))
        assert f(TAB, t, 3, nc, na, 64, 64, loss, only, None) < 0 and _err(lib) == W + f"replicas 0 and 2 share {shared}"
    t = _table(3)
    t[0].theta = None                                                                # a null pointer is named before a shared one
    t[2].parts = t[1].parts
    assert f(TAB, t, 3, nc, na, 64, 64, loss, only, None) < 0 and "replica 0: null pointer" in _err(lib)
    t = _table(2)
    for step in (0, -64):
        assert f(TAB, t, 2, nc, na, 64, step, loss, only, None) < 0 and _err(lib) == W + "cursor_step must be > 0"
    # 2 * 24 449 + 8 + 25 352 parameters: 291 blocks of 256 -> 873 doubles
    t[1].partial_capacity = 872
    assert f(TAB, t, 2, nc, na, 64, 64, loss, only, None) < 0 and _err(lib) == W + "partial workspace too small"
    assert f(TAB, _table(2, beta1=1.0), 2, nc, na, 64, 64, loss, only, None) < 0 and W + "betas (1, 0.999) outside [0, 1)" in _err(lib)
    assert f(TAB, _table(2, beta2=-0.5), 2, nc, na, 64, 64, loss, only, None) < 0 and "outside [0, 1)" in _err(lib)
    # an inactive run is not looked at: NULL pointers, a shared theta, no workspace, betas of any kind
    t = _table(3)
    t[1].active = 0
    for name in PTRS:
        setattr(t[1], name, None)
    t[1].partial_capacity = 0
    t[1].cfg.beta1 = 2.0
    assert f(TAB, t, 3, nc, na, 64, 0, loss, only, None) < 0 and _err(lib) == W + "cursor_step must be > 0"
    t[1].theta = t[0].theta
    assert f(TAB, t, 3, nc, na, 64, 0, loss, only, None) < 0 and _err(lib) == W + "cursor_step must be > 0"
    # the launch entry's own refusals
    g = lib.spo_wide_rows_ex_step_multi
    assert g(None, 2, nc, na, 64, loss, only, None) < 0 and _err(lib) == "wide_rows_ex_step_multi: null table"
    assert g(TAB, 33, nc, na, 64, loss, only, None) < 0 and _err(lib) == "wide_rows_ex_step_multi: n_replicas 33 outside [1,32]"
    assert g(TAB, 2, nc, na, 257, loss, only, None) < 0 and "wide_rows_ex_step_multi: shape or loss outside the row-group kernel" in _err(lib)
    assert g(TAB, 2, nc, na, 64, CLIP, 1, None) < 0 and "wide_rows_ex_step_multi: shape or loss outside the row-group kernel" in _err(lib)


def test_standalone_entries_keep_their_refusals(lib):
    """The stand-alone entries' checks and argument filling moved into shared code: their texts are what they were."""
    from safepo import _abi
    TAB = 0x7000000
    cfg = _abi.PpoCfg(obs_dim=60, act_dim=8, batch=64, beta1=0.9, beta2=0.999)
    h = lib.spo_wide_clip_adam_dev_log
    a = [TAB, TAB, TAB, TAB, 1000, 100, 200, 200, cfg, TAB, 0, 1000, 0, 0, TAB, TAB, TAB, 3 * 1024, None, None, TAB, 64, None]
    bad = list(a); bad[0] = None
    assert h(*bad) < 0 and _err(lib) == "wide_clip_adam_dev: bad args"
    bad = list(a); bad[5], bad[6] = 300, 200
    assert h(*bad) < 0 and _err(lib) == "wide_clip_adam_dev: parameter ranges out of order"
    bad = list(a); bad[10], bad[11] = 500, 400
    assert h(*bad) < 0 and _err(lib) == "wide_clip_adam_dev: optimiser range out of order"
    bad = list(a); bad[17] = 11
    assert h(*bad) < 0 and _err(lib) == "wide_clip_adam_dev: partial workspace too small"
    bad = list(a); bad[21] = 0
    assert h(*bad) < 0 and _err(lib) == "wide_clip_adam_dev_log: cursor_step must be > 0"
    bad = list(a); bad[8] = _abi.PpoCfg(obs_dim=60, act_dim=8, batch=64, beta1=1.5, beta2=0.999)
    assert h(*bad) < 0 and "wide_clip_adam_dev: betas (1.5, 0.999) outside [0, 1)" in _err(lib)
    e = lib.spo_wide_clip_adam_ex
    assert e(TAB, TAB, TAB, TAB, 1000, 100, 200, 200, cfg, -1, 0, 0, 1000, 0, 0, TAB, TAB, TAB, 3 * 1024, None) < 0 \
        and _err(lib) == "wide_clip_adam_ex: bad args"
    nc, na = (_abi.MlpNet.of(d) for d in NETS)
    k = lib.spo_wide_kl_penalty_grad_rows
    assert k(None, nc, na, TAB, TAB, TAB, TAB, TAB, TAB, TAB, TAB, TAB, TAB, 64, 0.02, 0.5, 0, TAB, None) < 0 \
        and _err(lib) == "wide_kl_penalty_grad_rows: null pointer"
    assert k(TAB, nc, na, TAB, TAB, TAB, None, TAB, TAB, TAB, TAB, TAB, TAB, 64, 0.02, 0.5, 0, TAB, None) < 0 \
        and _err(lib) == "wide_kl_penalty_grad_rows: critic targets are NULL"
    assert k(TAB, nc, na, TAB, TAB, TAB, TAB, TAB, TAB, TAB, TAB, TAB, TAB, 257, 0.02, 0.5, 0, TAB, None) < 0 \
        and _err(lib) == "wide_kl_penalty_grad_rows: rows 257 outside [1,256]"
    r = lib.spo_wide_kl_penalty_reduce_parts
    assert r(TAB, 64, 1000, 200, 0, 1, 0.5, TAB, None, TAB, TAB, None) < 0 and _err(lib) == "wide_kl_penalty_reduce_parts: null pointer"
    assert r(TAB, 257, 1000, 200, 0, 1, 0.5, TAB, TAB, TAB, TAB, None) < 0 and "wide_kl_penalty_reduce_parts: bad args (rows 257" in _err(lib)
    assert lib.spo_wide_reduce_parts(TAB, 64, 1000, 4, TAB, TAB, None) < 0 and _err(lib) == "wide_reduce_parts: bad args"


# ------------------------------------------------------------------------------------------------ the scripts' flag
def test_flag_parses_and_needs_batch_update(monkeypatch):
    from safepo.single_agent import _first_order, cpo, cup, focops, ppo_lag
    from safepo.utils import config
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0"])
    assert args.batch_klpen_rows is False
    called = []
    monkeypatch.setattr(_first_order, "run_seed_batch", lambda *a, **k: called.append((a, k)) or "batched")
    base = ["--task", "SynthSafe-v0", "--hidden-sizes", "128", "128", "--batch-klpen-rows", "True"]
    for argv in (["--seeds", "0", "1000"], ["--seed", "3"]):
        args, _ = config.single_agent_args(base + argv)
        assert args.batch_klpen_rows is True and args.batch_update is False
        for mod in (focops, cup):
            with pytest.raises(SystemExit, match="--batch-klpen-rows True widens --batch-update True for focops and cup.*give both"):
                mod.main(args, {})
        # the four PPO-family scripts and the six second-order scripts refuse the flag, with --batch-update True or without
        for extra in ([], ["--batch-update", "True"]):
            args2, _ = config.single_agent_args(base + argv + extra)
            with pytest.raises(SystemExit, match="--batch-klpen-rows True is not available for ppo_lag, ppo, pg and cppo_pid"):
                ppo_lag.main(args2, {})
            with pytest.raises(SystemExit, match="--batch-klpen-rows True is not available for the second-order scripts"):
                cpo.main(args2, {})
    assert called == []
    args, _ = config.single_agent_args(base + ["--seeds", "0", "1000", "--batch-update", "True"])
    for mod, variant in ((focops, "focops"), (cup, "cup")):
        assert mod.main(args, {}) == "batched"
        a, _k = called.pop()
        assert a[0].batch_klpen_rows is True and a[0].batch_update is True and variant in a and not called


def test_batch_wide_rows_on_focops_keeps_todays_refusal():
    from safepo.single_agent import cup, focops
    from safepo.utils import config
    for extra in ([], ["--batch-update", "True", "--batch-klpen-rows", "True"]):
        args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--hidden-sizes", "128", "128", "--seeds", "0", "1000",
                                            "--batch-wide-rows", "True"] + extra)
        for mod in (focops, cup):
            with pytest.raises(SystemExit) as ei:
                mod.main(args, {})
            assert str(ei.value) == ("--batch-wide-rows True is not available for focops and cup: the seed-batched row-group step is built "
                                     "for the clipped surrogate of ppo_lag, ppo, pg and cppo_pid only; the KL-penalty loss of focops / cup "
                                     "and the wide critic fit of the second-order scripts have no such form.  Run one process per seed")


def test_limits_are_named_before_anything_is_logged(monkeypatch, tmp_path):
    """hidden_sizes [128, 128] with two seeds under focops / cup: without --batch-klpen-rows the refusal text of before, word for
    word; with it a seed count or a shape that does not fit is refused before anything is logged, naming the limit."""
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
                               num_envs=4, steps_per_epoch=1024, total_steps=2048, use_eval=False, batch_update=True)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    cfg = {"hidden_sizes": [128, 128], "batch_size": 64}
    for variant in ("focops", "cup"):
        with pytest.raises(SystemExit) as ei:
            _first_order.run_seed_batch(ns(), {}, cfg, "adam", 0.2, variant)
        assert str(ei.value) == ("--seeds with more than one seed needs the persistent kernels' shapes (hidden_sizes [64, 64], obs_dim <= "
                                 "128, act_dim <= 16); SynthSafe-v0 with hidden_sizes [128, 128] runs on the wide-network "
                                 "kernels: one process per seed")
        with pytest.raises(SystemExit, match="at most 32 seeds share the row-group KL-penalty step's launches"):
            _first_order.run_seed_batch(ns(seeds=list(range(33)), batch_klpen_rows=True), {}, cfg, "adam", 0.2, variant)
        with pytest.raises(SystemExit, match="does not fit the row-group kernel's KL-penalty form"):
            _first_order.run_seed_batch(ns(batch_klpen_rows=True), {}, {"hidden_sizes": [512, 512], "batch_size": 64}, "adam", 0.2, variant)
        with pytest.raises(SystemExit, match="does not fit the row-group kernel's KL-penalty form"):
            _first_order.run_seed_batch(ns(batch_klpen_rows=True), {}, {"hidden_sizes": [128, 128], "batch_size": 512}, "adam", 0.2, variant)
        with pytest.raises(SystemExit, match="not a graph-replayed pass"):
            _first_order.run_seed_batch(ns(batch_klpen_rows=True, steps_per_epoch=128), {}, cfg, "adam", 0.2, variant)
    # the PPO family does not look at the flag inside run_seed_batch: today's refusal
    with pytest.raises(SystemExit, match="needs the persistent kernels' shapes"):
        _first_order.run_seed_batch(ns(batch_klpen_rows=True), {}, cfg, "adam", 0.2, "ppo")
    assert not os.path.exists(tmp_path / "runs")


# ------------------------------------------------------------------------------------------------ the sweep launcher
def test_benchmark_commands(capsys):
    from safepo.single_agent import benchmark
    algos = ["ppo_lag", "focops", "cup", "cpo"]
    base = ["--workers", "0", "--tasks", "SynthSafe-v0", "--algo"] + algos + ["--num-seeds", "3", "--seeds-per-run", "3"]
    plain = benchmark.main(base)
    assert not any("--batch-klpen-rows" in c for c in plain)
    # the flag without other widths, or without --batch-focops-cup, changes nothing
    assert benchmark.main(base + ["--batch-klpen-rows"]) == plain
    assert benchmark.main(base + ["--batch-klpen-rows", "--batch-focops-cup"]) == benchmark.main(base + ["--batch-focops-cup"])
    wide = benchmark.main(base + ["--hidden-sizes", "128", "128", "--batch-focops-cup"])
    assert benchmark.main(base + ["--hidden-sizes", "128", "128", "--batch-klpen-rows"]) == benchmark.main(base + ["--hidden-sizes", "128", "128"])
    assert len(wide) == 3 * len(algos) and not any("--seeds" in c for c in wide)
    rows = benchmark.main(base + ["--hidden-sizes", "128", "128", "--batch-focops-cup", "--batch-klpen-rows"])
    for algo in ("focops", "cup"):
        mine = [c for c in rows if f"{algo}.py " in c]
        assert len(mine) == 1 and ("--seed 0 --seeds 0 1000 2000 --hidden-sizes 128 128 --batch-update True --batch-klpen-rows True "
                                   "--write-terminal False") in mine[0]
    for algo in ("ppo_lag", "cpo"):
        mine = [c for c in rows if f"{algo}.py " in c]
        assert len(mine) == 3 and not any("--seeds" in c or "--batch-klpen-rows" in c for c in mine)
    # both row-group flags together: each family gets its own
    both = benchmark.main(base + ["--hidden-sizes", "128", "128", "--batch-focops-cup", "--batch-klpen-rows", "--batch-wide-rows"])
    assert [c for c in both if "focops.py " in c or "cup.py " in c] == [c for c in rows if "focops.py " in c or "cup.py " in c]
    assert len([c for c in both if "ppo_lag.py " in c]) == 1 and "--batch-wide-rows True" in [c for c in both if "ppo_lag.py " in c][0]
    # more seeds than the table holds: subprocesses of at most 32
    many = benchmark.main(["--workers", "0", "--tasks", "SynthSafe-v0", "--algo", "focops", "--num-seeds", "32", "--seeds-per-run", "32",
                           "--hidden-sizes", "256", "256", "--batch-focops-cup", "--batch-klpen-rows"])
    assert len(many) == 1 and many[0].count("000 ") >= 31
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------ the group's admission rule
def test_group_admission_with_and_without_the_keyword(monkeypatch):
    """Admission needs no device: a row-group group shares the steps of learning_iter_ex_all only with klpen_rows=True, and then
    where every engine's own pass would be the graph-replayed row-group step."""
    from safepo import _abi
    from safepo.common import engine
    from safepo.common.engine_group import PPOLagEngineGroup

    class _Comm:
        def __init__(self, world):
            self.world_size = world

    class _Wide:
        net_c, net_a = _abi.MlpNet.of(NETS[0]), _abi.MlpNet.of(NETS[1])

        def __init__(self, ok, kl_ok):
            self.ok, self.kl_ok = ok, kl_ok

        def rows_grad_ok(self, rows):
            return self.ok

        def klpen_rows_ok(self, rows):
            return self.kl_ok

    class _Pol:
        def __init__(self, hs):
            self.hidden_sizes = hs

    def fake(ks=False, world=1, rows_ok=True, kl_ok=True, M=64 * 5 + 7, batch=64, hs=(128, 128), graph_max=2048):
        e = object.__new__(engine.WidePPOLagEngine)
        e.D, e.A, e.M, e.dev, e.comm = 60, 8, M, torch.device("cpu"), _Comm(world)
        e._cfg_struct = lambda: _abi.PpoCfg(obs_dim=60, act_dim=8, batch=batch)
        e._feature_split_kernel_ok = lambda cfg: ks
        e.wide, e.policy, e.graph_max_batch = _Wide(rows_ok, kl_ok), _Pol(list(hs)), graph_max
        return e

    def kinds(g):
        return [g.batched_ex(KLPEN), g.batched_ex(KLPEN, None, True), g.batched_ex(CLIP), g.batched_ex(CLIP, None, True)]

    g0 = PPOLagEngineGroup([fake(), fake(), fake()])
    assert g0._rows and g0.batched() and kinds(g0) == [False] * 4                    # without the keyword: as ever
    g = PPOLagEngineGroup([fake(), fake(), fake()], klpen_rows=True)
    assert g._rows and not g._ks and g.batched() and kinds(g) == [True, True, True, False]
    assert kinds(PPOLagEngineGroup([fake() for _ in range(32)], klpen_rows=True)) == [True, True, True, False]
    assert kinds(PPOLagEngineGroup([fake() for _ in range(33)], klpen_rows=True)) == [False] * 4
    # the KL-penalty form's own LDS fit; the clipped surrogate's
    assert kinds(PPOLagEngineGroup([fake(), fake(kl_ok=False)], klpen_rows=True)) == [False, False, True, False]
    assert kinds(PPOLagEngineGroup([fake(), fake(rows_ok=False)], klpen_rows=True)) == [True, True, False, False]
    assert kinds(PPOLagEngineGroup([fake(M=128), fake(M=128)], klpen_rows=True)) == [False] * 4     # two minibatches: not graph-replayed
    assert kinds(PPOLagEngineGroup([fake(graph_max=0), fake()], klpen_rows=True)) == [False] * 4
    assert kinds(PPOLagEngineGroup([fake(batch=64), fake(batch=32)], klpen_rows=True)) == [False] * 4   # equal batch
    monkeypatch.setenv("SPO_WIDE_ROWS_FUSED", "0")                                   # (the PPO step's switch: not this step's)
    assert not g.batched() and kinds(g) == [True, True, True, False]
    monkeypatch.delenv("SPO_WIDE_ROWS_FUSED")
    with pytest.raises(_abi.SpoError, match="world size 1"):
        PPOLagEngineGroup([fake(), fake(world=2)], klpen_rows=True)
    # the keyword changes nothing for the other kinds of group
    ks = PPOLagEngineGroup([fake(ks=True, hs=(64, 64)), fake(ks=True, hs=(64, 64))], klpen_rows=True)
    assert ks._ks and not ks._rows
