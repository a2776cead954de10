"""CPU tests (no GPU) of the seed-batched feature-split critic fit (129-512 observations): the entry points are declared,
exported and bound; the support rule over its whole range; the block -> (run, workgroup) mapping of the launch (the function the
kernel itself uses); what the launch refuses on the host; CPOEngineGroup(ks_form=True)'s grouping rules, its loop on recording
stand-in engines, its fallback and its error path; the opt-in flags of the scripts and of the sweep launcher; and the clip
condition of the GPU tests' problems (run 0 clips, run 1 never does, on the very initialisations and scalars
test_gpu_seed_batch_critic_ks.py uses)."""
import ctypes
import os
import random
import re
import shlex
import sys

import numpy as np
import pytest
import torch

import critic_ks_batch_problem as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("spo_critic_fit_iter_ks_multi", "spo_critic_fit_ks_multi_supported", "spo_critic_fit_ks_multi_block_map",
               "spo_debug_critic_fit_ks_multi_counters")
KS_MAX = 16


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


def _cap(D):
    """The rule, recomputed from S: at most 24 working blocks per XCD label, a run being 2 S blocks."""
    S = (D + 63) // 64
    return min(KS_MAX, 8 * (24 // (2 * S)))


# ------------------------------------------------------------------------------------------------ symbols
def test_symbols_declared_exported_and_bound(lib):
    from safepo import _abi
    c_int, c_int64, P_ = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    header = open(os.path.join(ROOT, "include", "safepo_hip.h")).read()
    assert "#define SPO_KS_MAX_REPLICAS 16" in header and _abi.KS_MAX_REPLICAS == KS_MAX
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name
    assert _abi.PROTOTYPES["spo_critic_fit_iter_ks_multi"] == (c_int, [ctypes.POINTER(_abi.CriticFitReplica), c_int, c_int64, P_])
    assert _abi.PROTOTYPES["spo_critic_fit_ks_multi_supported"] == (c_int, [c_int] * 3)
    assert _abi.PROTOTYPES["spo_critic_fit_ks_multi_block_map"] == (c_int, [c_int] * 3 + [ctypes.POINTER(c_int)] * 2)
    assert _abi.PROTOTYPES["spo_debug_critic_fit_ks_multi_counters"] == (c_int, [P_, c_int])


def test_counters_refuse_a_null_array(lib):
    assert lib.spo_debug_critic_fit_ks_multi_counters(None, 0) < 0 and "null pointer" in lib.spo_last_error().decode()


# ------------------------------------------------------------------------------------------------ support rule
def test_supported_rule(lib):
    f = lib.spo_critic_fit_ks_multi_supported
    for D in range(1, 514):
        for B in (0, 1, 64, 65, 128, 129):
            got = [f(D, B, n) for n in range(0, 18)]
            want = [int(1 <= D <= 512 and 1 <= B <= 128 and 1 <= n <= _cap(D)) for n in range(0, 18)]
            assert got == want, (D, B, got, want)
    assert [_cap(D) for D in (376, 384, 385, 512)] == [16, 16, 8, 8]
    assert [f(376, 128, 16), f(384, 128, 16), f(385, 128, 8), f(385, 128, 9), f(512, 128, 8), f(512, 128, 9)] == [1, 1, 1, 0, 1, 0]


# ------------------------------------------------------------------------------------------------ block mapping
def _walk(fn, D, n, blocks):
    out = []
    for b in blocks:
        rep, wg = ctypes.c_int(-1), ctypes.c_int(-1)
        out.append((b, fn(b, D, n, ctypes.byref(rep), ctypes.byref(wg)), rep.value, wg.value))
    return out


@pytest.mark.parametrize("D", [129, 192, 376, 448, 512])
def test_block_mapping(lib, D):
    f = lib.spo_critic_fit_ks_multi_block_map
    S = (D + 63) // 64
    wgs = 2 * S
    for n in range(1, _cap(D) + 1):
        grid = 8 * wgs * ((n + 7) // 8)
        seen, per_label = {}, [0] * 8
        for b, work, rep, wg in _walk(f, D, n, range(grid)):
            x, k = b & 7, b >> 3
            want_rep, want_wg = 8 * (k // wgs) + x, k % wgs
            if want_rep >= n:
                assert work == 0, (D, n, b)
                continue
            assert work == 1 and (rep, wg) == (want_rep, want_wg), (D, n, b, rep, wg)
            assert 0 <= rep < n and 0 <= wg < wgs
            assert (b & 7) == (rep & 7)                                  # run r sits only on blocks of label r & 7
            assert (rep, wg) not in seen, (D, n, b, seen[(rep, wg)])     # every block serves at most one (run, workgroup)
            seen[(rep, wg)] = b
            per_label[x] += 1
        assert sorted(seen) == [(r, w) for r in range(n) for w in range(wgs)]   # one-to-one onto all pairs
        assert max(per_label) <= 24                                      # 24 one-CU workgroups on an XCD's 32 CUs
        for _b, work, _r, _w in _walk(f, D, n, (-1, grid, grid + 5, 8 * wgs * 2)):
            assert work == 0                                             # outside the grid
        assert f(0, D, n, None, None) == 1                               # (the outputs are optional)
    for n in (0, -3, _cap(D) + 1, 17):
        assert f(0, D, n, None, None) == 0                               # run counts outside the cap
    assert f(0, 0, 1, None, None) == 0 and f(0, 513, 1, None, None) == 0


# ------------------------------------------------------------------------------------------------ host refusals
POINTERS = ("theta", "adam_m", "adam_v", "obs", "target_r", "target_c", "perm", "losses_out", "stale_sq_io", "sync_ws")


def _table(n, D=376, A=17, batch=128):
    from safepo import _abi
    reps = (_abi.CriticFitReplica * max(n, 1))()
    for i in range(n):
        base = 0x100000 * (i + 1)
        r = reps[i]
        for k, name in enumerate(POINTERS):
            setattr(r, name, base + 256 * k)
        r.cfg = _abi.PpoCfg(obs_dim=D, act_dim=A, batch=batch)
        r.active = 1
    return reps


def test_host_validation_happens_before_any_device_work(lib):
    """No GPU here: anything that reached HIP would fail with a HIP error instead of these messages (as test_abi_and_host.py
    does for the single launch)."""
    f = lib.spo_critic_fit_iter_ks_multi

    def err():
        return lib.spo_last_error().decode()

    M = 647
    assert f(None, 2, M, None) < 0 and "null replica table" in err()
    assert f(_table(1), 0, M, None) < 0 and "0 replicas outside [1, 16]" in err()
    assert f(_table(17), 17, M, None) < 0 and "17 replicas outside [1, 16]" in err()
    assert f(_table(9, D=448), 9, M, None) < 0 and "at most 8 runs" in err()              # the shape's cap: S = 7
    assert f(_table(16, D=385), 16, M, None) < 0 and "at most 8 runs" in err()
    assert f(_table(2), 2, 0, None) < 0 and "bad sizes" in err()
    assert f(_table(2), 2, -64, None) < 0 and "bad sizes" in err()
    for field, value in (("obs_dim", 192), ("act_dim", 3), ("batch", 64)):
        t = _table(3)
        setattr(t[2].cfg, field, value)
        assert f(t, 3, M, None) < 0 and "replica 2 has obs_dim / act_dim / batch" in err(), field
    for kw in ({"D": 0}, {"D": 513}, {"batch": 0}, {"batch": 129}):
        assert f(_table(2, **kw), 2, M, None) < 0 and "outside [1,512] / [1,128]" in err(), kw
    assert f(_table(2, A=0), 2, M, None) < 0 and "act_dim 0" in err()
    for field in POINTERS:
        t = _table(2)
        setattr(t[1], field, None)
        want = "stale_sq_io is NULL in replica 1" if field == "stale_sq_io" else "null pointer in replica 1"
        assert f(t, 2, M, None) < 0 and want in err(), field
    t = _table(2)
    t[0].adam_step = -1
    assert f(t, 2, M, None) < 0 and "replica 0: negative adam_step" in err()
    for field in ("theta", "sync_ws", "stale_sq_io"):
        t = _table(3)
        setattr(t[2], field, getattr(t[0], field))
        assert f(t, 3, M, None) < 0 and "replicas 0 and 2 share theta, sync_ws or stale_sq_io" in err(), field
    assert f(_table(2, batch=1), 2, 1 << 30, None) < 0 and "too many minibatch steps" in err()
    # a run that sits out may leave perm and losses_out null; its other pointers are still checked
    t = _table(3)
    for r in t:
        r.active = 0
        r.perm = r.losses_out = None
    assert f(t, 3, M, None) == 0                                   # all runs inactive: nothing enqueued (no HIP call: 0 without a GPU)
    t[1].stale_sq_io = None
    assert f(t, 3, M, None) < 0 and "stale_sq_io is NULL in replica 1" in err()
    t = _table(3)
    for r in t:
        r.active = 0
    t[2].theta = None
    assert f(t, 3, M, None) < 0 and "null pointer in replica 2" in err()


# ------------------------------------------------------------------------------------------------ CPOEngineGroup on stand-ins
class _StubComm:
    world_size = 1


class _StubPolicy:
    hidden_sizes = [64, 64]

    def __init__(self, v):
        self.theta = torch.full((6,), float(v))


class _StubEngine:
    """Records what the group asks of an engine; critic_fit is WideCPOEngine.critic_fit's feature-split loop without the launch.
    Holds the state the group's loop reads, rescales and restores (parameters, moments, stale norm and vector, clock, error word)."""
    D, A, M, dev, ls_off = 376, 17, 256, torch.device("cpu"), 2

    def __init__(self, learning_iters, v=1.0):
        self.log, self.cfg, self.comm = [], {"learning_iters": learning_iters, "batch_size": 128}, _StubComm()
        self.policy, self.adam_m, self.adam_v = _StubPolicy(v), torch.full((6,), v + 0.25), torch.full((6,), v + 0.5)
        self.stale_sq, self.adam_step = torch.tensor([v + 0.75]), 7
        self.flat_grad = torch.arange(6, dtype=torch.float32) + v
        self.sync_ws = torch.zeros(32, dtype=torch.int64)

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
    """A ks_form group whose launch is replaced by a recorder that moves the state the way the launch would."""
    from safepo.common.engine_group import CPOEngineGroup
    group = CPOEngineGroup(es, ks_form=True)
    group.batched_ks = lambda: True
    launches = []

    def fit_iter_ks_all(perms, active=None):
        launches.append((list(perms), list(active)))
        out = []
        for i, e in enumerate(es):
            if not active[i]:
                out.append(None)
                continue
            e.log.append(("launch", len(launches) - 1, perms[i]))
            e.policy.theta += 1.0; e.adam_m += 1.0; e.adam_v += 1.0; e.stale_sq *= 0.25
            e.adam_step += 2
            out.append(torch.tensor([[1.0 + i, 2.0 * len(launches), -1.0]] * 2))
        if on_launch is not None:
            on_launch(len(launches) - 1)
        return out

    group.fit_iter_ks_all = fit_iter_ks_all
    return group, launches


def test_group_falls_back_to_per_engine_critic_fit_where_not_batched_ks():
    from safepo.common.engine_group import CPOEngineGroup
    es = [_StubEngine(n) for n in (1, 3, 2)]
    group = CPOEngineGroup(es, ks_form=True)
    assert len(group) == 3 and group.ks_form and not group.batched_ks() and not group.batched() and not group.batched_split()
    outs = group.critic_fit_all([e.perm_fn for e in es])
    alone = [_StubEngine(n) for n in (1, 3, 2)]
    alone_out = [e.critic_fit(e.perm_fn) for e in alone]
    for e, a, o, ao in zip(es, alone, outs, alone_out):
        assert e.log == a.log
        assert (o["loss_r"], o["loss_c"]) == (ao["loss_r"], ao["loss_c"]) and len(o["losses"]) == len(ao["losses"])
    g = CPOEngineGroup([_StubEngine(1)])                             # without the switch batched_ks() is never true
    assert g.ks_form is False and not g.batched_ks()


def test_group_ks_loop_order_masks_and_rescale():
    """The loop itself (the launch replaced by a recorder): per run, iteration it's shuffle is drawn before launch it and after
    launch it - 1, as WideCPOEngine.critic_fit draws it; a run with fewer learning_iters sits out the later launches; after the
    loop the run's stale vector is rescaled by sqrt(stale_sq / stale0) -- 0.5 per launch it took part in here."""
    n_its = (1, 3, 2)
    es = [_StubEngine(n, v=1.0 + i) for i, n in enumerate(n_its)]
    tails = [e.flat_grad.clone() for e in es]
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
        assert e.adam_step == 7 + 2 * n
        assert torch.equal(e.flat_grad[:2], tails[i][:2])            # the critics' part of flat_grad is not the rescale's
        assert torch.allclose(e.flat_grad[2:], tails[i][2:] * 0.5 ** n, rtol=1e-6)
    es0 = [_StubEngine(0), _StubEngine(0)]                           # no learning iterations at all: nothing launched, NaN means
    g0, l0 = _recording_group(es0)
    o = g0.critic_fit_all()
    assert l0 == [] and all(np.isnan(x["loss_r"]) and x["losses"] == [] for x in o)


def test_group_ks_loop_draws_default_shuffles_under_the_runs_generators():
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


def test_group_ks_error_restores_every_run_and_names_the_run():
    from safepo import _abi
    es = [_StubEngine(2, v=1.0 + i) for i in range(3)]
    before = [(e.policy.theta.clone(), e.adam_m.clone(), e.adam_v.clone(), e.stale_sq.clone(), e.flat_grad.clone(), e.adam_step) for e in es]

    def on_launch(k):
        if k == 1:                                                  # the exchange of run 1 gave up during the second launch
            es[1].sync_ws[8] = 1

    group, launches = _recording_group(es, on_launch)
    with pytest.raises(_abi.SpoError, match=r"replica 1 of 3: feature-split critic fit: exchange error 1"):
        group.critic_fit_all([e.perm_fn for e in es])
    assert len(launches) == 2
    for e, b in zip(es, before):
        assert torch.equal(e.policy.theta, b[0]) and torch.equal(e.adam_m, b[1]) and torch.equal(e.adam_v, b[2])
        assert torch.equal(e.stale_sq, b[3]) and torch.equal(e.flat_grad, b[4]) and e.adam_step == b[5]
        assert int(e.sync_ws[8]) == 0                                # the words are cleared


def _wide(lib, D, batch=128, persistent=False, hidden=(64, 64)):
    """A WideCPOEngine shell (no device behind it) with what the group's rules read."""
    from safepo import _abi
    from safepo.single_agent.cpo import WideCPOEngine
    w = object.__new__(WideCPOEngine)
    w.D, w.A, w.M, w.dev, w.comm, w.lib = D, 17, 647, torch.device("cpu"), _StubComm(), lib
    w._critics_on_persistent_kernel = persistent
    w.policy = type("Pol", (), {"hidden_sizes": list(hidden)})()
    w._cfg_struct = lambda: _abi.PpoCfg(obs_dim=D, act_dim=17, batch=batch)
    w._split_setup = lambda: None
    return w


def test_group_rules(lib, monkeypatch):
    from safepo import _abi
    from safepo.common.engine_group import CPOEngineGroup
    monkeypatch.delenv("SPO_WIDE_KS", raising=False)
    with pytest.raises(_abi.SpoError, match="WideCPOEngine"):       # today's behaviour without the switch
        CPOEngineGroup([_wide(lib, 376)])
    for bad in (_wide(lib, 128), _wide(lib, 513), _wide(lib, 376, hidden=(96, 96)), _wide(lib, 100, persistent=True)):
        with pytest.raises(_abi.SpoError, match="WideCPOEngine"):   # outside 129-512 observations / other widths
            CPOEngineGroup([bad], ks_form=True)
    dp = _wide(lib, 376)
    dp.comm = type("C", (), {"world_size": 2})()
    with pytest.raises(_abi.SpoError, match="world size 1 only"):
        CPOEngineGroup([dp], ks_form=True)
    # the cap at construction: 16 up to 384 observations, 8 above
    assert len(CPOEngineGroup([_wide(lib, 376) for _ in range(16)], ks_form=True)) == 16
    with pytest.raises(_abi.SpoError, match="at most 16"):
        CPOEngineGroup([_wide(lib, 376) for _ in range(17)], ks_form=True)
    assert len(CPOEngineGroup([_wide(lib, 448) for _ in range(8)], ks_form=True)) == 8
    with pytest.raises(_abi.SpoError, match="at most 8"):
        CPOEngineGroup([_wide(lib, 448) for _ in range(9)], ks_form=True)
    with pytest.raises(_abi.SpoError, match="at most 24"):          # stand-ins and CPOEngines keep the cap of 24, switch or not
        CPOEngineGroup([_StubEngine(1) for _ in range(25)], ks_form=True)
    with pytest.raises(_abi.SpoError, match="engine 1 has obs"):
        CPOEngineGroup([_wide(lib, 376), _wide(lib, 448)], ks_form=True)
    # batched_ks(): equal batches on the feature-split kernel, and only with the switch
    group = CPOEngineGroup([_wide(lib, 376) for _ in range(3)], ks_form=True)
    assert group.batched_ks() and not group.batched() and not group.batched_split()
    assert CPOEngineGroup([_wide(lib, 129), _wide(lib, 129)], ks_form=True).batched_ks()
    assert CPOEngineGroup([_wide(lib, 512, batch=1) for _ in range(8)], ks_form=True).batched_ks()
    assert not CPOEngineGroup([_wide(lib, 376), _wide(lib, 376, batch=64)], ks_form=True).batched_ks()      # unequal batch
    assert not CPOEngineGroup([_wide(lib, 376, batch=129) for _ in range(2)], ks_form=True).batched_ks()    # outside the kernel
    monkeypatch.setenv("SPO_WIDE_KS", "0")
    assert not group.batched_ks()                                   # the engines' own critic fit leaves the kernel too
    monkeypatch.delenv("SPO_WIDE_KS")
    with pytest.raises(ValueError, match="one perm and one active flag"):
        group.fit_iter_ks_all([None], [True, True, True])


# ------------------------------------------------------------------------------------------------ the flags
def test_flag_default_and_refusal_without_the_flag_it_widens():
    from safepo.utils import config
    args, _ = config.single_agent_args([])
    assert args.batch_critic_fit_feature_split is False and args.batch_critic_fit is False
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "--batch-critic-fit-feature-split", "True"])
    assert args.batch_critic_fit_feature_split is True
    for name in ("cpo", "pcpo", "trpo_lag", "rcpo", "trpo", "natural_pg"):
        mod = __import__(f"safepo.single_agent.{name}", fromlist=["main"])
        with pytest.raises(SystemExit, match="--batch-critic-fit-feature-split True widens --batch-critic-fit True"):
            mod.main(args, {})
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "--batch-critic-fit", "True",
                                        "--batch-critic-fit-feature-split", "True"])
    assert config.critic_seed_batch(args) is True
    args, _ = config.single_agent_args(["--seeds", "3", "--batch-critic-fit", "True", "--batch-critic-fit-feature-split", "True"])
    assert config.critic_seed_batch(args) is False                  # one seed stays --seed


def test_flag_refusals_before_any_device_work(monkeypatch):
    from safepo.single_agent import cpo, trpo_lag
    from safepo.utils import config
    both = ["--batch-critic-fit", "True", "--batch-critic-fit-feature-split", "True"]
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "4", "4"] + both)
    with pytest.raises(SystemExit, match="same seed twice"):
        cpo.main(args, {})
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds"] + [str(s) for s in range(17)] + both)
    for mod in (cpo, trpo_lag):
        with pytest.raises(SystemExit, match="at most 16 seeds share a launch with --batch-critic-fit-feature-split True"):
            mod.main(args, {})
    # without the new flag every refusal is the parent's: 17 seeds pass this check (the cap of 24 holds) and 25 are refused with its text
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--batch-critic-fit", "True", "--seeds"] + [str(s) for s in range(25)])
    with pytest.raises(SystemExit, match=r"--seeds: at most 24 seeds share the critic fit's launch, got 25"):
        trpo_lag.main(args, {})
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000"])
    with pytest.raises(SystemExit, match=r"Opt in with --batch-critic-fit True: the seeds' critic fits then share one persistent launch"):
        cpo.main(args, {})
    args, _ = config.single_agent_args(["--task", "SynthSafe-v0", "--seeds", "0", "1000", "--batch-critic-fit-split", "True"])
    with pytest.raises(SystemExit, match=r"--batch-critic-fit-split True widens --batch-critic-fit True \(65-128 observations, up to 32 seeds\): give both"):
        cpo.main(args, {})


def test_help_text_names_the_flags_and_their_measurement(capsys):
    from safepo.single_agent import benchmark
    from safepo.utils import config
    for parse, flag in ((config.single_agent_args, "--batch-critic-fit-feature-split"),
                        (benchmark.parse_args, "--batch-second-order-feature-split")):
        capsys.readouterr()
        with pytest.raises(SystemExit):
            parse(["--help"])
        text = " ".join(capsys.readouterr().out.split())
        assert flag in text and "profiles/seed_batch_critic_ks/step_times.txt" in text, flag
    for name in ("step_times.txt", "kernel_isa_compare.txt", "resource_usage.txt"):
        assert os.path.exists(os.path.join(ROOT, "profiles", "seed_batch_critic_ks", name)), name


def _cmd(algo, task, seeds, gpu, extra=()):
    from safepo.single_agent import benchmark
    head = [shlex.quote(sys.executable), shlex.quote(os.path.join(benchmark.HERE, f"{algo}.py")), "--task", task, "--seed", str(seeds[0])]
    if len(seeds) > 1:
        head += ["--seeds"] + [str(s) for s in seeds]
    return " ".join(head + list(extra) + ["--write-terminal", "False", "--experiment", "benchmark", "--total-steps", "10000000",
                                            "--num-envs", "10", "--steps-per-epoch", "20000", "--device-id", str(gpu)])


HUMANOID, SYNTH, CAR = "SafetyHumanoidVelocity-v1", "SynthSafe-v0", "SafetyCarGoal1-v0"
ALGOS = ("cpo", "pcpo", "rcpo", "trpo_lag", "trpo", "natural_pg")


def test_launcher_groups_humanoid_only_with_both_flags(monkeypatch):
    from safepo.single_agent import benchmark
    monkeypatch.setattr(benchmark, "visible_gpus", lambda: 1)
    flag = ("--batch-critic-fit", "True")
    ks = ("--batch-critic-fit", "True", "--batch-critic-fit-feature-split", "True")
    s10 = [1000 * k for k in range(10)]
    base = ["--workers", "0", "--tasks", HUMANOID, SYNTH, CAR, "--algo"] + list(ALGOS) + ["ppo_lag", "--num-seeds", "10", "--seeds-per-run", "10"]
    with pytest.raises(SystemExit, match="--batch-second-order-feature-split widens --batch-second-order: give both"):
        benchmark.main(base + ["--batch-second-order-feature-split"])
    got = benchmark.main(base + ["--batch-second-order", "--batch-second-order-feature-split"])
    want = []
    for t in (HUMANOID, SYNTH, CAR):
        for a in ALGOS:
            if t == HUMANOID:                                       # at most 8 seeds per subprocess, the script flag appended
                want += [_cmd(a, t, s10[:8], 0, ks), _cmd(a, t, s10[8:], 0, ks)]
            elif t == SYNTH:
                want.append(_cmd(a, t, s10, 0, flag))
            else:                                                    # 72 observations: not this flag's
                want.extend(_cmd(a, t, [s], 0) for s in s10)
        want.append(_cmd("ppo_lag", t, s10, 0)) if t != HUMANOID else want.extend(_cmd("ppo_lag", t, [s], 0) for s in s10)
    assert got == want
    # without the new flag: what the launcher prints today -- HumanoidVelocity one subprocess per seed, no command names the flag
    got = benchmark.main(base + ["--batch-second-order"])
    want = []
    for t in (HUMANOID, SYNTH, CAR):
        for a in ALGOS:
            want.append(_cmd(a, t, s10, 0, flag)) if t == SYNTH else want.extend(_cmd(a, t, [s], 0) for s in s10)
        want.append(_cmd("ppo_lag", t, s10, 0)) if t != HUMANOID else want.extend(_cmd("ppo_lag", t, [s], 0) for s in s10)
    assert got == want and not any("feature-split" in c for c in got)
    # --seeds-per-run 1: the flags alone change nothing
    one = ["--workers", "0", "--tasks", HUMANOID, "--algo", "cpo", "--num-seeds", "2"]
    assert benchmark.main(one + ["--batch-second-order", "--batch-second-order-feature-split"]) == benchmark.main(one)


# ------------------------------------------------------------------------------------------------ the clip condition
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_clip_condition_on_the_tests_own_initialisation(shape, monkeypatch):
    """At every batch of the GPU tests: the float32 oracle (CriticFitter, cpo.py:541-571) on ActorVCritic's own initialisation
    and the runs' own learning rates and bounds has run 0 (max_grad_norm 0.6) clip its first step with a 5 % margin and run 1
    (max_grad_norm 1000) stay below a twentieth of its bound on every step of both iterations."""
    from oracle import restatement as R
    norms = []
    orig = torch.nn.utils.clip_grad_norm_

    def recording(params, max_norm, *a, **kw):
        n = orig(params, max_norm, *a, **kw)
        norms.append(float(n))
        return n

    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", recording)
    D, A = shape
    for batch in P.BATCHES:
        for r in range(2):
            del norms[:]
            pol = P.make_policy(shape, r)
            ref = R.OraclePolicy(D, A)
            ref.load_state_dict({k: v.detach().clone() for k, v in pol.state_dict().items()})
            n_act = sum(p.numel() for p in ref.actor.parameters())
            for p in ref.actor.parameters():                        # any vector of that norm: only its norm enters the clip
                p.grad = torch.full_like(p, float(np.sqrt(P.stale_sq0(r) / n_act)))
            fitter = R.CriticFitter(ref, lr=P.lr_critic(r), max_grad_norm=P.max_grad_norm(r))
            obs, tgt_r, tgt_c = P.make_rows(shape, r, batch)
            for perm in P.make_perms(r, batch):
                for k in range(P.n_steps(batch)):
                    idx = perm[k * batch:(k + 1) * batch].long()
                    fitter.minibatch_step(obs[idx], tgt_r[idx], tgt_c[idx])
            assert len(norms) == 2 * P.n_steps(batch) == 12
            print(f"{shape} batch {batch} run {r}: joint norms {min(norms):.3f} .. {max(norms):.3f}, bound {P.max_grad_norm(r)}")
            if r == 0:
                assert norms[0] > 1.05 * P.max_grad_norm(0), norms
            else:
                assert max(norms) < 0.05 * P.max_grad_norm(1), norms
