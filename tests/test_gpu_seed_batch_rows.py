"""GPU tests of the seed-batched row-group step (spo_wide_rows_multi_upload + spo_wide_rows_step_multi, csrc/mlp_rows.hip;
PPOLagEngineGroup of WidePPOLagEngines on the row-group kernel; --batch-wide-rows): every run of a batched step is compared BIT FOR
BIT with its own stand-alone sequence spo_wide_ppo_grad_rows + spo_wide_rows_clip_adam_dev_log on a copy of the same state, over four
consecutive steps that end on the last rows of the permutation."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
STEPS = 4
GUARD = 64                     # elements of sentinel on either side of an inactive run's buffers
STATE = ("theta", "m", "v", "grad", "pow4", "cursor", "scal4", "loss_log", "losses3")


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from safepo import _abi
    return _abi.load(g.LIB)


def _guarded(n, dtype, dev, fill):
    """A buffer of n elements between GUARD sentinel elements: (whole allocation, the view a run uses)."""
    whole = torch.full((n + 2 * GUARD,), -77, dtype=dtype, device=dev)
    view = whole[GUARD:GUARD + n]
    view.copy_(fill)
    return whole, view


class _Run:
    """One run's state and data: random parameters / moments / buffer, its own shuffle, the device clocks of step `t0`."""

    def __init__(self, lib, D, A, hidden, rows, seed, max_grad_norm, dev):
        from safepo import _abi
        g = torch.Generator().manual_seed(seed)
        self.net_c, self.net_a = _abi.MlpNet.of([D] + hidden + [1]), _abi.MlpNet.of([D] + hidden + [A])
        Pc, Pa = int(lib.spo_mlp_param_count(self.net_c)), int(lib.spo_mlp_param_count(self.net_a))
        self.Pc, self.P, self.rows, self.M = Pc, 2 * Pc + A + Pa, rows, STEPS * rows
        P, M = self.P, self.M
        f32 = dict(dtype=torch.float32)
        theta = 0.2 * torch.randn(P, generator=g, **f32)
        theta[2 * Pc:2 * Pc + A] = -0.5 + 0.1 * torch.randn(A, generator=g, **f32)          # log_std
        t0 = 3 + seed % 5
        b1, b2 = 0.9, 0.999
        fills = {
            "theta": theta, "m": 0.01 * torch.randn(P, generator=g, **f32), "v": 1e-4 * torch.rand(P, generator=g, **f32),
            "grad": torch.zeros(P, **f32),
            "pow4": torch.tensor([b1 ** t0, b2 ** t0, b1 ** (t0 + 2), b2 ** (t0 + 2), 3e-4 * (1 + seed % 3), 1e-3], dtype=torch.float64),
            "cursor": torch.zeros(1, dtype=torch.int64), "scal4": torch.zeros(4, **f32),
            "loss_log": torch.full((STEPS * 3,), float("nan"), **f32), "losses3": torch.zeros(3, **f32),
            "parts": torch.zeros(int(lib.spo_wide_grad_rows_part_floats(P, rows)), **f32),
            "partial": torch.zeros(3 * 1024, dtype=torch.float64),
        }
        self.whole, self.t = {}, {}
        for k, v in fills.items():
            self.whole[k], self.t[k] = _guarded(v.numel(), v.dtype, dev, v.to(dev))
        self.obs = torch.randn(M, D, generator=g, **f32).to(dev)
        self.act = torch.randn(M, A, generator=g, **f32).to(dev)
        self.logp_old = (-0.5 * A + 0.3 * torch.randn(M, generator=g, **f32)).to(dev)
        self.tgt_r, self.tgt_c = torch.randn(M, generator=g, **f32).to(dev), torch.randn(M, generator=g, **f32).to(dev)
        self.adv = torch.randn(M, generator=g, **f32).to(dev)
        self.perm = torch.randperm(M, generator=g).to(torch.int64).to(dev)
        self.cfg = _abi.PpoCfg(obs_dim=D, act_dim=A, batch=rows, use_critic_norm=1, use_value_coefficient=seed % 2, clip=0.2,
                               max_grad_norm=max_grad_norm, lr_actor=3e-4, lr_critic=3e-4, beta1=b1, beta2=b2, adam_eps=1e-8, l2_coef=0.001)

    def snapshot(self):
        return {k: self.t[k].clone() for k in STATE}

    def restore(self, snap):
        for k in STATE:
            self.t[k].copy_(snap[k])
        self.t["parts"].zero_()
        self.t["partial"].zero_()

    def standalone_steps(self, lib):
        """STEPS stand-alone steps from the current state; the state after each."""
        from safepo import _abi
        p, t, st, out = _abi.ptr, self.t, _abi.stream_ptr(), []
        for _ in range(STEPS):
            _abi.check(lib.spo_wide_ppo_grad_rows(p(t["theta"]), self.net_c, self.net_a, p(self.obs), p(self.act), p(self.logp_old),
                                                  p(self.tgt_r), p(self.tgt_c), p(self.adv), p(self.perm), p(t["cursor"]), self.rows,
                                                  float(self.cfg.clip), p(t["parts"]), st), "spo_wide_ppo_grad_rows")
            _abi.check(lib.spo_wide_rows_clip_adam_dev_log(
                p(t["parts"]), self.rows, p(t["theta"]), p(t["grad"]), p(t["m"]), p(t["v"]), self.P, self.Pc, 2 * self.Pc, 2 * self.Pc,
                self.cfg, p(t["pow4"]), p(t["losses3"]), p(t["scal4"]), p(t["partial"]), t["partial"].numel(), p(t["loss_log"]),
                p(t["cursor"]), self.rows, st), "spo_wide_rows_clip_adam_dev_log")
            out.append(self.snapshot())
        return out

    def fill(self, r, active):
        p, t = (lambda x: x.data_ptr()), self.t
        r.theta, r.adam_m, r.adam_v, r.grad, r.parts = p(t["theta"]), p(t["m"]), p(t["v"]), p(t["grad"]), p(t["parts"])
        r.obs, r.act, r.logp_old = p(self.obs), p(self.act), p(self.logp_old)
        r.target_r, r.target_c, r.adv = p(self.tgt_r), p(self.tgt_c), p(self.adv)
        r.perm, r.cursor_dev, r.pow4_dev = p(self.perm), p(t["cursor"]), p(t["pow4"])
        r.losses3_out, r.scalars4_out, r.partial_ws, r.partial_capacity = p(t["losses3"]), p(t["scal4"]), p(t["partial"]), t["partial"].numel()
        r.loss_log_dev, r.cfg, r.active = p(t["loss_log"]), self.cfg, int(active)


def _bits(x):
    return x.contiguous().view(torch.uint8)


CASES = [
    # obs, act, hidden, rows, S, inactive run
    pytest.param(60, 8, [128, 128], 64, 1, None, id="60x8-128x128-S1"),
    pytest.param(60, 8, [128, 128], 64, 3, None, id="60x8-128x128-S3"),
    pytest.param(60, 8, [128, 128], 64, 9, None, id="60x8-128x128-S9"),
    pytest.param(7, 3, [20, 36], 20, 3, 1, id="7x3-20x36-S3-middle-inactive"),
    pytest.param(72, 2, [32, 32, 32], 16, 2, None, id="72x2-32x32x32-S2"),
    pytest.param(24, 17, [64, 64], 64, 32, None, id="24x17-64x64-S32"),
]


@pytest.mark.parametrize("D,A,hidden,rows,S,inactive", CASES)
def test_batched_step_is_each_runs_standalone_step(lib, D, A, hidden, rows, S, inactive):
    from safepo import _abi
    dev = torch.device("cuda:0")
    # run i clipped (a small max_grad_norm) for even i, unclipped for odd i: both kinds share a launch from S = 2 on
    runs = [_Run(lib, D, A, hidden, rows, 11 + i, 1e-3 if i % 2 == 0 else 1e6, dev) for i in range(S)]
    assert lib.spo_wide_rows_multi_supported(runs[0].net_c, runs[0].net_a, rows, S) == 1
    start = [r.snapshot() for r in runs]
    want = [r.standalone_steps(lib) for r in runs]
    for r, s0 in zip(runs, start):
        r.restore(s0)
    whole_before = None
    if inactive is not None:
        whole_before = {k: v.clone() for k, v in runs[inactive].whole.items()}
    reps = (_abi.WideRowsReplica * S)()
    for i, r in enumerate(runs):
        r.fill(reps[i], i != inactive)
    table = torch.zeros(int(lib.spo_wide_rows_multi_table_bytes(S)), dtype=torch.uint8, device=dev)
    st = _abi.stream_ptr()
    _abi.check(lib.spo_wide_rows_multi_upload(_abi.ptr(table), reps, S, runs[0].net_c, runs[0].net_a, rows, rows, st), "upload")
    got = []
    for _ in range(STEPS):
        _abi.check(lib.spo_wide_rows_step_multi(_abi.ptr(table), S, runs[0].net_c, runs[0].net_a, rows, st), "step_multi")
        got.append([r.snapshot() for r in runs])
    torch.cuda.synchronize(dev)
    for i, r in enumerate(runs):
        if i == inactive:
            continue
        for k in range(STEPS):
            for name in STATE:
                assert torch.equal(_bits(got[k][i][name]), _bits(want[i][k][name])), (i, k, name)
        assert int(got[-1][i]["cursor"].item()) == r.M                          # the last rows of the permutation were in use
        assert not torch.isnan(got[-1][i]["loss_log"]).any()
        coef = float(got[-1][i]["scal4"][0].item())
        assert (coef < 1.0) if i % 2 == 0 else (coef == 1.0), (i, coef)         # clipped and unclipped runs in one launch
    if inactive is not None:
        # an inactive run: nothing of it is read or written -- its buffers, guard bytes included, are what they were
        for k, v in runs[inactive].whole.items():
            assert torch.equal(_bits(v), _bits(whole_before[k])), k
        # ... also with its pointers NULL
        for name, _ in _abi.WideRowsReplica._fields_:
            if name not in ("cfg", "active", "partial_capacity"):
                setattr(reps[inactive], name, None)
        _abi.check(lib.spo_wide_rows_multi_upload(_abi.ptr(table), reps, S, runs[0].net_c, runs[0].net_a, rows, rows, st), "upload")
        for i, r in enumerate(runs):
            r.restore(start[i])
        _abi.check(lib.spo_wide_rows_step_multi(_abi.ptr(table), S, runs[0].net_c, runs[0].net_a, rows, st), "step_multi")
        torch.cuda.synchronize(dev)
        for i, r in enumerate(runs):
            if i != inactive:
                for name in STATE:
                    assert torch.equal(_bits(r.t[name]), _bits(want[i][0][name])), (i, name)


def test_step_can_be_captured_and_upload_cannot(lib):
    """spo_wide_rows_step_multi makes no allocation, copy or host read: a captured graph of it replays the step; the upload is
    refused under capture."""
    from safepo import _abi
    dev = torch.device("cuda:0")
    S, rows = 2, 20
    runs = [_Run(lib, 7, 3, [20, 36], rows, 5 + i, 0.5, dev) for i in range(S)]
    start = [r.snapshot() for r in runs]
    want = [r.standalone_steps(lib) for r in runs]
    for r, s0 in zip(runs, start):
        r.restore(s0)
    reps = (_abi.WideRowsReplica * S)()
    for i, r in enumerate(runs):
        r.fill(reps[i], True)
    table = torch.zeros(int(lib.spo_wide_rows_multi_table_bytes(S)), dtype=torch.uint8, device=dev)
    nc, na = runs[0].net_c, runs[0].net_a
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        _abi.check(lib.spo_wide_rows_multi_upload(_abi.ptr(table), reps, S, nc, na, rows, rows, _abi.stream_ptr()), "upload")
        _abi.check(lib.spo_wide_rows_step_multi(_abi.ptr(table), S, nc, na, rows, _abi.stream_ptr()), "warm-up")   # (sets the LDS limit)
    torch.cuda.synchronize(dev)
    for r, s0 in zip(runs, start):
        r.restore(s0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        rc = lib.spo_wide_rows_multi_upload(_abi.ptr(table), reps, S, nc, na, rows, rows, _abi.stream_ptr())
        msg = lib.spo_last_error().decode()
        _abi.check(lib.spo_wide_rows_step_multi(_abi.ptr(table), S, nc, na, rows, _abi.stream_ptr()), "step_multi")
    assert rc < 0 and "wide_rows_multi_upload" in msg and "capture" in msg
    for _ in range(STEPS):
        g.replay()
    torch.cuda.synchronize(dev)
    for i, r in enumerate(runs):
        for name in STATE:
            assert torch.equal(_bits(r.t[name]), _bits(want[i][-1][name])), (i, name)


# ------------------------------------------------------------------------------------------------ the group against single engines
D_G, A_G, HIDDEN_G = 60, 8, [128, 128]
N_G, T_G = 16, 21                # 336 rows: five whole minibatches of 64 and a ragged one of 16
LAMS = [0.0, 0.3, 1.1]
ITERS = [4, 3, 2]                # learning_iters per run; runs 0 and 1 additionally get a target_kl that stops them early


def _rollout_engine(i, dev, target_kl, learning_iters):
    """Run i: 16 envs x 21 steps of the synthetic device env behind a WidePPOLagEngine at hidden [128, 128], ready for an update."""
    from safepo.common.engine import WidePPOLagEngine
    from safepo.common.env import SynthDeviceEnv
    from safepo.common.model import ActorVCritic
    torch.manual_seed(300 + i)
    pol = ActorVCritic(D_G, A_G, hidden_sizes=HIDDEN_G).to(dev)
    cfg = {"hidden_sizes": HIDDEN_G, "gamma": 0.99, "target_kl": target_kl, "batch_size": 64, "learning_iters": learning_iters,
           "max_grad_norm": 40.0}
    eng = WidePPOLagEngine(pol, N_G, T_G, cfg, dev)
    env = SynthDeviceEnv(N_G, D_G, A_G, seed=7 + i, p_term=0.02, p_cost=0.1, trunc_len=10, device=dev, normalize_obs=True,
                         obs_scale=2.0, obs_shift=0.5)
    rms = env.fuse_normalize(True)
    obs, _ = env.reset()
    eng.rollout_epoch(env, obs, rms=rms)
    eng.drain_episode_events(None)
    g = torch.Generator().manual_seed(900 + i)
    perms = [torch.randperm(N_G * T_G, generator=g).to(torch.int32).to(dev) for _ in range(5)]
    return eng, (lambda it: perms[it])


def _same_bits(x, y):
    return x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def test_group_update_equals_each_engines_update_with_staggered_stops(lib):
    from safepo.common.engine import WidePPOLagEngine
    from safepo.common.engine_group import PPOLagEngineGroup
    dev = torch.device("cuda:0")
    # the unstopped KL after every pass of runs 0 and 1 -> targets that stop run 0 after one pass and run 1 after two
    kls = []
    for i in (0, 1):
        eng, perm_fn = _rollout_engine(i, dev, 1e9, ITERS[i])
        seen, read = [], eng.kl_read
        eng.kl_read = lambda seen=seen, read=read: seen.append(read()) or seen[-1]
        WidePPOLagEngine.update(eng, LAMS[i], perm_fn)
        kls.append(seen)
    assert kls[0][0] > 0 and kls[1][1] > kls[1][0] > 0, kls
    targets = [0.5 * kls[0][0], 0.5 * (kls[1][0] + kls[1][1]), 1e9]
    alone = []
    for i in range(3):
        eng, perm_fn = _rollout_engine(i, dev, targets[i], ITERS[i])
        assert eng.wide.rows_grad_ok(64) and not eng._feature_split_kernel_ok(eng._cfg_struct())
        out = eng.update(LAMS[i], perm_fn)
        alone.append((out, (eng.policy.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone()), eng.adam_step))
    built = [_rollout_engine(i, dev, targets[i], ITERS[i]) for i in range(3)]
    group = PPOLagEngineGroup([e for e, _ in built])
    assert group._rows and group.batched()
    outs = group.update(LAMS, [f for _, f in built])
    stops = [a[0]["stop_iter"] for a in alone]
    print(f"unstopped KLs {kls}, targets {targets[:2]}, stops {stops}")
    assert stops == [1, 2, 2]                                                  # the runs stop at different passes
    for i, ((eng, _), out, (aout, astate, astep)) in enumerate(zip(built, outs, alone)):
        assert set(out) == set(aout)
        for k in ("stop_iter", "kl", "loss_r", "loss_c", "loss_pi"):
            assert out[k] == aout[k], (i, k, out[k], aout[k])
        assert len(out["losses"]) == out["stop_iter"] and all(_same_bits(x, y) for x, y in zip(out["losses"], aout["losses"])), i
        assert eng.adam_step == astep == 6 * out["stop_iter"] and eng.buffer.ptr == 0
        for name, x, y in zip(("theta", "adam_m", "adam_v"), (eng.policy.theta, eng.adam_m, eng.adam_v), astate):
            assert _same_bits(x, y), f"run {i}: {name} differs in {int((x != y).sum())} of {x.numel()} entries"
    assert not torch.equal(alone[0][1][0], alone[1][1][0])
    # with the fused optimiser off the group steps engine by engine -- and says so
    os.environ["SPO_WIDE_ROWS_FUSED"] = "0"
    try:
        assert not group.batched()
    finally:
        del os.environ["SPO_WIDE_ROWS_FUSED"]


# ------------------------------------------------------------------------------------------------ the script against --seed
def _args(log_dir, **kw):
    import argparse
    a = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=N_G, experiment="t", log_dir=str(log_dir), device="cuda",
                           device_id=0, write_terminal=True, headless=False, total_steps=2 * N_G * T_G, steps_per_epoch=N_G * T_G,
                           randomize=False, cost_limit=25.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035,
                           cfg_override={"learning_iters": 3}, env_kwargs={"obs_dim": D_G, "act_dim": A_G, "trunc_len": 16},
                           hidden_sizes=list(HIDDEN_G), batch_wide_rows=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _run_record(log_dir):
    import csv
    rows = list(csv.DictReader(open(os.path.join(log_dir, "progress.csv"))))
    assert len(rows) == 2
    cols = [{k: v for k, v in row.items() if not k.startswith("Time/")} for row in rows]
    return cols, torch.load(os.path.join(log_dir, "torch_save", "model0.pt"))


def test_script_with_seeds_equals_the_seed_runs(lib, tmp_path, capsys):
    from safepo.single_agent import ppo_lag
    seeds = [0, 1, 2]
    alone = []
    for s in seeds:
        d = tmp_path / f"alone_{s}"
        ppo_lag.main(_args(d, seed=s), {})
        alone.append(_run_record(d))
    dirs = [str(tmp_path / f"group_{s}") for s in seeds]
    with pytest.raises(SystemExit, match="wide-network"):                  # without --batch-wide-rows True: today's refusal
        ppo_lag.main(_args(tmp_path / "unused", seeds=list(seeds), log_dirs=dirs), {})
    assert not any(os.path.exists(d) for d in dirs)
    res = ppo_lag.main(_args(tmp_path / "unused", seeds=list(seeds), log_dirs=dirs, batch_wide_rows=True), {})
    assert res["group"]._rows and res["group"].batched() and res["group"]._rows_graphs      # the updates ran as shared launches
    assert list(res["policies"][0].hidden_sizes) == HIDDEN_G
    for d, s, want in zip(dirs, seeds, alone):
        got = _run_record(d)
        assert got[0] == want[0], f"seed {s}: progress.csv differs: " + str(
            [(k, x[k], y[k]) for x, y in zip(got[0], want[0]) for k in x if x[k] != y.get(k)][:6])
        assert set(got[1]) == set(want[1]) and all(torch.equal(got[1][k], want[1][k]) for k in got[1]), f"seed {s}: saved actor differs"
    capsys.readouterr()
    assert alone[0][0] != alone[1][0] and alone[1][0] != alone[2][0]        # (not three copies of one run)
