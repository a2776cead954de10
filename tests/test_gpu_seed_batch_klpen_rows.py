"""GPU tests of the seed-batched row-group step of FOCOPS / CUP (spo_wide_rows_ex_multi_upload + spo_wide_rows_ex_step_multi,
csrc/mlp_rows.hip + csrc/wide.hip; PPOLagEngineGroup(..., klpen_rows=True); --batch-klpen-rows): every run of a batched step is
compared BIT FOR BIT with its own stand-alone five-launch sequence (the gradient launch, the group sum, spo_wide_clip_adam_dev_log's
three) on a copy of the same state, over four consecutive steps that end on the last rows of the permutation.  No tolerance
anywhere: the yardstick is the stand-alone step, which tests/test_gpu_klpen_rows.py holds to the fp64 gate."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
STEPS = 4
GUARD = 64                     # elements of sentinel on either side of a run's buffers
STATE = ("theta", "m", "v", "grad", "pow4", "cursor", "scal4", "loss_log", "losses3")
CLIP, KLPEN = 0, 1             # SPO_ACTOR_LOSS_*
KINDS = {"focops": (KLPEN, 0), "cup2": (KLPEN, 1), "cup1": (CLIP, 0)}      # kind -> (actor_loss, actor_only)


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


def _actor_mean(theta, off_a, dims, x):
    """The actor of the flat parameter vector (W_l [d_{l+1}][d_l] row-major, then b_l; tanh between the layers) on the CPU."""
    off, h = off_a, x
    for l in range(len(dims) - 1):
        K, N = dims[l], dims[l + 1]
        W = theta[off:off + N * K].view(N, K); off += N * K
        b = theta[off:off + N]; off += N
        h = h @ W.t() + b
        if l + 2 < len(dims):
            h = torch.tanh(h)
    return h


class _Run:
    """One run's state and data: random parameters / moments / buffer, its own shuffle, the device clocks of step `t0` (the
    critics') and `t0 + 2` (the actor's), its own learning rates.  The old distribution is the actor BEFORE a perturbation of
    theta, so the rows' KLs to it spread; `kl_med` is the median KL of the first minibatch's rows, computed here on the CPU."""

    def __init__(self, lib, D, A, hidden, rows, seed, max_grad_norm, kind, dev, steps=STEPS):
        from safepo import _abi
        g = torch.Generator().manual_seed(seed)
        self.actor_loss, self.actor_only = KINDS[kind]
        self.net_c, self.net_a = _abi.MlpNet.of([D] + hidden + [1]), _abi.MlpNet.of([D] + hidden + [A])
        Pc, Pa = int(lib.spo_mlp_param_count(self.net_c)), int(lib.spo_mlp_param_count(self.net_a))
        self.Pc, self.P, self.rows, self.M, self.steps = Pc, 2 * Pc + A + Pa, rows, steps * rows, steps
        P, M = self.P, self.M
        f32 = dict(dtype=torch.float32)
        theta = 0.2 * torch.randn(P, generator=g, **f32)
        theta[2 * Pc:2 * Pc + A] = -0.5 + 0.1 * torch.randn(A, generator=g, **f32)          # log_std
        obs = torch.randn(M, D, generator=g, **f32)
        perm = torch.randperm(M, generator=g).to(torch.int64)
        old_mean = _actor_mean(theta, 2 * Pc + A, [D] + hidden + [A], obs)
        old_std = torch.exp(theta[2 * Pc:2 * Pc + A])
        theta = theta + 0.03 * torch.randn(P, generator=g, **f32)                           # the step's theta: away from the old policy
        mu = _actor_mean(theta, 2 * Pc + A, [D] + hidden + [A], obs[perm[:rows]])
        vrat = (torch.exp(theta[2 * Pc:2 * Pc + A]) / old_std) ** 2
        dm = (mu - old_mean[perm[:rows]]) / old_std
        kl_rows = (0.5 * (vrat + dm * dm - 1.0 - torch.log(vrat))).sum(1)
        self.kl_med, self.kl_min = float(kl_rows.median()), float(kl_rows.min())
        self.kl_bound, self.pg_coef = self.kl_med, 1.0 / (1.5 + 0.25 * (seed % 4))
        t0 = 3 + seed % 5
        b1, b2 = 0.9, 0.999
        n_parts = lib.spo_wide_kl_penalty_rows_part_floats(P, 2 * Pc, rows) if self.actor_loss == KLPEN else lib.spo_wide_grad_rows_part_floats(P, rows)
        fills = {
            "theta": theta, "m": 0.01 * torch.randn(P, generator=g, **f32), "v": 1e-4 * torch.rand(P, generator=g, **f32),
            "grad": torch.zeros(P, **f32),
            "pow4": torch.tensor([b1 ** t0, b2 ** t0, b1 ** (t0 + 2), b2 ** (t0 + 2), 3e-4 * (1 + seed % 3), 1e-3 * (1 + seed % 2)],
                                 dtype=torch.float64),
            "cursor": torch.zeros(1, dtype=torch.int64), "scal4": torch.zeros(4, **f32),
            "loss_log": torch.full((steps * 3,), float("nan"), **f32), "losses3": torch.full((3,), 0.25, **f32),
            "parts": torch.zeros(int(n_parts), **f32),
            "partial": torch.zeros(3 * 1024, dtype=torch.float64),
        }
        self.whole, self.t = {}, {}
        for k, v in fills.items():
            self.whole[k], self.t[k] = _guarded(v.numel(), v.dtype, dev, v.to(dev))
        # the group sum's pg_grad / sums: the tail of `parts` behind the row groups (safepo.common.wide.klpen_grad_rows)
        if self.actor_loss == KLPEN:
            tail = self.t["parts"][self.t["parts"].numel() - (P + 3) // 4 * 4 - _abi.KLPEN_SUMS - 4:]
            self.pg_grad, self.sums = tail, tail[(P + 3) // 4 * 4:(P + 3) // 4 * 4 + _abi.KLPEN_SUMS]
        else:
            self.pg_grad = self.sums = torch.zeros(0, device=dev, **f32)
        self.obs, self.perm = obs.to(dev), perm.to(dev)
        self.old_mean, self.old_std = old_mean.contiguous().to(dev), old_std.contiguous().to(dev)
        self.act = (old_mean + 0.6 * torch.randn(M, A, generator=g, **f32)).to(dev)
        self.logp_old = (-0.5 * A + 0.3 * torch.randn(M, generator=g, **f32)).to(dev)
        self.tgt_r, self.tgt_c = torch.randn(M, generator=g, **f32).to(dev), torch.randn(M, generator=g, **f32).to(dev)
        self.adv = torch.randn(M, generator=g, **f32).to(dev)
        self.cfg = _abi.PpoCfg(obs_dim=D, act_dim=A, batch=rows, use_critic_norm=1, use_value_coefficient=seed % 2, clip=0.2,
                               max_grad_norm=max_grad_norm, lr_actor=3e-4, lr_critic=3e-4, beta1=b1, beta2=b2, adam_eps=1e-8, l2_coef=0.001)

    def snapshot(self):
        s = {k: self.t[k].clone() for k in STATE}
        s["sums"] = self.sums.clone()
        return s

    def restore(self, snap):
        for k in STATE:
            self.t[k].copy_(snap[k])
        self.t["parts"].zero_()
        self.t["partial"].zero_()

    def standalone_steps(self, lib):
        """self.steps stand-alone steps from the current state (the launches of WidePPOLagEngine.minibatch_step_ex on the row-group
        kernel with device clocks); the state after each."""
        from safepo import _abi
        p, t, st, out = _abi.ptr, self.t, _abi.stream_ptr(), []
        P, Pc, ao = self.P, self.Pc, self.actor_only
        lo = 2 * Pc if ao else 0
        for _ in range(self.steps):
            if self.actor_loss == KLPEN:
                _abi.check(lib.spo_wide_kl_penalty_grad_rows(
                    p(t["theta"]), self.net_c, self.net_a, p(self.obs), p(self.act), p(self.logp_old), None if ao else p(self.tgt_r),
                    None if ao else p(self.tgt_c), p(self.adv), p(self.old_mean), p(self.old_std), p(self.perm), p(t["cursor"]), self.rows,
                    self.kl_bound, self.pg_coef, ao, p(t["parts"]), st), "spo_wide_kl_penalty_grad_rows")
                _abi.check(lib.spo_wide_kl_penalty_reduce_parts(p(t["parts"]), self.rows, P, 2 * Pc, ao, 1, self.pg_coef, p(t["grad"]),
                                                                p(self.pg_grad), p(self.sums), p(t["losses3"]), st),
                           "spo_wide_kl_penalty_reduce_parts")
            else:
                _abi.check(lib.spo_wide_ppo_grad_rows(p(t["theta"]), self.net_c, self.net_a, p(self.obs), p(self.act), p(self.logp_old),
                                                      p(self.tgt_r), p(self.tgt_c), p(self.adv), p(self.perm), p(t["cursor"]), self.rows,
                                                      float(self.cfg.clip), p(t["parts"]), st), "spo_wide_ppo_grad_rows")
                _abi.check(lib.spo_wide_reduce_parts(p(t["parts"]), self.rows, P, 3, p(t["grad"]), p(t["losses3"]), st), "spo_wide_reduce_parts")
            _abi.check(lib.spo_wide_clip_adam_dev_log(
                p(t["theta"]), p(t["grad"]), p(t["m"]), p(t["v"]), P, Pc, 2 * Pc, 2 * Pc, self.cfg, p(t["pow4"]), lo, P, lo, 0,
                None if ao else p(t["losses3"]), p(t["scal4"]), p(t["partial"]), t["partial"].numel(), p(t["loss_log"]), p(t["losses3"]),
                p(t["cursor"]), self.rows, st), "spo_wide_clip_adam_dev_log")
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
        r.old_mean, r.old_std, r.kl_bound, r.pg_coef = p(self.old_mean), p(self.old_std), self.kl_bound, self.pg_coef


def _bits(x):
    return x.contiguous().view(torch.uint8)


def _make_runs(lib, D, A, hidden, rows, S, kind, dev, steps=STEPS, seed0=11):
    """S runs of one shape.  Run i is unclipped (max_grad_norm 1e6) for odd i and for the last of several runs, else clipped (1e-3);
    kl_bound: run 0 the median KL of its first minibatch's rows, the last of several runs below every row's KL (F = 0), the others
    multiples of their median."""
    runs = []
    for i in range(S):
        last = S > 1 and i == S - 1
        r = _Run(lib, D, A, hidden, rows, seed0 + i, 1e6 if (i % 2 == 1 or last) else 1e-3, kind, dev, steps)
        r.unclipped = i % 2 == 1 or last
        if last:
            r.kl_bound = 0.5 * r.kl_min
        elif i > 0:
            r.kl_bound = r.kl_med * (0.6 + 0.2 * i)
        runs.append(r)
    return runs


CASES = [
    # obs, act, hidden, rows, S, inactive run
    pytest.param(60, 8, [128, 128], 64, 1, None, id="60x8-128x128-S1"),
    pytest.param(60, 8, [128, 128], 64, 3, None, id="60x8-128x128-S3"),
    pytest.param(60, 8, [128, 128], 64, 9, None, id="60x8-128x128-S9"),
    pytest.param(7, 3, [20, 36], 20, 3, 1, id="7x3-20x36-S3-middle-inactive"),
    pytest.param(72, 2, [32, 32, 32], 16, 2, None, id="72x2-32x32x32-S2"),
    pytest.param(24, 17, [64, 64], 64, 32, None, id="24x17-64x64-S32"),
]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("D,A,hidden,rows,S,inactive", CASES)
def test_batched_step_is_each_runs_standalone_step(lib, D, A, hidden, rows, S, inactive, kind):
    from safepo import _abi
    dev = torch.device("cuda:0")
    actor_loss, actor_only = KINDS[kind]
    runs = _make_runs(lib, D, A, hidden, rows, S, kind, dev)
    nc, na = runs[0].net_c, runs[0].net_a
    assert lib.spo_wide_rows_ex_multi_supported(nc, na, rows, actor_loss, actor_only, S) == 1
    start = [r.snapshot() for r in runs]
    want = [r.standalone_steps(lib) for r in runs]
    torch.cuda.synchronize(dev)
    # ---- what the stand-alone steps alone must show, or the comparison below proves nothing about these branches
    live = [i for i in range(S) if i != inactive]
    for i in live:
        coef = float(want[i][-1]["scal4"][0].item())
        if not (actor_only and S > 1 and i == S - 1):        # (CUP's second stage with F = 0 and no KL yet: a zero gradient)
            assert (coef == 1.0) if runs[i].unclipped else (coef < 1.0), (i, coef)
    if S > 1:
        assert any(runs[i].unclipped for i in live) and any(not runs[i].unclipped for i in live)   # both kinds share a launch
    if kind == "focops":
        cnt0 = float(want[0][0]["sums"][2].item())
        print(f"{kind}: run 0 kl_bound {runs[0].kl_bound:.5g} (median), {cnt0:.0f} of {rows} rows inside")
        assert rows / 4 <= cnt0 <= 3 * rows / 4, cnt0                       # 0 < F < 1: the combine g_KL + F g_PG is exercised
        if S > 1:
            assert float(want[S - 1][0]["sums"][2].item()) == 0.0           # F = 0: a kl_bound below every row's KL
    assert len({(r.kl_bound, r.pg_coef) for r in runs}) == S
    assert all(float(r.t["pow4"][0].item()) != float(r.t["pow4"][2].item()) for r in runs)   # critics' and actor's clocks differ
    for r, s0 in zip(runs, start):
        r.restore(s0)
    whole_before = None
    if inactive is not None:
        whole_before = {k: v.clone() for k, v in runs[inactive].whole.items()}
    reps = (_abi.WideRowsExReplica * S)()
    for i, r in enumerate(runs):
        r.fill(reps[i], i != inactive)
    table = torch.zeros(int(lib.spo_wide_rows_ex_multi_table_bytes(S)), dtype=torch.uint8, device=dev)
    st = _abi.stream_ptr()
    _abi.check(lib.spo_wide_rows_ex_multi_upload(_abi.ptr(table), reps, S, nc, na, rows, rows, actor_loss, actor_only, st), "upload")
    got = []
    for _ in range(STEPS):
        _abi.check(lib.spo_wide_rows_ex_step_multi(_abi.ptr(table), S, nc, na, rows, actor_loss, actor_only, st), "step_multi")
        got.append([r.snapshot() for r in runs])
    torch.cuda.synchronize(dev)
    names = STATE + (("sums",) if actor_loss == KLPEN else ())
    for i in live:
        r = runs[i]
        for k in range(STEPS):
            for name in names:
                assert torch.equal(_bits(got[k][i][name]), _bits(want[i][k][name])), (i, k, name)
        assert int(got[-1][i]["cursor"].item()) == r.M                          # the last rows of the permutation were in use
        assert not torch.isnan(got[-1][i]["loss_log"].view(STEPS, 3)[:, 2]).any()
        if actor_only:
            # the critics' parameters, moments and clocks are what they were before the launch
            c_end = 2 * r.Pc
            for name in ("theta", "m", "v"):
                assert torch.equal(_bits(got[-1][i][name][:c_end]), _bits(start[i][name][:c_end])), (i, name)
                assert not torch.equal(_bits(got[-1][i][name][c_end:]), _bits(start[i][name][c_end:])), (i, name)
            assert torch.equal(_bits(got[-1][i]["pow4"][:2]), _bits(start[i]["pow4"][:2]))
            assert not torch.equal(_bits(got[-1][i]["pow4"][2:4]), _bits(start[i]["pow4"][2:4]))
    if inactive is not None:
        # an inactive run: nothing of it is read or written -- its buffers, guard bytes included, are what they were
        for k, v in runs[inactive].whole.items():
            assert torch.equal(_bits(v), _bits(whole_before[k])), k
        # ... also with its pointers NULL
        for name, _ in _abi.WideRowsExReplica._fields_:
            if name not in ("cfg", "active", "partial_capacity", "kl_bound", "pg_coef"):
                setattr(reps[inactive], name, None)
        _abi.check(lib.spo_wide_rows_ex_multi_upload(_abi.ptr(table), reps, S, nc, na, rows, rows, actor_loss, actor_only, st), "upload")
        for i, r in enumerate(runs):
            r.restore(start[i])
        _abi.check(lib.spo_wide_rows_ex_step_multi(_abi.ptr(table), S, nc, na, rows, actor_loss, actor_only, st), "step_multi")
        torch.cuda.synchronize(dev)
        for i in live:
            for name in STATE:
                assert torch.equal(_bits(runs[i].t[name]), _bits(want[i][0][name])), (i, name)
    # the guard elements around every taking-part run's buffers are intact too
    for i in live:
        for k, v in runs[i].whole.items():
            assert bool((v[:GUARD] == -77).all()) and bool((v[-GUARD:] == -77).all()), (i, k)


@pytest.mark.parametrize("kind", list(KINDS))
def test_step_can_be_captured_and_upload_cannot(lib, kind):
    """spo_wide_rows_ex_step_multi makes no allocation, copy or host read: eight steps captured into ONE graph are eight eager
    stand-alone steps; the upload is refused under capture."""
    from safepo import _abi
    dev = torch.device("cuda:0")
    S, rows, n = 2, 20, 8
    actor_loss, actor_only = KINDS[kind]
    runs = _make_runs(lib, 7, 3, [20, 36], rows, S, kind, dev, steps=n, seed0=5)
    start = [r.snapshot() for r in runs]
    want = [r.standalone_steps(lib) for r in runs]
    for r, s0 in zip(runs, start):
        r.restore(s0)
    reps = (_abi.WideRowsExReplica * S)()
    for i, r in enumerate(runs):
        r.fill(reps[i], True)
    table = torch.zeros(int(lib.spo_wide_rows_ex_multi_table_bytes(S)), dtype=torch.uint8, device=dev)
    nc, na = runs[0].net_c, runs[0].net_a
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        _abi.check(lib.spo_wide_rows_ex_multi_upload(_abi.ptr(table), reps, S, nc, na, rows, rows, actor_loss, actor_only, _abi.stream_ptr()),
                   "upload")
        _abi.check(lib.spo_wide_rows_ex_step_multi(_abi.ptr(table), S, nc, na, rows, actor_loss, actor_only, _abi.stream_ptr()),
                   "warm-up")                                                  # (sets the LDS limit)
    torch.cuda.synchronize(dev)
    for r, s0 in zip(runs, start):
        r.restore(s0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        rc = lib.spo_wide_rows_ex_multi_upload(_abi.ptr(table), reps, S, nc, na, rows, rows, actor_loss, actor_only, _abi.stream_ptr())
        msg = lib.spo_last_error().decode()
        for _ in range(n):
            _abi.check(lib.spo_wide_rows_ex_step_multi(_abi.ptr(table), S, nc, na, rows, actor_loss, actor_only, _abi.stream_ptr()),
                       "step_multi")
    assert rc < 0 and "wide_rows_ex_multi_upload" in msg and "capture" in msg
    g.replay()
    torch.cuda.synchronize(dev)
    for i, r in enumerate(runs):
        for name in STATE:
            assert torch.equal(_bits(r.t[name]), _bits(want[i][-1][name])), (i, name)
        assert int(r.t["cursor"].item()) == r.M


# ------------------------------------------------------------------------------------------------ the group against single engines
D_G, A_G, HIDDEN_G = 60, 8, [128, 128]
N_G, T_G = 16, 21                # 336 rows: five whole minibatches of 64 and a ragged one of 16
LAMS = [0.0, 0.3, 1.1]
ITERS = [4, 3, 2]                # learning_iters per run; runs 0 and 1 additionally get a target_kl taken from a probe's KLs


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
    perms = [torch.randperm(N_G * T_G, generator=g).to(torch.int32).to(dev) for _ in range(10)]
    return eng, (lambda it: perms[it])


def _same_bits(x, y):
    return x.shape == y.shape and torch.equal(_bits(x), _bits(y))


def _same_out(out, aout, i):
    assert set(out) == set(aout)
    for k, v in aout.items():
        if k in ("losses", "second_stage_losses"):
            assert len(out[k]) == len(v) and all(_same_bits(x, y) for x, y in zip(out[k], v)), (i, k)
        else:
            assert out[k] == v or (out[k] != out[k] and v != v), (i, k, out[k], v)


@pytest.mark.parametrize("algo", ["focops", "cup"])
def test_group_update_equals_each_engines_update_with_staggered_stops(lib, algo):
    from safepo.common.engine_group import PPOLagEngineGroup
    dev = torch.device("cuda:0")
    upd = "update_" + algo
    # target_kl (FOCOPS: also every row's kl_bound) per run: run 1's lies between the KLs its unstopped update reads after its first
    # and its second pass, run 0's below the first; run 2 is stopped by its learning_iters alone.  (Under FOCOPS the bound shapes the
    # trajectory itself, so only CUP's first stage -- the clipped surrogate -- is certain to stop run 1 where the probe says.)
    eng, perm_fn = _rollout_engine(1, dev, 1e9, ITERS[1])
    seen, read = [], eng.kl_to_old
    eng.kl_to_old = lambda: seen.append(read()) or seen[-1]
    getattr(eng, upd)(LAMS[1], perm_fn)
    assert seen[1] > seen[0] > 0, seen
    targets = [0.3 * seen[0], 0.5 * (seen[0] + seen[1]), 1e9]
    alone = []
    for i in range(3):
        eng, perm_fn = _rollout_engine(i, dev, targets[i], ITERS[i])
        assert eng._row_group_step_ok(64, KLPEN, algo == "cup") and not eng._feature_split_kernel_ok(eng._cfg_struct())
        out = getattr(eng, upd)(LAMS[i], perm_fn)
        alone.append((out, (eng.policy.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone()), (eng.adam_step, eng.adam_step_actor_extra)))
    stops = [a[0]["stop_iter"] for a in alone]
    print(f"{algo}: run 1's unstopped KLs {seen}, targets {targets}, stops {stops}, "
          f"second stage {[a[0].get('second_stage_stop_iter') for a in alone]}")
    assert stops[2] == 2 and len(set(stops)) >= 2 and (algo != "cup" or stops[1] == 2)       # the runs stop at different passes
    for keyword in (True, False):
        built = [_rollout_engine(i, dev, targets[i], ITERS[i]) for i in range(3)]
        group = PPOLagEngineGroup([e for e, _ in built], klpen_rows=True) if keyword else PPOLagEngineGroup([e for e, _ in built])
        assert group._rows
        assert group.batched_ex(KLPEN) == keyword and group.batched_ex(CLIP) == keyword and group.batched_ex(KLPEN, None, True) == keyword
        assert not group.batched_ex(CLIP, None, True)                          # (no actor-only step with the clipped surrogate)
        outs = getattr(group, upd)(LAMS, [f for _, f in built])
        kinds = {k[2:] for k in group._rows_graphs if isinstance(k, tuple) and k[0] == "ex"} if keyword else set()
        assert kinds == ({(KLPEN, False)} if algo == "focops" else {(CLIP, False), (KLPEN, True)}) if keyword else not group._rows_graphs
        for i, ((eng, _), out, (aout, astate, asteps)) in enumerate(zip(built, outs, alone)):
            _same_out(out, aout, i)
            assert (eng.adam_step, eng.adam_step_actor_extra) == asteps and eng.adam_step == 6 * out["stop_iter"] and eng.buffer.ptr == 0
            if algo == "cup":
                assert eng.adam_step_actor_extra == 6 * out["second_stage_stop_iter"]
            for name, x, y in zip(("theta", "adam_m", "adam_v"), (eng.policy.theta, eng.adam_m, eng.adam_v), astate):
                assert _same_bits(x, y), f"klpen_rows={keyword}, run {i}: {name} differs in {int((x != y).sum())} of {x.numel()} entries"
    assert not torch.equal(alone[0][1][0], alone[1][1][0])


# ------------------------------------------------------------------------------------------------ the script against --seed
def _args(log_dir, **kw):
    import argparse
    a = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=N_G, experiment="t", log_dir=str(log_dir), device="cuda",
                           device_id=0, write_terminal=True, headless=False, total_steps=2 * N_G * T_G, steps_per_epoch=N_G * T_G,
                           randomize=False, cost_limit=25.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035,
                           cfg_override={"learning_iters": 3}, env_kwargs={"obs_dim": D_G, "act_dim": A_G, "trunc_len": 16},
                           hidden_sizes=list(HIDDEN_G), batch_wide_rows=False, batch_update=False, batch_klpen_rows=False)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _run_record(log_dir):
    import csv
    rows = list(csv.DictReader(open(os.path.join(log_dir, "progress.csv"))))
    assert len(rows) == 2
    cols = [{k: v for k, v in row.items() if not k.startswith("Time/")} for row in rows]
    return cols, torch.load(os.path.join(log_dir, "torch_save", "model0.pt"))


@pytest.mark.parametrize("algo", ["focops", "cup"])
def test_script_with_seeds_equals_the_seed_runs(lib, tmp_path, capsys, algo):
    import importlib
    mod = importlib.import_module("safepo.single_agent." + algo)
    seeds = [0, 1, 2]
    alone = []
    for s in seeds:
        d = tmp_path / f"alone_{s}"
        mod.main(_args(d, seed=s), {})
        alone.append(_run_record(d))
    dirs = [str(tmp_path / f"group_{s}") for s in seeds]
    with pytest.raises(SystemExit, match="wide-network"):                  # without --batch-klpen-rows True: today's refusal
        mod.main(_args(tmp_path / "unused", seeds=list(seeds), log_dirs=dirs, batch_update=True), {})
    assert not any(os.path.exists(d) for d in dirs)
    res = mod.main(_args(tmp_path / "unused", seeds=list(seeds), log_dirs=dirs, batch_update=True, batch_klpen_rows=True), {})
    group = res["group"]
    assert group._rows and group._klpen_rows and group.batched_ex(KLPEN, None, algo == "cup")
    assert any(isinstance(k, tuple) and k[0] == "ex" for k in group._rows_graphs)                    # the updates ran as shared launches
    assert list(res["policies"][0].hidden_sizes) == HIDDEN_G
    for d, s, want in zip(dirs, seeds, alone):
        got = _run_record(d)
        assert got[0] == want[0], f"seed {s}: progress.csv differs: " + str(
            [(k, x[k], y[k]) for x, y in zip(got[0], want[0]) for k in x if x[k] != y.get(k)][:6])
        assert set(got[1]) == set(want[1]) and all(torch.equal(got[1][k], want[1][k]) for k in got[1]), f"seed {s}: saved actor differs"
    capsys.readouterr()
    assert alone[0][0] != alone[1][0] and alone[1][0] != alone[2][0]        # (not three copies of one run)
