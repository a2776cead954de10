"""GPU parity tests (run with -m gpu on an MI355X): HIP path, through the C ABI, against
(a) golden fixtures produced by the unmodified reference and (b) the CPU oracle on seeded inputs.

Tolerances (north_star): segment masks / indices bit-exact; fp32 losses, gradients and parameters
within 1e-5 relative (absolute floors stated per test); GAE values: bit-pattern equal to the
sequential fp64 reference except where the re-associated fp64 scan lands within 1e-16 of an fp32
rounding boundary (<= 1 ulp, expected frequency ~1e-8 per element)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_gate as G  # noqa: E402
from oracle import restatement as R  # noqa: E402  (checker only)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _ulp_diff(a, b):
    ai = a.view(np.int32).astype(np.int64)
    bi = b.view(np.int32).astype(np.int64)
    ai = np.where(ai < 0, -(ai & 0x7FFFFFFF), ai)
    bi = np.where(bi < 0, -(bi & 0x7FFFFFFF), bi)
    return np.abs(ai - bi)


def _assert_params_close(got, ref, lr, nsteps, rtol=2e-4, atol=2e-6, what=""):
    """TRAJECTORY check of the free-running multi-epoch replays only (round 5: every other caller moved to the fp64 yardstick,
    tests/envelope.py, and each of these replays has a yardstick test beside it --
    test_second_order_family_traces_under_the_fp64_yardstick).  Parameters after Adam steps over several epochs of a
    free-running HIP state against the reference's recorded state: Adam divides by sqrt(v), so an element whose gradient
    is at rounding-noise level gets an O(lr) step of arbitrary sign on BOTH sides -- at most 0.1 % of the elements may leave
    the rtol / atol band, and none by more than the distance Adam can move an element (2 x lr x nsteps)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    bad = err > (atol + rtol * np.abs(ref))
    assert bad.mean() <= 1e-3, f"{what}: {bad.sum()}/{bad.size} parameters outside rtol={rtol}, atol={atol}"
    assert err.max() <= 2.0 * lr * nsteps, f"{what}: max |diff| {err.max():.3e} exceeds 2*lr*steps"


def _fill_update_problem(eng, problem):
    """Loads (obs, act, logp, tgt_r, tgt_c, adv) rows into the engine's dense buffer as one env of M steps."""
    obs, act, logp, tgt_r, tgt_c, adv = problem
    M, D, A = obs.shape[0], obs.shape[1], act.shape[1]
    b = eng.buffer
    b.data["obs"].view(-1, D).copy_(obs); b.data["act"].view(-1, A).copy_(act)
    b.data["log_prob"].view(-1).copy_(logp); b.data["target_value_r"].view(-1).copy_(tgt_r)
    b.data["target_value_c"].view(-1).copy_(tgt_c); b.adv_mix.view(-1).copy_(adv)


def _hip_prefix_runs(eng, pol, theta0, perm_dev, batch, ks):
    """HIP trajectory at checkpoints: for each k, restart from theta0 / zero Adam state and run the first k minibatch
    steps of the shuffle in ONE persistent launch.  Returns {k: (theta float64, losses [k,3])}."""
    full, out = eng.M, {}
    for k in ks:
        pol.theta.copy_(theta0); eng.adam_m.zero_(); eng.adam_v.zero_(); eng.adam_step = 0
        eng.M = k * batch
        losses = eng.learning_iter(perm_dev[:k * batch].contiguous())
        eng.check_sync_error()
        out[k] = (pol.theta.detach().cpu().numpy().astype(np.float64), losses.cpu().numpy().astype(np.float64))
    eng.M = full
    return out


def _assert_trajectory_in_envelope(hip_runs, problem, sd0, perm, batch, ks, what, c=3.0, **oracle_kw):
    """The drift-envelope gate (tests/envelope.py): the HIP losses of every step and the HIP parameters at the checkpoints
    `ks` may be no further from the oracle's float64 trajectory than c x the distance of the reference fp32 arithmetic
    (the oracle in float32) from it; the first 8 steps additionally agree with the fp32 oracle to north_star's 1e-5."""
    import envelope as E
    kmax = max(ks)
    l32, t32 = E.oracle_trajectory(sd0, problem, perm, batch, kmax, torch.float32, ks, **oracle_kw)
    l64, t64 = E.oracle_trajectory(sd0, problem, perm, batch, kmax, torch.float64, ks, **oracle_kw)
    lh = hip_runs[kmax][1]
    np.testing.assert_allclose(lh[:8], l32[:8], rtol=1e-5, atol=1e-6, err_msg=f"{what}: first 8 steps")
    report = {"loss": E.assert_loss_envelope(lh, l32, l64, what, c=c)}
    for k in ks:
        # a shorter launch is a prefix of the longer one: same per-step losses, bit for bit
        assert np.array_equal(hip_runs[k][1], lh[:k]), f"{what}: the {k}-step launch is not a prefix of the {kmax}-step launch"
        report[k] = E.assert_theta_envelope(hip_runs[k][0], t32[k], t64[k], f"{what}: theta after {k} steps", c=c)
    return report


def _run_gae(dev, reward, cost, v_r, v_c, seg, boot_r, boot_c, gamma=0.99, lam=0.95, lam_c=0.95):
    from safepo.common.buffer import VectorizedOnPolicyBuffer
    from safepo.common.engine import _Space
    N, T = reward.shape
    buf = VectorizedOnPolicyBuffer(_Space(3), _Space(2), size=T, num_envs=N, device=dev, gamma=gamma, lam=lam, lam_c=lam_c)
    put = lambda k, v: buf.data[k].copy_(torch.from_numpy(np.ascontiguousarray(v)))
    put("reward", reward); put("cost", cost); put("value_r", v_r); put("value_c", v_c)
    buf.seg_end.copy_(torch.from_numpy(np.ascontiguousarray(seg.astype(np.uint8))))
    buf.boot_r.copy_(torch.from_numpy(boot_r)); buf.boot_c.copy_(torch.from_numpy(boot_c))
    return buf


def _raw_gae(buf):
    """Launch only the scan (no standardisation) and return host arrays."""
    from safepo import _abi
    d = buf.data
    _abi.check(buf._lib.spo_gae_fused(
        _abi.ptr(d["reward"]), _abi.ptr(d["cost"]), _abi.ptr(d["value_r"]), _abi.ptr(d["value_c"]),
        _abi.ptr(buf.seg_end), _abi.ptr(buf.boot_r), _abi.ptr(buf.boot_c), _abi.ptr(d["adv_r"]), _abi.ptr(d["adv_c"]),
        _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(buf._partials), buf.num_envs, buf.size,
        buf._gamma, buf._lam, buf._lam_c, _abi.stream_ptr()), "gae")
    torch.cuda.synchronize()
    return tuple(d[k].cpu().numpy() for k in ("adv_r", "adv_c", "target_value_r", "target_value_c"))


def _assert_gae_close(got, ref, what):
    for g, r, name in zip(got, ref, ("adv_r", "adv_c", "tgt_r", "tgt_c")):
        ulp = _ulp_diff(np.ascontiguousarray(g), np.ascontiguousarray(r))
        bad = int((ulp > 0).sum())
        assert ulp.max() <= 1, f"{what}/{name}: max ulp diff {ulp.max()}"
        assert bad <= max(1, int(1e-5 * g.size)), f"{what}/{name}: {bad}/{g.size} elements differ by 1 ulp"
        np.testing.assert_allclose(g, r, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("tag", ["a", "b", "c", "d"])
def test_gae_golden_reference_buffer(dev, golden_dir, tag):
    z = np.load(os.path.join(golden_dir, "gae.npz"))
    i = lambda k: z[f"{tag}_in_{k}"]
    buf = _run_gae(dev, i("reward"), i("cost"), i("value_r"), i("value_c"), i("seg_end"), i("boot_r"), i("boot_c"))
    got = _raw_gae(buf)
    ref = tuple(z[f"{tag}_raw_{k}"] for k in ("adv_r", "adv_c", "target_value_r", "target_value_c"))
    _assert_gae_close(got, ref, f"golden {tag}")
    if tag != "d":
        data = buf.get(lagrangian_multiplier=0.25)
        np.testing.assert_allclose(data["adv_r"].cpu().numpy(), z[f"{tag}_get_adv_r"], rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(data["adv_c"].cpu().numpy(), z[f"{tag}_get_adv_c"], rtol=1e-5, atol=2e-6)
        mix = R.adv_mix(torch.from_numpy(z[f"{tag}_get_adv_r"]), torch.from_numpy(z[f"{tag}_get_adv_c"]), 0.25)
        np.testing.assert_allclose(data["advantage"].cpu().numpy(), mix.numpy(), rtol=1e-5, atol=2e-6)


def _random_case(N, T, p_seg, seed, finish_last=True):
    rng = np.random.default_rng(seed)
    reward = rng.standard_normal((N, T)).astype(np.float32)
    cost = (rng.random((N, T)) < 0.1).astype(np.float32)
    v_r = rng.standard_normal((N, T)).astype(np.float32)
    v_c = rng.standard_normal((N, T)).astype(np.float32)
    seg = rng.random((N, T)) < p_seg
    if finish_last:
        seg[:, T - 1] = True
    term = seg & (rng.random((N, T)) < 0.3)
    boot_r = np.where(seg & ~term, rng.standard_normal((N, T)), 0).astype(np.float32)
    boot_c = np.where(seg & ~term, rng.standard_normal((N, T)), 0).astype(np.float32)
    return reward, cost, v_r, v_c, seg, boot_r, boot_c


@pytest.mark.parametrize("N,T,p", [(257, 128, 1 / 64), (33, 1000, 1 / 100), (10, 2000, 1 / 500), (65, 77, 0.05),
                                   (7, 300, 0.0), (1, 4, 0.5), (130, 16, 0.2), (5, 129, 0.01), (4096, 128, 1 / 64)])
def test_gae_vs_oracle_random(dev, N, T, p):
    case = _random_case(N, T, p, seed=N * 1000 + T)
    buf = _run_gae(dev, *case)
    got = _raw_gae(buf)
    ref = R.gae_dense(*case, 0.99, 0.95, 0.95)
    _assert_gae_close(got, ref, f"N={N},T={T}")


def _raw_gae_folded(buf, gamma=0.99):
    """The folded form of the scan: reward / cost carry fl(r + fl(gamma32 * bootstrap)) at path ends (what
    spo_boundary_step_fold writes), no bootstrap arrays."""
    from safepo import _abi
    d = buf.data
    g32 = np.float32(gamma)
    seg = buf.seg_end.cpu().numpy().astype(bool)
    fold = {}
    for k, bk in (("reward", buf.boot_r), ("cost", buf.boot_c)):
        r, bt = d[k].cpu().numpy(), bk.cpu().numpy()
        fold[k] = torch.from_numpy(np.where(seg, (r + (g32 * bt).astype(np.float32)).astype(np.float32), r)).to(d[k].device)
    _abi.check(buf._lib.spo_gae_fused(
        _abi.ptr(fold["reward"]), _abi.ptr(fold["cost"]), _abi.ptr(d["value_r"]), _abi.ptr(d["value_c"]),
        _abi.ptr(buf.seg_end), None, None, _abi.ptr(d["adv_r"]), _abi.ptr(d["adv_c"]),
        _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(buf._partials), buf.num_envs, buf.size,
        buf._gamma, buf._lam, buf._lam_c, _abi.stream_ptr()), "gae folded")
    torch.cuda.synchronize()
    return tuple(d[k].cpu().numpy() for k in ("adv_r", "adv_c", "target_value_r", "target_value_c"))


@pytest.mark.parametrize("N,T,p", [(257, 128, 1 / 64), (33, 1000, 1 / 100), (65, 77, 0.05), (1, 4, 0.5), (130, 16, 0.2),
                                   (4096, 128, 1 / 64), (40000, 128, 1 / 64)])
def test_gae_folded_form_is_bit_identical(dev, N, T, p):
    """The layout the engine / bench use -- gamma * bootstrap folded into the reward at the boundary step, no bootstrap
    arrays -- against the plain form on the same inputs: every output bit; and the timed entry point runs the same scan."""
    case = _random_case(N, T, p, seed=N + 7 * T)
    buf = _run_gae(dev, *case)
    base = _raw_gae(buf)
    folded = _raw_gae_folded(buf)
    for b, f in zip(base, folded):
        assert np.array_equal(b.view(np.uint32), f.view(np.uint32))
    if N * T <= 600000:
        _assert_gae_close(base, R.gae_dense(*case, 0.99, 0.95, 0.95), f"N={N},T={T}")
    buf.ptr = T
    buf.compute_gae(None)
    durs = buf.time_scan_dispatches(5)
    assert len(durs) == 5 and all(0.0 < d < 1e-2 for d in durs), durs


def test_gae_fed_by_the_boundary_kernels_own_fold_full_size(dev):
    """the scan fed with the fold arrays spo_boundary_step_fold ITSELF wrote (not a numpy-built fold) at
    the headline size, random terminations / time-outs / final observations on every step: seg_end bit-equal to the
    oracle's boundary logic, all four outputs bit-pattern-equal (<= 1 ulp on <= 1e-5 of the elements, the re-associated
    fp64 carry) to the sequential reference scan on the device-held inputs, and the unfolded form on the same epoch
    bit-identical to the folded one.  Then the API path on top of an engine-collected epoch: a
    reference-style finish_path() and an in-place reward edit must both reach the scan."""
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    N, T, D, A = 4096, 128, 60, 8
    torch.manual_seed(3)
    pol = ActorVCritic(D, A).to(dev)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 0.02, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 40.0}
    eng = PPOLagEngine(pol, N, T, cfg, dev)
    g = torch.Generator(device=dev).manual_seed(11)
    rnd = lambda *sh: torch.randn(*sh, generator=g, device=dev)
    uni = lambda *sh: torch.rand(*sh, generator=g, device=dev)
    b = eng.buffer
    b.data["value_r"].copy_(rnd(N, T)); b.data["value_c"].copy_(rnd(N, T))
    segs, boots_r, boots_c = [], [], []
    for t in range(T):
        nobs, fobs = rnd(N, D), rnd(N, D)
        rew, cost = rnd(N), (uni(N) < 0.1).float()
        term, trunc = (uni(N) < 1 / 96).float(), (uni(N) < 1 / 64).float()
        eng.post_step(t, nobs, rew, cost, term, trunc, fobs)
        if t in (0, 63, T - 1):             # the oracle's boundary logic on the values the device used (spot-checked steps)
            vn = (eng.vnext_r.cpu().numpy(), eng.vnext_c.cpu().numpy()) if t == T - 1 else (np.zeros(N, np.float32),) * 2
            sg, br, bc = R.boundary_step(term.cpu().numpy(), trunc.cpu().numpy(), t == T - 1, vn[0], vn[1],
                                         eng.vfinal_r.cpu().numpy(), eng.vfinal_c.cpu().numpy())
            assert np.array_equal(b.seg_end[:, t].cpu().numpy(), np.asarray(sg).astype(np.uint8))
            assert np.array_equal(b.boot_r[:, t].cpu().numpy(), np.asarray(br, np.float32))
            assert np.array_equal(b.boot_c[:, t].cpu().numpy(), np.asarray(bc, np.float32))
    assert b._fold_cols == T and b.ptr == T
    host = lambda x: x.cpu().numpy()
    inp = [host(b.data[k]) for k in ("reward", "cost", "value_r", "value_c")] + [host(b.seg_end).astype(bool), host(b.boot_r), host(b.boot_c)]
    assert inp[4][:, -1].all() and 0.01 < inp[4].mean() < 0.05
    # the fold the kernel wrote == the reference's first two roundings, bit for bit
    g32 = np.float32(0.99)
    for fold, r, bt in ((b.reward_fold, inp[0], inp[5]), (b.cost_fold, inp[1], inp[6])):
        want = np.where(inp[4], (r + (g32 * bt).astype(np.float32)).astype(np.float32), r)
        assert np.array_equal(host(fold).view(np.uint32), want.view(np.uint32))
    ref = R.gae_dense(*inp, 0.99, 0.95, 0.95)
    from safepo import _abi
    d = b.data
    outs = ("adv_r", "adv_c", "target_value_r", "target_value_c")
    def scan(rew, cst, br, bc):
        _abi.check(b._lib.spo_gae_fused(_abi.ptr(rew), _abi.ptr(cst), _abi.ptr(d["value_r"]), _abi.ptr(d["value_c"]), _abi.ptr(b.seg_end),
                                        _abi.ptr(br), _abi.ptr(bc), *[_abi.ptr(d[k]) for k in outs], _abi.ptr(b._partials), N, T,
                                        0.99, 0.95, 0.95, _abi.stream_ptr()), "gae")
        torch.cuda.synchronize()
        return tuple(host(d[k]).copy() for k in outs)
    folded = scan(b.reward_fold, b.cost_fold, None, None)
    _assert_gae_close(folded, ref, "boundary kernel's fold -> scan, 4096x128")
    plain = scan(d["reward"], d["cost"], b.boot_r, b.boot_c)
    for f, u in zip(folded, plain):
        assert np.array_equal(f.view(np.uint32), u.view(np.uint32))
    # engine entry: compute_gae picks the folded form; targets are untouched by the standardisation
    b.compute_gae(None)
    assert b.last_scan_folded
    assert np.array_equal(host(d["target_value_c"]).view(np.uint32), folded[3].view(np.uint32))
    # API calls on top of the engine-collected epoch: a new bootstrap value through finish_path ...
    b.path_start_idx_list = [0] * N
    b.finish_path(torch.tensor([1.5]), torch.tensor([-0.25]), idx=7)
    b.compute_gae(None)
    assert not b.last_scan_folded, "finish_path() must invalidate the folded arrays"
    inp2 = [x.copy() for x in inp]
    inp2[5][7, T - 1], inp2[6][7, T - 1] = 1.5, -0.25
    ref2 = R.gae_dense(*[x[7:8] for x in inp2], 0.99, 0.95, 0.95)
    assert np.array_equal(host(d["target_value_r"])[7:8].view(np.uint32), ref2[2].view(np.uint32)) or \
        _ulp_diff(host(d["target_value_r"])[7:8], ref2[2]).max() <= 1
    assert abs(host(d["target_value_r"])[7, T - 1] - folded[2][7, T - 1]) > 1e-3       # the new bootstrap really arrived
    # ... and an in-place reward edit (reward shaping) with force_unfolded
    eng2_fold = b._fold_cols
    b._fold_cols = T                                # as if the epoch were still folded
    d["reward"][5].add_(1.0)
    b.compute_gae(None, force_unfolded=True)
    inp3 = [x.copy() for x in inp2]
    inp3[0][5] += np.float32(1.0)
    ref3 = R.gae_dense(*[x[5:6] for x in inp3], 0.99, 0.95, 0.95)
    assert _ulp_diff(host(d["target_value_r"])[5:6], ref3[2]).max() <= 1


@pytest.mark.parametrize("N,T", [(4096, 6), (1000, 5), (70, 4), (257, 3)])
def test_boundary_step_on_many_workgroups_equals_the_one_block_kernel(dev, N, T):
    """spo_boundary_step_fold_mb (num_envs / 256 workgroups, running event count in a per-step prefix array) against the
    one-block spo_boundary_step_fold on the same random steps: buffers, masks, bootstrap and fold arrays, episode accumulators
    and the EVENT LOG (env order within a step, the order of the reference's Python loop ppo_lag.py:199-230) bit-identical."""
    from safepo import _abi
    lib = _abi.load()
    g = torch.Generator(device=dev).manual_seed(N + T)
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)

    def state():
        return {"reward": torch.zeros((N, T), **f32), "cost": torch.zeros((N, T), **f32), "seg": torch.zeros((N, T), dtype=torch.uint8, device=dev),
                "boot_r": torch.zeros((N, T), **f32), "boot_c": torch.zeros((N, T), **f32), "fold_r": torch.zeros((N, T), **f32),
                "fold_c": torch.zeros((N, T), **f32), "ret": torch.zeros(N, **f64), "ecost": torch.zeros(N, **f64), "len": torch.zeros(N, **f64),
                "events": torch.zeros((N * T, 4), **f64)}
    A, B = state(), state()
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    prefix = torch.zeros(T + 1, dtype=torch.int32, device=dev)
    for t in range(T):
        rew, cost = torch.randn(N, generator=g, **f32), (torch.rand(N, generator=g, **f32) < 0.2).float()
        term, trunc = (torch.rand(N, generator=g, **f32) < 0.1).float(), (torch.rand(N, generator=g, **f32) < 0.15).float()
        vals = [torch.randn(N, generator=g, **f32) for _ in range(4)]
        common = [rew, cost, term, trunc] + vals
        for S, fn, cnt in ((A, lib.spo_boundary_step_fold, count), (B, lib.spo_boundary_step_fold_mb, prefix)):
            _abi.check(fn(*[_abi.ptr(x) for x in common], _abi.ptr(S["reward"]), _abi.ptr(S["cost"]), _abi.ptr(S["seg"]), _abi.ptr(S["boot_r"]),
                          _abi.ptr(S["boot_c"]), _abi.ptr(S["ret"]), _abi.ptr(S["ecost"]), _abi.ptr(S["len"]), _abi.ptr(S["events"]), _abi.ptr(cnt),
                          N * T, N, T, t, int(t == T - 1), _abi.ptr(S["fold_r"]), _abi.ptr(S["fold_c"]), 0.99, _abi.stream_ptr()), "boundary")
        assert int(prefix[t + 1]) == int(count[0])
    n = int(count[0])
    assert 0 < n < N * T
    for k in A:
        assert torch.equal(A[k], B[k]), k
    assert int(prefix[0]) == 0 and bool((prefix[1:] >= prefix[:-1]).all())


@pytest.mark.parametrize("N,T,D", [(4096, 6, 60), (1000, 5, 17), (31, 4, 64), (300, 3, 100)])
def test_values_and_boundary_in_one_launch_equal_the_two_calls(dev, N, T, D):
    """spo_values_boundary_step_fold (critics on the final observations + the step's boundary logic in one launch, the values
    handed over through LDS) against spo_values followed by spo_boundary_step_fold_mb: the values, buffers, masks, bootstrap and
    fold arrays, episode accumulators and the ordered event log bit-identical (obs_dim 100: its own two-launch fallback)."""
    from safepo import _abi
    from safepo.common.model import ActorVCritic
    lib = _abi.load()
    A_ = 5
    torch.manual_seed(N)
    pol = ActorVCritic(D, A_).to(dev)
    g = torch.Generator(device=dev).manual_seed(N + T)
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)

    def state():
        return {"reward": torch.zeros((N, T), **f32), "cost": torch.zeros((N, T), **f32), "seg": torch.zeros((N, T), dtype=torch.uint8, device=dev),
                "boot_r": torch.zeros((N, T), **f32), "boot_c": torch.zeros((N, T), **f32), "fold_r": torch.zeros((N, T), **f32),
                "fold_c": torch.zeros((N, T), **f32), "ret": torch.zeros(N, **f64), "ecost": torch.zeros(N, **f64), "len": torch.zeros(N, **f64),
                "events": torch.zeros((N * T, 4), **f64), "prefix": torch.zeros(T + 1, dtype=torch.int32, device=dev),
                "vf_r": torch.zeros(N, **f32), "vf_c": torch.zeros(N, **f32)}
    X, Y = state(), state()
    for t in range(T):
        rew, cost = torch.randn(N, generator=g, **f32), (torch.rand(N, generator=g, **f32) < 0.2).float()
        term, trunc = (torch.rand(N, generator=g, **f32) < 0.1).float(), (torch.rand(N, generator=g, **f32) < 0.15).float()
        vnext = [torch.randn(N, generator=g, **f32) for _ in range(2)]
        fobs = torch.randn((N, D), generator=g, **f32)

        def tail(S):
            return [_abi.ptr(S["reward"]), _abi.ptr(S["cost"]), _abi.ptr(S["seg"]), _abi.ptr(S["boot_r"]), _abi.ptr(S["boot_c"]),
                    _abi.ptr(S["ret"]), _abi.ptr(S["ecost"]), _abi.ptr(S["len"]), _abi.ptr(S["events"]), _abi.ptr(S["prefix"]), N * T, N, T, t,
                    int(t == T - 1), _abi.ptr(S["fold_r"]), _abi.ptr(S["fold_c"]), 0.99, _abi.stream_ptr()]
        head = [_abi.ptr(x) for x in (rew, cost, term, trunc, vnext[0], vnext[1])]
        _abi.check(lib.spo_values(_abi.ptr(pol.theta), _abi.ptr(fobs), _abi.ptr(X["vf_r"]), _abi.ptr(X["vf_c"]), N, D, A_, _abi.stream_ptr()), "values")
        _abi.check(lib.spo_boundary_step_fold_mb(*head, _abi.ptr(X["vf_r"]), _abi.ptr(X["vf_c"]), *tail(X)), "boundary")
        _abi.check(lib.spo_values_boundary_step_fold(_abi.ptr(pol.theta), _abi.ptr(fobs), _abi.ptr(Y["vf_r"]), _abi.ptr(Y["vf_c"]), D, A_,
                                                     *head, *tail(Y)), "fused")
        for k in X:
            assert torch.equal(X[k], Y[k]), (t, k)
    assert 0 < int(X["prefix"][T]) < N * T and float(X["boot_r"].abs().sum()) > 0


def test_gae_segment_mask_edge_cases(dev):
    # every step ends a path / single long path / all-terminated bootstraps / -0.0 deltas
    N, T = 9, 64
    reward, cost, v_r, v_c, seg, boot_r, boot_c = _random_case(N, T, 0.0, 5)
    seg[:] = True
    ref = R.gae_dense(reward, cost, v_r, v_c, seg, boot_r, boot_c, 0.99, 0.95, 0.95)
    got = _raw_gae(_run_gae(dev, reward, cost, v_r, v_c, seg, boot_r, boot_c))
    for g, r in zip(got, ref):
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32))       # no scan involved: exact
    z = np.zeros((N, T), np.float32)
    nz = -z
    seg[:] = False; seg[:, -1] = True
    got = _raw_gae(_run_gae(dev, nz, nz, z, z, seg, z, z))
    ref = R.gae_dense(nz, nz, z, z, seg, z, z, 0.99, 0.95, 0.95)
    for g, r in zip(got, ref):
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32))       # sign of zero preserved


def test_gae_unfinished_tail_is_zero(dev):
    N, T = 6, 128
    case = list(_random_case(N, T, 0.0, 11, finish_last=False))
    case[4][:, 50] = True                      # only one path end, at t=50
    got = _raw_gae(_run_gae(dev, *case))
    for g in got:
        assert np.all(g[:, 51:] == 0)
    seg2 = case[4].copy(); seg2[:, -1] = True
    ref = R.gae_dense(case[0], case[1], case[2], case[3], seg2, case[5], case[6], 0.99, 0.95, 0.95)
    for g, r in zip(got, ref):
        _assert_gae_close((g[:, :51],), (r[:, :51],), "finished prefix")


def test_gae_full_size_properties(dev):
    """BASELINE config 2 size: linearity in (reward, bootstrap) at fixed values==0, and the
    advantage-statistics kernel against numpy."""
    N, T = 4096, 128
    r1, c1, v_r, v_c, seg, b_r, b_c = _random_case(N, T, 1 / 64, 99)
    z = np.zeros_like(r1)
    a1 = _raw_gae(_run_gae(dev, r1, c1, z, z, seg, b_r, b_c))[0]
    a2 = _raw_gae(_run_gae(dev, 2 * r1, c1, z, z, seg, 2 * b_r, b_c))[0]
    np.testing.assert_allclose(a2, 2 * a1, rtol=1e-6, atol=1e-6)
    buf = _run_gae(dev, r1, c1, v_r, v_c, seg, b_r, b_c)
    raw = _raw_gae(buf)
    data = buf.get(lagrangian_multiplier=0.5)
    sr, sc = R.adv_standardize(torch.from_numpy(raw[0].reshape(-1)), torch.from_numpy(raw[1].reshape(-1)))
    np.testing.assert_allclose(data["adv_r"].cpu().numpy(), sr.numpy(), rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(data["adv_c"].cpu().numpy(), sc.numpy(), rtol=1e-5, atol=2e-6)
    assert abs(float(data["adv_r"].mean())) < 1e-5 and abs(float(data["adv_r"].std()) - 1) < 1e-4


def _policy_from_npz(z, prefix, dev):
    from safepo.common.model import ActorVCritic
    obs_dim, act_dim = z[prefix + "actor.mean.0.weight"].shape[1], z[prefix + "actor.log_std"].shape[0]
    pol = ActorVCritic(obs_dim, act_dim).to(dev)
    sd = {k[len(prefix):]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith(prefix)}
    pol.load_state_dict(sd)
    return pol


def test_policy_step_golden(dev, golden_dir):
    z = np.load(os.path.join(golden_dir, "model.npz"))
    pol = _policy_from_npz(z, "sd_", dev)
    # flat vector is the reference parameter order
    ref = R.OraclePolicy(60, 8)
    ref.load_state_dict({k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("sd_")})
    assert np.array_equal(pol.theta.cpu().numpy(), R.flat_params(ref).numpy())
    obs = torch.from_numpy(z["obs"]).to(dev)
    act, logp, v_r, v_c = pol.step(obs, eps=torch.from_numpy(z["eps"]).to(dev))
    np.testing.assert_allclose(act.cpu().numpy(), z["act"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(logp.cpu().numpy(), z["logp"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(v_r.cpu().numpy(), z["v_r"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(v_c.cpu().numpy(), z["v_c"], rtol=1e-5, atol=2e-6)
    a, l, r5, c5 = pol.step(obs[5], deterministic=True)
    np.testing.assert_allclose(r5.cpu().numpy(), z["row5_v_r"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(a.cpu().numpy(), z["act_det"][5], rtol=1e-5, atol=2e-6)
    vr, vc = pol.values(obs)
    np.testing.assert_allclose(vr.cpu().numpy(), z["v_r"], rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("obs_dim,act_dim,n", [(6, 2, 5), (17, 6, 70), (60, 8, 4096), (100, 16, 33), (33, 1, 64)])
def test_policy_step_shapes_vs_oracle(dev, obs_dim, act_dim, n):
    from safepo.common.model import ActorVCritic
    torch.manual_seed(obs_dim)
    pol = ActorVCritic(obs_dim, act_dim).to(dev)
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(act_dim) * 0.3)
    ref = R.OraclePolicy(obs_dim, act_dim)
    ref.load_state_dict({k: v.cpu().clone() for k, v in pol.state_dict().items()})
    obs, eps = torch.randn(n, obs_dim), torch.randn(n, act_dim)
    act, logp, v_r, v_c = pol.step(obs.to(dev), eps=eps.to(dev))
    with torch.no_grad():
        a, l, r, c = ref.step_with_eps(obs, eps)
    np.testing.assert_allclose(act.cpu().numpy(), a.numpy(), rtol=1e-5, atol=3e-6)
    np.testing.assert_allclose(logp.cpu().numpy(), l.numpy(), rtol=1e-5, atol=3e-5)
    np.testing.assert_allclose(v_r.cpu().numpy(), r.numpy(), rtol=1e-5, atol=3e-6)
    np.testing.assert_allclose(v_c.cpu().numpy(), c.numpy(), rtol=1e-5, atol=3e-6)


def _load_epoch_into_engine(z, e, eng, dev):
    b = eng.buffer
    N, T = b.num_envs, b.size
    for k in ("obs", "act", "reward", "cost", "value_r", "value_c", "log_prob"):
        b.data[k].copy_(torch.from_numpy(z[f"e{e}_raw_{k}"]))
    b.seg_end.copy_(torch.from_numpy(z[f"e{e}_seg_end"]))
    b.boot_r.copy_(torch.from_numpy(z[f"e{e}_boot_r"]))
    b.boot_c.copy_(torch.from_numpy(z[f"e{e}_boot_c"]))
    b.ptr = T


@pytest.mark.parametrize("fname", ["ppo_lag_trace.npz", "ppo_lag_trace_humanoid.npz", "ppo_lag_trace_car.npz"])
def test_ppo_lag_update_vs_reference_main_trace(dev, golden_dir, fname):
    """The epochs of the reference ppo_lag.main(): same buffers, same shuffles, same initial weights ->
    per-minibatch losses, early-stop iteration, KL and parameters after every epoch.  Trajectory quantities are gated by
    the drift envelope (tests/envelope.py): T32 = the values the reference itself recorded, T64 = the oracle replaying
    the same recorded inputs in float64; the HIP path may be at most 3x as far from T64 as the reference is.
    `_humanoid` (round 5): the reference's own run with ActorVCritic(376, 17) (oracle/make_golden_humanoid.py) -- the update runs
    on the persistent feature-split kernel (csrc/update_ks.hip) behind WidePPOLagEngine.  `_car`: the same at Car-class dims (72 / 2: the
    128-wide instantiation of the three-workgroup kernel)."""
    import envelope as E
    from safepo.common.engine import PPOLagEngine, WidePPOLagEngine
    z = np.load(os.path.join(golden_dir, fname))
    N, T, epochs = int(z["meta_num_envs"]), int(z["meta_T"]), int(z["meta_epochs"])
    pol = _policy_from_npz(z, "init_sd_", dev)
    cfg = {"hidden_sizes": [64, 64], "gamma": float(z["meta_cfg_gamma"]), "target_kl": float(z["meta_cfg_target_kl"]),
           "batch_size": int(z["e0_batch_size"]), "learning_iters": int(z["meta_cfg_learning_iters"]),
           "max_grad_norm": float(z["meta_cfg_max_grad_norm"])}
    wide = not pol.kernels_supported("ppo")
    eng = (WidePPOLagEngine if wide else PPOLagEngine)(pol, N, T, cfg, dev)
    assert wide == fname.endswith("_humanoid.npz") and (not wide or eng._feature_split_kernel_ok(eng._cfg_struct()))
    t64 = E.replay_ppo_lag_trace(z, torch.float64)
    ratios, kl_rows = [], []
    steps_done = 0
    tk = lambda: ({"floor_abs_max": E.theta_floor(3e-4, max(steps_done, 1)), "noise_directions": True} if wide else {})
    for e in range(epochs):
        ref_before = np.concatenate([z[f"e{e}_sd_before_{k}"].reshape(-1) for k in pol.state_dict()])
        ratios.append(E.assert_theta_envelope(pol.theta.cpu().numpy(), ref_before, t64["theta_before"][e],
                                              f"theta before epoch {e}", **tk())[0])
        _load_epoch_into_engine(z, e, eng, dev)
        lam = float(z[f"e{e}_row_Train_LagragianMultiplier"])
        n_perm = len([k for k in z.files if k.startswith(f"e{e}_perm")])
        perms = [torch.from_numpy(z[f"e{e}_perm{i}"].astype(np.int32)).to(dev) for i in range(n_perm)]
        eng.lr_factor = 1.0 - e / epochs
        out = eng.update(lam, perm_fn=lambda it: perms[min(it, n_perm - 1)])
        b = eng.buffer
        assert np.array_equal(b.data["target_value_r"].cpu().numpy(), z[f"e{e}_raw_target_value_r"])
        np.testing.assert_allclose(b.data["adv_r"].cpu().numpy().reshape(-1), z[f"e{e}_get_adv_r"], rtol=1e-5, atol=2e-6)
        got = torch.cat(out["losses"], 0).cpu().numpy()
        ref = z[f"e{e}_mb_losses"]
        steps_done += len(ref)
        assert out["stop_iter"] == int(z[f"e{e}_row_Train_StopIter"]), (out["stop_iter"], out["kl"])
        if e == 0:
            np.testing.assert_allclose(got[:3], ref[:3], rtol=1e-5, atol=1e-6)       # first steps from identical weights
        ratios.append(E.assert_loss_envelope(got, ref, t64["losses"][e], f"losses of epoch {e}", window=len(ref)))
        kl_rows.append((f"epoch {e}", out["kl"], float(z[f"e{e}_row_Train_KL"]), t64["kl"][e]))
    # the early-stop KL after each epoch's free-running passes: as far from the float64 replay as the reference's own values are
    print("KL yardstick (worst hip, reference):", E.gate_scalars(kl_rows, "Train/KL", rel_floor=1e-6))
    ref_final = np.concatenate([z[f"final_sd_{k}"].reshape(-1) for k in pol.state_dict()])
    ratios.append(E.assert_theta_envelope(pol.theta.cpu().numpy(), ref_final, t64["theta_final"], "final theta", **tk())[0])
    print("drift envelope ratios (<= 1 passes):", np.round(ratios, 3))


def _synthetic_update_problem(M, D, A, seed):
    g = torch.Generator().manual_seed(seed)
    obs = torch.randn(M, D, generator=g)
    act = torch.randn(M, A, generator=g)
    logp = -A * 0.9 - 0.5 * (act ** 2).sum(-1) + 0.1 * torch.randn(M, generator=g)
    tgt_r, tgt_c = torch.randn(M, generator=g), torch.rand(M, generator=g)
    adv = torch.randn(M, generator=g)
    return obs, act, logp, tgt_r, tgt_c, adv


@pytest.mark.parametrize("M,D,A,batch", [(256, 60, 8, 64), (150, 60, 8, 64), (200, 12, 2, 64), (64, 33, 5, 64),
                                         (300, 60, 8, 128), (40, 20, 3, 64), (150, 100, 4, 64), (130, 128, 16, 64),
                                         # round 6, the row-split kernel's edges: a second row group without rows (batch <= 32), a
                                         # ragged one (batch 33 / 50), one-feature and 64-feature observations, act_dim 1 and 16
                                         (100, 5, 1, 20), (77, 64, 16, 7), (165, 16, 3, 33), (250, 1, 2, 50), (96, 48, 16, 32)])
def test_minibatch_grad_and_step_vs_oracle(dev, M, D, A, batch):
    """First-minibatch gradient (pre-clip), losses, and parameters after one full pass
    (partial last batch included) against torch autograd + Adam on the CPU oracle."""
    from safepo import _abi
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    torch.manual_seed(M + D)
    pol = ActorVCritic(D, A).to(dev)
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    ref = R.OraclePolicy(D, A)
    ref.load_state_dict({k: v.cpu().clone() for k, v in pol.state_dict().items()})
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=M)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": batch, "learning_iters": 1,
           "max_grad_norm": 0.5 if M == 256 else 40.0}          # one case with the clip active
    eng = PPOLagEngine(pol, 1, M, cfg, dev)
    b = eng.buffer
    b.data["obs"].copy_(obs.view(1, M, D)); b.data["act"].copy_(act.view(1, M, A))
    b.data["log_prob"].copy_(logp.view(1, M)); b.data["target_value_r"].copy_(tgt_r.view(1, M))
    b.data["target_value_c"].copy_(tgt_c.view(1, M)); b.adv_mix.copy_(adv.view(1, M))
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(3))
    # --- split kernel: gradient of the first minibatch
    c = eng._cfg_struct()
    nb = min(batch, M)
    idx = perm[:nb].to(torch.int32).to(dev)
    d = b.data
    _abi.check(eng.lib.spo_ppo_lag_grad(_abi.ptr(pol.theta), _abi.ptr(d["obs"]), _abi.ptr(d["act"]), _abi.ptr(d["log_prob"]),
                                        _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(b.adv_mix),
                                        _abi.ptr(idx), nb, nb, c, _abi.ptr(eng.flat_grad), _abi.ptr(eng.losses3),
                                        _abi.stream_ptr()), "grad")
    upd = R.PPOLagUpdater(ref, epochs=1, max_grad_norm=cfg["max_grad_norm"])
    ref0 = {k: v.clone() for k, v in ref.state_dict().items()}
    rec = {}
    ii = perm[:nb]
    l3 = upd.minibatch_step(obs[ii], act[ii], logp[ii], tgt_r[ii], tgt_c[ii], adv[ii], record=rec)
    g_ref = rec["grad_preclip"].numpy()
    g_got = eng.flat_grad.cpu().numpy()
    scale = np.abs(g_ref).max()
    assert np.abs(g_got - g_ref).max() <= 1e-5 * scale                 # north_star: grads within 1e-5 (of the scale)
    np.testing.assert_allclose(eng.losses3.cpu().numpy(), np.asarray(l3), rtol=1e-5, atol=0)
    # --- persistent kernel: one full pass, compare with the oracle restarted from the same weights
    ref.load_state_dict(ref0)
    upd = R.PPOLagUpdater(ref, epochs=1, max_grad_norm=cfg["max_grad_norm"])
    losses_ref = []
    for s in range(0, M, batch):
        ii = perm[s:s + batch]
        losses_ref.append(upd.minibatch_step(obs[ii], act[ii], logp[ii], tgt_r[ii], tgt_c[ii], adv[ii]))
    losses = eng.learning_iter(perm.to(torch.int32).to(dev))
    eng.check_sync_error()
    np.testing.assert_allclose(losses.cpu().numpy(), np.asarray(losses_ref), rtol=1e-4, atol=2e-6)
    # parameters after the pass: no further from the float64 trajectory than 3 x the float32 oracle is (every element: max-norm)
    import envelope as E
    nst = len(losses_ref)
    _, t64 = E.oracle_trajectory(ref0, (obs, act, logp, tgt_r, tgt_c, adv), perm, batch, nst, torch.float64, [nst],
                                 max_grad_norm=cfg["max_grad_norm"])
    E.assert_theta_envelope(pol.theta.cpu().numpy(), R.flat_params(ref).numpy(), t64[nst], f"theta after {nst} steps")
    # optimiser state round-trips through adam_m / adam_v
    m_ref = torch.cat([upd.opt_r.state[p]["exp_avg"].reshape(-1) for p in ref.reward_critic.parameters()])
    np.testing.assert_allclose(eng.adam_m[:m_ref.numel()].cpu().numpy(), m_ref.numpy(), rtol=1e-3, atol=1e-7)


@pytest.mark.parametrize("spec", ["1", "0"])
def test_intermittent_clip_vs_oracle(dev, spec, monkeypatch):
    """clip_grad_norm_ active on SOME steps (bound = median of the unclipped run's joint norms): the persistent launch
    validates the clip after the next step's forward while steps are unclipped and falls back to waiting for the norm
    after a clipped one, so runs of clipped / unclipped steps in both orders must all match the oracle
    (ppo_lag.py:325 clip_grad_norm_ over actor + both critics)."""
    import subprocess, sys
    if spec == "0":
        # the switch is read once per process: the non-speculative form is checked in a child process
        env = dict(os.environ, SPO_UPDATE_SPEC="0")
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", __file__, "-k",
                            "test_intermittent_clip_vs_oracle and 1"], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    M, D, A, batch = 1536, 60, 8, 64
    torch.manual_seed(11)
    pol = ActorVCritic(D, A).to(dev)
    ref = R.OraclePolicy(D, A)
    ref.load_state_dict({k: v.cpu().clone() for k, v in pol.state_dict().items()})
    ref0 = {k: v.clone() for k, v in ref.state_dict().items()}
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=5)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(3))

    thetas = []

    def oracle_run(bound):
        ref.load_state_dict(ref0)
        upd = R.PPOLagUpdater(ref, epochs=1, max_grad_norm=bound)
        out, norms = [], []
        thetas.clear()
        for s in range(0, M, batch):
            ii = perm[s:s + batch]
            rec = {}
            out.append(upd.minibatch_step(obs[ii], act[ii], logp[ii], tgt_r[ii], tgt_c[ii], adv[ii], record=rec))
            norms.append(float(rec["grad_preclip"].double().norm()))
            thetas.append(R.flat_params(ref).numpy().copy())
        return np.asarray(out), np.asarray(norms)

    _, free_norms = oracle_run(1e9)
    bound = float(np.median(free_norms))
    losses_ref, norms = oracle_run(bound)
    clipped = norms > bound
    flips = int(np.sum(clipped[1:] != clipped[:-1]))
    assert clipped.any() and (~clipped).any() and flips >= 4, (clipped, bound)
    assert np.abs(norms / bound - 1).min() > 1e-4           # no step sits on the bound (the decision is not a rounding matter)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": batch, "learning_iters": 1,
           "max_grad_norm": bound}
    eng = PPOLagEngine(pol, 1, M, cfg, dev)
    b = eng.buffer
    b.data["obs"].copy_(obs.view(1, M, D)); b.data["act"].copy_(act.view(1, M, A))
    b.data["log_prob"].copy_(logp.view(1, M)); b.data["target_value_r"].copy_(tgt_r.view(1, M))
    b.data["target_value_c"].copy_(tgt_c.view(1, M)); b.adv_mix.copy_(adv.view(1, M))
    losses = eng.learning_iter(perm.to(torch.int32).to(dev))
    eng.check_sync_error()
    np.testing.assert_allclose(losses.cpu().numpy(), losses_ref, rtol=1e-4, atol=2e-6)
    # the same clipped / unclipped sequence in float64 (no step sits on the bound: asserted above) is the yardstick
    import envelope as E
    nst = len(losses_ref)
    ends_all = list(range(1, nst + 1))
    l64, t64 = E.oracle_trajectory(ref0, (obs, act, logp, tgt_r, tgt_c, adv), perm, batch, nst, torch.float64, ends_all,
                                   max_grad_norm=bound)
    E.assert_loss_envelope(losses.cpu().numpy(), losses_ref, l64, "intermittent clip: losses", window=nst)
    E.assert_theta_envelope(pol.theta.cpu().numpy(), R.flat_params(ref).numpy(), t64[nst], "intermittent clip: theta")
    # launches that END on a clipped step right after an unclipped one (the verdict of the last step has no next forward to
    # hide behind: the helpers restore and redo after the loop) and on an unclipped step right after a clipped one
    ends = [k for k in range(2, len(clipped) + 1) if clipped[k - 1] and not clipped[k - 2]][:2] + \
           [k for k in range(2, len(clipped) + 1) if not clipped[k - 1] and clipped[k - 2]][:1]
    assert len(ends) == 3
    for k in ends:
        pol.load_state_dict({kk: v.to(dev) for kk, v in ref0.items()})
        eng.adam_m.zero_(); eng.adam_v.zero_(); eng.adam_step = 0
        sub = PPOLagEngine(pol, 1, k * batch, cfg, dev)
        for name in ("obs", "act", "log_prob", "target_value_r", "target_value_c"):
            src = {"obs": obs, "act": act, "log_prob": logp, "target_value_r": tgt_r, "target_value_c": tgt_c}[name]
            sub.buffer.data[name].copy_(src[perm[:k * batch]].view(1, k * batch, *src.shape[1:]))
        sub.buffer.adv_mix.copy_(adv[perm[:k * batch]].view(1, k * batch))
        l_k = sub.learning_iter(torch.arange(k * batch, dtype=torch.int32, device=dev))
        sub.check_sync_error()
        np.testing.assert_allclose(l_k.cpu().numpy(), losses_ref[:k], rtol=1e-4, atol=2e-6)
        E.assert_theta_envelope(pol.theta.cpu().numpy(), thetas[k - 1], t64[k], f"intermittent clip: theta after {k} steps")


def test_split_path_equals_persistent(dev):
    """spo_ppo_lag_grad + spo_clip_adam (data-parallel form, world size 1) == persistent kernel."""
    from safepo import _abi
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    M, D, A = 192, 60, 8
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=1)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 40.0}
    thetas = []
    for mode in ("persistent", "split"):
        torch.manual_seed(5)
        pol = ActorVCritic(D, A).to(dev)
        eng = PPOLagEngine(pol, 1, M, cfg, dev)
        b = eng.buffer
        b.data["obs"].copy_(obs.view(1, M, D)); b.data["act"].copy_(act.view(1, M, A))
        b.data["log_prob"].copy_(logp.view(1, M)); b.data["target_value_r"].copy_(tgt_r.view(1, M))
        b.data["target_value_c"].copy_(tgt_c.view(1, M)); b.adv_mix.copy_(adv.view(1, M))
        perm = torch.arange(M, dtype=torch.int32, device=dev).flip(0).contiguous()
        if mode == "persistent":
            eng.learning_iter(perm)
        else:
            c = eng._cfg_struct()
            d = b.data
            for k in range(M // 64):
                _abi.check(eng.lib.spo_ppo_lag_grad(_abi.ptr(pol.theta), _abi.ptr(d["obs"]), _abi.ptr(d["act"]),
                                                    _abi.ptr(d["log_prob"]), _abi.ptr(d["target_value_r"]),
                                                    _abi.ptr(d["target_value_c"]), _abi.ptr(b.adv_mix),
                                                    perm.data_ptr() + 4 * 64 * k, 64, 64, c, _abi.ptr(eng.flat_grad),
                                                    _abi.ptr(eng.losses3), _abi.stream_ptr()), "grad")
                _abi.check(eng.lib.spo_clip_adam(_abi.ptr(pol.theta), _abi.ptr(eng.adam_m), _abi.ptr(eng.adam_v),
                                                 _abi.ptr(eng.flat_grad), k, 1.0, c, _abi.stream_ptr()), "adam")
        thetas.append(pol.theta.cpu().numpy())
    np.testing.assert_allclose(thetas[0], thetas[1], rtol=1e-5, atol=1e-7)


def test_actor_kl_vs_oracle(dev):
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    torch.manual_seed(2)
    M, D, A = 1000, 60, 8
    pol = ActorVCritic(D, A).to(dev)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 0.02, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 40.0}
    eng = PPOLagEngine(pol, 1, M, cfg, dev)
    obs = torch.randn(M, D)
    eng.buffer.data["obs"].copy_(obs.view(1, M, D))
    ref = R.OraclePolicy(D, A)
    ref.load_state_dict({k: v.cpu().clone() for k, v in pol.state_dict().items()})
    eng.snapshot_old_distribution()
    with torch.no_grad():
        od = ref.actor(obs)
        old_mean, old_std = od.mean.clone(), od.stddev.clone()
    np.testing.assert_allclose(eng.mean_old.cpu().numpy(), old_mean.numpy(), rtol=1e-5, atol=2e-6)
    with torch.no_grad():
        pol.theta.add_(0.01 * torch.randn_like(pol.theta))
    ref.load_state_dict({k: v.cpu().clone() for k, v in pol.state_dict().items()})
    kl = eng.kl_to_old()
    assert kl == pytest.approx(R.actor_kl(ref, obs, old_mean, old_std), rel=1e-4)


@pytest.mark.parametrize("n,steps", [(8, 32), (70, 20), (3, 130)])
def test_collect_boundary_update_end_to_end(dev, n, steps):
    from smoke_check import smoke_check
    smoke_check(num_envs=n, steps=steps, seed=n)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("shape", [(60, 8, [64, 64]), (70, 20, [96, 96])])
def test_rollout_epoch_replayed_from_a_graph_equals_the_eager_loop(dev, monkeypatch, normalize, shape):
    """engine.rollout_epoch: T x (collect_step -> env.step -> post_step) replayed from ONE captured HIP graph leaves the
    buffer, the boundary marks, the episode log, the normaliser state and (after the update) the parameters bit-identical to
    the eager loop, epoch after epoch (same noise: the graph-safe generator continues the eager Philox sequence).  Both the
    persistent-kernel engine and the wide-network engine."""
    from safepo.common.engine import PPOLagEngine, WidePPOLagEngine
    from safepo.common.env import SynthDeviceEnv
    from safepo.common.model import ActorVCritic
    D, A, hidden = shape
    N, T, epochs = 512, 24, 4

    def run(graph):
        monkeypatch.setenv("SPO_ROLLOUT_GRAPH", "1" if graph else "0")
        torch.manual_seed(11)
        pol = ActorVCritic(D, A, hidden_sizes=hidden).to(dev)
        cfg = {"hidden_sizes": hidden, "gamma": 0.99, "target_kl": float("inf"), "batch_size": 64, "learning_iters": 2,
               "max_grad_norm": 40.0}
        eng = (PPOLagEngine if pol.kernels_supported() else WidePPOLagEngine)(pol, N, T, cfg, dev)
        env = SynthDeviceEnv(N, D, A, seed=5, p_term=0.02, p_cost=0.1, trunc_len=10, device=dev, normalize_obs=normalize,
                             obs_scale=2.0, obs_shift=0.5)
        rms = env.fuse_normalize(True)
        obs, _ = env.reset()
        snaps = []
        for e in range(epochs):
            obs = eng.rollout_epoch(env, obs, rms=rms)
            n_ep = eng.drain_episode_events(None)
            b = eng.buffer
            snap = {k: v.clone() for k, v in b.data.items()}
            snap.update(seg_end=b.seg_end.clone(), boot_r=b.boot_r.clone(), boot_c=b.boot_c.clone(), next_obs=obs.clone(),
                        events=eng.events[:n_ep].clone(), prefix=eng.events_prefix.clone(), ep_ret=eng.ep_ret.clone(),
                        ep_len=eng.ep_len.clone(), n_ep=torch.tensor(n_ep))
            if rms is not None:
                snap["rms"] = rms.state.clone()
            assert b.ptr == T and env.step_count == 1 + (e + 1) * T
            eng.update(0.001)
            snap["theta"] = pol.theta.clone()
            snaps.append(snap)
        return snaps, getattr(eng, "_rollout_graphs", {})

    eager, g0 = run(False)
    graph, g1 = run(True)
    assert not g0 and len(g1) == 1
    for e, (x, y) in enumerate(zip(eager, graph)):
        assert int(x["n_ep"]) == int(y["n_ep"]) and int(x["n_ep"]) > 0
        for k in x:
            assert torch.equal(x[k], y[k]), (e, k)


@pytest.mark.parametrize("D,affine", [(60, True), (60, False), (7, True), (128, True), (376, True)])
def test_synth_env_one_launch_step_equals_the_two_kernel_form(dev, D, affine):
    """spo_synth_env_step_rel (flags + observations + the affine map of the raw observation in one launch, device step base)
    against spo_synth_env_step (two kernels) followed by the two tensor operations it replaces: bit-identical, over steps with
    terminations and truncations."""
    from safepo import _abi
    lib = _abi.load()
    N, seed = 1000, 77
    f32 = dict(dtype=torch.float32, device=dev)

    def fresh():
        return ([torch.zeros((N, D), **f32), torch.zeros((N, D), **f32)] + [torch.zeros(N, **f32) for _ in range(4)]
                + [torch.zeros(N, dtype=torch.int32, device=dev)])
    a, b = fresh(), fresh()
    base = torch.tensor([40], dtype=torch.int64, device=dev)
    for k in range(1, 30):
        _abi.check(lib.spo_synth_env_step(*[_abi.ptr(x) for x in a], N, D, seed, 40 + k, 0.05, 0.3, 9, _abi.stream_ptr()), "two-kernel")
        if affine:
            a[0].mul_(1.7).add_(-0.3)
        _abi.check(lib.spo_synth_env_step_rel(*[_abi.ptr(x) for x in b], N, D, seed, k, _abi.ptr(base), 0.05, 0.3, 9, int(affine),
                                              1.7, -0.3, _abi.stream_ptr()), "one-launch")
        for x, y, name in zip(a, b, ("obs", "final_obs", "reward", "cost", "terminated", "truncated", "t_env")):
            assert torch.equal(x, y), (k, name)
    assert float(a[4].sum()) > 0 and float(a[5].sum()) > 0


@pytest.mark.parametrize("N,T,D,A", [(4096, 12, 60, 8), (300, 9, 17, 3)])
def test_side_by_side_collect_kernels_equal_the_sequential_ones(dev, tmp_path, N, T, D, A):
    """The round-4 collect kernels (policy_step_par_kernel: the three networks side by side, 32 rows per workgroup, batched
    weight staging; the critics-only form with the boundary logic behind it; the normaliser's count added by the step kernel)
    against the round-3 ones (SPO_STEP_PAR=0: networks in turn, spo_values + spo_boundary_step_fold_mb): two epochs of the
    collect loop from the same seeds leave bit-identical buffers, marks, bootstrap values, episode logs, normaliser states and
    (after the update) parameters.  The selection is read once per process, hence two worker processes."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = []
    for par in ("1", "0"):
        out = str(tmp_path / f"collect_par{par}.npz")
        env = dict(os.environ, SPO_STEP_PAR=par, SPO_ROLLOUT_GRAPH="0")
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "collect_worker.py"), out, str(N), str(T), str(D), str(A)],
                           capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        files.append(np.load(out))
    x, y = files
    assert sorted(x.files) == sorted(y.files) and len(x["e0_events"]) > 0
    for k in x.files:
        assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), k


def test_ppo_lag_main_entrypoint_synthetic(dev, tmp_path):
    """safepo.single_agent.ppo_lag.main on the device-resident synthetic env: runs, logs the
    reference's columns, writes progress.csv / config.json / torch_save/model0.pt."""
    import argparse
    import csv
    from safepo.single_agent import ppo_lag
    args = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=16, experiment="t",
                              log_dir=str(tmp_path / "exp" / "task" / "run"), device="cuda", device_id=0,
                              write_terminal=True, headless=False, total_steps=2 * 16 * 64, steps_per_epoch=16 * 64,
                              randomize=False, cost_limit=25.0, lagrangian_multiplier_init=0.001,
                              lagrangian_multiplier_lr=0.035, cfg_override={"learning_iters": 3},
                              env_kwargs={"trunc_len": 16})
    ppo_lag.main(args, {})
    rows = list(csv.DictReader(open(tmp_path / "exp" / "task" / "run" / "progress.csv")))
    assert len(rows) == 2
    for col in ("Metrics/EpRet", "Metrics/EpCost", "Metrics/EpLen", "Train/Epoch", "Train/TotalSteps", "Train/StopIter",
                "Train/KL", "Train/LagragianMultiplier", "Train/LR", "Loss/Loss_reward_critic", "Loss/Loss_cost_critic",
                "Loss/Loss_actor", "Time/Rollout", "Time/Update", "Time/Total", "Value/RewardAdv", "Value/CostAdv"):
        assert col in rows[0], col
    assert float(rows[0]["Metrics/EpLen"]) == 16.0
    sd = torch.load(tmp_path / "exp" / "task" / "run" / "torch_save" / "model0.pt")
    assert set(sd) == {"log_std", "mean.0.weight", "mean.0.bias", "mean.2.weight", "mean.2.bias", "mean.4.weight", "mean.4.bias"}
    assert os.path.exists(tmp_path / "exp" / "task" / "run" / "config.json")


def test_library_is_loaded_from_tree(dev):
    from safepo import _abi
    _abi.load()
    maps = open("/proc/self/maps").read()
    assert "libsafepo_hip.so" in maps


# ---------------------------------------------------------------------------------------- CPO (config 3)
def _cpo_engine(z, prefix, dev, N, T, cfg_over=None):
    from safepo.single_agent.cpo import CPOEngine, default_cfg
    pol = _policy_from_npz(z, prefix, dev)
    cfg = dict(default_cfg)
    cfg.update(cfg_over or {})
    if not pol.kernels_supported("cpo"):                    # (dims outside the LDS-resident kernels: the wide engine)
        from safepo.single_agent.cpo import make_engine
        return pol, make_engine(pol, N, T, cfg, dev)
    return pol, CPOEngine(pol, N, T, cfg, dev)


def test_cpo_fvp_known_answers_from_reference(dev, golden_dir):
    """FVP vectors recorded from the reference's double-backward fvp() (cpo.py:132-157)."""
    z = np.load(os.path.join(golden_dir, "cpo_trace.npz"))
    N, T = int(z["meta_num_envs"]), int(z["meta_T"])
    pol, eng = _cpo_engine(z, "init_sd_", dev, N, T)
    eng.buffer.data["obs"].copy_(torch.from_numpy(z["e0_raw_obs"]))
    for i in range(3):
        sd = {"actor." + k[len(f"fvp_sd{i}_"):]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith(f"fvp_sd{i}_")}
        pol.load_state_dict(sd, strict=False)
        got = eng.fvp(torch.from_numpy(z[f"fvp_in{i}"]).to(dev)).cpu().numpy()
        ref = z[f"fvp_out{i}"]
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max())


def test_cpo_surrogate_gradients_vs_oracle(dev):
    from safepo.single_agent.cpo import CPOEngine, default_cfg
    from safepo.common.model import ActorVCritic
    torch.manual_seed(4)
    M, D, A = 1000, 60, 8
    pol = ActorVCritic(D, A).to(dev)
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    eng = CPOEngine(pol, 1, M, dict(default_cfg), dev)
    obs, act, logp, _, _, adv = _synthetic_update_problem(M, D, A, seed=9)
    b = eng.buffer
    b.data["obs"].copy_(obs.view(1, M, D)); b.data["act"].copy_(act.view(1, M, A)); b.data["log_prob"].copy_(logp.view(1, M))
    b.data["adv_r"].copy_(adv.view(1, M)); b.data["adv_c"].copy_((adv * 0.5 + 0.1).view(1, M))
    ref = R.OraclePolicy(D, A)
    ref.load_state_dict({k: v.cpu().clone() for k, v in pol.state_dict().items()})
    data = {"obs": obs, "act": act, "log_prob": logp, "adv_r": adv, "adv_c": adv * 0.5 + 0.1}
    for which, key, sign in (("r", "adv_r", -1.0), ("c", "adv_c", 1.0)):
        ref.actor.zero_grad()
        loss = R.cpo_surrogate(ref, data, which)
        loss.backward()
        g_ref = R.actor_flat_grads(ref.actor).numpy()
        g, mean = eng.surrogate_grad(b.data[key], sign)
        np.testing.assert_allclose(g.cpu().numpy(), g_ref, rtol=1e-4, atol=1e-5 * np.abs(g_ref).max())
        assert sign * mean == pytest.approx(float(loss.detach()), rel=1e-5)
    # FVP against the oracle's double backward, random direction
    v = torch.randn(eng.Pa)
    hv_ref = R.cpo_fvp(v, ref, obs).numpy()
    np.testing.assert_allclose(eng.fvp(v.to(dev)).cpu().numpy(), hv_ref, rtol=1e-4, atol=1e-5 * np.abs(hv_ref).max())
    # line-search evaluation at the unchanged parameters: KL == 0, losses == the surrogates
    eng.snapshot_old_distribution()
    lr_, lc_, kl = eng.linesearch_eval()
    assert kl == pytest.approx(0.0, abs=1e-9)
    assert lr_ == pytest.approx(float(R.cpo_surrogate(ref, data, "r")), rel=1e-5)
    assert lc_ == pytest.approx(float(R.cpo_surrogate(ref, data, "c")), rel=1e-5)


@pytest.mark.parametrize("ep_costs", [-1.0, 0.3])
def test_cpo_actor_step_drift_envelope(dev, ep_costs):
    """The trust-region step (two surrogate gradients, 2 x 15 CG iterations on Fisher-vector products, case analysis, line
    search: cpo.py:350-532) amplifies rounding through the CG recurrences, which is why the trace replays above compare at
    5e-3.  Here the deviation is SHOWN to be rounding: the oracle takes the same step in float64 (yardstick) and in float32
    (the reference's arithmetic), and the HIP step may be at most 3x as far from the float64 one as the float32 oracle is
    (+ a floor of 1e-7 of the scale) -- for the curvature x^T H x, the step length alpha, the step norm and the actor
    parameters after the step; the discrete decisions (case, accepted line-search step) must coincide."""
    import copy
    from safepo.single_agent.cpo import CPOEngine, default_cfg
    from safepo.common.model import ActorVCritic
    torch.manual_seed(14)
    M, D, A = 4096, 60, 8
    pol = ActorVCritic(D, A).to(dev)
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    eng = CPOEngine(pol, 1, M, dict(default_cfg), dev)
    obs, act, logp, _, _, adv = _synthetic_update_problem(M, D, A, seed=21)
    adv_c = adv.flip(0) * 0.5 + 0.1
    b = eng.buffer
    b.data["obs"].copy_(obs.view(1, M, D)); b.data["act"].copy_(act.view(1, M, A)); b.data["log_prob"].copy_(logp.view(1, M))
    b.data["adv_r"].copy_(adv.view(1, M)); b.data["adv_c"].copy_(adv_c.view(1, M))
    ref32 = R.OraclePolicy(D, A)
    ref32.load_state_dict({k: v.cpu().clone() for k, v in pol.state_dict().items()})
    ref64 = copy.deepcopy(ref32).double()
    data32 = {"obs": obs, "act": act, "log_prob": logp, "adv_r": adv, "adv_c": adv_c}
    data64 = {k: v.double() for k, v in data32.items()}
    o32 = R.cpo_policy_update(ref32, data32, ep_costs, target_kl=default_cfg["target_kl"])
    o64 = R.cpo_policy_update(ref64, data64, ep_costs, target_kl=default_cfg["target_kl"])
    th32 = R.actor_flat_params(ref32.actor).double().numpy()
    th64 = R.actor_flat_params(ref64.actor).double().numpy()
    out = eng.policy_update(ep_costs)
    th_hip = eng.theta_actor.double().cpu().numpy()
    assert out["case"] == o32["case"] == o64["case"]
    assert out["acceptance_step"] == o32["accept"] == o64["accept"] and out["acceptance_step"] >= 1
    for name, hip, v32, v64 in (("xHx", out["xHx"], float(o32["xHx"]), float(o64["xHx"])),
                                ("alpha", out["alpha"], float(o32["alpha"]), float(o64["alpha"])),
                                ("final_step_norm", out["final_step_norm"], float((o32["step_frac"] * o32["step_direction"]).norm()),
                                 float((o64["step_frac"] * o64["step_direction"]).norm()))):
        G.gate(hip, v32, v64, name, norms=G.MAX)
    G.gate(th_hip, th32, th64, f"cpo step envelope (ep_costs {ep_costs}) theta", rel_floor=1e-7, norms=G.L2)
    G.gate(th_hip, th32, th64, f"cpo step envelope (ep_costs {ep_costs}) theta", norms=G.MAX)
    print(f"cpo step envelope (ep_costs {ep_costs}): case {out['case']}; xHx hip {out['xHx']:.9g} f32 {float(o32['xHx']):.9g} f64 {float(o64['xHx']):.9g}")


def test_cpo_update_vs_reference_main_trace(dev, golden_dir):
    """Replays the reference cpo.main(): CG, case analysis (incl. an infeasible-recovery epoch), line search,
    actor parameters after the step, critic fit with the recorded shuffles."""
    z = np.load(os.path.join(golden_dir, "cpo_trace.npz"))
    N, T, epochs = int(z["meta_num_envs"]), int(z["meta_T"]), int(z["meta_epochs"])
    pol, eng = _cpo_engine(z, "init_sd_", dev, N, T, {"learning_iters": int(z["meta_cfg_learning_iters"]),
                                                       "batch_size": int(z["e0_batch_size"]),
                                                       "target_kl": float(z["meta_cfg_target_kl"])})
    cases = []
    for e in range(epochs):
        ref_before = np.concatenate([z[f"e{e}_sd_before_{k}"].reshape(-1) for k in pol.state_dict()])
        _assert_params_close(pol.theta.cpu().numpy(), ref_before, 1e-3, 8, rtol=2e-3, atol=2e-5, what=f"theta before epoch {e}")
        _load_epoch_into_engine(z, e, eng, dev)
        eng.buffer.compute_gae(None)
        assert np.array_equal(eng.buffer.data["target_value_c"].cpu().numpy(), z[f"e{e}_raw_target_value_c"])
        ep_costs = float(z[f"e{e}_get_stats_Metrics_EpCost"]) - float(z["meta_arg_cost_limit"])
        out = eng.policy_update(ep_costs)
        cases.append(out["case"])
        assert out["acceptance_step"] == int(z[f"e{e}_Misc_AcceptanceStep"])
        assert out["xHx"] == pytest.approx(float(z[f"e{e}_Misc_xHx"]), rel=5e-3)
        assert out["H_inv_g"] == pytest.approx(float(z[f"e{e}_Misc_H_inv_g"]), rel=5e-3)
        assert out["gradient_norm"] == pytest.approx(float(z[f"e{e}_Misc_gradient_norm"]), rel=1e-4)
        assert out["final_step_norm"] == pytest.approx(float(z[f"e{e}_Misc_FinalStepNorm"]), rel=5e-3)
        assert out["alpha"] == pytest.approx(float(z[f"e{e}_Misc_Alpha"]), rel=5e-3)
        assert out["kl"] == pytest.approx(float(z[f"e{e}_Train_KL"]), rel=2e-2)
        assert out["loss_actor"] == pytest.approx(float(z[f"e{e}_Loss_Loss_actor"]), rel=1e-3, abs=1e-6)
        act_ref = np.concatenate([z[f"e{e}_actor_after_{k}"].reshape(-1) for k in pol.actor.state_dict()])
        np.testing.assert_allclose(eng.theta_actor.cpu().numpy(), act_ref, rtol=5e-3, atol=2e-5)
        iters = int(z["meta_cfg_learning_iters"])
        perms = [torch.from_numpy(z[f"e{e}_perm{i}"].astype(np.int32)).to(dev) for i in range(iters)]
        fit = eng.critic_fit(perm_fn=lambda it: perms[it])
        eng.buffer.reset()
        got = torch.cat(fit["losses"], 0).cpu().numpy()
        np.testing.assert_allclose(got, z[f"e{e}_mb_losses"][:, :2], rtol=2e-3, atol=1e-5)
    assert cases[1] in (0, 1)
    ref_final = np.concatenate([z[f"final_sd_{k}"].reshape(-1) for k in pol.state_dict()])
    _assert_params_close(pol.theta.cpu().numpy(), ref_final, 1e-3, 12, rtol=5e-3, atol=5e-5, what="final theta")


def test_cpo_trace_epochs_one_by_one_under_the_fp64_yardstick(dev, golden_dir):
    """The replay above lets the HIP state run free over the epochs and compares at 5e-3 / 2e-2 -- wide enough to hide a
    0.4 % defect.  Here every epoch of the reference's cpo.main() trace is taken on its own: parameters = the
    reference's recorded state before the epoch, buffer = its recorded rollout, and the trust-region step is gated by the
    fp64 yardstick with the reference's OWN recorded float32 numbers as the float32 leg: |HIP - f64| <= 3 |reference - f64| +
    1e-6 of the value, for x^T H x, alpha, the step norm, the gradient norm, H_inv_g and the actor parameters after the
    step (float64 = the oracle on the same inputs, cpo.py:350-532); the discrete decisions must coincide."""
    import copy
    z = np.load(os.path.join(golden_dir, "cpo_trace.npz"))
    N, T, epochs = int(z["meta_num_envs"]), int(z["meta_T"]), int(z["meta_epochs"])
    tkl = float(z["meta_cfg_target_kl"])
    pol, eng = _cpo_engine(z, "init_sd_", dev, N, T, {"learning_iters": int(z["meta_cfg_learning_iters"]),
                                                       "batch_size": int(z["e0_batch_size"]), "target_kl": tkl})
    D, A, M = pol.obs_dim, pol.act_dim, N * T
    worst = {}
    for e in range(epochs):
        sd = {k: torch.from_numpy(z[f"e{e}_sd_before_{k}"].copy()) for k in pol.state_dict()}
        pol.load_state_dict(sd)
        _load_epoch_into_engine(z, e, eng, dev)
        eng.buffer.compute_gae(None)
        d = eng.buffer.data
        data64 = {"obs": d["obs"].view(M, D).double().cpu(), "act": d["act"].view(M, A).double().cpu(),
                  "log_prob": d["log_prob"].view(M).double().cpu(), "adv_r": d["adv_r"].view(M).double().cpu(),
                  "adv_c": d["adv_c"].view(M).double().cpu()}
        ref64 = R.OraclePolicy(D, A)
        ref64.load_state_dict(sd)
        ref64 = ref64.double()
        ep_costs = float(z[f"e{e}_get_stats_Metrics_EpCost"]) - float(z["meta_arg_cost_limit"])
        o64 = R.cpo_policy_update(ref64, data64, ep_costs, target_kl=tkl)
        out = eng.policy_update(ep_costs)
        eng.buffer.reset()
        assert out["case"] == o64["case"] and out["acceptance_step"] == o64["accept"] == int(z[f"e{e}_Misc_AcceptanceStep"])
        step64 = float((o64["step_frac"] * o64["step_direction"]).norm())
        for name, hip, ref32, v64 in (("xHx", out["xHx"], float(z[f"e{e}_Misc_xHx"]), float(o64["xHx"])),
                                      ("alpha", out["alpha"], float(z[f"e{e}_Misc_Alpha"]), float(o64["alpha"])),
                                      ("gradient_norm", out["gradient_norm"], float(z[f"e{e}_Misc_gradient_norm"]), float(o64["g"].norm())),
                                      ("H_inv_g", out["H_inv_g"], float(z[f"e{e}_Misc_H_inv_g"]), float(o64["x"].norm())),
                                      ("final_step_norm", out["final_step_norm"], float(z[f"e{e}_Misc_FinalStepNorm"]), step64)):
            g = G.gate(hip, ref32, v64, f"epoch {e} {name}", norms=G.MAX)
            worst[name] = max(worst.get(name, 0.0), g.d_hip / (abs(v64) + 1e-30))
        th_hip = eng.theta_actor.double().cpu().numpy()
        th64 = R.actor_flat_params(ref64.actor).numpy()
        th32 = np.concatenate([z[f"e{e}_actor_after_{k}"].reshape(-1) for k in pol.actor.state_dict()]).astype(np.float64)
        G.gate(th_hip, th32, th64, f"epoch {e} theta", rel_floor=1e-7, norms=G.L2)
        g = G.gate(th_hip, th32, th64, f"epoch {e} theta", norms=G.MAX)
        worst["theta"] = max(worst.get("theta", 0.0), g.d_hip / g.scale)
    print("cpo trace, per-epoch relative distance to float64:", {k: f"{v:.2e}" for k, v in worst.items()})


@pytest.mark.parametrize("algo", ["cpo", "pcpo", "natural_pg", "trpo", "rcpo", "trpo_lag", "cpo_humanoid", "cpo_car", "cpo_humanoid_b128",
                                  "pcpo_humanoid", "trpo_lag_humanoid"])
def test_second_order_family_traces_under_the_fp64_yardstick(dev, golden_dir, algo):
    """every trust-region script of the reference under the gate cpo got in round 4, critic fit included.
    The reference's main() trace is replayed with the ACTOR reset to the reference's recorded parameters at every epoch (its
    step carries no optimiser state) and the two CRITICS + their Adam state running free through all epochs, on the HIP path and
    by the oracle in float64 (tests/envelope.py::replay_second_order_trace; in float32 that replay reproduces the reference's
    recorded numbers bit for bit on the build box).  With the reference's RECORDED float32 numbers as the float32 leg:
      * x^T H x, alpha, |g|, |H^-1 g|, the step norm, the KL and the logged actor loss: relative distance to float64 at most
        3 x the largest the reference itself shows for that quantity over the epochs (+ 1e-6);
      * the actor after the step, the critics before every epoch and at the end: max-norm and L2 gates (3 x + floor);
      * the critic fit's per-minibatch losses: the loss envelope per epoch;
      * the discrete decisions (optimisation case, accepted line-search candidate) equal.
    The free-running replays below (5e-3) stay as trajectory checks."""
    import envelope as E
    from safepo.common.lagrange import Lagrange
    # "cpo_humanoid" (round 5): the reference's cpo.main() with ActorVCritic(376, 17) -- WideCPOEngine: surrogate gradients,
    # Fisher-vector products and line search on the wide kernels, the critic fit on the feature-split kernel
    # "cpo_car": the same at Car-class dims (72 / 2): wide actor step, critic fit on the persistent two-critic kernel (KIN = 128)
    # "cpo_humanoid_b128": 376 / 17 with the reference's default 128-row critic-fit minibatches (the kernel's two-chunk path)
    # "pcpo_humanoid", "trpo_lag_humanoid": pcpo.main() / trpo_lag.main() at 376 / 17 (projection step; line search + multiplier)
    algo, fname = {"cpo_humanoid": ("cpo", "cpo_trace_humanoid.npz"), "cpo_car": ("cpo", "cpo_trace_car.npz"),
                   "cpo_humanoid_b128": ("cpo", "cpo_trace_humanoid_b128.npz"),
                   "pcpo_humanoid": ("pcpo", "pcpo_trace_humanoid.npz"),
                   "trpo_lag_humanoid": ("trpo_lag", "trpo_lag_trace_humanoid.npz")}.get(algo, (algo, f"{algo}_trace.npz"))
    z = np.load(os.path.join(golden_dir, fname))
    N, T, epochs = int(z["meta_num_envs"]), int(z["meta_T"]), int(z["meta_epochs"])
    iters = int(z["meta_cfg_learning_iters"])
    pol, eng = _cpo_engine(z, "init_sd_", dev, N, T, {"learning_iters": iters, "batch_size": int(z["e0_batch_size"]),
                                                       "target_kl": float(z["meta_cfg_target_kl"])})
    wide = type(eng).__name__ == "WideCPOEngine"
    assert wide == fname.endswith(("_humanoid.npz", "_car.npz", "_b128.npz"))
    # wide: tests/envelope.py::adam_noise_directions; max-norm floor 5e-6 of the critics' scale after Adam steps behind a 376-wide
    # first layer (an MFMA accumulator chains 94 sequential products where the reference's blocked sgemm sums 16-wide partials:
    # tests/envelope.py::theta_floor measures the same factor of ~5 on the maximum with the L2 distance inside 3 x)
    nd = {"noise_directions": True, "rel_floor": 5e-6} if wide else {"rel_floor": 1e-6}
    o64, crit64_final = E.replay_second_order_trace(z, algo, torch.float64)
    lagrange = Lagrange(cost_limit=float(z["meta_arg_cost_limit"]),
                        lagrangian_multiplier_init=float(z["meta_arg_lagrangian_multiplier_init"]),
                        lagrangian_multiplier_lr=float(z["meta_arg_lagrangian_multiplier_lr"])) if algo in ("rcpo", "trpo_lag") else None
    n_act = sum(v.numel() for v in pol.actor.state_dict().values())
    n_crit = pol.theta.numel() - n_act
    kinds = {k: [] for k in ("xHx", "alpha", "gradient_norm", "H_inv_g", "final_step_norm", "kl", "loss_actor")}
    logged = {"xHx": "Misc_xHx", "alpha": "Misc_Alpha", "gradient_norm": "Misc_gradient_norm", "H_inv_g": "Misc_H_inv_g",
              "final_step_norm": "Misc_FinalStepNorm", "kl": "Train_KL", "loss_actor": "Loss_Loss_actor"}
    worst = {}
    for e in range(epochs):
        ref_before = np.concatenate([z[f"e{e}_sd_before_{k}"].reshape(-1) for k in pol.state_dict()])
        worst[f"critics before {e}"] = E.gate_array(pol.theta[:n_crit].cpu().numpy(), ref_before[:n_crit], o64[e]["critics_before"],
                                                    f"{algo}: critics before epoch {e}", **nd)[0]
        pol.load_state_dict({"actor." + k: torch.from_numpy(z[f"e{e}_sd_before_actor.{k}"].copy()) for k in pol.actor.state_dict()},
                            strict=False)
        _load_epoch_into_engine(z, e, eng, dev)
        ep_costs = float(z[f"e{e}_get_stats_Metrics_EpCost"]) - float(z["meta_arg_cost_limit"])
        if algo == "cpo":
            eng.buffer.compute_gae(None)
            out = eng.policy_update(ep_costs)
        elif algo == "pcpo":
            eng.buffer.compute_gae(None)
            out = eng.pcpo_update(ep_costs)
        else:
            if lagrange is not None:
                lagrange.update_lagrange_multiplier(float(z[f"e{e}_get_stats_Metrics_EpCost"]))
                eng.buffer.compute_gae(lagrange.lagrangian_multiplier)
                adv = eng.buffer.adv_mix.reshape(-1)
            else:
                eng.buffer.compute_gae(None)
                adv = eng.buffer.data["adv_r"].reshape(-1)
            out = eng.trust_region_update(adv, algo in ("trpo", "trpo_lag"))
        r64 = o64[e]
        if r64["accept"] is not None:
            assert out["acceptance_step"] == r64["accept"] == int(z[f"e{e}_Misc_AcceptanceStep"]), (e, out["acceptance_step"], r64["accept"])
        if r64["case"] is not None:
            assert out["case"] == r64["case"], (e, out["case"], r64["case"])
        for k in kinds:
            kinds[k].append((f"epoch {e}", float(out[k]), float(z[f"e{e}_{logged[k]}"]), r64[k]))
        act_ref = np.concatenate([z[f"e{e}_actor_after_{k}"].reshape(-1) for k in pol.actor.state_dict()])
        worst[f"actor after {e}"] = E.gate_array(eng.theta_actor.cpu().numpy(), act_ref, r64["actor_after"],
                                                 f"{algo}: actor after the step of epoch {e}", rel_floor=1e-6)[0]
        perms = [torch.from_numpy(z[f"e{e}_perm{i}"].astype(np.int32)).to(dev) for i in range(iters)]
        fit = eng.critic_fit(perm_fn=lambda it: perms[it])
        eng.buffer.reset()
        got = torch.cat(fit["losses"], 0).cpu().numpy()
        worst[f"critic losses {e}"] = E.assert_loss_envelope(got, z[f"e{e}_mb_losses"][:, :2], r64["critic_losses"],
                                                             f"{algo}: critic-fit losses of epoch {e}", window=len(got))
    ref_final = np.concatenate([z[f"final_sd_{k}"].reshape(-1) for k in pol.state_dict()])
    worst["critics final"] = E.gate_array(pol.theta[:n_crit].cpu().numpy(), ref_final[:n_crit], crit64_final, f"{algo}: critics at the end",
                                          **nd)[0]
    for k, rows in kinds.items():
        # (the logged actor loss is a mean over standardised advantages at ratio 1 -- zero up to rounding: measured against
        #  the advantages' unit scale)
        worst[k] = E.gate_scalars(rows, f"{algo} {k}", rel_floor=1e-6, scale=1.0 if k == "loss_actor" else None)
    print(f"{algo}: yardstick report", {k: (f"{v:.2e}" if isinstance(v, float) else tuple(f"{x:.2e}" for x in v)) for k, v in worst.items()})


def test_pcpo_update_vs_reference_main_trace(dev, golden_dir):
    """Replays the reference pcpo.main(): two CG solves, the projection step, line search (incl. an epoch that
    backtracks six times), actor parameters after the step, critic fit with the recorded shuffles."""
    z = np.load(os.path.join(golden_dir, "pcpo_trace.npz"))
    N, T, epochs = int(z["meta_num_envs"]), int(z["meta_T"]), int(z["meta_epochs"])
    pol, eng = _cpo_engine(z, "init_sd_", dev, N, T, {"learning_iters": int(z["meta_cfg_learning_iters"]),
                                                       "batch_size": int(z["e0_batch_size"]),
                                                       "target_kl": float(z["meta_cfg_target_kl"])})
    steps = []
    for e in range(epochs):
        _load_epoch_into_engine(z, e, eng, dev)
        eng.buffer.compute_gae(None)
        ep_costs = float(z[f"e{e}_get_stats_Metrics_EpCost"]) - float(z["meta_arg_cost_limit"])
        out = eng.pcpo_update(ep_costs)
        steps.append(out["acceptance_step"])
        assert out["acceptance_step"] == int(z[f"e{e}_Misc_AcceptanceStep"])
        assert out["xHx"] == pytest.approx(float(z[f"e{e}_Misc_xHx"]), rel=5e-3)
        assert out["H_inv_g"] == pytest.approx(float(z[f"e{e}_Misc_H_inv_g"]), rel=5e-3)
        assert out["gradient_norm"] == pytest.approx(float(z[f"e{e}_Misc_gradient_norm"]), rel=1e-4)
        assert out["final_step_norm"] == pytest.approx(float(z[f"e{e}_Misc_FinalStepNorm"]), rel=5e-3)
        assert out["alpha"] == pytest.approx(float(z[f"e{e}_Misc_Alpha"]), rel=5e-3)
        assert out["kl"] == pytest.approx(float(z[f"e{e}_Train_KL"]), rel=2e-2)
        act_ref = np.concatenate([z[f"e{e}_actor_after_{k}"].reshape(-1) for k in pol.actor.state_dict()])
        np.testing.assert_allclose(eng.theta_actor.cpu().numpy(), act_ref, rtol=5e-3, atol=3e-5)
        iters = int(z["meta_cfg_learning_iters"])
        perms = [torch.from_numpy(z[f"e{e}_perm{i}"].astype(np.int32)).to(dev) for i in range(iters)]
        fit = eng.critic_fit(perm_fn=lambda it: perms[it])
        eng.buffer.reset()
        got = torch.cat(fit["losses"], 0).cpu().numpy()
        np.testing.assert_allclose(got, z[f"e{e}_mb_losses"][:, :2], rtol=2e-3, atol=1e-5)
    assert max(steps) > 1
    ref_final = np.concatenate([z[f"final_sd_{k}"].reshape(-1) for k in pol.state_dict()])
    _assert_params_close(pol.theta.cpu().numpy(), ref_final, 1e-3, 12, rtol=5e-3, atol=5e-5, what="final theta")


def test_cpo_critic_fit_two_launch_form_vs_oracle_and_one_launch_form(dev, monkeypatch):
    """Critic fit at the reference batch of 128 on one GPU: two co-resident persistent launches, each with 64 of every 128
    rows, exchanging the gradient inside the step (CPOEngine._split_setup).  Against the CPU restatement of
    cpo.py:534-571 (incl. the stale actor gradient in the joint clip) and against the one-launch form of the same steps."""
    from safepo.single_agent.cpo import CPOEngine, default_cfg
    from safepo.common.model import ActorVCritic
    M, D, A, iters = 2048, 60, 8, 3
    obs, _act, _lp, tgt_r, tgt_c, _adv = _synthetic_update_problem(M, D, A, seed=21)
    g = torch.Generator().manual_seed(5)
    perms = [torch.randperm(M, generator=g).to(torch.int32) for _ in range(iters)]
    cfg = dict(default_cfg)
    cfg.update(learning_iters=iters, batch_size=128)

    def run(split: bool):
        monkeypatch.setenv("SPO_CPO_SPLIT", "force" if split else "0")   # "0": spo_critic_fit_iter = the row-split kernel (round 6)
        torch.manual_seed(11)
        pol = ActorVCritic(D, A).to(dev)
        eng = CPOEngine(pol, 1, M, cfg, dev)
        b = eng.buffer
        b.data["obs"].copy_(obs.view(1, M, D)); b.data["target_value_r"].copy_(tgt_r.view(1, M)); b.data["target_value_c"].copy_(tgt_c.view(1, M))
        eng.stale_sq.fill_(2500.0)                     # a stale actor gradient of norm 50: the joint clip (40) is active
        init = {k: v.cpu().clone() for k, v in pol.state_dict().items()}
        fit = eng.critic_fit(perm_fn=lambda it: perms[it].to(dev))
        assert (eng._split is not False and eng._split is not None) == split
        return init, pol.theta.cpu().clone(), torch.cat(fit["losses"], 0).cpu()
    init, th_split, loss_split = run(True)
    _, th_one, loss_one = run(False)

    def oracle(dtype):
        ref = R.OraclePolicy(D, A)
        ref.load_state_dict(init)
        ref = ref.to(dtype)
        # the stale actor gradient: any vector of norm 50 on the actor's .grad (only its norm enters the critics' clip)
        n_act_ = sum(p.numel() for p in ref.actor.parameters())
        for p in ref.actor.parameters():
            p.grad = torch.full_like(p, 50.0 / np.sqrt(n_act_))
        fitter = R.CriticFitter(ref)
        o_, tr_, tc_ = obs.to(dtype), tgt_r.to(dtype), tgt_c.to(dtype)
        want_losses = []
        for it in range(iters):
            pm = perms[it].long()
            for k in range(M // 128):
                idx = pm[k * 128:(k + 1) * 128]
                want_losses.append(fitter.minibatch_step(o_[idx], tr_[idx], tc_[idx]))
        return np.asarray(want_losses, np.float64), torch.cat([p.detach().reshape(-1) for p in ref.parameters()]).double().numpy(), n_act_
    # both forms under the drift envelope (round 5: instead of rtol 2e-4 / 2e-3 with 0.1 % of the parameters exempt): float64 =
    # the oracle's critic fit in double, float32 = the same in the reference's arithmetic
    import envelope as E
    l32, th32, n_act = oracle(torch.float32)
    l64, th64, _ = oracle(torch.float64)
    n_crit = th_split.numel() - n_act
    np.testing.assert_allclose(loss_split.numpy()[:4], l32[:4], rtol=1e-5, atol=1e-6)      # first steps from identical weights
    for name, th, ls in (("split", th_split, loss_split), ("one launch", th_one, loss_one)):
        E.assert_loss_envelope(ls.numpy(), l32, l64, f"critic fit, {name} form: losses", window=len(l32))
        E.assert_theta_envelope(th.numpy()[:n_crit], th32[:n_crit], th64[:n_crit], f"critic fit, {name} form: critics")


def test_cpo_full_size_surrogate_gradients_and_fvp_fp64_yardstick(dev):
    """BASELINE config 3 at ITS size: the two surrogate gradients and one Fisher-vector product over all
    4096 x 128 = 524 288 rows -- the shape the 821 k env-steps/s line runs (256 workgroups x 2048 rows, per-workgroup
    partial vectors, fixed-order reduction) -- against the oracle's autograd / double backward (cpo.py:132-157, 356-378) in
    float64 (yardstick) and float32 (the reference's arithmetic): |HIP - f64| <= 3 |f32 - f64| + floor."""
    import copy
    from safepo.single_agent.cpo import CPOEngine, default_cfg
    from safepo.common.model import ActorVCritic
    torch.set_num_threads(8)
    torch.manual_seed(31)
    N, T, D, A = 4096, 128, 60, 8
    M = N * T
    pol = ActorVCritic(D, A).to(dev)
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    eng = CPOEngine(pol, N, T, dict(default_cfg), dev)
    obs, act, logp, _, _, adv = _synthetic_update_problem(M, D, A, seed=33)
    adv_c = adv.flip(0) * 0.5 + 0.1
    b = eng.buffer
    b.data["obs"].copy_(obs.view(N, T, D)); b.data["act"].copy_(act.view(N, T, A)); b.data["log_prob"].copy_(logp.view(N, T))
    b.data["adv_r"].copy_(adv.view(N, T)); b.data["adv_c"].copy_(adv_c.view(N, T))
    ref32 = R.OraclePolicy(D, A)
    ref32.load_state_dict({k: v.cpu().clone() for k, v in pol.state_dict().items()})
    ref64 = copy.deepcopy(ref32).double()
    data32 = {"obs": obs, "act": act, "log_prob": logp, "adv_r": adv, "adv_c": adv_c}
    data64 = {k: v.double() for k, v in data32.items()}

    def gate(name, hip, v32, v64, floor_rel=2e-7):
        G.gate(hip, v32, v64, f"cpo full size {name}", rel_floor=floor_rel, norms=G.L2)
        G.gate(hip, v32, v64, f"cpo full size {name}", floor=floor_rel * np.abs(v64).max() * 8, norms=G.MAX)

    for which, key, sign in (("r", "adv_r", -1.0), ("c", "adv_c", 1.0)):
        outs = []
        for ref, data in ((ref32, data32), (ref64, data64)):
            ref.actor.zero_grad()
            loss = R.cpo_surrogate(ref, data, which)
            loss.backward()
            outs.append((R.actor_flat_grads(ref.actor).double().numpy().copy(), float(loss.detach())))
        g, mean = eng.surrogate_grad(b.data[key], sign)
        gate(f"surrogate gradient {which}", g.cpu().numpy(), outs[0][0], outs[1][0])
        # the surrogate value is a mean of O(1) terms that cancel to ~1e-3: its rounding floor is relative to the terms'
        # magnitude mean|ratio * adv|, not to the cancelled mean
        with torch.no_grad():
            lp64 = ref64.actor(data64["obs"]).log_prob(data64["act"]).sum(-1)
            term_scale = float((torch.exp(lp64 - data64["log_prob"]) * data64[key]).abs().mean())
        G.gate(sign * mean, outs[0][1], outs[1][1], f"cpo full size surrogate value {which}", scale=term_scale, rel_floor=1e-7, norms=G.MAX)
    v = torch.randn(eng.Pa, generator=torch.Generator().manual_seed(5))
    hv32 = R.cpo_fvp(v, ref32, obs).double().numpy()
    hv64 = R.cpo_fvp(v.double(), ref64, obs.double()).numpy()
    gate("Fisher-vector product", eng.fvp(v.to(dev)).cpu().numpy(), hv32, hv64)
    # the same product again (workspace reuse) and linearity: H(2v) == 2 H(v) to rounding
    h1 = eng.fvp(v.to(dev)); h2 = eng.fvp((2 * v).to(dev))
    assert torch.equal(h1, eng.fvp(v.to(dev)))
    np.testing.assert_allclose(h2.cpu().numpy(), 2 * h1.cpu().numpy(), rtol=1e-5, atol=1e-7 * float(h1.abs().max()))


def _oracle_critic_trajectory(sd, obs, tgt_r, tgt_c, perm, batch, nsteps, dtype, checkpoints, stale_norm):
    """`nsteps` consecutive critic-fit steps of the oracle (R.CriticFitter, cpo.py:541-571) in `dtype`; the actor's stale
    gradient has norm `stale_norm`.  Returns (losses [nsteps, 2], {k: critic parameters after k steps}) as float64."""
    D, A = obs.shape[1], sd["actor.log_std"].shape[0]
    ref = R.OraclePolicy(D, A)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in sd.items()})
    ref = ref.to(dtype)
    n_act = sum(p.numel() for p in ref.actor.parameters())
    for p_ in ref.actor.parameters():
        p_.grad = torch.full_like(p_, stale_norm / np.sqrt(n_act))
    fitter = R.CriticFitter(ref)
    obs, tgt_r, tgt_c = obs.to(dtype), tgt_r.to(dtype), tgt_c.to(dtype)
    perm = torch.as_tensor(perm, dtype=torch.long)
    losses, thetas = np.zeros((nsteps, 2)), {}
    crit = lambda: torch.cat([p_.detach().reshape(-1) for p_ in list(ref.reward_critic.parameters()) + list(ref.cost_critic.parameters())])
    for s_ in range(nsteps):
        ii = perm[s_ * batch:(s_ + 1) * batch]
        losses[s_] = fitter.minibatch_step(obs[ii], tgt_r[ii], tgt_c[ii])
        if (s_ + 1) in checkpoints:
            thetas[s_ + 1] = crit().double().numpy().copy()
    return losses, thetas


_CRITIC_ENVELOPE_CACHE = {}


@pytest.mark.parametrize("form", ["split_one_grid", "one_launch"])
def test_cpo_full_size_critic_fit_drift_envelope(dev, form, monkeypatch):
    """BASELINE config 3's critic fit at its size: ONE persistent launch of 4096 steps of 128 rows over
    the 4096 x 128 buffer (cpo.py:534-571, stale actor gradient of norm 50 in the joint clip), in the split form (two
    workgroup pairs of one grid, 64 of every 128 rows each) and in the one-launch form, under the same drift envelope as
    the PPO-Lagrangian step: per-step losses and the critics' parameters after 8 / 64 / 512 / 4096 steps may be at most
    3x as far from the oracle's float64 trajectory as the oracle's float32 trajectory is; first 8 steps at 1e-5."""
    import envelope as E
    from safepo.single_agent.cpo import CPOEngine, default_cfg
    from safepo.common.model import ActorVCritic
    monkeypatch.setenv("SPO_CPO_SPLIT", "force" if form == "split_one_grid" else "0")   # one_launch: the row-split kernel (round 6)
    torch.set_num_threads(8)
    N, T, D, A, batch = 4096, 128, 60, 8, 128
    M = N * T
    ks = (8, 64, 512, 4096)
    obs, _a, _l, tgt_r, tgt_c, _adv = _synthetic_update_problem(M, D, A, seed=41)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(6)).to(torch.int32)
    torch.manual_seed(17)
    pol = ActorVCritic(D, A).to(dev)
    cfg = dict(default_cfg)
    cfg.update(learning_iters=1, batch_size=batch)
    eng = CPOEngine(pol, N, T, cfg, dev)
    bd = eng.buffer.data
    bd["obs"].copy_(obs.view(N, T, D)); bd["target_value_r"].copy_(tgt_r.view(N, T)); bd["target_value_c"].copy_(tgt_c.view(N, T))
    sd0 = {k: v.detach().cpu().clone() for k, v in pol.state_dict().items()}
    theta0 = pol.theta.clone()
    perm_dev = perm.to(dev)
    n_crit = pol.log_std_offset                      # reward critic + cost critic come first in the flat vector
    hip = {}
    for k in ks:
        pol.theta.copy_(theta0); eng.adam_m.zero_(); eng.adam_v.zero_(); eng.adam_step = 0
        eng.stale_sq.fill_(2500.0)
        eng.M = k * batch
        fit = eng.critic_fit(perm_fn=lambda it: perm_dev[:k * batch].contiguous())
        assert (eng._split is not False and eng._split is not None) == (form == "split_one_grid")
        hip[k] = (pol.theta[:n_crit].double().cpu().numpy(), torch.cat(fit["losses"], 0).double().cpu().numpy())
    eng.M = M
    kmax = max(ks)
    if "traj" not in _CRITIC_ENVELOPE_CACHE:             # same seeds in both parametrisations: the oracle runs once
        _CRITIC_ENVELOPE_CACHE["traj"] = (
            _oracle_critic_trajectory(sd0, obs, tgt_r, tgt_c, perm, batch, kmax, torch.float32, ks, 50.0),
            _oracle_critic_trajectory(sd0, obs, tgt_r, tgt_c, perm, batch, kmax, torch.float64, ks, 50.0),
            {k: v.clone() for k, v in sd0.items()})
    (l32, t32), (l64, t64), sd_c = _CRITIC_ENVELOPE_CACHE["traj"]
    assert all(torch.equal(sd_c[k], sd0[k]) for k in sd0)
    lh = hip[kmax][1]
    np.testing.assert_allclose(lh[:8], l32[:8], rtol=1e-5, atol=1e-6, err_msg=f"{form}: first 8 critic-fit steps")
    r_loss = E.assert_loss_envelope(lh, l32, l64, f"critic fit ({form})")
    rep = {}
    for k in ks:
        assert np.array_equal(hip[k][1], lh[:k]), f"{form}: the {k}-step launch is not a prefix of the {kmax}-step launch"
        rep[k] = E.assert_theta_envelope(hip[k][0], t32[k], t64[k], f"critic fit ({form}): critics after {k} steps")
    print(f"critic fit envelope ({form}): loss ratio {r_loss:.2f}; theta " +
          "; ".join(f"k={k}: ratio {rep[k][0]:.2f} |hip-f64| {rep[k][1]['l2_hip']:.2e} |f32-f64| {rep[k][1]['l2_f32']:.2e}" for k in ks))


def test_cpo_main_entrypoint_synthetic(dev, tmp_path):
    import argparse
    import csv
    from safepo.single_agent import cpo
    args = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=16, experiment="t",
                              log_dir=str(tmp_path / "exp" / "task" / "run"), device="cuda", device_id=0,
                              write_terminal=True, headless=False, total_steps=2 * 16 * 64, steps_per_epoch=16 * 64,
                              randomize=False, cost_limit=25.0, lagrangian_multiplier_init=0.001,
                              lagrangian_multiplier_lr=0.035, cfg_override={"learning_iters": 2},
                              env_kwargs={"trunc_len": 16})
    cpo.main(args, {})
    rows = list(csv.DictReader(open(tmp_path / "exp" / "task" / "run" / "progress.csv")))
    assert len(rows) == 2
    for col in ("Metrics/EpRet", "Train/KL", "Loss/Loss_actor", "Misc/Alpha", "Misc/FinalStepNorm", "Misc/xHx",
                "Misc/gradient_norm", "Misc/H_inv_g", "Misc/AcceptanceStep", "Time/Update"):
        assert col in rows[0], col
    assert float(rows[0]["Misc/xHx"]) >= 0


def test_crosslane_helpers_selftest(dev):
    """DPP row sums and gfx950 permlane-swap reductions used inside the MFMA kernels."""
    from safepo import _abi
    x = torch.randn(64)
    out = torch.zeros(192, device=dev)
    xin = x.to(dev)
    _abi.check(_abi.load().spo_debug_crosslane_selftest(_abi.ptr(xin), _abi.ptr(out), _abi.stream_ptr()), "selftest")
    o = out.cpu().numpy()
    xn = x.numpy().reshape(4, 16)
    np.testing.assert_allclose(o[:64].reshape(4, 16), np.broadcast_to(xn.sum(0), (4, 16)), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(o[64:128].reshape(4, 16)[:, 15], xn.sum(1), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(o[128 + 63], xn.sum(), rtol=1e-6, atol=1e-6)


def test_host_env_path_through_main(dev, tmp_path):
    """Host (numpy) vector env with object-array final_observation, as gymnasium provides it."""
    import argparse
    import csv
    from safepo.single_agent import ppo_lag
    args = argparse.Namespace(seed=1, use_eval=False, task="SynthHost-v0", num_envs=6, experiment="t",
                              log_dir=str(tmp_path / "exp" / "task" / "run"), device="cuda", device_id=0,
                              write_terminal=True, headless=False, total_steps=6 * 40, steps_per_epoch=6 * 40,
                              randomize=False, cost_limit=25.0, lagrangian_multiplier_init=0.001,
                              lagrangian_multiplier_lr=0.035, cfg_override={"learning_iters": 2},
                              env_kwargs={"trunc_len": 9, "p_term": 0.05, "obs_dim": 17, "act_dim": 3})
    out = ppo_lag.main(args, {})
    rows = list(csv.DictReader(open(tmp_path / "exp" / "task" / "run" / "progress.csv")))
    assert len(rows) == 1 and float(rows[0]["Metrics/EpLen"]) <= 9.0
    b = out["engine"].buffer
    assert b.seg_end[:, -1].all()
    assert torch.isfinite(out["policy"].theta).all()


def test_forced_data_parallel_path_equals_persistent(dev, monkeypatch):
    """engine.learning_iter through the split grad / all-reduce / clip+Adam loop (world size 1) gives
    the same parameters and per-minibatch losses as the persistent kernel."""
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    M, D, A = 200, 60, 8
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=2)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 40.0}
    res = []
    for forced in ("0", "1"):
        monkeypatch.setenv("SPO_FORCE_DP", forced)
        torch.manual_seed(5)
        pol = ActorVCritic(D, A).to(dev)
        eng = PPOLagEngine(pol, 1, M, cfg, dev)
        b = eng.buffer
        b.data["obs"].copy_(obs.view(1, M, D)); b.data["act"].copy_(act.view(1, M, A))
        b.data["log_prob"].copy_(logp.view(1, M)); b.data["target_value_r"].copy_(tgt_r.view(1, M))
        b.data["target_value_c"].copy_(tgt_c.view(1, M)); b.adv_mix.copy_(adv.view(1, M))
        perm = torch.randperm(M, generator=torch.Generator().manual_seed(1)).to(torch.int32).to(dev)
        losses = eng.learning_iter(perm)
        res.append((pol.theta.cpu().numpy(), losses.cpu().numpy(), eng.adam_step))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(res[0][1], res[1][1], rtol=1e-5, atol=1e-7)
    assert res[0][2] == res[1][2] == 4


def test_limits_and_edge_shapes(dev):
    """Largest supported dims (obs 64 in the update kernels, act 16), single env / single step, and the
    loud failures outside the envelope."""
    from safepo import _abi
    from safepo.common.engine import PPOLagEngine
    from smoke_check import smoke_check
    from safepo.common.model import ActorVCritic
    pol = ActorVCritic(64, 16).to(dev)
    M = 96
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 40.0}
    eng = PPOLagEngine(pol, 1, M, cfg, dev)
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, 64, 16, seed=3)
    b = eng.buffer
    b.data["obs"].copy_(obs.view(1, M, 64)); b.data["act"].copy_(act.view(1, M, 16)); b.data["log_prob"].copy_(logp.view(1, M) - 10)
    b.data["target_value_r"].copy_(tgt_r.view(1, M)); b.data["target_value_c"].copy_(tgt_c.view(1, M)); b.adv_mix.copy_(adv.view(1, M))
    ref = R.OraclePolicy(64, 16)
    ref.load_state_dict({k: v.cpu().clone() for k, v in pol.state_dict().items()})
    ref0 = {k: v.clone() for k, v in ref.state_dict().items()}
    upd = R.PPOLagUpdater(ref, epochs=1)
    perm = torch.arange(M)
    lr = [upd.minibatch_step(obs[s:s + 64], act[s:s + 64], logp[s:s + 64] - 10, tgt_r[s:s + 64], tgt_c[s:s + 64], adv[s:s + 64])
          for s in range(0, M, 64)]
    losses = eng.learning_iter(perm.to(torch.int32).to(dev))
    np.testing.assert_allclose(losses.cpu().numpy(), np.asarray(lr), rtol=1e-4, atol=2e-6)
    import envelope as E
    _, t64 = E.oracle_trajectory(ref0, (obs, act, logp - 10, tgt_r, tgt_c, adv), perm, 64, 2, torch.float64, [2])
    E.assert_theta_envelope(pol.theta.cpu().numpy(), R.flat_params(ref).numpy(), t64[2], "64x16: theta after 2 steps")
    # outside the envelope of the LDS-resident kernels: ROUTED to the wide path (tests/test_gpu_wide_dims.py), not refused;
    # the C entry points themselves still fail loudly when called with dims they are not built for
    from safepo.single_agent.cpo import CPOEngine, WideCPOEngine, make_engine, default_cfg as cpo_cfg
    assert type(make_engine(ActorVCritic(100, 4).to(dev), 2, 8, dict(cpo_cfg), dev)) is WideCPOEngine
    with pytest.raises(NotImplementedError, match="obs_dim <= 64"):
        CPOEngine(ActorVCritic(100, 4).to(dev), 2, 8, dict(cpo_cfg), dev)
    lib, z = _abi.load(), torch.zeros(4096, device=dev)
    with pytest.raises(_abi.SpoError, match="obs_dim"):
        _abi.check(lib.spo_values(_abi.ptr(z), _abi.ptr(z), _abi.ptr(z), _abi.ptr(z), 2, 129, 4, None), "spo_values")
    with pytest.raises(_abi.SpoError, match="act_dim"):
        _abi.check(lib.spo_values(_abi.ptr(z), _abi.ptr(z), _abi.ptr(z), _abi.ptr(z), 2, 10, 17, None), "spo_values")
    with pytest.raises(_abi.SpoError, match="obs_dim"):
        _abi.check(lib.spo_cpo_fvp(_abi.ptr(z), _abi.ptr(z), _abi.ptr(z), 2, 100, 4, _abi.ptr(z), _abi.ptr(z), _abi.ptr(z), None), "spo_cpo_fvp")
    smoke_check(num_envs=1, steps=3, seed=3)     # (M=1 gives std()=NaN in the reference too)


def test_obs_normalizer_vs_oracle_running_mean_std(dev):
    """a-2: device RunningMeanStd update + normalise against the numpy restatement of gymnasium's algorithm."""
    from safepo.common.env import DeviceObsNormalizer
    rng = np.random.default_rng(0)
    D = 60
    norm = DeviceObsNormalizer(D, dev)
    ref = R.RunningMeanStd((D,))
    for step, n in enumerate((4096, 4096, 7, 300)):
        x = (rng.standard_normal((n, D)) * (1 + np.arange(D)) + 3.0 * np.arange(D)).astype(np.float32)
        want = ref.normalize(x.astype(np.float64)).astype(np.float32)
        got = norm.normalize_(torch.from_numpy(x.copy()).to(dev)).cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
    rms = norm.obs_rms
    np.testing.assert_allclose(rms.mean, ref.mean, rtol=1e-10)
    np.testing.assert_allclose(rms.var, ref.var, rtol=1e-10)
    assert rms.count == pytest.approx(ref.count)
    # frozen statistics (evaluation mode): no update
    x = rng.standard_normal((5, D)).astype(np.float32)
    got = norm.normalize_(torch.from_numpy(x.copy()).to(dev), update=False).cpu().numpy()
    np.testing.assert_allclose(got, ((x - ref.mean) / np.sqrt(ref.var + 1e-8)).astype(np.float32), rtol=1e-5, atol=1e-5)


def test_fused_normalise_policy_step_vs_oracle(dev, tmp_path):
    """a-1 + a-2 fused (spo_policy_step_norm): RAW observations in; statistics merged, rows normalised on load, networks
    evaluated, buffer slot and the caller's tensor filled with the normalised rows -- against the restated
    RunningMeanStd / normalize (float64, rounded to fp32 once) followed by the oracle policy step on the normalised rows."""
    import argparse
    from safepo.common.engine import PPOLagEngine
    from safepo.common.env import DeviceObsNormalizer
    from safepo.common.model import ActorVCritic
    rng = np.random.default_rng(1)
    N, T, D, A = 300, 3, 60, 8
    torch.manual_seed(5)
    pol = ActorVCritic(D, A).to(dev)
    ref = R.OraclePolicy(D, A)
    ref.load_state_dict({k: v.cpu().clone() for k, v in pol.state_dict().items()})
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 0.02, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 40.0}
    eng = PPOLagEngine(pol, N, T, cfg, dev)
    norm = DeviceObsNormalizer(D, dev)
    rms = R.RunningMeanStd((D,))
    for t in range(T):
        x = (rng.standard_normal((N, D)) * (1 + 0.2 * np.arange(D)) + 0.5 * np.arange(D)).astype(np.float32)
        eps = rng.standard_normal((N, A)).astype(np.float32)
        want = rms.normalize(x.astype(np.float64)).astype(np.float32)          # update, then normalise
        obs = torch.from_numpy(x.copy()).to(dev)
        norm.pending = True
        act = eng.collect_step(t, obs, torch.from_numpy(eps).to(dev), rms=norm)
        assert not norm.pending
        got = obs.cpu().numpy()
        assert _ulp_diff(got, want).max() <= 1, "normalised rows (in place)"
        assert np.array_equal(eng.buffer.data["obs"][:, t].cpu().numpy(), got), "buffer slot holds the normalised rows"
        with torch.no_grad():
            a_ref, lp_ref, vr_ref, vc_ref = ref.step_with_eps(torch.from_numpy(got), torch.from_numpy(eps))
        np.testing.assert_allclose(act.cpu().numpy(), a_ref.numpy(), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(eng.logp.cpu().numpy(), lp_ref.numpy(), rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose(eng.v_r.cpu().numpy(), vr_ref.numpy(), rtol=1e-5, atol=1e-5)
        eng.buffer.advance()
    st = norm.obs_rms
    np.testing.assert_allclose(st.mean, rms.mean, rtol=1e-12)
    np.testing.assert_allclose(st.var, rms.var, rtol=1e-12)
    assert st.count == pytest.approx(rms.count)
    # second call on the same tensor: nothing pending -> the plain step, no second normalisation
    eng.buffer.reset()
    obs2 = obs.clone()
    eng.collect_step(0, obs2, torch.zeros((N, A), device=dev), rms=norm)
    assert torch.equal(obs2, obs)
    # the training loop end to end with a normalising device env (fused path) + evaluation with frozen restored statistics
    from safepo.single_agent import ppo_lag
    from safepo.evaluate import eval_single_agent
    args = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=16, experiment="t",
                              log_dir=str(tmp_path / "exp" / "task" / "run"), device="cuda", device_id=0,
                              write_terminal=False, headless=False, total_steps=16 * 32 * 2, steps_per_epoch=16 * 32,
                              randomize=False, cost_limit=25.0, lagrangian_multiplier_init=0.001,
                              lagrangian_multiplier_lr=0.035,
                              env_kwargs={"normalize_obs": True, "obs_scale": 3.0, "obs_shift": 1.5, "trunc_len": 16})
    out = ppo_lag.main(args, {})
    env_rms = out["engine"] and out["policy"] is not None
    assert env_rms
    import joblib
    state = joblib.load(open(tmp_path / "exp" / "task" / "run" / "state0.pkl", "rb"))["Normalizer"]
    mean = np.asarray(state.mean if hasattr(state, "mean") else state["mean"])
    assert abs(float(mean.mean()) - 1.5) < 0.3, "running mean tracks the shifted observations (the fused path updated it)"


def test_pg_unclipped_surrogate_and_ppo_lambda_zero(dev):
    """f2 siblings on the same kernels: pg = no ratio clip (pg.py:309), ppo = lambda 0 (ppo.py:272)."""
    from safepo import _abi
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    from safepo.single_agent._first_order import NO_CLIP
    M, D, A = 64, 60, 8
    torch.manual_seed(8)
    pol = ActorVCritic(D, A).to(dev)
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=21)
    logp = logp + 0.5 * torch.randn(M)                       # push many ratios outside [0.8, 1.2]
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": 64, "learning_iters": 1,
           "max_grad_norm": 40.0, "clip": NO_CLIP}
    eng = PPOLagEngine(pol, 1, M, cfg, dev)
    b = eng.buffer
    b.data["obs"].copy_(obs.view(1, M, D)); b.data["act"].copy_(act.view(1, M, A)); b.data["log_prob"].copy_(logp.view(1, M))
    b.data["target_value_r"].copy_(tgt_r.view(1, M)); b.data["target_value_c"].copy_(tgt_c.view(1, M)); b.adv_mix.copy_(adv.view(1, M))
    ref = R.OraclePolicy(D, A)
    ref.load_state_dict({k: v.cpu().clone() for k, v in pol.state_dict().items()})
    dist = ref.actor(obs)
    ratio = torch.exp(dist.log_prob(act).sum(-1) - logp)
    assert ((ratio < 0.8) | (ratio > 1.2)).float().mean() > 0.3
    loss_pg = -(ratio * adv).mean()
    ref.actor.zero_grad()
    loss_pg.backward()
    g_ref = torch.cat([p.grad.reshape(-1) for p in ref.actor.parameters()]).numpy()
    idx = torch.arange(M, dtype=torch.int32, device=dev)
    d = b.data
    _abi.check(eng.lib.spo_ppo_lag_grad(_abi.ptr(pol.theta), _abi.ptr(d["obs"]), _abi.ptr(d["act"]), _abi.ptr(d["log_prob"]),
                                        _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(b.adv_mix),
                                        _abi.ptr(idx), M, M, eng._cfg_struct(), _abi.ptr(eng.flat_grad), _abi.ptr(eng.losses3),
                                        _abi.stream_ptr()), "grad")
    got = eng.flat_grad[pol.log_std_offset:].cpu().numpy()
    np.testing.assert_allclose(got, g_ref, rtol=1e-4, atol=1e-5 * np.abs(g_ref).max())
    assert float(eng.losses3[2]) == pytest.approx(float(loss_pg), rel=1e-5)
    # lambda == 0 leaves adv_r untouched by the mix kernel (bit pattern)
    b.data["adv_r"].copy_(adv.view(1, M)); b.data["adv_c"].copy_(tgt_c.view(1, M))
    b.sums.copy_(torch.tensor([0.0, float(M - 1), 0.0, float(M)], dtype=torch.float64))     # mean 0, std 1
    _abi.check(eng.lib.spo_adv_apply(_abi.ptr(d["adv_r"]), _abi.ptr(d["adv_c"]), _abi.ptr(b.adv_mix), _abi.ptr(b.sums), M,
                                     0.0, 0, 0, None, _abi.stream_ptr()), "apply")
    assert torch.equal(b.adv_mix.view(-1).cpu(), adv)


@pytest.mark.parametrize("algo", ["ppo", "pg", "cppo_pid", "focops", "cup"])
def test_sibling_entrypoints_synthetic(dev, tmp_path, algo):
    import argparse
    import csv
    import importlib
    mod = importlib.import_module(f"safepo.single_agent.{algo}")
    args = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=8, experiment="t",
                              log_dir=str(tmp_path / "exp" / "task" / "run"), device="cuda", device_id=0,
                              write_terminal=True, headless=False, total_steps=2 * 8 * 32, steps_per_epoch=8 * 32,
                              randomize=False, cost_limit=0.5, lagrangian_multiplier_init=0.001,
                              lagrangian_multiplier_lr=0.035, cfg_override={"learning_iters": 2},
                              env_kwargs={"trunc_len": 8, "p_cost": 0.5})
    mod.main(args, {})
    rows = list(csv.DictReader(open(tmp_path / "exp" / "task" / "run" / "progress.csv")))
    assert len(rows) == 2
    assert ("Train/LagragianMultiplier" in rows[0]) == (algo in ("cppo_pid", "focops", "cup"))
    assert ("Train/SeconStageStopIter" in rows[0]) == (algo == "cup")
    if algo == "cppo_pid":
        assert float(rows[1]["Train/LagragianMultiplier"]) > 0.0          # cost 4/episode > limit 0.5

@pytest.mark.parametrize("algo,suffix", [("focops", ""), ("cup", ""), ("focops", "_humanoid"), ("cup", "_humanoid")])
def test_kl_penalty_family_vs_reference_main_trace(dev, golden_dir, algo, suffix):
    """The epochs of the reference focops.main() / cup.main(): same buffers, shuffles and initial weights ->
    per-minibatch losses (critics + the KL-penalty actor loss with its indicator), early-stop iterations of both
    stages, KL and parameters after every epoch.  `_humanoid` (round 5): focops.main() / cup.main() with ActorVCritic(376, 17), on the
    feature-split kernel's KL-penalty instantiation (CUP's second stage: its actor-only launch)."""
    from safepo.common.engine import PPOLagEngine, WidePPOLagEngine
    z = np.load(os.path.join(golden_dir, f"{algo}_trace{suffix}.npz"))
    N, T, epochs = int(z["meta_num_envs"]), int(z["meta_T"]), int(z["meta_epochs"])
    pol = _policy_from_npz(z, "init_sd_", dev)
    cfg = {"hidden_sizes": [64, 64], "gamma": float(z["meta_cfg_gamma"]), "target_kl": float(z["meta_cfg_target_kl"]),
           "batch_size": int(z["e0_batch_size"]), "learning_iters": int(z["meta_cfg_learning_iters"]),
           "max_grad_norm": float(z["meta_cfg_max_grad_norm"])}
    wide = not pol.kernels_supported("ppo")
    eng = (WidePPOLagEngine if wide else PPOLagEngine)(pol, N, T, cfg, dev)
    assert wide == bool(suffix)
    # the drift envelope of the PPO-Lagrangian trace test: T64 = the oracle replaying the recorded inputs in float64, T32 = the
    # values the reference itself recorded (round 5: instead of rtol 2e-4 ... 5e-4 and a KL at 3e-3)
    import envelope as E
    o64, theta64_final = E.replay_kl_penalty_trace(z, algo, torch.float64)
    ratios, kl_rows = [], []
    steps_done = 0
    tk = lambda: ({"floor_abs_max": E.theta_floor(3e-4, max(steps_done, 1)), "noise_directions": True} if wide else {})
    for e in range(epochs):
        ref_before = np.concatenate([z[f"e{e}_sd_before_{k}"].reshape(-1) for k in pol.state_dict()])
        ratios.append(E.assert_theta_envelope(pol.theta.cpu().numpy(), ref_before, o64[e]["theta_before"], f"theta before epoch {e}", **tk())[0])
        _load_epoch_into_engine(z, e, eng, dev)
        lam = float(z[f"e{e}_row_Train_LagragianMultiplier"])
        n_perm = len([k for k in z.files if k.startswith(f"e{e}_perm")])
        perms = [torch.from_numpy(z[f"e{e}_perm{i}"].astype(np.int32)).to(dev) for i in range(n_perm)]
        eng.lr_factor = 1.0 - e / epochs
        perm_fn = lambda it: perms[min(it, n_perm - 1)]
        if algo == "focops":
            out = eng.update_focops(lam, perm_fn=perm_fn)
        else:
            out = eng.update_cup(lam, perm_fn=perm_fn)
            assert out["second_stage_stop_iter"] == int(z[f"e{e}_row_Train_SeconStageStopIter"])
            # parameters between the stages (recorded when the reference builds its second DataLoader)
            assert torch.isnan(torch.cat(out["second_stage_losses"], 0)[:, :2]).all()      # critics untouched
        assert out["stop_iter"] == int(z[f"e{e}_row_Train_StopIter"]) == o64[e]["stop_iter"], (out["stop_iter"], out["kl"])
        got = torch.cat(out["losses"], 0).cpu().numpy()
        ref = z[f"e{e}_mb_losses"]
        steps_done += len(ref)
        if e == 0:
            np.testing.assert_allclose(got[:3], ref[:3], rtol=1e-5, atol=1e-6)       # first steps from identical weights
        ratios.append(E.assert_loss_envelope(got, ref, o64[e]["losses"], f"losses of epoch {e}", window=len(ref)))
        kl_rows.append((f"epoch {e}", out["kl"], float(z[f"e{e}_row_Train_KL"]), o64[e]["kl"]))
    print("KL yardstick (worst hip, reference):", E.gate_scalars(kl_rows, f"{algo} Train/KL", rel_floor=1e-6))
    ref_final = np.concatenate([z[f"final_sd_{k}"].reshape(-1) for k in pol.state_dict()])
    ratios.append(E.assert_theta_envelope(pol.theta.cpu().numpy(), ref_final, theta64_final, "final theta", **tk())[0])
    print(f"{algo}: drift envelope ratios (<= 1 passes):", np.round(ratios, 3))


@pytest.mark.parametrize("M,D,A,actor_only", [(192, 60, 8, False), (150, 17, 6, True), (100, 100, 3, True),
                                               (64, 128, 16, False)])
def test_kl_penalty_minibatch_steps_vs_oracle(dev, M, D, A, actor_only):
    """One pass of KL-penalty minibatch steps (partial last batch included, indicator active on part of the batch)
    against torch autograd + Adam in the oracle; the actor's optimiser clock is ahead of the critics'."""
    from safepo import _abi
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    torch.manual_seed(M + D)
    pol = ActorVCritic(D, A).to(dev)
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    ref = R.OraclePolicy(D, A)
    ref.load_state_dict({k: v.cpu().clone() for k, v in pol.state_dict().items()})
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=M)
    with torch.no_grad():
        dist = ref.actor(obs)
        old_mean = dist.mean + 0.05 * torch.randn(M, A)          # a nearby "old" policy: KL straddles the bound
        old_std = dist.stddev * torch.exp(0.05 * torch.randn(A))
    with torch.no_grad():
        kl0 = torch.distributions.kl_divergence(dist, torch.distributions.Normal(old_mean, old_std)).sum(-1)
    kl_bound = float(kl0.quantile(0.55)) if not actor_only else float("inf")       # between two samples, not on one
    pg_coef = 1 / 1.5 if not actor_only else -0.37
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": 64, "learning_iters": 1,
           "max_grad_norm": 40.0}
    eng = PPOLagEngine(pol, 1, M, cfg, dev)
    b = eng.buffer
    b.data["obs"].copy_(obs.view(1, M, D)); b.data["act"].copy_(act.view(1, M, A))
    b.data["log_prob"].copy_(logp.view(1, M)); b.data["target_value_r"].copy_(tgt_r.view(1, M))
    b.data["target_value_c"].copy_(tgt_c.view(1, M))
    eng.mean_old.copy_(old_mean); eng.std_old.copy_(old_std[0] if old_std.dim() > 1 else old_std)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(3))
    eng.adam_step_actor_extra = 5
    theta0 = pol.theta.clone()
    ref0 = {k: v.clone() for k, v in ref.state_dict().items()}

    def oracle(dtype):
        """One pass in `dtype`; 5 earlier actor-only steps move the actor's Adam clock ahead (zero gradients leave the moments
        at 0).  Returns (losses, flat parameters, number of masked samples, smallest |KL - bound| met)."""
        rp = R.OraclePolicy(D, A)
        rp.load_state_dict(ref0)
        rp = rp.to(dtype)
        upd = R.KLPenaltyUpdater(rp)
        for _ in range(5):
            upd.opt_a.zero_grad()
            for prm in rp.actor.parameters():
                prm.grad = torch.zeros_like(prm)
            upd.opt_a.step()
        o_, a_, lp_, tr_, tc_, ad_, om_ = (t.to(dtype) for t in (obs, act, logp, tgt_r, tgt_c, adv, old_mean))
        os_full = (old_std.expand(M, A) if old_std.dim() == 1 else old_std).to(dtype)
        out, n_masked, margin = [], 0, float("inf")
        for s0 in range(0, M, 64):
            idx = perm[s0:s0 + 64]
            with torch.no_grad():
                kl_i = torch.distributions.kl_divergence(rp.actor(o_[idx]), torch.distributions.Normal(om_[idx], os_full[idx])).sum(-1)
                n_masked += int((kl_i > kl_bound).sum())
                margin = min(margin, float((kl_i - kl_bound).abs().min()))
            if actor_only:
                l = upd.cup_second_stage_step(o_[idx], a_[idx], lp_[idx], ad_[idx], om_[idx], os_full[idx],
                                              0.37 / ((1 - 0.99 * 0.95) / (1 - 0.99)), 0.99)
                out.append([np.nan, np.nan, l])
            else:
                out.append(list(upd.focops_step(o_[idx], a_[idx], lp_[idx], tr_[idx], tc_[idx], ad_[idx], om_[idx], os_full[idx], kl_bound)))
        return np.asarray(out, np.float64), R.flat_params(rp).double().numpy(), n_masked, margin
    ref_losses, th32, n_masked, margin = oracle(torch.float32)
    l64, th64, n_masked64, _ = oracle(torch.float64)
    if not actor_only:
        assert 0 < n_masked < M, n_masked             # the indicator is exercised on both sides
        assert n_masked == n_masked64 and margin > 1e-6, (n_masked, n_masked64, margin)     # ... and no sample sits ON the bound
    losses = eng.learning_iter_ex(perm.to(torch.int32).to(dev), torch.as_tensor(adv).to(dev).contiguous(),
                                  _abi.ACTOR_LOSS_KL_PENALTY, kl_bound, pg_coef, actor_only)
    eng.check_sync_error()
    got = losses.cpu().numpy()
    n_steps = (M + 63) // 64
    np.testing.assert_allclose(got[:1], ref_losses[:1], rtol=1e-5, atol=1e-6, equal_nan=True)       # first step from identical weights
    # the pass under the drift envelope (round 5: instead of rtol 2e-4 / 5e-4 with 0.1 % of the parameters exempt)
    import envelope as E
    cols = [2] if actor_only else [0, 1, 2]
    # (floor: the KL-penalty actor loss is a difference of two means of O(1) terms -- rounding is relative to the terms, not to
    #  the difference; 3e-6 of the loss is still a third of north_star's 1e-5)
    E.assert_loss_envelope(got[:, cols], ref_losses[:, cols], l64[:, cols], "KL-penalty pass: losses", window=n_steps, floor_rel=3e-6)
    E.assert_theta_envelope(pol.theta.cpu().numpy(), th32, th64, "KL-penalty pass: theta")
    if actor_only:
        off = int(_abi.load().spo_param_offset(D, A, 2))
        assert torch.equal(pol.theta[:off], theta0[:off])        # critics untouched
        assert eng.adam_step == 0 and eng.adam_step_actor_extra == 5 + n_steps


def test_kl_penalty_refuses_wide_minibatch(dev):
    from safepo import _abi
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    pol = ActorVCritic(12, 2).to(dev)
    eng = PPOLagEngine(pol, 1, 256, {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 0.02, "batch_size": 128,
                                     "learning_iters": 1, "max_grad_norm": 40.0}, dev)
    eng.snapshot_old_distribution()
    with pytest.raises(_abi.SpoError, match="batch_size 128 > 64"):
        eng.learning_iter_ex(torch.arange(256, dtype=torch.int32, device=dev), eng.buffer.adv_mix,
                             _abi.ACTOR_LOSS_KL_PENALTY, 0.02, 1.0)



class _TargetEnv:
    """Tiny device env with an action-dependent reward (test utility): reward = -mean((a - tanh(W obs))^2),
    cost = 1 if |a_0| > 0.5; truncation every 16 steps.  A working collect->GAE->update loop must raise the return."""
    is_device_env = True

    def __init__(self, n, D, A, dev, seed=0):
        g = torch.Generator(device="cpu").manual_seed(seed)
        self.W = (torch.randn(D, A, generator=g) / D ** 0.5).to(dev)
        self.n, self.D, self.A, self.dev, self.t = n, D, A, dev, 0
        self.obs = torch.randn(n, D, device=dev)
        self.obs_rms = None

    def reset(self):
        return self.obs, {}

    def step(self, act):
        tgt = torch.tanh(self.obs @ self.W)
        reward = -((act - tgt) ** 2).mean(-1)
        cost = (act[:, 0].abs() > 0.5).float()
        self.t += 1
        trunc = torch.full((self.n,), float(self.t % 16 == 0), device=self.dev)
        nxt = torch.randn(self.n, self.D, device=self.dev)
        info = {"final_observation": nxt.clone()}
        self.obs = nxt
        return nxt, reward.contiguous(), cost, torch.zeros(self.n, device=self.dev), trunc, info


def test_end_to_end_learning_on_action_dependent_env(dev):
    from safepo.common.engine import PPOLagEngine
    from safepo.common.lagrange import Lagrange
    from safepo.common.model import ActorVCritic
    torch.manual_seed(0)
    N, T, D, A = 256, 64, 12, 3
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 0.02, "batch_size": 64, "learning_iters": 10, "max_grad_norm": 40.0}
    pol = ActorVCritic(D, A).to(dev)
    eng = PPOLagEngine(pol, N, T, cfg, dev)
    env = _TargetEnv(N, D, A, dev)
    lag = Lagrange(cost_limit=4.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035)
    obs, _ = env.reset()
    returns, costs = [], []
    for epoch in range(25):
        ep_r = 0.0
        for t in range(T):
            act = eng.collect_step(t, obs)
            nobs, rew, cost, term, trunc, info = env.step(act.clone())
            ep_r += float(rew.mean())
            eng.post_step(t, nobs, rew, cost, term, trunc, info["final_observation"])
            obs = nobs
        eng.drain_episode_events(None)
        returns.append(ep_r / T)
        costs.append(float(np.mean(eng.cost_deque)))
        lag.update_lagrange_multiplier(costs[-1])
        out = eng.update(lag.lagrangian_multiplier)
        assert np.isfinite(out["kl"]) and torch.isfinite(pol.theta).all()
    first, last = np.mean(returns[:3]), np.mean(returns[-3:])
    assert last > first + 0.25 * abs(first), (first, last)          # mean squared error to the target drops clearly
    assert costs[-1] < costs[0]                                    # and the cost (|a_0| > 0.5 rate) comes down


@pytest.mark.parametrize("form", ["row_split_form", "main_plus_helper_waves", "four_wave_form"])
def test_long_trajectory_parity_1024_steps(dev, form):
    """1 024 consecutive optimiser steps (one pass over 65 536 samples) against the CPU oracle with the drift envelope:
    per-minibatch losses along the whole trajectory and the parameters after 8 / 64 / 512 / 1 024 steps stay within
    3x the fp32 reference arithmetic's own distance from the float64 trajectory (k = 1, 8, 8192 steps;
    the 8 192-step case is test_full_size_update_parity_drift_envelope).  Both forms of the persistent kernel: the
    four-wave form still serves the critic fit of the second-order scripts, the KL-penalty losses, obs_dim > 64 and the
    data-parallel launches (SPO_UPDATE_FORM is read once per process, so that form runs in a child process)."""
    if form != "row_split_form":
        # (the row-split kernel of round 6 is the default form; the other two still serve the data-parallel launches, the KL-penalty
        # losses, obs_dim > 64 and SPO_UPDATE_FORM=2 / 0: each in a child process, the switch is read once per process)
        import subprocess, sys
        env = dict(os.environ, SPO_UPDATE_FORM="0" if form == "four_wave_form" else "2")
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", __file__, "-k",
                            "test_long_trajectory_parity_1024_steps and row_split_form"], env=env,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    M, D, A = 65536, 60, 8
    torch.manual_seed(3)
    pol = ActorVCritic(D, A).to(dev)
    problem = _synthetic_update_problem(M, D, A, seed=77)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 40.0}
    eng = PPOLagEngine(pol, 1, M, cfg, dev)
    _fill_update_problem(eng, problem)
    sd0 = {k: v.detach().cpu().clone() for k, v in pol.state_dict().items()}
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(5))
    ks = (8, 64, 512, 1024)
    runs = _hip_prefix_runs(eng, pol, pol.theta.clone(), perm.to(torch.int32).to(dev), 64, ks)
    rep = _assert_trajectory_in_envelope(runs, problem, sd0, perm, 64, ks, "1024-step trajectory")
    print("drift envelope (ratio <= 1 passes):", rep)


@pytest.mark.parametrize("tag", ["a", "c"])
def test_buffer_reference_api_store_finish_path_get(dev, golden_dir, tag):
    """The reference's own call sequence -- store() per step, finish_path() per ended path, get() --
    on the dense device buffer, against the outputs of the reference VectorizedOnPolicyBuffer."""
    from safepo.common.buffer import VectorizedOnPolicyBuffer
    from safepo.common.engine import _Space
    z = np.load(os.path.join(golden_dir, "gae.npz"))
    i = lambda k: z[f"{tag}_in_{k}"]
    N, T = i("reward").shape
    buf = VectorizedOnPolicyBuffer(obs_space=_Space(6), act_space=_Space(2), size=T, num_envs=N, gamma=0.99, device=dev)
    for t in range(T):
        buf.store(obs=torch.from_numpy(i("obs")[:, t]).to(dev), act=torch.from_numpy(i("act")[:, t]).to(dev),
                  reward=torch.from_numpy(i("reward")[:, t]), cost=torch.from_numpy(i("cost")[:, t]),
                  value_r=torch.from_numpy(i("value_r")[:, t]), value_c=torch.from_numpy(i("value_c")[:, t]),
                  log_prob=torch.from_numpy(i("log_prob")[:, t]))
        for n in range(N):
            if i("seg_end")[n, t]:
                buf.finish_path(last_value_r=torch.tensor([i("boot_r")[n, t]]), last_value_c=torch.tensor([i("boot_c")[n, t]]), idx=n)
    with pytest.raises(AssertionError, match="Buffer overflow"):
        buf.store(reward=torch.zeros(N))
    data = buf.get()
    assert set(data) >= {"obs", "act", "reward", "cost", "done", "value_r", "value_c", "adv_r", "adv_c",
                         "target_value_r", "target_value_c", "log_prob"}
    for k in ("obs", "act", "reward", "cost", "value_r", "value_c", "log_prob"):
        assert np.array_equal(data[k].cpu().numpy(), z[f"{tag}_get_{k}"]), k
    for k in ("target_value_r", "target_value_c"):
        assert _ulp_diff(data[k].cpu().numpy(), z[f"{tag}_get_{k}"]).max() <= 1, k
    np.testing.assert_allclose(data["adv_r"].cpu().numpy(), z[f"{tag}_get_adv_r"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(data["adv_c"].cpu().numpy(), z[f"{tag}_get_adv_c"], rtol=1e-5, atol=2e-6)
    assert buf.ptr == 0 and buf.ptr_list == [0] * N


def test_use_eval_branch(dev, tmp_path):
    import argparse
    import csv
    from safepo.single_agent import ppo_lag
    args = argparse.Namespace(seed=0, use_eval=True, task="SynthSafe-v0", num_envs=4, experiment="t",
                              log_dir=str(tmp_path / "exp" / "task" / "run"), device="cuda", device_id=0,
                              write_terminal=True, headless=False, total_steps=2 * 4 * 32, steps_per_epoch=4 * 32,
                              randomize=False, cost_limit=25.0, lagrangian_multiplier_init=0.001,
                              lagrangian_multiplier_lr=0.035, cfg_override={"learning_iters": 1},
                              env_kwargs={"trunc_len": 8})
    ppo_lag.main(args, {})
    rows = list(csv.DictReader(open(tmp_path / "exp" / "task" / "run" / "progress.csv")))
    assert len(rows) == 2 and float(rows[0]["Metrics/EvalEpLen"]) == 8.0 and "Time/Eval" in rows[0]


@pytest.mark.parametrize("algo,line_search", [("natural_pg", False), ("trpo", True), ("rcpo", False), ("trpo_lag", True)])
def test_trust_region_family_vs_reference_main_trace(dev, golden_dir, algo, line_search):
    """f4: natural_pg / trpo / rcpo / trpo_lag on the CPO kernels against traces of the reference mains.  The two
    Lagrangian siblings (rcpo.py:325-326, trpo_lag.py:326-327) take the multiplier from the host Lagrange object fed with
    the recorded EpCost statistics and run the update on the mixed advantage."""
    from safepo.common.lagrange import Lagrange
    z = np.load(os.path.join(golden_dir, f"{algo}_trace.npz"))
    lagrangian = algo in ("rcpo", "trpo_lag")
    lagrange = Lagrange(cost_limit=float(z["meta_arg_cost_limit"]),
                        lagrangian_multiplier_init=float(z["meta_arg_lagrangian_multiplier_init"]),
                        lagrangian_multiplier_lr=float(z["meta_arg_lagrangian_multiplier_lr"])) if lagrangian else None
    N, T, epochs = int(z["meta_num_envs"]), int(z["meta_T"]), int(z["meta_epochs"])
    pol, eng = _cpo_engine(z, "init_sd_", dev, N, T, {"learning_iters": int(z["meta_cfg_learning_iters"]),
                                                       "batch_size": int(z["e0_batch_size"]),
                                                       "target_kl": float(z["meta_cfg_target_kl"])})
    for e in range(epochs):
        _load_epoch_into_engine(z, e, eng, dev)
        if lagrangian:
            lagrange.update_lagrange_multiplier(float(z[f"e{e}_get_stats_Metrics_EpCost"]))
            lam = lagrange.lagrangian_multiplier
            assert lam == pytest.approx(float(z[f"e{e}_row_Train_LagragianMultiplier"]), rel=1e-6)
            eng.buffer.compute_gae(lam)
            adv = eng.buffer.adv_mix.reshape(-1)
        else:
            eng.buffer.compute_gae(None)
            adv = eng.buffer.data["adv_r"].reshape(-1)
        out = eng.trust_region_update(adv, line_search)
        assert out["xHx"] == pytest.approx(float(z[f"e{e}_Misc_xHx"]), rel=5e-3)
        assert out["H_inv_g"] == pytest.approx(float(z[f"e{e}_Misc_H_inv_g"]), rel=5e-3)
        assert out["gradient_norm"] == pytest.approx(float(z[f"e{e}_Misc_gradient_norm"]), rel=1e-4)
        assert out["final_step_norm"] == pytest.approx(float(z[f"e{e}_Misc_FinalStepNorm"]), rel=5e-3)
        assert out["alpha"] == pytest.approx(float(z[f"e{e}_Misc_Alpha"]), rel=5e-3)
        assert out["kl"] == pytest.approx(float(z[f"e{e}_Train_KL"]), rel=2e-2)
        assert out["loss_actor"] == pytest.approx(float(z[f"e{e}_Loss_Loss_actor"]), rel=2e-3, abs=1e-6)
        if line_search:
            assert out["acceptance_step"] == int(z[f"e{e}_Misc_AcceptanceStep"])
        act_ref = np.concatenate([z[f"e{e}_actor_after_{k}"].reshape(-1) for k in pol.actor.state_dict()])
        np.testing.assert_allclose(eng.theta_actor.cpu().numpy(), act_ref, rtol=5e-3, atol=2e-5)
        iters = int(z["meta_cfg_learning_iters"])
        perms = [torch.from_numpy(z[f"e{e}_perm{i}"].astype(np.int32)).to(dev) for i in range(iters)]
        fit = eng.critic_fit(perm_fn=lambda it: perms[it])
        eng.buffer.reset()
        np.testing.assert_allclose(torch.cat(fit["losses"], 0).cpu().numpy(), z[f"e{e}_mb_losses"][:, :2], rtol=2e-3, atol=1e-5)
    ref_final = np.concatenate([z[f"final_sd_{k}"].reshape(-1) for k in pol.state_dict()])
    _assert_params_close(pol.theta.cpu().numpy(), ref_final, 1e-3, 12, rtol=5e-3, atol=5e-5, what="final theta")


@pytest.mark.parametrize("algo", ["natural_pg", "trpo", "rcpo", "trpo_lag"])
def test_trust_region_entrypoints_synthetic(dev, tmp_path, algo):
    import argparse
    import csv
    import importlib
    mod = importlib.import_module(f"safepo.single_agent.{algo}")
    args = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=8, experiment="t",
                              log_dir=str(tmp_path / "exp" / "task" / "run"), device="cuda", device_id=0,
                              write_terminal=True, headless=False, total_steps=2 * 8 * 32, steps_per_epoch=8 * 32,
                              randomize=False, cost_limit=0.5, lagrangian_multiplier_init=0.001,
                              lagrangian_multiplier_lr=0.035, cfg_override={"learning_iters": 2},
                              env_kwargs={"trunc_len": 8, "p_cost": 0.5})
    mod.main(args, {})
    rows = list(csv.DictReader(open(tmp_path / "exp" / "task" / "run" / "progress.csv")))
    assert len(rows) == 2 and float(rows[0]["Misc/xHx"]) >= 0
    assert ("Train/LagragianMultiplier" in rows[0]) == (algo in ("rcpo", "trpo_lag"))
    assert ("Misc/AcceptanceStep" in rows[0]) == (algo in ("trpo", "trpo_lag"))


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_multi_agent_masked_gae_popart_bit_exact(dev, golden_dir, tag):
    """f3 (first piece): SeparatedReplayBuffer.compute_returns / compute_cost_returns with PopArt denormalisation --
    fp32, reference operation order => bit-identical to the reference buffer."""
    from safepo.common.buffer import SeparatedReplayBuffer
    from safepo.common.engine import _Space
    from safepo.common.popart import PopArt
    z = np.load(os.path.join(golden_dir, "ma_gae.npz"))
    g = lambda k: torch.from_numpy(z[f"{tag}_{k}"].copy())
    T, N = z[f"{tag}_rewards"].shape[:2]
    cfg = dict(episode_length=T, n_rollout_threads=N, hidden_size=8, recurrent_N=1, gamma=0.96, gae_lambda=0.95,
               use_gae=True, use_popart=True, use_valuenorm=True, use_proper_time_limits=False,
               algorithm_name="mappolag", device="cuda:0")
    buf = SeparatedReplayBuffer(cfg, _Space(6), _Space(9), _Space(3))
    buf.rewards.copy_(g("rewards")); buf.costs.copy_(g("costs")); buf.masks.copy_(g("masks"))
    buf.value_preds.copy_(g("value_preds")); buf.cost_preds.copy_(g("cost_preds"))
    norm = PopArt(1)
    norm.running_mean.copy_(g("rm")); norm.running_mean_sq.copy_(g("rms")); norm.debiasing_term.copy_(g("deb").reshape(()))
    mean, var = norm.running_mean_var()
    assert np.array_equal(mean.numpy(), z[f"{tag}_mean"]) and np.array_equal(var.numpy(), z[f"{tag}_var"])
    buf.cost_returns[:-1].fill_(7.0)                        # (row T is never written by either recurrence)
    buf.compute_returns(g("next_v").to(dev), norm)
    assert bool((buf.cost_returns[:-1] == 7.0).all())       # the reward side leaves cost_returns alone (buffer.py:356-377)
    assert np.array_equal(buf.returns.cpu().numpy().view(np.uint32), z[f"{tag}_returns"].view(np.uint32))
    # ... and the cost side leaves `returns` alone even when it is given a DIFFERENT normaliser (buffer.py:379-384)
    other = PopArt(1)
    other.running_mean.fill_(3.0); other.running_mean_sq.fill_(11.0); other.debiasing_term.fill_(0.5)
    buf.compute_cost_returns(g("next_c").to(dev), other)
    assert np.array_equal(buf.returns.cpu().numpy().view(np.uint32), z[f"{tag}_returns"].view(np.uint32))
    buf.compute_cost_returns(g("next_c").to(dev), norm)
    assert np.array_equal(buf.returns.cpu().numpy().view(np.uint32), z[f"{tag}_returns"].view(np.uint32))
    assert np.array_equal(buf.cost_returns.cpu().numpy().view(np.uint32), z[f"{tag}_cost_returns"].view(np.uint32))


@pytest.mark.parametrize("algo", ["pair", "twophase", "a2a", "helper16", "rowsplit", "rowsplit_4_ranks", "rowsplit_8_ranks"])
def test_in_kernel_gradient_exchange_two_ranks_one_gpu(dev, tmp_path, algo):
    """SURVEY.md 8(e) in-kernel form: two ranks (two processes, this one GPU, regions mapped through IPC handles) run
    the data-parallel persistent kernel.  Replicas must stay bit-identical and match the kernel / all-reduce / kernel
    form of the same steps.  "rowsplit" (round 6): the row-split kernel, its one-hand-off all-to-all of tagged words behind the
    row groups' L2 hand-off (SPO_XR_FORM_ROW_SPLIT; 2 x 6 co-resident workgroups here); at 4 and 8 ranks the same form runs as
    reduce-scatter + all-gather (every word reduced by its owner rank in rank order, then broadcast: 24 / 48 workgroups)."""
    import json
    import socket
    import subprocess
    import sys
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    out = tmp_path / "p2p.json"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    nproc = 8 if algo.endswith("_8_ranks") else 4 if algo.endswith("_4_ranks") else 2     # (rank-order sums over more than one peer)
    algo = algo.replace("_4_ranks", "").replace("_8_ranks", "")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", SPO_P2P_ALGO="pair" if algo in ("a2a", "helper16") else algo)
    if algo == "a2a":
        env["SPO_P2P_A2A"] = "1"        # main + helper kernel with the flag-based all-to-all exchange on the helper waves
    if algo == "helper16":
        env["SPO_P2P_HELPER"] = "2"     # main + helper kernel, packed-word recursive doubling on the helper waves (round 5)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "tests", "p2p_worker.py"), str(out), "1000", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    assert res["p2p_created"], res
    assert res["selftest"] == [0, 0], res
    assert res["replicas_identical"] and res["finite"], res
    assert res["frac_outside_1e-5"] <= 1e-3 and res["max_abs_diff_vs_allreduce_form"] < 2e-3, res
    assert res["loss_max_abs_diff"] < 1e-4, res
    assert res["timeout_raises_on_every_rank"] and res["fallback_replicas_identical"], res
    print("p2p", res)


@pytest.mark.parametrize("form", ["in_kernel", "rccl_form"])
def test_data_parallel_global_batch_equals_reference_minibatches(dev, tmp_path, form):
    """SURVEY.md 8(e) "Partitioning", exact-semantics option (VERDICT r1 missing item 6): cfg dp_batch = "global" gives every
    rank batch_size / world rows of its shard per step; the rank-mean gradient is then the gradient of the reference's
    64-row minibatch, so two ranks x 32 rows must reproduce the oracle's single-process steps on the union of the rows
    (ppo_lag.py:297-336; order of the sums aside).  Both exchange forms."""
    import json
    import socket
    import subprocess
    import sys
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    out = tmp_path / "dp_exact.json"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "tests", "dp_exact_worker.py"), str(out),
           "1" if form == "in_kernel" else "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    assert res["in_kernel_exchange"] == (form == "in_kernel") and res["local_batch"] == 32 and res["steps"] == 16, res
    assert res["replicas_identical"], res
    assert res["loss_max_rel_diff"] < 1e-4, res
    assert res["theta_frac_outside"] <= 1e-3 and res["theta_max_abs_diff"] < 1e-5 and res["theta_moved"] > 1e-3, res
    print("dp_exact", res)


@pytest.mark.parametrize("shape", ["100,20,64,64", "60,8,128,128", "376,17,64,64", "130,8,64,64", "100,20,64,64,launch_per_layer"])
def test_data_parallel_wide_engine_global_batch_equals_reference_minibatches(dev, tmp_path, shape):
    """The same exact-semantics check for a policy OUTSIDE the persistent kernels' envelope (act_dim 20; hidden [128, 128]): the
    wide-network engine all-reduces the flat gradient of the three networks per minibatch step before the joint clip
    (ppo_lag.py:325), so two ranks x 32 rows reproduce the oracle's 64-row steps on the union of the rows.  Hidden [64, 64] with
    obs_dim <= 512 / act_dim <= 32 (HumanoidVelocity's 376 / 17): the gradient of a step comes from ONE launch of the
    feature-split kernel (spo_ppo_lag_grad_ks, round 6); `launch_per_layer` (SPO_WIDE_KS=0) keeps the 20-launch form covered."""
    import json
    import socket
    import subprocess
    import sys
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    out = tmp_path / "dp_exact_wide.json"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    per_layer = shape.endswith(",launch_per_layer")
    if per_layer:
        shape, env["SPO_WIDE_KS"] = shape[:-len(",launch_per_layer")], "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "tests", "dp_exact_worker.py"), str(out), "0", shape]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    assert res["engine"] == "WidePPOLagEngine" and not res["in_kernel_exchange"] and res["local_batch"] == 32 and res["steps"] == 16, res
    assert res["grad_kernel"] == (shape.endswith(",64,64") and not per_layer), res
    assert res["replicas_identical"], res
    assert res["loss_max_rel_diff"] < 1e-4, res
    assert res["theta_frac_outside"] <= 1e-3 and res["theta_max_abs_diff"] < 1e-5 and res["theta_moved"] > 1e-3, res


@pytest.mark.parametrize("B,K,N", [(8192, 48, 128), (8192, 128, 128), (8192, 128, 6), (100, 7, 1), (65, 130, 70), (1, 1, 1)])
def test_ma_plain_products_run_on_the_mfma_kernel_vs_torch(dev, B, K, N):
    """f3: every plain product of the multi-agent networks -- collect-size blocks, heads, input gradients,
    tangent passes -- runs on the hand-written fp32 MFMA kernel; torch.matmul in fp32 is this test's second product, held to
    the same bound against the float64 product (an implementation that is not ours calibrates the bound)."""
    from safepo import _abi
    lib = _abi.load()
    g = torch.Generator(device=dev).manual_seed(B + K + N)
    x = torch.randn(B, K, device=dev, generator=g)
    w = torch.randn(N, K, device=dev, generator=g)
    dy = torch.randn(B, N, device=dev, generator=g)
    ref_fwd = (x.double() @ w.double().T)
    ref_bwd = (dy.double() @ w.double())
    for mode, a, ref, shape in ((0, x, ref_fwd, (B, N)), (1, dy, ref_bwd, (B, K))):
        y = torch.full(shape, float("nan"), device=dev)
        _abi.check(lib.spo_debug_ma_gemm(0, mode, _abi.ptr(a), _abi.ptr(w), _abi.ptr(y), B, K, N, _abi.stream_ptr()), "gemm")
        outs = [y, torch.matmul(a, w.T if mode == 0 else w)]
        scale = float(ref.abs().max()) + 1e-6
        for y in outs:                                   # both within fp32 rounding of the float64 product
            assert float((y.double() - ref).abs().max()) <= 2e-6 * scale * max(1.0, (K if mode == 0 else N) ** 0.5)
        assert torch.isfinite(outs[0]).all()


# ====================================================================== f3: multi-agent MAPPO-L
def _ma_cfg(dev, **over):
    from safepo.multi_agent.mappolag import default_cfg
    cfg = dict(default_cfg)
    cfg.update(device=str(dev), **over)
    return cfg


class _Sp:
    def __init__(self, n):
        self.shape = (n,)


@pytest.mark.parametrize("D,H,nb,O,actor,B", [(20, 64, 3, 5, True, 97), (33, 64, 3, 1, False, 97), (48, 128, 3, 6, True, 1030), (60, 128, 2, 1, False, 1031), (48, 128, 3, 6, True, 33001), (128, 128, 2, 1, False, 32900),
                                               (100, 512, 2, 1, False, 259), (7, 33, 1, 2, True, 5), (64, 128, 2, 16, True, 4100),
                                               (48, 128, 1, 9, True, 2049)])
def test_ma_network_forward_backward_vs_oracle(dev, D, H, nb, O, actor, B):
    """LayerNorm -> [Linear, ELU, LayerNorm] x nb -> head: outputs and the full flat gradient (in-tree MFMA GEMMs + fused
    LayerNorm/ELU kernels) against torch autograd on the CPU restatement, under the fp64 yardstick (tests/ma_yardstick.py):
    at most 3x as far from the float64 evaluation as the restatement's own float32 arithmetic, + 1e-6 of the scale."""
    import ma_yardstick as Y
    from oracle import ma_restatement as MR
    from safepo.common.model import MultiAgentActor, MultiAgentCritic
    torch.manual_seed(D + H)
    cfg = _ma_cfg(dev, hidden_size=H, layer_N=nb - 1)
    net = MultiAgentActor(cfg, _Sp(D), _Sp(O), dev) if actor else MultiAgentCritic(cfg, _Sp(D), dev)
    with torch.no_grad():
        net.theta.add_(0.1 * torch.randn_like(net.theta))            # LayerNorm weights/biases and heads off their defaults
    ref = MR.MANet(D, H, nb, O, actor)
    ref.load_reference_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    assert torch.equal(ref.flat(), net.theta.cpu())
    ref64 = Y.to_dtype(ref, torch.float64)
    x = torch.randn(B, D) * 1.5 + 0.3
    out, saved = net.net_forward(x.to(dev), keep=True)
    ref_out, out64 = ref(x), ref64(x.double())
    Y.gate(out.cpu().numpy(), ref_out.detach().numpy(), out64.detach().numpy(), 1e-6, "forward")
    dout = torch.randn(B, O)
    ref_out.backward(dout)
    out64.backward(dout.double())
    grad = torch.full_like(net.theta, float("nan"))
    net.net_backward(saved, dout.to(dev), grad)

    def flat_grads(r):                         # log_std has no gradient through the mean head: NaN marks its slot
        return torch.cat([(p.grad if p.grad is not None else torch.full_like(p, float("nan"))).reshape(-1)
                          for p in r.ordered_parameters()]).double().numpy()
    got, want, want64 = grad.double().cpu().numpy(), flat_grads(ref), flat_grads(ref64)
    if actor:                                  # ... and spo_ma_backward leaves it alone (spo_ma_actor_loss owns it)
        o = net.offset(6)
        assert np.isnan(got[o:o + O]).all() and np.isnan(want[o:o + O]).all()
    m = ~np.isnan(want)
    d_hip, d_32 = Y.gate(got[m], want[m], want64[m], 1e-6, "flat gradient")
    print(f"ma net {D}x{H}x{nb}->{O} B={B}: grad max|hip-f64| {d_hip:.2e} vs |f32-f64| {d_32:.2e} (scale {np.abs(want64[m]).max():.2e})")


MA_ROW_NAMES = ("value_loss", "critic_grad_norm", "policy_loss", "entropy", "actor_grad_norm", "ratio", "cost_loss", "cost_grad_norm",
                "lamda", "popart_mean", "popart_mean_sq", "popart_debias")


def _gate_nets_vs_golden(Y, nets_hip, z, prefix, nets64, what):
    """Parameters after optimiser steps: HIP against the float64 oracle, with the REFERENCE's recorded fp32 result as the
    float32 leg of the yardstick (floor 1e-5 of the largest parameter: north_star's bar)."""
    for nm, net in nets_hip:
        pre = f"{prefix}_{nm}_"
        gold = np.concatenate([z[k].reshape(-1) for k in z.files if k.startswith(pre)])
        d_hip, d_32 = Y.gate(net.theta.cpu().numpy(), gold, nets64[nm].flat().numpy(), 1e-5, f"{what} {nm} parameters")
        print(f"{what} {nm}: max|hip-f64| {d_hip:.2e} vs |reference-f64| {d_32:.2e}")


@pytest.mark.parametrize("tag", ["default", "mamujoco"])
def test_ma_trainer_ppo_update_vs_reference_golden(dev, golden_dir, tag):
    """Three MAPPO_L_Trainer.ppo_update steps against the reference's own trainer (tests/golden/ma_mappolag.npz): value /
    cost / policy losses, the three gradient norms, entropy, ratio, the in-loop multiplier, PopArt statistics, and the
    parameters of all three networks afterwards.  Gate (round 4): the fp64 yardstick with the reference's recorded fp32
    numbers as the float32 leg -- |HIP - f64| <= 3 |reference - f64| + 1e-5 of the scale (1e-6 for the forward pass)."""
    import ma_yardstick as Y
    from oracle import ma_restatement as MR
    from safepo.multi_agent.mappolag import MAPPO_L_Policy, MAPPO_L_Trainer
    z = np.load(os.path.join(golden_dir, "ma_mappolag.npz"))
    gc = MR.cfg_from_golden(z, tag)
    cfg = _ma_cfg(dev, **{k: gc[k] for k in gc})
    cfg["hidden_size"], cfg["layer_N"] = int(gc["hidden_size"]), int(gc["layer_N"])
    s = MR.sample_from_golden(z, tag)
    D, S, A = s["obs"].shape[1], s["share_obs"].shape[1], s["actions"].shape[1]
    pol = MAPPO_L_Policy(cfg, _Sp(D), _Sp(S), _Sp(A))
    for nm, net in (("actor", pol.actor), ("critic", pol.critic), ("cost_critic", pol.cost_critic)):
        pre = f"{tag}_init_{nm}_"
        net.load_state_dict({k[len(pre):]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith(pre)})
    # ---- float64 yardstick: the restatement (pinned to this fixture at 2e-5 on the CPU) in double
    nets0 = MR.nets_from_golden(z, tag)
    n64 = {k: Y.to_dtype(v, torch.float64) for k, v in nets0.items()}
    with torch.no_grad():
        mean64 = n64["actor"](s["obs"].double())
        logp64 = MR.log_probs(mean64, n64["actor"].std(), s["actions"].double())
        val64 = n64["critic"](s["share_obs"].double())
    # forward parity on the reference's own numbers
    Y.gate(pol.actor.net_forward(s["obs"].to(dev)).cpu().numpy(), z[f"{tag}_fwd_mean"], mean64.numpy(), 1e-6, "actor mean")
    lp, _ = pol.actor.evaluate_actions(s["obs"].to(dev), None, s["actions"].to(dev), None)
    Y.gate(lp.cpu().numpy(), z[f"{tag}_fwd_logp"], logp64.numpy(), 1e-6, "log-probabilities")
    Y.gate(pol.get_values(s["share_obs"].to(dev), None, None).cpu().numpy(), z[f"{tag}_fwd_values"], val64.numpy(), 1e-6, "values")
    tr = MAPPO_L_Trainer(cfg, pol)
    sample = (s["share_obs"], s["obs"], None, None, s["actions"], s["value_preds"], s["returns"], None, s["active_masks"],
              s["old_logp"], s["adv"], None, s["factor"], s["cost_preds"], s["cost_returns"], None, s["cost_adv"],
              s["aver_episode_costs"])
    sample = tuple(t.to(dev) if torch.is_tensor(t) else t for t in sample)
    rows = []
    for _ in range(3):
        vl, cgn, plo, ent, agn, imp, cl, cogn = tr.ppo_update(sample)
        vn = tr.value_normalizer
        rows.append([vl.item(), cgn.item(), plo.item(), ent.item(), agn.item(), imp.detach().mean().item(), cl.item(), cogn.item(),
                     float(tr.lamda_lagr), float(vn.running_mean), float(vn.running_mean_sq), float(vn.debiasing_term)])
    recs64, nets64, _ = Y.oracle_steps(gc, nets0, s, "mappolag", 3, torch.float64)
    Y.gate_rows(rows, z[f"{tag}_steps"], [r["row"] for r in recs64], 1e-5, f"{tag} logged scalars", MA_ROW_NAMES)
    # the FIRST step starts from identical parameters and statistics: north_star's 1e-5 directly against the reference
    np.testing.assert_allclose(rows[0], z[f"{tag}_steps"][0], rtol=1e-5, atol=1e-7)
    _gate_nets_vs_golden(Y, (("actor", pol.actor), ("critic", pol.critic), ("cost_critic", pol.cost_critic)), z, f"{tag}_final", nets64, tag)


def _ma_sibling(algo):
    import importlib
    M = importlib.import_module(f"safepo.multi_agent.{algo}")
    return M, getattr(M, f"{algo.upper()}_Policy"), getattr(M, f"{algo.upper()}_Trainer")


@pytest.mark.parametrize("tag", ["happo_default", "happo_masked", "mappo_default", "mappo_mamujoco"])
def test_ma_happo_mappo_trainer_vs_reference_golden(dev, golden_dir, tag):
    """HAPPO / MAPPO on the MAPPO-L kernels (joint ratio x factor vs per-dimension ratios; value loss over active rows):
    three reference Trainer.ppo_update steps on a fixed sample, then one reference Trainer.train over a filled buffer
    (tests/golden/ma_happo_mappo.npz) -- logged scalars, PopArt statistics and both networks afterwards, under the fp64
    yardstick with the reference's recorded numbers as the float32 leg (floor 1e-5 of the scale)."""
    import ma_yardstick as Y
    from oracle import ma_restatement as MR
    from safepo.common.buffer import SeparatedReplayBuffer
    algo = tag.split("_")[0]
    M, Pol, Tr = _ma_sibling(algo)
    z = np.load(os.path.join(golden_dir, "ma_happo_mappo.npz"))
    gc = MR.cfg_from_golden(z, tag)
    cfg = dict(M.default_cfg)
    cfg.update(device=str(dev), **gc)
    for k in ("hidden_size", "layer_N", "learning_iters", "num_mini_batch"):
        cfg[k] = int(gc[k])
    s = MR.sample_from_golden(z, tag)
    D, S, A = s["obs"].shape[1], s["share_obs"].shape[1], s["actions"].shape[1]
    names = ("value_loss", "critic_grad_norm", "policy_loss", "entropy", "actor_grad_norm", "ratio", "popart_mean", "popart_mean_sq",
             "popart_debias")

    def load(pol, which):
        for nm, net in (("actor", pol.actor), ("critic", pol.critic)):
            pre = f"{tag}_{which}_{nm}_"
            net.load_state_dict({k[len(pre):]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith(pre)})
    pol = Pol(cfg, _Sp(D), _Sp(S), _Sp(A))
    assert pol.cost_critic is None
    load(pol, "init")
    tr = Tr(cfg, pol)
    sample = (s["share_obs"], s["obs"], None, None, s["actions"], s["value_preds"], s["returns"], None, s["active_masks"],
              s["old_logp"], s["adv"], None, s["factor"])
    sample = tuple(t.to(dev) if torch.is_tensor(t) else t for t in sample)
    rows = []
    for _ in range(3):
        vl, cgn, plo, ent, agn, imp = tr.ppo_update(sample)
        vn = tr.value_normalizer
        rows.append([vl.item(), cgn.item(), plo.item(), ent.item(), agn.item(), imp.item(), float(vn.running_mean),
                     float(vn.running_mean_sq), float(vn.debiasing_term)])
    recs64, nets64, _ = Y.oracle_steps(gc, MR.nets_from_golden(z, tag), s, algo, 3, torch.float64)
    Y.gate_rows(rows, z[f"{tag}_steps"], [r["row"] for r in recs64], 1e-5, f"{tag} logged scalars", names)
    np.testing.assert_allclose(rows[0], z[f"{tag}_steps"][0], rtol=1e-5, atol=1e-7)          # first step: 1e-5 against the reference
    _gate_nets_vs_golden(Y, (("actor", pol.actor), ("critic", pol.critic)), z, f"{tag}_final", nets64, tag)
    # ---- Trainer.train over the reference's filled buffer
    T, N = z[f"{tag}_buf_factor"].shape[0:2]
    cfg.update(episode_length=int(T), n_rollout_threads=int(N))
    pol = Pol(cfg, _Sp(D), _Sp(S), _Sp(A))
    load(pol, "tinit")
    tr = Tr(cfg, pol)
    buf = SeparatedReplayBuffer(cfg, _Sp(D), _Sp(S), _Sp(A))
    buf_keys = ("share_obs", "obs", "actions", "action_log_probs", "value_preds", "returns", "active_masks", "factor")
    for k in buf_keys:
        getattr(buf, k).copy_(torch.from_numpy(z[f"{tag}_buf_{k}"].copy()))

    class _Log:
        def __init__(self):
            self.rows = []

        def store(self, **kw):
            self.rows.append([kw["Loss/Loss_reward_critic"], kw["Misc/Reward_critic_norm"], kw["Loss/Loss_actor"],
                              kw["Misc/Entropy"], kw["Misc/Ratio"]])
    lg = _Log()
    tr.train(buf, lg)
    # float64 yardstick of the same call (the reference shuffles its single whole-buffer minibatch: that only reorders sums)
    tr64, n64 = Y.oracle_trainer(gc, MR.nets_from_golden(z, tag, "tinit"), algo, torch.float64)
    b64 = {k: torch.from_numpy(z[f"{tag}_buf_{k}"].copy()).double() for k in buf_keys}
    b64["rewards"] = torch.zeros_like(b64["factor"])
    iters = int(gc["learning_iters"])
    got64 = np.asarray(MR.train_agent(tr64, b64, [torch.arange(b64["factor"].numel())] * iters, gc))
    Y.gate_rows(lg.rows, z[f"{tag}_train_rows"], got64[:, [0, 1, 2, 3, 5]], 1e-5, f"{tag} Trainer.train rows",
                ("value_loss", "critic_grad_norm", "policy_loss", "entropy", "ratio"))
    vn = tr.value_normalizer
    Y.gate([float(vn.running_mean), float(vn.running_mean_sq), float(vn.debiasing_term)], z[f"{tag}_train_popart"], got64[-1, 6:9], 1e-5,
           f"{tag} PopArt statistics after train()")
    _gate_nets_vs_golden(Y, (("actor", pol.actor), ("critic", pol.critic)), z, f"{tag}_tfinal", n64, f"{tag} train()")


@pytest.mark.parametrize("algo", ["happo", "mappo"])
def test_ma_happo_mappo_runner_end_to_end_synthetic(dev, tmp_path, algo):
    """safepo.multi_agent.{happo,mappo}.train() on the synthetic env: the shorter collect / insert / compute path (no
    cost critic), the reference's log columns and checkpoints; the team reward improves."""
    import argparse
    import csv
    M, _, _ = _ma_sibling(algo)
    cfg = dict(M.default_cfg)
    cfg.update(M.mamujoco_cfg)
    cfg.update(device=str(dev), n_rollout_threads=64, n_eval_rollout_threads=4, episode_length=16, num_env_steps=64 * 16 * 12,
               hidden_size=64, log_dir=str(tmp_path / "run"), seed=0, actor_lr=3e-3, critic_lr=3e-3,
               env_name="SynthMultiAgent-v0", env_kwargs={"trunc_len": 16, "num_agents": 3, "obs_dim": 12, "act_dim": 2})
    args = argparse.Namespace(task="SynthMultiAgent-v0", seed=0, model_dir="")
    torch.manual_seed(0)
    runner = M.train(args, cfg)
    rows = list(csv.DictReader(open(tmp_path / "run" / "progress.csv")))
    assert len(rows) == 12
    for col in ("Metrics/EpRet", "Metrics/EpCost", "Loss/Loss_reward_critic", "Loss/Loss_actor", "Misc/Reward_critic_norm",
                "Misc/Entropy", "Misc/Ratio", "Time/FPS"):
        assert col in rows[0], col
    assert "Loss/Loss_cost_critic" not in rows[0]
    rets = [float(r["Metrics/EpRet"]) for r in rows]
    assert np.isfinite(rets).all() and np.mean(rets[-3:]) > np.mean(rets[:3]), rets
    assert runner.policy[0].cost_critic is None
    assert os.path.exists(tmp_path / "run" / "models_seed0" / "critic_agent2.pt")


@pytest.mark.parametrize("D,H,nb,O,B", [(20, 32, 3, 5, 97), (48, 128, 2, 6, 1030), (33, 64, 1, 3, 260)])
def test_ma_network_tangent_pass_vs_autograd(dev, D, H, nb, O, B):
    """spo_ma_jvp (forward-mode pass: in-tree MFMA GEMMs + LayerNorm/ELU tangent kernel) against torch.func.jvp on the CPU
    restatement, and the Fisher-vector product built from it against the reference's double-backward form -- both under the
    fp64 yardstick (float32 autograd / double backward as the float32 leg, floor 1e-6 of the scale)."""
    import ma_yardstick as Y
    from torch.func import functional_call, jvp
    from oracle import ma_restatement as MR
    from safepo.common.model import MultiAgentActor
    torch.manual_seed(D + H + nb)
    cfg = _ma_cfg(dev, hidden_size=H, layer_N=nb - 1)
    net = MultiAgentActor(cfg, _Sp(D), _Sp(O), dev)
    with torch.no_grad():
        net.theta.add_(0.1 * torch.randn_like(net.theta))
    ref = MR.MANet(D, H, nb, O, True)
    ref.load_reference_state_dict({k: v.cpu() for k, v in net.state_dict().items()})
    x = torch.randn(B, D) * 1.5 + 0.3
    t = torch.randn(net.theta.numel())
    names = [n for n, _ in ref.named_parameters()]
    by_id = {id(p): n for n, p in ref.named_parameters()}
    order = [by_id[id(p)] for p in ref.ordered_parameters()]
    prm = {n: p.detach() for n, p in ref.named_parameters()}
    tan, off = {}, 0
    for n in order:
        k = prm[n].numel()
        tan[n] = t[off:off + k].view_as(prm[n])
        off += k
    assert off == t.numel() and set(names) == set(order)
    tan = {n: tan[n] for n in prm}                      # same pytree structure (key order) as the primals
    _, want = jvp(lambda pp: functional_call(ref, pp, (x,)), (prm,), (tan,))
    ref64 = Y.to_dtype(ref, torch.float64)
    prm64 = {n: p.detach() for n, p in ref64.named_parameters()}
    _, want64 = jvp(lambda pp: functional_call(ref64, pp, (x.double(),)), (prm64,), ({n: v.double() for n, v in tan.items()},))
    out, saved = net.net_forward(x.to(dev), keep=True)
    got = net.net_jvp(saved, t.to(dev))
    Y.gate(got.cpu().numpy(), want.numpy(), want64.numpy(), 1e-6, "tangent pass")              # fp64 yardstick (ma_yardstick.py)
    # Fisher-vector product of MACPO: J^T M J p + log_std block + 0.1 p  ==  double backward of the reference's KL expression
    from safepo.multi_agent.macpo import MACPO_Policy, MACPO_Trainer, default_cfg
    c2 = dict(default_cfg)
    c2.update(device=str(dev), hidden_size=H, layer_N=nb - 1)
    pol = MACPO_Policy(c2, _Sp(D), _Sp(D), _Sp(O))
    pol.actor.theta.copy_(net.theta)
    tr = MACPO_Trainer(c2, pol)
    _, saved = pol.actor.net_forward(x.to(dev), keep=True)
    std = tr._std()
    m_diag = (2.0 / (1e-8 + 2.0 * std * std)).reshape(1, -1)
    got_f = tr.fisher_vector_product(saved, t.to(dev), m_diag, tr._kl_hessian_logstd()).cpu()
    orc = MR.OracleMATrainer({"actor_lr": 1e-3, "critic_lr": 1e-3, "opti_eps": 1e-5, "weight_decay": 0.0}, ref, MR.MANet(D, H, nb, 1, False),
                             MR.MANet(D, H, nb, 1, False), algo="macpo")
    want_f = orc._fvp({"obs": x, "actions": torch.zeros(B, O)}, t)
    orc64, _ = Y.oracle_trainer(orc.cfg, {"actor": ref, "critic": orc.critic, "cost_critic": orc.cost_critic}, "macpo", torch.float64)
    want_f64 = orc64._fvp({"obs": x.double(), "actions": torch.zeros(B, O, dtype=torch.float64)}, t.double())
    Y.gate(got_f.numpy(), want_f.numpy(), want_f64.numpy(), 1e-6, "Fisher-vector product vs double backward")


@pytest.mark.parametrize("tag", ["safe", "unsafe", "mamujoco", "recover", "deep_safe"])
def test_ma_macpo_trainer_vs_reference_golden(dev, golden_dir, tag):
    """Two MACPO_Trainer.trpo_update steps against the reference's own trainer (tests/golden/ma_macpo.npz), five settings
    covering optim cases 0-3: critic losses / norms, KL, improvement, expected improvement, the cost surrogate,
    (lam, nu), both conjugate-gradient solutions, the step, and the actor after the line search.  Ten CG iterations amplify
    fp32 reduction-order noise, which is why round 3 compared at 5e-3 / 1e-2; now the deviation is SHOWN to be that: the
    restatement takes the same two steps in float64 and every quantity is gated |HIP - f64| <= 3 |reference - f64| + floor."""
    import ma_yardstick as Y
    from oracle import ma_restatement as MR
    from safepo.multi_agent.macpo import MACPO_Policy, MACPO_Trainer, default_cfg
    z = np.load(os.path.join(golden_dir, "ma_macpo.npz"))
    gc = MR.cfg_from_golden(z, tag)
    cfg = dict(default_cfg)
    cfg.update(device=str(dev), **gc)
    for k in ("hidden_size", "layer_N", "searching_steps", "conjugate_gradient_iters"):
        cfg[k] = int(gc[k])
    s = MR.sample_from_golden(z, tag)
    D, S, A = s["obs"].shape[1], s["share_obs"].shape[1], s["actions"].shape[1]
    pol = MACPO_Policy(cfg, _Sp(D), _Sp(S), _Sp(A))
    for nm, net in (("actor", pol.actor), ("critic", pol.critic), ("cost_critic", pol.cost_critic)):
        pre = f"{tag}_init_{nm}_"
        net.load_state_dict({k[len(pre):]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith(pre)})
    tr = MACPO_Trainer(cfg, pol)
    sample = (s["share_obs"], s["obs"], None, None, s["actions"], s["value_preds"], s["returns"], None, s["active_masks"],
              s["old_logp"], s["adv"], None, s["factor"], s["cost_preds"], s["cost_returns"], None, s["cost_adv"],
              s["aver_episode_costs"])
    sample = tuple(t.to(dev) if torch.is_tensor(t) else t for t in sample)
    tr64, n64 = Y.oracle_trainer(gc, MR.nets_from_golden(z, tag), "macpo", torch.float64)
    s64 = Y.to_dtype(s, torch.float64)
    names = ("value_loss", "critic_grad_norm", "kl", "improve", "expected_improve", "cost_surrogate", "cost_grad_norm", "wrp", "lam", "nu",
             "b.b", "popart_mean", "popart_mean_sq", "popart_debias")
    rows, gold_rows, rows64 = [], [], []
    for it in range(2):
        r = tr.trpo_update(sample)
        (vl, cgn, kl, improve, expected, _ent, _ratio, cost_loss, cost_gn, wrp, _cp, _cr, bgrad, lam, nu, g_dir, b_dir, x, _mu,
         _std, bb) = r
        rec64 = tr64.ppo_update(s64)
        vn = tr.value_normalizer
        rows.append([float(vl), float(cgn), float(kl), float(improve), float(expected), float(cost_loss), float(cost_gn), float(wrp),
                     float(lam), float(nu), float(bb), float(vn.running_mean), float(vn.running_mean_sq), float(vn.debiasing_term)])
        gold_rows.append(z[f"{tag}_steps"][it]); rows64.append(rec64["row"])
        for got, key, k64 in ((bgrad, "cost_grad", "b"), (g_dir, "g_step_dir", "g_dir"), (b_dir, "b_step_dir", "b_dir"), (x, "x", "x")):
            d_hip, d_32 = Y.gate(got.cpu().numpy(), z[f"{tag}_s{it}_{key}"], rec64[k64].numpy(), 1e-5, f"step {it} {key}")
            print(f"macpo {tag} step {it} {key}: max|hip-f64| {d_hip:.2e} vs |reference-f64| {d_32:.2e}")
        Y.gate(pol.actor.theta.cpu().numpy(), z[f"{tag}_s{it}_actor_after"], n64["actor"].flat().numpy(), 1e-5, f"step {it} actor after")
    # improve / expected_improve / kl are differences of nearly equal numbers: their scale is the surrogate's, not their own
    scale_of = {2: None, 3: None, 4: None}
    for c, nm in enumerate(names):
        col = lambda rr: np.asarray(rr, np.float64)[:, c]
        sc = max(np.abs(col(rows64)).max(), np.abs(np.asarray(rows64, np.float64)[:, 5]).max()) if c in scale_of else None
        Y.gate(col(rows), col(gold_rows), col(rows64), 1e-5, f"{tag} column {nm}", scale=sc)
    _gate_nets_vs_golden(Y, (("critic", pol.critic), ("cost_critic", pol.cost_critic)), z, f"{tag}_final", n64, tag)


def test_ma_macpo_runner_end_to_end_synthetic(dev, tmp_path):
    """safepo.multi_agent.macpo.train() on the synthetic env: trust-region actor steps per agent in HAPPO order, the
    reference's MACPO log columns; KL stays inside the trust region and the run is finite."""
    import argparse
    import csv
    from safepo.multi_agent import macpo
    cfg = dict(macpo.default_cfg)
    cfg.update(macpo.mamujoco_cfg)
    cfg.update(device=str(dev), n_rollout_threads=64, n_eval_rollout_threads=4, episode_length=16, num_env_steps=64 * 16 * 8,
               hidden_size=64, log_dir=str(tmp_path / "run"), seed=0, critic_lr=3e-3, env_name="SynthMultiAgent-v0",
               env_kwargs={"trunc_len": 16, "num_agents": 3, "obs_dim": 12, "act_dim": 2}, cost_limit=1.0)
    args = argparse.Namespace(task="SynthMultiAgent-v0", seed=0, model_dir="")
    torch.manual_seed(0)
    runner = macpo.train(args, cfg)
    rows = list(csv.DictReader(open(tmp_path / "run" / "progress.csv")))
    assert len(rows) == 8
    for col in ("Metrics/EpRet", "Metrics/EpCost", "Loss/Loss_reward_critic", "Loss/Loss_cost_critic", "Loss/Loss_actor_improve",
                "Loss/Loss_actor_expected_improve", "Misc/Reward_critic_norm", "Misc/Cost_critic_norm", "Misc/Entropy", "Misc/Ratio",
                "Misc/KL", "Time/FPS"):
        assert col in rows[0], col
    assert "Loss/Loss_actor" not in rows[0]
    kls = [float(r["Misc/KL"]) for r in rows]
    assert np.isfinite(kls).all() and max(kls) < cfg["target_kl"] + 1e-6, kls
    assert all(np.isfinite(float(r["Metrics/EpRet"])) for r in rows)
    assert torch.isfinite(runner.policy[0].actor.theta).all()


def test_benchmark_launcher_then_evaluate_round_trip(dev, tmp_path, monkeypatch):
    """The callers either side of the path (reference safepo/single_agent/benchmark.py, multi_agent/benchmark.py,
    evaluate.py): launch one single-agent and one multi-agent run as subprocesses through the sweep launchers, then
    evaluate the saved checkpoints through benchmark_eval / single_runs_eval."""
    import glob
    from safepo import evaluate
    from safepo.multi_agent import benchmark as mb
    from safepo.single_agent import benchmark as sb
    work = tmp_path / "w"
    work.mkdir()
    monkeypatch.chdir(work)                      # the scripts log under ../runs relative to where they are started
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    monkeypatch.setenv("PYTHONPATH", os.pathsep.join([os.path.join(root, "safe-policy-optimization_amd"), os.environ.get("PYTHONPATH", "")]))
    sb.main(["--tasks", "SynthSafe-v0", "--algo", "ppo_lag", "--num-seeds", "1", "--workers", "1", "--experiment", "bench",
             "--total-steps", "2048", "--num-envs", "16", "--steps-per-epoch", "1024"])
    runs = glob.glob(str(tmp_path / "runs" / "bench" / "SynthSafe-v0" / "ppo_lag" / "seed-000-*"))
    assert len(runs) == 1 and os.path.exists(os.path.join(runs[0], "torch_save")) and os.path.exists(os.path.join(runs[0], "progress.csv"))
    res = evaluate.benchmark_eval(["--benchmark-dir", str(tmp_path / "runs" / "bench"), "--eval-episodes", "2",
                                   "--save-dir", str(tmp_path / "results")])
    (rm, rs, cm, cs) = res[("SynthSafe-v0", "ppo_lag")]
    assert np.isfinite([rm, rs, cm, cs]).all() and cm >= 0
    assert "ppo_lag in SynthSafe-v0 evaluation reward" in open(tmp_path / "results" / "eval_result.txt").read()
    mb.main(["--tasks", "SynthMultiAgent-v0", "--algo", "mappolag", "--num-seeds", "1", "--workers", "1", "--experiment", "mabench",
             "--total-steps", "8000", "--num-envs", "8"])
    mruns = glob.glob(str(tmp_path / "runs" / "mabench" / "SynthMultiAgent-v0" / "mappolag" / "seed-000-*"))
    assert len(mruns) == 1
    r, c = evaluate.single_runs_eval(mruns[0], 2)
    assert np.isfinite([r, c]).all()


@pytest.mark.parametrize("D,nb,O,actor,B", [(48, 3, 6, True, 33001), (96, 2, 1, False, 40000)])
def test_ma_block_kernel_forms_agree(dev, tmp_path, D, nb, O, actor, B):
    """Round-3 forms of the training-size kernels (wave-private row tiles in the block forward / backward, head backward fused
    with the top LayerNorm backward) against the round-1/2 forms (SPO_MA_FWD_WAVE=0, SPO_MA_FUSE_HEAD=0), each in its own process
    (the knobs are read once): the forward -- outputs AND every stored activation / statistic -- must be identical bit for bit;
    the gradients differ only by the order of their row-partial sums."""
    import subprocess
    import sys
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ma_forms_worker.py")
    res = {}
    for name, env_over in (("new", {}), ("old", {"SPO_MA_FWD_WAVE": "0", "SPO_MA_FUSE_HEAD": "0"})):
        env = dict(os.environ)
        env.pop("SPO_MA_FWD_WAVE", None); env.pop("SPO_MA_FUSE_HEAD", None)
        env.update(env_over)
        out = str(tmp_path / f"{name}.npz")
        r = subprocess.run([sys.executable, worker, out, str(D), str(nb), str(O), str(int(actor)), str(B)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[name] = np.load(out)
    assert np.array_equal(res["new"]["out"], res["old"]["out"])
    assert np.array_equal(res["new"]["ws"], res["old"]["ws"])
    g_new, g_old = res["new"]["grad"], res["old"]["grad"]
    scale = np.abs(g_old).max()
    assert scale > 0 and np.abs(g_new - g_old).max() <= 2e-6 * scale + 1e-9, (np.abs(g_new - g_old).max(), scale)


@pytest.mark.parametrize("rows", [8192, 2111, 70])
def test_ma_collect_forward_is_bit_identical_to_the_per_network_path(dev, rows):
    """f3 collect step: spo_ma_collect_forward takes ALL networks of a step through one launch (feature
    LayerNorm, blocks, head, Gaussian sample on chip).  From 2 048 rows upwards the per-network path runs the same fused-block
    arithmetic, so every output must be identical bit for bit; below that the per-network path uses the plain GEMM +
    LayerNorm kernels and the comparison is at 1e-5.  Also: the unsupported-geometry return value."""
    from safepo import _abi
    from safepo.common.model import MultiAgentActor, MultiAgentCritic
    lib = _abi.load()
    torch.manual_seed(rows)
    specs = [(48, 3, 6, True, False), (96, 3, 1, False, False), (20, 1, 2, True, True), (128, 2, 1, False, False),
             (64, 4, 16, True, False), (96, 3, 1, False, False)]
    nets, xs = [], []
    for D, nb, O, actor, det in specs:
        cfg = _ma_cfg(dev, hidden_size=128, layer_N=nb - 1)
        net = MultiAgentActor(cfg, _Sp(D), _Sp(O), dev) if actor else MultiAgentCritic(cfg, _Sp(D), dev)
        with torch.no_grad():
            net.theta.add_(0.1 * torch.randn_like(net.theta))
        nets.append(net)
        xs.append(torch.randn((rows, D), device=dev) * 2 + 0.3)
    arr = (_abi.MaCollectNet * len(nets))()
    outs = []
    for i, ((D, nb, O, actor, det), net, x) in enumerate(zip(specs, nets, xs)):
        c = arr[i]
        c.theta, c.net, c.x, c.deterministic = _abi.ptr(net.theta), net._net, _abi.ptr(x), int(det)
        out = torch.full((rows, O), float("nan"), device=dev)
        c.out = _abi.ptr(out)
        rec = {"out": out}
        if actor:
            rec["eps"] = torch.randn((rows, O), device=dev)
            rec["act"], rec["logp"] = torch.full_like(out, float("nan")), torch.full_like(out, float("nan"))
            c.eps, c.act, c.logp = (None if det else _abi.ptr(rec["eps"])), _abi.ptr(rec["act"]), _abi.ptr(rec["logp"])
            c.std_x_coef, c.std_y_coef = net.std_x_coef, net.std_y_coef
        outs.append(rec)
    scratch = torch.empty(int(lib.spo_ma_collect_scratch_floats(len(nets))), device=dev)
    _abi.check(lib.spo_ma_collect_forward(len(nets), arr, rows, _abi.ptr(scratch), _abi.stream_ptr()), "collect_forward")
    torch.cuda.synchronize()
    exact = rows >= 2048
    for (D, nb, O, actor, det), net, x, rec in zip(specs, nets, xs, outs):
        mean = net.net_forward(x)
        if exact:
            assert torch.equal(rec["out"], mean), (D, nb, O)
        else:
            np.testing.assert_allclose(rec["out"].cpu().numpy(), mean.cpu().numpy(), rtol=1e-5, atol=1e-5)
        if actor:
            act, logp = torch.empty_like(mean), torch.empty_like(mean)
            # sampling from the fused kernel's own mean: the Gaussian arithmetic must agree bit for bit at every size
            _abi.check(lib.spo_ma_sample(_abi.ptr(rec["out"]), _abi.ptr(net.log_std), None if det else _abi.ptr(rec["eps"]),
                                         net.std_x_coef, net.std_y_coef, int(det), _abi.ptr(act), _abi.ptr(logp), rows, O,
                                         _abi.stream_ptr()), "ma_sample")
            assert torch.equal(rec["act"], act) and torch.equal(rec["logp"], logp), (D, nb, O)
            if det:
                assert torch.equal(rec["act"], rec["out"])
    # geometry outside the fused kernel: a positive return value and nothing launched
    cfg = _ma_cfg(dev, hidden_size=64, layer_N=1)
    small = MultiAgentCritic(cfg, _Sp(12), dev)
    one = (_abi.MaCollectNet * 1)()
    xo, oo = torch.randn((rows, 12), device=dev), torch.zeros((rows, 1), device=dev)
    one[0].theta, one[0].net, one[0].x, one[0].out = _abi.ptr(small.theta), small._net, _abi.ptr(xo), _abi.ptr(oo)
    assert lib.spo_ma_collect_forward(1, one, rows, _abi.ptr(scratch), _abi.stream_ptr()) == _abi.MA_COLLECT_UNSUPPORTED
    assert float(oo.abs().sum()) == 0.0


def test_ma_runner_collect_fused_launch_equals_per_network_collect(dev, tmp_path):
    """Runner.collect (mappolag.py:411-447) with the one-launch collect against the per-network launches: same seed, same
    torch.randn draws -> values, actions, log-probabilities and cost predictions equal bit for bit (4 096 threads: both sides
    on the fused-block arithmetic); then two episodes through the captured graph end to end."""
    from safepo.multi_agent import mappolag
    from safepo.common.env import SynthMultiAgentEnv
    cfg = _ma_cfg(dev, **mappolag.mamujoco_cfg)
    cfg.update(n_rollout_threads=4096, episode_length=4, hidden_size=128, log_dir=str(tmp_path / "run"), seed=0,
               env_name="SynthMultiAgent-v0", use_eval=False, collect_graph=False)
    env = SynthMultiAgentEnv(4096, num_agents=3, obs_dim=48, act_dim=6, trunc_len=4, device=dev)
    r = mappolag.Runner(env, None, cfg)
    r.logger.verbose = False
    r.warmup()
    got = {}
    for fused in (True, False):
        r.config["collect_fused"] = fused
        r._fused_unsupported = False
        torch.manual_seed(123)
        got[fused] = r.collect(0)
    assert not r._fused_unsupported
    v1, a1, l1, _, _, c1, _ = got[True]
    v0, a0, l0, _, _, c0, _ = got[False]
    assert v1.shape == v0.shape and torch.equal(v1, v0) and torch.equal(c1, c0)
    for x, y in zip(a1 + l1, a0 + l0):
        assert torch.equal(x, y)
    assert float(a1[0].std()) > 0.1
    # end to end through the captured graph
    r.config.update(collect_fused=True, collect_graph=True)
    for ep in range(2):
        for step in range(4):
            values, actions, lps, rnn, rnn_c, cps, rnn_k = r.collect(step)
            obs, share_obs, rewards, costs, dones, infos, _ = env.step(actions)
            r.insert((obs, share_obs, rewards, costs, dones, infos, values, actions, lps, rnn, rnn_c, cps, rnn_k, costs.mean()))
        r.compute()
        r.train()
    assert r._inplace_ok and sorted(r._step_graphs) == [0, 1, 2, 3] and not getattr(r, "_graph_failed", False)
    assert all(torch.isfinite(t.policy.actor.theta).all() for t in r.trainer)
    # the per-step graphs write into the buffer rows: a replay under a seed equals the eager one-launch collect under that seed
    torch.manual_seed(7)
    r.config["collect_graph"] = False
    ve, ae, le, _, _, ce, _ = [x.clone() if torch.is_tensor(x) else [y.clone() for y in x] for x in r.collect(2)]
    r.config["collect_graph"] = True
    vg, ag, lg, _, _, cg, _ = r.collect(2)
    assert vg.data_ptr() == r._stack["value_preds"][:, 2].data_ptr() and ag[1].data_ptr() == r.buffer[1].actions[2].data_ptr()
    assert torch.equal(vg, ve) and torch.equal(cg, ce)                   # values do not depend on the random draws
    assert all(torch.isfinite(x).all() for x in ag + lg) and ag[0].shape == ae[0].shape
    first = ag[0].clone()
    r.collect(2)                                                         # a second replay of the same graph draws new noise
    assert not torch.equal(r.buffer[0].actions[2], first)
    # a parameter vector that moved (module.to(), a re-flattened network) invalidates the captured pointers: recaptured
    act0 = r.trainer[0].policy.actor
    act0.float()                                                         # nn.Module._apply -> _flatten(): new theta storage
    with torch.no_grad():
        act0.theta.mul_(0.0)                                             # mean 0 for every row from now on
    r.collect(2)
    assert sorted(r._step_graphs) == [2]
    assert float((r.buffer[0].actions[2] - r.buffer[0].actions[2].mean()).abs().max()) > 0 and \
        abs(float(r.buffer[0].actions[2].mean())) < 0.1
    # insert() with rows that are already in place must leave them alone and still fill the rest
    b = r.buffer[0]
    s0 = b.step
    vals, acts, lps, rnn, rnn_c, cps, rnn_k = r.collect(s0)
    keep_act = acts[0].clone()
    obs, share_obs, rewards, costs, dones, infos, _ = env.step(acts)
    r.insert((obs, share_obs, rewards, costs, dones, infos, vals, acts, lps, rnn, rnn_c, cps, rnn_k, costs.mean()))
    assert torch.equal(b.actions[s0], keep_act) and torch.equal(b.rewards[s0], rewards[:, 0])
    assert torch.equal(b.obs[s0 + 1], obs[:, 0]) and float(b.active_masks[s0 + 1].min()) == 1.0
    # the one-launch insert (spo_ma_insert_step) against the torch copies, with done patterns of every kind: no agent, one
    # agent, all agents of a thread done
    dones = torch.zeros((4096, 3), dtype=torch.bool, device=dev)
    dones[5, 1] = True; dones[9] = True; dones[4095, 2] = True; dones[4095, 0] = True
    snaps = {}
    for fused in (True, False):
        r.config["insert_fused"] = fused
        for bb in r.buffer:
            bb.step = 1
        for f in ("obs", "share_obs", "rewards", "costs", "masks", "active_masks"):
            r._stack[f].fill_(-7.0)
        r.insert((obs, share_obs, rewards, costs, dones, infos, vals, acts, lps, rnn, rnn_c, cps, rnn_k, costs.mean()))
        snaps[fused] = {f: r._stack[f].clone() for f in ("obs", "share_obs", "rewards", "costs", "masks", "active_masks")}
    for f, t in snaps[True].items():
        assert torch.equal(t, snaps[False][f]), f
    m, am = snaps[True]["masks"], snaps[True]["active_masks"]
    assert float(m[:, 2, 9].sum()) == 0.0 and float(m[:, 2, 5].sum()) == 3.0 and float(am[1, 2, 5]) == 0.0 and float(am[:, 2, 9].sum()) == 3.0
    assert float(am[0, 2, 4095]) == 0.0 and float(am[1, 2, 4095]) == 1.0 and float(m[0, 2, 4095]) == 1.0


@pytest.mark.parametrize("algo", ["happo", "mappo"])
def test_ma_unconstrained_runners_through_the_one_launch_collect(dev, tmp_path, algo):
    """happo / mappo Runners (no cost critic: 2 networks per agent, 5-tuple collect) at hidden 128 through the one-launch
    collect, the per-step graphs writing into the buffer rows and the one-launch insert (no cost field): same seed ->
    values / actions / log-probabilities equal to the per-network launches bit for bit; then two episodes end to end."""
    import importlib
    from safepo.common.env import SynthMultiAgentEnv
    M = importlib.import_module(f"safepo.multi_agent.{algo}")
    cfg = dict(M.default_cfg)
    cfg.update(M.mamujoco_cfg)
    cfg.update(device=str(dev), n_rollout_threads=2048, episode_length=4, hidden_size=128, log_dir=str(tmp_path / "run"), seed=0,
               env_name="SynthMultiAgent-v0", use_eval=False, collect_graph=False)
    env = SynthMultiAgentEnv(2048, num_agents=2, obs_dim=20, act_dim=3, trunc_len=4, device=dev)
    r = M.Runner(env, None, cfg)
    r.logger.verbose = False
    r.warmup()
    got = {}
    for fused in (True, False):
        r.config["collect_fused"] = fused
        r._fused_unsupported = False
        torch.manual_seed(5)
        got[fused] = r.collect(0)
    assert not r._fused_unsupported and len(got[True]) == 5
    assert torch.equal(got[True][0], got[False][0])
    for x, y in zip(got[True][1] + got[True][2], got[False][1] + got[False][2]):
        assert torch.equal(x, y)
    r.config.update(collect_fused=True, collect_graph=True)
    for ep in range(2):
        for step in range(4):
            values, actions, lps, rnn, rnn_c = r.collect(step)
            obs, share_obs, rewards, costs, dones, infos, _ = env.step(actions)
            r.insert((obs, share_obs, rewards, costs, dones, infos, values, actions, lps, rnn, rnn_c, None, None, None))
            assert torch.equal(r.buffer[1].obs[step + 1], obs[:, 1]) and torch.equal(r.buffer[0].rewards[step], rewards[:, 0])
        r.compute()
        r.train()
    assert r._inplace_ok and sorted(r._step_graphs) == [0, 1, 2, 3]
    assert all(torch.isfinite(t.policy.actor.theta).all() and torch.isfinite(t.policy.critic.theta).all() for t in r.trainer)


def test_ma_side_stream_critics_equal_the_sequential_update(dev, tmp_path):
    """MAPPO_L_Trainer.ppo_update runs the two critics on side streams while the actor runs on the caller's (cfg
    train_streams, default on; the four PopArt statistics updates keep their order).  One agent's train() over a collected
    episode with and without the side streams, from the same state: every parameter, Adam moment, the multiplier and the
    PopArt state must be identical bit for bit."""
    from safepo.multi_agent import mappolag
    from safepo.common.env import SynthMultiAgentEnv
    cfg = _ma_cfg(dev, **mappolag.mamujoco_cfg)
    cfg.update(n_rollout_threads=4096, episode_length=8, hidden_size=128, log_dir=str(tmp_path / "run"), seed=0,
               env_name="SynthMultiAgent-v0", use_eval=False)
    env = SynthMultiAgentEnv(4096, num_agents=2, obs_dim=48, act_dim=6, trunc_len=8, device=dev)
    r = mappolag.Runner(env, None, cfg)
    r.logger.verbose = False
    r.warmup()
    for step in range(8):
        values, actions, lps, rnn, rnn_c, cps, rnn_k = r.collect(step)
        obs, share_obs, rewards, costs, dones, infos, _ = env.step(actions)
        r.insert((obs, share_obs, rewards, costs, dones, infos, values, actions, lps, rnn, rnn_c, cps, rnn_k, costs.mean()))
    r.compute()
    tr, b = r.trainer[0], r.buffer[0]
    b.update_factor(torch.ones(8, 4096, 1, device=dev))
    pol = tr.policy
    opts = (pol.actor_optimizer, pol.critic_optimizer, pol.cost_optimizer)

    def snapshot():
        return ([n.theta.clone() for n in pol.networks()], [(o.m.clone(), o.v.clone(), o.t) for o in opts],
                tr._popart_state.clone(), tr._lamda.clone())

    def restore(snap):
        for n, th in zip(pol.networks(), snap[0]):
            n.theta.copy_(th)
        for o, (m, v, t) in zip(opts, snap[1]):
            o.m.copy_(m); o.v.copy_(v); o.t = t
        tr._popart_state.copy_(snap[2]); tr._lamda.copy_(snap[3])
        tr._sync_normalizer()
    start = snapshot()
    perms = [torch.randperm(8 * 4096, device=dev) for _ in range(cfg["learning_iters"])]
    outs = {}
    for streams in (True, False):
        restore(start)
        tr.config["train_streams"] = streams
        tr.train(b, logger=None, perm_fn=lambda it: perms[it])
        torch.cuda.synchronize()
        outs[streams] = snapshot()
    assert getattr(tr, "_side", None) is not None
    for x, y in zip(outs[True][0], outs[False][0]):
        assert torch.equal(x, y)
    for (m1, v1, t1), (m2, v2, t2) in zip(outs[True][1], outs[False][1]):
        assert torch.equal(m1, m2) and torch.equal(v1, v2) and t1 == t2
    assert torch.equal(outs[True][2], outs[False][2]) and torch.equal(outs[True][3], outs[False][3])
    assert not torch.equal(outs[True][0][0], start[0][0])


def test_ma_mappolag_runner_end_to_end_synthetic(dev, tmp_path):
    """safepo.multi_agent.mappolag.train() on the synthetic 4-agent env: collect -> insert -> fused GAE/PopArt -> HAPPO
    sequential updates, logger rows and per-agent checkpoints in the reference's formats; the team reward improves."""
    import argparse
    import csv
    from safepo.multi_agent import mappolag
    cfg = _ma_cfg(dev, **mappolag.mamujoco_cfg)
    cfg.update(n_rollout_threads=64, n_eval_rollout_threads=4, episode_length=16, num_env_steps=64 * 16 * 12, hidden_size=64,
               log_dir=str(tmp_path / "run"), seed=0, actor_lr=3e-3, critic_lr=3e-3, env_name="SynthMultiAgent-v0",
               env_kwargs={"trunc_len": 16, "num_agents": 3, "obs_dim": 12, "act_dim": 2}, cost_limit=1.0)
    args = argparse.Namespace(task="SynthMultiAgent-v0", seed=0, model_dir="")
    torch.manual_seed(0)
    runner = mappolag.train(args, cfg)
    rows = list(csv.DictReader(open(tmp_path / "run" / "progress.csv")))
    assert len(rows) == 12
    for col in ("Metrics/EpRet", "Metrics/EpCost", "Loss/Loss_reward_critic", "Loss/Loss_cost_critic", "Loss/Loss_actor",
                "Misc/Reward_critic_norm", "Misc/Cost_critic_norm", "Misc/Entropy", "Misc/Ratio", "Time/FPS"):
        assert col in rows[0], col
    rets = [float(r["Metrics/EpRet"]) for r in rows]
    assert np.isfinite(rets).all() and np.mean(rets[-3:]) > np.mean(rets[:3]), rets
    for a in range(3):
        sd = torch.load(tmp_path / "run" / "models_seed0" / f"actor_agent{a}.pt")
        assert "act.action_out.log_std" in sd and sd["base.mlp.fc1.0.weight"].shape == (64, 12)
    assert float(runner.trainer[0].lamda_lagr) >= 0.0


@pytest.mark.parametrize("algo,fname", [("mappolag", "ma_runner_trace.npz"), ("happo", "ma_runner_trace_happo.npz"),
                                        ("macpo", "ma_runner_trace_macpo.npz")])
def test_ma_runner_compute_and_train_vs_reference_runner_trace(dev, golden_dir, tmp_path, algo, fname):
    """Replays episodes of the reference multi-agent Runner (mappolag / happo / macpo traces): same buffers, agent order and
    minibatch permutations -> returns (/ cost returns) after compute() (fused GAE + PopArt kernel, next values from the HIP
    networks), every stored loss / norm / entropy / ratio (/ KL, improvement), multipliers, PopArt statistics and all
    networks of every agent after each episode's HAPPO-sequential training.  Gate (round 4): the fp64 yardstick with the
    reference's recorded numbers as the float32 leg, floor 1e-5 of the scale (1e-6 for the returns)."""
    import importlib
    M = importlib.import_module(f"safepo.multi_agent.{algo}")
    z = np.load(os.path.join(golden_dir, fname))
    use_cost = algo in ("mappolag", "macpo")
    A, EP = int(z["meta_agents"]), int(z["meta_episodes"])
    T, N = int(z["cfg_episode_length"]), int(z["cfg_n_rollout_threads"])
    over = {k[4:]: float(z[k]) for k in z.files if k.startswith("cfg_")}
    cfg = dict(M.default_cfg)
    cfg.update(M.mamujoco_cfg)
    cfg.update(device=str(dev), **over)
    for k in ("hidden_size", "layer_N", "learning_iters", "num_mini_batch", "episode_length", "n_rollout_threads", "searching_steps",
              "conjugate_gradient_iters"):
        if k in cfg:
            cfg[k] = int(cfg[k])
    cfg["use_policy_active_masks"] = bool(cfg["use_policy_active_masks"])
    cfg["use_value_active_masks"] = bool(cfg.get("use_value_active_masks", False))
    cfg.update(log_dir=str(tmp_path / "run"), seed=0, env_name="trace", algorithm_name=algo)
    D, S, Adim = z["e0_a0_obs"].shape[-1], z["e0_a0_share_obs"].shape[-1], z["e0_a0_actions"].shape[-1]

    class _Spaces:
        num_agents = A
        observation_space = [_Sp(D)] * A
        share_observation_space = [_Sp(S)] * A
        action_space = [_Sp(Adim)] * A
    runner = M.Runner(_Spaces(), None, cfg)

    def nets_of(pol):
        return [("actor", pol.actor), ("critic", pol.critic)] + ([("cost_critic", pol.cost_critic)] if use_cost else [])
    for a in range(A):
        for nm, net in nets_of(runner.policy[a]):
            pre = f"init_a{a}_{nm}_"
            net.load_state_dict({k[len(pre):]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith(pre)})
    buf_keys = ["share_obs", "obs", "actions", "action_log_probs", "value_preds", "rewards", "masks", "active_masks"]
    buf_keys += ["cost_preds", "costs"] if use_cost else []
    iters = 1 if algo == "macpo" else cfg["learning_iters"]
    if algo == "mappolag":
        keys = ("Loss/Loss_reward_critic", "Loss/Loss_cost_critic", "Loss/Loss_actor", "Misc/Reward_critic_norm",
                "Misc/Cost_critic_norm", "Misc/Entropy", "Misc/Ratio")
    elif algo == "happo":
        keys = ("Loss/Loss_reward_critic", "Loss/Loss_actor", "Misc/Reward_critic_norm", "Misc/Entropy", "Misc/Ratio")
    else:
        keys = ("Loss/Loss_reward_critic", "Loss/Loss_cost_critic", "Loss/Loss_actor_improve", "Loss/Loss_actor_expected_improve",
                "Misc/Reward_critic_norm", "Misc/Cost_critic_norm", "Misc/Entropy", "Misc/Ratio", "Misc/KL")
    # float64 yardstick: the restatement replays the same episodes in double (tests/ma_yardstick.py); the REFERENCE's recorded
    # fp32 numbers are the float32 leg.  (macpo: ten CG iterations amplify reduction-order noise -- the gate widens with the
    # reference's own distance from float64 instead of a blanket 2e-2.)
    import ma_yardstick as Y
    eps64, _ = Y.runner_replay(z, algo, torch.float64)
    net_names = ("actor", "critic", "cost_critic") if use_cost else ("actor", "critic")
    for e in range(EP):
        for a in range(A):
            b = runner.buffer[a]
            for k in buf_keys:
                getattr(b, k).copy_(torch.from_numpy(z[f"e{e}_a{a}_{k}"]))
            if use_cost:
                b.aver_episode_costs = torch.from_numpy(z[f"e{e}_a{a}_aver_episode_costs"].copy()).to(dev)
        runner.compute()
        # episode 0: single evaluation of the initial networks (floor 1e-6); later episodes: after optimiser steps (1e-5)
        fl = 1e-6 if e == 0 else 1e-5
        for a in range(A):          # (row T of `returns` is never written by the recurrence)
            Y.gate(runner.buffer[a].returns.cpu().numpy()[:-1], z[f"e{e}_a{a}_returns"][:-1], eps64[e]["returns"][a][:-1], fl,
                   f"episode {e} agent {a} returns")
            if use_cost:
                Y.gate(runner.buffer[a].cost_returns.cpu().numpy()[:-1], z[f"e{e}_a{a}_cost_returns"][:-1], eps64[e]["cost_returns"][a][:-1],
                       fl, f"episode {e} agent {a} cost returns")
        order = [int(i) for i in z[f"e{e}_agent_order"]]
        perm_of = {a: [z[f"e{e}_perm{pos * iters + it}"] for it in range(iters)] for pos, a in enumerate(order)}
        runner.logger.epoch_dict.clear()
        runner.train(order=order, perm_fn=lambda a, it: perm_of[a][it])
        cols = dict((key, col) for col, key in Y.RUNNER_COLS[algo])
        surr = np.abs(eps64[e]["rows"][:, 5]).max() if algo == "macpo" else None      # scale of the macpo differences (see the trainer test)
        for key in keys:
            got = np.asarray(runner.logger.epoch_dict[key], np.float64)
            if key not in cols:        # (entropy / ratio of the macpo trace: not in the restatement's row) against the reference at 1e-4
                np.testing.assert_allclose(got, z[f"e{e}_stored_{key.replace('/', '_')}"], rtol=1e-4, atol=1e-6, err_msg=f"episode {e} {key}")
                continue
            sc = max(np.abs(eps64[e]["rows"][:, cols[key]]).max(), surr) if key in ("Loss/Loss_actor_improve", "Loss/Loss_actor_expected_improve",
                                                                                    "Misc/KL") else None
            Y.gate(got, z[f"e{e}_stored_{key.replace('/', '_')}"], eps64[e]["rows"][:, cols[key]], 1e-5, f"episode {e} {key}", scale=sc)
        for a in range(A):
            tr = runner.trainer[a]
            if algo == "mappolag":
                Y.gate([float(tr.lamda_lagr)], [float(z[f"e{e}_a{a}_lamda"])], [eps64[e]["lamda"][a]], 1e-5, f"episode {e} agent {a} multiplier")
            Y.gate(tr._popart_state.cpu().numpy(), z[f"e{e}_a{a}_popart"], eps64[e]["popart"][a], 1e-5, f"episode {e} agent {a} PopArt")
            for nm, net in nets_of(tr.policy):
                pre = f"e{e}_a{a}_after_{nm}_"
                gold = np.concatenate([z[k].reshape(-1) for k in z.files if k.startswith(pre)])
                d_hip, d_32 = Y.gate(net.theta.cpu().numpy(), gold, eps64[e]["theta"][a][nm], 1e-5, f"episode {e} agent {a} {nm}")
            print(f"{algo} episode {e}: last network max|hip-f64| {d_hip:.2e} vs |reference-f64| {d_32:.2e}")


def test_ma_mappolag_data_parallel_two_ranks_one_gpu(dev, tmp_path):
    """MAPPO-L sharded over rollout threads: two ranks (two processes on this GPU, gloo) x half the threads must equal one
    rank x all threads -- every mean (surrogate, entropy weights, value losses, PopArt batch statistics, advantage
    standardisation, lambda delta) is taken over the global batch and the flat gradients are all-reduced."""
    import json
    import socket
    import subprocess
    import sys
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    out = tmp_path / "ma_dp.json"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "ma_dp_worker.py"), str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    assert res["replicas_identical"], res
    assert res["frac_outside"] <= 1e-3 and res["max_abs_diff_vs_single_rank"] < 5e-4, res
    assert res["lamda"][0] == pytest.approx(res["lamda"][1], rel=1e-5), res
    np.testing.assert_allclose(res["popart"][0], res["popart"][1], rtol=1e-5)
    np.testing.assert_allclose(res["losses"][0], res["losses"][1], rtol=2e-4, atol=2e-6)
    assert res["moved"] > 1e-4


@pytest.mark.parametrize("shape", ["60,8,64,64", "100,4,64,64", "60,20,96,96"])
def test_cpo_data_parallel_two_ranks_one_gpu(dev, tmp_path, shape):
    """CPO sharded over envs.  Gradients g and b, every Fisher-vector product and the line-search
    sums are all-reduced means, so two ranks x half the envs reproduce one rank x all envs; the critic fit runs the
    persistent kernel with the in-kernel exchange and keeps the replicas bit-identical.  Also for shapes outside the CPO
    kernels' envelope (WideCPOEngine: obs 100 keeps the persistent critic fit and its in-kernel exchange; act 20 / hidden 96
    all-reduces the critics' flat gradient per minibatch step)."""
    import json
    import socket
    import subprocess
    import sys
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    out = tmp_path / "cpo_dp.json"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "tests", "cpo_dp_worker.py"), str(out), shape]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.load(open(out))
    assert res["engine"] == ("CPOEngine" if shape == "60,8,64,64" else "WideCPOEngine"), res
    assert res["p2p"] == (shape != "60,20,96,96") and res["replicas_identical"] and res["finite"], res
    assert len(set(res["case"])) == 1 and len(set(res["acceptance_step"])) == 1, res      # two ranks, one rank, oracle f32 / f64
    # round 5: both HIP runs under the fp64 yardstick (the oracle's step on the same rows in float32 and float64, computed by
    # the worker) instead of a 2e-3 comparison with each other
    import envelope as E
    for k in ("xHx", "gradient_norm", "H_inv_g", "alpha", "final_step_norm", "kl"):
        two, one, f32, f64 = res[k]
        E.gate_scalars([("two ranks", two, f32, f64), ("one rank", one, f32, f64)], f"cpo data-parallel {shape}: {k}", rel_floor=2e-6)
    two, one, f32, f64 = res["loss_actor"]
    E.gate_scalars([("two ranks", two, f32, f64), ("one rank", one, f32, f64)], f"cpo data-parallel {shape}: loss_actor", rel_floor=2e-6, scale=1.0)
    ad = res["actor_dist_to_f64"]
    for who in ("two_ranks", "one_rank"):
        assert ad[who][0] <= 3.0 * ad["f32"][0] + 1e-6 * ad["scale"], (who, ad)
        assert ad[who][1] <= 3.0 * ad["f32"][1] + 1e-7 * ad["scale"] * np.sqrt(ad["n"]), (who, ad)
    print("cpo data-parallel", shape, "actor |.-f64| max / L2:", ad)


def test_full_size_learning_iteration_is_deterministic(dev):
    """BASELINE config 2 size (4096 envs x 128 steps = 524 288 rows, 8192 minibatch steps in ONE persistent launch):
    size-independent properties -- two runs from the same state with the same shuffle are bit-identical (fixed-order
    reductions, tagged granule exchange, no atomics on data), every parameter stays finite and moves, the per-step losses
    are finite, and the optimiser step count advances by the number of minibatches."""
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    N, T, D, A = 4096, 128, 60, 8
    M = N * T
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 40.0}
    g = torch.Generator(device=dev).manual_seed(123)
    obs = torch.randn(N, T, D, device=dev, generator=g)
    act = torch.randn(N, T, A, device=dev, generator=g)
    logp = -A * 0.92 - 0.5 * (act ** 2).sum(-1) + 0.05 * torch.randn(N, T, device=dev, generator=g)
    tgt_r, tgt_c = torch.randn(N, T, device=dev, generator=g), torch.rand(N, T, device=dev, generator=g)
    adv = torch.randn(N, T, device=dev, generator=g)
    perm = torch.randperm(M, device=dev, generator=g).to(torch.int32)
    outs = []
    for _ in range(2):
        torch.manual_seed(9)
        pol = ActorVCritic(D, A).to(dev)
        theta0 = pol.theta.clone()
        eng = PPOLagEngine(pol, N, T, cfg, dev)
        b = eng.buffer
        b.data["obs"].copy_(obs); b.data["act"].copy_(act); b.data["log_prob"].copy_(logp)
        b.data["target_value_r"].copy_(tgt_r); b.data["target_value_c"].copy_(tgt_c); b.adv_mix.copy_(adv)
        losses = eng.learning_iter(perm)
        eng.check_sync_error()
        outs.append((pol.theta.clone(), losses.clone(), eng.adam_step, eng.adam_m.clone(), eng.adam_v.clone()))
    assert outs[0][2] == outs[1][2] == M // 64
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.equal(outs[0][3], outs[1][3]) and torch.equal(outs[0][4], outs[1][4])
    assert torch.isfinite(outs[0][0]).all() and torch.isfinite(outs[0][1]).all()
    assert outs[0][1].shape == (M // 64, 3)
    moved = (outs[0][0] - theta0).abs()
    assert float(moved.max()) > 1e-3 and float((moved > 0).float().mean()) > 0.99
    assert float(outs[0][4].min()) >= 0.0                      # second moments


def test_two_engines_update_concurrently_on_two_streams(dev):
    """the main + helper update kernel's clip backup rows and norm granules are per (device, stream) scratch, so
    two engines of one process may run their persistent launches at the same time on two streams.  Two engines with different
    data and a clip bound that is active on part of the steps (backups restored, steps repeated): three learning iterations each,
    launched concurrently, must equal the same iterations run one engine after the other, bit for bit."""
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    N, T, D, A = 256, 128, 60, 8
    M = N * T
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 0.9}

    def make(seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        torch.manual_seed(seed)
        pol = ActorVCritic(D, A).to(dev)
        eng = PPOLagEngine(pol, N, T, cfg, dev)
        b = eng.buffer
        act = torch.randn(N, T, A, device=dev, generator=g)
        b.data["obs"].copy_(torch.randn(N, T, D, device=dev, generator=g)); b.data["act"].copy_(act)
        b.data["log_prob"].copy_(-A * 0.92 - 0.5 * (act ** 2).sum(-1) + 0.05 * torch.randn(N, T, device=dev, generator=g))
        b.data["target_value_r"].copy_(torch.randn(N, T, device=dev, generator=g))
        b.data["target_value_c"].copy_(torch.rand(N, T, device=dev, generator=g))
        b.adv_mix.copy_(torch.randn(N, T, device=dev, generator=g))
        perms = [torch.randperm(M, device=dev, generator=g).to(torch.int32) for _ in range(3)]
        return eng, perms
    results = {}
    for mode in ("sequential", "concurrent"):
        engs = [make(11), make(22)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        losses = [[], []]
        if mode == "sequential":
            for k, (eng, perms) in enumerate(engs):
                for p in perms:
                    losses[k].append(eng.learning_iter(p).clone())
                torch.cuda.synchronize()
        else:
            for it in range(3):
                for k, (eng, perms) in enumerate(engs):
                    with torch.cuda.stream(streams[k]):
                        losses[k].append(eng.learning_iter(perms[it]).clone())
            torch.cuda.synchronize()
        for eng, _ in engs:
            eng.check_sync_error()
        results[mode] = [(e.policy.theta.clone(), e.adam_m.clone(), torch.stack(l)) for (e, _), l in zip(engs, losses)]
    for k in range(2):
        for x, y in zip(results["sequential"][k], results["concurrent"][k]):
            assert torch.equal(x, y), k
    assert not torch.equal(results["sequential"][0][0], results["sequential"][1][0])


def test_full_size_update_parity_drift_envelope(dev):
    """The headline launch against the oracle (ppo_lag.py:297-336): BASELINE config 2 size, 4096 envs x
    128 steps = 524 288 rows, one learning iteration = 8 192 minibatch steps in ONE persistent launch, same initial weights,
    same shuffle.  First 8 steps at 1e-5 against the fp32 oracle; then every 64-step window of the per-minibatch losses and
    the parameters after 8 / 64 / 512 / 2 048 / 8 192 steps must be no further from the oracle's float64 trajectory than
    3x the fp32 oracle (= the reference's arithmetic) is itself: drift is shown to be rounding, not assumed."""
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    N, T, D, A = 4096, 128, 60, 8
    M = N * T
    torch.manual_seed(11)
    pol = ActorVCritic(D, A).to(dev)
    problem = _synthetic_update_problem(M, D, A, seed=2024)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 40.0}
    eng = PPOLagEngine(pol, N, T, cfg, dev)
    _fill_update_problem(eng, problem)
    sd0 = {k: v.detach().cpu().clone() for k, v in pol.state_dict().items()}
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(6))
    ks = (8, 64, 512, 2048, 8192)
    runs = _hip_prefix_runs(eng, pol, pol.theta.clone(), perm.to(torch.int32).to(dev), 64, ks)
    assert eng.adam_step == 8192
    rep = _assert_trajectory_in_envelope(runs, problem, sd0, perm, 64, ks, "full-size learning iteration")
    print("drift envelope (ratio <= 1 passes):", rep)


def test_row_split_kernel_is_the_default_and_exchange_modes_agree(dev, monkeypatch):
    """Round 6: spo_ppo_lag_update_iter runs the row-split kernel (csrc/update_rs.hip) where spo_update_rs_supported.  Its exchange
    stores are plain when the placement census finds the six workgroups on one XCD and write-through otherwise (SPO_RS_SAFE=1
    forces that): correctness must not depend on placement, so both modes give the same bits -- over three consecutive launches
    on one stream (tags and slot parities carry over from launch to launch), with the clip active on part of the steps (the
    speculative layer-1 update is restored and redone, the column waves repeat L1), and the debug counters see steps and redos."""
    import ctypes
    from safepo import _abi
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    lib = _abi.load()
    assert lib.spo_update_rs_supported(60, 8, 64, 3) == 1 and lib.spo_update_rs_supported(64, 16, 1, 3) == 1
    assert lib.spo_update_rs_supported(65, 8, 64, 3) == 0 and lib.spo_update_rs_supported(60, 17, 64, 3) == 0
    assert lib.spo_update_rs_supported(60, 8, 65, 3) == 0 and lib.spo_update_rs_supported(60, 8, 128, 2) == 1
    assert lib.spo_update_rs_supported(60, 8, 129, 2) == 0 and lib.spo_update_rs_supported(60, 8, 64, 1) == 0
    if int(os.environ.get("SPO_UPDATE_FORM", "3")) < 3:
        pytest.skip("SPO_UPDATE_FORM selects an older form in this process")
    M, D, A, batch = 64 * 37 + 19, 60, 8, 64
    problem = _synthetic_update_problem(M, D, A, seed=31)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": batch, "learning_iters": 1, "max_grad_norm": 1.2}
    g = torch.Generator().manual_seed(9)
    perms = [torch.randperm(M, generator=g).to(torch.int32).to(dev) for _ in range(3)]
    outs = {}
    for mode in ("fast", "safe"):
        monkeypatch.setenv("SPO_RS_SAFE", "1" if mode == "safe" else "0")
        torch.manual_seed(4)
        pol = ActorVCritic(D, A).to(dev)
        eng = PPOLagEngine(pol, 1, M, cfg, dev)
        _fill_update_problem(eng, problem)
        c4 = (ctypes.c_ulonglong * 4)()
        _abi.check(lib.spo_debug_update_counters(c4, 1), "counters")
        losses = [eng.learning_iter(p).clone() for p in perms]
        eng.check_sync_error()
        _abi.check(lib.spo_debug_update_counters(c4, 1), "counters")
        nst = (M + batch - 1) // batch
        assert int(c4[0]) == 3 * nst, (list(c4), nst)
        assert 0 < int(c4[1]) < 3 * nst, list(c4)            # clipped on part of the steps: the late-verdict path ran
        outs[mode] = (pol.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), torch.stack(losses))
    for x, y in zip(outs["fast"], outs["safe"]):
        assert torch.equal(x, y)
    assert torch.isfinite(outs["fast"][0]).all() and torch.isfinite(outs["fast"][3]).all()


@pytest.mark.parametrize("M,D,batch", [(128 * 9 + 70, 60, 128), (100 * 7, 33, 100), (65 * 5 + 3, 64, 65), (64 * 6 + 10, 12, 64),
                                       (30 * 8, 60, 30)])
def test_row_split_critic_fit_shapes_vs_oracle(dev, M, D, batch, monkeypatch):
    """The second-order scripts' critic fit (cpo.py:541-571) on the row-split kernel: four row groups per critic above 64 rows per
    minibatch, two up to 64 -- ragged and partial minibatches, the stale actor gradient in (and rescaled by) the joint clip --
    against the restatement in float32 (first steps at 1e-5) and under the float64 yardstick after the pass."""
    import envelope as E
    from safepo.single_agent.cpo import CPOEngine, default_cfg
    from safepo.common.model import ActorVCritic
    if int(os.environ.get("SPO_UPDATE_FORM", "3")) < 3:
        pytest.skip("SPO_UPDATE_FORM selects an older form in this process")
    monkeypatch.setenv("SPO_CPO_SPLIT", "0")
    A = 4
    obs, _a, _l, tgt_r, tgt_c, _adv = _synthetic_update_problem(M, D, A, seed=M)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(2)).to(torch.int32)
    torch.manual_seed(M + 1)
    pol = ActorVCritic(D, A).to(dev)
    cfg = dict(default_cfg)
    cfg.update(learning_iters=1, batch_size=batch)
    eng = CPOEngine(pol, 1, M, cfg, dev)
    assert eng.lib.spo_update_rs_supported(D, A, batch, 2) == 1
    bd = eng.buffer.data
    bd["obs"].copy_(obs.view(1, M, D)); bd["target_value_r"].copy_(tgt_r.view(1, M)); bd["target_value_c"].copy_(tgt_c.view(1, M))
    sd0 = {k: v.detach().cpu().clone() for k, v in pol.state_dict().items()}
    eng.stale_sq.fill_(2500.0)                         # a stale actor gradient of norm 50: the joint clip (40) is active
    fit = eng.critic_fit(perm_fn=lambda it: perm.to(dev))
    assert eng._split in (None, False)
    nst = (M + batch - 1) // batch
    lh = torch.cat(fit["losses"], 0).double().cpu().numpy()
    assert lh.shape == (nst, 2)
    n_crit = pol.log_std_offset
    l32, t32 = _oracle_critic_trajectory(sd0, obs, tgt_r, tgt_c, perm, batch, nst, torch.float32, (nst,), 50.0)
    l64, t64 = _oracle_critic_trajectory(sd0, obs, tgt_r, tgt_c, perm, batch, nst, torch.float64, (nst,), 50.0)
    np.testing.assert_allclose(lh[:4], l32[:4], rtol=1e-5, atol=1e-6)
    E.assert_loss_envelope(lh, l32, l64, f"row-split critic fit {M}/{D}/{batch}", window=nst)
    E.assert_theta_envelope(pol.theta[:n_crit].double().cpu().numpy(), t32[nst], t64[nst], f"row-split critic fit {M}/{D}/{batch}")
    # the stale norm was rescaled by every step's clip coefficient (cpo.py:557): strictly smaller, still positive
    assert 0.0 < float(eng.stale_sq.item()) < 2500.0


# ---------------------------------------------------------------------------------------------------------------------
# Wide networks: ActorVCritic(obs_dim, act_dim, hidden_sizes) beyond [64, 64] (reference model.py:131; the
# isaac_gym_specific_cfg regime of ppo_lag.py:54-65) on the wide-network kernels.
def _wide_pair(D, A, hidden, dev, seed):
    from safepo.common.model import ActorVCritic
    torch.manual_seed(seed)
    pol = ActorVCritic(D, A, hidden_sizes=hidden).to(dev)
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    ref = R.OraclePolicy(D, A, hidden_sizes=tuple(hidden))
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.state_dict().items()})
    assert [k for k in pol.state_dict()] == [k for k in ref.state_dict()]
    return pol, ref


@pytest.mark.parametrize("D,A,hidden,n", [(60, 8, [128, 128], 257), (33, 3, [256, 96], 70), (60, 8, [1024, 1024, 512], 130),
                                          (17, 2, [32], 5)])
def test_wide_policy_step_vs_oracle(dev, D, A, hidden, n):
    """ActorVCritic.step / values / actor forward for hidden_sizes other than [64, 64] (model.py:149-170) against the oracle
    with the same state_dict: every Linear on the in-tree fp32 MFMA GEMM, tanh, rsample and log-prob kernels."""
    pol, ref = _wide_pair(D, A, hidden, dev, seed=5 + n)
    g = torch.Generator().manual_seed(n)
    obs, eps = torch.randn(n, D, generator=g), torch.randn(n, A, generator=g)
    act, logp, v_r, v_c = pol.step(obs.to(dev), eps=eps.to(dev))
    with torch.no_grad():
        a_ref, lp_ref, vr_ref, vc_ref = ref.step_with_eps(obs, eps)
    tol = dict(rtol=2e-5, atol=5e-6)
    np.testing.assert_allclose(act.cpu().numpy(), a_ref.numpy(), **tol)
    np.testing.assert_allclose(logp.cpu().numpy(), lp_ref.numpy(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(v_r.cpu().numpy(), vr_ref.numpy(), **tol)
    np.testing.assert_allclose(v_c.cpu().numpy(), vc_ref.numpy(), **tol)
    a_det, _, _, _ = pol.step(obs.to(dev), deterministic=True)
    with torch.no_grad():
        np.testing.assert_allclose(a_det.cpu().numpy(), ref.actor(obs).mean.numpy(), **tol)
    vr2, vc2 = pol.values(obs.to(dev))
    assert torch.equal(vr2, v_r) and torch.equal(vc2, v_c)
    a1, lp1, _, _ = pol.step(obs[0].to(dev), eps=eps[0].to(dev))             # single-row form of the reference API
    np.testing.assert_allclose(a1.cpu().numpy(), a_ref[0].numpy(), **tol)


@pytest.mark.parametrize("D,A,hidden,batch,steps,cfg_kw", [
    (60, 8, [128, 128], 64, 8, {}),
    (60, 8, [256, 96], 100, 4, {"max_grad_norm": 0.5}),
    (60, 8, [1024, 1024, 512], 8192, 2, {"use_critic_norm": False, "use_value_coefficient": True, "max_grad_norm": 1.0}),
])
def test_wide_minibatch_steps_vs_oracle(dev, D, A, hidden, batch, steps, cfg_kw):
    """The PPO-Lagrangian minibatch step (ppo_lag.py:306-329: MSE + critic L2, clipped surrogate, value coefficient, joint
    clip_grad_norm_, three Adam optimisers) for wide networks against the oracle: per-step losses at 1e-5, parameters after
    the steps; [128, 128] at the default batch of 64 and [1024, 1024, 512] at 8 192 rows with isaac_gym_specific_cfg's options."""
    from safepo.common.engine import WidePPOLagEngine
    pol, ref = _wide_pair(D, A, hidden, dev, seed=3)
    ref0 = {k: v.clone() for k, v in ref.state_dict().items()}
    M = batch * steps
    cfg = {"hidden_sizes": hidden, "gamma": 0.99, "target_kl": 0.02, "batch_size": batch, "learning_iters": 1, "max_grad_norm": 40.0}
    cfg.update(cfg_kw)
    eng = WidePPOLagEngine(pol, 1, M, cfg, dev)
    problem = _synthetic_update_problem(M, D, A, seed=17)
    _fill_update_problem(eng, problem)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(2))
    losses = eng.learning_iter(perm.to(torch.int32).to(dev)).cpu().numpy()
    kw = {k: v for k, v in cfg_kw.items() if k in ("use_critic_norm", "use_value_coefficient")}
    upd = R.PPOLagUpdater(ref, epochs=1, max_grad_norm=cfg["max_grad_norm"], **kw)
    obs, act, logp, tgt_r, tgt_c, adv = problem
    want = []
    for k in range(steps):
        ii = perm[k * batch:(k + 1) * batch]
        want.append(upd.minibatch_step(obs[ii], act[ii], logp[ii], tgt_r[ii], tgt_c[ii], adv[ii]))
    np.testing.assert_allclose(losses, np.asarray(want), rtol=1e-5, atol=2e-6)
    import envelope as E
    _, t64 = E.oracle_trajectory(ref0, problem, perm, batch, steps, torch.float64, [steps], max_grad_norm=cfg["max_grad_norm"],
                                 hidden_sizes=hidden, **kw)
    E.assert_theta_envelope(pol.theta.cpu().numpy(), R.flat_params(ref).numpy(), t64[steps], f"wide {hidden}: theta after {steps} steps")
    assert eng.adam_step == steps


def test_wide_kl_and_entrypoint_synthetic(dev, tmp_path):
    """Full-batch KL for a wide actor against the oracle, then ppo_lag.main() end to end with hidden_sizes [128, 128] on the
    synthetic env (collect, boundary logic, GAE, update, logger) and with the shape options of isaac_gym_specific_cfg."""
    import argparse
    import csv
    from safepo.common.engine import WidePPOLagEngine
    from safepo.single_agent import ppo_lag
    D, A, hidden, M = 60, 8, [128, 128], 3000
    pol, ref = _wide_pair(D, A, hidden, dev, seed=9)
    cfg = {"hidden_sizes": hidden, "gamma": 0.99, "target_kl": 0.02, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 40.0}
    eng = WidePPOLagEngine(pol, 1, M, cfg, dev)
    obs = torch.randn(M, D, generator=torch.Generator().manual_seed(4))
    eng.buffer.data["obs"].copy_(obs.view(1, M, D))
    eng.snapshot_old_distribution()
    with torch.no_grad():
        old = ref.actor(obs)
        old_mean, old_std = old.mean.clone(), old.stddev.clone()
        delta = 0.01 * torch.randn(pol.theta.numel(), generator=torch.Generator().manual_seed(8))
        pol.theta.add_(delta.to(dev))
        ref.load_state_dict({k: v.detach().cpu().clone() for k, v in pol.state_dict().items()})
    assert eng.kl_to_old() == pytest.approx(R.actor_kl(ref, obs, old_mean, old_std), rel=2e-5)
    assert set(ppo_lag.isaac_gym_specific_cfg) >= {"hidden_sizes", "num_mini_batch", "use_value_coefficient", "use_critic_norm"}
    for tag, override in (("w128", {"hidden_sizes": [128, 128], "learning_iters": 2, "batch_size": 256}),
                          ("isaac_shape", dict(ppo_lag.isaac_gym_specific_cfg, hidden_sizes=[96, 64, 32], learning_iters=2,
                                               total_steps=2 * 16 * 64, steps_per_epoch=16 * 64))):       # the exported dict itself
        cfg_run = dict(override)                   # "batch_size": None removes default_cfg's key: minibatches of M // num_mini_batch rows
        args = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=16, experiment="t",
                                  log_dir=str(tmp_path / tag / "task" / "run"), device="cuda", device_id=0, write_terminal=True,
                                  headless=False, total_steps=2 * 16 * 64, steps_per_epoch=16 * 64, randomize=False, cost_limit=25.0,
                                  lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035, cfg_override=cfg_run,
                                  env_kwargs={"trunc_len": 16})
        out = ppo_lag.main(args, {})
        rows = list(csv.DictReader(open(tmp_path / tag / "task" / "run" / "progress.csv")))
        assert len(rows) == 2 and np.isfinite(float(rows[-1]["Loss/Loss_actor"])) and np.isfinite(float(rows[-1]["Train/KL"]))
        assert type(out["engine"]).__name__ == "WidePPOLagEngine"
        if tag == "isaac_shape":
            assert out["engine"]._cfg_struct().batch == 16 * 64 // 4 and out["engine"]._cfg_struct().use_value_coefficient == 1


@pytest.mark.parametrize("dp_batch", ["local", "global"])
def test_bench_self_launches_two_ranks_on_one_gpu(dev, dp_batch):
    """`python bench.py --gpus 2` WITHOUT a launcher (how the driver invokes it) spawns its own two ranks (here both on
    cuda:0: SPO_BENCH_ONE_GPU=1), runs the data-parallel epoch with the in-kernel gradient exchange and prints ONE line with
    n_gpus = 2, per-rank timings and the exchange form; `--dp-batch global` runs the exact-semantics partitioning (global
    minibatch of 64 = 2 x 32 rows)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["SPO_BENCH_ONE_GPU"] = "1"
    # the local-batch run also carries BASELINE config 5 on the N > 1 path: the MAPPO-L Runner sharded over the two ranks
    c5 = ["--config5-threads", "128"] if dp_batch == "local" else ["--no-config5"]
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--num-envs", "256",
                        "--num-steps", "32", "--learning-iters", "2", "--full", "--no-cpu-baseline", "--no-config3", "--stream-envs",
                        "2048", "--dp-batch", dp_batch] + c5, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["global_envs"] == 512 and d["scaling"] == "weak"
    assert len(d["per_rank"]) == 2 and all(p["ms_per_step"] > 0 for p in d["per_rank"])
    ex = d["exchange"]
    assert ex["dp_batch"] == dp_batch and ex["host_collectives_world"] == 2 and ex["all_ranks_on_one_gpu"] is True
    assert ex["form"].startswith("in-kernel") and ex["selftest_result"] == [0, 0], ex
    # the start-up auto-tune ran on every rank, pinned ONE form everywhere (the line's `form` is what rank 0's library
    # reports as current; `chosen` is the table's verdict, which the max-reduce over the ranks makes the same on all of them), and
    # lists the round-6 form
    tab = ex["autotune"]
    assert tab and tab.get("chosen") and "default_form" in tab, tab
    assert any(k.startswith("row-split kernel") and v is not None for k, v in tab.items() if k not in ("chosen", "unit", "default_form", "margin")), tab
    assert tab["chosen"] in ex["form"] or tab["chosen"].startswith("kernel /"), (tab["chosen"], ex["form"])
    assert d.get("replicas_identical_after_run") is True, d.get("replicas_identical_after_run")
    per_rank_rows = 64 if dp_batch == "local" else 32
    assert d["config"]["minibatch_steps_per_epoch"] == (256 * 32 // per_rank_rows) * 2
    assert d["value"] == pytest.approx(2 * 256 * 32 / (d["ms_per_step"] * 1e-3), rel=1e-3)
    if dp_batch == "local":
        c = d["config5_mappolag"]
        assert "error" not in c, c
        assert c["n_gpus"] == 2 and c["scaling"] == "strong" and "split over 2 ranks (64 each)" in c["workload"], c
        assert c["env_steps_per_s"] > 0 and c["parallelism"].startswith("dp2 over rollout threads")
    else:
        assert d["config5_mappolag"] is None


def test_bench_plain_run_times_steps_and_dumps_outputs(dev, tmp_path):
    """A plain `bench.py --gpus 1` run prints the headline fields only (no --full sections), times exactly --steps epochs and,
    with --dump-outputs, writes what the last timed epoch computed as float32 / float64 .npy files under 64 MB: the parameters
    after the update, the next observation, the epoch's buffer after collect and GAE, the losses of every minibatch step."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SPO_BENCH_ONE_GPU")}
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--num-envs", "256", "--num-steps", "32", "--learning-iters", "2", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["n_gpus"] == 1 and d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] == pytest.approx(256 * 32 / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert not {"roofline", "cpu_baseline", "config3_cpo", "config5_mappolag", "wide_minibatch_step"} & set(d), sorted(d)
    files = {f.stem: np.load(f) for f in out.glob("*.npy")}
    assert {"theta", "next_obs", "obs", "act", "adv_r", "target_value_r", "losses", "update_stats"} <= set(files), sorted(files)
    assert all(x.dtype in (np.float32, np.float64) for x in files.values())
    assert sum(x.nbytes for x in files.values()) < 64 << 20
    assert files["adv_r"].shape == (256, 32) and files["losses"].shape == (2 * 256 * 32 // 64, 3)
    assert files["update_stats"][0] == 2 and np.isfinite(files["theta"]).all() and np.isfinite(files["losses"]).all()
