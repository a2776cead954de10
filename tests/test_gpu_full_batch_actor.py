"""GPU tests of the full-batch actor kernels for obs_dim <= 64 at every width form, under the float64 yardstick.

1. spo_cpo_surrogate_grad / spo_cpo_fvp / spo_cpo_linesearch_eval (csrc/cpo.hip, KIN 16 / 32 / 64) through CPOEngine: g, b, every
   conjugate-gradient product and every line-search accept / reject of cpo, pcpo, rcpo, trpo_lag, trpo and natural_pg.
2. spo_actor_mean / spo_actor_kl (actor_full_kernel of csrc/policy.hip, KIN 16 / 32 / 64 / 128) by direct ABI calls: the
   old-distribution snapshot and the early-stop KL of every first-order script.

The reference is the same operation in plain torch float64 on the CPU (oracle/restatement.py, autograd,
torch.distributions.kl_divergence), the yardstick the same oracle in float32, and a HIP result passes when
|hip - f64| <= 3 |f32 - f64| + floor, with the floors of tests/test_gpu_cpo_obs128.py::test_cpo128_primitives_vs_oracle (1e-6 of
mean|adv_r|, of max|f64|, of kl64).  Scalars of one kind are gated across all shapes of one row count (envelope.gate_scalars: one
scalar's |f32 - f64| is a single draw of rounding noise), vectors with envelope.gate_array.  No element, case or shape is exempted.
The cases, their problems and oracles and the gates are in tests/full_batch_actor_cases.py; after the last test of this file the
worst ratio |hip - f64| / (3 |f32 - f64| + floor) per (entry point, KIN form, rows) is printed (profiles/full_batch_actor/)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import full_batch_actor_cases as C  # noqa: E402


@pytest.fixture(autouse=True)
def _leave_no_global_state():
    threads, rng = torch.get_num_threads(), torch.get_rng_state()
    yield
    torch.set_num_threads(threads)
    torch.set_rng_state(rng)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    C.RATIOS.clear()
    yield torch.device("cuda:0")
    print("\n==== worst gate ratios (<= 1 passes) ====\n" + C.ratio_table() + "\n==== end of gate ratios ====")


# --------------------------------------------------------------------------------------------------------- 1. csrc/cpo.hip
def _cpo_engine(dev, D, A, M):
    """CPOEngine over case (D, A, M): 1 env x M steps, the buffer filled with the case's batch."""
    from safepo.common.model import ActorVCritic
    from safepo.single_agent.cpo import CPOEngine, default_cfg
    p = C.cpo_problem(D, A, M)
    pol = ActorVCritic(D, A)
    pol.load_state_dict(p["state_dict"])
    pol = pol.to(dev)
    eng = CPOEngine(pol, 1, M, dict(default_cfg), dev)
    assert eng.Pa == p["Pa"] and eng.lib.spo_cpo_num_partials(M) == min((M + 63) // 64, 256)
    d = eng.buffer.data
    for k, v in p["data"].items():
        d[k].copy_(v.view(d[k].shape))
    return eng, p


def _snapshot_and_move(eng, p):
    eng.snapshot_old_distribution()
    with torch.no_grad():
        eng.theta_actor.add_(p["delta"].to(eng.dev))


@pytest.mark.parametrize("M", list(C.CPO_CASES))
def test_cpo_primitives_vs_fp64_oracle(dev, M):
    """Every shape of this row count: both surrogate gradients (log_std != 0), the Fisher-vector product of a seeded direction
    with its log_std block and damping, and the line search at the snapshot and at moved parameters (log_std moved too).
    M = 3037 is 47 chunks and a 29-row tail, one per workgroup; M = 1 and 63 a single partial chunk; M = 16 477 the smallest
    count at which a workgroup accumulates over two chunks (c += gridDim.x), one of them ragged."""
    groups = {k: [] for k in ("surrogate mean", "line search at theta_old", "line search at moved parameters", "KL at moved parameters")}
    entry = {"surrogate mean": "spo_cpo_surrogate_grad"}
    for D, A in C.CPO_CASES[M]:
        eng, p = _cpo_engine(dev, D, A, M)
        o32, o64 = C.cpo_oracle(D, A, M, "float32"), C.cpo_oracle(D, A, M, "float64")
        tag, s, d = f"({D}, {A}, M {M})", o64["adv_scale"], eng.buffer.data
        for which, key, sign in (("r", "adv_r", -1.0), ("c", "adv_c", 1.0)):
            g, mean = eng.surrogate_grad(d[key], sign)
            C.gate_vector("spo_cpo_surrogate_grad", D, M, g.cpu().numpy(), o32["grad_" + which], o64["grad_" + which], f"surrogate gradient {which} {tag}")
            groups["surrogate mean"].append((f"{which} {tag}", D, sign * mean, o32["loss_" + which], o64["loss_" + which], s))
            g2, mean2 = eng.surrogate_grad(d[key], sign)
            assert torch.equal(g, g2) and mean == mean2, tag
        # Fisher-vector product: H v + 0.1 v with the 2 / A diagonal on log_std
        v, u = p["v"].to(dev), p["u"].to(dev)
        Fv = eng.fvp(v)
        C.gate_vector("spo_cpo_fvp", D, M, Fv.cpu().numpy(), o32["Fv"], o64["Fv"], f"fvp {tag}")
        assert torch.equal(Fv, eng.fvp(v)), tag
        np.testing.assert_allclose(eng.fvp(2 * v).cpu().numpy(), 2 * Fv.cpu().numpy(), rtol=1e-5, atol=1e-7 * float(Fv.abs().max()))
        raw = eng._fvp_local(v).double().cpu().numpy()           # J^T diag(1 / sigma^2) J v / (M A): no damping, no log_std diagonal
        assert (raw[:A] == 0).all() and float(p["v"].double().numpy() @ raw) >= 0.0, tag
        uFv, vFu = float(p["u"].double().numpy() @ Fv.double().cpu().numpy()), float(p["v"].double().numpy() @ eng.fvp(u).double().cpu().numpy())
        asym32, floor = abs(o32["uFv"] - o32["vFu"]), 1e-6 * abs(o64["uFv"])
        print(f"fvp symmetry {tag}: |u.Fv - v.Fu| hip {abs(uFv - vFu):.3e}  f32 {asym32:.3e}  floor {floor:.3e}")
        assert abs(uFv - vFu) <= 3.0 * asym32 + floor, (tag, uFv, vFu, asym32, floor)
        # line search: the snapshot is net_forward_lean's, the line search net_forward's -> no exact zero promised here
        eng.snapshot_old_distribution()
        l_r, l_c, kl = eng.linesearch_eval()
        print(f"line search at theta_old {tag}: kl {kl:.3e}")
        assert kl == pytest.approx(0.0, abs=1e-9), tag
        assert (l_r, l_c, kl) == eng.linesearch_eval(), tag
        for which, hip in (("r", l_r), ("c", l_c)):
            groups["line search at theta_old"].append((f"{which} {tag}", D, hip, o32["loss_" + which], o64["loss_" + which], s))
        with torch.no_grad():
            eng.theta_actor.add_(p["delta"].to(dev))
        l_r, l_c, kl = eng.linesearch_eval()
        for which, hip in (("r", l_r), ("c", l_c)):
            k = "moved_loss_" + which
            groups["line search at moved parameters"].append((f"{which} {tag}", D, hip, o32[k], o64[k], s))
        groups["KL at moved parameters"].append((tag, D, kl, o32["moved_kl"], o64["moved_kl"], None))
    for what, members in groups.items():
        C.gate_group(entry.get(what, "spo_cpo_linesearch_eval"), M, members, what)


@pytest.mark.parametrize("capacity", C.LS_CAPPED)
def test_cpo_linesearch_capped_grid(dev, capacity):
    """spo_cpo_linesearch_eval called directly at M = 3037 with room for one (capacity 3: each wave walks 48 tiles) and two
    (capacity 7) workgroups' partials, at moved parameters, under the gates of the full grid; room for none is refused."""
    from safepo import _abi
    M = C.CPO_ROWS_ALL
    losses, kls = [], []
    for D, A in C.CPO_CASES[M]:
        eng, p = _cpo_engine(dev, D, A, M)
        o32, o64 = C.cpo_oracle(D, A, M, "float32"), C.cpo_oracle(D, A, M, "float64")
        _snapshot_and_move(eng, p)
        d, ptr = eng.buffer.data, _abi.ptr
        parts = torch.full((capacity,), float("nan"), dtype=torch.float64, device=dev)
        sums = torch.zeros(3, dtype=torch.float64, device=dev)
        call = lambda cap: eng.lib.spo_cpo_linesearch_eval(
            ptr(eng.policy.theta), ptr(d["obs"]), ptr(d["act"]), ptr(d["log_prob"]), ptr(d["adv_r"]), ptr(d["adv_c"]), ptr(eng.mean_old),
            ptr(eng.logstd_old), M, D, A, ptr(parts), cap, ptr(sums), _abi.stream_ptr())
        _abi.check(call(capacity), "spo_cpo_linesearch_eval")
        sm = sums.cpu()
        assert int(torch.isfinite(parts).sum()) == 3 * (capacity // 3)            # one triple per launched workgroup, nothing beyond
        tag, s = f"({D}, {A}, capacity {capacity})", o64["adv_scale"]
        losses.append((f"r {tag}", D, -float(sm[0]) / M, o32["moved_loss_r"], o64["moved_loss_r"], s))
        losses.append((f"c {tag}", D, float(sm[1]) / M, o32["moved_loss_c"], o64["moved_loss_c"], s))
        kls.append((tag, D, float(sm[2]) / (M * A), o32["moved_kl"], o64["moved_kl"], None))
        with pytest.raises(_abi.SpoError, match="partial capacity too small"):
            _abi.check(call(2), "spo_cpo_linesearch_eval")
    entry = f"spo_cpo_linesearch_eval/cap{capacity}"
    C.gate_group(entry, M, losses, "capped line search at moved parameters")
    C.gate_group(entry, M, kls, "capped KL at moved parameters")


# ------------------------------------------------------------------------------------------------------ 2. csrc/policy.hip
def _actor(dev, D, A, rows):
    from safepo.common.model import ActorVCritic
    p = C.actor_problem(D, A, rows)
    pol = ActorVCritic(D, A)
    pol.load_state_dict(p["state_dict"])
    theta = pol.to(dev).theta
    off = pol.log_std_offset
    return theta, p["obs"].to(dev), off, p


def _means(theta, obs, rows, D, A, skip=0, out=None):
    """spo_actor_mean over rows [skip, rows) with the obs and output pointers advanced by `skip` rows.  The float4 loads of the
    D % 4 == 0 path need 16-byte-aligned rows: torch's allocations are, and skip * D * 4 bytes is a multiple of 16 there."""
    from safepo import _abi
    out = torch.full((rows, A), float("nan"), dtype=torch.float32, device=obs.device) if out is None else out
    obs_ptr = obs.data_ptr() + 4 * skip * D
    assert D % 4 != 0 or obs_ptr % 16 == 0
    _abi.check(_abi.load().spo_actor_mean(_abi.ptr(theta), obs_ptr, out.data_ptr() + 4 * skip * A, rows - skip, D, A, _abi.stream_ptr()),
               "spo_actor_mean")
    return out


def _kl_sum(theta, obs, mean_old, logstd_old, rows, D, A, capacity=1024):
    from safepo import _abi
    parts = torch.full((max(capacity, 1),), float("nan"), dtype=torch.float64, device=obs.device)
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=obs.device)
    _abi.check(_abi.load().spo_actor_kl(_abi.ptr(theta), _abi.ptr(obs), _abi.ptr(mean_old), _abi.ptr(logstd_old), _abi.ptr(parts), capacity,
                                        _abi.ptr(out), rows, D, A, _abi.stream_ptr()), "spo_actor_kl")
    assert int(torch.isfinite(parts).sum()) == min((rows + 63) // 64, 768, capacity)          # one partial per launched workgroup
    return float(out.item())


def _snapshot_then_kl(dev, D, A, rows, capacity=1024):
    """-> (means, KL at unchanged theta, KL(old || moved) per row) of case (D, A, rows), the way the engines use the two calls."""
    theta, obs, off, p = _actor(dev, D, A, rows)
    means = _means(theta, obs, rows, D, A)
    logstd_old = theta[off:off + A].clone()
    kl0 = _kl_sum(theta, obs, means, logstd_old, rows, D, A, capacity)
    theta.add_(p["delta"].to(dev))
    return means, kl0, _kl_sum(theta, obs, means, logstd_old, rows, D, A, capacity) / rows


@pytest.mark.parametrize("rows", C.ACTOR_ROWS)
def test_actor_mean_and_kl_vs_fp64_oracle(dev, rows):
    """Every shape at this row count: the per-row means against the float64 forward, KL == 0.0 exactly at unchanged theta (MODE 0
    and MODE 1 run the same net_forward_lean), and KL(old || moved) / rows with theta -- log_std included -- moved."""
    kls = []
    for D, A in C.ACTOR_SHAPES:
        o32, o64 = C.actor_oracle(D, A, rows, "float32"), C.actor_oracle(D, A, rows, "float64")
        means, kl0, kl = _snapshot_then_kl(dev, D, A, rows)
        tag = f"({D}, {A}, rows {rows})"
        C.gate_vector("spo_actor_mean", D, rows, means.cpu().numpy(), o32["mean"], o64["mean"], f"means {tag}")
        assert kl0 == 0.0, (tag, kl0)
        kls.append((tag, D, kl, o32["kl"], o64["kl"], None))
    C.gate_group("spo_actor_kl", rows, kls, "KL at moved parameters")


@pytest.mark.parametrize("D,A", C.ACTOR_SHAPES)
def test_actor_mean_is_position_independent(dev, D, A):
    """The means of rows [k, M) computed on their own (pointers advanced by k rows) are bit-identical to rows k..M of the full
    call: k = 16 shifts every row by one tile, 37 and 1 move it to another lane of another tile, and the tail tile, the
    clamped rows and the tiles a wave picks up all change with k."""
    for rows in C.ACTOR_ROWS:
        theta, obs, _, _ = _actor(dev, D, A, rows)
        full = _means(theta, obs, rows, D, A)
        assert bool(torch.isfinite(full).all())
        for k in ((1, 16, 37) if D % 4 else (16, 37)):
            if k >= rows:
                continue
            part = _means(theta, obs, rows, D, A, skip=k)
            assert bool(torch.isnan(part[:k]).all()), (rows, k)                      # nothing written in front of the pointer
            assert torch.equal(part[k:], full[k:]), (rows, k, float((part[k:] - full[k:]).abs().max()))


@pytest.mark.parametrize("capacity", C.KL_CAPPED)
def test_actor_kl_capped_grid_runs_the_loop_body_again(dev, capacity):
    """kl_partials_capacity 1 and 2 at 1000 rows: 63 tiles over 4 and 8 waves, 16 and 8 trips through prefetch, mask and consume
    (the full grid makes one).  Under the float64 gate; not bit-equal to the full grid (the sums are taken in another order)."""
    rows, kls = 1000, []
    for D, A in C.ACTOR_SHAPES:
        o32, o64 = C.actor_oracle(D, A, rows, "float32"), C.actor_oracle(D, A, rows, "float64")
        _, kl0, kl = _snapshot_then_kl(dev, D, A, rows, capacity)
        assert kl0 == 0.0, (D, A, kl0)
        kls.append((f"({D}, {A}, capacity {capacity})", D, kl, o32["kl"], o64["kl"], None))
    C.gate_group(f"spo_actor_kl/cap{capacity}", rows, kls, "capped KL at moved parameters")


def test_actor_second_tile_under_the_default_grid(dev):
    """49 169 rows at (6, 2): the first count at which a wave of the 768-workgroup grid takes a second tile, and the last of
    those tiles is ragged.  Both entry points under the float64 gates; the means are bit-identical to the same rows computed
    in two calls of 49 152 and 17 rows."""
    D, A, rows = C.ACTOR_SECOND_TILE
    o32, o64 = C.actor_oracle(D, A, rows, "float32"), C.actor_oracle(D, A, rows, "float64")
    theta, obs, _, _ = _actor(dev, D, A, rows)
    head = 768 * 64
    two = _means(theta, obs, head, D, A, out=torch.full((rows, A), float("nan"), dtype=torch.float32, device=dev))
    assert bool(torch.isnan(two[head:]).all())
    _means(theta, obs, rows, D, A, skip=head, out=two)
    means, kl0, kl = _snapshot_then_kl(dev, D, A, rows)
    tag = f"({D}, {A}, rows {rows})"
    C.gate_vector("spo_actor_mean", D, rows, means.cpu().numpy(), o32["mean"], o64["mean"], f"means {tag}")
    assert torch.equal(means, two)
    assert kl0 == 0.0
    C.gate_group("spo_actor_kl", rows, [(tag, D, kl, o32["kl"], o64["kl"], None)], "KL at moved parameters")


def test_actor_entry_points_refuse_what_lies_outside(dev):
    from safepo import _abi
    lib, p, st = _abi.load(), _abi.ptr, _abi.stream_ptr()
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    rows = 16
    for D, A, word in ((129, 4, "obs_dim"), (64, 17, "act_dim")):
        theta, obs, mean, ls = z(3 * (64 * D + 64 * 64 + 64 * 17 + 256)), z(rows, D), z(rows, A), z(A)
        with pytest.raises(_abi.SpoError, match=word):
            _abi.check(lib.spo_actor_mean(p(theta), p(obs), p(mean), rows, D, A, st), "spo_actor_mean")
        with pytest.raises(_abi.SpoError, match=word):
            _abi.check(lib.spo_actor_kl(p(theta), p(obs), p(mean), p(ls), p(z(4, dt=torch.float64)), 4, p(z(1, dt=torch.float64)), rows, D, A, st),
                       "spo_actor_kl")
    D, A = 12, 2
    theta, obs, _, _ = _actor(dev, D, A, 17)
    with pytest.raises(_abi.SpoError, match="capacity"):
        _abi.check(lib.spo_actor_kl(p(theta), p(obs), p(z(17, A)), p(z(A)), p(z(1, dt=torch.float64)), 0, p(z(1, dt=torch.float64)), 17, D, A, st),
                   "spo_actor_kl")
