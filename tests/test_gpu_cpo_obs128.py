"""GPU tests of the full-batch CPO kernels for 65-128-dim observations (csrc/cpo.hip, KIN = 128; spo_cpo128_*): the Car /
Racecar / Doggo / Ant shapes of the reference's default sweep (single_agent/benchmark.py:5-44) with the default [64, 64]
networks.  WideCPOEngine routes its three full-batch primitives (surrogate gradient cpo.py:356-381, Fisher-vector product
cpo.py:132-157, line-search sums cpo.py:473-491) to them; everything is gated against the CPU oracle (oracle/restatement.py)
with the gates -- and the floors -- of the existing tests named in each docstring.  No element or case is exempted."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_gate as G  # noqa: E402
from oracle import restatement as R  # noqa: E402  (checker only)
from test_gpu_parity import _synthetic_update_problem, _wide_pair  # noqa: E402

SHAPES = [(72, 2), (104, 12), (128, 16), (65, 1)]


@pytest.fixture(autouse=True)
def _leave_no_global_state():
    """The full-size test raises torch's CPU thread count for its float64 oracle; later test files build their float64 problems
    with whatever count they find (blocked sums round differently), so it -- and the CPU generator's state -- is put back."""
    threads, rng = torch.get_num_threads(), torch.get_rng_state()
    yield
    torch.set_num_threads(threads)
    torch.set_rng_state(rng)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _cpo_problem(D, A, hidden, N, T, dev, seed, expect_new_path=True):
    from safepo.single_agent import cpo
    M = N * T
    pol, ref = _wide_pair(D, A, hidden, dev, seed=seed)
    cfg = dict(cpo.default_cfg)
    cfg["hidden_sizes"] = hidden
    eng = cpo.make_engine(pol, N, T, cfg, dev)
    assert type(eng) is cpo.WideCPOEngine
    assert eng._actor_on_full_batch_kernels is expect_new_path
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=seed + 1)
    adv_c = adv.flip(0) * 0.5 + 0.1
    b = eng.buffer
    b.data["obs"].copy_(obs.view(N, T, D)); b.data["act"].copy_(act.view(N, T, A)); b.data["log_prob"].copy_(logp.view(N, T))
    b.data["adv_r"].copy_(adv.view(N, T)); b.data["adv_c"].copy_(adv_c.view(N, T))
    b.data["target_value_r"].copy_(tgt_r.view(N, T)); b.data["target_value_c"].copy_(tgt_c.view(N, T))
    data = {"obs": obs, "act": act, "log_prob": logp, "adv_r": adv, "adv_c": adv_c, "target_value_r": tgt_r, "target_value_c": tgt_c}
    return pol, ref, eng, data


def test_routing(dev, monkeypatch):
    """WideCPOEngine stays the engine for these dims (make_engine / kernels_supported unchanged); the flag that routes its three
    primitives is set exactly for hidden [64, 64], 65 <= obs_dim <= 128, act_dim <= 16 and SPO_CPO_OBS128 != 0."""
    from safepo import _abi
    from safepo.common.model import ActorVCritic
    from safepo.single_agent import cpo
    cfg = dict(cpo.default_cfg)

    def flag(D, A, hidden=(64, 64)):
        c = dict(cfg)
        c["hidden_sizes"] = list(hidden)
        eng = cpo.make_engine(ActorVCritic(D, A, hidden_sizes=list(hidden)).to(dev), 2, 8, c, dev)
        assert type(eng) is cpo.WideCPOEngine
        return eng._actor_on_full_batch_kernels

    monkeypatch.delenv("SPO_CPO_OBS128", raising=False)
    for D, A in SHAPES:
        assert flag(D, A) is True, (D, A)
    assert flag(129, 4) is False
    assert flag(376, 17) is False
    assert flag(72, 2, (128, 128)) is False
    assert flag(72, 17) is False
    monkeypatch.setenv("SPO_CPO_OBS128", "0")
    for D, A in SHAPES:
        assert flag(D, A) is False, (D, A)
    monkeypatch.setenv("SPO_CPO_OBS128", "1")
    assert flag(72, 2) is True
    monkeypatch.delenv("SPO_CPO_OBS128", raising=False)

    # the entry points themselves refuse what lies outside their range, naming the dimension
    lib = _abi.load()
    M = 64
    for D in (64, 129):
        A = 2
        z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
        theta, obs, act, vec = z(lib.spo_param_count(D, A)), z(M, D), z(M, A), z(M)
        Pa = A + 64 * D + 64 + 64 * 64 + 64 + A * 64 + A
        pw, lw, out = z(Pa), z(1, dt=torch.float64), z(Pa)
        p = _abi.ptr
        with pytest.raises(_abi.SpoError, match="obs_dim"):
            _abi.check(lib.spo_cpo128_surrogate_grad(p(theta), p(obs), p(act), p(vec), p(vec), 1.0, M, D, A, p(pw), p(lw), p(out),
                                                     p(lw), _abi.stream_ptr()), "spo_cpo128_surrogate_grad")
        with pytest.raises(_abi.SpoError, match="obs_dim"):
            _abi.check(lib.spo_cpo128_fvp(p(theta), p(obs), p(out), M, D, A, p(pw), p(lw), p(out), _abi.stream_ptr()),
                       "spo_cpo128_fvp")
        with pytest.raises(_abi.SpoError, match="obs_dim"):
            _abi.check(lib.spo_cpo128_linesearch_eval(p(theta), p(obs), p(act), p(vec), p(vec), p(vec), p(act), p(z(A)), M, D, A,
                                                      p(z(3, dt=torch.float64)), 3, p(z(3, dt=torch.float64)), _abi.stream_ptr()),
                       "spo_cpo128_linesearch_eval")


@pytest.mark.parametrize("M", [3037, 1, 63])
@pytest.mark.parametrize("D,A", SHAPES)
def test_cpo128_primitives_vs_oracle(dev, D, A, M):
    """The gates of tests/test_gpu_wide_dims.py::test_wide_cpo_primitives_vs_oracle, on the KIN = 128 kernels: M = 3037 is 47
    64-row chunks and a ragged 29-row tail over 48 workgroups; M = 1 and M = 63 are a single partial chunk.  The KL at unchanged
    parameters is exactly 0 (the snapshot and the line-search kernel run the same LDS-resident forward)."""
    pol, ref, eng, data = _cpo_problem(D, A, [64, 64], 1, M, dev, seed=7 + D)
    eng.CHUNK = 1024            # ignored on this path
    b = eng.buffer
    ref64 = copy.deepcopy(ref).double()
    data64 = {k: v.double() for k, v in data.items()}
    floor = 1e-6 * float(data["adv_r"].abs().mean())
    for which, key, sign in (("r", "adv_r", -1.0), ("c", "adv_c", 1.0)):
        ref.actor.zero_grad()
        loss = R.cpo_surrogate(ref, data, which)
        loss.backward()
        g_ref = R.actor_flat_grads(ref.actor).numpy()
        g, mean = eng.surrogate_grad(b.data[key], sign)
        np.testing.assert_allclose(g.cpu().numpy(), g_ref, rtol=1e-4, atol=1e-5 * np.abs(g_ref).max())
        G.gate(sign * mean, loss.detach(), R.cpo_surrogate(ref64, data64, which).detach(), f"surrogate {which}", floor=floor, norms=G.MAX)
    v = torch.randn(eng.Pa, generator=torch.Generator().manual_seed(3))
    hv32 = R.cpo_fvp(v, ref, data["obs"]).double().numpy()
    hv64 = R.cpo_fvp(v.double(), ref64, data64["obs"]).numpy()
    hv_t = eng.fvp(v.to(dev))
    hv = hv_t.double().cpu().numpy()
    G.gate(hv, hv32, hv64, f"fvp ({D}, {A}, M {M})", norms=G.MAX)
    np.testing.assert_allclose(hv, hv32, rtol=1e-4, atol=1e-5 * np.abs(hv64).max())
    # call-to-call consistency: bit-identical repeats, linear in the direction
    assert torch.equal(hv_t, eng.fvp(v.to(dev)))
    h2 = eng.fvp((2 * v).to(dev))
    np.testing.assert_allclose(h2.cpu().numpy(), 2 * hv_t.cpu().numpy(), rtol=1e-5, atol=1e-7 * float(hv_t.abs().max()))
    g1, m1 = eng.surrogate_grad(b.data["adv_r"], -1.0)
    g2, m2 = eng.surrogate_grad(b.data["adv_r"], -1.0)
    assert torch.equal(g1, g2) and m1 == m2
    # line search: unchanged parameters -> KL == 0 and the two surrogates; moved parameters -> the oracle's values
    eng.snapshot_old_distribution()
    l_r, l_c, kl = eng.linesearch_eval()
    assert kl == 0.0
    assert (l_r, l_c, kl) == eng.linesearch_eval()
    with torch.no_grad():
        G.gate(l_r, R.cpo_surrogate(ref, data, "r"), R.cpo_surrogate(ref64, data64, "r"), "line search r at theta_old", floor=floor, norms=G.MAX)
        G.gate(l_c, R.cpo_surrogate(ref, data, "c"), R.cpo_surrogate(ref64, data64, "c"), "line search c at theta_old", floor=floor, norms=G.MAX)

        def moved(rf, dt):
            old = rf.actor(dt["obs"])
            old_mean, old_std = old.mean.clone(), old.stddev.clone()
            R.actor_set_flat_params(rf.actor, R.actor_flat_params(rf.actor) + delta.to(old_mean.dtype))
            kl_ = torch.distributions.kl_divergence(torch.distributions.Normal(old_mean, old_std), rf.actor(dt["obs"])).mean()
            return float(kl_), float(R.cpo_surrogate(rf, dt, "r")), float(R.cpo_surrogate(rf, dt, "c"))
        delta = 0.02 * torch.randn(eng.Pa, generator=torch.Generator().manual_seed(5))
        eng.theta_actor.add_(delta.to(dev))
        kl32, r32, c32 = moved(ref, data)
        kl64, r64, c64 = moved(ref64, data64)
    l_r, l_c, kl = eng.linesearch_eval()
    assert kl == pytest.approx(kl32, rel=1e-4)
    G.gate(kl, kl32, kl64, "KL at moved parameters", floor=1e-6 * kl64, norms=G.MAX)
    G.gate(l_r, r32, r64, "line search r at moved parameters", floor=floor, norms=G.MAX)
    G.gate(l_c, c32, c64, "line search c at moved parameters", floor=floor, norms=G.MAX)


@pytest.mark.parametrize("D,A", [(72, 2), (128, 16)])
def test_cpo128_full_size_surrogate_gradients_and_fvp_fp64_yardstick(dev, D, A):
    """tests/test_gpu_parity.py::test_cpo_full_size_surrogate_gradients_and_fvp_fp64_yardstick at Car-class and at the largest
    supported dims: 4096 x 128 = 524 288 rows (256 workgroups x 32 chunks, per-workgroup partial vectors, fixed-order reduction),
    the norm and max gates with the same floor_rel = 2e-7."""
    torch.set_num_threads(8)
    N, T = 4096, 128
    pol, ref32, eng, data32 = _cpo_problem(D, A, [64, 64], N, T, dev, seed=31 + D)
    b = eng.buffer
    ref64 = copy.deepcopy(ref32).double()
    data64 = {k: v.double() for k, v in data32.items()}

    def gate(name, hip, v32, v64, floor_rel=2e-7):
        G.gate(hip, v32, v64, f"cpo128 full size ({D}, {A}) {name}", rel_floor=floor_rel, norms=G.L2)
        G.gate(hip, v32, v64, f"cpo128 full size ({D}, {A}) {name}", floor=floor_rel * np.abs(v64).max() * 8, norms=G.MAX)

    for which, key, sign in (("r", "adv_r", -1.0), ("c", "adv_c", 1.0)):
        outs = []
        for ref, data in ((ref32, data32), (ref64, data64)):
            ref.actor.zero_grad()
            loss = R.cpo_surrogate(ref, data, which)
            loss.backward()
            outs.append((R.actor_flat_grads(ref.actor).double().numpy().copy(), float(loss.detach())))
        g, mean = eng.surrogate_grad(b.data[key], sign)
        gate(f"surrogate gradient {which}", g.cpu().numpy(), outs[0][0], outs[1][0])
        with torch.no_grad():
            lp64 = ref64.actor(data64["obs"]).log_prob(data64["act"]).sum(-1)
            term_scale = float((torch.exp(lp64 - data64["log_prob"]) * data64[key]).abs().mean())
        G.gate(sign * mean, outs[0][1], outs[1][1], f"cpo128 full size ({D}, {A}) surrogate value {which}", scale=term_scale, rel_floor=1e-7, norms=G.MAX)
    v = torch.randn(eng.Pa, generator=torch.Generator().manual_seed(5))
    hv32 = R.cpo_fvp(v, ref32, data32["obs"]).double().numpy()
    hv64 = R.cpo_fvp(v.double(), ref64, data64["obs"]).numpy()
    h1 = eng.fvp(v.to(dev))
    gate("Fisher-vector product", h1.cpu().numpy(), hv32, hv64)
    assert torch.equal(h1, eng.fvp(v.to(dev)))


def _actor_step_check(dev, D, A, ep_costs, expect_new_path):
    """The body of tests/test_gpu_wide_dims.py::test_wide_cpo_actor_step_drift_envelope."""
    M = 4096
    pol, ref32, eng, data32 = _cpo_problem(D, A, [64, 64], 1, M, dev, seed=14, expect_new_path=expect_new_path)
    eng.CHUNK = 1500
    ref64 = copy.deepcopy(ref32).double()
    data64 = {k: v.double() for k, v in data32.items()}
    tk = eng.cfg["target_kl"]
    o32 = R.cpo_policy_update(ref32, data32, ep_costs, target_kl=tk)
    o64 = R.cpo_policy_update(ref64, data64, ep_costs, target_kl=tk)
    th32 = R.actor_flat_params(ref32.actor).double().numpy()
    th64 = R.actor_flat_params(ref64.actor).double().numpy()
    out = eng.policy_update(ep_costs)
    th_hip = eng.theta_actor.double().cpu().numpy()
    assert out["case"] == o32["case"] == o64["case"]
    assert out["acceptance_step"] == o32["accept"] == o64["accept"]
    for name, hip, v32, v64 in (("xHx", out["xHx"], float(o32["xHx"]), float(o64["xHx"])),
                                ("alpha", out["alpha"], float(o32["alpha"]), float(o64["alpha"]))):
        G.gate(hip, v32, v64, f"step ({D}, {A}, {ep_costs}) {name}", rel_floor=2e-6, norms=G.MAX)
    G.gate(th_hip, th32, th64, f"step ({D}, {A}, {ep_costs}) theta", rel_floor=1e-7, norms=G.L2)
    G.gate(th_hip, th32, th64, f"step ({D}, {A}, {ep_costs}) theta", norms=G.MAX)
    np.testing.assert_allclose(eng.flat_grad[eng.ls_off:].cpu().numpy(), out["b"].cpu().numpy())


@pytest.mark.parametrize("ep_costs", [-1.0, 0.3])
@pytest.mark.parametrize("D,A", [(72, 2), (104, 12)])
def test_cpo128_actor_step_drift_envelope(dev, D, A, ep_costs, monkeypatch):
    """CPO's whole trust-region step (cpo.py:350-532) with the three primitives on the KIN = 128 kernels."""
    monkeypatch.delenv("SPO_CPO_OBS128", raising=False)
    _actor_step_check(dev, D, A, ep_costs, True)


@pytest.mark.parametrize("ep_costs", [-1.0, 0.3])
@pytest.mark.parametrize("D,A", [(72, 2), (104, 12)])
def test_chunked_wide_path_unchanged_under_the_knob(dev, D, A, ep_costs, monkeypatch):
    """SPO_CPO_OBS128=0: the same step on the launch-per-layer wide kernels in row chunks, same gates."""
    monkeypatch.setenv("SPO_CPO_OBS128", "0")
    _actor_step_check(dev, D, A, ep_costs, False)


def test_reference_trace_at_car_dims_runs_on_the_new_kernels(dev, golden_dir, monkeypatch):
    """tests/golden/cpo_trace_car.npz (the reference's cpo.main() at 72 / 2) through
    test_second_order_family_traces_under_the_fp64_yardstick[cpo_car]'s own gates, with the engine asserted to be on the
    KIN = 128 kernels and every primitive call counted."""
    import test_gpu_parity as P
    from safepo.single_agent import cpo
    monkeypatch.delenv("SPO_CPO_OBS128", raising=False)
    made, calls = [], {"surr": 0, "fvp": 0, "ls": 0}
    inner = P._cpo_engine

    def engine(*a, **k):
        pol, eng = inner(*a, **k)
        assert type(eng) is cpo.WideCPOEngine and eng._actor_on_full_batch_kernels is True
        lib = eng.lib

        class Counting:
            def __getattr__(self, name):
                fn = getattr(lib, name)
                key = {"spo_cpo128_surrogate_grad": "surr", "spo_cpo128_fvp": "fvp", "spo_cpo128_linesearch_eval": "ls"}.get(name)
                assert not name.startswith(("spo_mlp_jvp", "spo_wide_fvp_cotangent", "spo_wide_linesearch_sums")), name   # the chunked path
                if key is None:
                    return fn

                def counted(*args):
                    calls[key] += 1
                    return fn(*args)
                return counted
        eng.lib = Counting()
        made.append(eng)
        return pol, eng

    monkeypatch.setattr(P, "_cpo_engine", engine)
    P.test_second_order_family_traces_under_the_fp64_yardstick(dev, golden_dir, "cpo_car")
    assert len(made) == 1
    assert calls["surr"] >= 2 and calls["fvp"] >= 10 and calls["ls"] >= 1, calls
