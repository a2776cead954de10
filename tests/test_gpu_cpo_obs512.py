"""GPU tests of the full-batch CPO kernels for 129-512-dim observations and up to 32 actions (csrc/cpo.hip, spo_cpo512_*: W1
streamed through LDS in 64-feature slices, two output tiles): HumanoidVelocity's 376 / 17 with the default [64, 64] networks, the
last shape of the reference's default sweep (single_agent/benchmark.py:5-44) whose actor step ran on the chunked wide path.
WideCPOEngine routes its three full-batch primitives (surrogate gradient cpo.py:356-381, Fisher-vector product cpo.py:132-157,
line-search sums cpo.py:473-491) and the snapshot of the old means (cpo.py:361) to them under `_actor_on_streamed_kernels`.
Everything is gated against the CPU oracle (oracle/restatement.py) with the gates -- and the floors -- of
tests/test_gpu_cpo_obs128.py; the cases and their oracle values live in tests/cpo_obs512_cases.py, computed once and shared.
Every test sets SPO_CPO_OBS512 itself.  No element or case is exempted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cpo_obs512_cases as C  # noqa: E402
import fp64_gate as G  # noqa: E402
from test_gpu_cpo_obs128 import _actor_step_check  # noqa: E402


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
    return torch.device("cuda:0")


def _engine_for(D, A, hidden, dev, rows=(2, 8)):
    from safepo.common.model import ActorVCritic
    from safepo.single_agent import cpo
    cfg = dict(cpo.default_cfg)
    cfg["hidden_sizes"] = list(hidden)
    eng = cpo.make_engine(ActorVCritic(D, A, hidden_sizes=list(hidden)).to(dev), rows[0], rows[1], cfg, dev)
    assert type(eng) is cpo.WideCPOEngine
    return eng


def test_routing(dev, monkeypatch):
    """WideCPOEngine stays the engine for these dims; `_actor_on_streamed_kernels` is set exactly for hidden [64, 64],
    129 <= obs_dim <= 512, act_dim <= 32 and SPO_CPO_OBS512 != 0, and `_actor_on_full_batch_kernels` keeps its meaning."""
    from safepo import _abi
    on = [(129, 1), (376, 17), (512, 32)]
    off = [(128, 16, (64, 64)), (513, 4, (64, 64)), (376, 33, (64, 64)), (376, 17, (128, 128))]
    monkeypatch.delenv("SPO_CPO_OBS128", raising=False)
    full_batch = lambda D, A, hidden: tuple(hidden) == (64, 64) and 65 <= D <= 128 and A <= 16
    for knob in ("1", "0"):
        monkeypatch.setenv("SPO_CPO_OBS512", knob)
        for D, A in on:
            eng = _engine_for(D, A, (64, 64), dev)
            assert eng._actor_on_streamed_kernels is (knob == "1"), (D, A, knob)
            assert eng._actor_on_full_batch_kernels is False, (D, A, knob)
        for D, A, hidden in off:
            eng = _engine_for(D, A, hidden, dev)
            assert eng._actor_on_streamed_kernels is False, (D, A, hidden, knob)
            assert eng._actor_on_full_batch_kernels is full_batch(D, A, hidden), (D, A, hidden, knob)

    # the entry points themselves, called on the device, refuse what lies outside their range, naming the dimension
    lib = _abi.load()
    M = 64
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    p = _abi.ptr
    for D, A, word in ((128, 2, "obs_dim"), (513, 2, "obs_dim"), (376, 33, "act_dim")):
        Pa = A + 64 * D + 64 + 64 * 64 + 64 + A * 64 + A
        theta, obs, act, vec = z(2 * (64 * D + 64 + 64 * 64 + 64 + 64 + 1) + Pa), z(M, D), z(M, A), z(M)
        pw, lw, out, d3 = z(Pa), z(1, dt=torch.float64), z(Pa), z(3, dt=torch.float64)
        with pytest.raises(_abi.SpoError, match=word):
            _abi.check(lib.spo_cpo512_surrogate_grad(p(theta), p(obs), p(act), p(vec), p(vec), 1.0, M, D, A, p(pw), p(lw), p(out),
                                                     p(lw), _abi.stream_ptr()), "spo_cpo512_surrogate_grad")
        with pytest.raises(_abi.SpoError, match=word):
            _abi.check(lib.spo_cpo512_fvp(p(theta), p(obs), p(out), M, D, A, p(pw), p(lw), p(out), _abi.stream_ptr()),
                       "spo_cpo512_fvp")
        with pytest.raises(_abi.SpoError, match=word):
            _abi.check(lib.spo_cpo512_linesearch_eval(p(theta), p(obs), p(act), p(vec), p(vec), p(vec), p(act), p(z(A)), M, D, A,
                                                      p(d3), 3, p(d3), _abi.stream_ptr()), "spo_cpo512_linesearch_eval")
        with pytest.raises(_abi.SpoError, match=word):
            _abi.check(lib.spo_cpo512_actor_mean(p(theta), p(obs), p(act), M, D, A, _abi.stream_ptr()), "spo_cpo512_actor_mean")


def _case_engine(D, A, M, dev):
    """The engine of case (D, A, M) with tests/cpo_obs512_cases.py's parameters and batch loaded (one environment, M steps)."""
    from safepo.common.model import ActorVCritic
    from safepo.single_agent import cpo
    p = C.problem(D, A, M)
    pol = ActorVCritic(D, A, hidden_sizes=[64, 64])
    pol.load_state_dict({k: v.clone() for k, v in p["state_dict"].items()})
    pol = pol.to(dev)
    cfg = dict(cpo.default_cfg)
    cfg["hidden_sizes"] = [64, 64]
    eng = cpo.make_engine(pol, 1, M, cfg, dev)
    assert type(eng) is cpo.WideCPOEngine and eng._actor_on_streamed_kernels is True
    b, d = eng.buffer, p["data"]
    b.data["obs"].copy_(d["obs"].view(1, M, D)); b.data["act"].copy_(d["act"].view(1, M, A)); b.data["log_prob"].copy_(d["log_prob"].view(1, M))
    b.data["adv_r"].copy_(d["adv_r"].view(1, M)); b.data["adv_c"].copy_(d["adv_c"].view(1, M))
    b.data["target_value_r"].copy_(d["target_value_r"].view(1, M)); b.data["target_value_c"].copy_(d["target_value_c"].view(1, M))
    return p, eng


@pytest.mark.parametrize("D,A,M", C.CASES)
def test_cpo512_primitives_vs_oracle(dev, D, A, M, monkeypatch):
    """The body and gates of tests/test_gpu_cpo_obs128.py::test_cpo128_primitives_vs_oracle on the streamed-W1 kernels.  M = 3037
    is 47 64-row chunks and a ragged 29-row tail over 48 workgroups; M = 1 and M = 63 are a single partial chunk; 16 477 rows make
    workgroups 0 and 1 walk two chunks (the second of workgroup 1 is the tail); at 49 157 rows every workgroup accumulates over
    three chunks and workgroup 0 takes a fourth of 5 rows (surrogate gradient and Fisher-vector product only).  The KL at unchanged
    parameters is exactly 0: the snapshot (spo_cpo512_actor_mean) and the line-search kernel run the same forward."""
    monkeypatch.setenv("SPO_CPO_OBS512", "1")
    p, eng = _case_engine(D, A, M, dev)
    eng.CHUNK = 1024            # ignored on this path
    b = eng.buffer
    o32, o64 = C.oracle(D, A, M, "float32"), C.oracle(D, A, M, "float64")
    floor = o64["floor"]
    for which, key, sign in (("r", "adv_r", -1.0), ("c", "adv_c", 1.0)):
        g_ref = o32["grad_" + which]
        g, mean = eng.surrogate_grad(b.data[key], sign)
        np.testing.assert_allclose(g.cpu().numpy(), g_ref, rtol=1e-4, atol=1e-5 * np.abs(g_ref).max())
        G.gate(sign * mean, o32["loss_" + which], o64["loss_" + which], f"surrogate {which}", floor=floor, norms=G.MAX)
    v = p["v"]
    hv_t = eng.fvp(v.to(dev))
    C.gate_fvp(hv_t.double().cpu().numpy(), o32["Fv"], o64["Fv"], f"({D}, {A}, M {M})")
    # call-to-call consistency: bit-identical repeats, linear in the direction
    assert torch.equal(hv_t, eng.fvp(v.to(dev)))
    h2 = eng.fvp((2 * v).to(dev))
    np.testing.assert_allclose(h2.cpu().numpy(), 2 * hv_t.cpu().numpy(), rtol=1e-5, atol=1e-7 * float(hv_t.abs().max()))
    g1, m1 = eng.surrogate_grad(b.data["adv_r"], -1.0)
    g2, m2 = eng.surrogate_grad(b.data["adv_r"], -1.0)
    assert torch.equal(g1, g2) and m1 == m2
    if not C.line_search_checked(M):
        return
    # line search: unchanged parameters -> KL == 0 and the two surrogates; moved parameters -> the oracle's values
    eng.snapshot_old_distribution()
    l_r, l_c, kl = eng.linesearch_eval()
    assert kl == 0.0
    assert (l_r, l_c, kl) == eng.linesearch_eval()
    G.gate(l_r, o32["loss_r"], o64["loss_r"], "line search r at theta_old", floor=floor, norms=G.MAX)
    G.gate(l_c, o32["loss_c"], o64["loss_c"], "line search c at theta_old", floor=floor, norms=G.MAX)
    eng.theta_actor.add_(p["delta"].to(dev))
    l_r, l_c, kl = eng.linesearch_eval()
    assert kl == pytest.approx(o32["moved_kl"], rel=1e-4)
    G.gate(kl, o32["moved_kl"], o64["moved_kl"], "KL at moved parameters", floor=1e-6 * o64["moved_kl"], norms=G.MAX)
    G.gate(l_r, o32["moved_loss_r"], o64["moved_loss_r"], "line search r at moved parameters", floor=floor, norms=G.MAX)
    G.gate(l_c, o32["moved_loss_c"], o64["moved_loss_c"], "line search c at moved parameters", floor=floor, norms=G.MAX)


def test_snapshot_means_match_the_oracle(dev, monkeypatch):
    """spo_cpo512_actor_mean through snapshot_old_distribution at 376 / 17, 3037 rows: every mean under the fp64 yardstick
    (3 x the float32 oracle's own distance + 1e-6 of the scale), log_std and std snapshots exact."""
    monkeypatch.setenv("SPO_CPO_OBS512", "1")
    D, A, M = C.HUMANOID + (3037,)
    p, eng = _case_engine(D, A, M, dev)
    eng.mean_old.fill_(float("nan"))
    eng.snapshot_old_distribution()
    with torch.no_grad():
        m32 = C.oracle_policy(D, A, M).actor(p["data"]["obs"]).mean.double().numpy()
        m64 = C.oracle_policy(D, A, M, torch.float64).actor(p["data"]["obs"].double()).mean.numpy()
    hip = eng.mean_old.view(M, A).double().cpu().numpy()
    G.gate(hip, m32, m64, "means", norms=G.MAX)
    ls = p["state_dict"]["actor.log_std"] if "actor.log_std" in p["state_dict"] else eng.policy.actor.log_std.detach().cpu()
    assert torch.equal(eng.logstd_old.cpu(), ls.reshape(-1)) and torch.equal(eng.std_old, torch.exp(eng.logstd_old))


@pytest.mark.parametrize("ep_costs", [-1.0, 0.3])
def test_cpo512_actor_step_drift_envelope(dev, ep_costs, monkeypatch):
    """CPO's whole trust-region step (cpo.py:350-532) at 376 / 17, 4096 rows, with the three primitives on the streamed-W1
    kernels: tests/test_gpu_cpo_obs128.py::_actor_step_check's case, acceptance step, xHx, alpha, parameters under the fp64
    yardstick and the stale actor gradient."""
    monkeypatch.setenv("SPO_CPO_OBS512", "1")
    from safepo.single_agent import cpo
    made = []
    inner = cpo.make_engine
    monkeypatch.setattr(cpo, "make_engine", lambda *a, **k: made.append(inner(*a, **k)) or made[-1])
    _actor_step_check(dev, 376, 17, ep_costs, False)          # (False: `_actor_on_full_batch_kernels`, the 65-128 flag)
    assert len(made) == 1 and made[0]._actor_on_streamed_kernels is True


@pytest.mark.parametrize("ep_costs", [-1.0, 0.3])
def test_chunked_wide_path_unchanged_under_the_knob(dev, ep_costs, monkeypatch):
    """SPO_CPO_OBS512=0: the same step on the launch-per-layer wide kernels in row chunks, same gates."""
    monkeypatch.setenv("SPO_CPO_OBS512", "0")
    from safepo.single_agent import cpo
    made = []
    inner = cpo.make_engine
    monkeypatch.setattr(cpo, "make_engine", lambda *a, **k: made.append(inner(*a, **k)) or made[-1])
    _actor_step_check(dev, 376, 17, ep_costs, False)
    assert len(made) == 1 and made[0]._actor_on_streamed_kernels is False


@pytest.mark.parametrize("algo", ["cpo_humanoid", "pcpo_humanoid", "trpo_lag_humanoid"])
def test_reference_traces_at_humanoid_dims_run_on_the_new_kernels(dev, golden_dir, algo, monkeypatch):
    """tests/golden/{cpo,pcpo,trpo_lag}_trace_humanoid.npz (the reference's main() at 376 / 17) through
    test_second_order_family_traces_under_the_fp64_yardstick's own gates, with the engine asserted to be on the streamed-W1
    kernels, every primitive call counted and no call of the chunked path's kernels made."""
    import test_gpu_parity as P
    from safepo.single_agent import cpo
    monkeypatch.setenv("SPO_CPO_OBS512", "1")
    made, calls = [], {"surr": 0, "fvp": 0, "ls": 0, "mean": 0}
    inner = P._cpo_engine

    def engine(*a, **k):
        pol, eng = inner(*a, **k)
        assert type(eng) is cpo.WideCPOEngine and eng._actor_on_streamed_kernels is True
        lib = eng.lib

        class Counting:
            def __getattr__(self, name):
                fn = getattr(lib, name)
                key = {"spo_cpo512_surrogate_grad": "surr", "spo_cpo512_fvp": "fvp", "spo_cpo512_linesearch_eval": "ls",
                       "spo_cpo512_actor_mean": "mean"}.get(name)
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
    P.test_second_order_family_traces_under_the_fp64_yardstick(dev, golden_dir, algo)
    assert len(made) == 1
    assert calls["surr"] >= 2 and calls["fvp"] >= 10 and calls["ls"] >= 1 and calls["mean"] >= 1, calls
