"""GPU tests of the row-chunk full-batch CPO kernels (csrc/cpo_rows.hip, spo_cpo_rows_*): WideCPOEngine's three primitives and the
old-mean snapshot for hidden widths other than [64, 64], against the CPU oracle through the gates of
tests/test_gpu_cpo_obs128.py::test_cpo128_primitives_vs_oracle and ::_actor_step_check."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp64_gate as G  # noqa: E402
from oracle import restatement as R  # noqa: E402  (checker only)
from test_gpu_cpo_obs128 import _cpo_problem  # noqa: E402

# (obs_dim, act_dim, hidden); the first takes the two-chunks-per-workgroup row count as well
SHAPES = [(60, 8, [128, 128]), (7, 3, [20, 36]), (72, 2, [32, 32, 32]), (128, 16, [128, 128, 128]), (24, 1, [128, 16])]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rows(kind):
    from safepo import _abi
    lib = _abi.load()
    C, Gr = lib.spo_cpo_rows_chunk_rows(), lib.spo_cpo_rows_num_partials(1 << 30)
    return {"one": 1, "c-1": C - 1, "47c+29": 47 * C + 29, "gc+c+29": Gr * C + C + 29}[kind]


def _problem(D, A, hidden, M, dev, seed):
    """_cpo_problem for the old flag (False here), the new flag asserted to be what the envelope predicate says."""
    from safepo import _abi
    pol, ref, eng, data = _cpo_problem(D, A, hidden, 1, M, dev, seed=seed, expect_new_path=False)
    assert eng._actor_on_streamed_kernels is False
    assert eng._actor_on_row_group_kernels is bool(_abi.load().spo_cpo_rows_supported(eng.wide.net_a))
    return pol, ref, eng, data


@pytest.mark.parametrize("D,A,hidden,kind", [(D, A, h, k) for D, A, h in SHAPES for k in ("one", "c-1", "47c+29")]
                         + [SHAPES[0] + ("gc+c+29",)])
def test_cpo_rows_primitives_vs_oracle(dev, D, A, hidden, kind, monkeypatch):
    """Row counts from the chunk size C and the grid G: 1 and C - 1 (one partial chunk), 47 C + 29 (a ragged tail), and
    G C + C + 29: workgroups 0 and 1 walk a second chunk and workgroup 1's is the ragged tail -- the smallest case in which an
    accumulator that is reset, or counted twice, between chunks shows.  Shapes with three hidden layers lie outside the shipped
    envelope (the NL = 3 instantiation needs a scratch frame) and run the same gates on the chunked path."""
    monkeypatch.delenv("SPO_CPO_ROWS", raising=False)
    M = _rows(kind)
    pol, ref, eng, data = _problem(D, A, hidden, M, dev, seed=7 + D)
    assert eng._actor_on_row_group_kernels is (len(hidden) == 2)
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
    G.gate(hv, hv32, hv64, f"fvp ({D}, {A}, {hidden}, M {M})", norms=G.MAX)
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


def test_routing(dev, monkeypatch):
    """The flag is set exactly inside the envelope with the knob on; [64, 64] shapes keep their flags."""
    from safepo import _abi
    from safepo.common.model import ActorVCritic
    from safepo.single_agent import cpo

    def flags(D, A, hidden):
        c = dict(cpo.default_cfg)
        c["hidden_sizes"] = list(hidden)
        eng = cpo.make_engine(ActorVCritic(D, A, hidden_sizes=list(hidden)).to(dev), 2, 8, c, dev)
        if type(eng) is not cpo.WideCPOEngine:
            return None
        return eng._actor_on_row_group_kernels, eng._actor_on_full_batch_kernels, eng._actor_on_streamed_kernels

    monkeypatch.delenv("SPO_CPO_ROWS", raising=False)
    for D, A, h in SHAPES:
        assert flags(D, A, h) == (len(h) == 2, False, False), (D, A, h)
    assert flags(72, 2, [64, 64]) == (False, True, False)
    assert flags(376, 17, [64, 64]) == (False, False, True)
    assert flags(60, 8, [64, 64]) is None                        # CPOEngine, as before
    for D, A, h in ((60, 8, [256, 256]), (376, 17, [128, 128]), (60, 17, [128, 128])):
        assert flags(D, A, h) == (False, False, False), (D, A, h)
    monkeypatch.setenv("SPO_CPO_ROWS", "0")
    assert flags(60, 8, [128, 128]) == (False, False, False)
    assert flags(72, 2, [64, 64]) == (False, True, False)
    monkeypatch.setenv("SPO_CPO_ROWS", "1")
    assert flags(60, 8, [128, 128]) == (True, False, False)
    # every entry point refuses an out-of-range net, naming the dimension
    lib, p = _abi.load(), _abi.ptr
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dev)
    t, d3 = z(64), z(3, dt=torch.float64)
    for sizes, word in (([129, 128, 128, 2], "obs_dim"), ([60, 128, 129, 2], "hidden width"), ([60, 128, 128, 17], "act_dim")):
        net = _abi.MlpNet.of(sizes)
        for name, call in (("surrogate_grad", lambda: lib.spo_cpo_rows_surrogate_grad(p(t), p(t), p(t), p(t), p(t), 1.0, 1, net, p(t), p(d3), p(t), p(d3), _abi.stream_ptr())),
                           ("fvp", lambda: lib.spo_cpo_rows_fvp(p(t), p(t), p(t), 1, net, p(t), p(d3), p(t), _abi.stream_ptr())),
                           ("linesearch_eval", lambda: lib.spo_cpo_rows_linesearch_eval(p(t), p(t), p(t), p(t), p(t), p(t), p(t), p(t), 1, net, p(d3), 3, p(d3), _abi.stream_ptr())),
                           ("actor_mean", lambda: lib.spo_cpo_rows_actor_mean(p(t), p(t), p(t), 1, net, _abi.stream_ptr()))):
            with pytest.raises(_abi.SpoError, match=word):
                _abi.check(call(), "spo_cpo_rows_" + name)


@pytest.mark.parametrize("knob", ["1", "0"])
@pytest.mark.parametrize("ep_costs", [-1.0, 0.3])
def test_cpo_rows_actor_step_drift_envelope(dev, ep_costs, knob, monkeypatch):
    """CPO's whole trust-region step (cpo.py:350-532) at 60 / 8 [128, 128], 4096 rows, through the gates of
    tests/test_gpu_cpo_obs128.py::_actor_step_check; knob 0: the chunked path still passes the same gates."""
    monkeypatch.setenv("SPO_CPO_ROWS", knob)
    D, A, M = 60, 8, 4096
    pol, ref32, eng, data32 = _cpo_problem(D, A, [128, 128], 1, M, dev, seed=14, expect_new_path=False)
    assert eng._actor_on_row_group_kernels is (knob == "1")
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
