"""GPU tests of the row-split update kernel's KIN = 128 form (csrc/update_rs.hip; spo_update_rs128_supported): observations of
65 .. 128 values -- the Car / Racecar / Doggo / Ant navigation tasks of the reference's default sweep -- with the default [64, 64]
networks.  spo_ppo_lag_update_iter (three networks, two row groups) runs on it by default; SPO_RS_OBS128=0 restores the four-wave
kernel.  (The critic fit's form -- two critics, four row groups -- was measured slower than the split form it would replace and
is not built: its tests are not here.)  Everything is gated against the CPU oracle
(oracle/restatement.py) with the project's existing gates: the first steps at rtol 1e-5 / atol 1e-6 against the float32 oracle,
the pass under the float64 drift envelope (tests/envelope.py) with its default factor, no floors beyond its own and no exempted
directions.  No test provokes a timeout of the exchange."""
import ctypes
import faulthandler
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import restatement as R  # noqa: E402  (checker only)
import envelope as E  # noqa: E402
from test_gpu_parity import (_synthetic_update_problem, _fill_update_problem,  # noqa: E402
                             _assert_trajectory_in_envelope, _hip_prefix_runs)

TIME_LIMIT_S = 420          # per test; the full-size test runs 8 192 oracle steps in float32 and in float64 on the CPU
CFG = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "learning_iters": 1}


@pytest.fixture(autouse=True)
def _time_limit_and_global_state():
    """Every test under its own time limit (a watchdog thread that ends the process: it also fires while the main thread waits
    inside a HIP call); torch's CPU thread count and generator state are put back for the test files that run later."""
    threads, rng = torch.get_num_threads(), torch.get_rng_state()
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()
    torch.set_num_threads(threads)
    torch.set_rng_state(rng)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_routing(monkeypatch):
    for k in ("SPO_RS_OBS128", "SPO_RS_SAFE", "SPO_CPO_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    # (read once per process by the library: cannot be undone from here, and these tests are about the default form)
    assert int(os.environ.get("SPO_UPDATE_FORM", "3")) >= 3, "SPO_UPDATE_FORM selects an older form in this process: unset it"


def _counters(lib, reset=1):
    from safepo import _abi
    c4 = (ctypes.c_ulonglong * 4)()
    _abi.check(lib.spo_debug_update_counters(c4, reset), "counters")
    return [int(x) for x in c4]


def _ppo_engine(D, A, M, batch, max_grad_norm, dev, seed, log_std=False):
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    torch.manual_seed(seed)
    pol = ActorVCritic(D, A).to(dev)
    if log_std:
        with torch.no_grad():
            pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    eng = PPOLagEngine(pol, 1, M, dict(CFG, batch_size=batch, max_grad_norm=max_grad_norm), dev)
    return pol, eng


@pytest.mark.parametrize("D,A", [(72, 2), (128, 16)])
def test_row_split_kernel_is_the_default_at_obs_65_to_128_and_exchange_modes_agree(dev, monkeypatch, D, A):
    """spo_ppo_lag_update_iter runs the row-split kernel where spo_update_rs128_supported: the debug counters see 3 x ceil(M / 64)
    steps of it (0 on the four-wave kernel), the clip active on part of them (the second counter: at KIN = 128 layer 1's Adam
    runs behind the joint norm, so nothing is redone and that counter counts the clipped steps).  Plain and write-through
    exchange stores (SPO_RS_SAFE) give the same bits over three consecutive launches.  With SPO_RS_OBS128=0 the counters stay 0 and the four-wave kernel's first steps agree with the default run's at the first-steps
    tolerance."""
    from safepo import _abi
    lib = _abi.load()
    assert lib.spo_update_rs128_supported(D, A, 64, 3) == 1 and lib.spo_update_rs_supported(D, A, 64, 3) == 0
    M, batch = 64 * 37 + 19, 64
    nst = (M + batch - 1) // batch
    problem = _synthetic_update_problem(M, D, A, seed=31)
    g = torch.Generator().manual_seed(9)
    perms = [torch.randperm(M, generator=g).to(torch.int32).to(dev) for _ in range(3)]
    outs = {}
    for mode in ("fast", "safe"):
        monkeypatch.setenv("SPO_RS_SAFE", "1" if mode == "safe" else "0")
        pol, eng = _ppo_engine(D, A, M, batch, 1.2, dev, seed=4)
        _fill_update_problem(eng, problem)
        _counters(lib)
        losses = [eng.learning_iter(p).clone() for p in perms]
        eng.check_sync_error()
        c4 = _counters(lib)
        assert c4[0] == 3 * nst, (c4, nst)
        assert 0 < c4[1] < 3 * nst, c4                      # clipped on part of the steps
        outs[mode] = (pol.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), torch.stack(losses))
    for x, y in zip(outs["fast"], outs["safe"]):
        assert torch.equal(x, y)
    assert torch.isfinite(outs["fast"][0]).all() and torch.isfinite(outs["fast"][3]).all()
    monkeypatch.delenv("SPO_RS_SAFE")
    # the knob: four steps on either kernel from the same state
    first = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("SPO_RS_OBS128", knob)
        pol, eng = _ppo_engine(D, A, 4 * batch, batch, 1.2, dev, seed=4)
        _fill_update_problem(eng, tuple(t[:4 * batch] for t in problem))
        _counters(lib)
        l4 = eng.learning_iter(torch.arange(4 * batch, dtype=torch.int32, device=dev)).clone()
        eng.check_sync_error()
        c4 = _counters(lib)
        assert c4[0] == (4 if knob == "1" else 0), (knob, c4)
        first[knob] = (pol.theta.cpu().numpy(), l4.cpu().numpy())
    np.testing.assert_allclose(first["0"][1], first["1"][1], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(first["0"][0], first["1"][0], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("D,A", [(72, 2), (104, 12)])
def test_clip_on_part_of_the_steps_vs_oracle(dev, D, A):
    """clip_grad_norm_ active on SOME steps (bound = between the two middle joint norms of the unclipped float32 oracle): at
    KIN = 128 layer 1's Adam waits for the joint norm and takes the coefficient, layers 2 / 3 as up to 64.  Losses and parameters
    against the oracle; the counters see clipped and unclipped steps, as many of each as the oracle."""
    from safepo import _abi
    lib = _abi.load()
    M, batch = 64 * 20 + 7, 64
    nst = (M + batch - 1) // batch
    problem = _synthetic_update_problem(M, D, A, seed=5)
    obs, act, logp, tgt_r, tgt_c, adv = problem
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(3))
    pol, eng = _ppo_engine(D, A, M, batch, 40.0, dev, seed=11)
    sd0 = {k: v.detach().cpu().clone() for k, v in pol.state_dict().items()}

    def oracle_norms(bound):
        ref = R.OraclePolicy(D, A)
        ref.load_state_dict({k: v.clone() for k, v in sd0.items()})
        upd = R.PPOLagUpdater(ref, epochs=1, max_grad_norm=bound)
        norms = []
        for s in range(0, M, batch):
            ii = perm[s:s + batch]
            rec = {}
            upd.minibatch_step(obs[ii], act[ii], logp[ii], tgt_r[ii], tgt_c[ii], adv[ii], record=rec)
            norms.append(float(rec["grad_preclip"].double().norm()))
        return np.asarray(norms)

    free = np.sort(oracle_norms(1e9))
    bound = float(0.5 * (free[nst // 2 - 1] + free[nst // 2]))          # between two norms: no step of the free run sits on it
    norms = oracle_norms(bound)
    clipped = norms > bound
    assert 0.1 * nst <= clipped.sum() <= 0.9 * nst, (clipped, bound)
    assert np.abs(norms / bound - 1).min() > 1e-4           # no step sits on the bound (the decision is not a rounding matter)
    pol, eng = _ppo_engine(D, A, M, batch, bound, dev, seed=11)
    assert all(torch.equal(v.detach().cpu(), sd0[k]) for k, v in pol.state_dict().items())
    _fill_update_problem(eng, problem)
    _counters(lib)
    losses = eng.learning_iter(perm.to(torch.int32).to(dev))
    eng.check_sync_error()
    c4 = _counters(lib)
    assert c4[0] == nst and 0 < c4[1] < nst, (c4, nst, int(clipped.sum()))
    assert c4[1] == int(clipped.sum()), (c4, int(clipped.sum()))
    l32, t32 = E.oracle_trajectory(sd0, problem, perm, batch, nst, torch.float32, [nst], max_grad_norm=bound)
    l64, t64 = E.oracle_trajectory(sd0, problem, perm, batch, nst, torch.float64, [nst], max_grad_norm=bound)
    lh = losses.double().cpu().numpy()
    np.testing.assert_allclose(lh[:4], l32[:4], rtol=1e-5, atol=1e-6)
    print("clip on part of the steps", D, A, "clipped", int(clipped.sum()), "of", nst, "redone", c4[1],
          "loss ratio", E.loss_envelope(lh, l32, l64, window=nst)[0], "theta ratio", E.theta_envelope(pol.theta.cpu().numpy(), t32[nst], t64[nst])[0])
    E.assert_loss_envelope(lh, l32, l64, f"clip on part of the steps {D}/{A}: losses", window=nst)
    E.assert_theta_envelope(pol.theta.cpu().numpy(), t32[nst], t64[nst], f"clip on part of the steps {D}/{A}: theta")


@pytest.mark.parametrize("batch", [64, 30, 1])
@pytest.mark.parametrize("D,A", [(65, 1), (72, 2), (97, 6), (104, 12), (128, 16)])
def test_step_parity_vs_oracle(dev, D, A, batch):
    """Ragged and partial minibatches (a second row group without rows at batch <= 32), every tile count of the padded input
    layer: the pre-clip gradient of the first minibatch (read off the first Adam moment of a one-step launch without clip:
    m = (1 - beta1) g) at 1e-5 of its scale, the first steps' losses at rtol 1e-5 / atol 1e-6 against the float32 oracle, losses
    and parameters after the pass under the float64 envelope."""
    from safepo import _abi
    lib = _abi.load()
    M = {64: 64 * 5 + 21, 30: 30 * 5 + 11, 1: 7}[batch]
    nst = (M + batch - 1) // batch
    problem = _synthetic_update_problem(M, D, A, seed=M + D)
    obs, act, logp, tgt_r, tgt_c, adv = problem
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(3))
    # --- one step without clip: the gradient
    pol, eng = _ppo_engine(D, A, batch, batch, 1e9, dev, seed=M + D, log_std=True)
    sd0 = {k: v.detach().cpu().clone() for k, v in pol.state_dict().items()}
    _fill_update_problem(eng, tuple(t[perm[:batch]] for t in problem))
    _counters(lib)
    eng.learning_iter(torch.arange(batch, dtype=torch.int32, device=dev))
    eng.check_sync_error()
    assert _counters(lib)[0] == 1
    ref = R.OraclePolicy(D, A)
    ref.load_state_dict({k: v.clone() for k, v in sd0.items()})
    rec = {}
    ii = perm[:batch]
    R.PPOLagUpdater(ref, epochs=1, max_grad_norm=1e9).minibatch_step(obs[ii], act[ii], logp[ii], tgt_r[ii], tgt_c[ii], adv[ii], record=rec)
    g_ref = rec["grad_preclip"].numpy()
    g_got = eng.adam_m.cpu().numpy().astype(np.float64) / (1.0 - 0.9)
    assert g_got.shape == g_ref.shape
    assert np.abs(g_got - g_ref).max() <= 1e-5 * np.abs(g_ref).max(), (np.abs(g_got - g_ref).max(), np.abs(g_ref).max())
    # --- the pass
    pol, eng = _ppo_engine(D, A, M, batch, 40.0, dev, seed=M + D, log_std=True)
    assert all(torch.equal(v.detach().cpu(), sd0[k]) for k, v in pol.state_dict().items())
    _fill_update_problem(eng, problem)
    losses = eng.learning_iter(perm.to(torch.int32).to(dev))
    eng.check_sync_error()
    assert _counters(lib)[0] == nst
    l32, t32 = E.oracle_trajectory(sd0, problem, perm, batch, nst, torch.float32, [nst])
    l64, t64 = E.oracle_trajectory(sd0, problem, perm, batch, nst, torch.float64, [nst])
    lh = losses.double().cpu().numpy()
    assert lh.shape == (nst, 3)
    np.testing.assert_allclose(lh[:4], l32[:4], rtol=1e-5, atol=1e-6)
    E.assert_loss_envelope(lh, l32, l64, f"step parity {D}/{A}/{batch}: losses", window=nst)
    E.assert_theta_envelope(pol.theta.cpu().numpy(), t32[nst], t64[nst], f"step parity {D}/{A}/{batch}: theta")


def test_full_size_learning_iteration_drift_envelope_104_12(dev):
    """One learning iteration at the benchmark's size -- 8 192 minibatch steps of 64 rows over 4096 x 128 rows in ONE launch -- at
    104 / 12 under the drift envelope of test_full_size_update_parity_drift_envelope: first 8 steps at 1e-5, every 64-step window
    of the losses and the parameters after 8 / 64 / 512 / 8 192 steps no further from the float64 trajectory than 3 x the float32
    oracle is."""
    from safepo import _abi
    lib = _abi.load()
    N, T, D, A = 4096, 128, 104, 12
    M = N * T
    torch.set_num_threads(8)
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    torch.manual_seed(11)
    pol = ActorVCritic(D, A).to(dev)
    problem = _synthetic_update_problem(M, D, A, seed=2024)
    eng = PPOLagEngine(pol, N, T, dict(CFG, batch_size=64, max_grad_norm=40.0), dev)
    _fill_update_problem(eng, problem)
    sd0 = {k: v.detach().cpu().clone() for k, v in pol.state_dict().items()}
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(6))
    ks = (8, 64, 512, 8192)
    _counters(lib)
    runs = _hip_prefix_runs(eng, pol, pol.theta.clone(), perm.to(torch.int32).to(dev), 64, ks)
    assert _counters(lib)[0] == sum(ks)
    rep = _assert_trajectory_in_envelope(runs, problem, sd0, perm, 64, ks, "full-size learning iteration at 104 / 12")
    print("drift envelope at 104 / 12 (ratio <= 1 passes):", rep)


def test_critic_fit_at_these_dims_stays_on_the_previous_routing(dev, monkeypatch):
    """The four-row-group critic fit at KIN = 128 was measured slower than the split form and is not built
    (spo_update_rs128_supported(..., 2) == 0): WideCPOEngine.critic_fit at 72 / 2 keeps its routing -- no row-split steps."""
    from safepo import _abi
    from safepo.single_agent import cpo
    from safepo.common.model import ActorVCritic
    lib = _abi.load()
    D, A, N, T, batch = 72, 2, 8, 128, 128
    assert lib.spo_update_rs128_supported(D, A, batch, 2) == 0
    obs, _a, _l, tgt_r, tgt_c, _adv = _synthetic_update_problem(N * T, D, A, seed=8)
    torch.manual_seed(3)
    pol = ActorVCritic(D, A).to(dev)
    cfg = dict(cpo.default_cfg)
    cfg.update(learning_iters=1, batch_size=batch)
    eng = cpo.make_engine(pol, N, T, cfg, dev)
    assert type(eng) is cpo.WideCPOEngine and eng._critics_on_persistent_kernel
    bd = eng.buffer.data
    bd["obs"].copy_(obs.view(N, T, D)); bd["target_value_r"].copy_(tgt_r.view(N, T)); bd["target_value_c"].copy_(tgt_c.view(N, T))
    _counters(lib)
    fit = eng.critic_fit()
    assert _counters(lib)[0] == 0
    assert torch.isfinite(torch.cat(fit["losses"], 0)).all()


def test_the_knob_does_not_reach_observations_up_to_64(dev, monkeypatch):
    """One launch at 60 / 8 gives identical bits with SPO_RS_OBS128 0 and 1, on the row-split kernel both times."""
    from safepo import _abi
    lib = _abi.load()
    D, A, M, batch = 60, 8, 64 * 12 + 5, 64
    problem = _synthetic_update_problem(M, D, A, seed=77)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(1)).to(torch.int32).to(dev)
    outs = []
    for knob in ("0", "1"):
        monkeypatch.setenv("SPO_RS_OBS128", knob)
        pol, eng = _ppo_engine(D, A, M, batch, 1.2, dev, seed=6)
        _fill_update_problem(eng, problem)
        _counters(lib)
        losses = eng.learning_iter(perm).clone()
        eng.check_sync_error()
        assert _counters(lib)[0] == (M + batch - 1) // batch
        outs.append((pol.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), losses))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
