"""GPU tests of the row-split update kernel's two-batch layer-1 hand-off (csrc/update_rs.hip, template flag L1P, SPO_RS_L1_PIPE)
and of its unclipped fast path for the joint clip.  Neither changes per-element arithmetic or a summation order, so the reference
is the one-batch form on the same machine (SPO_RS_L1_PIPE=0, read at every launch) and the comparison is bit for bit; one case pins
the knob to 1 against the float32 oracle.  No test provokes a timeout of the exchange."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import restatement as R  # noqa: E402  (checker only)
from test_gpu_parity import _synthetic_update_problem, _fill_update_problem  # noqa: E402

CFG = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "learning_iters": 1}
# The value targets and advantages of _synthetic_update_problem times this, per shape: as they come the joint gradient norm sits
# above 1.2 on (nearly) every step of these launches and the unclipped path would go uncompared.  Float32 oracle, the three
# launches of a case, steps above the bound 1.2 / steps: 18 / 114 at 60 / 8 / 64 (scale 0.7), 10 / 66 at 60 / 8 / 50, 21 / 33 at
# 64 / 16 / 33, 15 / 33 at 20 / 3 / 64, 6 / 30 at 12 / 2 / 64 (scale 0.6); no step within 1.7e-3 (relative) of the bound.
CASES = [  # obs, act, batch, M, max_grad_norm, target scale
    (60, 8, 64, 64 * 37 + 19, 1.2, 0.7),      # NT1 = 4; ragged last minibatch; clip on part of the steps
    (60, 8, 64, 64 * 37 + 19, 40.0, 0.7),     # ... and never
    (60, 8, 50, 50 * 21 + 7, 1.2, 0.6),       # fewer than 32 valid rows in the second row group's tile
    (64, 16, 33, 33 * 11, 1.2, 0.6),          # the second row group holds one row; full KIN and act width
    (20, 3, 64, 64 * 10 + 1, 1.2, 0.6),       # KIN = 32, NT1 = 2: one tile per batch
    (12, 2, 64, 64 * 10, 1.2, 0.6),           # KIN = 16: the knob must change nothing
]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_routing(monkeypatch):
    for k in ("SPO_RS_OBS128", "SPO_RS_SAFE", "SPO_RS_L1_PIPE", "SPO_FORCE_DP"):
        monkeypatch.delenv(k, raising=False)
    assert int(os.environ.get("SPO_UPDATE_FORM", "3")) >= 3, "SPO_UPDATE_FORM selects an older form in this process: unset it"
    assert os.environ.get("SPO_RS_ROWS", "32") != "16", "SPO_RS_ROWS=16 selects the four-row-group form in this process: unset it"


def _counters(lib, reset=1):
    from safepo import _abi
    c4 = (ctypes.c_ulonglong * 4)()
    _abi.check(lib.spo_debug_update_counters(c4, reset), "counters")
    return [int(x) for x in c4]


def _engine(D, A, batch, M, mg, scale, dev, init_seed=4, problem_seed=31):
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    torch.manual_seed(init_seed)
    pol = ActorVCritic(D, A).to(dev)
    eng = PPOLagEngine(pol, 1, M, dict(CFG, batch_size=batch, max_grad_norm=mg), dev)
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=problem_seed)
    problem = (obs, act, logp, scale * tgt_r, scale * tgt_c, scale * adv)
    _fill_update_problem(eng, problem)
    return eng, problem


def _state(eng):
    return eng.policy.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone()


# ------------------------------------------------------------------------------------------------ 1. same bits as the one-batch form
@pytest.mark.parametrize("D,A,batch,M,mg,scale", CASES, ids=lambda v: str(v))
def test_two_batch_handoff_gives_the_bits_of_the_one_batch_form(dev, monkeypatch, D, A, batch, M, mg, scale):
    from safepo import _abi
    lib = _abi.load()
    assert lib.spo_update_rs_supported(D, A, batch, 3) == 1
    nst = (M + batch - 1) // batch
    g = torch.Generator().manual_seed(9)
    perms = [torch.randperm(M, generator=g).to(torch.int32).to(dev) for _ in range(3)]
    outs, counts = {}, {}
    for pipe in ("0", "1"):
        for safe in ("0", "1"):
            monkeypatch.setenv("SPO_RS_L1_PIPE", pipe)
            monkeypatch.setenv("SPO_RS_SAFE", safe)
            eng, _ = _engine(D, A, batch, M, mg, scale, dev)
            _counters(lib)
            losses = [eng.learning_iter(p).clone() for p in perms]       # three consecutive launches on one stream
            eng.check_sync_error()
            counts[pipe, safe] = _counters(lib)[:2]
            outs[pipe, safe] = _state(eng) + (torch.stack(losses),)
    print(f"{D}/{A}/{batch}, max_grad_norm {mg}: [steps, redone] per (pipe, safe) {counts}")
    ref = outs["0", "0"]
    assert all(torch.isfinite(t).all() for t in ref)
    for key, got in outs.items():
        for name, x, y in zip(("theta", "adam_m", "adam_v", "losses"), got, ref):
            assert torch.equal(x, y), f"(pipe, safe) = {key}: {name} differs in {int((x != y).sum())} of {x.numel()} entries"
    for key, c in counts.items():
        assert c[0] == 3 * nst, (key, c, nst)
        assert c == counts["0", "0"], (key, c, counts["0", "0"])        # the same steps, the same steps redone
    if mg == 1.2:
        assert 0 < counts["1", "0"][1] < 3 * nst, counts                 # the restore-and-redo path ran in the new form
    else:
        assert counts["1", "0"][1] == 0, counts


# ------------------------------------------------------------------------------------------------ 2. the two-network launch
@pytest.mark.parametrize("D", [60, 20])
def test_critic_fit_two_networks_same_bits(dev, monkeypatch, D):
    """The critic fit at batch 64 (two row groups, two networks) through the engine that calls spo_critic_fit_iter, the stale actor
    gradient (norm 50) going into the joint clip (40) as in test_row_split_critic_fit_shapes_vs_oracle: the clip is active."""
    from safepo.single_agent.cpo import CPOEngine, default_cfg
    from safepo.common.model import ActorVCritic
    monkeypatch.setenv("SPO_CPO_SPLIT", "0")
    A, batch, M = 4, 64, 64 * 9 + 13
    obs, _a, _l, tgt_r, tgt_c, _adv = _synthetic_update_problem(M, D, A, seed=M + D)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(2)).to(torch.int32).to(dev)
    nst = (M + batch - 1) // batch
    outs = {}
    for pipe in ("0", "1"):
        monkeypatch.setenv("SPO_RS_L1_PIPE", pipe)
        torch.manual_seed(M + 1)
        pol = ActorVCritic(D, A).to(dev)
        cfg = dict(default_cfg)
        cfg.update(learning_iters=2, batch_size=batch)
        eng = CPOEngine(pol, 1, M, cfg, dev)
        assert eng.lib.spo_update_rs_supported(D, A, batch, 2) == 1
        bd = eng.buffer.data
        bd["obs"].copy_(obs.view(1, M, D)); bd["target_value_r"].copy_(tgt_r.view(1, M)); bd["target_value_c"].copy_(tgt_c.view(1, M))
        eng.stale_sq.fill_(2500.0)
        _counters(eng.lib)
        fit = eng.critic_fit(perm_fn=lambda it: perm)
        eng.check_sync_error()
        c = _counters(eng.lib)
        assert eng._split in (None, False)
        assert c[0] == 2 * nst and 0 < c[1] <= 2 * nst, (c, nst)           # the row-split kernel ran it, with the clip active
        outs[pipe] = _state(eng) + (torch.cat(fit["losses"], 0).clone(), eng.stale_sq.clone(), torch.tensor(c[:2]))
    assert 0.0 < float(outs["0"][4].item()) < 2500.0                       # the stale norm went in and came out rescaled
    for name, x, y in zip(("theta", "adam_m", "adam_v", "losses", "stale_sq", "counters"), outs["1"], outs["0"]):
        assert torch.equal(x, y), f"{name} differs in {int((x != y).sum())} of {x.numel()} entries"
    assert all(torch.isfinite(t).all() for t in outs["0"][:5])


# ------------------------------------------------------------------------------------------------ 3. the seed-batched launch
def test_seed_batched_launch_follows_the_knob(dev, monkeypatch):
    """Three runs with their own parameters, buffers and max_grad_norm: ONE batched launch with the two-batch hand-off equals
    three stand-alone launches of the one-batch form."""
    from safepo import _abi
    from safepo.common.engine_group import PPOLagEngineGroup
    lib = _abi.load()
    D, A, batch, M = 60, 8, 64, 64 * 9 + 5
    norms = (1.2, 40.0, 1.2)

    def build():
        es, perms = [], []
        for r, mg in enumerate(norms):
            eng, _ = _engine(D, A, batch, M, mg, 0.7, dev, init_seed=100 + r, problem_seed=1000 + r)
            es.append(eng)
            perms.append(torch.randperm(M, generator=torch.Generator().manual_seed(50 + r)).to(torch.int32).to(dev))
        return es, perms

    monkeypatch.setenv("SPO_RS_L1_PIPE", "0")
    es, perms = build()
    want = []
    for e, p in zip(es, perms):
        losses = e.learning_iter(p).clone()
        e.check_sync_error()
        want.append(_state(e) + (losses,))
    monkeypatch.setenv("SPO_RS_L1_PIPE", "1")
    es, perms = build()
    group = PPOLagEngineGroup(es)
    assert group.batched()
    c2 = (ctypes.c_ulonglong * 2)()
    _abi.check(lib.spo_debug_rs_multi_counters(c2, 1), "multi counters")
    losses = group.learning_iter_all(perms)
    group.check_sync_error()
    _abi.check(lib.spo_debug_rs_multi_counters(c2, 1), "multi counters")
    assert int(c2[0]) == 3, list(c2)                                       # one launch of three runs
    for r, e in enumerate(es):
        for name, x, y in zip(("theta", "adam_m", "adam_v", "losses"), _state(e) + (losses[r],), want[r]):
            assert torch.equal(x, y), f"run {r}: {name} differs in {int((x != y).sum())} of {x.numel()} entries"


# ------------------------------------------------------------------------------------------------ 4. the new form against the oracle
def test_two_batch_handoff_vs_oracle(dev, monkeypatch):
    """SPO_RS_L1_PIPE=1 pinned: the first 8 steps at 60 / 8 with the clip (1.2) active on part of them, against the float32 oracle
    at the 1e-5 bar the drift-envelope gate sets for the first 8 steps; the parameters after them under the float64 yardstick
    (Adam divides by sqrt(v): elements with rounding-level gradients have no element-wise 1e-5 bar, tests/envelope.py)."""
    import envelope as E
    from safepo import _abi
    monkeypatch.setenv("SPO_RS_L1_PIPE", "1")
    D, A, batch, M, mg = 60, 8, 64, 64 * 12 + 7, 1.2
    eng, (obs, act, logp, tgt_r, tgt_c, adv) = _engine(D, A, batch, M, mg, 0.7, dev)
    ref = R.OraclePolicy(D, A)
    sd0 = {k: v.cpu().clone() for k, v in eng.policy.state_dict().items()}
    ref.load_state_dict(sd0)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(3))
    upd = R.PPOLagUpdater(ref, epochs=1, max_grad_norm=mg)
    losses_ref, norms = [], []
    for s in range(0, 8 * batch, batch):
        ii = perm[s:s + batch]
        rec = {}
        losses_ref.append(upd.minibatch_step(obs[ii], act[ii], logp[ii], tgt_r[ii], tgt_c[ii], adv[ii], record=rec))
        norms.append(float(rec["grad_preclip"].double().norm()))
    print("joint norms of the first 8 steps (oracle):", np.round(norms, 4))
    assert np.abs(np.asarray(norms) / mg - 1).min() > 1e-4                 # no step sits on the bound
    lib = _abi.load()
    _counters(lib)
    eng.M = 8 * batch
    losses = eng.learning_iter(perm[:8 * batch].to(torch.int32).to(dev).contiguous())
    eng.check_sync_error()
    c = _counters(lib)
    assert c[0] == 8 and c[1] == int((np.asarray(norms) > mg).sum()), (c, norms)
    np.testing.assert_allclose(losses.cpu().numpy(), np.asarray(losses_ref), rtol=1e-5, atol=1e-6)
    _, t64 = E.oracle_trajectory(sd0, (obs, act, logp, tgt_r, tgt_c, adv), perm, batch, 8, torch.float64, [8], max_grad_norm=mg)
    E.assert_theta_envelope(eng.policy.theta.cpu().numpy(), R.flat_params(ref).numpy(), t64[8], "two-batch hand-off: theta after 8 steps")
