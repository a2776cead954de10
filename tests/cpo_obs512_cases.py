"""The cases of tests/test_gpu_cpo_obs512.py (no test in here): shapes and row counts of the streamed-W1 full-batch CPO kernels
(spo_cpo512_* of csrc/cpo.hip: 129 <= obs_dim <= 512, act_dim <= 32), the problem of each case built on the CPU exactly as
tests/test_gpu_cpo_obs128.py::_cpo_problem builds it (test_gpu_parity._wide_pair's parameters, _synthetic_update_problem's batch),
and what the three primitives return for it by the oracle (oracle/restatement.py, autograd, torch.distributions) in float32 -- the
yardstick -- and in float64 -- the reference.  tests/test_cpo_obs512_host.py checks on the CPU that the gates of the GPU test say
something at these cases.

Every oracle result is computed once per process (functools.lru_cache) and shared; callers do not modify what they get.  The
oracles run on a stated number of torch threads (blocked sums round differently with the thread count) and put the count back."""
import copy
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "safe-policy-optimization_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fp64_gate as G  # noqa: E402
from fp64_gate import ORACLE_THREADS  # noqa: E402  (the float32 yardstick and the float64 reference of the GPU test)
from oracle import restatement as R  # noqa: E402
from test_gpu_parity import _synthetic_update_problem  # noqa: E402  (its tests carry the gpu marker; the builder needs no GPU)

# (129, 1): the third slice holds one feature; (192, 16): whole slices, one full output tile; (376, 17): HumanoidVelocity -- a
# ragged 56-feature slice, a ragged 16-tile, one action in the second output tile; (512, 32): the largest
SHAPES = [(129, 1), (192, 16), (376, 17), (512, 32)]
HUMANOID = (376, 17)
ROWS = [3037, 1, 63]                          # 47 chunks + a 29-row tail over 48 workgroups; single partial chunks
ROWS_CROSS_CHUNK = 256 * 64 + 64 + 29         # 16 477: workgroups 0 and 1 walk two chunks, workgroup 1's second one is the tail
ROWS_THREE_CHUNKS = 3 * 256 * 64 + 5          # 49 157: every workgroup accumulates over three chunks, workgroup 0 a fourth of 5 rows
#                                               (surrogate gradient and Fisher-vector product only)
CASES = [(D, A, M) for D, A in SHAPES for M in ROWS] + [HUMANOID + (ROWS_CROSS_CHUNK,), HUMANOID + (ROWS_THREE_CHUNKS,)]
MOVE = 0.02                                   # line search: theta_actor += MOVE * randn (test_cpo128_primitives_vs_oracle)


def seed_of(D):
    return 7 + D                              # test_cpo128_primitives_vs_oracle's


def line_search_checked(M):
    return M != ROWS_THREE_CHUNKS


@functools.lru_cache(maxsize=None)
def problem(D, A, M):
    """state_dict of the policy, the float32 batch and the two directions of case (D, A, M), all on the CPU; torch's generator
    is left as found.  Same draws as _cpo_problem(D, A, [64, 64], 1, M, dev, seed_of(D)) of tests/test_gpu_cpo_obs128.py."""
    from safepo.common.model import ActorVCritic
    rng = torch.get_rng_state()
    torch.manual_seed(seed_of(D))
    pol = ActorVCritic(D, A, hidden_sizes=[64, 64])
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    torch.set_rng_state(rng)
    sd = {k: v.detach().clone() for k, v in pol.state_dict().items()}
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=seed_of(D) + 1)
    adv_c = adv.flip(0) * 0.5 + 0.1
    Pa = A + 64 * D + 64 + 64 * 64 + 64 + A * 64 + A
    return {"state_dict": sd, "Pa": Pa,
            "v": torch.randn(Pa, generator=torch.Generator().manual_seed(3)),
            "delta": MOVE * torch.randn(Pa, generator=torch.Generator().manual_seed(5)),
            "data": {"obs": obs, "act": act, "log_prob": logp, "adv_r": adv, "adv_c": adv_c,
                     "target_value_r": tgt_r, "target_value_c": tgt_c}}


def oracle_policy(D, A, M, dtype=torch.float32):
    p = problem(D, A, M)
    ref = R.OraclePolicy(D, A, hidden_sizes=(64, 64))
    assert list(ref.state_dict()) == list(p["state_dict"])
    ref.load_state_dict({k: v.clone() for k, v in p["state_dict"].items()})
    return ref.to(dtype)


@functools.lru_cache(maxsize=None)
def oracle(D, A, M, dtype_name, threads=ORACLE_THREADS):
    """What CPOEngine's three primitives return for case (D, A, M), by the oracle in `dtype_name` on `threads` torch threads:
    float64 numpy vectors and python floats."""
    dtype = getattr(torch, dtype_name)
    with G.on_oracle_threads(threads):
        p = problem(D, A, M)
        ref = oracle_policy(D, A, M, dtype)
        data = {k: v.to(dtype) for k, v in p["data"].items()}
        assert R.actor_flat_params(ref.actor).numel() == p["Pa"]
        out = {"floor": 1e-6 * float(p["data"]["adv_r"].abs().mean())}
        for which in ("r", "c"):
            ref.actor.zero_grad()
            loss = R.cpo_surrogate(ref, data, which)
            loss.backward()
            out["grad_" + which] = R.actor_flat_grads(ref.actor).double().numpy().copy()
            out["loss_" + which] = float(loss.detach())
        out["Fv"] = R.cpo_fvp(p["v"].to(dtype), ref, data["obs"]).detach().double().numpy().copy()
        if line_search_checked(M):
            with torch.no_grad():
                old = ref.actor(data["obs"])
                old_mean, old_std = old.mean.clone(), old.stddev.clone()
                R.actor_set_flat_params(ref.actor, R.actor_flat_params(ref.actor) + p["delta"].to(dtype))
                out["moved_kl"] = float(torch.distributions.kl_divergence(torch.distributions.Normal(old_mean, old_std),
                                                                          ref.actor(data["obs"])).mean())
                out["moved_loss_r"] = float(R.cpo_surrogate(ref, data, "r"))
                out["moved_loss_c"] = float(R.cpo_surrogate(ref, data, "c"))
        return out


def gate_fvp(hv, hv32, hv64, what=""):
    """test_cpo128_primitives_vs_oracle's two Fisher-vector gates: fp64_gate.gate at 1e-6 max|f64| in the max-norm, and the
    float32 allclose."""
    G.gate(hv, hv32, hv64, f"fvp {what}", norms=G.MAX)
    np.testing.assert_allclose(hv, hv32, rtol=1e-4, atol=1e-5 * np.abs(hv64).max())
