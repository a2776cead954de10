"""GPU tests of data-parallel FOCOPS / CUP: the split KL-penalty gradient (spo_kl_penalty_grad), the optimiser step on the
all-reduced buffer (spo_clip_adam_ex) and PPOLagEngine's world_size > 1 branch of learning_iter_ex, two ranks on one GPU
(tests/kl_penalty_dp_worker.py) against the CPU oracle on the union of the ranks' rows."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "safe-policy-optimization_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _run_worker(tmp_path, use_p2p: str, shape: str, mode: str, dp_batch: str = "global", local_rows: int = 64) -> dict:
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    out = tmp_path / f"kl_dp_{mode}.json"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "kl_penalty_dp_worker.py"), str(out), use_p2p, shape, mode,
           dp_batch, str(local_rows)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.load(open(out))


def _check_trajectory(res, loss_rel=1e-4, theta_abs=1e-5):
    assert res["replicas_identical"], res
    assert res["theta_frac_outside"] <= 1e-3 and res["theta_max_abs_diff"] < theta_abs and res["theta_moved"] > 1e-3, res
    assert res["loss_max_rel_diff"] < loss_rel, res
    if "loss_max_scaled_diff" in res:
        assert res["loss_max_scaled_diff"] < 1e-4, res


PERSISTENT = ["60,8,64,64", "100,4,64,64"]
WIDE = ["100,20,64,64", "60,8,128,128", "376,17,64,64"]           # act_dim > 16, hidden [128, 128], HumanoidVelocity


def _engine(shape):
    return "PPOLagEngine" if shape in PERSISTENT else "WidePPOLagEngine"


@pytest.mark.parametrize("shape,p2p", [(s, p) for s in PERSISTENT for p in ("0", "1")] + [(s, "0") for s in WIDE])
def test_dp_focops_global_batch_equals_reference_minibatches(tmp_path, shape, p2p):
    """2 ranks x 32 rows per step against KLPenaltyUpdater.focops_step on the 64-row union.  Rank 0's rows all lie inside the KL
    bound, rank 1's about half of them: the fraction of the global minibatch differs from each rank's own (the worker checks
    that it does, and that every row's KL stays 10 % away from the bound), so only the global F reproduces the oracle.
    p2p = 1: the peer regions of the in-kernel exchange are present (asserted) and the path still takes kernel / all-reduce /
    kernel.  The wide shapes run the wide engine's split step (spo_wide_kl_penalty_split, two actor backward passes,
    spo_wide_kl_penalty_combine); 376 / 17 takes the launch-per-layer form under data parallelism."""
    res = _run_worker(tmp_path, p2p, shape, "focops")
    assert res["engine"] == _engine(shape), res
    assert res["in_kernel_exchange"] == (p2p == "1"), res
    assert res["local_batch"] == 32 and res["steps"] == 16 and res["clocks"] == [16, 0], res
    assert res["f_local_differs"] and res["kl_margin"] >= 0.1, res
    # 376 inputs: the float32 forward passes of GPU and oracle differ by ~1e-6 in the means.  The actor's loss (a mean of
    # random-sign ratio*adv terms) passes near 0 -- element-wise 1e-3 there, every loss within 1e-4 of its column's size; and a
    # parameter whose gradient is near 0 can take a different Adam step (the step is ~lr whatever the gradient's size): the
    # largest parameter difference is bounded by one step, lr = 3e-4, while the fraction outside the envelope stays <= 1e-3
    wide_in = shape.startswith("376,")
    _check_trajectory(res, loss_rel=1e-3 if wide_in else 1e-4, theta_abs=3e-4 if wide_in else 1e-5)


@pytest.mark.parametrize("shape", PERSISTENT + ["100,20,64,64"])
def test_dp_cup_both_stages_equal_reference(tmp_path, shape):
    """CUP: a pass of the clipped first stage with the actor's optimiser clock 5 steps ahead of the critics', then a pass of the
    actor-only second stage (F = 1): losses and parameters against KLPenaltyUpdater.minibatch_step / cup_second_stage_step; in the
    second stage only the actor's clock advances and the critics stay bit-equal."""
    res = _run_worker(tmp_path, "0", shape, "cup")
    assert res["engine"] == _engine(shape), res
    assert res["clocks"] == [[16, 5], [16, 21]], res
    assert res["critics_unchanged_stage2"], res
    assert res["stage1_theta_max_abs_diff"] < 1e-5, res
    _check_trajectory(res)


@pytest.mark.parametrize("shape,rows", [("60,8,64,64", 64), ("60,8,64,64", 128), ("100,20,64,64", 64)])
def test_dp_focops_local_batch_equals_reference_on_union(tmp_path, shape, rows):
    """dp_batch = local: every rank takes `rows` rows per step, the oracle steps on the union of both ranks' rows.  128 rows per
    rank: the gradient kernel's minibatch spans two 64-column passes (the counts and sums accumulate across them)."""
    res = _run_worker(tmp_path, "0", shape, "focops", dp_batch="local", local_rows=rows)
    assert res["engine"] == _engine(shape), res
    assert res["local_batch"] == rows and res["steps"] == 8, res
    assert res["f_local_differs"] and res["kl_margin"] >= 0.1, res
    _check_trajectory(res)


@pytest.mark.parametrize("algo", ["focops", "cup"])
def test_dp_focops_cup_main_two_ranks(tmp_path, algo):
    """focops.main / cup.main under 2 ranks on one GPU (SynthSafe-v0, 2 epochs, learning_iters 2): they run, log both epochs,
    record the gradient exchange and end with identical replicas."""
    res = _run_worker(tmp_path, "0", "0", f"e2e_{algo}")
    assert res["engine"] == "PPOLagEngine", res
    assert res["rows"] == 2 and res["stop_iter"], res
    assert res["second_stage"] == (algo == "cup"), res
    assert res["gradient_exchange"], res
    assert res["replicas_identical"], res


def test_clip_adam_ex_equals_clip_adam_bitwise():
    """spo_clip_adam_ex with equal clocks, every parameter and no combine is spo_clip_adam, bit for bit (also when it clips)."""
    from safepo import _abi
    import ctypes
    lib = _abi.load()
    dev = torch.device("cuda:0")
    D, A = 60, 8
    P = int(lib.spo_param_count(D, A))
    g = torch.Generator(device=dev).manual_seed(5)
    for max_norm in (40.0, 0.05):
        cfg = _abi.PpoCfg(obs_dim=D, act_dim=A, batch=64, use_critic_norm=1, use_value_coefficient=0, clip=0.2,
                          max_grad_norm=max_norm, lr_actor=2e-4, lr_critic=3e-4, beta1=0.9, beta2=0.999, adam_eps=1e-8,
                          l2_coef=0.001)
        th = torch.randn(P, device=dev, generator=g)
        m = 0.01 * torch.randn(P, device=dev, generator=g)
        v = 1e-4 * torch.rand(P, device=dev, generator=g)
        grad = torch.randn(P, device=dev, generator=g)
        outs = []
        for ex in (False, True):
            t_, m_, v_ = th.clone(), m.clone(), v.clone()
            if ex:
                rc = lib.spo_clip_adam_ex(_abi.ptr(t_), _abi.ptr(m_), _abi.ptr(v_), _abi.ptr(grad), None, None, 7, 7, 0.5, 0.0, 0,
                                          ctypes.byref(cfg), None, _abi.stream_ptr())
            else:
                rc = lib.spo_clip_adam(_abi.ptr(t_), _abi.ptr(m_), _abi.ptr(v_), _abi.ptr(grad), 7, 0.5, ctypes.byref(cfg),
                                       _abi.stream_ptr())
            _abi.check(rc, "clip_adam")
            outs.append((t_, m_, v_))
        torch.cuda.synchronize()
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        assert not torch.equal(outs[0][0], th)
