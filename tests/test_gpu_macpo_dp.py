"""Data-parallel MACPO on the GPU: the two kernels of the sharded trust-region step (spo_ma_trpo_linesearch_sums,
spo_ma_cg_init / spo_ma_cg_update) against torch under the fp64 yardstick (tests/ma_yardstick.py), the sharded form of
MACPO_Trainer at world size 1 against the reference's own golden, and two ranks on one GPU (tests/macpo_dp_worker.py)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---------------------------------------------------------------- line-search sums
def _ls_inputs(rows, A, seed):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    log_std = 1.0 + 0.3 * rn(A)
    std = 0.5 * torch.sigmoid(log_std / 1.0)
    mu_old = rn(rows, A)
    act = mu_old + std * rn(rows, A)
    d = act - mu_old
    std_old = 0.5 * torch.sigmoid((log_std + 0.05 * rn(A)) / 1.0)
    old_logp = -(d * d) / (2 * std_old * std_old) - torch.log(std_old) - 0.5 * np.log(2 * np.pi) + 0.02 * rn(rows, A)
    return {"mean": mu_old + 0.05 * rn(rows, A), "log_std": log_std, "act": act, "old_logp": old_logp, "adv": rn(rows),
            "cost_adv": rn(rows), "factor": 0.5 + torch.rand(rows, generator=g), "mu_old": mu_old, "std_old": std_old}


def _ls_torch(t, xc, yc, dtype):
    """The line-search expressions of MACPO_Trainer.trpo_update (host-driven path) in `dtype`: Normal log-probabilities per
    dimension, ratio = prod exp(logp - old), w = ratio * factor, the two surrogate sums, kl_divergence, as ROW SUMS, plus the
    sum of the magnitudes of every sum's terms (the scale its rounding error is relative to)."""
    t = {k: v.to(dtype) for k, v in t.items()}
    std = torch.sigmoid(t["log_std"] / xc) * yc
    d = t["act"] - t["mean"]
    logp = -(d * d) / (2 * std * std) - torch.log(std) - 0.5 * np.log(2 * np.pi)
    ratio = torch.prod(torch.exp(logp - t["old_logp"]), dim=-1, keepdim=True)
    w = ratio.reshape(-1) * t["factor"]
    so = t["std_old"].reshape(1, -1)
    quot = (so.pow(2) + (t["mu_old"] - t["mean"]).pow(2)) / (1e-8 + 2.0 * std.pow(2))
    kl = (torch.log(so) - torch.log(std) + quot - 0.5).sum(1, keepdim=True)
    sums = torch.stack([(w * t["adv"]).sum(), (w * t["cost_adv"]).sum(), kl.sum(), ratio.sum()])
    scales = torch.stack([(w * t["adv"]).abs().sum(), (w * t["cost_adv"]).abs().sum(),
                          (torch.log(so).abs() + torch.log(std).abs() + quot + 0.5).sum(), ratio.sum()])
    return sums.double().numpy(), ratio.reshape(-1).double().numpy(), scales.double().numpy()


def _ls_call(lib, t, xc, yc, dev, A=None, with_ratio=True):
    from safepo import _abi
    d = {k: v.to(dev).contiguous() for k, v in t.items()}
    rows = d["mean"].shape[0]
    A = d["mean"].shape[1] if A is None else A
    sums = torch.full((4,), float("nan"), dtype=torch.float64, device=dev)
    ratio = torch.full((rows,), float("nan"), dtype=torch.float32, device=dev) if with_ratio else None
    ws = torch.zeros(_abi.MA_LS_WS_DOUBLES, dtype=torch.float64, device=dev)
    rc = lib.spo_ma_trpo_linesearch_sums(_abi.ptr(d["mean"]), _abi.ptr(d["log_std"]), xc, yc, _abi.ptr(d["act"]), _abi.ptr(d["old_logp"]),
                                         _abi.ptr(d["adv"]), _abi.ptr(d["cost_adv"]), _abi.ptr(d["factor"]), _abi.ptr(d["mu_old"]),
                                         _abi.ptr(d["std_old"]), rows, A, _abi.ptr(sums), _abi.ptr(ratio), _abi.ptr(ws),
                                         _abi.stream_ptr())
    return rc, sums, ratio


@pytest.mark.parametrize("rows,A", [(1, 1), (70, 3), (2111, 16), (96, 6)])
def test_ma_trpo_linesearch_sums_vs_torch(dev, rows, A):
    """One row / one dimension, a partial wave, several workgroups with a ragged tail, the golden fixtures' shape: the four
    sums and the per-row ratio within 3x the distance of torch's float32 evaluation from the float64 one, + 1e-6 of the scale
    (the sum of the magnitudes of a sum's terms; the ratio's own largest value); bit-identical from call to call."""
    import ma_yardstick as Y
    from safepo import _abi
    lib = _abi.load()
    t = _ls_inputs(rows, A, 100 + rows)
    s32, r32, _ = _ls_torch(t, 1.0, 0.5, torch.float32)
    s64, r64, sc64 = _ls_torch(t, 1.0, 0.5, torch.float64)
    rc, sums, ratio = _ls_call(lib, t, 1.0, 0.5, dev)
    _abi.check(rc, "spo_ma_trpo_linesearch_sums")
    rc2, sums2, ratio2 = _ls_call(lib, t, 1.0, 0.5, dev)
    got = sums.cpu().numpy()
    for k, nm in enumerate(("sum w*adv", "sum w*cost_adv", "sum KL", "sum ratio")):
        d_hip, d_32 = Y.gate(got[k:k + 1], s32[k:k + 1], s64[k:k + 1], 1e-6, f"({rows},{A}) {nm}", scale=sc64[k])
        print(f"linesearch sums ({rows},{A}) {nm}: |hip-f64| {d_hip:.2e} vs |torch32-f64| {d_32:.2e} (scale {sc64[k]:.2e})")
    Y.gate(ratio.cpu().numpy(), r32, r64, 1e-6, f"({rows},{A}) per-row ratio")
    assert rc2 == 0 and torch.equal(sums, sums2) and torch.equal(ratio, ratio2)
    rc3, sums3, _ = _ls_call(lib, t, 1.0, 0.5, dev, with_ratio=False)           # the ratio output is optional
    assert rc3 == 0 and torch.equal(sums, sums3)


def test_ma_trpo_linesearch_sums_rejects_wide_actions(dev):
    from safepo import _abi
    lib = _abi.load()
    t = _ls_inputs(8, _abi.MAX_ACT + 1, 5)
    rc, sums, _ = _ls_call(lib, t, 1.0, 0.5, dev)
    assert rc != 0 and b"act_dim" in lib.spo_last_error()
    torch.cuda.synchronize(dev)
    assert torch.isnan(sums).all()              # nothing was launched
    rc0, _, _ = _ls_call(lib, _ls_inputs(8, 2, 5), 1.0, 0.5, dev, A=0)
    assert rc0 != 0


# ---------------------------------------------------------------- conjugate-gradient vector step
def _spd(n, seed):
    """avp(p) = A p for a symmetric positive-definite A of order n.  Dense up to n = 1000; beyond, diagonal plus rank 3 applied
    as vectors, so nothing of order n^2 exists."""
    g = torch.Generator().manual_seed(seed)
    cache = {}

    def on(t, p):                                   # the operator's pieces in p's dtype, on p's device
        key = (id(t), p.dtype, p.device)
        if key not in cache:
            cache[key] = t.to(p.dtype).to(p.device)
        return cache[key]
    if n <= 1000:
        m = torch.randn(n, n, generator=g, dtype=torch.float64) / max(n, 1) ** 0.5
        a = m @ m.T + 0.5 * torch.eye(n, dtype=torch.float64)
        return lambda p: on(a, p) @ p
    diag = 0.5 + torch.rand(n, generator=g, dtype=torch.float64)
    u = torch.randn(n, 3, generator=g, dtype=torch.float64) / n ** 0.5
    return lambda p: on(diag, p) * p + on(u, p) @ (on(u, p).T @ p)


def _cg_torch(avp_of, b, nsteps, tol=1e-10):
    """conjugate_gradient of the host-driven path (reference macpo.py:168-185) in b's dtype."""
    x = torch.zeros_like(b)
    r, p = b.clone(), b.clone()
    rdotr = torch.dot(r, r)
    for _ in range(nsteps):
        avp = avp_of(p)
        alpha = rdotr / (torch.dot(p, avp) + 1e-8)
        x += alpha * p
        r -= alpha * avp
        new_rdotr = torch.dot(r, r)
        p = r + (new_rdotr / rdotr) * p
        rdotr = new_rdotr
        if rdotr < tol:
            break
    return x


def _cg_hip(lib, avp_of, b, nsteps, tol, dev):
    from safepo import _abi
    b = b.to(dev)
    n = b.numel()
    x, r, p = (torch.full_like(b, float("nan")) for _ in range(3))
    state = torch.zeros(4, dtype=torch.float32, device=dev)
    ws = torch.zeros(_abi.MA_CG_WS_DOUBLES, dtype=torch.float64, device=dev)
    _abi.check(lib.spo_ma_cg_init(_abi.ptr(b), _abi.ptr(x), _abi.ptr(r), _abi.ptr(p), _abi.ptr(state), _abi.ptr(ws), n,
                                  _abi.stream_ptr()), "spo_ma_cg_init")
    for _ in range(nsteps):
        avp = avp_of(p).contiguous()
        _abi.check(lib.spo_ma_cg_update(_abi.ptr(avp), _abi.ptr(x), _abi.ptr(r), _abi.ptr(p), _abi.ptr(state), _abi.ptr(ws), n,
                                        tol, _abi.stream_ptr()), "spo_ma_cg_update")
    return x, state


@pytest.mark.parametrize("n", [1, 63, 1000, 100003])
def test_ma_cg_kernels_vs_torch_recurrence(dev, n):
    """Ten iterations on a symmetric positive-definite system: one element, a partial wave, one workgroup (one launch per
    update), several workgroups with a ragged tail (two launches, the last workgroup writes p).  x within 3x the distance of
    the float32 torch recurrence from the float64 one, + 1e-6 of the scale."""
    import ma_yardstick as Y
    from safepo import _abi
    lib = _abi.load()
    avp_of = _spd(n, 7 + n)
    b = torch.randn(n, generator=torch.Generator().manual_seed(n), dtype=torch.float64)
    x32 = _cg_torch(avp_of, b.float(), 10)
    x64 = _cg_torch(avp_of, b.clone(), 10)
    x, state = _cg_hip(lib, avp_of, b.float(), 10, 1e-10, dev)
    d_hip, d_32 = Y.gate(x.cpu().numpy(), x32.numpy(), x64.numpy(), 1e-6, f"CG solution, n = {n}")
    print(f"cg n={n}: max|hip-f64| {d_hip:.2e} vs |torch32-f64| {d_32:.2e}; state {state.tolist()}")
    x_again, _ = _cg_hip(lib, avp_of, b.float(), 10, 1e-10, dev)
    assert torch.equal(x, x_again)


@pytest.mark.parametrize("n", [63, 100003])
def test_ma_cg_done_flag_freezes_the_solve(dev, n):
    """residual_tol above the first residual: the first update sets the flag, and nine more leave x untouched -- ten enqueued
    updates give what the reference's `break` gives."""
    from safepo import _abi
    lib = _abi.load()
    avp_of = _spd(n, 7 + n)
    b = torch.randn(n, generator=torch.Generator().manual_seed(n)).float()
    x1, st1 = _cg_hip(lib, avp_of, b, 1, 1e30, dev)
    x10, st10 = _cg_hip(lib, avp_of, b, 10, 1e30, dev)
    assert st1[1].item() == 1.0 and st10[1].item() == 1.0
    assert torch.equal(x1, x10) and torch.equal(st1, st10)
    assert torch.isfinite(x1).all() and x1.abs().max() > 0
    want = _cg_torch(avp_of, b, 10, tol=1e30)                   # the reference breaks after its first iteration
    np.testing.assert_allclose(x1.cpu().numpy(), want.numpy(), rtol=1e-5, atol=1e-6 * float(want.abs().max()))


# ---------------------------------------------------------------- the sharded form of the trainer
@pytest.mark.parametrize("tag", ["safe", "unsafe", "mamujoco", "recover", "deep_safe"])
def test_ma_macpo_sharded_form_vs_reference_golden(dev, golden_dir, tag):
    """macpo_sharded_form=True at world size 1: two trpo_update steps on the device-resident CG and the line-search sums
    kernel against the reference's own trainer (tests/golden/ma_macpo.npz) -- every recorded column, cost_grad, both CG
    solutions, the step and the actor after the line search under the gate and floors of
    test_ma_macpo_trainer_vs_reference_golden."""
    import macpo_dp_worker as W
    z = np.load(os.path.join(golden_dir, "ma_macpo.npz"))
    pol, tr, sample = W.golden_trainer(z, tag, dev, macpo_sharded_form=True)
    assert tr.sharded and tr.comm.world_size == 1
    rec = W.two_steps(pol, tr, sample)
    W.gate_against_golden(z, tag, rec)


def _launch_worker(tmp_path, out_name, *args):
    s_ = socket.socket(); s_.bind(("127.0.0.1", 0)); port = s_.getsockname()[1]; s_.close()
    out = tmp_path / out_name
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "macpo_dp_worker.py"), str(out)] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return out


@pytest.mark.parametrize("tag", ["safe", "recover"])
def test_ma_macpo_data_parallel_two_ranks_vs_reference_golden(dev, golden_dir, tmp_path, tag):
    """Two ranks (two processes on this GPU, gloo) x 48 of the 96 rows of a golden case, a feasible and a recovery one: the
    replicas stay bit-identical (actor, both critics, PopArt state), and the step on the WHOLE 96 rows holds the same gate
    against the reference's recorded result and the float64 oracle as the single-rank trainer."""
    import macpo_dp_worker as W
    out = _launch_worker(tmp_path, f"macpo_dp_{tag}.npz", "golden", tag)
    rec = dict(np.load(out))
    assert int(rec["world"]) == 2 and bool(rec["replicas_identical"])
    W.gate_against_golden(np.load(os.path.join(golden_dir, "ma_macpo.npz")), tag, rec)


def test_ma_macpo_train_data_parallel_two_ranks_one_gpu(dev, tmp_path):
    """MACPO_Trainer.train on a synthetic buffer split over two ranks against a single-rank trainer (the host-driven path) on
    the whole buffer: global advantage standardisation, all-reduced gradients / products / line-search sums.  Same case of the
    (lam, nu) analysis and the same accepted line-search step on both sides.  Bounds: those the project holds MACPO's fp32
    results to elsewhere (tests/test_oracle_golden.py, the macpo runner trace: rtol 2e-3, atol 2e-5 on parameters and stored
    scalars -- ten CG iterations amplify reduction-order noise); the two sides differ only in reduction order."""
    res = json.load(open(_launch_worker(tmp_path, "macpo_dp_train.json", "train")))
    assert res["world"] == 2 and res["replicas_identical"], {k: res[k] for k in ("world", "replicas_identical")}
    assert res["step_info"][0] == res["step_info"][1], res["step_info"]
    assert res["step_info"][0]["accepted_step"] >= 0 and res["actor_moved"] > 1e-4, (res["step_info"], res["actor_moved"])
    np.testing.assert_allclose(res["theta"], res["theta_single"], rtol=2e-3, atol=2e-5)
    np.testing.assert_allclose(res["popart"][0], res["popart"][1], rtol=1e-5)
    sc = np.abs(np.asarray(res["scalars"][1]))
    # kl / improve / expected improve are differences of nearly equal numbers: their scale is the surrogate's (column 5)
    np.testing.assert_allclose(res["scalars"][0], res["scalars"][1], rtol=2e-3, atol=2e-5 * max(1.0, sc[5]))
    assert res["ratio_mean"][0] == pytest.approx(res["ratio_mean"][1], rel=1e-5)
