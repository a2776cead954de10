"""GPU tests of the staged minibatch inputs of the row-split update kernel (csrc/update_rs.hip: rs_stage_inputs_kernel, template
flag STG, SPO_RS_STAGE / SPO_RS_STAGE_MAX_MB).  The pre-pass is pure data movement, so its records are compared with a torch gather
by torch.equal; the staged launch feeds the same bits into the same arithmetic in the same order, so its reference is the in-kernel
gather on the same machine (SPO_RS_STAGE=0, read at every launch) and the comparison is bit for bit."""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_parity import _synthetic_update_problem, _fill_update_problem  # noqa: E402

CFG = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "learning_iters": 1}
SHAPES = [(60, 8), (64, 16), (17, 3), (1, 1)]                 # KIN 64 with padding; no padding; KIN 32, D % 4 != 0; KIN 16
BATCHES = [(64, 64 * 3 + 5),                                  # short last minibatch
           (64, 37),                                          # one partial step
           (40, 40 * 2 + 9),                                  # second row group partly empty
           (32, 32 * 2)]                                      # second row group has no valid column


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _default_routing(monkeypatch):
    for k in ("SPO_RS_OBS128", "SPO_RS_SAFE", "SPO_RS_L1_PIPE", "SPO_FORCE_DP", "SPO_RS_STAGE", "SPO_RS_STAGE_MAX_MB"):
        monkeypatch.delenv(k, raising=False)
    assert int(os.environ.get("SPO_UPDATE_FORM", "3")) >= 3, "SPO_UPDATE_FORM selects an older form in this process: unset it"
    assert os.environ.get("SPO_RS_ROWS", "32") != "16", "SPO_RS_ROWS=16 selects the four-row-group form in this process: unset it"


def _lib():
    from safepo import _abi
    return _abi.load()


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
    _fill_update_problem(eng, (obs, act, logp, scale * tgt_r, scale * tgt_c, scale * adv))
    return eng


def _run(D, A, batch, Ms, mg, scale, dev, env, monkeypatch, n_perms=1):
    """A fresh engine, then one launch per (M in Ms, perm) on one stream under `env`: (theta, adam_m, adam_v, losses), the
    [steps, redone] counters, and spo_debug_rs_last_staged() after the last launch."""
    lib = _lib()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = _engine(D, A, batch, max(Ms), mg, scale, dev)
    g = torch.Generator().manual_seed(9)
    _counters(lib)
    losses = []
    for M in Ms:
        for _ in range(n_perms):
            perm = torch.randperm(M, generator=g).to(torch.int32).to(dev)
            eng.M = M
            losses.append(eng.learning_iter(perm).clone())
    eng.check_sync_error()
    staged = int(lib.spo_debug_rs_last_staged())
    counts = _counters(lib)[:2]
    for k in env:
        monkeypatch.delenv(k)
    out = (eng.policy.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), torch.cat(losses, 0))
    assert all(torch.isfinite(t).all() for t in out)
    return out, counts, staged


def _assert_same(got, ref, what):
    for name, x, y in zip(("theta", "adam_m", "adam_v", "losses"), got, ref):
        assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} of {x.numel()} entries"


# ------------------------------------------------------------------------------------------------ 1. the pre-pass against a gather
def _expected_records(obs, act, logp, adv, tgt_r, tgt_c, perm, D, A, B):
    M = obs.shape[0]
    kin = 16 if D <= 16 else 32 if D <= 32 else 64
    nsteps = (M + B - 1) // B
    s = torch.arange(nsteps).view(-1, 1)
    c = torch.arange(B).view(1, -1)
    ncols = torch.clamp(M - s * B, max=B)
    smp = perm.long()[s * B + torch.where(c < ncols, c, torch.zeros_like(c))]             # [nsteps, B]
    x = torch.zeros(nsteps, 64, kin)
    x[:, :B, :D] = obs[smp]
    a = torch.zeros(nsteps, 64, 16)
    a[:, :B, :A] = act[smp]
    sc = torch.zeros(nsteps, 4, 64)
    for i, t in enumerate((logp, adv, tgt_r, tgt_c)):
        sc[:, i, :B] = t[smp]
    return torch.cat([x.reshape(nsteps, -1), x.transpose(1, 2).reshape(nsteps, -1), a.reshape(nsteps, -1), sc.reshape(nsteps, -1)], 1)


@pytest.mark.parametrize("batch,M", BATCHES, ids=lambda v: str(v))
@pytest.mark.parametrize("D,A", SHAPES, ids=lambda v: str(v))
def test_staging_kernel_equals_a_torch_gather(dev, D, A, batch, M):
    from safepo import _abi
    lib = _lib()
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=7 * M + D)
    obs[0, 0] = float("nan"); obs[M - 1, D - 1] = -0.0                                  # bit copies, whatever the bits
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(M)).to(torch.int32)
    want = _expected_records(obs, act, logp, adv, tgt_r, tgt_c, perm, D, A, batch)
    nbytes = int(lib.spo_rs_stage_bytes(D, A, batch, M))
    assert nbytes == want.numel() * 4 and want.shape[1] * 4 % 256 == 0
    out = torch.full((nbytes // 4,), 7.0, dtype=torch.float32, device=dev)             # no word may be left as it was
    d = [t.to(dev).contiguous() for t in (obs, act, logp, tgt_r, tgt_c, adv)]
    p = perm.to(dev)
    _abi.check(lib.spo_debug_rs_stage(*[_abi.ptr(t) for t in d], _abi.ptr(p), M, D, A, batch, _abi.ptr(out), nbytes,
                                      _abi.stream_ptr()), "spo_debug_rs_stage")
    torch.cuda.synchronize()
    got = out.cpu().view(want.shape)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))                    # (as words: NaN and -0.0 included)


# ------------------------------------------------------------------------------------------------ 2. staged against unstaged launches
@pytest.mark.parametrize("batch,M", BATCHES, ids=lambda v: str(v))
@pytest.mark.parametrize("D,A", SHAPES, ids=lambda v: str(v))
def test_staged_launch_gives_the_bits_of_the_unstaged_one(dev, monkeypatch, D, A, batch, M):
    lib = _lib()
    assert lib.spo_update_rs_supported(D, A, batch, 3) == 1
    nst = (M + batch - 1) // batch
    ref, c0, s0 = _run(D, A, batch, [M], 40.0, 0.7, dev, {"SPO_RS_STAGE": "0"}, monkeypatch, n_perms=2)
    assert s0 == 0 and c0[0] == 2 * nst
    for form in ("1", "2"):
        got, c, staged = _run(D, A, batch, [M], 40.0, 0.7, dev, {"SPO_RS_STAGE": form}, monkeypatch, n_perms=2)
        assert staged in (1, 2) and c == c0, (form, staged, c, c0)
        _assert_same(got, ref, f"SPO_RS_STAGE={form}")
    got, c, staged = _run(D, A, batch, [M], 40.0, 0.7, dev, {}, monkeypatch, n_perms=2)  # unset: on
    assert staged == 1 and c == c0
    _assert_same(got, ref, "SPO_RS_STAGE unset")


@pytest.mark.parametrize("nsteps", [1, 2, 3, 4])
def test_pipeline_prologue_edges(dev, monkeypatch, nsteps):
    D, A, batch = 60, 8, 64
    M = batch * nsteps
    ref, c0, _ = _run(D, A, batch, [M], 40.0, 0.7, dev, {"SPO_RS_STAGE": "0"}, monkeypatch)
    assert c0[0] == nsteps
    for form in ("1", "2"):
        got, c, staged = _run(D, A, batch, [M], 40.0, 0.7, dev, {"SPO_RS_STAGE": form}, monkeypatch)
        assert staged == int(form) and c == c0
        _assert_same(got, ref, f"{nsteps} steps, SPO_RS_STAGE={form}")


@pytest.mark.parametrize("D,A,extra,form", [(60, 8, {"SPO_RS_SAFE": "1"}, 1),
                                           (20, 3, {"SPO_RS_L1_PIPE": "0"}, 1),       # KIN = 32: one hand-off form, staged
                                           (60, 8, {"SPO_RS_L1_PIPE": "0"}, 0)],      # KIN = 64, one-batch A/B form: not built staged
                         ids=lambda v: str(v))
def test_staged_launch_under_the_other_knobs(dev, monkeypatch, D, A, extra, form):
    batch, M = 64, 64 * 5 + 3
    ref, c0, _ = _run(D, A, batch, [M], 40.0, 0.7, dev, dict(extra, SPO_RS_STAGE="0"), monkeypatch)
    got, c, staged = _run(D, A, batch, [M], 40.0, 0.7, dev, dict(extra, SPO_RS_STAGE="1"), monkeypatch)
    assert staged == form and c == c0
    _assert_same(got, ref, str(extra))


def test_repeated_layer_1_runs_on_staged_inputs(dev, monkeypatch):
    """max_grad_norm 1.2 with the targets scaled by 0.7 (tests/test_gpu_rs_l1_pipe.py: 18 of these 114 steps above the bound in
    the float32 oracle): the clip is active on part of the steps, so layer 1 is restored, redone and repeated by the column waves."""
    D, A, batch, M = 60, 8, 64, 64 * 37 + 19
    nst = (M + batch - 1) // batch
    ref, c0, _ = _run(D, A, batch, [M], 1.2, 0.7, dev, {"SPO_RS_STAGE": "0"}, monkeypatch, n_perms=3)
    assert c0[0] == 3 * nst and 0 < c0[1] < 3 * nst, c0
    for form in ("1", "2"):
        got, c, staged = _run(D, A, batch, [M], 1.2, 0.7, dev, {"SPO_RS_STAGE": form}, monkeypatch, n_perms=3)
        assert staged == int(form) and c == c0, (c, c0)
        _assert_same(got, ref, f"clip active, SPO_RS_STAGE={form}")


# ------------------------------------------------------------------------------------------------ 3. routing
def test_routing(dev, monkeypatch):
    lib = _lib()
    D, A, batch = 60, 8, 64
    Ms = [64 * 2, 64 * 30 + 11]                                 # two launches on one stream; the second needs 31 records > 1 MiB
    assert lib.spo_rs_stage_bytes(D, A, batch, Ms[0]) < (1 << 20) < lib.spo_rs_stage_bytes(D, A, batch, Ms[1])
    torch.cuda.synchronize()
    assert lib.spo_update_scratch_release(None, 1) >= 0         # the stream's block starts from nothing: the second launch grows it
    staged_run, c0, staged = _run(D, A, batch, Ms, 40.0, 0.7, dev, {"SPO_RS_STAGE": "1"}, monkeypatch)
    assert staged == 1
    off, c, staged = _run(D, A, batch, Ms, 40.0, 0.7, dev, {"SPO_RS_STAGE": "0"}, monkeypatch)
    assert staged == 0 and c == c0
    _assert_same(off, staged_run, "SPO_RS_STAGE=0")
    capped, c, staged = _run(D, A, batch, Ms, 40.0, 0.7, dev, {"SPO_RS_STAGE_MAX_MB": "1"}, monkeypatch)
    assert staged == 0 and c == c0                              # (the last launch would need more than 1 MiB)
    _assert_same(capped, staged_run, "SPO_RS_STAGE_MAX_MB=1")
    shrink, c, staged = _run(D, A, batch, Ms[::-1], 40.0, 0.7, dev, {}, monkeypatch)      # large then small: the block is kept
    ref, c1, _ = _run(D, A, batch, Ms[::-1], 40.0, 0.7, dev, {"SPO_RS_STAGE": "0"}, monkeypatch)
    assert staged == 1 and c == c1
    _assert_same(shrink, ref, "large launch, then a small one")
