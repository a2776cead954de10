"""The fused Fisher-vector product of the multi-agent actor (spo_ma_fvp, csrc/ma_fvp.hip) on the GPU: J^T diag(m) J v against
forward-mode + reverse-mode autograd on a plain torch network built from the flat theta, in float32 and float64, under the
project's rule |hip - f64| <= 3 |f32 - f64| + 1e-6 * scale per parameter block (tests/fp64_gate.py)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


class Sp:
    def __init__(self, n):
        self.shape = (n,)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _offsets(lib, net):
    """(which, block) -> offset, and the (offset, count) list of every parameter block of the flat vector."""
    D, H, NB, O = net.in_dim, net.hidden, net.n_blocks, net.out_dim
    off = lambda w, k=0: int(lib.spo_ma_param_offset(net, w, k))
    blocks = [(off(0), D), (off(1), D)]
    for k in range(NB):
        blocks += [(off(2, k), H * (D if k == 0 else H)), (off(3, k), H), (off(4, k), H), (off(5, k), H)]
    blocks += [(off(6), O), (off(7), O * H), (off(8), O)]
    return off, blocks


def _mean_of(theta, x, net, off):
    """LayerNorm -> [Linear -> ELU -> LayerNorm] x n_blocks -> Linear, on views of the flat theta."""
    D, H = net.in_dim, net.hidden
    cut = lambda o, *shape: theta[o:o + int(np.prod(shape))].reshape(*shape)
    h = F.layer_norm(x, (D,), cut(off(0), D), cut(off(1), D))
    for k in range(net.n_blocks):
        h = F.elu(F.linear(h, cut(off(2, k), H, h.shape[1]), cut(off(3, k), H)))
        h = F.layer_norm(h, (H,), cut(off(4, k), H), cut(off(5, k), H))
    return F.linear(h, cut(off(7), net.out_dim, H), cut(off(8), net.out_dim))


def _oracle(theta, x, vec, m_diag, rows_global, net, off, dtype):
    theta, x, vec, m = (t.detach().cpu().to(dtype) for t in (theta, x, vec, m_diag))
    f = lambda th: _mean_of(th, x, net, off)
    _, dmu = torch.func.jvp(f, (theta,), (vec,))
    _, pull = torch.func.vjp(f, theta)
    return pull(dmu * (m / rows_global))[0].numpy()


def _problem(dev, D, H, NB, O, rows, seed=0):
    """An actor from the model's own initialiser with perturbed LayerNorm gains / biases and a non-constant log_std, x, the
    activations spo_ma_forward leaves, v ~ N(0, 1) and MACPO's m_diag = 2 / (1e-8 + 2 sigma^2)."""
    from safepo import _abi
    from safepo.common.model import MultiAgentActor
    from safepo.multi_agent.macpo import default_cfg
    torch.manual_seed(1000 * D + 10 * H + NB + O + seed)
    cfg = dict(default_cfg, device=str(dev), hidden_size=H, layer_N=NB - 1)
    actor = MultiAgentActor(cfg, Sp(D), Sp(O), dev)
    lib = _abi.load()
    off, blocks = _offsets(lib, actor._net)
    g = torch.Generator().manual_seed(seed + rows)
    for w, k in [(0, 0), (1, 0)] + [(w, k) for k in range(NB) for w in (4, 5)]:
        n = D if w < 2 else H
        actor.theta[off(w, k):off(w, k) + n] += (0.3 * torch.randn(n, generator=g)).to(dev)
    actor.theta[off(6):off(6) + O] += (0.5 * torch.randn(O, generator=g)).to(dev)
    x = torch.randn(rows, D, generator=g).to(dev)
    vec = torch.randn(actor.theta.numel(), generator=g).to(dev)
    std = torch.sigmoid(actor.log_std / actor.std_x_coef) * actor.std_y_coef
    m_diag = (2.0 / (1e-8 + 2.0 * std * std)).contiguous()
    _, saved = actor.net_forward(x, keep=True)
    return actor, lib, off, blocks, x, vec, m_diag, saved


def _fvp(lib, actor, vec, m_diag, rows, rows_global, ws, scratch, out):
    from safepo import _abi
    return lib.spo_ma_fvp(_abi.ptr(actor.theta), actor._net, _abi.ptr(vec), _abi.ptr(m_diag), rows, rows_global, _abi.ptr(ws),
                          _abi.ptr(scratch), _abi.ptr(out), _abi.stream_ptr())


BASE = dict(D=48, H=128, NB=2, O=6, rows=33, share=1)
CASES = [BASE] + [dict(BASE, **{k: v}) for k, vs in (("rows", (1, 31, 32, 8225)), ("H", (65, 64, 20)), ("D", (1, 128)), ("O", (1, 16)),
                                                       ("NB", (1,)), ("share", (2,))) for v in vs]


@pytest.mark.parametrize("c", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_ma_fvp_vs_autograd_under_the_fp64_gate(dev, c):
    """One axis varied at a time around (48, 128, 2 blocks, 6, 33 rows): the chunk edge and the masked tail (1, 31, 32, 33 rows), a
    second trip through the chunk loop of the capped grid (8 225 = 256 x 32 + 33), full / ragged / at-most-four-tile hidden
    widths, in_dim 1 / 48 / 128, out_dim 1 / 6 / 16, one block, and rows_global = 2 rows (a data-parallel share)."""
    import fp64_gate as G
    from safepo import _abi
    actor, lib, off, blocks, x, vec, m_diag, (_, ws) = _problem(dev, c["D"], c["H"], c["NB"], c["O"], c["rows"])
    rows, rows_g = c["rows"], c["share"] * c["rows"]
    assert lib.spo_ma_fvp_supported(actor._net) == 1
    scratch = torch.full((int(lib.spo_ma_fvp_scratch_floats(actor._net, rows)),), float("nan"), device=dev)
    out = torch.full_like(actor.theta, float("nan"))
    _abi.check(_fvp(lib, actor, vec, m_diag, rows, rows_g, ws, scratch, out), "spo_ma_fvp")
    hip = out.cpu().numpy()
    with G.on_oracle_threads():
        f32, f64 = (_oracle(actor.theta, x, vec, m_diag, rows_g, actor._net, off, dt) for dt in (torch.float32, torch.float64))
    ls, O = off(6), c["O"]
    assert (hip[ls:ls + O] == 0).all() and (f64[ls:ls + O] == 0).all()
    G.gate_blocks(hip, f32, f64, [b for b in blocks if b[0] != ls], f"ma_fvp {c}")


def test_ma_fvp_repeats_are_bit_identical_and_stay_inside_out(dev):
    """Two calls on the same inputs, the scratch poisoned in between: the same bytes, and the guard floats on both sides of
    `out` untouched."""
    from safepo import _abi
    actor, lib, off, blocks, x, vec, m_diag, (_, ws) = _problem(dev, 48, 128, 2, 6, 2049)
    P, G = actor.theta.numel(), 64
    scratch = torch.zeros(int(lib.spo_ma_fvp_scratch_floats(actor._net, 2049)), device=dev)
    bufs = []
    for poison in (float("nan"), -7.0):
        scratch.fill_(poison)
        buf = torch.full((P + 2 * G,), 123.0, device=dev)
        _abi.check(_fvp(lib, actor, vec, m_diag, 2049, 2049, ws, scratch, buf[G:G + P]), "spo_ma_fvp")
        bufs.append(buf.cpu())
    assert torch.equal(bufs[0], bufs[1])
    assert (bufs[0][:G] == 123.0).all() and (bufs[0][G + P:] == 123.0).all() and torch.isfinite(bufs[0]).all()


def _cg(avp_of, b, nsteps=10, tol=1e-10):
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


def test_macpo_trainer_takes_the_fused_product_by_default(dev, monkeypatch):
    """MACPO_Trainer.fisher_vector_product and a ten-iteration conjugate_gradient at the benchmark's shape (obs 48, hidden 128,
    layer_N 1, act 6) on 2 049 rows: the default routing and SPO_MA_FVP=0, alternating in one process, both under the gate
    against the float64 oracle (product: per block; CG solution: as one vector) -- and SPO_MA_FVP=0 gives, bit for bit, what
    the forward-mode + backward pair gives when called directly.
    The inputs come from the host's generator, so the problem is the same on every machine: ten unconverged CG iterations
    amplify rounding, and on a badly conditioned draw (one made with the device's generator: |f32 - f64| from 1.7e-3 to 9.7e-2
    of a solution of scale 40 with the oracle's summation order alone) the float32 leg is one draw of noise that either route
    passes or fails with the host's BLAS.  On this draw every leg is within 2x of the floor (hip 4.9e-5 / 4.4e-5, float32
    2.0e-5 to 6.7e-5 over 1, 2, 4, 8 oracle threads, floor 3.8e-5)."""
    import fp64_gate as G
    from safepo.multi_agent.macpo import MACPO_Policy, MACPO_Trainer, default_cfg, mamujoco_cfg
    torch.manual_seed(5)
    rows, D, A = 2049, 48, 6
    cfg = dict(default_cfg, **mamujoco_cfg)
    cfg.update(device=str(dev))
    pol = MACPO_Policy(cfg, Sp(D), Sp(2 * D), Sp(A))
    tr = MACPO_Trainer(cfg, pol)
    actor = pol.actor
    from safepo import _abi
    off, blocks = _offsets(_abi.load(), actor._net)
    g = torch.Generator().manual_seed(5)          # the host's generator: the same problem on every machine
    rn = lambda *shape: torch.randn(*shape, generator=g).to(dev)
    for w, k in ((0, 0), (1, 0), (4, 0), (5, 0), (4, 1), (5, 1)):
        n = D if w < 2 else 128
        actor.theta[off(w, k):off(w, k) + n] += 0.3 * rn(n)
    actor.theta[off(6):off(6) + A] += 0.5 * rn(A)
    x = rn(rows, D)
    p, b = rn(actor.theta.numel()), rn(actor.theta.numel())
    _, saved = actor.net_forward(x, keep=True)
    m_diag = (2.0 / (1e-8 + 2.0 * tr._std() ** 2)).reshape(1, -1)
    h_ls = tr._kl_hessian_logstd()
    assert actor.fvp_supported()

    def both(fn):
        res = []
        for knob in (None, "0", None, "0"):
            monkeypatch.delenv("SPO_MA_FVP", raising=False) if knob is None else monkeypatch.setenv("SPO_MA_FVP", knob)
            res.append(fn().cpu())
        assert torch.equal(res[0], res[2]) and torch.equal(res[1], res[3])
        assert not torch.equal(res[0], res[1])          # two routes: a different summation order shows in the last bits
        return res[0].numpy(), res[1].numpy()
    fused, pair = both(lambda: tr.fisher_vector_product(saved, p, m_diag, h_ls))
    direct = torch.zeros_like(p)
    actor.net_backward(saved, actor.net_jvp(saved, p) * (m_diag / rows), direct)
    ls = off(6)
    direct[ls:ls + A] = h_ls * p[ls:ls + A]
    assert np.array_equal(pair, (direct + 0.1 * p).cpu().numpy())

    def oracle_avp(dtype):
        hl = torch.zeros(actor.theta.numel(), dtype=dtype)
        hl[ls:ls + A] = h_ls.cpu().to(dtype)
        md = m_diag.reshape(-1)
        return lambda v: torch.from_numpy(_oracle(actor.theta, x, v, md, rows, actor._net, off, dtype)) + hl * v + 0.1 * v
    with G.on_oracle_threads():
        o32, o64 = oracle_avp(torch.float32), oracle_avp(torch.float64)
        f32, f64 = o32(p.cpu()).numpy(), o64(p.cpu().double()).numpy()
        x32, x64 = _cg(o32, b.cpu()).numpy(), _cg(o64, b.cpu().double()).numpy()
    for name, got in (("fused", fused), ("SPO_MA_FVP=0", pair)):
        G.gate_blocks(got, f32, f64, blocks, f"fisher_vector_product, {name}")
    xf, xp = both(lambda: tr.conjugate_gradient(saved, b, 10, m_diag, h_ls))
    for name, got in (("fused", xf), ("SPO_MA_FVP=0", xp)):
        G.gate(got, x32, x64, f"conjugate_gradient, {name}")
