"""The fused surrogate-gradient pair of the multi-agent actor (spo_ma_trpo_grads, csrc/ma_trpo_grads.hip) on the GPU against
torch.autograd.grad of -mean(factor * ratio * adv) and of the same with cost_adv on a plain torch network built from the flat
theta, in float32 and float64, under the project's rule |hip - f64| <= 3 |f32 - f64| + 1e-6 * scale per parameter block
(tests/fp64_gate.py)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_ma_fvp import Sp, _mean_of, _offsets, _problem, dev  # noqa: E402,F401  (the actor and its torch restatement)

pytestmark = pytest.mark.gpu


def _inputs(actor, off, x, seed, zero_cost):
    """act ~ N(mu, std) at theta, old_logp 0.1 off its log-probabilities (ratios away from 1), factor in [0.5, 1.5], independent
    normal advantages with adv == 0 on every third row.  -> (mean, act, old_logp, adv, cost_adv, factor) on the device."""
    g = torch.Generator().manual_seed(seed)
    rows, O = x.shape[0], actor.act_dim
    th = actor.theta.detach().cpu()
    mu = _mean_of(th, x.cpu(), actor._net, off)
    std = torch.sigmoid(th[off(6):off(6) + O] / actor.std_x_coef) * actor.std_y_coef
    act = mu + std * torch.randn(rows, O, generator=g)
    old_logp = torch.distributions.Normal(mu, std).log_prob(act) + 0.1 * torch.randn(rows, O, generator=g)
    adv, cadv = torch.randn(rows, generator=g), torch.randn(rows, generator=g)
    adv[::3] = 0.0
    if zero_cost:
        cadv.zero_()
    t = (act, old_logp, adv, cadv, 0.5 + torch.rand(rows, generator=g))
    return (actor.net_forward(x),) + tuple(u.contiguous().to(x.device) for u in t)


def _oracle(theta, x, t, rows_global, net, off, xc, yc, dtype):
    """-> [loss_r, loss_c], [grad_r, grad_c]"""
    theta = theta.detach().cpu().to(dtype).requires_grad_(True)
    act, old_logp, adv, cadv, factor = (v.detach().cpu().to(dtype) for v in t[1:])
    mu = _mean_of(theta, x.detach().cpu().to(dtype), net, off)
    std = torch.sigmoid(theta[off(6):off(6) + net.out_dim] / xc) * yc
    ratio = torch.prod(torch.exp(torch.distributions.Normal(mu, std).log_prob(act) - old_logp), dim=-1)
    losses = [-(factor * ratio * a).sum() / rows_global for a in (adv, cadv)]
    grads = [torch.autograd.grad(l, theta, retain_graph=True)[0].numpy() for l in losses]
    return [float(l.detach()) for l in losses], grads


def _call(lib, actor, ws, t, rows, rows_global, scratch, grad_r, grad_c, losses):
    from safepo import _abi
    return lib.spo_ma_trpo_grads(_abi.ptr(actor.theta), actor._net, _abi.ptr(ws), *(_abi.ptr(u) for u in t), actor.std_x_coef,
                                 actor.std_y_coef, rows, rows_global, _abi.ptr(scratch), _abi.ptr(grad_r), _abi.ptr(grad_c),
                                 _abi.ptr(losses), _abi.stream_ptr())


BASE = dict(D=48, H=128, NB=2, O=6, rows=33, share=1, zero_cost=False)
CASES = [BASE] + [dict(BASE, **{k: v}) for k, vs in (("rows", (1, 31, 32, 8225)), ("H", (65, 20)), ("D", (1, 128)), ("O", (1, 16)),
                                                       ("NB", (1,)), ("share", (2,)), ("zero_cost", (True,))) for v in vs]


def _case(dev, c, draw=0):
    """One call on NaN-filled scratch and outputs, and both oracles.  -> blocks, (hip, f32, f64) gradients [2, P] and losses [2]"""
    import fp64_gate as G
    from safepo import _abi
    actor, lib, off, blocks, x, _, _, (_, ws) = _problem(dev, c["D"], c["H"], c["NB"], c["O"], c["rows"], seed=draw)
    rows, rows_g = c["rows"], c["share"] * c["rows"]
    t = _inputs(actor, off, x, 11 + rows + 100 * draw, c["zero_cost"])
    assert lib.spo_ma_trpo_grads_supported(actor._net) == 1
    scratch = torch.full((int(lib.spo_ma_trpo_grads_scratch_floats(actor._net, rows)),), float("nan"), device=dev)
    grads, losses = torch.full((2, actor.theta.numel()), float("nan"), device=dev), torch.full((2,), float("nan"), device=dev)
    _abi.check(_call(lib, actor, ws, t, rows, rows_g, scratch, grads[0], grads[1], losses), "spo_ma_trpo_grads")
    with G.on_oracle_threads():
        (l32, g32), (l64, g64) = (_oracle(actor.theta, x, t, rows_g, actor._net, off, actor.std_x_coef, actor.std_y_coef, dt)
                                  for dt in (torch.float32, torch.float64))
    return blocks, (grads.cpu().numpy(), g32, g64), (losses.cpu().numpy(), l32, l64)


@pytest.mark.parametrize("c", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_ma_trpo_grads_vs_autograd_under_the_fp64_gate(dev, c):
    """One axis varied at a time around (48, 128, 2 blocks, 6, 33 rows): the masked tail, the chunk edge and a second trip through
    the chunk loop of the capped grid (8 225 = 256 x 32 + 33), ragged and at-most-four-tile hidden widths, in_dim 1 / 128, out_dim
    1 / 16, one block (both gradients resident; two blocks: the split form), rows_global = 2 rows.  With cost_adv == 0 on every row
    the cost gradient is exactly 0 in every entry: no gradient is derived from the other by a division.  Scratch and outputs start
    as NaN.  Every parameter block of each gradient and each loss is gated at its own scale.
    A one-entry block (the input LayerNorm's gain and bias at in_dim 1, log_std and the head bias at out_dim 1) is a single scalar,
    and one draw of the float32 oracle's rounding is no yardstick for it: over four input draws the oracle's own deviation of the
    input LayerNorm's bias gradient went from 1.1e-9 to 2.9e-7 and the kernel's from 1.8e-9 to 2.7e-7, each the larger one in some
    draw (profiles/ma_trpo_grads/one_entry_blocks.txt).  Such an entry is gated per gradient as a group over four draws, each
    member relative to its own float64 value (fp64_gate.gate_group)."""
    import fp64_gate as G
    blocks, (hip, g32, g64), (hl, l32, l64) = _case(dev, c)
    for k, name in enumerate(("reward", "cost")):
        if c["zero_cost"] and k == 1:
            assert (hip[1] == 0).all() and hl[1] == 0 and (g64[1] == 0).all()
            continue
        G.gate(hl[k], l32[k], l64[k], f"ma_trpo_grads {name} loss {c}")
        G.gate_blocks(hip[k], g32[k], g64[k], [b for b in blocks if b[1] > 1], f"ma_trpo_grads {name} gradient {c}")
    ones = [o for o, n in blocks if n == 1]
    if ones:
        draws = [(hip, g32, g64)] + [_case(dev, c, d)[1] for d in (1, 2, 3)]
        for k, name in enumerate(("reward", "cost")):
            for o in ones:
                G.gate_group([(h[k][o], a[k][o], b[k][o], None) for h, a, b in draws], f"ma_trpo_grads {name} gradient entry {o}, four draws {c}")


def test_ma_trpo_grads_repeats_are_bit_identical(dev):
    """Two calls at 8 225 rows, the scratch poisoned differently in between: the same bytes in both gradients and both losses."""
    from safepo import _abi
    actor, lib, off, _, x, _, _, (_, ws) = _problem(dev, 48, 128, 2, 6, 8225)
    t = _inputs(actor, off, x, 3, False)
    scratch = torch.empty(int(lib.spo_ma_trpo_grads_scratch_floats(actor._net, 8225)), device=dev)
    res = []
    for poison in (float("nan"), -7.0):
        scratch.fill_(poison)
        out = torch.full((2 * actor.theta.numel() + 2,), float("nan"), device=dev)
        P = actor.theta.numel()
        _abi.check(_call(lib, actor, ws, t, 8225, 8225, scratch, out[:P], out[P:2 * P], out[2 * P:]), "spo_ma_trpo_grads")
        res.append(out.cpu())
    assert torch.equal(res[0], res[1]) and torch.isfinite(res[0]).all()


@pytest.mark.parametrize("kw,rows,rc,word", [
    (dict(hidden=129), 33, -2, b"hidden 129"), (dict(in_dim=129), 33, -2, b"in_dim 129"), (dict(out_dim=17), 33, -2, b"out_dim 17"),
    (dict(n_blocks=3), 33, -2, b"n_blocks 3"), (dict(is_actor=0, out_dim=1), 33, -2, b"is_actor"), (dict(), 0, -1, b"bad args"),
])
def test_ma_trpo_grads_refusals(dev, kw, rows, rc, word):
    """Outside the envelope: -2 with the dimension named, supported 0, scratch -1.  rows = 0: -1 and scratch -1 for a supported net."""
    from safepo import _abi
    lib = _abi.load()
    net = _abi.MaNet(**dict(dict(in_dim=48, hidden=128, n_blocks=2, out_dim=6, is_actor=1), **kw))
    buf = torch.zeros(64, device=dev)
    p = _abi.ptr(buf)
    assert lib.spo_ma_trpo_grads(p, net, *([p] * 7), 1.0, 0.5, rows, rows, p, p, p, p, _abi.stream_ptr()) == rc
    assert word in lib.spo_last_error(), lib.spo_last_error()
    assert lib.spo_ma_trpo_grads_supported(net) == (1 if rc == -1 else 0) and lib.spo_ma_trpo_grads_scratch_floats(net, rows) == -1


@pytest.mark.parametrize("sharded", [False, True], ids=["host-driven", "sharded-form"])
def test_macpo_trainer_takes_the_fused_gradient_pair_when_asked(dev, monkeypatch, sharded):
    """MACPO_Trainer.trpo_update at obs 48 / hidden 128 / layer_N 1 / act 6 on 2 049 rows drawn from the host's generator, from the
    same start.  SPO_MA_GRADS_FUSED=1: the actor's net_backward raises, so the update can only pass on the fused pair.
    SPO_MA_GRADS_FUSED=0 and the default (the route is opt-in): net_trpo_grads raises, so the update is the loss + backward path as
    it was, and both give the same bits.  Both routes take the same case and accept the same step."""
    from safepo import _abi
    from safepo.common.model import _MAFlatNet
    from safepo.multi_agent.macpo import MACPO_Policy, MACPO_Trainer, default_cfg, mamujoco_cfg
    rows, D, A = 2049, 48, 6
    cfg = dict(default_cfg, **mamujoco_cfg)
    cfg.update(device=str(dev), macpo_sharded_form=sharded, cost_limit=1.0)
    backward = _MAFlatNet.net_backward

    def run(knob):
        monkeypatch.delenv("SPO_MA_GRADS_FUSED", raising=False) if knob is None else monkeypatch.setenv("SPO_MA_GRADS_FUSED", knob)
        torch.manual_seed(5)
        pol = MACPO_Policy(cfg, Sp(D), Sp(2 * D), Sp(A))
        tr = MACPO_Trainer(cfg, pol)
        g = torch.Generator().manual_seed(5)
        rn = lambda *s: torch.randn(*s, generator=g)
        obs, share = rn(rows, D), rn(rows, 2 * D)
        off, _ = _offsets(_abi.load(), pol.actor._net)
        mu, std = _mean_of(pol.actor.theta.detach().cpu(), obs, pol.actor._net, off), tr._std().cpu()
        act = mu + std * rn(rows, A)
        s = (share, obs, None, None, act, rn(rows, 1), rn(rows, 1) * 2, None, torch.ones(rows, 1), torch.distributions.Normal(mu, std).log_prob(act),
             rn(rows, 1), None, 0.5 + torch.rand(rows, 1, generator=g), rn(rows, 1), torch.rand(rows, 1, generator=g) * 3, None, rn(rows, 1),
             torch.tensor(0.7))

        def no_actor_backward(net, *a, **k):
            assert net is not pol.actor, "the fused route called the actor's net_backward"
            return backward(net, *a, **k)
        if knob == "1":
            monkeypatch.setattr(_MAFlatNet, "net_backward", no_actor_backward)
        else:
            monkeypatch.setattr(_MAFlatNet, "net_trpo_grads", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the old path called net_trpo_grads")))
        out = tr.trpo_update(tuple(u.to(dev) if torch.is_tensor(u) else u for u in s))
        monkeypatch.undo()
        return pol.actor.theta.clone(), out, dict(tr.last_step_info)
    (th1, out1, info1), (th0, out0, info0), (thd, outd, infod) = run("1"), run("0"), run(None)
    assert info1 == info0 == infod and info1["accepted_step"] >= 0, (info1, info0)
    assert torch.equal(th0, thd) and all(torch.equal(out0[i], outd[i]) for i in (2, 3, 6, 12))


def test_graph_capture_keeps_the_cycle_collector_off_and_puts_it_back(dev):
    """Inside _abi.graph_capture the collector is off, so no dead cycle that owns device objects is finalised while the stream
    captures; afterwards it is as it was, enabled or not."""
    import gc
    from safepo import _abi
    buf = torch.zeros(8, device=dev)
    for before in (True, False):
        gc.enable() if before else gc.disable()
        try:
            with _abi.graph_capture(torch.cuda.CUDAGraph(), capture_error_mode="thread_local"):
                inside = gc.isenabled()
                buf.add_(1.0)
            assert not inside and gc.isenabled() == before
        finally:
            gc.enable()
