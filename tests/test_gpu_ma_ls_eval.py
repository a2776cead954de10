"""The fused line-search candidate evaluation of the multi-agent actor (spo_ma_ls_eval, csrc/ma_ls_eval.hip) on the GPU against a
plain torch network + the reference's Normal.log_prob, ratio, surrogates and kl_divergence, in float32 and float64, under the
project's rule |hip - f64| <= 3 |f32 - f64| + 1e-6 * scale (tests/fp64_gate.py)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_ma_fvp import Sp, _mean_of, _offsets, _problem, dev  # noqa: E402,F401  (the actor and its torch restatement)

pytestmark = pytest.mark.gpu
KINDS = ("sum ratio*factor*adv", "sum ratio*factor*cost_adv", "sum KL_row", "sum ratio")
MEMBERS = {k: [] for k in KINDS}          # filled by the cases, gated as groups by the test after them
GUARD = 64


def _oracle(theta, x, t, net, off, xc, yc, dtype):
    """-> the four row sums, the sums of the absolute row terms, the ratio rows."""
    theta, x = theta.detach().cpu().to(dtype), x.detach().cpu().to(dtype)
    act, old_logp, adv, cadv, factor, mu_old, std_old = (v.detach().cpu().to(dtype) for v in t)
    mu = _mean_of(theta, x, net, off)
    std = torch.sigmoid(theta[off(6):off(6) + net.out_dim] / xc) * yc
    ratio = torch.prod(torch.exp(torch.distributions.Normal(mu, std).log_prob(act) - old_logp), dim=-1)
    kl = (torch.log(std_old) - torch.log(std) + (std_old.pow(2) + (mu_old - mu).pow(2)) / (1e-8 + 2.0 * std.pow(2)) - 0.5).sum(1)
    terms = torch.stack([ratio * factor * adv, ratio * factor * cadv, kl, ratio])
    return terms.sum(1).double().numpy(), terms.abs().sum(1).double().numpy(), ratio.double().numpy()


def _inputs(actor, off, x, seed):
    """mu_old / std_old / old_logp of theta_old (float32 on the host), act ~ N(mu_old, std_old), then theta <- the candidate."""
    g = torch.Generator().manual_seed(seed)
    rows, O, dv = x.shape[0], actor.act_dim, x.device
    th = actor.theta.detach().cpu()
    mu_old = _mean_of(th, x.cpu(), actor._net, off)
    std_old = torch.sigmoid(th[off(6):off(6) + O] / actor.std_x_coef) * actor.std_y_coef
    act = mu_old + std_old * torch.randn(rows, O, generator=g)
    old_logp = torch.distributions.Normal(mu_old, std_old).log_prob(act)
    v = torch.randn(th.numel(), generator=g)
    t = (act, old_logp, torch.randn(rows, generator=g), torch.randn(rows, generator=g), 0.5 + torch.rand(rows, generator=g), mu_old, std_old)
    actor.theta.copy_((th - 0.02 * v / v.norm()).to(dv))
    return tuple(u.contiguous().to(dv) for u in t)


def _call(actor, x, t, poison):
    from safepo import _abi
    rows = x.shape[0]
    sums = torch.full((4,), float("nan"), dtype=torch.float64, device=x.device)
    buf = torch.full((rows + 2 * GUARD,), 123.0, device=x.device)
    buf[GUARD:GUARD + rows] = float("nan")
    ws = torch.full((_abi.MA_LS_WS_DOUBLES,), poison, dtype=torch.float64, device=x.device)
    actor.net_ls_eval(x, *t, sums, buf[GUARD:GUARD + rows], ws)
    return sums.cpu(), buf.cpu()


BASE = dict(D=48, H=128, NB=2, O=6, rows=33)
CASES = [BASE] + [dict(BASE, **{k: v}) for k, vs in (("rows", (1, 31, 32, 8225)), ("H", (65, 64, 20)), ("D", (1, 128)), ("O", (1, 16)),
                                                       ("NB", (1,))) for v in vs]


@pytest.mark.parametrize("c", CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_ma_ls_eval_vs_torch_under_the_fp64_gate(dev, c):
    """One axis varied at a time around (48, 128, 2 blocks, 6, 33 rows): the chunk edge and the masked tail (1, 31, 32, 33 rows), a
    second trip through the chunk loop of the capped grid (8 225 = 256 x 32 + 33), full / ragged / at-most-four-tile hidden
    widths, in_dim 1 / 48 / 128, out_dim 1 / 6 / 16, one block.  The ratio rows are gated here, the four sums by the group test
    below (a single scalar's |f32 - f64| can be 0 by chance)."""
    import fp64_gate as G
    actor, lib, off, _, x, *_ = _problem(dev, c["D"], c["H"], c["NB"], c["O"], c["rows"])
    assert actor.ls_eval_supported()
    t = _inputs(actor, off, x, 7 + c["rows"])
    sums, buf = _call(actor, x, t, float("nan"))
    with G.on_oracle_threads():
        (s32, _, r32), (s64, a64, r64) = (_oracle(actor.theta, x, t, actor._net, off, actor.std_x_coef, actor.std_y_coef, dt)
                                          for dt in (torch.float32, torch.float64))
    assert (buf[:GUARD] == 123.0).all() and (buf[GUARD + c["rows"]:] == 123.0).all()
    G.gate(buf[GUARD:GUARD + c["rows"]].numpy(), r32, r64, f"ma_ls_eval ratio {c}")
    for k, kind in enumerate(KINDS):
        MEMBERS[kind].append((float(sums[k]), s32[k], s64[k], a64[k]))


@pytest.mark.parametrize("kind", KINDS)
def test_ma_ls_eval_sums_as_groups_over_the_cases(dev, kind):
    import fp64_gate as G
    assert len(MEMBERS[kind]) == len(CASES), "run after the cases above (same module, file order)"
    G.gate_group(MEMBERS[kind], f"ma_ls_eval {kind}")


def test_ma_ls_eval_repeats_are_bit_identical(dev):
    """Two calls at 8 225 rows, partial_ws poisoned differently in between: the same 32 + 4 * rows bytes."""
    actor, lib, off, _, x, *_ = _problem(dev, 48, 128, 2, 6, 8225)
    t = _inputs(actor, off, x, 3)
    (s0, b0), (s1, b1) = _call(actor, x, t, float("nan")), _call(actor, x, t, -7.0)
    assert torch.equal(s0, s1) and torch.equal(b0, b1) and torch.isfinite(s0).all() and torch.isfinite(b0).all()


@pytest.mark.parametrize("sharded", [False, True], ids=["host-driven", "sharded-form"])
def test_macpo_trainer_takes_the_fused_evaluation_when_asked(dev, monkeypatch, sharded):
    """MACPO_Trainer.trpo_update at obs 48 / hidden 128 / layer_N 1 / act 6 on 2 049 rows drawn from the host's generator, from
    the same start: SPO_MA_LS_FUSED=1 (the route is opt-in) and SPO_MA_LS_FUSED=0 take the same case and accept the same step;
    kl, loss_improve and the ratio of the fused route are gated against the float64 restatement of the accepted candidate (kl
    at the scale of its terms' magnitudes, loss_improve -- a difference of nearly equal surrogates -- at the surrogate's); and
    with the knob off the result is, bit for bit, that of the default routing in a run in which net_ls_eval raises."""
    import fp64_gate as G
    from safepo import _abi
    from safepo.common.model import _MAFlatNet
    from safepo.multi_agent.macpo import MACPO_Policy, MACPO_Trainer, default_cfg, mamujoco_cfg
    rows, D, A = 2049, 48, 6
    cfg = dict(default_cfg, **mamujoco_cfg)
    cfg.update(device=str(dev), macpo_sharded_form=sharded, cost_limit=1.0)

    def run(knob, broken=False):
        monkeypatch.delenv("SPO_MA_LS_FUSED", raising=False) if knob is None else monkeypatch.setenv("SPO_MA_LS_FUSED", knob)
        torch.manual_seed(5)
        pol = MACPO_Policy(cfg, Sp(D), Sp(2 * D), Sp(A))
        tr = MACPO_Trainer(cfg, pol)
        g = torch.Generator().manual_seed(5)
        rn = lambda *s: torch.randn(*s, generator=g)
        obs, share = rn(rows, D), rn(rows, 2 * D)
        th_old = pol.actor.theta.detach().cpu()
        off, _ = _offsets(_abi.load(), pol.actor._net)
        mu, std = _mean_of(th_old, obs, pol.actor._net, off), tr._std().cpu()
        act = mu + std * rn(rows, A)
        s = (share, obs, None, None, act, rn(rows, 1), rn(rows, 1) * 2, None, torch.ones(rows, 1), torch.distributions.Normal(mu, std).log_prob(act),
             rn(rows, 1), None, 0.5 + torch.rand(rows, 1, generator=g), rn(rows, 1), torch.rand(rows, 1, generator=g) * 3, None, rn(rows, 1),
             torch.tensor(0.7))
        if broken:
            monkeypatch.setattr(_MAFlatNet, "net_ls_eval", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the old path called net_ls_eval")))
        out = tr.trpo_update(tuple(u.to(dev) if torch.is_tensor(u) else u for u in s))
        monkeypatch.undo()
        return pol, off, th_old, s, out, dict(tr.last_step_info)
    pol, off, th_old, s, out, info = run("1")
    (p0, _, _, _, out0, info0), (p0b, _, _, _, out0b, info0b) = run("0"), run(None, broken=True)
    assert not torch.equal(out[6], out0[6])          # two routes: another summation order shows in the ratio's last bits
    assert info == info0 == info0b and info["accepted_step"] >= 0, (info, info0)
    assert all(torch.equal(out0[i], out0b[i]) for i in (2, 3, 6)) and torch.equal(p0.actor.theta, p0b.actor.theta)
    net = pol.actor._net
    t = (s[4], s[9], s[10].reshape(-1), s[16].reshape(-1), s[12].reshape(-1))
    res = {}
    with G.on_oracle_threads():
        for dt in (torch.float32, torch.float64):
            old = _mean_of(th_old.to(dt), s[1].to(dt), net, off)
            so = torch.sigmoid(th_old[off(6):off(6) + A].to(dt) / pol.actor.std_x_coef) * pol.actor.std_y_coef
            new, mag, ratio = _oracle(pol.actor.theta, s[1], t + (old, so), net, off, pol.actor.std_x_coef, pol.actor.std_y_coef, dt)
            before, _, _ = _oracle(th_old, s[1], t + (old, so), net, off, pol.actor.std_x_coef, pol.actor.std_y_coef, dt)
            kl_mag = 2 * torch.log(so).abs().sum().item() + A          # sum_d |log s_old| + |log s| + quot + 0.5 at s ~ s_old, quot ~ 0.5
            res[dt] = (new[2] / rows, (-new[0] + before[0]) / rows, ratio, kl_mag, mag[0] / rows)
    (kl32, im32, r32, _, _), (kl64, im64, r64, kl_scale, surr_scale) = res[torch.float32], res[torch.float64]
    G.gate(float(out[2]), kl32, kl64, "trpo_update kl", scale=kl_scale)
    G.gate(float(out[3]), im32, im64, "trpo_update loss_improve", scale=surr_scale)
    G.gate(out[6].reshape(-1).cpu().numpy(), r32, r64, "trpo_update ratio")
