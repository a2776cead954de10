"""Worker of tests/test_gpu_macpo_dp.py (not a test module), and the helpers that file shares with it.

Two ranks on ONE GPU (gloo for the host collectives), the way tests/ma_dp_worker.py runs MAPPO-L:

  golden <tag>   each rank holds 48 of the 96 rows of one case of tests/golden/ma_macpo.npz and takes two
                 MACPO_Trainer.trpo_update steps; rank 0 records what test_ma_macpo_trainer_vs_reference_golden records, so
                 the test can hold the sharded step to the same gate on the WHOLE 96 rows.
  train          each rank holds half of the rollout threads of a synthetic SeparatedReplayBuffer (T, N = 6, 8) and runs
                 MACPO_Trainer.train(); rank 0 also trains a single-rank trainer (the host-driven path) on the whole buffer."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "safe-policy-optimization_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "ma_macpo.npz")
ROW_NAMES = ("value_loss", "critic_grad_norm", "kl", "improve", "expected_improve", "cost_surrogate", "cost_grad_norm", "wrp", "lam",
             "nu", "b.b", "popart_mean", "popart_mean_sq", "popart_debias")
VECTORS = (("cost_grad", "b"), ("g_step_dir", "g_dir"), ("b_step_dir", "b_dir"), ("x", "x"))      # golden key, oracle record key


class Sp:
    def __init__(self, n):
        self.shape = (n,)


def golden_trainer(z, tag, dev, comm=None, lo=0, hi=None, **cfg_extra):
    """MACPO policy + trainer of golden case `tag` with the reference's initial parameters, and the rows [lo, hi) of its
    sample as the 18-tuple trpo_update takes."""
    from oracle import ma_restatement as MR
    from safepo.multi_agent.macpo import MACPO_Policy, MACPO_Trainer, default_cfg
    gc = MR.cfg_from_golden(z, tag)
    cfg = dict(default_cfg)
    cfg.update(device=str(dev), **gc)
    cfg.update(cfg_extra)
    for k in ("hidden_size", "layer_N", "searching_steps", "conjugate_gradient_iters"):
        cfg[k] = int(gc[k])
    s = MR.sample_from_golden(z, tag)
    rows = s["obs"].shape[0]
    D, S, A = s["obs"].shape[1], s["share_obs"].shape[1], s["actions"].shape[1]
    pol = MACPO_Policy(cfg, Sp(D), Sp(S), Sp(A))
    for nm, net in (("actor", pol.actor), ("critic", pol.critic), ("cost_critic", pol.cost_critic)):
        pre = f"{tag}_init_{nm}_"
        net.load_state_dict({k[len(pre):]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith(pre)})
    tr = MACPO_Trainer(cfg, pol, comm)
    part = {k: (v[lo:hi] if k != "aver_episode_costs" and v.dim() > 0 and v.shape[0] == rows else v) for k, v in s.items()}
    sample = (part["share_obs"], part["obs"], None, None, part["actions"], part["value_preds"], part["returns"], None,
              part["active_masks"], part["old_logp"], part["adv"], None, part["factor"], part["cost_preds"], part["cost_returns"],
              None, part["cost_adv"], part["aver_episode_costs"])
    sample = tuple(t.to(dev) if torch.is_tensor(t) else t for t in sample)
    return pol, tr, sample


def two_steps(pol, tr, sample):
    """Two trpo_update steps; everything test_ma_macpo_trainer_vs_reference_golden compares, as numpy arrays."""
    rec = {"rows": []}
    for it in range(2):
        r = tr.trpo_update(sample)
        (vl, cgn, kl, improve, expected, _ent, _ratio, cost_loss, cost_gn, wrp, _cp, _cr, bgrad, lam, nu, g_dir, b_dir, x, _mu,
         _std, bb) = r
        vn = tr.value_normalizer
        rec["rows"].append([float(vl), float(cgn), float(kl), float(improve), float(expected), float(cost_loss), float(cost_gn),
                            float(wrp), float(lam), float(nu), float(bb), float(vn.running_mean), float(vn.running_mean_sq),
                            float(vn.debiasing_term)])
        for got, (key, _k64) in zip((bgrad, g_dir, b_dir, x), VECTORS):
            rec[f"s{it}_{key}"] = got.cpu().numpy()
        rec[f"s{it}_actor_after"] = pol.actor.theta.cpu().numpy()
        rec[f"s{it}_case"] = np.asarray([tr.last_step_info["optim_case"], tr.last_step_info["accepted_step"]])
    rec["rows"] = np.asarray(rec["rows"], np.float64)
    rec["final_critic"], rec["final_cost_critic"] = pol.critic.theta.cpu().numpy(), pol.cost_critic.theta.cpu().numpy()
    return rec


def gate_against_golden(z, tag, rec):
    """The checks of test_ma_macpo_trainer_vs_reference_golden on a record of two_steps: every quantity within
    |HIP - f64| <= 3 |reference - f64| + floor (tests/ma_yardstick.py), the reference's own recorded fp32 result as the float32
    leg, the restatement in float64 as the yardstick, that test's floors."""
    import ma_yardstick as Y
    from oracle import ma_restatement as MR
    gc = MR.cfg_from_golden(z, tag)
    tr64, n64 = Y.oracle_trainer(gc, MR.nets_from_golden(z, tag), "macpo", torch.float64)
    s64 = Y.to_dtype(MR.sample_from_golden(z, tag), torch.float64)
    rows64 = []
    for it in range(2):
        rec64 = tr64.ppo_update(s64)
        rows64.append(rec64["row"])
        for key, k64 in VECTORS:
            d_hip, d_32 = Y.gate(rec[f"s{it}_{key}"], z[f"{tag}_s{it}_{key}"], rec64[k64].numpy(), 1e-5, f"{tag} step {it} {key}")
            print(f"macpo sharded {tag} step {it} {key}: max|hip-f64| {d_hip:.2e} vs |reference-f64| {d_32:.2e}")
        d_hip, d_32 = Y.gate(rec[f"s{it}_actor_after"], z[f"{tag}_s{it}_actor_after"], n64["actor"].flat().numpy(), 1e-5,
                             f"{tag} step {it} actor after")
        print(f"macpo sharded {tag} step {it} actor after: max|hip-f64| {d_hip:.2e} vs |reference-f64| {d_32:.2e}")
    rows, gold_rows, rows64 = rec["rows"], np.asarray(z[f"{tag}_steps"][:2], np.float64), np.asarray(rows64, np.float64)
    for c, nm in enumerate(ROW_NAMES):
        # improve / expected_improve / kl are differences of nearly equal numbers: their scale is the surrogate's, not their own
        sc = max(np.abs(rows64[:, c]).max(), np.abs(rows64[:, 5]).max()) if c in (2, 3, 4) else None
        d_hip, d_32 = Y.gate(rows[:, c], gold_rows[:, c], rows64[:, c], 1e-5, f"{tag} column {nm}", scale=sc)
        print(f"macpo sharded {tag} column {nm}: max|hip-f64| {d_hip:.2e} vs |reference-f64| {d_32:.2e}")
    for nm in ("critic", "cost_critic"):
        pre = f"{tag}_final_{nm}_"
        gold = np.concatenate([z[k].reshape(-1) for k in z.files if k.startswith(pre)])
        Y.gate(rec[f"final_{nm}"], gold, n64[nm].flat().numpy(), 1e-5, f"{tag} {nm} parameters")


def _replicas_identical(dist, world, tensors):
    flat = torch.cat([t.detach().reshape(-1).float().cpu() for t in tensors])
    gathered = [torch.empty_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat)
    return all(torch.equal(gathered[0], g) for g in gathered[1:])


def run_golden(comm, dev, out_path, tag):
    import torch.distributed as dist
    z = np.load(GOLDEN)
    rows = z[f"{tag}_obs"].shape[0]
    shard = rows // comm.world_size
    pol, tr, sample = golden_trainer(z, tag, dev, comm, comm.rank * shard, (comm.rank + 1) * shard)
    assert tr.sharded
    rec = two_steps(pol, tr, sample)
    same = _replicas_identical(dist, comm.world_size, [pol.actor.theta, pol.critic.theta, pol.cost_critic.theta, tr._popart_state])
    if comm.rank == 0:
        np.savez(out_path, replicas_identical=np.asarray(same), world=np.asarray(comm.world_size), **rec)


def run_train(comm, dev, out_path):
    import torch.distributed as dist
    from safepo import parallel as P
    from safepo.common.buffer import SeparatedReplayBuffer
    from safepo.multi_agent import macpo as M
    rank, world = comm.rank, comm.world_size
    T, N, D, S, A = 6, 8, 10, 14, 3
    cfg = dict(M.default_cfg)
    cfg.update(M.mamujoco_cfg)
    cfg.update(device=str(dev), hidden_size=32, episode_length=T, num_mini_batch=1, critic_lr=2e-3, cost_limit=1.0)
    g = torch.Generator().manual_seed(42)
    full = {"share_obs": torch.randn(T + 1, N, S, generator=g), "obs": torch.randn(T + 1, N, D, generator=g),
            "actions": torch.randn(T, N, A, generator=g), "action_log_probs": -1.0 + 0.1 * torch.randn(T, N, A, generator=g),
            "value_preds": torch.randn(T + 1, N, 1, generator=g), "cost_preds": torch.randn(T + 1, N, 1, generator=g),
            "returns": torch.randn(T + 1, N, 1, generator=g) * 2, "cost_returns": torch.rand(T + 1, N, 1, generator=g) * 3,
            "factor": torch.rand(T, N, 1, generator=g) + 0.5}

    def build(n_threads, lo, comm_):
        torch.manual_seed(3)
        c = dict(cfg, n_rollout_threads=n_threads)
        pol = M.MACPO_Policy(c, Sp(D), Sp(S), Sp(A))
        with torch.no_grad():
            for net in (pol.actor, pol.critic, pol.cost_critic):
                net.theta.add_(0.05 * torch.randn(net.theta.shape, generator=torch.Generator().manual_seed(9)).to(dev))
        tr = M.MACPO_Trainer(c, pol, comm_)
        buf = SeparatedReplayBuffer(c, Sp(D), Sp(S), Sp(A))
        for k, v in full.items():
            getattr(buf, k).copy_(v[:, lo:lo + n_threads])
        buf.active_masks.fill_(1.0)
        buf.aver_episode_costs = torch.tensor(0.7, device=dev)
        return pol, tr, buf
    shard = N // world
    pol, tr, buf = build(shard, rank * shard, comm)
    assert tr.sharded
    out = tr.train(buf, logger=None, perm_fn=lambda it: torch.arange(T * shard))
    nets = [pol.actor.theta, pol.critic.theta, pol.cost_critic.theta]
    res = {"world": world, "replicas_identical": _replicas_identical(dist, world, nets + [tr._popart_state])}
    if rank == 0:
        pol1, tr1, buf1 = build(N, 0, P.Comm.single())
        assert not tr1.sharded
        start = pol1.actor.theta.clone()
        out1 = tr1.train(buf1, logger=None, perm_fn=lambda it: torch.arange(T * N))
        got, ref = torch.cat(nets).cpu(), torch.cat([pol1.actor.theta, pol1.critic.theta, pol1.cost_critic.theta]).cpu()
        res["theta"], res["theta_single"] = got.tolist(), ref.tolist()
        res["popart"] = [tr._popart_state.tolist(), tr1._popart_state.tolist()]
        cols = (0, 1, 2, 3, 4, 7, 8)      # value loss, critic norm, kl, improve, expected improve, cost surrogate, cost critic norm
        res["scalars"] = [[float(out[k]) for k in cols], [float(out1[k]) for k in cols]]
        res["ratio_mean"] = [tr._ratio_mean, float(out1[6].mean())]
        res["step_info"] = [tr.last_step_info, tr1.last_step_info]
        res["actor_moved"] = float((pol1.actor.theta - start).abs().max())
        with open(out_path, "w") as f:
            json.dump(res, f)


def main(argv):
    import torch.distributed as dist
    from safepo import parallel as P
    comm = P.init_from_env(backend="gloo")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    if argv[2] == "golden":
        run_golden(comm, dev, argv[1], argv[3])
    else:
        run_train(comm, dev, argv[1])
    comm.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv)
