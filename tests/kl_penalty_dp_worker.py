"""Worker of tests/test_gpu_dp_kl_penalty.py (not a test module): two ranks on ONE GPU (gloo for the host collectives) run the
data-parallel FOCOPS / CUP minibatch steps (PPOLagEngine._learning_iter_ex_split) and rank 0 replays the same global minibatches
through the CPU oracle (oracle/restatement.KLPenaltyUpdater), or (mode e2e_*) the scripts' main() runs under the two ranks.

argv: out_path use_p2p shape mode dp_batch
  mode focops: one pass of FOCOPS steps; rank 0's old means put no row over target_kl, rank 1's about half of them, so the
               fraction of rows inside the bound differs between the ranks and the global minibatch;
  mode cup:    one pass of CUP's first stage (clipped surrogate, the actor's optimiser clock ahead of the critics'), then one pass
               of its actor-only second stage;
  mode e2e_focops / e2e_cup: safepo.single_agent.{focops,cup}.main on SynthSafe-v0."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "safe-policy-optimization_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def shard(rank: int, M: int, D: int, A: int):
    g = torch.Generator().manual_seed(9876 + rank)
    obs, act = torch.randn(M, D, generator=g), torch.randn(M, A, generator=g)
    logp = -A * 0.9 - 0.5 * (act ** 2).sum(-1) + 0.1 * torch.randn(M, generator=g)
    tgt_r, tgt_c = torch.randn(M, generator=g), torch.rand(M, generator=g)
    adv, adv_c = torch.randn(M, generator=g), torch.randn(M, generator=g)
    perms = [torch.randperm(M, generator=g) for _ in range(2)]
    return obs, act, logp, tgt_r, tgt_c, adv, adv_c, perms


def kl_offsets(rank: int, M: int, A: int, target_kl: float) -> torch.Tensor:
    """Per-row KL(new || old) the old means are set up with: rank 0 none over the bound, rank 1 every other row at 3x it."""
    small = torch.full((M,), 0.0)
    if rank == 0:
        return small
    return torch.where(torch.arange(M) % 2 == 0, torch.tensor(3.0 * target_kl), small)


def gather_cpu(t: torch.Tensor, world: int):
    t = t.detach().cpu().contiguous()
    out = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return out


def e2e(out_path: str, algo: str, rank: int, world: int):
    import argparse
    import csv
    import importlib
    mod = importlib.import_module(f"safepo.single_agent.{algo}")
    log_dir = os.path.join(os.path.dirname(out_path), f"e2e_{algo}", "task", "run")
    args = argparse.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=8, experiment="t", log_dir=log_dir,
                              device="cuda", device_id=0, write_terminal=True, headless=False, total_steps=2 * 8 * 32,
                              steps_per_epoch=8 * 32, randomize=False, cost_limit=0.5, lagrangian_multiplier_init=0.001,
                              lagrangian_multiplier_lr=0.035, cfg_override={"learning_iters": 2},
                              env_kwargs={"trunc_len": 8, "p_cost": 0.5})
    os.environ["LOCAL_RANK"] = "0"                 # both ranks on cuda:0
    ret = mod.main(args, {})
    res = {"world": world, "engine": type(ret["engine"]).__name__}
    if rank == 0:
        rows = list(csv.DictReader(open(os.path.join(log_dir, "progress.csv"))))
        cfg = json.load(open(os.path.join(log_dir, "config.json")))
        res.update(rows=len(rows), stop_iter=all("Train/StopIter" in r for r in rows),
                   second_stage=all("Train/SeconStageStopIter" in r for r in rows), gradient_exchange=cfg.get("gradient_exchange"))
    g = gather_cpu(ret["policy"].theta, world)
    res["replicas_identical"] = all(torch.equal(g[0], x) for x in g[1:])
    return res


def main(out_path: str, use_p2p: str, shape: str = "60,8,64,64", mode: str = "focops", dp_batch: str = "global",
         local_rows: str = "64"):
    from safepo import parallel as P
    os.environ["SPO_P2P"] = use_p2p
    if use_p2p == "1":
        os.environ["SPO_P2P_AUTOTUNE"] = "0"       # keep the peer regions (the auto-tune may release them for the RCCL form)
    comm = P.init_from_env(backend="gloo")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    rank, world = comm.rank, comm.world_size
    if mode.startswith("e2e_"):
        res = e2e(out_path, mode[4:], rank, world)
        if rank == 0:
            with open(out_path, "w") as f:
                json.dump(res, f)
        comm.barrier()
        dist.destroy_process_group()
        return

    from safepo import _abi
    from safepo.common.engine import PPOLagEngine, WidePPOLagEngine
    from safepo.common.model import ActorVCritic
    dims = [int(v) for v in shape.split(",")]
    D, A, hidden = dims[0], dims[1], dims[2:]
    GB = 64 if dp_batch == "global" else int(local_rows) * world       # global minibatch
    lb = GB // world
    M = max(512, 8 * lb)
    target_kl = 0.1 * A
    cfg = {"hidden_sizes": hidden, "gamma": 0.99, "target_kl": target_kl, "batch_size": GB if dp_batch == "global" else lb,
           "learning_iters": 1, "max_grad_norm": 40.0, "dp_batch": dp_batch}
    obs, act, logp, tgt_r, tgt_c, adv, adv_c, perms = shard(rank, M, D, A)
    torch.manual_seed(7)
    pol = ActorVCritic(D, A, hidden_sizes=hidden).to(dev)
    state0 = {k: v.detach().cpu().clone() for k, v in pol.state_dict().items()}
    eng = (PPOLagEngine if pol.kernels_supported("ppo") else WidePPOLagEngine)(pol, 1, M, cfg, dev, comm=comm)
    assert eng._cfg_struct().batch == lb
    b = eng.buffer
    b.data["obs"].copy_(obs.view(1, M, D)); b.data["act"].copy_(act.view(1, M, A))
    b.data["log_prob"].copy_(logp.view(1, M)); b.data["target_value_r"].copy_(tgt_r.view(1, M))
    b.data["target_value_c"].copy_(tgt_c.view(1, M)); b.adv_mix.copy_(adv.view(1, M)); b.data["adv_c"].copy_(adv_c.view(1, M))
    res = {"world": world, "in_kernel_exchange": eng.p2p is not None, "local_batch": lb, "steps": M // lb,
           "engine": type(eng).__name__}
    off = pol.log_std_offset
    nu, gamma = 0.7, cfg["gamma"]
    coef = (1 - gamma * 0.95) / (1 - gamma)
    if mode == "focops":
        eng.snapshot_old_distribution()
        std = eng.std_old.detach()
        kl = kl_offsets(rank, M, A, target_kl).to(dev)
        eng.mean_old += std[None, :] * torch.sqrt(2.0 * kl / A)[:, None]
        losses = eng.learning_iter_ex(perms[0].to(torch.int32).to(dev), b.adv_mix, _abi.ACTOR_LOSS_KL_PENALTY, target_kl, 1.0 / 1.5)
        res["clocks"] = [eng.adam_step, eng.adam_step_actor_extra]
        old_means = gather_cpu(eng.mean_old, world)
        old_std = eng.std_old.detach().cpu()
    else:
        eng.adam_step_actor_extra = 5                  # the actor's optimiser 5 steps ahead (as after earlier second stages)
        losses = eng.learning_iter_ex(perms[0].to(torch.int32).to(dev), b.adv_mix, _abi.ACTOR_LOSS_CLIP)
        eng.snapshot_old_distribution()
        theta_mid = pol.theta.detach().cpu().clone()
        clocks_mid = [eng.adam_step, eng.adam_step_actor_extra]
        losses2 = eng.learning_iter_ex(perms[1].to(torch.int32).to(dev), b.data["adv_c"], _abi.ACTOR_LOSS_KL_PENALTY,
                                       float("inf"), -nu * coef, True)
        th_end = pol.theta.detach().cpu()
        res["critics_unchanged_stage2"] = bool(torch.equal(theta_mid[:off], th_end[:off]))
        res["clocks"] = [clocks_mid, [eng.adam_step, eng.adam_step_actor_extra]]
        old_means = gather_cpu(eng.mean_old, world)
        old_std = eng.std_old.detach().cpu()
    eng.check_sync_error()
    theta = pol.theta.detach().cpu()
    gathered = gather_cpu(theta, world)
    res["replicas_identical"] = all(torch.equal(gathered[0], x) for x in gathered[1:])
    if rank == 0:
        from oracle import restatement as R          # checker only
        ref = R.OraclePolicy(D, A, hidden_sizes=tuple(hidden))
        ref.load_state_dict(state0)
        th0 = R.flat_params(ref).numpy().copy()
        upd = R.KLPenaltyUpdater(ref, epochs=1, max_grad_norm=cfg["max_grad_norm"])
        shards = [shard(r, M, D, A) for r in range(world)]

        def batch(s, it, cols):
            parts = [[sh[c][sh[7][it][s * lb:(s + 1) * lb]] for c in cols] for sh in shards]
            return [torch.cat([p[i] for p in parts], 0) for i in range(len(cols))]

        def batch_old(s, it):
            return torch.cat([old_means[r][shards[r][7][it][s * lb:(s + 1) * lb]] for r in range(world)], 0)

        ref_losses, f_local_differs, kl_margin = [], False, float("inf")
        if mode == "focops":
            for s in range(M // lb):
                ob, ac, lp, tr, tc, ad = batch(s, 0, (0, 1, 2, 3, 4, 5))
                om = batch_old(s, 0)
                with torch.no_grad():
                    d_ = ref.actor(ob)
                    klr = torch.distributions.kl_divergence(d_, torch.distributions.Normal(om, old_std)).sum(-1)
                kl_margin = min(kl_margin, float((klr - target_kl).abs().min() / target_kl))
                ind = (klr <= target_kl).float()
                f_loc = [float(ind[r * lb:(r + 1) * lb].mean()) for r in range(world)]
                f_local_differs |= any(abs(f - float(ind.mean())) > 1e-6 for f in f_loc)
                ref_losses.append(upd.focops_step(ob, ac, lp, tr, tc, ad, om, old_std, target_kl))
            got_l = losses.cpu().numpy()
        else:
            # the oracle's actor optimiser 5 steps ahead with zero moments, as the engine's clock
            for prm in ref.actor.parameters():
                upd.opt_a.state[prm] = {"step": torch.tensor(5.0), "exp_avg": torch.zeros_like(prm),
                                        "exp_avg_sq": torch.zeros_like(prm)}
            for s in range(M // lb):
                ref_losses.append(upd.minibatch_step(*batch(s, 0, (0, 1, 2, 3, 4, 5))))
            th_mid_ref = R.flat_params(ref).numpy().copy()
            res["stage1_theta_max_abs_diff"] = float(np.abs(theta_mid.numpy() - th_mid_ref).max())
            ref2 = []
            for s in range(M // lb):
                ob, ac, lp, ac_ = batch(s, 1, (0, 1, 2, 6))
                ref2.append(upd.cup_second_stage_step(ob, ac, lp, ac_, batch_old(s, 1), old_std, nu, gamma))
            got_l = np.concatenate([losses.cpu().numpy().reshape(-1), losses2[:, 2].cpu().numpy()])
            ref_losses = list(np.asarray(ref_losses).reshape(-1)) + ref2
        ref_l = np.asarray(ref_losses, dtype=np.float64).reshape(got_l.shape)
        th_ref = R.flat_params(ref).numpy()
        got = theta.numpy()
        res["f_local_differs"] = f_local_differs
        res["kl_margin"] = kl_margin
        res["loss_max_rel_diff"] = float(np.max(np.abs(got_l - ref_l) / (np.abs(ref_l) + 1e-6)))
        # the same difference against the size of each loss column (rms over the steps): the actor's loss is a mean of
        # random-sign ratio*adv terms and passes near 0, where the element-wise ratio measures only the forward pass's rounding
        cols = got_l.reshape(-1, 3) if mode == "focops" else None
        if cols is not None:
            refc = ref_l.reshape(-1, 3)
            rms = np.sqrt(np.mean(refc ** 2, axis=0))
            res["loss_max_scaled_diff"] = float(np.max(np.abs(cols - refc) / (rms + 1e-6)))
            res["loss_max_rel_diff_by_column"] = [float(v) for v in np.max(np.abs(cols - refc) / (np.abs(refc) + 1e-6), axis=0)]
        d = np.abs(got - th_ref)
        res["theta_max_abs_diff"] = float(d.max())
        res["theta_frac_outside"] = float(np.mean(d > 2e-6 + 3e-4 * np.abs(th_ref)))
        res["theta_moved"] = float(np.abs(th_ref - th0).max())
        with open(out_path, "w") as f:
            json.dump(res, f)
    comm.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(*sys.argv[1:])
