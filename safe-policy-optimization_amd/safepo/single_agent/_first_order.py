"""Shared driver of the first-order single-agent scripts (ppo_lag, ppo, pg, cppo_pid).

The reference keeps one near-identical copy of this loop per script (SURVEY.md section 2 rows 6 and 8:
ppo.py drops the Lagrange multiplier, `advantage = data["adv_r"]` (ppo.py:272); pg.py additionally drops
the ratio clip (pg.py:309); cppo_pid.py swaps Lagrange for PIDLagrangian (cppo_pid.py:39)).  Here the
variants are parameters of one loop over the same HIP kernels:
    multiplier = "adam" | "pid" | None       clip = 0.2 | None (no clipping)
The epoch structure follows safepo/single_agent/ppo_lag.py:159-386.
"""
from __future__ import annotations

import os
import random
import time

import numpy as np
import torch

from safepo import _abi
from safepo.common.engine import PPOLagEngine, WidePPOLagEngine
from safepo.common.env import make_sa_mujoco_env
from safepo.common.lagrange import Lagrange, PIDLagrangian
from safepo.common.logger import EpochLogger
from safepo.common.model import ActorVCritic
from safepo.parallel import dp_epoch_stat, init_from_env, require_equal_shards, shard_envs
from safepo.utils.config import KLPEN_ROWS_OTHER_SCRIPTS, WIDE_ROWS_NOT_BUILT, fold_overrides, isaac_gym_map, refuse_seed_batch, seed_list

NO_CLIP = 1e30      # clamp(ratio, 1-1e30, 1+1e30) is the identity: pg's unclipped surrogate on the same kernel


def _to_dev(x, dev):
    return torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x, dtype=torch.float32, device=dev).contiguous()


FOCOPS_LAM, FOCOPS_NU = 1.50, 2.00     # focops.py:44-45
CUP_LAMBDA, CUP_NU = 0.95, 0.20        # cup.py:44-45


def _eval_episodes(policy, eval_env, n_episodes: int, device):
    """Deterministic-policy episodes on the single eval env (ppo_lag.py:237-269) -> (returns, costs, lengths)."""
    eval_rews, eval_costs, eval_lens = [], [], []
    for _ in range(n_episodes):
        eval_obs, _ = eval_env.reset()
        eval_obs = _to_dev(eval_obs, device).reshape(1, -1)
        eval_rew, eval_cost, eval_len, eval_done = 0.0, 0.0, 0.0, False
        while not eval_done:
            act, _, _, _ = policy.step(eval_obs, deterministic=True)
            a_in = act if getattr(eval_env, "is_device_env", False) else act.detach().cpu().numpy()
            nobs, rew, cst, term, trunc, _ = eval_env.step(a_in)
            eval_rew += float(np.asarray(rew.cpu() if torch.is_tensor(rew) else rew).reshape(-1)[0])
            eval_cost += float(np.asarray(cst.cpu() if torch.is_tensor(cst) else cst).reshape(-1)[0])
            eval_len += 1
            t0 = np.asarray(term.cpu() if torch.is_tensor(term) else term).reshape(-1)[0]
            t1 = np.asarray(trunc.cpu() if torch.is_tensor(trunc) else trunc).reshape(-1)[0]
            eval_done = bool(t0) or bool(t1)
            eval_obs = _to_dev(nobs, device).reshape(1, -1)
        eval_rews.append(eval_rew); eval_costs.append(eval_cost); eval_lens.append(eval_len)
    return eval_rews, eval_costs, eval_lens


def _log_epoch(logger, args, out, variant, lagrange, epoch, next_lr, engine, env, is_root, *, t_rollout, t_eval, t_update, t_total):
    """The epoch's row of progress.csv (ppo_lag.py:351-386)."""
    if not logger.logged:
        logger.log_tabular("Metrics/EpRet")
        logger.log_tabular("Metrics/EpCost")
        logger.log_tabular("Metrics/EpLen")
        if args.use_eval:
            logger.log_tabular("Metrics/EvalEpRet")
            logger.log_tabular("Metrics/EvalEpCost")
            logger.log_tabular("Metrics/EvalEpLen")
        logger.log_tabular("Train/Epoch", epoch + 1)
        logger.log_tabular("Train/TotalSteps", (epoch + 1) * args.steps_per_epoch)
        logger.log_tabular("Train/StopIter", out["stop_iter"])
        if variant == "cup":
            logger.log_tabular("Train/SeconStageStopIter", out["second_stage_stop_iter"])   # (sic) cup.py:419
        logger.log_tabular("Train/KL", out["kl"])
        if lagrange is not None:
            logger.log_tabular("Train/LagragianMultiplier", lagrange.lagrangian_multiplier)
        logger.log_tabular("Train/LR", next_lr)
        logger.log_tabular("Loss/Loss_reward_critic")
        logger.log_tabular("Loss/Loss_cost_critic")
        logger.log_tabular("Loss/Loss_actor")
        logger.log_tabular("Time/Rollout", t_rollout)
        if args.use_eval:
            logger.log_tabular("Time/Eval", t_eval)
        logger.log_tabular("Time/Update", t_update)
        logger.log_tabular("Time/Total", t_total)
        stats = engine.buffer.stats.cpu()
        d = engine.buffer.data
        logger.log_tabular("Value/RewardAdv", d["adv_r"].mean().item())
        logger.log_tabular("Value/CostAdv", d["adv_c"].mean().item())
        logger.dump_tabular()
        if is_root and ((epoch + 1) % 100 == 0 or epoch == 0):
            logger.torch_save(itr=epoch)
            logger.save_state(state_dict={"Normalizer": getattr(env, "obs_rms", None)}, itr=epoch)
    else:
        logger.epoch_dict["Loss/Loss_reward_critic"] = []
        logger.epoch_dict["Loss/Loss_cost_critic"] = []
        logger.epoch_dict["Loss/Loss_actor"] = []
        for k in ("Metrics/EvalEpRet", "Metrics/EvalEpCost", "Metrics/EvalEpLen"):
            if k in logger.epoch_dict:
                logger.epoch_dict[k] = []


def run(args, cfg_env, default_cfg: dict, multiplier: str | None = "adam", clip: float | None = 0.2,
        variant: str = "ppo"):
    """variant: "ppo" (clipped surrogate family), "focops" (focops.py:279-367) or "cup" (cup.py:279-405)."""
    if variant != "ppo" and getattr(args, "batch_wide_obs", False) and not getattr(args, "batch_update", False):
        raise SystemExit("--batch-wide-obs True widens --batch-update True for focops and cup (hidden [64, 64], up to 512 observations "
                         "/ 32 actions: HumanoidVelocity): give both")
    if variant != "ppo" and getattr(args, "batch_wide_rows", False):
        raise SystemExit(WIDE_ROWS_NOT_BUILT.format(what="focops and cup"))
    if getattr(args, "batch_klpen_rows", False):
        if variant == "ppo":
            raise SystemExit(KLPEN_ROWS_OTHER_SCRIPTS.format(what="ppo_lag, ppo, pg and cppo_pid (their row-group step is shared with "
                                                                  "--batch-wide-rows True)"))
        if not getattr(args, "batch_update", False):
            raise SystemExit("--batch-klpen-rows True widens --batch-update True for focops and cup (shapes on the wide-network path's "
                             "row-group kernel: hidden sizes other than [64, 64], more than 512 observations or more than 32 actions): "
                             "give both")
    if len(seed_list(args)) > 1:
        if variant != "ppo" and not getattr(args, "batch_update", False):
            refuse_seed_batch(args, "focops and cup",
                              ".  (Opt in with --batch-update True: the seeds' minibatch steps then share one persistent launch.)")
        return run_seed_batch(args, cfg_env, default_cfg, multiplier, clip, variant)
    args.seed = seed_list(args)[0]      # (`--seeds s` alone is `--seed s`)
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if args.device == "cpu":
        raise RuntimeError("this build runs the PPO-Lagrangian hot path on a ROCm GPU only (--device cuda); "
                           "there is no CPU fallback")
    comm = init_from_env()
    local_rank = int(os.environ.get("LOCAL_RANK", args.device_id))
    device = torch.device(f"cuda:{local_rank if comm.world_size > 1 else args.device_id}")
    torch.cuda.set_device(device)
    if args.task in isaac_gym_map:
        raise NotImplementedError("Isaac Gym tasks (isaac_gym_specific_cfg) are not part of this build")
    config = dict(default_cfg)
    fold_overrides(config, args)
    config = {k: v for k, v in config.items() if v is not None}      # an override of None drops the key (e.g. batch_size,
    config["clip"] = NO_CLIP if clip is None else clip              # so that num_mini_batch decides as in isaac_gym_specific_cfg)

    require_equal_shards(args.num_envs, comm)
    _, n_local = shard_envs(args.num_envs, comm)
    env, obs_space, act_space = make_sa_mujoco_env(num_envs=n_local, env_id=args.task,
                                                   seed=args.seed + 1000 * comm.rank, device=device,
                                                   **(getattr(args, "env_kwargs", None) or {}))
    device_env = getattr(env, "is_device_env", False)
    eval_env = None
    if args.use_eval:
        eval_env, _, _ = make_sa_mujoco_env(num_envs=1, env_id=args.task, seed=None, device=device,
                                            **(getattr(args, "env_kwargs", None) or {}))

    steps_per_epoch = config.get("steps_per_epoch", args.steps_per_epoch)
    total_steps = config.get("total_steps", args.total_steps)
    local_steps_per_epoch = steps_per_epoch // args.num_envs
    epochs = total_steps // steps_per_epoch

    policy = ActorVCritic(obs_dim=obs_space.shape[0], act_dim=act_space.shape[0],
                          hidden_sizes=config["hidden_sizes"]).to(device)
    comm.broadcast_(policy.theta, 0)            # identical replicas
    # inside the persistent kernels' envelope (hidden_sizes [64, 64], obs_dim <= 128, act_dim <= 16 -- default_cfg on most tasks):
    # LDS-resident kernels; any other width / dims (HumanoidVelocity: 376 / 17): the wide-network kernels, all variants
    if policy.kernels_supported():
        engine = PPOLagEngine(policy, n_local, local_steps_per_epoch, config, device, comm=comm, lr=3e-4)
    else:
        engine = WidePPOLagEngine(policy, n_local, local_steps_per_epoch, config, device, comm=comm, lr=3e-4)
    if multiplier == "adam":
        upper = {"focops": FOCOPS_NU, "cup": CUP_NU}.get(variant)          # focops.py:136, cup.py:136
        lagrange = Lagrange(cost_limit=args.cost_limit, lagrangian_multiplier_init=args.lagrangian_multiplier_init,
                            lagrangian_multiplier_lr=args.lagrangian_multiplier_lr, lagrangian_upper_bound=upper)
    elif multiplier == "pid":
        lagrange = PIDLagrangian(cost_limit=args.cost_limit, lagrangian_multiplier_init=args.lagrangian_multiplier_init)
    else:
        lagrange = None

    dict_args = dict(vars(args))
    dict_args.update(config)
    if comm.world_size > 1:
        # which form of the per-minibatch gradient exchange this data-parallel run uses (it decides the order the ranks' gradients
        # are added in, hence the bits of a seeded run): recorded with the run
        tab = getattr(engine, "exchange_autotune", None)
        dict_args["gradient_exchange"] = (tab or {}).get("chosen") or ("in-kernel, default policy" if getattr(engine, "p2p", None) is not None
                                                                        else "kernel / all-reduce / kernel")
        if variant in ("focops", "cup"):             # (PPOLagEngine._learning_iter_ex_split, WidePPOLagEngine._minibatch_step_ex_split)
            dict_args["gradient_exchange"] = "kernel / all-reduce / kernel (split KL-penalty gradient)"
    is_root = comm.rank == 0
    log_dir = args.log_dir if is_root else os.path.join(args.log_dir, f"rank{comm.rank}")
    logger = EpochLogger(log_dir=log_dir, seed=str(args.seed), verbose=is_root)
    logger.save_config(dict_args)
    logger.setup_torch_saver(policy.actor)
    logger.log("Start with training.")

    # device envs that normalise observations hand the normaliser over: statistics merge + normalisation then run inside
    # the collect kernel (spo_policy_step_norm), one pass over the raw observations
    rms = env.fuse_normalize(True) if hasattr(env, "fuse_normalize") else None
    obs, _ = env.reset()
    obs = _to_dev(obs, device)
    timings = []
    for epoch in range(epochs):
        rollout_start_time = time.time()
        # ---- collect (ppo_lag.py:162-234): no host sync inside the loop for device envs
        obs = engine.rollout_epoch(env, obs, rms=rms)      # (one HIP-graph replay for capturable device envs)
        engine.drain_episode_events(logger)
        torch.cuda.synchronize(device)
        rollout_end_time = time.time()

        # ---- evaluation episodes (ppo_lag.py:237-269): deterministic policy on the single eval env.
        # (The reference steps `env` instead of `eval_env` inside this loop, which only works for
        #  --num-envs 1; the eval env is stepped here.)
        if args.use_eval:
            eval_rews, eval_costs, eval_lens = _eval_episodes(policy, eval_env, 1 if epoch < epochs - 1 else 10, device)
            logger.store(**{"Metrics/EvalEpRet": np.mean(eval_rews), "Metrics/EvalEpCost": np.mean(eval_costs),
                            "Metrics/EvalEpLen": np.mean(eval_lens)})
        torch.cuda.synchronize(device)
        eval_end_time = time.time()

        # ---- Lagrange multiplier (ppo_lag.py:271-273); EpCost mean is all-reduced over shards
        ep_costs = dp_epoch_stat(comm, logger, "Metrics/EpCost", device)
        if lagrange is not None:
            lagrange.update_lagrange_multiplier(ep_costs)
        # lambda == 0 makes (adv_r - 0*adv_c)/(0+1) == adv_r exactly: ppo / pg (ppo.py:272)
        lam = lagrange.lagrangian_multiplier if lagrange is not None else 0.0

        # ---- policy update (ppo_lag.py:275-350)
        engine.lr_factor = 1.0 - epoch / epochs if epochs > 0 else 1.0      # LinearLR(1 -> 0, total_iters=epochs)
        if variant == "focops":
            out = engine.update_focops(lam, focops_lam=FOCOPS_LAM)
        elif variant == "cup":
            out = engine.update_cup(lam, cup_lambda=CUP_LAMBDA)
        else:
            out = engine.update(lam)
        torch.cuda.synchronize(device)
        update_end_time = time.time()
        next_lr = 3e-4 * (1.0 - min(epoch + 1, epochs) / epochs)
        logger.store(**{"Loss/Loss_reward_critic": out["loss_r"], "Loss/Loss_cost_critic": out["loss_c"],
                        "Loss/Loss_actor": out["loss_pi"]})
        timings.append((rollout_end_time - rollout_start_time, update_end_time - eval_end_time))
        _log_epoch(logger, args, out, variant, lagrange, epoch, next_lr, engine, env, is_root,
                   t_rollout=rollout_end_time - rollout_start_time, t_eval=eval_end_time - rollout_end_time,
                   t_update=update_end_time - eval_end_time, t_total=update_end_time - rollout_start_time)
    logger.close()
    return {"timings": timings, "policy": policy, "engine": engine}


def _ks_shape_ok(obs_dim: int, act_dim: int, config: dict, rows: int) -> bool:
    """Would a one-GPU WidePPOLagEngine of this shape and config step on the feature-split kernel (its _feature_split_kernel_ok,
    answered before an engine exists)?"""
    batch = config.get("batch_size", max(rows // config.get("num_mini_batch", 1), 1))
    return os.environ.get("SPO_WIDE_KS", "1") != "0" and bool(_abi.load().spo_ks_supported(int(obs_dim), int(act_dim), int(batch)))


def _require_rows_batch(obs_dim: int, act_dim: int, config: dict, rows: int, n_seeds: int) -> None:
    """--batch-wide-rows True: SystemExit naming the limit unless `n_seeds` one-GPU WidePPOLagEngines of this shape and config
    would step as one seed-batched row-group launch (PPOLagEngineGroup._rows_batched, answered before an engine exists)."""
    lib = _abi.load()
    hidden = [int(h) for h in config["hidden_sizes"]]
    batch = int(config.get("batch_size", max(rows // config.get("num_mini_batch", 1), 1)))
    shape = f"{obs_dim} observations / {act_dim} actions, hidden_sizes {hidden}, minibatches of {batch} rows"
    if n_seeds > _abi.WIDE_ROWS_MAX_REPLICAS:
        raise SystemExit(f"--seeds: at most {_abi.WIDE_ROWS_MAX_REPLICAS} seeds share the row-group step's launches "
                         f"(--batch-wide-rows True), got {n_seeds}")
    if not 1 <= act_dim <= _abi.WIDE_MAX_ACT or not 1 <= len(hidden) <= 4:
        raise SystemExit(f"--batch-wide-rows True: {shape} is outside the wide-network path (act_dim <= {_abi.WIDE_MAX_ACT}, up to four "
                         "hidden layers)")
    net_c, net_a = _abi.MlpNet.of([obs_dim] + hidden + [1]), _abi.MlpNet.of([obs_dim] + hidden + [act_dim])
    if not lib.spo_wide_rows_multi_supported(net_c, net_a, batch, n_seeds):
        raise SystemExit(f"--batch-wide-rows True: {shape} does not fit the row-group kernel (at most 256 rows per minibatch, every "
                         "level's images of a 16-row group within one CU's 160 KB of LDS; SPO_WIDE_ROWS not 0): one process per seed")
    if os.environ.get("SPO_WIDE_ROWS_FUSED", "1") == "0":
        raise SystemExit("--batch-wide-rows True needs the fused optimiser of the row-group step (SPO_WIDE_ROWS_FUSED=0 is set)")
    graph_max = int(os.environ.get("SPO_WIDE_GRAPH_MAX_BATCH", "2048"))
    if not (0 < batch <= graph_max and (rows + batch - 1) // batch > 2):
        raise SystemExit(f"--batch-wide-rows True: {shape} over {rows} rows is not a graph-replayed pass (more than two minibatches of "
                         f"at most SPO_WIDE_GRAPH_MAX_BATCH = {graph_max} rows): nothing to share, one process per seed")


def _require_klpen_rows_batch(obs_dim: int, act_dim: int, config: dict, rows: int, n_seeds: int, variant: str) -> None:
    """--batch-klpen-rows True: SystemExit naming the limit unless `n_seeds` one-GPU WidePPOLagEngines of this shape and config
    would step FOCOPS' passes (variant "focops") or both of CUP's stages (variant "cup") as seed-batched row-group launches
    (PPOLagEngineGroup._rows_batched_ex, answered before an engine exists)."""
    lib = _abi.load()
    hidden = [int(h) for h in config["hidden_sizes"]]
    batch = int(config.get("batch_size", max(rows // config.get("num_mini_batch", 1), 1)))
    shape = f"{obs_dim} observations / {act_dim} actions, hidden_sizes {hidden}, minibatches of {batch} rows"
    if n_seeds > _abi.WIDE_ROWS_MAX_REPLICAS:
        raise SystemExit(f"--seeds: at most {_abi.WIDE_ROWS_MAX_REPLICAS} seeds share the row-group KL-penalty step's launches "
                         f"(--batch-klpen-rows True), got {n_seeds}")
    if not 1 <= act_dim <= _abi.WIDE_MAX_ACT or not 1 <= len(hidden) <= 4:
        raise SystemExit(f"--batch-klpen-rows True: {shape} is outside the wide-network path (act_dim <= {_abi.WIDE_MAX_ACT}, up to four "
                         "hidden layers)")
    net_c, net_a = _abi.MlpNet.of([obs_dim] + hidden + [1]), _abi.MlpNet.of([obs_dim] + hidden + [act_dim])
    kinds = [(_abi.ACTOR_LOSS_KL_PENALTY, 0)] if variant == "focops" else [(_abi.ACTOR_LOSS_CLIP, 0), (_abi.ACTOR_LOSS_KL_PENALTY, 1)]
    if not all(lib.spo_wide_rows_ex_multi_supported(net_c, net_a, batch, loss, actor_only, n_seeds) for loss, actor_only in kinds):
        raise SystemExit(f"--batch-klpen-rows True: {shape} does not fit the row-group kernel's KL-penalty form (at most 256 rows per "
                         "minibatch; every level's images of a 16-row group AND the rows' old distribution within one CU's 160 KB of "
                         "LDS; SPO_WIDE_ROWS not 0): one process per seed")
    graph_max = int(os.environ.get("SPO_WIDE_GRAPH_MAX_BATCH", "2048"))
    if not (0 < batch <= graph_max and (rows + batch - 1) // batch > 2):
        raise SystemExit(f"--batch-klpen-rows True: {shape} over {rows} rows is not a graph-replayed pass (more than two minibatches of "
                         f"at most SPO_WIDE_GRAPH_MAX_BATCH = {graph_max} rows): nothing to share, one process per seed")


class _SeedRun:
    """One run of a seed-batched process: what run() holds in local variables, per seed."""


def run_seed_batch(args, cfg_env, default_cfg: dict, multiplier: str | None, clip: float | None, variant: str = "ppo"):
    """`--seeds s0 s1 ...`: run() for several seeds in one process on one GPU (variant "focops" / "cup": with --batch-update True).  Every seed has its own env, policy, engine,
    multiplier and logger (in the log directory its own `--seed` run would write) and draws every random number from its own
    generator state (ReplicaRNG), so each is the stand-alone run of its seed; rollout, evaluation, multiplier update and logging
    run seed by seed, the update runs through PPOLagEngineGroup -- the seeds' minibatch steps in one persistent launch.  The
    Time/ columns hold the wall time of the phase for ALL seeds of the process."""
    from safepo.common.engine_group import PPOLagEngineGroup, ReplicaRNG
    seeds = seed_list(args)
    if len(set(seeds)) != len(seeds):
        raise SystemExit(f"--seeds {seeds}: the same seed twice")
    if args.device == "cpu":
        raise RuntimeError("this build runs the PPO-Lagrangian hot path on a ROCm GPU only (--device cuda); "
                           "there is no CPU fallback")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--seeds with more than one seed does not combine with torchrun (data-parallel runs): one GPU per process")
    device = torch.device(f"cuda:{args.device_id}")
    torch.cuda.set_device(device)
    if args.task in isaac_gym_map:
        raise NotImplementedError("Isaac Gym tasks (isaac_gym_specific_cfg) are not part of this build")
    config = dict(default_cfg)
    fold_overrides(config, args)
    config = {k: v for k, v in config.items() if v is not None}
    config["clip"] = NO_CLIP if clip is None else clip
    log_dirs = getattr(args, "log_dirs", None) or [os.path.join(args.log_dir, "-".join(["seed", str(s).zfill(3)])) for s in seeds]
    if len(log_dirs) != len(seeds):
        raise ValueError("args.log_dirs: one directory per seed")
    env_kwargs = getattr(args, "env_kwargs", None) or {}
    steps_per_epoch = config.get("steps_per_epoch", args.steps_per_epoch)
    total_steps = config.get("total_steps", args.total_steps)
    local_steps_per_epoch = steps_per_epoch // args.num_envs
    epochs = total_steps // steps_per_epoch

    wide_obs = bool(getattr(args, "batch_wide_obs", False))
    wide_rows = bool(getattr(args, "batch_wide_rows", False))
    klpen_rows = variant != "ppo" and bool(getattr(args, "batch_klpen_rows", False))
    if wide_obs and list(config["hidden_sizes"]) == [64, 64] and len(seeds) > _abi.KS_MAX_REPLICAS:
        raise SystemExit(f"--seeds: at most {_abi.KS_MAX_REPLICAS} seeds share a launch with --batch-wide-obs True (8 above 256 "
                         f"observations), got {len(seeds)}")
    runs = []
    for seed, log_dir in zip(seeds, log_dirs):
        r = _SeedRun()
        r.seed, r.rng = seed, ReplicaRNG(seed, device)
        with r.rng:                                   # the order of run(): env, eval env, policy, ..., reset
            r.env, obs_space, act_space = make_sa_mujoco_env(num_envs=args.num_envs, env_id=args.task, seed=seed, device=device,
                                                             **env_kwargs)
            r.eval_env = None
            if args.use_eval:
                r.eval_env, _, _ = make_sa_mujoco_env(num_envs=1, env_id=args.task, seed=None, device=device, **env_kwargs)
            r.policy = ActorVCritic(obs_dim=obs_space.shape[0], act_dim=act_space.shape[0],
                                    hidden_sizes=config["hidden_sizes"]).to(device)
            if r.policy.kernels_supported():
                r.engine = PPOLagEngine(r.policy, args.num_envs, local_steps_per_epoch, config, device, lr=3e-4)
            elif wide_obs and list(config["hidden_sizes"]) == [64, 64] and _ks_shape_ok(obs_space.shape[0], act_space.shape[0], config,
                                                                                         args.num_envs * local_steps_per_epoch):
                # --batch-wide-obs True: the feature-split kernel's shapes (up to 512 observations / 32 actions, HumanoidVelocity's
                # 376 / 17) -- WidePPOLagEngines, whose minibatch steps share one spo_update_iter_ex_ks_multi launch.  The seed cap
                # depends on the observation count, which only the (first) environment tells: checked before anything is logged
                D, A = obs_space.shape[0], act_space.shape[0]
                lib = _abi.load()
                if not lib.spo_update_ks_multi_supported(D, A, 1, len(seeds)):
                    cap = max(n for n in range(1, _abi.KS_MAX_REPLICAS + 1) if lib.spo_update_ks_multi_supported(D, A, 1, n))
                    raise SystemExit(f"--seeds: at most {cap} seeds share the feature-split kernel's launch at {D} observations "
                                     f"(--batch-wide-obs True: {_abi.KS_MAX_REPLICAS} up to 256 observations, 8 up to 512), got {len(seeds)}")
                r.engine = WidePPOLagEngine(r.policy, args.num_envs, local_steps_per_epoch, config, device, lr=3e-4)
            elif wide_rows and not (list(config["hidden_sizes"]) == [64, 64] and _ks_shape_ok(
                    obs_space.shape[0], act_space.shape[0], config, args.num_envs * local_steps_per_epoch)):
                # --batch-wide-rows True: the shapes WidePPOLagEngine steps through the row-group kernel (csrc/mlp_rows.hip) --
                # WidePPOLagEngines, whose minibatch steps share the three launches of spo_wide_rows_step_multi.  Whether the shape and
                # the seed count fit is known once the (first) environment tells the dims: checked before anything is logged
                _require_rows_batch(obs_space.shape[0], act_space.shape[0], config, args.num_envs * local_steps_per_epoch, len(seeds))
                r.engine = WidePPOLagEngine(r.policy, args.num_envs, local_steps_per_epoch, config, device, lr=3e-4)
            elif klpen_rows and not (list(config["hidden_sizes"]) == [64, 64] and _ks_shape_ok(
                    obs_space.shape[0], act_space.shape[0], config, args.num_envs * local_steps_per_epoch)):
                # --batch-klpen-rows True (focops, cup): the same shapes, whose FOCOPS / CUP steps share the five launches of
                # spo_wide_rows_ex_step_multi.  Checked before anything is logged, as above
                _require_klpen_rows_batch(obs_space.shape[0], act_space.shape[0], config, args.num_envs * local_steps_per_epoch,
                                          len(seeds), variant)
                r.engine = WidePPOLagEngine(r.policy, args.num_envs, local_steps_per_epoch, config, device, lr=3e-4)
            else:
                raise SystemExit(f"--seeds with more than one seed needs the persistent kernels' shapes (hidden_sizes [64, 64], obs_dim <= "
                                 f"128, act_dim <= 16); {args.task} with hidden_sizes {config['hidden_sizes']} runs on the wide-network "
                                 "kernels: one process per seed")
            if multiplier == "adam":
                upper = {"focops": FOCOPS_NU, "cup": CUP_NU}.get(variant)          # focops.py:136, cup.py:136
                r.lagrange = Lagrange(cost_limit=args.cost_limit, lagrangian_multiplier_init=args.lagrangian_multiplier_init,
                                      lagrangian_multiplier_lr=args.lagrangian_multiplier_lr, lagrangian_upper_bound=upper)
            elif multiplier == "pid":
                r.lagrange = PIDLagrangian(cost_limit=args.cost_limit, lagrangian_multiplier_init=args.lagrangian_multiplier_init)
            else:
                r.lagrange = None
            dict_args = dict(vars(args))
            dict_args.update(config)
            dict_args.update(seed=seed, log_dir=log_dir)          # (what the stand-alone run of this seed records)
            r.logger = EpochLogger(log_dir=log_dir, seed=str(seed), verbose=True)
            r.logger.save_config(dict_args)
            r.logger.setup_torch_saver(r.policy.actor)
            r.logger.log("Start with training.")
            r.rms = r.env.fuse_normalize(True) if hasattr(r.env, "fuse_normalize") else None
            obs, _ = r.env.reset()
            r.obs = _to_dev(obs, device)
        runs.append(r)
    group = (PPOLagEngineGroup([r.engine for r in runs], rngs=[r.rng for r in runs], klpen_rows=True) if klpen_rows
             else PPOLagEngineGroup([r.engine for r in runs], rngs=[r.rng for r in runs]))

    timings = []
    for epoch in range(epochs):
        rollout_start_time = time.time()
        for r in runs:
            with r.rng:
                r.obs = r.engine.rollout_epoch(r.env, r.obs, rms=r.rms)
            r.engine.drain_episode_events(r.logger)
        torch.cuda.synchronize(device)
        rollout_end_time = time.time()
        if args.use_eval:
            for r in runs:
                with r.rng:
                    rews, costs, lens = _eval_episodes(r.policy, r.eval_env, 1 if epoch < epochs - 1 else 10, device)
                r.logger.store(**{"Metrics/EvalEpRet": np.mean(rews), "Metrics/EvalEpCost": np.mean(costs),
                                  "Metrics/EvalEpLen": np.mean(lens)})
        torch.cuda.synchronize(device)
        eval_end_time = time.time()
        lams = []
        for r in runs:
            ep_costs = float(r.logger.get_stats("Metrics/EpCost"))
            if r.lagrange is not None:
                r.lagrange.update_lagrange_multiplier(ep_costs)
            lams.append(r.lagrange.lagrangian_multiplier if r.lagrange is not None else 0.0)
            r.engine.lr_factor = 1.0 - epoch / epochs if epochs > 0 else 1.0
        if variant == "focops":                        # (the shuffles are drawn under the runs' generator states)
            outs = group.update_focops(lams, focops_lam=FOCOPS_LAM)
        elif variant == "cup":
            outs = group.update_cup(lams, cup_lambda=CUP_LAMBDA)
        else:
            outs = group.update(lams)
        torch.cuda.synchronize(device)
        update_end_time = time.time()
        next_lr = 3e-4 * (1.0 - min(epoch + 1, epochs) / epochs)
        timings.append((rollout_end_time - rollout_start_time, update_end_time - eval_end_time))
        for r, out in zip(runs, outs):
            r.logger.store(**{"Loss/Loss_reward_critic": out["loss_r"], "Loss/Loss_cost_critic": out["loss_c"],
                              "Loss/Loss_actor": out["loss_pi"]})
            _log_epoch(r.logger, args, out, variant, r.lagrange, epoch, next_lr, r.engine, r.env, True,
                       t_rollout=rollout_end_time - rollout_start_time, t_eval=eval_end_time - rollout_end_time,
                       t_update=update_end_time - eval_end_time, t_total=update_end_time - rollout_start_time)
    for r in runs:
        r.logger.close()
    return {"timings": timings, "policies": [r.policy for r in runs], "engines": [r.engine for r in runs], "group": group,
            "policy": runs[0].policy, "engine": runs[0].engine}
