"""Command line of the single-agent scripts: same flags, defaults and types as the reference
`single_agent_args()` (safepo/utils/config.py:144-191).  Isaac Gym tasks are recognised by name
(isaac_gym_map) but need the isaacgym package, exactly like the reference."""
from __future__ import annotations

import argparse

isaac_gym_map = {
    "ShadowHandOver_Safe_finger": "shadow_hand_over_safe_finger",
    "ShadowHandOver_Safe_joint": "shadow_hand_over_safe_joint",
    "ShadowHandCatchOver2Underarm_Safe_finger": "shadow_hand_catch_over_2_underarm_safe_finger",
    "ShadowHandCatchOver2Underarm_Safe_joint": "shadow_hand_catch_over_2_underarm_safe_joint",
    "FreightFrankaCloseDrawer": "freight_franka_close_drawer",
    "FreightFrankaPickAndPlace": "freight_franka_pick_and_place",
}


def strtobool(val: str) -> int:
    """distutils.util.strtobool (removed in Python 3.12) -- same accepted spellings."""
    v = str(val).lower()
    if v in ("y", "yes", "t", "true", "on", "1"):
        return 1
    if v in ("n", "no", "f", "false", "off", "0"):
        return 0
    raise ValueError(f"invalid truth value {val!r}")


def _bool(x):
    return bool(strtobool(x))


SINGLE_AGENT_FLAGS = [
    ("--seed", int, 0, "Random seed"),
    ("--use-eval", _bool, False, "Use evaluation environment for testing"),
    ("--task", str, "SafetyPointGoal1-v0", "The task to run"),
    ("--num-envs", int, 10, "The number of parallel game environments"),
    ("--experiment", str, "single_agent_exp", "Experiment name"),
    ("--log-dir", str, "../runs", "directory to save agent logs"),
    ("--device", str, "cuda", "The device to run the model on (this build: a ROCm GPU; reference default cpu)"),
    ("--device-id", int, 0, "The device id to run the model on"),
    ("--write-terminal", _bool, True, "Toggles terminal logging"),
    ("--headless", _bool, False, "Toggles headless mode"),
    ("--total-steps", int, 10000000, "Total timesteps of the experiments"),
    ("--steps-per-epoch", int, 20000, "The number of steps to run in each environment per policy rollout"),
    ("--randomize", bool, False, "Wheather to randomize the environments' initial states"),
    ("--cost-limit", float, 25.0, "cost_lim"),
    ("--lagrangian-multiplier-init", float, 0.001, "initial value of lagrangian multiplier"),
    ("--lagrangian-multiplier-lr", float, 0.035, "learning rate of lagrangian multiplier"),
]


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="RL Policy")
    for name, typ, default, help_ in SINGLE_AGENT_FLAGS:
        parser.add_argument(name, type=typ, default=default, help=help_)
    return parser


def seed_list(args) -> list:
    """The seeds of this process: `--seeds` where given, else [--seed]."""
    seeds = getattr(args, "seeds", None)
    return [int(s) for s in seeds] if seeds else [int(args.seed)]


def fold_overrides(config: dict, args) -> dict:
    """A script's default_cfg with the command line's and the caller's overrides folded in: --hidden-sizes first, then
    args.cfg_override (set programmatically), which wins."""
    hidden = getattr(args, "hidden_sizes", None)
    if hidden is not None:
        config["hidden_sizes"] = [int(h) for h in hidden]
    config.update(getattr(args, "cfg_override", None) or {})
    return config


WIDE_ROWS_NOT_BUILT = ("--batch-wide-rows True is not available for {what}: the seed-batched row-group step is built for the clipped "
                       "surrogate of ppo_lag, ppo, pg and cppo_pid only; the KL-penalty loss of focops / cup and the wide critic fit of "
                       "the second-order scripts have no such form.  Run one process per seed")


KLPEN_ROWS_OTHER_SCRIPTS = ("--batch-klpen-rows True is not available for {what}: the seed-batched row-group KL-penalty step is the "
                            "FOCOPS / CUP step (focops, cup with --batch-update True)")


def refuse_seed_batch(args, what: str, hint: str = "") -> None:
    """For the scripts without a seed-batched form: more than one seed is an error, not a silent single run."""
    if len(seed_list(args)) > 1:
        raise SystemExit(f"--seeds with more than one seed is not available for {what}: the seed-batched update exists for the "
                         "PPO-Lagrangian family (ppo_lag, ppo, pg, cppo_pid) on the persistent kernels, one GPU; run one process per seed"
                         + hint)


def critic_seed_batch(args) -> bool:
    """The second-order scripts (cpo, pcpo, rcpo, trpo_lag, trpo, natural_pg): several seeds run in one process only with
    --batch-critic-fit True (their critic fits then share one launch per iteration); without it they are refused as ever."""
    if getattr(args, "batch_wide_rows", False):
        raise SystemExit(WIDE_ROWS_NOT_BUILT.format(what="the second-order scripts"))
    if getattr(args, "batch_klpen_rows", False):
        raise SystemExit(KLPEN_ROWS_OTHER_SCRIPTS.format(what="the second-order scripts"))
    if getattr(args, "batch_critic_fit_split", False) and not getattr(args, "batch_critic_fit", False):
        raise SystemExit("--batch-critic-fit-split True widens --batch-critic-fit True (65-128 observations, up to 32 seeds): give both")
    if getattr(args, "batch_critic_fit_feature_split", False) and not getattr(args, "batch_critic_fit", False):
        raise SystemExit("--batch-critic-fit-feature-split True widens --batch-critic-fit True (129-512 observations, up to 16 seeds): "
                         "give both")
    if len(seed_list(args)) <= 1:
        return False
    if not getattr(args, "batch_critic_fit", False):
        refuse_seed_batch(args, "the second-order scripts",
                          ".  (Opt in with --batch-critic-fit True: the seeds' critic fits then share one persistent launch.)")
    return True


# (quoted by --help here and in single_agent/benchmark.py; source: profiles/seed_batch_critic/step_times.txt)
CRITIC_BATCH_FIGURES = ("Measured at 60 / 8, 4096 x 128 rows, batch 128: one critic-fit step of ALL seeds takes 9.9 / 11.2 / 14.2 us at 8 / 16 / "
                        "24 seeds against 9.8 us per seed one after the other (7.9 x / 13.9 x / 16.5 x the aggregate step rate; one seed alone: "
                        "9.90 against 9.76 us, which is why one seed stays `--seed`); cpo's second epoch with 8 seeds: Time/Update 0.56 s "
                        "against 3.35 s (profiles/seed_batch_critic/step_times.txt).")


# (quoted by --help here and in single_agent/benchmark.py; source: profiles/seed_batch_critic_split/step_times.txt)
CRITIC_SPLIT_BATCH_FIGURES = ("Measured at 72 / 2, 4096 x 128 rows, batch 128, one GPU: one split critic-fit step of ALL seeds takes 18.3 / 18.5 / "
                              "19.4 us at 8 / 16 / 32 seeds against 15.7 us per seed one after the other (6.9 x / 13.6 x / 25.9 x the aggregate "
                              "step rate; one seed alone: 17.75 against 15.74 us, which is why one seed stays `--seed`); cpo's second epoch with "
                              "8 seeds at 72 observations: Time/Update 0.94 s against 5.34 s, one sample each "
                              "(profiles/seed_batch_critic_split/step_times.txt).")


# (quoted by --help here and in single_agent/benchmark.py; source: profiles/seed_batch_critic_ks/step_times.txt)
CRITIC_KS_BATCH_FIGURES = ("Measured at 376 / 17, 4096 x 128 rows, batch 128: one critic-fit step of ALL seeds takes 26.5 / 26.5 / 26.5 / 26.8 us at 2 / 4 / "
                           "8 / 16 seeds against 25.9 us per seed one after the other (1.95 x / 3.92 x / 7.81 x / 15.48 x the aggregate step rate; 16 "
                           "seeds, two per XCD, lose nothing measurable); one seed alone: 26.58 against 25.90 us, which is why one seed stays "
                           "`--seed`; 512 / 32 with 8 seeds: 26.66 us against 207.54 (7.79 x); the critic fit is 0.96 of a stand-alone run's "
                           "Time/Update at this shape; cpo's second epoch with 8 seeds at 376 / 17: Time/Update 1.45 s against 8.85 s, one "
                           "sample each (profiles/seed_batch_critic_ks/step_times.txt).")


# (quoted by --help here and in single_agent/benchmark.py; source: profiles/seed_batch_klpen/step_times.txt)
KLPEN_BATCH_FIGURES = ("Measured at 4096 x 128 rows, batch 64: one FOCOPS step of ALL seeds takes 12.7 / 12.9 / 13.0 us at 8 / 16 / 32 seeds (60 / 8) against "
                       "12.2 us per seed one after the other (7.6 x / 15.1 x / 30.0 x the aggregate step rate; 72 / 2 the same ratios; CUP's second "
                       "stage 7.7 x / 15.4 x / 30.7 x), no knee up to 32; one seed alone: 12.62 against 12.16 us, which is why one seed stays "
                       "`--seed` (profiles/seed_batch_klpen/step_times.txt).")


# (quoted by --help here and in single_agent/benchmark.py; source: profiles/seed_batch_ks/step_times.txt)
KS_BATCH_FIGURES = ("Measured at 376 / 17, 4096 x 128 rows, batch 64: one clipped-surrogate step of ALL seeds takes 16.4 / 16.5 / 16.6 us at 2 / 4 / 8 "
                    "seeds against 16.2 us per seed one after the other (1.98 x / 3.93 x / 7.81 x the aggregate step rate; the FOCOPS step 18.0 / 18.1 / "
                    "18.1 us against 17.8-17.9 per seed: 7.85 x at 8; CUP's second stage 7.81 x at 8); one seed alone: 16.49 against 16.23 us, which is "
                    "why one seed stays `--seed`; 192 / 8 with 16 seeds, two per XCD: 17.64 us against 274.96 (15.6 x); ppo_lag's second epoch with 8 "
                    "seeds at 376 / 17: Time/Update 3.06 s against 21.31 s, one sample each (profiles/seed_batch_ks/step_times.txt).")


# (quoted by --help here and in single_agent/benchmark.py; source: profiles/seed_batch_rows/step_times.txt)
ROWS_BATCH_FIGURES = ("Measured at 60 / 8, 4096 x 128 rows, batch 64: with hidden [128, 128] one step of ALL seeds takes 32.7 / 36.2 / 44.3 / "
                      "52.4 / 91.3 us at 2 / 4 / 8 / 16 / 32 seeds against 30.3 us per seed one after the other (1.87 x / 3.38 x / 5.55 x / "
                      "9.38 x / 10.84 x the aggregate step rate; the time per seed-step stops falling between 16 and 32 seeds, where 12 "
                      "gradient workgroups per seed pass the card's 256 CUs); with [256, 256] 68.0 / 76.9 / 100.1 / 138.5 / 267.3 us against "
                      "59.8 per seed (1.76 x / 3.11 x / 4.78 x / 6.90 x / 7.16 x: flat beyond 16); one seed alone: 30.82 against 30.28 us, "
                      "which is why one seed stays `--seed` (profiles/seed_batch_rows/step_times.txt).")


# (quoted by --help here and in single_agent/benchmark.py; source: profiles/seed_batch_klpen_rows/step_times.txt)
KLPEN_ROWS_BATCH_FIGURES = "Not measured (profiles/seed_batch_klpen_rows/step_times.txt)."


def single_agent_args(argv=None):
    """-> (args, cfg_env).  cfg_env is {} for non-Isaac tasks (reference config.py:172-191)."""
    parser = build_parser()
    # (not a reference flag, so not in build_parser's table) several independent runs in ONE process on one GPU
    parser.add_argument("--seeds", type=int, nargs="+", default=None,
                        help="seed-batched run (ppo_lag, ppo, pg, cppo_pid; focops and cup with --batch-update True): one env / policy / optimiser / logger per seed, each "
                             "the run `--seed` of that seed would be, their updates sharing one persistent launch (up to 32 seeds; "
                             "run r is placed on XCD r mod 8; one minibatch step of ALL seeds takes 7.8-7.9 us up to 16 seeds and 8.2 us at 32 "
                             "against 7.7 us for one seed alone at 60 / 8, profiles/seed_batch/step_times.txt).  Default: [--seed], the ordinary single run")
    parser.add_argument("--batch-critic-fit", type=_bool, default=False,
                        help="second-order scripts (cpo, pcpo, rcpo, trpo_lag, trpo, natural_pg) with --seeds: run the seeds in one "
                             "process, their critic fits sharing one persistent launch per iteration (up to 24 seeds, eight workgroups "
                             "each, run r on XCD r mod 8; hidden [64, 64], obs_dim <= 64), each seed the run its `--seed` would be.  "
                             + CRITIC_BATCH_FIGURES + "  Default False: several seeds are refused for these scripts")
    parser.add_argument("--batch-critic-fit-split", type=_bool, default=False,
                        help="with --batch-critic-fit True: also take tasks with 65-128 observations (hidden [64, 64]: the Ant / Car / "
                             "Doggo / Racecar navigation tasks), whose critic fit runs the two-replica split form -- the seeds' split "
                             "critic fits then share one persistent launch per iteration (spo_critic_fit_iter_split_multi: up to 32 "
                             "seeds, four workgroups each, run r on XCD r mod 8), each seed the run its `--seed` would be.  "
                             + CRITIC_SPLIT_BATCH_FIGURES + "  Default False: such tasks are refused with several seeds")
    parser.add_argument("--batch-critic-fit-feature-split", type=_bool, default=False,
                        help="with --batch-critic-fit True: also take tasks with 129-512 observations and up to 32 actions (hidden "
                             "[64, 64]: HumanoidVelocity's 376 / 17), whose critic fit runs on the feature-split kernel -- the seeds' "
                             "critic fits then share one launch per iteration (spo_critic_fit_iter_ks_multi: up to 16 seeds up to 384 "
                             "observations, 8 up to 512; 2 x ceil(obs_dim / 64) workgroups each, run r on XCD r mod 8), each seed the "
                             "run its `--seed` would be.  " + CRITIC_KS_BATCH_FIGURES
                             + "  Default False: such tasks are refused with several seeds")
    parser.add_argument("--batch-update", type=_bool, default=False,
                        help="focops and cup with --seeds: run the seeds in one process, their minibatch steps sharing one persistent "
                             "launch per pass (spo_update_iter_ex_multi: up to 32 seeds, one workgroup per network each, run r on XCD "
                             "r mod 8; hidden [64, 64], obs_dim <= 128, act_dim <= 16), each seed the run its `--seed` would be.  "
                             + KLPEN_BATCH_FIGURES + "  Default False: several seeds are refused for these scripts")
    parser.add_argument("--batch-wide-obs", type=_bool, default=False,
                        help="the six first-order scripts with --seeds (focops and cup: with --batch-update True as well): also take "
                             "shapes outside the persistent kernels but inside the feature-split kernel -- hidden [64, 64], up to 512 "
                             "observations / 32 actions, minibatches of up to 64 rows: HumanoidVelocity's 376 / 17 -- whose minibatch "
                             "steps then share one launch per pass (spo_update_iter_ex_ks_multi: up to 16 seeds up to 256 observations, "
                             "8 up to 512; 3 x ceil(obs_dim / 64) workgroups each, run r on XCD r mod 8), each seed the run its `--seed` "
                             "would be.  " + KS_BATCH_FIGURES + "  Default False: such tasks are refused with several seeds")
    parser.add_argument("--hidden-sizes", type=int, nargs="+", default=None,
                        help="widths of the hidden layers of all three networks (reference model.py:131), e.g. --hidden-sizes 128 128.  "
                             "Default: the script's default_cfg ([64, 64]: the persistent kernels).  Any other widths run on the "
                             "wide-network kernels; an args.cfg_override[\"hidden_sizes\"] set programmatically still wins")
    parser.add_argument("--batch-wide-rows", type=_bool, default=False,
                        help="ppo_lag, ppo, pg and cppo_pid with --seeds: also take shapes that step on the wide-network path's "
                             "row-group kernel -- hidden sizes other than [64, 64] (--hidden-sizes), more than 512 observations or more "
                             "than 32 actions, minibatches of up to 256 rows whose images fit one CU's LDS -- whose minibatch steps then "
                             "share the step's three launches (spo_wide_rows_step_multi: up to 32 seeds, run r a slice of the grid; no "
                             "per-XCD budget: no workgroup waits for another), each seed the run its `--seed` would be.  "
                             + ROWS_BATCH_FIGURES + "  Default False: such shapes are refused with several seeds; focops, cup and the "
                             "second-order scripts refuse the flag (not built)")
    parser.add_argument("--batch-klpen-rows", type=_bool, default=False,
                        help="focops and cup with --seeds and --batch-update True: also take shapes that step on the wide-network "
                             "path's row-group kernel -- hidden sizes other than [64, 64] (--hidden-sizes), more than 512 observations "
                             "or more than 32 actions, minibatches of up to 256 rows whose images and old distribution fit one CU's "
                             "LDS -- whose FOCOPS steps and both of CUP's stages then share the step's five launches "
                             "(spo_wide_rows_ex_step_multi: up to 32 seeds of one shape, run r a slice of each grid; world size 1; "
                             "graph-replayed passes only; no workgroup waits for another), each seed the run its `--seed` would be.  "
                             + KLPEN_ROWS_BATCH_FIGURES + "  Default False: such shapes are refused with several seeds; the other ten "
                             "scripts refuse the flag")
    args = parser.parse_args(argv)
    if args.task in isaac_gym_map:
        raise Exception("Please install isaacgym to run Isaac Gym tasks!")
    return args, {}


multi_agent_velocity_map = {
    "Safety2x4AntVelocity-v0": {"agent_conf": "2x4", "scenario": "Ant"},
    "Safety4x2AntVelocity-v0": {"agent_conf": "4x2", "scenario": "Ant"},
    "Safety2x3HalfCheetahVelocity-v0": {"agent_conf": "2x3", "scenario": "HalfCheetah"},
    "Safety6x1HalfCheetahVelocity-v0": {"agent_conf": "6x1", "scenario": "HalfCheetah"},
    "Safety3x1HopperVelocity-v0": {"agent_conf": "3x1", "scenario": "Hopper"},
    "Safety2x3Walker2dVelocity-v0": {"agent_conf": "2x3", "scenario": "Walker2d"},
    "Safety2x1SwimmerVelocity-v0": {"agent_conf": "2x1", "scenario": "Swimmer"},
    "Safety9|8HumanoidVelocity-v0": {"agent_conf": "9|8", "scenario": "Humanoid"},
}


multi_agent_goal_tasks = [f"Safety{robot}MultiGoal{level}-v0" for robot in ("Point", "Ant") for level in (0, 1, 2)]


def multi_agent_args(algo: str, argv=None):
    """CLI of the multi-agent scripts (reference safepo/utils/config.py:194-278): same flags; the training config
    starts from the algorithm's defaults (the reference's marl_cfg/<algo>/config.yaml, here a dict in the algorithm
    module), with the `mamujoco` overrides for MuJoCo-style tasks -- the Synth* tasks count as such."""
    import importlib
    import time
    p = argparse.ArgumentParser(description="RL Policy")
    p.add_argument("--use-eval", type=_bool, default=False)
    p.add_argument("--task", type=str, default="SynthMultiAgent-v0")
    p.add_argument("--agent-conf", type=str, default="2x4")
    p.add_argument("--scenario", type=str, default="Ant")
    p.add_argument("--experiment", type=str, default="Base")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--model-dir", type=str, default="")
    p.add_argument("--cost-limit", type=float, default=25.0)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--device-id", type=int, default=0)
    p.add_argument("--write-terminal", type=_bool, default=True)
    p.add_argument("--headless", type=_bool, default=False)
    p.add_argument("--total-steps", type=int, default=None)
    p.add_argument("--num-envs", type=int, default=None)
    p.add_argument("--randomize", type=bool, default=False)
    args = p.parse_args(argv)
    if args.task in isaac_gym_map:
        raise NotImplementedError("Isaac Gym tasks need the isaacgym package (not part of this build)")
    mod = importlib.import_module(f"safepo.multi_agent.{algo}")
    cfg_train = dict(mod.default_cfg)
    if args.task in multi_agent_velocity_map or args.task in multi_agent_goal_tasks or args.task.startswith("Synth"):
        cfg_train.update(mod.mamujoco_cfg)
        if args.task in multi_agent_velocity_map:
            args.agent_conf = multi_agent_velocity_map[args.task]["agent_conf"]
            args.scenario = multi_agent_velocity_map[args.task]["scenario"]
    cfg_train["use_eval"] = args.use_eval
    cfg_train["cost_limit"] = args.cost_limit
    cfg_train["algorithm_name"] = algo
    cfg_train["device"] = args.device + ":" + str(args.device_id)
    cfg_train["env_name"] = args.task
    cfg_train["seed"] = args.seed
    if args.total_steps:
        cfg_train["num_env_steps"] = args.total_steps
    if args.num_envs:
        cfg_train["n_rollout_threads"] = args.num_envs
        cfg_train["n_eval_rollout_threads"] = args.num_envs
    relpath = "-".join(["-".join(["seed", str(args.seed).zfill(3)]), time.strftime("%Y-%m-%d-%H-%M-%S")])
    cfg_train["log_dir"] = "../runs/" + args.experiment + "/" + args.task + "/" + algo + "/" + relpath
    return args, {}, cfg_train


def run_as_script(main, script_file):
    """The `if __name__ == "__main__":` block that every single-agent script of the reference repeats verbatim (e.g.
    ppo_lag.py:392-409): parse the reference's flags, build log_dir = <log_dir>/<experiment>/<task>/<algo>/seed-XXX-<time>, and run
    main() with stdout / stderr redirected into seed<N>_terminal.log / seed<N>_error.log unless --write-terminal is set."""
    import os
    import sys
    import time
    args, cfg_env = single_agent_args()
    stamp = time.strftime("%Y-%m-%d-%H-%M-%S")
    algo = os.path.basename(script_file).split(".")[0]
    seeds = seed_list(args)
    args.seed = seeds[0]                # (`--seeds s` alone is `--seed s`: the ordinary single run)
    if len(seeds) > 1:
        if len(set(seeds)) != len(seeds):
            raise SystemExit(f"--seeds {seeds}: the same seed twice would write one log directory twice")
        # every seed logs where its own `--seed` run would; --seed itself (terminal log, args.log_dir) is the first of them
        args.log_dirs = [os.path.join(args.log_dir, args.experiment, args.task, algo, "-".join(["seed", str(s).zfill(3), stamp]))
                         for s in seeds]
    relpath = stamp
    subfolder = "-".join(["seed", str(args.seed).zfill(3)])
    relpath = "-".join([subfolder, relpath])
    args.log_dir = os.path.join(args.log_dir, args.experiment, args.task, algo, relpath)
    if not args.write_terminal:
        os.makedirs(args.log_dir, exist_ok=True)
        with open(os.path.join(args.log_dir, f"seed{args.seed}_terminal.log"), "w", encoding="utf-8") as f_out, \
                open(os.path.join(args.log_dir, f"seed{args.seed}_error.log"), "w", encoding="utf-8") as f_err:
            sys.stdout, sys.stderr = f_out, f_err
            return main(args, cfg_env)
    return main(args, cfg_env)
