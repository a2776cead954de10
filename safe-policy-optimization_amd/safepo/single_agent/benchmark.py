"""Sweep launcher of the single-agent scripts: reference safepo/single_agent/benchmark.py (same flags; one
`python <algo>.py --task ... --seed ... --write-terminal False --experiment ... --total-steps ... --num-envs ...
--steps-per-epoch ...` subprocess per (seed, task, algo), `--workers` at a time).

MI355X specifics: every run is a whole-GPU job (persistent kernels), so runs are dealt round-robin over the visible GPUs
through `--device-id`, and `--workers` defaults to one per GPU.  `--workers 0` only prints the commands.
`--seeds-per-run K` (not a reference flag; default 1 = one subprocess per seed, as the reference) puts up to K seeds of one
(task, algorithm) into ONE subprocess through the scripts' `--seeds`: their updates share one persistent launch (ppo_lag,
cppo_pid -- and ppo / pg -- on the persistent kernels' shapes); the other algorithms, and HumanoidVelocity, keep one subprocess
per seed.  `--batch-second-order` (default off) lets cpo / pcpo / rcpo / trpo_lag / trpo / natural_pg join that grouping on
the tasks whose observations fit the persistent CPO kernels (at most 24 seeds per subprocess), with `--batch-critic-fit True`
on those commands: their critic fits share one persistent launch per iteration; `--batch-second-order-wide-obs` (default off,
needs `--batch-second-order`) adds the Ant / Car / Doggo / Racecar navigation tasks (65-128 observations, up to 32 seeds per
subprocess, `--batch-critic-fit True --batch-critic-fit-split True`).  `--batch-focops-cup` (default off) does the
same for focops / cup with `--batch-update True` (up to 32 seeds per subprocess): their minibatch steps share one persistent launch
per pass.  `--batch-wide-obs` (default off) also groups HumanoidVelocity (376 / 17: the feature-split kernel) for ppo_lag / ppo /
pg / cppo_pid -- and, with `--batch-focops-cup`, for focops / cup -- at most 8 seeds per subprocess, `--batch-wide-obs True` on
those commands.
"""
from __future__ import annotations

import argparse
import os
import shlex
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

from safepo.utils.config import CRITIC_KS_BATCH_FIGURES, CRITIC_SPLIT_BATCH_FIGURES, KLPEN_BATCH_FIGURES, KLPEN_ROWS_BATCH_FIGURES, KS_BATCH_FIGURES, ROWS_BATCH_FIGURES

HERE = os.path.dirname(os.path.abspath(__file__))
ALGOS = ["pcpo", "ppo_lag", "cup", "focops", "rcpo", "trpo_lag", "cpo", "cppo_pid"]
NAVI_TASKS = [f"Safety{robot}{task}{level}-v0" for level in (1, 2) for robot in ("Ant", "Car", "Doggo", "Point", "Racecar")
              for task in ("Button", "Circle", "Goal", "Push")]
VEL_TASKS = [f"Safety{robot}Velocity-v1" for robot in ("Ant", "HalfCheetah", "Hopper", "Walker2d", "Swimmer", "Humanoid")]


def visible_gpus() -> int:
    try:
        import torch
        return max(torch.cuda.device_count(), 1)
    except Exception:  # noqa: BLE001 -- the launcher itself needs no GPU
        return 1


def default_tasks():
    try:
        import safety_gymnasium  # noqa: F401
        return NAVI_TASKS + VEL_TASKS
    except ImportError:
        return ["SynthSafe-v0"]           # no simulator in this image: the synthetic device env


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--tasks", nargs="+", default=default_tasks(), help="the ids of the environment to benchmark")
    p.add_argument("--algo", nargs="+", default=ALGOS, help="the ids of the algorithm to benchmark")
    p.add_argument("--num-seeds", type=int, default=3, help="the number of random seeds")
    p.add_argument("--start-seed", type=int, default=0, help="the number of the starting seed")
    p.add_argument("--workers", type=int, default=None, help="concurrent runs (default: one per visible GPU)")
    p.add_argument("--experiment", type=str, default="benchmark", help="name of the experiment")
    p.add_argument("--total-steps", type=int, default=10000000, help="total number of steps")
    p.add_argument("--num-envs", type=int, default=10, help="number of environments to run in parallel")
    p.add_argument("--steps-per-epoch", type=int, default=20000, help="number of steps per epoch")
    p.add_argument("--seeds-per-run", type=int, default=1,
                   help="seeds of one (task, algorithm) per subprocess (--seeds of the scripts: ppo_lag, ppo, pg, cppo_pid; up to 32.  "
                        "The update's step takes 7.8-7.9 us for all seeds together up to 16 and 8.2 us at 32 where one seed alone takes "
                        "7.7 (60 / 8; profiles/seed_batch/step_times.txt): no knee up to 32, so the largest K the sweep has seeds for)")
    p.add_argument("--batch-second-order", action="store_true",
                   help="with --seeds-per-run: also group cpo / pcpo / rcpo / trpo_lag / trpo / natural_pg (at most 24 seeds per "
                        "subprocess, --batch-critic-fit True on those commands; observations up to 64 values).  One "
                        "critic-fit step of ALL seeds takes 9.9 / 11.2 / 14.2 us at 8 / 16 / 24 seeds against 9.8 us per seed one after "
                        "the other (60 / 8; profiles/seed_batch_critic/step_times.txt): the time per seed falls up to the cap, so the "
                        "largest K the sweep has seeds for.  Default off: these algorithms keep one subprocess per seed")
    p.add_argument("--batch-second-order-wide-obs", action="store_true",
                   help="with --batch-second-order: also group those scripts on the Ant / Car / Doggo / Racecar navigation tasks (65-128 "
                        "observations; up to 32 seeds per subprocess, --batch-critic-fit True --batch-critic-fit-split True on those "
                        "commands): their two-replica split critic fits share one persistent launch per iteration.  "
                        + CRITIC_SPLIT_BATCH_FIGURES + "  Default off: those tasks keep one subprocess per seed")
    p.add_argument("--batch-second-order-feature-split", action="store_true",
                   help="with --batch-second-order: also group those scripts on HumanoidVelocity (376 / 17: the critic fit on the "
                        "feature-split kernel; at most 8 seeds per subprocess, --batch-critic-fit True "
                        "--batch-critic-fit-feature-split True on those commands): their critic fits share one launch per "
                        "iteration.  " + CRITIC_KS_BATCH_FIGURES + "  Default off: HumanoidVelocity keeps one subprocess per seed")
    p.add_argument("--batch-focops-cup", action="store_true",
                   help="with --seeds-per-run: also group focops / cup (--batch-update True on those commands; HumanoidVelocity "
                        "excepted).  " + KLPEN_BATCH_FIGURES + "  Default off: these algorithms keep one subprocess per seed")
    p.add_argument("--batch-wide-obs", action="store_true",
                   help="with --seeds-per-run: also group HumanoidVelocity (376 / 17: the feature-split kernel) for ppo_lag / ppo / pg "
                        "/ cppo_pid, and with --batch-focops-cup for focops / cup, at most 8 seeds per subprocess "
                        "(--batch-wide-obs True on those commands).  " + KS_BATCH_FIGURES + "  Default off: HumanoidVelocity keeps "
                        "one subprocess per seed")
    p.add_argument("--hidden-sizes", type=int, nargs="+", default=None,
                   help="--hidden-sizes of every command (widths of the hidden layers; default: the scripts' [64, 64]).  Any other "
                        "widths run on the wide-network kernels: no script's --seeds form takes them except with --batch-wide-rows")
    p.add_argument("--batch-wide-rows", action="store_true",
                   help="with --seeds-per-run and --hidden-sizes other than 64 64: group ppo_lag / ppo / pg / cppo_pid (up to 32 seeds "
                        "per subprocess, --batch-wide-rows True on those commands): their minibatch steps share the three launches of "
                        "the row-group step.  " + ROWS_BATCH_FIGURES + "  Default off: such widths keep one subprocess per seed")
    p.add_argument("--batch-klpen-rows", action="store_true",
                   help="with --seeds-per-run, --batch-focops-cup and --hidden-sizes other than 64 64: group focops / cup (up to 32 seeds "
                        "per subprocess, --batch-update True --batch-klpen-rows True on those commands): their FOCOPS / CUP steps share "
                        "the five launches of the row-group KL-penalty step.  " + KLPEN_ROWS_BATCH_FIGURES + "  Default off: such widths "
                        "keep one subprocess per seed")
    return p.parse_args(argv)


SEED_BATCHED_ALGOS = ("ppo_lag", "ppo", "pg", "cppo_pid")     # the scripts with a `--seeds` form (persistent-kernel shapes only)
CRITIC_BATCHED_ALGOS = ("cpo", "pcpo", "rcpo", "trpo_lag", "trpo", "natural_pg")   # ... with --batch-critic-fit True
KLPEN_BATCHED_ALGOS = ("focops", "cup")                       # ... with --batch-update True (persistent-kernel shapes only)
CRITIC_BATCH_MAX = 24                                         # include/safepo_hip.h SPO_RS_CRITIC_MAX_REPLICAS
WIDE_OBS_NAV_ROBOTS = ("Ant", "Car", "Doggo", "Racecar")      # navigation tasks with 65 .. 128 observations: WideCPOEngine
CRITIC_SPLIT_BATCH_MAX = 32                                   # include/safepo_hip.h SPO_CRITIC_SPLIT_MAX_REPLICAS
CRITIC_KS_BATCH_MAX = 8                                       # seeds per subprocess at 376 observations: one run per XCD label
ROWS_BATCH_MAX = 32                                           # include/safepo_hip.h SPO_WIDE_ROWS_MAX_REPLICAS
KS_BATCH_MAX = 8                                              # spo_update_ks_multi_supported at 376 observations (S = 6: one run per XCD)


def _takes_seeds(algo: str, task: str) -> bool:
    """Can `--seeds` alone carry several seeds for this (algorithm, task)?  HumanoidVelocity (376 / 17) is outside the persistent
    kernels' shapes: its seeds share a launch only with `--batch-wide-obs True` (_takes_wide_obs_batch)."""
    return algo in SEED_BATCHED_ALGOS and "Humanoid" not in task


def _takes_klpen_batch(algo: str, task: str) -> bool:
    """Can `--seeds ... --batch-update True` carry several seeds for this (algorithm, task)?  As _takes_seeds: every task but
    HumanoidVelocity runs on the persistent kernels (up to 128 observations); that one needs `--batch-wide-obs True` as well."""
    return algo in KLPEN_BATCHED_ALGOS and "Humanoid" not in task


def _takes_critic_batch(algo: str, task: str) -> bool:
    """Can `--seeds ... --batch-critic-fit True` carry several seeds for this (algorithm, task)?  The full-batch CPO kernels of
    CPOEngine end at 64 observations: HumanoidVelocity and the Ant / Car / Doggo / Racecar navigation tasks run on WideCPOEngine."""
    wide = "Humanoid" in task or _is_wide_obs_nav(task)
    return algo in CRITIC_BATCHED_ALGOS and not wide


def _is_wide_obs_nav(task: str) -> bool:
    return "Velocity" not in task and any(task.startswith(f"Safety{r}") for r in WIDE_OBS_NAV_ROBOTS)


def _takes_critic_split_batch(algo: str, task: str) -> bool:
    """Can `--seeds ... --batch-critic-fit True --batch-critic-fit-split True` carry several seeds?  The Ant / Car / Doggo /
    Racecar navigation tasks (65-128 observations: the split critic fit); not HumanoidVelocity (376: the feature-split kernel)."""
    return algo in CRITIC_BATCHED_ALGOS and _is_wide_obs_nav(task)


def _takes_critic_ks_batch(algo: str, task: str) -> bool:
    """Can `--seeds ... --batch-critic-fit True --batch-critic-fit-feature-split True` carry several seeds?  HumanoidVelocity
    (376 / 17, hidden [64, 64]: the critic fit on the feature-split kernel) for the six second-order scripts."""
    return algo in CRITIC_BATCHED_ALGOS and "Humanoid" in task


def _takes_wide_obs_batch(algo: str, task: str, klpen_too: bool) -> bool:
    """Can `--seeds ... --batch-wide-obs True` carry several seeds?  HumanoidVelocity (376 / 17, hidden [64, 64]: the feature-split
    kernel) for the PPO family, and for focops / cup where --batch-focops-cup adds `--batch-update True`."""
    return "Humanoid" in task and (algo in SEED_BATCHED_ALGOS or (klpen_too and algo in KLPEN_BATCHED_ALGOS))


def build_commands(args, script_dir: str = HERE, n_gpus: int | None = None):
    n_gpus = n_gpus or visible_gpus()
    if getattr(args, "batch_second_order_wide_obs", False) and not getattr(args, "batch_second_order", False):
        raise SystemExit("--batch-second-order-wide-obs widens --batch-second-order: give both")
    if getattr(args, "batch_second_order_feature_split", False) and not getattr(args, "batch_second_order", False):
        raise SystemExit("--batch-second-order-feature-split widens --batch-second-order: give both")
    per_run = max(getattr(args, "seeds_per_run", 1), 1)
    if per_run > 32:
        raise SystemExit("--seeds-per-run: at most 32 seeds share a launch")
    seeds = [args.start_seed + 1000 * k for k in range(args.num_seeds)]
    commands = []
    for g0 in range(0, len(seeds), per_run):
        group = seeds[g0:g0 + per_run]
        for task in args.tasks:
            total, per_epoch, envs = args.total_steps, args.steps_per_epoch, args.num_envs
            if "Doggo" in task:                     # benchmark.py:99-102: the long-horizon robot gets 10x the budget
                total, per_epoch, envs = 100000000, 200000, 20
            for algo in args.algo:
                # one command for the whole group where the script takes --seeds, else one per seed as ever
                critic = getattr(args, "batch_second_order", False) and _takes_critic_batch(algo, task)
                klpen = getattr(args, "batch_focops_cup", False) and _takes_klpen_batch(algo, task)
                split = (getattr(args, "batch_second_order", False) and getattr(args, "batch_second_order_wide_obs", False)
                         and _takes_critic_split_batch(algo, task))
                critic_ks = (getattr(args, "batch_second_order", False) and getattr(args, "batch_second_order_feature_split", False)
                             and _takes_critic_ks_batch(algo, task))
                wide = (getattr(args, "batch_wide_obs", False)
                        and _takes_wide_obs_batch(algo, task, getattr(args, "batch_focops_cup", False)))
                # --hidden-sizes other than [64, 64]: every script steps on the wide-network kernels, whose only seed-batched form is
                # the row-group step of the PPO family (--batch-wide-rows)
                hidden = getattr(args, "hidden_sizes", None)
                custom = hidden is not None and [int(h) for h in hidden] != [64, 64]
                rows = custom and getattr(args, "batch_wide_rows", False) and algo in SEED_BATCHED_ALGOS
                # ... and, for focops / cup, the row-group KL-penalty step (--batch-klpen-rows with --batch-focops-cup)
                klpen_rows = (custom and getattr(args, "batch_klpen_rows", False) and getattr(args, "batch_focops_cup", False)
                              and algo in KLPEN_BATCHED_ALGOS)
                if custom:
                    critic = klpen = split = critic_ks = wide = False
                runs = [[s] for s in group]
                if len(group) > 1 and (rows or klpen_rows):
                    runs = [group[i:i + ROWS_BATCH_MAX] for i in range(0, len(group), ROWS_BATCH_MAX)]
                elif custom:
                    pass
                elif len(group) > 1 and (_takes_seeds(algo, task) or klpen):
                    runs = [group]
                elif len(group) > 1 and wide:
                    runs = [group[i:i + KS_BATCH_MAX] for i in range(0, len(group), KS_BATCH_MAX)]
                elif len(group) > 1 and critic:
                    runs = [group[i:i + CRITIC_BATCH_MAX] for i in range(0, len(group), CRITIC_BATCH_MAX)]
                elif len(group) > 1 and split:
                    runs = [group[i:i + CRITIC_SPLIT_BATCH_MAX] for i in range(0, len(group), CRITIC_SPLIT_BATCH_MAX)]
                elif len(group) > 1 and critic_ks:
                    runs = [group[i:i + CRITIC_KS_BATCH_MAX] for i in range(0, len(group), CRITIC_KS_BATCH_MAX)]
                for run in runs:
                    batched = len(run) > 1
                    commands.append(" ".join([
                        shlex.quote(sys.executable), shlex.quote(os.path.join(script_dir, f"{algo}.py")), "--task", shlex.quote(task),
                        "--seed", str(run[0])] + (["--seeds"] + [str(s) for s in run] if batched else [])
                        + (["--batch-critic-fit", "True"] if batched and critic else [])
                        + (["--batch-critic-fit", "True", "--batch-critic-fit-split", "True"] if batched and split else [])
                        + (["--batch-critic-fit", "True", "--batch-critic-fit-feature-split", "True"] if batched and critic_ks else [])
                        + (["--batch-update", "True"] if batched and (klpen or (wide and algo in KLPEN_BATCHED_ALGOS)) else [])
                        + (["--batch-wide-obs", "True"] if batched and wide else [])
                        + (["--hidden-sizes"] + [str(int(h)) for h in hidden] if hidden is not None else [])
                        + (["--batch-wide-rows", "True"] if batched and rows else [])
                        + (["--batch-update", "True", "--batch-klpen-rows", "True"] if batched and klpen_rows else []) + [
                        "--write-terminal", "False", "--experiment",
                        shlex.quote(args.experiment), "--total-steps", str(total), "--num-envs", str(envs), "--steps-per-epoch",
                        str(per_epoch), "--device-id", str(len(commands) % n_gpus)]))
    return commands


def run_experiment(command: str) -> int:
    print(f"running {command}", flush=True)
    rc = subprocess.Popen(shlex.split(command)).wait()
    assert rc == 0, f"exit code {rc}: {command}"
    return rc


def main(argv=None):
    args = parse_args(argv)
    commands = build_commands(args)
    print("======= commands to run:")
    for c in commands:
        print(c)
    workers = visible_gpus() if args.workers is None else args.workers
    if workers <= 0:
        print("not running the experiments because --workers is set to 0; just printing the commands to run")
        return commands
    with ThreadPoolExecutor(max_workers=workers, thread_name_prefix="safepo-benchmark-worker-") as ex:
        futures = [ex.submit(run_experiment, c) for c in commands]
    for fu in futures:
        fu.result()
    return commands


if __name__ == "__main__":
    main()
