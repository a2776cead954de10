"""Development aid (GPU box): the seed-batched feature-split launch (spo_update_iter_ex_ks_multi, csrc/update_ks.hip; S independent
runs, each on its own 3 x ceil(obs_dim / 64) workgroups of one XCD, in ONE launch) against S back-to-back single launches of
spo_update_iter_ex_ks, over 4096 x 128-row buffers:
    python tools/seed_batch_ks_bench.py [--calls 16] [--warmup 2] [--out profiles/seed_batch_ks/step_times.txt]
    python tools/seed_batch_ks_bench.py --end-to-end      # ppo_lag --seeds --batch-wide-obs True at S = 8 against eight runs -> appended
    python tools/seed_batch_ks_bench.py --resource-usage  # no GPU: registers / spills / scratch of the kernels -> resource_usage.txt
Three modes at 376 / 17 (HumanoidVelocity): "clip" (the clipped-surrogate step of ppo_lag / ppo / pg / cppo_pid and CUP's first
stage), "focops" (KL-penalty loss, three networks) and "cup2" (CUP's second stage: KL-penalty loss, the actor alone), S = 1 / 2 / 4
/ 8; and the clipped-surrogate step at 192 / 8 with S = 8 / 16, where two runs share an XCD.  One child process per (shape, mode),
each under a time limit of its own; inside it, for every S, the two paths ALTERNATE call by call.  A sample is a HIP event pair
around one learning iteration of all S runs (8 192 steps of 64 rows each): one batched launch, or S single launches enqueued back
to back; parameters, optimiser state and clocks are put back and the runs' error words are read outside the timed window."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "safe-policy-optimization_amd"))

# (obs_dim, act_dim, mode, run counts)
CASES = [(376, 17, "clip", [1, 2, 4, 8]), (376, 17, "focops", [1, 2, 4, 8]), (376, 17, "cup2", [1, 2, 4, 8]), (192, 8, "clip", [8, 16])]
N, T, BATCH = 4096, 128, 64
OUT_DIR = os.path.join(ROOT, "profiles", "seed_batch_ks")
WHAT = {"clip": "the clipped-surrogate step", "focops": "the FOCOPS step", "cup2": "CUP's second stage (actor alone)"}


def child(D, A, mode, s_list, calls, warmup):
    import ctypes
    import torch
    from safepo import _abi
    from safepo.common.engine import WidePPOLagEngine
    from safepo.common.engine_group import PPOLagEngineGroup
    from safepo.common.model import ActorVCritic
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = _abi.load()
    M = N * T
    nst = M // BATCH
    g = torch.Generator(device=dev).manual_seed(1)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 0.02, "batch_size": BATCH, "learning_iters": 1, "max_grad_norm": 40.0}
    actor_loss = _abi.ACTOR_LOSS_CLIP if mode == "clip" else _abi.ACTOR_LOSS_KL_PENALTY
    actor_only = mode == "cup2"
    kl_bound = 0.02 if mode == "focops" else float("inf")
    pg_coef = {"focops": 1.0 / 1.5, "cup2": -0.2 * (1 - 0.99 * 0.95) / (1 - 0.99), "clip": 0.0}[mode]

    def counters():
        c3 = (ctypes.c_ulonglong * 3)()
        _abi.check(lib.spo_debug_update_ks_multi_counters(c3, 1), "ks multi counters")
        return int(c3[0]), int(c3[1]), int(c3[2])

    engines, perms, advs, theta0 = [], [], [], []
    for r in range(max(s_list)):
        torch.manual_seed(D + r)
        pol = ActorVCritic(D, A).to(dev)
        eng = WidePPOLagEngine(pol, N, T, cfg, dev)
        assert eng._feature_split_kernel_ok(eng._cfg_struct())
        b = eng.buffer
        for k in ("obs", "act", "target_value_r", "target_value_c"):
            b.data[k].normal_(generator=g)
        b.data["log_prob"].copy_(-A * 0.92 - 0.5 * (b.data["act"] ** 2).sum(-1) + 0.1 * torch.randn(N, T, device=dev, generator=g))
        eng.snapshot_old_distribution()                     # the old distribution: the initial policy, as at the start of an update
        engines.append(eng)
        advs.append(torch.randn(N, T, device=dev, generator=g))
        perms.append(torch.randperm(M, device=dev, generator=g).to(torch.int32))
        theta0.append(pol.theta.clone())

    entry = {"obs_dim": D, "act_dim": A, "mode": mode, "rows": []}
    for S in s_list:
        es = engines[:S]
        group = PPOLagEngineGroup(es)
        assert group.batched_ex(actor_loss)

        def restore():
            for e, t0 in zip(es, theta0):
                e.policy.theta.copy_(t0); e.adam_m.zero_(); e.adam_v.zero_(); e.adam_step = 0; e.adam_step_actor_extra = 0

        def batched():
            group.learning_iter_ex_all(perms[:S], advs[:S], actor_loss, [kl_bound] * S, [pg_coef] * S, actor_only)

        def single():
            for e, p, adv in zip(es, perms, advs):
                e.learning_iter_ex(p, adv, actor_loss, kl_bound, pg_coef, actor_only)

        us = {"batched": [], "single": []}
        errs, wt = 0, 0
        for i in range(warmup + calls):
            for name, call in (("single", single), ("batched", batched)):
                restore()
                counters()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                c = counters()
                assert c[:2] == ((1, S) if name == "batched" else (0, 0)), (name, S, c)
                wt += c[2]
                try:
                    group.check_sync_error()
                except _abi.SpoError as err:                      # (an exchange timed out: recorded, not hidden)
                    errs += 1
                    print("ERR", name, S, err, flush=True)
                if i >= warmup:
                    us[name].append(e0.elapsed_time(e1) * 1e3 / nst)
        entry["rows"].append({"S": S, "us": us, "err_calls": errs, "write_through_runs": wt, "batched_runs": (warmup + calls) * S})
        print(f"S {S} done", flush=True)
    print("RESULT " + json.dumps(entry))


def end_to_end_child(mode, seeds, log_root):
    """mode "batched": ppo_lag.main with --seeds and --batch-wide-obs True; "sequential": one main() per seed, one after the other.
    Two epochs each at the benchmark's size (the first carries the lazy set-up and the rollout-graph capture); the second epoch's
    Time/ columns are read."""
    import argparse as ap
    import csv
    from safepo.single_agent import ppo_lag

    def args(**kw):
        a = ap.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=N, experiment="e2e", log_dir=log_root, device="cuda",
                         device_id=0, write_terminal=True, headless=False, total_steps=2 * N * T, steps_per_epoch=N * T, randomize=False,
                         cost_limit=25.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035, cfg_override={},
                         env_kwargs={"obs_dim": 376, "act_dim": 17}, batch_update=False, batch_wide_obs=False)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def second_epoch(d):
        row = list(csv.DictReader(open(os.path.join(d, "progress.csv"))))[1]
        return {k: float(row[k]) for k in ("Time/Rollout", "Time/Update", "Time/Total", "Train/StopIter")}

    t0 = time.time()
    if mode == "batched":
        dirs = [os.path.join(log_root, f"b{s}") for s in seeds]
        ppo_lag.main(args(seeds=list(seeds), log_dirs=dirs, batch_wide_obs=True), {})
        rows = [second_epoch(d) for d in dirs]
        out = {"rollout_s": rows[0]["Time/Rollout"], "update_s": rows[0]["Time/Update"], "total_s": rows[0]["Time/Total"]}
    else:
        rows = []
        for s in seeds:
            d = os.path.join(log_root, f"s{s}")
            ppo_lag.main(args(seed=s, log_dir=d), {})
            rows.append(second_epoch(d))
        out = {k2: sum(r[k] for r in rows) for k, k2 in (("Time/Rollout", "rollout_s"), ("Time/Update", "update_s"), ("Time/Total", "total_s"))}
    out.update(mode=mode, stop_iters=[r["Train/StopIter"] for r in rows], wall_s=time.time() - t0)
    print("RESULT " + json.dumps(out))


def resource_usage():
    """hipcc -Rpass-analysis=kernel-resource-usage on csrc/update_ks.hip with the build's own flags (cross-compiles; no GPU): the
    two seed-batched kernels next to the single launches' kernels."""
    import tempfile
    import __graft_entry__ as ge
    src = os.path.join(ge.CSRC, "update_ks.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [ge._hipcc()] + ge.HIPCC_FLAGS + ge.EXTRA_FLAGS.get("update_ks.hip", []) + ["-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                                                          "-o", os.path.join(tmp, "update_ks.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    want = ("ppo_update_ks_kernel", "ppo_update_ks_multi_kernel", "klpen_update_ks_kernel", "klpen_update_ks_multi_kernel")
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            name = subprocess.run(["c++filt", text.split(":", 1)[1].strip()], capture_output=True, text=True).stdout.strip()
            mm = re.search(r"(\w+_kernel)\(", name)
            base = mm.group(1) if mm else None
            cur = None
            if base in want:
                cur = rows[base] = {"name": base}
        elif cur is not None and ":" in text:
            k, val = text.split(":", 1)
            cur[k.strip()] = val.strip()
    keys = ["VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
            "LDS Size [bytes/block]"]
    lines = ["kernel-resource-usage of csrc/update_ks.hip (gfx950): the seed-batched kernels (ks_entry<false, AMODE> with the run's "
             "arguments read from a device table and the workgroup index from rs_multi_map) under their single-launch counterparts (the "
             "same body, arguments in the kernel-argument segment, workgroup index blockIdx.x >> 3).  AMODE 0: clipped surrogate "
             "(ppo_update_ks*), 1: KL penalty (klpen_update_ks*).",
             "LDS is taken dynamically (LDS Size shows the static part, 0): KsLds::SIZE * 4 = 140 928 bytes for all four, one workgroup "
             "per CU."]
    assert sorted(rows) == sorted(want), sorted(rows)
    for name in want:
        lines.append(name)
        lines.append("    " + "  ".join(f"{k}: {rows[name].get(k, '?')}" for k in keys))
    for single, multi in ((want[0], want[1]), (want[2], want[3])):      # a batched kernel with scratch where its counterpart has none is a defect
        if int(rows[single]["ScratchSize [bytes/lane]"]) == 0:
            assert int(rows[multi]["ScratchSize [bytes/lane]"]) == 0, (rows[single], rows[multi])
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, "resource_usage.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", path)


def stats(us):
    s = sorted(us)
    return s[len(s) // 2], s[0]


def run_child(argv, timeout):
    """One GPU step under its own time limit (`timeout -k 10 <s>`); the child's output is passed on line by line as it comes, its
    RESULT line is returned.  A child that fails or runs out of time ends the tool: nothing more is started on the GPU."""
    p = subprocess.Popen(["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    result = None
    for line in p.stdout:
        if line.startswith("RESULT "):
            result = line[7:]
        else:
            print("  | " + line.rstrip()[:200], flush=True)
    rc = p.wait()
    if rc != 0 or result is None:
        raise SystemExit(f"child {argv} failed with {rc}")
    return json.loads(result)


def decide(D, A, mode, rows):
    """Per S: is the batched launch ahead of S sequential launches by more than three times the larger median - minimum spread?"""
    out = [f"{D}/{A} {mode}:"]
    for r in rows:
        S = r["S"]
        (sm, sl), (bm, bl) = stats(r["us"]["single"]), stats(r["us"]["batched"])
        spread = max(sm - sl, bm - bl)
        verdict = "AHEAD beyond the spread" if sm - bm > 3 * spread else ("BEHIND beyond the spread" if bm - sm > 3 * spread else "within the spread")
        out.append(f"    S = {S}: batched {bm:.2f} us (spread {bm - bl:.2f}) against {sm:.2f} us (spread {sm - sl:.2f}) for {S} single "
                   f"launch{'es' if S > 1 else ''}: {sm / bm:.2f}x the aggregate step rate; gain {sm - bm:+.2f} us against 3 x the larger "
                   f"spread {3 * spread:.2f} us: {verdict}")
    out.append(f"    calls that set an error word: {sum(r['err_calls'] for r in rows)}; runs of batched launches on write-through stores: "
               f"{sum(r['write_through_runs'] for r in rows)} of {sum(r['batched_runs'] for r in rows)}")
    out.append("")
    return out


def parent(args):
    lines = [f"hidden [64, 64], {N} x {T} = {N * T} rows per run, minibatches of {BATCH}: one learning iteration = {N * T // BATCH} steps per run.",
             "us/step = one HIP event pair around the learning iteration of ALL S runs / its steps (a step = every run advancing one minibatch);",
             "us/run-step = us/step / S.  single = S launches of spo_update_iter_ex_ks back to back; batched = one spo_update_iter_ex_ks_multi launch.",
             "modes: " + "; ".join(f"{k} = {v}" for k, v in WHAT.items()) + ".",
             f"one process per (shape, mode), the two paths alternating call by call, {args.warmup} warm-up then {args.calls} timed calls each; "
             "median (minimum).",
             "rate = aggregate run-steps/s of batched over single (medians); wins = the batched median beats the single median by more "
             "than 3 x max(median - min) of the two sides; err = calls after which a run's error word was set; wt = runs of the batched "
             "launches whose placement census chose write-through stores.", ""]
    lines.append(f"{'obs/act':>8} {'mode':>7} {'S':>3} {'single us/step':>22} {'batched us/step':>22} {'single us/run-step':>20} "
                 f"{'batched us/run-step':>20} {'rate':>7} {'wins':>5} {'err':>4} {'wt':>4}")
    deciding = []
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for D, A, mode, s_list in CASES:
        e = run_child(["--child", f"{D},{A},{mode}," + "/".join(map(str, s_list)), "--calls", str(args.calls), "--warmup", str(args.warmup)],
                      args.child_timeout)
        for row in e["rows"]:
            S = row["S"]
            (sm, sl), (bm, bl) = stats(row["us"]["single"]), stats(row["us"]["batched"])
            win = (sm - bm) > 3 * max(sm - sl, bm - bl)
            lines.append(f"{D:>4}/{A:<3} {mode:>7} {S:>3} {sm:13.2f} ({sl:6.2f}) {bm:13.2f} ({bl:6.2f}) {sm / S:12.3f} ({sl / S:6.3f}) "
                         f"{bm / S:12.3f} ({bl / S:6.3f}) {sm / bm:6.2f}x {'yes' if win else 'NO':>5} {row['err_calls']:>4} "
                         f"{row['write_through_runs']:>4}")
        print(f"{D}/{A} {mode} done", flush=True)
        deciding.append(decide(D, A, mode, e["rows"]))
        with open(args.out + ".partial", "w") as f:              # (kept up to date: a later child that fails loses nothing measured)
            f.write("\n".join(lines + [""] + [ln for d in deciding for ln in d]) + "\n")
    lines.append("")
    lines += [ln for d in deciding for ln in d]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    os.remove(args.out + ".partial")
    print("\n".join(lines))


def end_to_end(args):
    import tempfile
    seeds = [1000 * k for k in range(8)]
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for mode in ("sequential", "batched"):
            res[mode] = run_child(["--e2e-child", mode, "--e2e-dir", os.path.join(tmp, mode), "--e2e-seeds"] + [str(s) for s in seeds],
                                  args.child_timeout)
    q, b = res["sequential"], res["batched"]
    lines = ["", f"END TO END: ppo_lag on SynthSafe-v0 at 376 / 17, {N} envs x {T} steps per epoch, default configuration, eight seeds; the "
             "SECOND epoch of every run (the first carries lazy set-up and the rollout-graph capture), from the loggers' Time/ columns.",
             "sequential = eight `--seed` runs one after the other in one process (columns summed over the runs); batched = one `--seeds ... "
             "--batch-wide-obs True` run (the columns hold the phase's wall time for all eight seeds).  One sample each: no spread was measured.",
             f"{'':>12} {'Time/Rollout s':>15} {'Time/Update s':>15} {'Time/Total s':>14}   Train/StopIter per seed",
             f"{'sequential':>12} {q['rollout_s']:15.3f} {q['update_s']:15.3f} {q['total_s']:14.3f}   {q['stop_iters']}",
             f"{'batched':>12} {b['rollout_s']:15.3f} {b['update_s']:15.3f} {b['total_s']:14.3f}   {b['stop_iters']}",
             f"{'ratio':>12} {q['rollout_s'] / b['rollout_s']:14.2f}x {q['update_s'] / b['update_s']:14.2f}x {q['total_s'] / b['total_s']:13.2f}x", ""]
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=280)
    ap.add_argument("--out", default=os.path.join(OUT_DIR, "step_times.txt"))
    ap.add_argument("--child", default="")
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--e2e-child", default="")
    ap.add_argument("--e2e-dir", default="")
    ap.add_argument("--e2e-seeds", type=int, nargs="+", default=[])
    ap.add_argument("--resource-usage", action="store_true")
    a = ap.parse_args()
    assert a.calls >= 16, "at least 16 timed calls"
    if a.resource_usage:
        resource_usage()
    elif a.child:
        d_, a_, m_, s_ = a.child.split(",")
        child(int(d_), int(a_), m_, [int(x) for x in s_.split("/")], a.calls, a.warmup)
    elif a.e2e_child:
        end_to_end_child(a.e2e_child, a.e2e_seeds, a.e2e_dir)
    elif a.end_to_end:
        end_to_end(a)
    else:
        parent(a)
