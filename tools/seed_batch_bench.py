"""Development aid (GPU box): the seed-batched PPO-Lagrangian launch (spo_ppo_lag_update_iter_multi, csrc/update_rs.hip; S independent
runs, each on its own six co-XCD workgroups, in ONE persistent launch) against S back-to-back single launches of
spo_ppo_lag_update_iter, over 4096 x 128-row buffers:
    python tools/seed_batch_bench.py [--calls 16] [--warmup 2] [--out profiles/seed_batch/step_times.txt]
    python tools/seed_batch_bench.py --end-to-end        # ppo_lag --seeds at S = 8 against eight sequential runs -> appended
    python tools/seed_batch_bench.py --resource-usage    # no GPU: registers / spills / scratch of the kernels -> resource_usage.txt
One child process per shape; inside it, for every S, the two paths ALTERNATE call by call.  A sample is a HIP event pair around one
learning iteration of all S runs (8 192 steps of 64 rows each): one batched launch, or S single launches enqueued back to back;
parameters and optimiser state are put back and the runs' error words are read outside the timed window.  Reported per shape and
S: median and minimum of the window per step (one step = every run advancing one minibatch), the same per replica-step, the
aggregate rate of the batched launch relative to the single launches, whether that gain exceeds both sides' median - minimum
spread, how many runs took the write-through path of the placement census, and whether any call set an error word."""
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

SHAPES = [(60, 8), (72, 2)]
S_LIST = [1, 2, 4, 8, 16, 32]
N, T, BATCH = 4096, 128, 64
OUT_DIR = os.path.join(ROOT, "profiles", "seed_batch")


def child(D, A, calls, warmup):
    import ctypes
    import torch
    from safepo import _abi
    from safepo.common.engine import PPOLagEngine
    from safepo.common.engine_group import PPOLagEngineGroup
    from safepo.common.model import ActorVCritic
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = _abi.load()
    M = N * T
    nst = M // BATCH
    g = torch.Generator(device=dev).manual_seed(1)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": BATCH, "learning_iters": 1, "max_grad_norm": 40.0}

    def counters():
        c4, c2 = (ctypes.c_ulonglong * 4)(), (ctypes.c_ulonglong * 2)()
        _abi.check(lib.spo_debug_update_counters(c4, 1), "counters")
        _abi.check(lib.spo_debug_rs_multi_counters(c2, 1), "multi counters")
        return int(c4[0]), int(c2[0]), int(c2[1])

    engines, perms, theta0 = [], [], []
    for r in range(max(S_LIST)):
        torch.manual_seed(D + r)
        pol = ActorVCritic(D, A).to(dev)
        eng = PPOLagEngine(pol, N, T, cfg, dev)
        b = eng.buffer
        for k in ("obs", "act", "target_value_r", "target_value_c"):
            b.data[k].normal_(generator=g)
        b.data["log_prob"].copy_(-A * 0.92 - 0.5 * (b.data["act"] ** 2).sum(-1) + 0.1 * torch.randn(N, T, device=dev, generator=g))
        b.adv_mix.normal_(generator=g)
        engines.append(eng)
        perms.append(torch.randperm(M, device=dev, generator=g).to(torch.int32))
        theta0.append(pol.theta.clone())

    entry = {"obs_dim": D, "act_dim": A, "rows": []}
    for S in S_LIST:
        es = engines[:S]
        group = PPOLagEngineGroup(es)
        assert group.batched()

        def restore():
            for e, t0 in zip(es, theta0):
                e.policy.theta.copy_(t0); e.adam_m.zero_(); e.adam_v.zero_(); e.adam_step = 0

        def batched():
            group.learning_iter_all(perms[:S])

        def single():
            for e, p in zip(es, perms):
                e.learning_iter(p)

        us = {"batched": [], "single": []}
        safe_runs, errs = 0, 0
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
                steps, runs, safe = counters()
                assert steps == S * nst, (name, S, steps)
                assert runs == (S if name == "batched" else 0), (name, S, runs)
                try:
                    group.check_sync_error()
                except _abi.SpoError as err:                      # (an exchange timed out: recorded, not hidden)
                    errs += 1
                    print("ERR", name, S, err, flush=True)
                if i >= warmup:
                    us[name].append(e0.elapsed_time(e1) * 1e3 / nst)
                    safe_runs += safe
        entry["rows"].append({"S": S, "us": us, "write_through_runs": safe_runs, "batched_runs": S * calls, "err_calls": errs})
        print(f"S {S} done", flush=True)
    print("RESULT " + json.dumps(entry))


def end_to_end_child(mode, seeds, log_root):
    """mode "batched": ppo_lag.main with --seeds; "sequential": one main() per seed, one after the other.  Two epochs each at the
    benchmark's size (the first carries the lazy set-up and the rollout-graph capture); the second epoch's Time/ columns are read."""
    import argparse as ap
    import csv
    from safepo.single_agent import ppo_lag

    def args(**kw):
        a = ap.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=N, experiment="e2e", log_dir=log_root, device="cuda",
                         device_id=0, write_terminal=True, headless=False, total_steps=2 * N * T, steps_per_epoch=N * T, randomize=False,
                         cost_limit=25.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035, cfg_override={}, env_kwargs={})
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def second_epoch(d):
        row = list(csv.DictReader(open(os.path.join(d, "progress.csv"))))[1]
        return {k: float(row[k]) for k in ("Time/Rollout", "Time/Update", "Time/Total", "Train/StopIter")}

    t0 = time.time()
    if mode == "batched":
        dirs = [os.path.join(log_root, f"b{s}") for s in seeds]
        ppo_lag.main(args(seeds=list(seeds), log_dirs=dirs), {})
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
    """hipcc -Rpass-analysis=kernel-resource-usage on csrc/update_rs.hip with the build's own flags (cross-compiles; no GPU)."""
    import tempfile
    import __graft_entry__ as ge
    src = os.path.join(ge.CSRC, "update_rs.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [ge._hipcc()] + ge.HIPCC_FLAGS + ge.EXTRA_FLAGS.get("update_rs.hip", []) + ["-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                                                          "-o", os.path.join(tmp, "update_rs.o")]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(r.stderr)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            name = subprocess.run(["c++filt", text.split(":", 1)[1].strip()], capture_output=True, text=True).stdout.strip()
            m2 = re.search(r"ppo_update_rs(_multi)?_kernel<[^>]*>", name or text)
            cur = {"name": m2.group(0) if m2 else (name or text)}
            rows.append(cur)
        elif cur is not None and ":" in text:
            k, val = text.split(":", 1)
            cur[k.strip()] = val.strip()
    keys = ["VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
            "LDS Size [bytes/block]"]
    lines = ["kernel-resource-usage of csrc/update_rs.hip (gfx950): every instantiation of ppo_update_rs_kernel<KIN, R, PROF, XW, NCT> (the "
             "single launch) and of ppo_update_rs_multi_kernel<KIN> (the seed-batched launch: rs_body<KIN, 2, FAST, false, 0, 2, MULTI>, "
             "its arguments read from a device table instead of the kernel-argument segment).",
             "LDS is taken dynamically (LDS Size shows the static part, 0): RsLds<KIN, 2> = 71 936 / 80 640 / 98 048 / 132 864 bytes at KIN "
             "16 / 32 / 64 / 128 of the 163 840."]
    for row in sorted(rows, key=lambda r: ("multi" in r["name"], r["name"])):
        if row["name"].startswith("ppo_update_rs"):
            lines.append(row["name"])
            lines.append("    " + "  ".join(f"{k}: {row.get(k, '?')}" for k in keys))
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
    """The child's output is passed on line by line as it comes; its RESULT line is returned."""
    import threading
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    killer = threading.Timer(timeout, p.kill)
    killer.start()
    result = None
    try:
        for line in p.stdout:
            if line.startswith("RESULT "):
                result = line[7:]
            else:
                print("  | " + line.rstrip()[:200], flush=True)
        rc = p.wait()
    finally:
        killer.cancel()
    if rc != 0 or result is None:
        raise SystemExit(f"child {argv} failed with {rc}")          # (nothing more is started on the GPU)
    return json.loads(result)


def decide(D, A, rows):
    """The quantities that decide what may be claimed, from the BATCHED launch's own samples: the step at S = 8, 16, 32 against
    S = 1 (one run per XCD should cost nothing; more share an L2), each with its median - minimum spread, and where the time per
    replica-step stops falling."""
    b = {r["S"]: stats(r["us"]["batched"]) for r in rows}
    out = [f"{D}/{A}: batched us/step, median (median - minimum):  " + "   ".join(f"S={S}: {m:.2f} ({m - lo:.2f})" for S, (m, lo) in b.items())]
    m1, l1 = b[1]
    for S in (8, 16, 32):
        m, lo = b[S]
        spread = max(m - lo, m1 - l1)
        verdict = "within the spread" if abs(m - m1) <= spread else ("slower" if m > m1 else "faster")
        out.append(f"    step at S = {S} against S = 1: {m - m1:+.2f} us ({m / m1:.2f}x), spread {spread:.2f} us: {verdict}")
    m8, l8 = b[8]
    for S in (16, 32):
        m, lo = b[S]
        spread = max((m - lo) / S, (m8 - l8) / 8)
        d = m / S - m8 / 8
        verdict = "within the spread" if abs(d) <= spread else ("SLOWER per replica-step than S = 8" if d > 0 else "faster per replica-step than S = 8")
        out.append(f"    replica-step at S = {S} against S = 8: {m / S:.3f} against {m8 / 8:.3f} us, spread {spread:.3f} us: {verdict}")
    out.append(f"    write-through runs: {sum(r['write_through_runs'] for r in rows)} of {sum(r['batched_runs'] for r in rows)}; "
               f"calls that set an error word: {sum(r['err_calls'] for r in rows)}")
    out.append("")
    return out


def parent(args):
    lines = [f"hidden [64, 64], {N} x {T} = {N * T} rows per run, minibatches of {BATCH}: one learning iteration = {N * T // BATCH} steps per run.",
             "us/step = one HIP event pair around the learning iteration of ALL S runs / its steps (a step = every run advancing one minibatch);",
             "us/replica-step = us/step / S.  single = S launches of spo_ppo_lag_update_iter back to back; batched = one "
             "spo_ppo_lag_update_iter_multi launch.",
             f"one process per shape, the two paths alternating call by call, {args.warmup} warm-up then {args.calls} timed calls each; "
             "median (minimum).",
             "rate = aggregate replica-steps/s of batched over single (medians); wins = the batched median beats the single median by more "
             "than max(median - min) of the two sides;",
             "wt = runs of the timed batched calls whose placement census chose write-through stores / runs; err = calls after which a run's "
             "error word was set.", ""]
    lines.append(f"{'obs/act':>8} {'S':>3} {'single us/step':>22} {'batched us/step':>22} {'single us/rep-step':>20} "
                 f"{'batched us/rep-step':>20} {'rate':>7} {'wins':>5} {'wt':>9} {'err':>4}")
    deciding = []
    for D, A in SHAPES:
        e = run_child(["--child", f"{D},{A}", "--calls", str(args.calls), "--warmup", str(args.warmup)], args.child_timeout)
        for row in e["rows"]:
            S = row["S"]
            (sm, sl), (bm, bl) = stats(row["us"]["single"]), stats(row["us"]["batched"])
            win = (sm - bm) > max(sm - sl, bm - bl)
            lines.append(f"{D:>4}/{A:<3} {S:>3} {sm:13.2f} ({sl:6.2f}) {bm:13.2f} ({bl:6.2f}) {sm / S:12.3f} ({sl / S:6.3f}) "
                         f"{bm / S:12.3f} ({bl / S:6.3f}) {sm / bm:6.2f}x {'yes' if win else 'NO':>5} "
                         f"{row['write_through_runs']:>4}/{row['batched_runs']:<4} {row['err_calls']:>4}")
        print(f"shape {D}/{A} done", flush=True)
        deciding.append(decide(D, A, e["rows"]))
    lines.append("")
    lines += [ln for d in deciding for ln in d]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
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
    lines = ["", f"END TO END: ppo_lag on SynthSafe-v0, {N} envs x {T} steps per epoch, default configuration (learning_iters 40, target_kl 0.02), "
             "eight seeds; the SECOND epoch of every run (the first carries lazy set-up and the rollout-graph capture), from the loggers' Time/ columns.",
             "sequential = eight `--seed` runs one after the other in one process (columns summed over the runs); batched = one `--seeds` run "
             "(the columns hold the phase's wall time for all eight seeds).  One sample each: no spread was measured.",
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
    ap.add_argument("--child-timeout", type=int, default=900)
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
        d_, a_ = (int(x) for x in a.child.split(","))
        child(d_, a_, a.calls, a.warmup)
    elif a.e2e_child:
        end_to_end_child(a.e2e_child, a.e2e_seeds, a.e2e_dir)
    elif a.end_to_end:
        end_to_end(a)
    else:
        parent(a)
