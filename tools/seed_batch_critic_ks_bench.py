"""Development aid (GPU box): the seed-batched feature-split critic fit (spo_critic_fit_iter_ks_multi, csrc/update_ks.hip; S
independent runs, each on its own 2 x ceil(obs_dim / 64) workgroups of one XCD label, in ONE launch) against S back-to-back single
launches of spo_critic_fit_iter_ks, over 4096 x 128-row buffers with minibatches of 128 rows:
    python tools/seed_batch_critic_ks_bench.py [--calls 16] [--warmup 2] [--out profiles/seed_batch_critic_ks/step_times.txt]
    python tools/seed_batch_critic_ks_bench.py --end-to-end   # cpo --seeds --batch-critic-fit-feature-split True at S = 8 against eight runs -> appended
376 / 17 (HumanoidVelocity) at S = 1 / 2 / 4 / 8 / 16 -- at 16 two runs share an XCD label -- and 512 / 32 at S = 8.  One child
process per shape, each under a time limit of its own; inside it, for every S, the two paths ALTERNATE call by call.  A sample is
a HIP event pair around one critic-fit iteration of all S runs (4 096 steps of 128 rows each): one batched launch, or S single
launches enqueued back to back; parameters, optimiser state and stale norms are put back and the runs' error words are read
outside the timed window."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "safe-policy-optimization_amd"))

# (obs_dim, act_dim, run counts)
CASES = [(376, 17, [1, 2, 4, 8, 16]), (512, 32, [8])]
N, T, BATCH = 4096, 128, 128
OUT_DIR = os.path.join(ROOT, "profiles", "seed_batch_critic_ks")


def child(D, A, s_list, calls, warmup):
    import ctypes
    import torch
    from safepo import _abi
    from safepo.common.model import ActorVCritic
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = _abi.load()
    M = N * T
    nst = M // BATCH
    g = torch.Generator(device=dev).manual_seed(1)
    cfg = _abi.PpoCfg(obs_dim=D, act_dim=A, batch=BATCH, use_critic_norm=1, use_value_coefficient=0, clip=0.2, max_grad_norm=40.0,
                      lr_actor=3e-4, lr_critic=1e-3, beta1=0.9, beta2=0.999, adam_eps=1e-8, l2_coef=0.001)

    def counters():
        c3 = (ctypes.c_ulonglong * 3)()
        _abi.check(lib.spo_debug_critic_fit_ks_multi_counters(c3, 1), "critic_fit_ks multi counters")
        return int(c3[0]), int(c3[1]), int(c3[2])

    runs = []
    for r in range(max(s_list)):
        torch.manual_seed(D + r)
        theta0 = ActorVCritic(D, A).to(dev).theta.detach().clone()
        runs.append({"theta0": theta0, "theta": theta0.clone(), "m": torch.zeros_like(theta0), "v": torch.zeros_like(theta0),
                     "obs": torch.randn(M, D, device=dev, generator=g), "tgt_r": torch.randn(M, device=dev, generator=g),
                     "tgt_c": torch.rand(M, device=dev, generator=g), "perm": torch.randperm(M, device=dev, generator=g).to(torch.int32),
                     "stale": torch.full((1,), 0.5, device=dev), "losses": torch.empty((nst, 3), device=dev),
                     "sync_ws": torch.zeros(32, dtype=torch.int64, device=dev)})

    entry = {"obs_dim": D, "act_dim": A, "rows": []}
    for S in s_list:
        assert lib.spo_critic_fit_ks_multi_supported(D, BATCH, S) == 1
        rs = runs[:S]
        reps = (_abi.CriticFitReplica * S)()
        for t, x in zip(reps, rs):
            t.theta, t.adam_m, t.adam_v, t.adam_step = _abi.ptr(x["theta"]), _abi.ptr(x["m"]), _abi.ptr(x["v"]), 0
            t.obs, t.target_r, t.target_c = _abi.ptr(x["obs"]), _abi.ptr(x["tgt_r"]), _abi.ptr(x["tgt_c"])
            t.perm, t.losses_out, t.stale_sq_io = _abi.ptr(x["perm"]), _abi.ptr(x["losses"]), _abi.ptr(x["stale"])
            t.sync_ws, t.cfg, t.active = _abi.ptr(x["sync_ws"]), cfg, 1

        def restore():
            for x in rs:
                x["theta"].copy_(x["theta0"]); x["m"].zero_(); x["v"].zero_(); x["stale"].fill_(0.5)

        def batched():
            _abi.check(lib.spo_critic_fit_iter_ks_multi(reps, S, M, _abi.stream_ptr()), "spo_critic_fit_iter_ks_multi")

        def single():
            for x in rs:
                _abi.check(lib.spo_critic_fit_iter_ks(
                    _abi.ptr(x["theta"]), _abi.ptr(x["m"]), _abi.ptr(x["v"]), 0, _abi.ptr(x["obs"]), _abi.ptr(x["tgt_r"]),
                    _abi.ptr(x["tgt_c"]), _abi.ptr(x["perm"]), M, cfg, _abi.ptr(x["stale"]), _abi.ptr(x["losses"]),
                    _abi.ptr(x["sync_ws"]), _abi.stream_ptr()), "spo_critic_fit_iter_ks")

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
                words = torch.stack([x["sync_ws"][8] for x in rs]).cpu().tolist()
                if any(words):                                    # (an exchange timed out: recorded, not hidden)
                    errs += 1
                    print("ERR", name, S, words, flush=True)
                    for x in rs:
                        x["sync_ws"][8] = 0
                if i >= warmup:
                    us[name].append(e0.elapsed_time(e1) * 1e3 / nst)
        entry["rows"].append({"S": S, "us": us, "err_calls": errs, "write_through_runs": wt, "batched_runs": (warmup + calls) * S})
        print(f"S {S} done", flush=True)
    print("RESULT " + json.dumps(entry))


def end_to_end_child(mode, seeds, log_root):
    """mode "batched": cpo.main with --seeds, --batch-critic-fit True and --batch-critic-fit-feature-split True; "sequential": one
    main() per seed, one after the other.  Two epochs each at the benchmark's size (the first carries the lazy set-up and the
    rollout-graph capture); the second epoch's Time/ columns are read.  In the sequential runs the critic fit is also timed by
    itself (a device synchronisation on either side of WideCPOEngine.critic_fit): its share of Time/Update."""
    import argparse as ap
    import csv
    import torch
    from safepo.single_agent import cpo

    def args(**kw):
        a = ap.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=N, experiment="e2e", log_dir=log_root, device="cuda",
                         device_id=0, write_terminal=True, headless=False, total_steps=2 * N * T, steps_per_epoch=N * T, randomize=False,
                         cost_limit=25.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035, cfg_override={},
                         env_kwargs={"obs_dim": 376, "act_dim": 17})
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def second_epoch(d):
        row = list(csv.DictReader(open(os.path.join(d, "progress.csv"))))[1]
        return {k: float(row[k]) for k in ("Time/Rollout", "Time/Update", "Time/Total")}

    t0 = time.time()
    fit_s = []
    if mode == "batched":
        dirs = [os.path.join(log_root, f"b{s}") for s in seeds]
        cpo.main(args(seeds=list(seeds), log_dirs=dirs, batch_critic_fit=True, batch_critic_fit_feature_split=True), {})
        rows = [second_epoch(d) for d in dirs]
        out = {"rollout_s": rows[0]["Time/Rollout"], "update_s": rows[0]["Time/Update"], "total_s": rows[0]["Time/Total"]}
    else:
        inner = cpo.WideCPOEngine.critic_fit

        def timed(self, perm_fn=None):
            torch.cuda.synchronize()
            t = time.time()
            out = inner(self, perm_fn)
            torch.cuda.synchronize()
            fit_s.append(time.time() - t)
            return out

        cpo.WideCPOEngine.critic_fit = timed
        rows = []
        for s in seeds:
            d = os.path.join(log_root, f"s{s}")
            cpo.main(args(seed=s, log_dir=d), {})
            rows.append(second_epoch(d))
        out = {k2: sum(r[k] for r in rows) for k, k2 in (("Time/Rollout", "rollout_s"), ("Time/Update", "update_s"), ("Time/Total", "total_s"))}
        out["critic_fit_s"] = sum(fit_s[1::2])                    # the second epoch's critic fit of every seed
    out.update(mode=mode, wall_s=time.time() - t0)
    print("RESULT " + json.dumps(out))


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


def decide(D, A, rows):
    """Per S: is the batched launch ahead of S sequential launches by more than three times the larger median - minimum spread?"""
    out = [f"{D}/{A}:"]
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
    lines = [f"hidden [64, 64], {N} x {T} = {N * T} rows per run, minibatches of {BATCH}: one critic-fit iteration = {N * T // BATCH} steps per run.",
             "us/step = one HIP event pair around the critic-fit iteration of ALL S runs / its steps (a step = every run advancing one minibatch);",
             "us/run-step = us/step / S.  single = S launches of spo_critic_fit_iter_ks back to back; batched = one spo_critic_fit_iter_ks_multi launch.",
             f"one process per shape, the two paths alternating call by call, {args.warmup} warm-up then {args.calls} timed calls each; "
             "median (minimum).",
             "rate = aggregate run-steps/s of batched over single (medians); wins = the batched median beats the single median by more "
             "than 3 x max(median - min) of the two sides; err = calls after which a run's error word was set; wt = runs of the batched "
             "launches whose placement census chose write-through stores.", ""]
    lines.append(f"{'obs/act':>8} {'S':>3} {'single us/step':>22} {'batched us/step':>22} {'single us/run-step':>20} "
                 f"{'batched us/run-step':>20} {'rate':>7} {'wins':>5} {'err':>4} {'wt':>4}")
    deciding = []
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for D, A, s_list in CASES:
        e = run_child(["--child", f"{D},{A}," + "/".join(map(str, s_list)), "--calls", str(args.calls), "--warmup", str(args.warmup)],
                      args.child_timeout)
        for row in e["rows"]:
            S = row["S"]
            (sm, sl), (bm, bl) = stats(row["us"]["single"]), stats(row["us"]["batched"])
            win = (sm - bm) > 3 * max(sm - sl, bm - bl)
            lines.append(f"{D:>4}/{A:<3} {S:>3} {sm:13.2f} ({sl:6.2f}) {bm:13.2f} ({bl:6.2f}) {sm / S:12.3f} ({sl / S:6.3f}) "
                         f"{bm / S:12.3f} ({bl / S:6.3f}) {sm / bm:6.2f}x {'yes' if win else 'NO':>5} {row['err_calls']:>4} "
                         f"{row['write_through_runs']:>4}")
        print(f"{D}/{A} done", flush=True)
        deciding.append(decide(D, A, e["rows"]))
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
    lines = ["", f"END TO END: cpo on SynthSafe-v0 at 376 / 17, {N} envs x {T} steps per epoch, default configuration, eight seeds; the "
             "SECOND epoch of every run (the first carries lazy set-up and the rollout-graph capture), from the loggers' Time/ columns.",
             "sequential = eight `--seed` runs one after the other in one process (columns summed over the runs); batched = one `--seeds ... "
             "--batch-critic-fit True --batch-critic-fit-feature-split True` run (the columns hold the phase's wall time for all eight "
             "seeds).  One sample each: no spread was measured.",
             f"{'':>12} {'Time/Rollout s':>15} {'Time/Update s':>15} {'Time/Total s':>14}",
             f"{'sequential':>12} {q['rollout_s']:15.3f} {q['update_s']:15.3f} {q['total_s']:14.3f}",
             f"{'batched':>12} {b['rollout_s']:15.3f} {b['update_s']:15.3f} {b['total_s']:14.3f}",
             f"{'ratio':>12} {q['rollout_s'] / b['rollout_s']:14.2f}x {q['update_s'] / b['update_s']:14.2f}x {q['total_s'] / b['total_s']:13.2f}x",
             "",
             f"SHARE of the critic fit in Time/Update, stand-alone (the sequential runs above; WideCPOEngine.critic_fit timed by itself "
             f"between two device synchronisations, second epoch, summed over the eight seeds): {q['critic_fit_s']:.3f} s of "
             f"{q['update_s']:.3f} s = {100.0 * q['critic_fit_s'] / q['update_s']:.1f} %.  One sample.", ""]
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
    a = ap.parse_args()
    assert a.calls >= 16, "at least 16 timed calls"
    if a.child:
        d_, a_, s_ = a.child.split(",")
        child(int(d_), int(a_), [int(x) for x in s_.split("/")], a.calls, a.warmup)
    elif a.e2e_child:
        end_to_end_child(a.e2e_child, a.e2e_seeds, a.e2e_dir)
    elif a.end_to_end:
        end_to_end(a)
    else:
        parent(a)
