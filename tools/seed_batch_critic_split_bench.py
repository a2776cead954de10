"""Development aid (GPU box): the seed-batched split critic fit (spo_critic_fit_iter_split_multi, csrc/update.hip; S independent
runs, each on its own four co-XCD workgroups, in ONE persistent launch) against S back-to-back single launches of
spo_critic_fit_iter_split -- the parent's path -- over 4096 x 128-row buffers, minibatches of 128 (two 64-row halves), 72 / 2:
    python tools/seed_batch_critic_split_bench.py [--calls 16] [--warmup 2] [--out profiles/seed_batch_critic_split/step_times.txt]
    python tools/seed_batch_critic_split_bench.py --end-to-end   # cpo --seeds (8 seeds, both flags) against eight --seed runs, 72 obs
One child process; inside it, for every S, the two paths ALTERNATE call by call.  A sample is a HIP event pair around one
critic-fit iteration of all S runs (4 096 steps of 128 rows each): one batched launch, or S single launches enqueued back to back;
parameters, optimiser state and the stale norm of both replicas are put back and the runs' error words are read outside the timed
window.  Reported per S: median and minimum of the window per step (one step = every run advancing one minibatch), the same per
replica-step, the aggregate rate of the batched launch relative to the single launches, whether the per-step difference exceeds
three times the larger median - minimum spread of the two sides (only then is a gain claimed), how many runs of the batched calls
took the shared-L2 body (the launch's third counter), and whether any call set an error word."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "safe-policy-optimization_amd"))

D, A = 72, 2
S_LIST = [1, 8, 16, 32]
N, T, BATCH = 4096, 128, 128
OUT_DIR = os.path.join(ROOT, "profiles", "seed_batch_critic_split")


def child(calls, warmup):
    import ctypes
    import torch
    from safepo import _abi
    from safepo.common.engine_group import CPOEngineGroup
    from safepo.common.model import ActorVCritic
    from safepo.single_agent.cpo import WideCPOEngine, make_engine
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = _abi.load()
    M = N * T
    nst = M // BATCH
    g = torch.Generator(device=dev).manual_seed(1)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 0.01, "batch_size": BATCH, "learning_iters": 1, "max_grad_norm": 40.0}

    def counters():
        c3 = (ctypes.c_ulonglong * 3)()
        _abi.check(lib.spo_debug_critic_fit_split_multi_counters(c3, 1), "split multi counters")
        return [int(x) for x in c3]

    engines, halves, theta0 = [], [], []      # (halves: the runs' shuffles, cut per call)
    for r in range(max(S_LIST)):
        torch.manual_seed(D + r)
        pol = ActorVCritic(D, A).to(dev)
        eng = make_engine(pol, N, T, cfg, dev)
        assert type(eng) is WideCPOEngine and eng._split_setup() is not None
        for k in ("obs", "target_value_r", "target_value_c"):
            eng.buffer.data[k].normal_(generator=g)
        engines.append(eng)
        halves.append(torch.randperm(M, device=dev, generator=g).to(torch.int32))
        theta0.append(pol.theta.clone())

    def single_iter(e, h):
        st, d = e._split_setup(), e.buffer.data
        p = h.view(nst, 128)                                      # (the halves are cut inside the window on both sides, as a run does)
        h0, h1 = p[:, :64].contiguous().view(-1), p[:, 64:].contiguous().view(-1)
        l0 = torch.empty((nst, 3), dtype=torch.float32, device=dev)
        l1 = torch.empty_like(l0)
        _abi.check(lib.spo_critic_fit_iter_split(
            _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v), _abi.ptr(st["theta1"]), _abi.ptr(st["m1"]),
            _abi.ptr(st["v1"]), e.adam_step, _abi.ptr(d["obs"]), _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]),
            _abi.ptr(h0), _abi.ptr(h1), M // 2, CPOEngineGroup._split_cfg(e), _abi.ptr(e.stale_sq), _abi.ptr(st["stale1"]),
            _abi.ptr(l0), _abi.ptr(l1), _abi.ptr(e.sync_ws), _abi.ptr(st["sync_ws"]), st["regions"], st["step"] & 0xFFFFFFFF,
            _abi.stream_ptr()), "spo_critic_fit_iter_split")
        st["step"] += nst
        e.adam_step += nst

    rows = []
    for S in S_LIST:
        es = engines[:S]
        group = CPOEngineGroup(es, split_form=True)
        assert group.batched_split()

        def restore():
            for e, t0 in zip(es, theta0):
                st = e._split_setup()
                e.policy.theta.copy_(t0); e.adam_m.zero_(); e.adam_v.zero_(); e.stale_sq.fill_(0.25); e.adam_step = 0
                st["theta1"].copy_(t0); st["m1"].zero_(); st["v1"].zero_(); st["stale1"].fill_(0.25)

        def batched():
            group.fit_iter_split_all(halves[:S])

        def single():
            for e, h in zip(es, halves):
                single_iter(e, h)

        def error_words():
            words = torch.stack([e.sync_ws[8] for e in es] + [e._split_setup()["sync_ws"][8] for e in es]).cpu().tolist()
            return [int(w) & 0xFFFFFFFF for w in words]

        us = {"batched": [], "single": []}
        l2_runs, errs = 0, 0
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
                launches, runs, l2 = counters()
                assert (launches, runs) == ((1, S) if name == "batched" else (0, 0)), (name, S, launches, runs)
                if any(error_words()):                            # (an exchange timed out: recorded, not hidden)
                    errs += 1
                    print("ERR", name, S, error_words(), flush=True)
                if i >= warmup:
                    us[name].append(e0.elapsed_time(e1) * 1e3 / nst)
                    l2_runs += l2
            if errs:
                break
        rows.append({"S": S, "us": us, "l2_runs": l2_runs, "batched_runs": S * calls, "err_calls": errs})
        print(f"S {S} done", flush=True)
        if errs:
            break                                                 # (nothing more is started after an error word)
    print("RESULT " + json.dumps({"rows": rows}))


def end_to_end_child(mode, seeds, log_root):
    """mode "batched": cpo.main with --seeds and both flags; "sequential": one main() per seed, one after the other.  Two epochs
    each at the benchmark's size (the first carries the lazy set-up); the second epoch's Time/ columns are read."""
    import argparse as ap
    import csv
    from safepo.single_agent import cpo

    def args(**kw):
        a = ap.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=N, experiment="e2e", log_dir=log_root, device="cuda",
                         device_id=0, write_terminal=True, headless=False, total_steps=2 * N * T, steps_per_epoch=N * T, randomize=False,
                         cost_limit=25.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035, cfg_override={},
                         env_kwargs={"obs_dim": D})
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def second_epoch(d):
        row = list(csv.DictReader(open(os.path.join(d, "progress.csv"))))[1]
        return {k: float(row[k]) for k in ("Time/Rollout", "Time/Update", "Time/Total")}

    t0 = time.time()
    if mode == "batched":
        dirs = [os.path.join(log_root, f"b{s}") for s in seeds]
        cpo.main(args(seeds=list(seeds), log_dirs=dirs, batch_critic_fit=True, batch_critic_fit_split=True), {})
        rows = [second_epoch(d) for d in dirs]
        out = {"rollout_s": rows[0]["Time/Rollout"], "update_s": rows[0]["Time/Update"], "total_s": rows[0]["Time/Total"]}
    else:
        rows = []
        for s in seeds:
            d = os.path.join(log_root, f"s{s}")
            cpo.main(args(seed=s, log_dir=d), {})
            rows.append(second_epoch(d))
        out = {k2: sum(r[k] for r in rows) for k, k2 in (("Time/Rollout", "rollout_s"), ("Time/Update", "update_s"), ("Time/Total", "total_s"))}
    out.update(mode=mode, wall_s=time.time() - t0)
    print("RESULT " + json.dumps(out))


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
            elif not line.startswith(("|", "-", "+")) and line.strip():      # (the loggers' tables are not passed on)
                print("  | " + line.rstrip()[:200], flush=True)
        rc = p.wait()
    finally:
        killer.cancel()
    if rc != 0 or result is None:
        raise SystemExit(f"child {argv} failed with {rc}")          # (nothing more is started on the GPU)
    return json.loads(result)


def parent(args):
    nst = N * T // BATCH
    lines = [f"split critic fit (n_nets 2, two replicas of 64 rows each), hidden [64, 64], {D} / {A}, {N} x {T} = {N * T} rows per run, "
             f"minibatches of {BATCH}: one iteration = {nst} steps per run.",
             "us/step = one HIP event pair around the iteration of ALL S runs / its steps (a step = every run advancing one minibatch);",
             "us/replica-step = us/step / S.  single = S launches of spo_critic_fit_iter_split back to back (the parent commit's path); "
             "batched = one spo_critic_fit_iter_split_multi launch.",
             f"one process, one GPU, the two paths alternating call by call, {args.warmup} warm-up then {args.calls} timed calls each; "
             "median (minimum).",
             "rate = aggregate replica-steps/s of batched over single (medians); wins = the per-step difference of the medians exceeds "
             "three times the larger (median - minimum) of the two sides, in favour of the batched launch;",
             "L2 = runs of the timed batched calls whose placement census chose the shared-L2 body / runs; err = calls after which a "
             "run's error word was set.", "",
             f"{'S':>3} {'single us/step':>22} {'batched us/step':>22} {'single us/rep-step':>20} {'batched us/rep-step':>20} {'rate':>7} "
             f"{'wins':>5} {'L2':>9} {'err':>4}"]
    e = run_child(["--child", "--calls", str(args.calls), "--warmup", str(args.warmup)], args.child_timeout)
    for row in e["rows"]:
        S = row["S"]
        if not row["us"]["single"] or not row["us"]["batched"]:
            lines.append(f"{S:>3} stopped on an error word before a timed call")
            continue
        (sm, sl), (bm, bl) = stats(row["us"]["single"]), stats(row["us"]["batched"])
        win = (sm - bm) > 3.0 * max(sm - sl, bm - bl)
        lines.append(f"{S:>3} {sm:13.2f} ({sl:6.2f}) {bm:13.2f} ({bl:6.2f}) {sm / S:12.3f} ({sl / S:6.3f}) {bm / S:12.3f} ({bl / S:6.3f}) "
                     f"{sm / bm:6.2f}x {'yes' if win else 'NO':>5} {row['l2_runs']:>4}/{row['batched_runs']:<4} {row['err_calls']:>4}")
    lines.append("")
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
    lines = ["", f"END TO END: cpo on SynthSafe-v0 with {D} observations, {N} envs x {T} steps per epoch, default configuration (batch 128, "
             "learning_iters 10), eight seeds; the SECOND epoch of every run (the first carries lazy set-up), from the loggers' Time/ columns.",
             "sequential = eight `--seed` runs one after the other in one process (columns summed over the runs); batched = one `--seeds "
             "... --batch-critic-fit True --batch-critic-fit-split True` run (the columns hold the phase's wall time for all eight seeds).  "
             "One sample each: no spread was measured.",
             f"{'':>12} {'Time/Rollout s':>15} {'Time/Update s':>15} {'Time/Total s':>14}",
             f"{'sequential':>12} {q['rollout_s']:15.3f} {q['update_s']:15.3f} {q['total_s']:14.3f}",
             f"{'batched':>12} {b['rollout_s']:15.3f} {b['update_s']:15.3f} {b['total_s']:14.3f}",
             f"{'ratio':>12} {q['rollout_s'] / b['rollout_s']:14.2f}x {q['update_s'] / b['update_s']:14.2f}x {q['total_s'] / b['total_s']:13.2f}x", ""]
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=540)
    ap.add_argument("--out", default=os.path.join(OUT_DIR, "step_times.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--e2e-child", default="")
    ap.add_argument("--e2e-dir", default="")
    ap.add_argument("--e2e-seeds", type=int, nargs="+", default=[])
    a = ap.parse_args()
    assert a.calls >= 16, "at least 16 timed calls"
    if a.child:
        child(a.calls, a.warmup)
    elif a.e2e_child:
        end_to_end_child(a.e2e_child, a.e2e_seeds, a.e2e_dir)
    elif a.end_to_end:
        end_to_end(a)
    else:
        parent(a)
