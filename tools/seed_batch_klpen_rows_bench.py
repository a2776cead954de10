"""Development aid (GPU box): the seed-batched row-group step of FOCOPS / CUP (spo_wide_rows_ex_step_multi, csrc/mlp_rows.hip +
csrc/wide.hip; S independent runs as slices blockIdx.y of the step's five launches, replayed from one captured graph) against S
stand-alone engines' graph replays back to back, over 4096 x 128-row buffers at batch 64:
    python tools/seed_batch_klpen_rows_bench.py [--calls 16] [--warmup 1] [--hidden 128x128 256x256] [--kinds focops cup1 cup2] [--s-list 1 2 4 8 16 32]
    python tools/seed_batch_klpen_rows_bench.py --end-to-end         # focops --seeds --batch-update True --batch-klpen-rows True at S = 8 against eight runs -> appended
    python tools/seed_batch_klpen_rows_bench.py --resource-usage     # no GPU: registers / scratch / load kinds of the new kernels -> resource_usage.txt
    python tools/seed_batch_klpen_rows_bench.py --isa-compare REV    # no GPU: this tree's csrc/mlp_rows.hip and csrc/wide.hip against git revision REV's -> kernel_isa_compare.txt
60 / 8 with hidden [128, 128] and [256, 256], S = 1 / 2 / 4 / 8 / 16 / 32, the step's three kinds: focops (KL penalty, critics + actor),
cup1 (CUP's first stage: the clipped surrogate), cup2 (CUP's second stage: KL penalty, the actor alone).  One child process per
(shape, kind), each under a time limit of its own; inside it, for every S, the two paths ALTERNATE call by call.  A sample is a HIP
event pair around one learning iteration of all S runs (8 192 steps of 64 rows each): PPOLagEngineGroup(klpen_rows=True)
.learning_iter_ex_all, or S WidePPOLagEngine.learning_iter_ex calls enqueued back to back; parameters, optimiser state and clocks are
put back outside the timed window.  Both paths include their per-pass host work (the clocks' and the permutation's upload; the
batched path's table upload).  A run of this tool that covers only part of the protocol says so in what it writes."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "safe-policy-optimization_amd"))

D, A = 60, 8
S_LIST = [1, 2, 4, 8, 16, 32]
N, T, BATCH = 4096, 128, 64
KINDS = {"focops": (1, False), "cup1": (0, False), "cup2": (1, True)}        # kind -> (actor_loss, actor_only)
OUT_DIR = os.path.join(ROOT, "profiles", "seed_batch_klpen_rows")
SOURCES = ("mlp_rows.hip", "wide.hip")


def child(hidden, kind, s_list, calls, warmup):
    import torch
    from safepo.common.engine import WidePPOLagEngine
    from safepo.common.engine_group import PPOLagEngineGroup
    from safepo.common.model import ActorVCritic
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    M = N * T
    nst = M // BATCH
    actor_loss, actor_only = KINDS[kind]
    g = torch.Generator(device=dev).manual_seed(1)
    cfg = {"hidden_sizes": hidden, "gamma": 0.99, "target_kl": 0.02, "batch_size": BATCH, "learning_iters": 1, "max_grad_norm": 40.0}
    engines, perms, theta0, advs = [], [], [], []
    for r in range(max(s_list)):
        torch.manual_seed(D + r)
        pol = ActorVCritic(D, A, hidden_sizes=hidden).to(dev)
        eng = WidePPOLagEngine(pol, N, T, cfg, dev)
        assert eng._row_group_step_ok(BATCH, actor_loss, actor_only) and not eng._feature_split_kernel_ok(eng._cfg_struct())
        b = eng.buffer
        for k in ("obs", "act", "target_value_r", "target_value_c"):
            b.data[k].normal_(generator=g)
        b.data["log_prob"].copy_(-A * 0.92 - 0.5 * (b.data["act"] ** 2).sum(-1) + 0.1 * torch.randn(N, T, device=dev, generator=g))
        b.adv_mix.normal_(generator=g)
        eng.snapshot_old_distribution()
        engines.append(eng)
        advs.append(b.adv_mix)
        perms.append(torch.randperm(M, device=dev, generator=g).to(torch.int32))
        theta0.append(pol.theta.clone())
    for S in s_list:
        es = engines[:S]
        group = PPOLagEngineGroup(es, klpen_rows=True)
        assert group._rows and group.batched_ex(actor_loss, None, actor_only)
        kl_bounds, pg_coefs = [0.02] * S, [1.0 / 1.5] * S

        def restore():
            for e, t0 in zip(es, theta0):
                e.policy.theta.copy_(t0); e.adam_m.zero_(); e.adam_v.zero_(); e.adam_step = 0; e.adam_step_actor_extra = 0

        def batched():
            group.learning_iter_ex_all(perms[:S], advs[:S], actor_loss, kl_bounds, pg_coefs, actor_only)

        def single():
            for e, p, adv in zip(es, perms, advs):
                e.learning_iter_ex(p, adv, actor_loss, 0.02, 1.0 / 1.5, actor_only)

        us = {"batched": [], "single": []}
        for i in range(warmup + calls):
            for name, call in (("single", single), ("batched", batched)):
                restore()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                if i >= warmup:
                    us[name].append(e0.elapsed_time(e1) * 1e3 / nst)
            print(f"hidden {hidden} {kind} S {S} call {i}", flush=True)
        print("ROW " + json.dumps({"hidden": hidden, "kind": kind, "S": S, "us": us}), flush=True)


def end_to_end_child(mode, seeds, log_root):
    """mode "batched": focops.main with --seeds, --hidden-sizes 128 128, --batch-update True and --batch-klpen-rows True;
    "sequential": one main() per seed, one after the other.  Two epochs each at the benchmark's size; the second epoch's Time/
    columns are read."""
    import argparse as ap
    import csv
    from safepo.single_agent import focops

    def args(**kw):
        a = ap.Namespace(seed=0, use_eval=False, task="SynthSafe-v0", num_envs=N, experiment="e2e", log_dir=log_root, device="cuda",
                         device_id=0, write_terminal=True, headless=False, total_steps=2 * N * T, steps_per_epoch=N * T, randomize=False,
                         cost_limit=25.0, lagrangian_multiplier_init=0.001, lagrangian_multiplier_lr=0.035, cfg_override={},
                         env_kwargs={"obs_dim": D, "act_dim": A}, hidden_sizes=[128, 128], batch_update=False, batch_klpen_rows=False)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def second_epoch(d):
        row = list(csv.DictReader(open(os.path.join(d, "progress.csv"))))[1]
        return {k: float(row[k]) for k in ("Time/Rollout", "Time/Update", "Time/Total", "Train/StopIter")}

    t0 = time.time()
    if mode == "batched":
        dirs = [os.path.join(log_root, f"b{s}") for s in seeds]
        focops.main(args(seeds=list(seeds), log_dirs=dirs, batch_update=True, batch_klpen_rows=True), {})
        rows = [second_epoch(d) for d in dirs]
        out = {"rollout_s": rows[0]["Time/Rollout"], "update_s": rows[0]["Time/Update"], "total_s": rows[0]["Time/Total"]}
    else:
        rows = []
        for s in seeds:
            d = os.path.join(log_root, f"s{s}")
            focops.main(args(seed=s, log_dir=d), {})
            rows.append(second_epoch(d))
        out = {k2: sum(r[k] for r in rows) for k, k2 in (("Time/Rollout", "rollout_s"), ("Time/Update", "update_s"), ("Time/Total", "total_s"))}
    out.update(mode=mode, stop_iters=[r["Train/StopIter"] for r in rows], wall_s=time.time() - t0)
    print("RESULT " + json.dumps(out))


# ---------------------------------------------------------------------------------------------------- no GPU: the compiled kernels
def _device_asm(src, include_dir):
    """(kernels: demangled name -> instruction lines, resource remarks: demangled name -> dict) of one .hip file's device code."""
    import tempfile
    import __graft_entry__ as ge
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        cmd = [ge._hipcc()] + ge.HIPCC_FLAGS + ge.EXTRA_FLAGS.get(os.path.basename(src), []) + [
            "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-I", include_dir, src, "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr)
        lines = open(out).read().split("\n")
    names = [m.group(1) for line in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)] if m]
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    dem = {n: p.strip().replace("(anonymous namespace)::", "") for n, p in zip(names, plain)}
    kernels = {}
    for name in names:
        st = next(k for k, line in enumerate(lines) if line.startswith(name + ":"))
        en = next(k for k in range(st, len(lines)) if lines[k].startswith(".Lfunc_end"))
        body = []
        for line in lines[st + 1:en]:
            line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
            if line and name not in line:
                body.append(line)
        kernels[dem[name]] = body
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            n = text.split(":", 1)[1].strip()
            cur = None
            if n in dem:
                cur = res[dem[n]] = {}
        elif cur is not None and ":" in text:
            k, val = text.rsplit(":", 1)
            cur[k.strip()] = val.strip()
    return kernels, res


def _parent_name(d):
    """The name a MULTI = false instantiation had before its kernel took the MULTI template parameter."""
    d = re.sub(r"^void mlp_rows_klpen_reduce_kernel<false>\(MrRedArg<false>::Kl\)", "mlp_rows_klpen_reduce_kernel(MrKlReduceArgs)", d)
    return re.sub(r"wide_adam_kernel<(true|false), false>\(WideKernArg<false>::AdamEx, ", r"wide_adam_kernel<\1>(WideAdamExArgs, ", d)


def isa_compare(rev):
    import tempfile
    import __graft_entry__ as ge
    sha = lambda body: hashlib.sha256("\n".join(body).encode()).hexdigest()[:12]
    lines = [
        "csrc/mlp_rows.hip and csrc/wide.hip, hipcc " + " ".join(ge.HIPCC_FLAGS) + f", device assembly (-S) of revision {rev} (the parent) and of",
        "this tree, kernel by kernel: the instruction text and the kernel descriptor's directives between the kernel's label and its end,",
        "comments and blank lines dropped, function-local labels renumbered (.LBB<n>_<k> -> .LBB_<k>), lines that only name the kernel",
        "dropped.  Two stand-alone kernels took a defaulted MULTI template parameter, which changes their mangled names and nothing else:",
        "mlp_rows_klpen_reduce_kernel<false>(MrRedArg<false>::Kl) is compared with the parent's mlp_rows_klpen_reduce_kernel(MrKlReduceArgs),",
        "wide_adam_kernel<C, false>(WideKernArg<false>::AdamEx, ...) with wide_adam_kernel<C>(WideAdamExArgs, ...).  sha = first 12 hex",
        "digits of the SHA-256 of the text; same = equal text AND equal resource remarks (registers, scratch, occupancy, LDS); scratch =",
        "ScratchSize [bytes/lane].", ""]
    total_same = total_parent = 0
    for src in SOURCES:
        rel = "safe-policy-optimization_amd/csrc/" + src
        with tempfile.TemporaryDirectory() as tmp:
            old = os.path.join(tmp, src)
            with open(old, "w") as f:
                f.write(subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{rel}"], capture_output=True, text=True, check=True).stdout)
            pk, pres = _device_asm(old, ge.CSRC)
        tk, tres = _device_asm(os.path.join(ge.CSRC, src), ge.CSRC)
        rows, same, new = [], 0, 0
        for d, body in tk.items():
            sc = tres[d].get("ScratchSize [bytes/lane]")
            p = _parent_name(d)
            if p in pk:
                ok = pk[p] == body and pres[p] == tres[d]
                same += ok
                rows.append((d, len(body), sha(pk[p]), sha(body), "yes" if ok else "NO", f"{pres[p].get('ScratchSize [bytes/lane]')}/{sc}"))
            else:
                new += 1
                rows.append((d, len(body), "-", sha(body), "new", f"-/{sc}"))
        gone = [p for p in pk if p not in {_parent_name(d) for d in tk}]
        w = min(max(len(r[0]) for r in rows), 96) + 2
        lines += ["csrc/" + src, f"{'kernel':<{w}}{'lines':>7}{'parent sha':>14}{'this sha':>14}{'same':>6}{'scratch p/t':>13}"]
        lines += [f"{r[0][:w - 2]:<{w}}{r[1]:>7}{r[2]:>14}{r[3]:>14}{r[4]:>6}{r[5]:>13}" for r in rows]
        lines += ["", f"{same} of {len(pk)} kernels of the parent compile to the same instruction text and resource figures; {new} new kernels; "
                  f"{len(gone)} gone.", ""]
        total_same += same
        total_parent += len(pk)
        assert same == len(pk) and not gone, f"{src}: an existing kernel's code changed"
    lines.append(f"Both files: {total_same} of {total_parent} parent kernels same.")
    _write("kernel_isa_compare.txt", lines)


NEW_KERNELS = ("mlp_rows_grad_kernel<true, 1, true>", "mlp_rows_grad_kernel<false, 1, true>", "mlp_rows_klpen_reduce_kernel<true>",
               "mlp_rows_reduce_multi_kernel", "wide_prep_multi_kernel", "wide_prep_range_multi_kernel", "wide_coef_multi_kernel",
               "wide_adam_kernel<true, true>")
STANDALONE_OF = ("mlp_rows_grad_kernel<true, 1, false>", "mlp_rows_grad_kernel<false, 1, false>", "mlp_rows_klpen_reduce_kernel<false>",
                 "mlp_rows_reduce_kernel(", "wide_prep_kernel(", "wide_prep_range_kernel(", "wide_coef_kernel(", "wide_adam_kernel<true, false>")


def resource_usage():
    import __graft_entry__ as ge
    keys = ["VGPRs", "AGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
            "LDS Size [bytes/block]"]
    lines = ["kernel-resource-usage of csrc/mlp_rows.hip and csrc/wide.hip (gfx950, cross-compiled): the kernels of the row-group FOCOPS / CUP",
             "step, each stand-alone kernel (arguments in the kernel-argument segment) followed by its seed-batched form (run blockIdx.y's",
             "arguments read from a device table).  The gradient kernel's LDS is dynamic (the shape's images and the rows' old distribution, up",
             "to 160 KB; LDS Size shows the static part).  Behind the remarks: instruction counts by kind.  The table itself is read with",
             "scalar loads (s_load_*: const __restrict__, uniform index); the pointers it holds are generic to the compiler, so the batched",
             "kernels address global memory with flat_* instead of global_* instructions (as the other table-driven kernels of this project",
             "do) -- no scratch in any of them.  (CUP's first stage uses mlp_rows_grad_kernel<V, 0, true> of profiles/seed_batch_rows/.)", ""]
    found = {}
    for src in SOURCES:
        tk, tres = _device_asm(os.path.join(ge.CSRC, src), ge.CSRC)
        for d, body in tk.items():
            found[d] = (body, tres[d])
    for old, new in zip(STANDALONE_OF, NEW_KERNELS):
        for tag in (old, new):
            d = next(k for k in found if tag in k)
            body, res = found[d]
            cnt = lambda p: sum(1 for line in body if line.startswith(p))
            lines.append(d)
            lines.append("    " + "  ".join(f"{k}: {res.get(k, '?')}" for k in keys))
            lines.append(f"    s_load_*: {cnt('s_load')}  global_*: {cnt('global_')}  flat_*: {cnt('flat_')}  scratch_*: {cnt('scratch_')}  "
                         f"v_mfma_*: {cnt('v_mfma')}  instruction lines: {sum(1 for line in body if not line.startswith('.'))}")
            assert int(res["ScratchSize [bytes/lane]"]) == 0 and int(res["VGPRs Spill"]) == 0, d
    _write("resource_usage.txt", lines)


def _write(name, lines):
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, name)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", path)


def stats(us):
    s = sorted(us)
    return s[len(s) // 2], s[0]


def _run_child(argv, limit):
    """One child under its own time limit (coreutils timeout), its output passed on line by line as it comes; -> (lines, error)."""
    p = subprocess.Popen(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + argv, stdout=subprocess.PIPE,
                         text=True)
    lines = []
    for line in p.stdout:
        lines.append(line.rstrip("\n"))
        if not line.startswith(("ROW ", "RESULT ")):
            print(line, end="", flush=True)
    rc = p.wait()
    return lines, (None if rc == 0 else (f"time limit of {limit} s" if rc in (124, 137) else f"exit status {rc}"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--hidden", nargs="+", default=["128x128", "256x256"])
    ap.add_argument("--kinds", nargs="+", default=list(KINDS), choices=list(KINDS))
    ap.add_argument("--s-list", type=int, nargs="+", default=S_LIST)
    ap.add_argument("--child-limit", type=int, default=900, help="seconds per (shape, kind) child")
    ap.add_argument("--out", default=os.path.join(OUT_DIR, "step_times.txt"))
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--resource-usage", action="store_true")
    ap.add_argument("--isa-compare", metavar="REV", default=None)
    ap.add_argument("--child", nargs=2, default=None, metavar=("HIDDEN", "KIND"))
    ap.add_argument("--e2e-child", default=None)
    ap.add_argument("--log-root", default=None)
    a = ap.parse_args()
    if a.child:
        return child([int(h) for h in a.child[0].split("x")], a.child[1], a.s_list, a.calls, a.warmup)
    if a.e2e_child:
        return end_to_end_child(a.e2e_child, [1000 * i for i in range(8)], a.log_root)
    if a.resource_usage:
        return resource_usage()
    if a.isa_compare:
        return isa_compare(a.isa_compare)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if a.end_to_end:
        import tempfile
        res = {}
        for mode in ("batched", "sequential"):
            with tempfile.TemporaryDirectory() as tmp:
                lines, err = _run_child(["--e2e-child", mode, "--log-root", tmp], a.child_limit)
            if err:                                   # (a fault or a hang: nothing more is started on the GPU)
                raise SystemExit(f"end-to-end child ({mode}) ended with {err}")
            res[mode] = json.loads(next(line for line in lines if line.startswith("RESULT "))[7:])
        b, s = res["batched"], res["sequential"]
        text = [f"", f"End to end, one sample each: focops on SynthSafe-v0 at {D} / {A}, --hidden-sizes 128 128, {N} envs x {T} steps, second epoch.",
                f"  --seeds (8 seeds) --batch-update True --batch-klpen-rows True: Time/Update {b['update_s']:.2f} s, Time/Rollout "
                f"{b['rollout_s']:.2f} s, Time/Total {b['total_s']:.2f} s (stop_iters {b['stop_iters']})",
                f"  eight --seed runs, summed:                                     Time/Update {s['update_s']:.2f} s, Time/Rollout "
                f"{s['rollout_s']:.2f} s, Time/Total {s['total_s']:.2f} s (stop_iters {s['stop_iters']})"]
        with open(a.out, "a") as f:
            f.write("\n".join(text) + "\n")
        print("\n".join(text))
        return
    text = [f"Seed-batched row-group FOCOPS / CUP step (spo_wide_rows_ex_step_multi) against S stand-alone WidePPOLagEngine passes back to back,",
            f"one MI355X, {D} / {A}, {N} x {T} rows, batch {BATCH}: us per minibatch step of ALL S runs (a pass is {N * T // BATCH} steps, graph-replayed,",
            f"eight steps per graph launch), medians of {a.calls} with the minima beside them, the two paths alternating call by call.",
            "Kinds: focops = KL penalty, critics + actor; cup1 = CUP's first stage (clipped surrogate); cup2 = CUP's second stage (KL penalty,",
            "the actor alone).  rate = single median / batched median: the aggregate step rate of the batched launches against the sequential",
            "ones.  spread = (median - minimum) / median, the larger of the two paths; a gain counts where rate - 1 exceeds three times it.",
            f"This run: hidden {a.hidden}, kinds {a.kinds}, S {a.s_list}; whatever of the protocol (hidden 128x128 and 256x256, all three kinds,",
            f"S {S_LIST}, 16 calls) is not listed below was not measured.", ""]
    for h in a.hidden:
        for kind in a.kinds:
            lines, err = _run_child(["--child", h, kind, "--calls", str(a.calls), "--warmup", str(a.warmup), "--s-list"]
                                    + [str(s) for s in a.s_list], a.child_limit)
            rows = [json.loads(line[4:]) for line in lines if line.startswith("ROW ")]
            text.append(f"hidden [{h.replace('x', ', ')}], {kind}")
            text.append(f"{'S':>4}{'single med':>12}{'min':>9}{'batched med':>13}{'min':>9}{'per run-step':>14}{'rate':>8}{'spread':>8}  gain")
            for row in rows:
                (sm, s0), (bm, b0) = stats(row["us"]["single"]), stats(row["us"]["batched"])
                spread = max((sm - s0) / sm, (bm - b0) / bm)
                rate = sm / bm
                text.append(f"{row['S']:>4}{sm:>12.2f}{s0:>9.2f}{bm:>13.2f}{b0:>9.2f}{bm / row['S']:>14.2f}{rate:>8.2f}{spread:>8.3f}  "
                            + ("yes" if rate - 1 > 3 * spread else ("LOSS" if 1 - rate > 3 * spread else "within noise")))
            if err:
                text.append(f"(the child ended with {err} after S = {[r['S'] for r in rows]}: nothing more was started on the GPU)")
            text.append("")
            with open(a.out, "w") as f:
                f.write("\n".join(text) + "\n")
            if err:
                print("\n".join(text))
                raise SystemExit(f"child {h} {kind}: {err}")
    print("\n".join(text))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
