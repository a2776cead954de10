"""Development aid (GPU box): the three full-batch CPO primitives and one whole policy_update of WideCPOEngine at Car / Doggo /
largest-supported dims, on the KIN = 128 LDS-resident kernels (csrc/cpo.hip, spo_cpo128_*) and on the chunked wide path
(SPO_CPO_OBS128=0), M = 4096 x 128 rows:
    python tools/cpo_obs128_bench.py [--calls 24] [--warmup 3] [--rounds 2] [--out profiles/cpo_obs128/primitives.txt]
    python tools/cpo_obs128_bench.py --resource-usage        # no GPU: registers / spills / scratch of the kernels -> resource_usage.txt
Every setting runs in a fresh child process (the knob is read when the engine is built), the two settings alternate `rounds` times
and their samples are pooled.  A sample is a HIP event pair around ONE call (for policy_update that includes its host
synchronisations: the line search reads its sums back); the parameters are restored outside the timed window.  Reported per
shape and item: median and min in microseconds of either path, and whether the new path wins by more than the larger
median - min spread of the two sides."""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "safe-policy-optimization_amd"))

SHAPES = [(72, 2), (104, 12), (128, 16)]
N, T = 4096, 128
ITEMS = ["surrogate_grad", "fvp", "linesearch_sums", "policy_update"]
OUT_DIR = os.path.join(ROOT, "profiles", "cpo_obs128")


def child(calls, warmup):
    import torch
    from safepo.common.model import ActorVCritic
    from safepo.single_agent import cpo
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    res = []
    for D, A in SHAPES:
        torch.manual_seed(D)
        pol = ActorVCritic(D, A).to(dev)
        eng = cpo.make_engine(pol, N, T, dict(cpo.default_cfg), dev)
        assert type(eng) is cpo.WideCPOEngine
        g = torch.Generator(device=dev).manual_seed(1)
        b = eng.buffer
        for k in ("obs", "act", "adv_r"):
            b.data[k].normal_(generator=g)
        b.data["log_prob"].copy_(-A * 0.92 - 0.5 * (b.data["act"] ** 2).sum(-1) + 0.1 * torch.randn(N, T, device=dev, generator=g))
        b.data["adv_c"].copy_(b.data["adv_r"].flip(0) * 0.5 + 0.1)
        v = torch.randn(eng.Pa, device=dev, generator=g)
        theta0 = pol.theta.clone()
        eng.snapshot_old_distribution()
        runs = {
            "surrogate_grad": lambda: eng._surrogate_grad_local(b.data["adv_r"], -1.0),
            "fvp": lambda: eng._fvp_local(v),
            "linesearch_sums": lambda: eng._linesearch_sums_local(b.data["adv_r"], b.data["adv_c"]),
            "policy_update": lambda: eng.policy_update(-1.0),
        }
        entry = {"obs_dim": D, "act_dim": A, "rows": N * T, "new_path": bool(eng._actor_on_full_batch_kernels), "us": {}}
        for name in ITEMS:
            us = []
            for i in range(warmup + calls):
                pol.theta.copy_(theta0)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = runs[name]()
                e1.record()
                torch.cuda.synchronize()
                if i >= warmup:
                    us.append(e0.elapsed_time(e1) * 1e3)
            entry["us"][name] = us
            if name == "policy_update":
                entry["case"], entry["acceptance_step"] = int(out["case"]), int(out["acceptance_step"])
        res.append(entry)
        del eng, pol
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(res))


def resource_usage():
    """hipcc -Rpass-analysis=kernel-resource-usage on csrc/cpo.hip with the build's own flags (cross-compiles; no GPU)."""
    import __graft_entry__ as ge
    src = os.path.join(ge.CSRC, "cpo.hip")
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [ge._hipcc()] + ge.HIPCC_FLAGS + ge.EXTRA_FLAGS.get("cpo.hip", []) + ["-Rpass-analysis=kernel-resource-usage", "-c", src,
                                                                                    "-o", os.path.join(tmp, "cpo.o")]
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
            cur = {"name": name or text}
            rows.append(cur)
        elif cur is not None and ":" in text:
            k, val = text.split(":", 1)
            cur[k.strip()] = val.strip()
    keys = ["VGPRs", "AGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]
    lines = ["kernel-resource-usage of csrc/cpo.hip (gfx950; LDS Size is the static part: cpo_actor_kernel takes its own dynamically: 147 776 B in mode 0, 151 680 B in mode 2)"]
    for row in rows:
        if "128" in row["name"] or "reduce" in row["name"] or "sum3" in row["name"]:
            lines.append(row["name"])
            lines.append("    " + "  ".join(f"{k}: {row.get(k, '?')}" for k in keys))
    os.makedirs(OUT_DIR, exist_ok=True)
    path = os.path.join(OUT_DIR, "resource_usage.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", path)


def stats(us):
    s = sorted(us)
    return s[len(s) // 2], s[0]


def parent(args):
    pooled = {"0": None, "1": None}
    for rnd in range(args.rounds):
        for knob in ("0", "1"):
            env = dict(os.environ, SPO_CPO_OBS128=knob)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--warmup", str(args.warmup)],
                               env=env, capture_output=True, text=True, timeout=args.child_timeout)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"child SPO_CPO_OBS128={knob} failed with {r.returncode}")
            res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            for e in res:
                assert e["new_path"] == (knob == "1"), e
            if pooled[knob] is None:
                pooled[knob] = res
            else:
                for a, e in zip(pooled[knob], res):
                    for k in ITEMS:
                        a["us"][k] += e["us"][k]
            print(f"round {rnd} SPO_CPO_OBS128={knob} done", flush=True)
    lines = [f"WideCPOEngine, hidden [64, 64], M = {N} x {T} = {N * T} rows; microseconds per call, HIP event pair around one call, "
             f"{args.warmup} warm-up calls then {args.calls} timed calls per child process, {args.rounds} alternating rounds pooled",
             "wide = SPO_CPO_OBS128=0 (launch-per-layer wide kernels in row chunks: the path before the KIN = 128 kernels); "
             "new = default (spo_cpo128_*)",
             "wins = new median < wide median by more than max(median - min) of the two sides", ""]
    lines.append(f"{'obs/act':>8} {'item':<16} {'wide median':>12} {'wide min':>10} {'new median':>11} {'new min':>9} {'speed-up':>9}  wins")
    all_win = True
    for old, new in zip(pooled["0"], pooled["1"]):
        for k in ITEMS:
            (om, ol), (nm, nl) = stats(old["us"][k]), stats(new["us"][k])
            win = (om - nm) > max(om - ol, nm - nl)
            all_win &= win
            lines.append(f"{old['obs_dim']:>4}/{old['act_dim']:<3} {k:<16} {om:12.1f} {ol:10.1f} {nm:11.1f} {nl:9.1f} {om / nm:8.2f}x  {'yes' if win else 'NO'}")
        lines.append(f"{'':>8} policy_update: case {old['case']} / acceptance step {old['acceptance_step']} (wide), "
                     f"case {new['case']} / acceptance step {new['acceptance_step']} (new)")
    lines += ["", "every primitive and the whole step win at every shape" if all_win else "NOT every item wins: see the NO rows", ""]
    ru = os.path.join(OUT_DIR, "resource_usage.txt")
    if os.path.exists(ru):
        lines += open(ru).read().splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(OUT_DIR, "primitives.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--resource-usage", action="store_true")
    a = ap.parse_args()
    assert a.calls >= 20, "at least 20 timed calls"
    if a.resource_usage:
        resource_usage()
    elif a.child:
        child(a.calls, a.warmup)
    else:
        parent(a)
