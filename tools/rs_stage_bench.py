"""Development aid (GPU box): the row-split PPO-Lagrangian step (csrc/update_rs.hip) with STAGED minibatch inputs against the
parent commit's build of the library and against this build's in-kernel gather, over a 4096 x 128 buffer:
    python tools/rs_stage_bench.py --lib parent=PATH [--lib NAME=PATH ...] [--shapes 60,8 20,3] [--calls 16] [--warmup 3] [--out FILE]
In the manner of tools/rs_l1_pipe_bench.py: one child process per shape; inside it ALL sides alternate launch by launch (every
library is loaded into the same process and keeps its own scratch; the one engine calls through whichever is due).  A sample is a
HIP event pair around ONE call of spo_ppo_lag_update_iter -- 8 192 steps of 64 rows, three networks, the staging pre-pass of that
launch INSIDE the timed interval, the engine's closing error check included; parameters and optimiser state are put back outside it.
Sides: this build with SPO_RS_STAGE=1 (x^T of dW1 from the record), =2 (x^T kept as an LDS image) and =0 (in-kernel gather); every
other library once (a library without the knob ignores it).  Reported per side: median and minimum in microseconds per step, the
median - minimum spread, whether the parameters after the launch equal the first side's bit for bit, and against "parent":
keeps = the medians differ by more than 3 x the larger of the two spreads (DESIGN.md 3.3.2's rule)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "safe-policy-optimization_amd"))
N, T = 4096, 128


def child(D, A, libs, calls, warmup, mgn):
    import torch
    from safepo import _abi
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    this = _abi.load()
    sides = [(f"this stage={f}", this, f) for f in ("1", "2", "0")]
    for name, path in libs:
        lib = ctypes.CDLL(path)
        for sym, (res, args) in _abi.PROTOTYPES.items():          # (an older build lacks the newest entry points: bind what it has)
            fn = getattr(lib, sym, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, args
        sides.append((name, lib, "1"))
    M = N * T
    nst = M // 64
    g = torch.Generator(device=dev).manual_seed(1)
    torch.manual_seed(D)
    pol = ActorVCritic(D, A).to(dev)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": 64, "learning_iters": 1, "max_grad_norm": mgn}
    eng = PPOLagEngine(pol, N, T, cfg, dev)
    b = eng.buffer
    for k in ("obs", "act", "target_value_r", "target_value_c"):
        b.data[k].normal_(generator=g)
    b.data["log_prob"].copy_(-A * 0.92 - 0.5 * (b.data["act"] ** 2).sum(-1) + 0.1 * torch.randn(N, T, device=dev, generator=g))
    b.adv_mix.normal_(generator=g)
    perm = torch.randperm(M, device=dev, generator=g).to(torch.int32)
    theta0 = pol.theta.clone()
    us = {s[0]: [] for s in sides}
    after, redone, staged = {}, {}, {}
    c4 = (ctypes.c_ulonglong * 4)()
    for i in range(warmup + calls):
        for name, lib, form in sides:
            pol.theta.copy_(theta0); eng.adam_m.zero_(); eng.adam_v.zero_(); eng.adam_step = 0
            os.environ["SPO_RS_STAGE"] = form
            eng.lib = lib
            assert lib.spo_debug_update_counters(c4, 1) == 0
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.learning_iter(perm)
            eng.check_sync_error()
            e1.record()
            torch.cuda.synchronize()
            assert lib.spo_debug_update_counters(c4, 1) == 0 and int(c4[0]) == nst, (name, list(c4))
            redone[name] = int(c4[1])
            fn = getattr(lib, "spo_debug_rs_last_staged", None)
            staged[name] = int(fn()) if fn is not None else 0
            if i >= warmup:
                us[name].append(e0.elapsed_time(e1) * 1e3 / nst)
            if i == 0:
                after[name] = (pol.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone())
    first = sides[0][0]
    same = {k: all(torch.equal(x, y) for x, y in zip(v, after[first])) for k, v in after.items()}
    print("RESULT " + json.dumps({"obs_dim": D, "act_dim": A, "max_grad_norm": mgn, "us": us, "same_bits": same, "redone": redone,
                                  "staged": staged}))


def stats(v):
    s = sorted(v)
    return s[len(s) // 2], s[0]


def parent(args):
    libs = [x.split("=", 1) for x in args.lib]
    lines = [f"hidden [64, 64], buffer {N} x {T} rows; microseconds PER MINIBATCH STEP = one launch's HIP event pair / its 8 192 steps of 64 rows "
             "(spo_ppo_lag_update_iter, three networks; the staging pre-pass of the launch is inside the interval);",
             f"one process per shape, all sides alternating launch by launch, {args.warmup} warm-up then {args.calls} timed launches each; "
             f"max_grad_norm {args.max_grad_norm}",
             "this = the in-tree build; stage = SPO_RS_STAGE; form = spo_debug_rs_last_staged(); "
             "keeps = |median - parent's median| > 3 x max(median - min) of the two sides", ""]
    for name, path in libs:
        lines.append(f"  {name} = {os.path.relpath(os.path.abspath(path), ROOT)}")
    lines.append("")
    for shape in args.shapes:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, "--calls", str(args.calls), "--warmup", str(args.warmup),
                            "--max-grad-norm", str(args.max_grad_norm)] + [x for l in args.lib for x in ("--lib", l)],
                           capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            raise SystemExit(f"child {shape} failed with {r.returncode}")              # (nothing more is started on the GPU)
        e = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        base = "parent" if "parent" in e["us"] else None
        lines.append(f"obs / act {e['obs_dim']} / {e['act_dim']}")
        lines.append(f"  {'side':<20} {'form':>4} {'median':>8} {'min':>8} {'spread':>7} {'vs parent':>10} {'keeps':>6}  same bits  redone")
        for k, v in e["us"].items():
            m, lo = stats(v)
            if base and k != base:
                bm, bl = stats(e["us"][base])
                d = bm - m
                keeps = "yes" if abs(d) > 3 * max(bm - bl, m - lo) else "NO"
                rel = f"{100 * d / bm:+.2f} %"
            else:
                keeps, rel = "", ""
            lines.append(f"  {k:<20} {e['staged'][k]:>4} {m:8.3f} {lo:8.3f} {m - lo:7.3f} {rel:>10} {keeps:>6}  {str(e['same_bits'][k]):<9}  {e['redone'][k]}")
        lines.append("")
        print(f"shape {shape} done", flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="NAME=PATH of another build of libsafepo_hip.so (parent=... first)")
    ap.add_argument("--shapes", nargs="+", default=["60,8"])
    ap.add_argument("--calls", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-grad-norm", type=float, default=40.0)
    ap.add_argument("--child-timeout", type=int, default=400)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    assert a.calls >= 16, "at least 16 timed launches"
    if a.child:
        d_, a_ = (int(x) for x in a.child.split(","))
        child(d_, a_, [x.split("=", 1) for x in a.lib], a.calls, a.warmup, a.max_grad_norm)
    else:
        parent(a)
