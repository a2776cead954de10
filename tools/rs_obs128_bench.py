"""Development aid (GPU box): the PPO-Lagrangian minibatch step at Car / Doggo / largest-supported dims on the row-split kernel's
KIN = 128 form (csrc/update_rs.hip, spo_update_rs128_supported) against the routing before it (SPO_RS_OBS128=0: the four-wave
kernel), over a 4096 x 128 buffer:
    python tools/rs_obs128_bench.py [--calls 24] [--warmup 3] [--out profiles/rs_obs128/step_times.txt]
    python tools/rs_obs128_bench.py --resource-usage        # no GPU: registers / spills / scratch of the kernels -> resource_usage.txt
One child process per shape; inside it the two routings ALTERNATE launch by launch (the C side reads SPO_RS_OBS128 at every
launch).  A sample is a HIP event pair around ONE launch -- 8 192 steps of 64 rows (spo_ppo_lag_update_iter, three networks; the
window includes the engine's closing error check) -- and parameters and optimiser state are put back outside the timed window.
(The critic fit's four-row-group form at these dims was measured with an earlier version of this tool, lost and was removed:
DESIGN_NOTES.md.)  Reported per shape and call: median and minimum in microseconds per step of either routing, and
whether the new form's median beats the other's by more than the larger median - minimum spread of the two sides."""
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
ITEMS = ["ppo_lag_step"]
OUT_DIR = os.path.join(ROOT, "profiles", "rs_obs128")


def child(D, A, calls, warmup):
    import ctypes
    import torch
    from safepo import _abi
    from safepo.common.engine import PPOLagEngine
    from safepo.common.model import ActorVCritic
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    lib = _abi.load()
    M = N * T
    g = torch.Generator(device=dev).manual_seed(1)

    def counters():
        c4 = (ctypes.c_ulonglong * 4)()
        _abi.check(lib.spo_debug_update_counters(c4, 1), "counters")
        return int(c4[0])

    def fill(eng):
        b = eng.buffer
        for k in ("obs", "act", "target_value_r", "target_value_c"):
            b.data[k].normal_(generator=g)
        b.data["log_prob"].copy_(-A * 0.92 - 0.5 * (b.data["act"] ** 2).sum(-1) + 0.1 * torch.randn(N, T, device=dev, generator=g))

    def time_pair(sides, steps):
        """sides: {name: (env, call, restore, expected row-split steps)}; alternates them; returns {name: [us per step]}."""
        us = {k: [] for k in sides}
        for i in range(warmup + calls):
            for name, (env, call, restore, want) in sides.items():
                restore()
                for k, v in env.items():
                    os.environ[k] = v
                counters()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                assert counters() == want, (name, want)
                if i >= warmup:
                    us[name].append(e0.elapsed_time(e1) * 1e3 / steps)
        return us

    entry = {"obs_dim": D, "act_dim": A, "us": {}}
    # ---- the PPO-Lagrangian step: one engine, the knob alone selects the kernel
    torch.manual_seed(D)
    pol = ActorVCritic(D, A).to(dev)
    cfg = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 1e9, "batch_size": 64, "learning_iters": 1, "max_grad_norm": 40.0}
    eng = PPOLagEngine(pol, N, T, cfg, dev)
    fill(eng)
    eng.buffer.adv_mix.normal_(generator=g)
    perm = torch.randperm(M, device=dev, generator=g).to(torch.int32)
    theta0 = pol.theta.clone()

    def restore():
        pol.theta.copy_(theta0); eng.adam_m.zero_(); eng.adam_v.zero_(); eng.adam_step = 0

    def step():
        eng.learning_iter(perm)
        eng.check_sync_error()

    nst = M // 64
    entry["us"]["ppo_lag_step"] = time_pair({"new": ({"SPO_RS_OBS128": "1"}, step, restore, nst),
                                             "old": ({"SPO_RS_OBS128": "0"}, step, restore, 0)}, nst)
    del eng, pol
    print("RESULT " + json.dumps(entry))


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
            m2 = re.search(r"ppo_update_rs_kernel<[^>]*>", name or text)
            cur = {"name": m2.group(0) if m2 else (name or text)}
            rows.append(cur)
        elif cur is not None and ":" in text:
            k, val = text.split(":", 1)
            cur[k.strip()] = val.strip()
    keys = ["VGPRs", "AGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]
    lines = ["kernel-resource-usage of csrc/update_rs.hip (gfx950), ppo_update_rs_kernel<KIN, R, PROF, XW, NCT>: the KIN = 128 instantiation "
             "and, for comparison, the KIN = 64 one of the same form (R = 2 row groups, XW = 0: one GPU, NCT = 2).",
             "LDS is taken dynamically (LDS Size shows the static part, 0): RsLds<128, 2> = 132 864 bytes, RsLds<64, 2> = 98 048 bytes "
             "of the 163 840."]
    for row in rows:
        if re.match(r"ppo_update_rs_kernel<(128|64), 2, false, 0, 2>", row["name"]):
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


def parent(args):
    lines = [f"hidden [64, 64], buffer {N} x {T} = {N * T} rows; microseconds PER MINIBATCH STEP = one launch's HIP event pair / its steps "
             f"(ppo_lag_step: 8 192 steps of 64 rows, three networks);",
             f"one process per shape, the two routings alternating launch by launch, {args.warmup} warm-up then {args.calls} timed launches each",
             "old = SPO_RS_OBS128=0 (the routing before the KIN = 128 form: the four-wave kernel); new = default (row-split kernel, KIN = 128)",
             "wins = new median < old median by more than max(median - min) of the two sides", ""]
    lines.append(f"{'obs/act':>8} {'call':<16} {'old median':>11} {'old min':>9} {'new median':>11} {'new min':>9} {'speed-up':>9}  wins")
    for D, A in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{D},{A}", "--calls", str(args.calls), "--warmup", str(args.warmup)],
                           capture_output=True, text=True, timeout=args.child_timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            raise SystemExit(f"child {D}/{A} failed with {r.returncode}")          # (nothing more is started on the GPU)
        e = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        for k in ITEMS:
            if k not in e["us"]:
                continue
            (om, ol), (nm, nl) = stats(e["us"][k]["old"]), stats(e["us"][k]["new"])
            win = (om - nm) > max(om - ol, nm - nl)
            lines.append(f"{D:>4}/{A:<3} {k:<16} {om:11.2f} {ol:9.2f} {nm:11.2f} {nl:9.2f} {om / nm:8.2f}x  {'yes' if win else 'NO'}")
        print(f"shape {D}/{A} done", flush=True)
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(OUT_DIR, "step_times.txt"))
    ap.add_argument("--child", default="")
    ap.add_argument("--resource-usage", action="store_true")
    a = ap.parse_args()
    assert a.calls >= 24, "at least 24 timed launches"
    if a.resource_usage:
        resource_usage()
    elif a.child:
        d_, a_ = (int(x) for x in a.child.split(","))
        child(d_, a_, a.calls, a.warmup)
    else:
        parent(a)
