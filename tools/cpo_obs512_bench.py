"""Development aid (GPU box): the three full-batch CPO primitives and one whole policy_update of WideCPOEngine at HumanoidVelocity's
dims (376 / 17) and at both ends of the range (129 / 1, 512 / 32), on the streamed-W1 kernels (csrc/cpo.hip, spo_cpo512_*) and on
the chunked wide path (SPO_CPO_OBS512=0: the routing before these kernels), M = 4096 x 128 rows:
    python tools/cpo_obs512_bench.py [--calls 48] [--warmup 3] [--out profiles/cpo_obs512/primitives.txt]
    python tools/cpo_obs512_bench.py --resource-usage        # no GPU: registers / spills / scratch of the kernels -> resource_usage.txt
Both routes live in ONE process: two engines over equal policies and equal batches, one built with the knob at 0 and one with it
at 1 (the knob is read when the engine is built), and their calls alternate, wide - new - wide - new ..., so both see the same
clocks and the same neighbours.  A sample is a HIP event pair around ONE call (for policy_update that includes its host
synchronisations: the line search reads its sums back); the parameters are restored outside the timed window.  Reported per
shape and item: median and min in microseconds of either path, and whether the new path is ahead by more than the larger
median - min spread of the two sides."""
import argparse
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "safe-policy-optimization_amd"))

SHAPES = [(376, 17), (129, 1), (512, 32)]
N, T = 4096, 128
ITEMS = ["surrogate_grad", "fvp", "linesearch_sums", "policy_update"]
OUT_DIR = os.path.join(ROOT, "profiles", "cpo_obs512")


def _side(D, A, knob, dev):
    import torch
    from safepo.common.model import ActorVCritic
    from safepo.single_agent import cpo
    os.environ["SPO_CPO_OBS512"] = knob
    torch.manual_seed(D)
    pol = ActorVCritic(D, A).to(dev)
    eng = cpo.make_engine(pol, N, T, dict(cpo.default_cfg), dev)
    assert type(eng) is cpo.WideCPOEngine and eng._actor_on_streamed_kernels is (knob == "1")
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
    return {"pol": pol, "eng": eng, "theta0": theta0, "runs": runs}


def measure(calls, warmup):
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    res = []
    for D, A in SHAPES:
        sides = {knob: _side(D, A, knob, dev) for knob in ("0", "1")}
        assert torch.equal(sides["0"]["theta0"], sides["1"]["theta0"])
        assert torch.equal(sides["0"]["eng"].buffer.data["obs"], sides["1"]["eng"].buffer.data["obs"])
        entry = {"obs_dim": D, "act_dim": A, "us": {"0": {}, "1": {}}, "step": {}}
        for name in ITEMS:
            us = {"0": [], "1": []}
            for i in range(warmup + calls):
                for knob in ("0", "1"):
                    s = sides[knob]
                    s["pol"].theta.copy_(s["theta0"])
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = s["runs"][name]()
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= warmup:
                        us[knob].append(e0.elapsed_time(e1) * 1e3)
                    if name == "policy_update":
                        entry["step"][knob] = (int(out["case"]), int(out["acceptance_step"]))
            for knob in ("0", "1"):
                entry["us"][knob][name] = us[knob]
            print(f"{D}/{A} {name} done", flush=True)
        res.append(entry)
        del sides
        torch.cuda.empty_cache()
    return res


def resource_usage():
    """hipcc -Rpass-analysis=kernel-resource-usage on csrc/cpo.hip with the build's own flags (cross-compiles; no GPU)."""
    import tempfile
    import __graft_entry__ as ge
    src = os.path.join(ge.CSRC, "cpo.hip")
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
    lines = ["kernel-resource-usage of csrc/cpo.hip (gfx950), the streamed-W1 kernels.  LDS Size is the static part: cpo512_actor_kernel takes "
             "its own dynamically, 70 784 B in mode 0 (surrogate gradient) and 97 536 B in mode 1 (Fisher-vector product).",
             "Template arguments: <mode, X4> / <mean-only, X4>; X4 = obs_dim is a multiple of 4 (aligned 16-byte observation loads: 376, "
             "192, 512); the other form (129) addresses every observation element on its own and spills a few registers to scratch."]
    for row in rows:
        if "cpo512" in row["name"]:
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


def report(args, res):
    lines = [f"WideCPOEngine, hidden [64, 64], M = {N} x {T} = {N * T} rows; microseconds per call, HIP event pair around one call; both "
             f"routes in one process, calls alternating wide / new, {args.warmup} warm-up calls then {args.calls} timed calls per route",
             "wide = SPO_CPO_OBS512=0 (launch-per-layer wide kernels in row chunks: the routing before the streamed-W1 kernels); "
             "new = SPO_CPO_OBS512=1 (spo_cpo512_*)",
             "ahead = new median < wide median by more than max(median - min) of the two sides", ""]
    lines.append(f"{'obs/act':>8} {'item':<16} {'wide median':>12} {'wide min':>10} {'new median':>11} {'new min':>9} {'speed-up':>9}  ahead")
    all_win = True
    for e in res:
        for k in ITEMS:
            (om, ol), (nm, nl) = stats(e["us"]["0"][k]), stats(e["us"]["1"][k])
            win = (om - nm) > max(om - ol, nm - nl)
            all_win &= win
            lines.append(f"{e['obs_dim']:>4}/{e['act_dim']:<3} {k:<16} {om:12.1f} {ol:10.1f} {nm:11.1f} {nl:9.1f} {om / nm:8.2f}x  {'yes' if win else 'NO'}")
        (c0, a0), (c1, a1) = e["step"]["0"], e["step"]["1"]
        lines.append(f"{'':>8} policy_update: case {c0} / acceptance step {a0} (wide), case {c1} / acceptance step {a1} (new)")
    lines += ["", "every primitive and the whole step are ahead at every shape" if all_win else "NOT every item is ahead: see the NO rows", ""]
    ru = os.path.join(OUT_DIR, "resource_usage.txt")
    if os.path.exists(ru):
        lines += open(ru).read().splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(OUT_DIR, "primitives.txt"))
    ap.add_argument("--resource-usage", action="store_true")
    a = ap.parse_args()
    assert a.calls >= 20, "at least 20 timed calls"
    if a.resource_usage:
        resource_usage()
    else:
        report(a, measure(a.calls, a.warmup))
