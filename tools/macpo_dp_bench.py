"""MACPO trust-region step: the host-driven path against the sharded form forced at world size 1, same process.

    python tools/macpo_dp_bench.py time [--rows 10000] [--calls 32] [--warmup 4] [--out FILE]
        one MACPO_Trainer.trpo_update at the mamujoco configuration (hidden 128, layer_N = 1; observations / actions of the
        synthetic multi-agent env) per call, the two paths interleaved call by call, every call from the same parameters,
        optimiser state and PopArt statistics (restored outside the timed region).  Median and minimum per path.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/macpo_dp_bench.py cg --path host|sharded --iters K
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/macpo_dp_bench.py fvp --iters K
        `--solves` conjugate-gradient solves of K iterations (or K Fisher-vector products alone) and nothing else, for a
        kernel trace of its own.

    python tools/macpo_dp_bench.py launches --host DIR_K1 DIR_K2 --sharded DIR_K1 DIR_K2 --fvp DIR_K1 DIR_K2 --iters K1 K2 [--out FILE]
        launches per CG iteration of each path = (launches at K2 - launches at K1) / ((K2 - K1) * solves): set-up and one-time
        launches cancel.  Appended to FILE."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "safe-policy-optimization_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


class Sp:
    def __init__(self, n):
        self.shape = (n,)


def build(rows, sharded, seed=0):
    import torch
    from safepo.multi_agent import macpo as M
    dev = torch.device("cuda:0")
    D, A, agents = 48, 6, 4                        # SynthMAEnv defaults
    S = D * agents // 2
    cfg = dict(M.default_cfg)
    cfg.update(M.mamujoco_cfg)
    cfg.update(device="cuda:0", macpo_sharded_form=bool(sharded), cost_limit=1.0)
    torch.manual_seed(seed)
    pol = M.MACPO_Policy(cfg, Sp(D), Sp(S), Sp(A))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for net in pol.networks():
            net.theta.add_(0.02 * torch.randn(net.theta.shape, generator=g).to(dev))
    tr = M.MACPO_Trainer(cfg, pol)
    obs, share = torch.randn(rows, D, generator=g), torch.randn(rows, S, generator=g)
    with torch.no_grad():
        mean = pol.actor.net_forward(obs.to(dev)).cpu()
    std = tr._std().cpu()
    act = mean + std * torch.randn(rows, A, generator=g)
    old_logp = -((act - mean) ** 2) / (2 * std * std) - torch.log(std) - 0.9189385332
    rn = lambda *s: torch.randn(*s, generator=g)
    sample = (share, obs, None, None, act, rn(rows, 1), rn(rows, 1) * 2, None, torch.ones(rows, 1), old_logp, rn(rows, 1), None,
              0.5 + torch.rand(rows, 1, generator=g), rn(rows, 1), torch.rand(rows, 1, generator=g) * 3, None, rn(rows, 1),
              torch.tensor(0.7))
    sample = tuple(t.to(dev) if torch.is_tensor(t) else t for t in sample)
    return pol, tr, sample


class Snapshot:
    """Parameters, Adam state and PopArt statistics of a trainer, to start every timed call from the same point."""

    def __init__(self, pol, tr):
        self.pol, self.tr = pol, tr
        opts = (pol.actor_optimizer, pol.critic_optimizer, pol.cost_optimizer)
        self.saved = [(net.theta.clone(), o.m.clone(), o.v.clone(), o.t) for net, o in zip(pol.networks(), opts)]
        self.popart = tr._popart_state.clone()

    def restore(self):
        pol = self.pol
        opts = (pol.actor_optimizer, pol.critic_optimizer, pol.cost_optimizer)
        for net, o, (th, m, v, t) in zip(pol.networks(), opts, self.saved):
            net.theta.copy_(th); o.m.copy_(m); o.v.copy_(v); o.t = t
        self.tr._popart_state.copy_(self.popart)


def cmd_time(a):
    import torch
    sides = {}
    for name, sharded in (("host-driven path (world size 1 as shipped)", False), ("sharded form forced (macpo_sharded_form=True)", True)):
        pol, tr, sample = build(a.rows, sharded)
        sides[name] = (pol, tr, sample, Snapshot(pol, tr), [])
    info = {}
    for k in range(a.warmup + a.calls):
        for name, (pol, tr, sample, snap, times) in sides.items():
            snap.restore()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.trpo_update(sample)
            torch.cuda.synchronize()
            if k >= a.warmup:
                times.append((time.perf_counter() - t0) * 1e3)
            info[name] = dict(tr.last_step_info)
    n_par = sides[next(iter(sides))][0].actor.theta.numel()
    lines = [f"# python tools/macpo_dp_bench.py time --rows {a.rows} --calls {a.calls} --warmup {a.warmup}",
             f"# one MACPO_Trainer.trpo_update per call, {a.rows} rows, hidden 128, layer_N 1, obs 48 / share_obs 96 / act 6, "
             f"actor {n_par} parameters; {torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]}; paths interleaved, same start state every call",
             "path | median ms | min ms | median - min ms | optim_case | accepted line-search step"]
    res = {}
    for name, (_, _, _, _, times) in sides.items():
        med, mn = statistics.median(times), min(times)
        res[name] = (med, mn)
        lines.append(f"{name} | {med:.3f} | {mn:.3f} | {med - mn:.3f} | {info[name]['optim_case']} | {info[name]['accepted_step']}")
    (h_med, h_min), (s_med, s_min) = res.values()
    spread = max(h_med - h_min, s_med - s_min)
    verdict = ("slower than the host-driven path by more than either side's median-to-min spread" if s_med - h_med > spread else
               "faster than the host-driven path by more than either side's median-to-min spread" if h_med - s_med > spread else
               "within either side's median-to-min spread of the host-driven path")
    lines.append(f"sharded form / host-driven path, medians: {s_med / h_med:.3f} ({verdict})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


def cmd_cg(a, fvp_only=False):
    import torch
    pol, tr, sample = build(a.rows, a.path == "sharded")
    obs = sample[1]
    _, saved = pol.actor.net_forward(obs, keep=True)
    std = tr._std()
    m_diag = (2.0 / (1e-8 + 2.0 * std * std)).reshape(1, -1)
    h_ls = tr._kl_hessian_logstd()
    b = torch.randn(pol.actor.theta.numel(), generator=torch.Generator().manual_seed(5)).to(obs.device)
    torch.cuda.synchronize()
    for _ in range(a.solves):
        if fvp_only:
            for _ in range(a.iters):
                tr.fisher_vector_product(saved, b, m_diag, h_ls)
        else:
            tr.conjugate_gradient(saved, b, a.iters, m_diag, h_ls)
    torch.cuda.synchronize()
    print(json.dumps({"mode": "fvp" if fvp_only else "cg", "path": a.path, "solves": a.solves, "iters": a.iters}))


def total_launches(d):
    hits = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not hits:
        raise SystemExit(f"no *kernel_stats.csv under {d}")
    with open(max(hits, key=os.path.getsize)) as f:
        return sum(int(r["Calls"]) for r in csv.DictReader(f))


def cmd_launches(a):
    k1, k2 = a.iters
    per = {}
    for name, dirs in (("host-driven path", a.host), ("sharded form", a.sharded), ("Fisher-vector product alone", a.fvp)):
        n1, n2 = total_launches(dirs[0]), total_launches(dirs[1])
        per[name] = (n2 - n1) / ((k2 - k1) * a.solves)
    f = per["Fisher-vector product alone"]
    lines = [f"# launches per conjugate-gradient iteration: rocprofv3 --kernel-trace --stats of `macpo_dp_bench.py cg` at {k1} and {k2} "
             f"iterations x {a.solves} solves per path, difference / {(k2 - k1) * a.solves} (set-up launches cancel)",
             "path | launches per CG iteration | of which the Fisher-vector product | vector step"]
    for name in ("host-driven path", "sharded form"):
        lines.append(f"{name} | {per[name]:.2f} | {f:.2f} | {per[name] - f:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "a") as fo:
            fo.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["time", "cg", "fvp", "launches"])
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--path", choices=["host", "sharded"], default="host")
    ap.add_argument("--iters", type=int, nargs="+", default=[10])
    ap.add_argument("--solves", type=int, default=4)
    ap.add_argument("--host", nargs=2)
    ap.add_argument("--sharded", nargs=2)
    ap.add_argument("--fvp", nargs=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode == "time":
        assert a.calls >= 32, "medians of at least 32 calls"
        cmd_time(a)
    elif a.mode == "launches":
        cmd_launches(a)
    else:
        a.iters = a.iters[0]
        cmd_cg(a, fvp_only=a.mode == "fvp")


if __name__ == "__main__":
    main()
