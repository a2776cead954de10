"""MACPO's Fisher-vector product: the fused kernel (spo_ma_fvp, the default) against SPO_MA_FVP=0 (spo_ma_jvp + spo_ma_backward).

    python tools/ma_fvp_bench.py [--rows 10000] [--calls 32] [--warmup 4] [--out FILE]
        (a) one MACPO_Trainer.fisher_vector_product and (b) one MACPO_Trainer.trpo_update per call at the mamujoco configuration
        (hidden 128, layer_N = 1, obs 48, act 6; the set-up of tools/macpo_dp_bench.py), the two routes alternating call by call
        in one process, every trpo_update from the same parameters, optimiser state and PopArt statistics.  Median and minimum
        per route; a gain is claimed only where it exceeds three times the larger median-to-minimum spread."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import macpo_dp_bench as B  # noqa: E402  (also puts the package on sys.path)

ROUTES = (("fused kernel (default)", "1"), ("SPO_MA_FVP=0 (jvp + backward)", "0"))


def timed(fn, calls, warmup, before=None):
    import torch
    times = {name: [] for name, _ in ROUTES}
    for k in range(warmup + calls):
        for name, knob in ROUTES:
            os.environ["SPO_MA_FVP"] = knob
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def table(title, times):
    lines = [title, "route | median ms | min ms | median - min ms"]
    stats = {n: (statistics.median(t), min(t)) for n, t in times.items()}
    for n, (med, mn) in stats.items():
        lines.append(f"{n} | {med:.3f} | {mn:.3f} | {med - mn:.3f}")
    (f_med, f_min), (p_med, p_min) = stats.values()
    spread = max(f_med - f_min, p_med - p_min)
    gain = p_med - f_med
    verdict = ("a gain: more than three times the larger median-to-minimum spread" if gain > 3 * spread else
               "a loss: more than three times the larger median-to-minimum spread" if -gain > 3 * spread else
               "no claim: within three times the larger median-to-minimum spread")
    lines.append(f"fused / SPO_MA_FVP=0, medians: {f_med / p_med:.3f} ({verdict})")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.calls >= 32, "medians of at least 32 calls"
    import torch
    pol, tr, sample = B.build(a.rows, False)
    assert pol.actor.fvp_supported()
    snap = B.Snapshot(pol, tr)
    _, saved = pol.actor.net_forward(sample[1], keep=True)
    std = tr._std()
    m_diag = (2.0 / (1e-8 + 2.0 * std * std)).reshape(1, -1)
    h_ls = tr._kl_hessian_logstd()
    p = torch.randn(pol.actor.theta.numel(), generator=torch.Generator().manual_seed(5)).to(sample[1].device)
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# python tools/ma_fvp_bench.py --rows {a.rows} --calls {a.calls} --warmup {a.warmup}",
             f"# {a.rows} rows, hidden 128, layer_N 1, obs 48 / act 6, actor {p.numel()} parameters; {arch}; routes alternating call by call"]
    lines += table("(a) one MACPO_Trainer.fisher_vector_product (wall time, launch to synchronize)",
                   timed(lambda: tr.fisher_vector_product(saved, p, m_diag, h_ls), a.calls, a.warmup))
    lines += table("(b) one MACPO_Trainer.trpo_update (host-driven form), same start state every call",
                   timed(lambda: tr.trpo_update(sample), a.calls, a.warmup, before=snap.restore))
    os.environ.pop("SPO_MA_FVP", None)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
