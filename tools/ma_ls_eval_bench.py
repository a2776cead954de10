"""MACPO's line search: the fused candidate evaluation (spo_ma_ls_eval, SPO_MA_LS_FUSED=1) against the default (spo_ma_forward +
the row pass).

    python tools/ma_ls_eval_bench.py [--rows 10000] [--calls 32] [--warmup 4] [--out FILE]
        (a) one candidate evaluation with its one host read -- net_ls_eval against net_forward + spo_ma_trpo_linesearch_sums, the
        sharded form's candidate (the host-driven form's old candidate is longer: spo_ma_log_probs, a dozen torch launches, three
        reads) -- and (b), (c) one MACPO_Trainer.trpo_update per call in the host-driven and the sharded form at the mamujoco
        configuration (hidden 128, layer_N = 1, obs 48, act 6; the set-up of tools/macpo_dp_bench.py), the two routes alternating
        call by call in one process, every trpo_update from the same parameters, optimiser state and PopArt statistics.  The
        line search takes the candidates the problem needs: the same start gives the same count on every call, it is printed
        per route (accepted step + 1) and must agree.  Median and minimum per route; a gain is claimed only where it exceeds
        three times the larger median-to-minimum spread."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import macpo_dp_bench as B  # noqa: E402  (also puts the package on sys.path)

ROUTES = (("fused evaluation (SPO_MA_LS_FUSED=1)", "1"), ("forward + row pass (default)", "0"))


def timed(fn, calls, warmup, before=None):
    import torch
    times = {name: [] for name, _ in ROUTES}
    for k in range(warmup + calls):
        for name, knob in ROUTES:
            os.environ["SPO_MA_LS_FUSED"] = knob
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(knob)
            torch.cuda.synchronize()
            if k >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def table(title, times, note=""):
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
    lines.append(f"fused / default, medians: {f_med / p_med:.3f}, gain {gain:.3f} ms{note} ({verdict})")
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
    from safepo import _abi
    lib = _abi.load()
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    lines = [f"# python tools/ma_ls_eval_bench.py --rows {a.rows} --calls {a.calls} --warmup {a.warmup}",
             f"# {a.rows} rows, hidden 128, layer_N 1, obs 48 / act 6; {arch}; routes alternating call by call"]
    for title, sharded in (("(b) one MACPO_Trainer.trpo_update, host-driven form", False), ("(c) one MACPO_Trainer.trpo_update, sharded form at world size 1", True)):
        pol, tr, sample = B.build(a.rows, sharded)
        actor = pol.actor
        assert actor.ls_eval_supported()
        if not sharded:
            # (a): the candidate theta_old - 0.02 v / |v| against theta_old's mean
            f = lambda t: t.float().contiguous()
            obs, act, old_lp = f(sample[1]), f(sample[4]), f(sample[9])
            adv, cadv, factor = f(sample[10]).reshape(-1), f(sample[16]).reshape(-1), f(sample[12]).reshape(-1)
            mu_old, std_old = actor.net_forward(obs), tr._std().clone()
            theta_old = actor.theta.clone()
            v = torch.randn(theta_old.numel(), generator=torch.Generator().manual_seed(5)).to(obs.device)
            actor.theta.copy_(theta_old - 0.02 * v / v.norm())
            ratio = torch.empty(a.rows, device=obs.device)

            def candidate(knob):
                if knob == "1":
                    actor.net_ls_eval(obs, act, old_lp, adv, cadv, factor, mu_old, std_old, tr._ls_sums, ratio, tr._ls_ws)
                else:
                    mu = actor.net_forward(obs)
                    _abi.check(lib.spo_ma_trpo_linesearch_sums(
                        _abi.ptr(mu), _abi.ptr(actor.log_std), actor.std_x_coef, actor.std_y_coef, _abi.ptr(act), _abi.ptr(old_lp),
                        _abi.ptr(adv), _abi.ptr(cadv), _abi.ptr(factor), _abi.ptr(mu_old), _abi.ptr(std_old), a.rows, actor.act_dim,
                        _abi.ptr(tr._ls_sums), _abi.ptr(ratio), _abi.ptr(tr._ls_ws), _abi.stream_ptr()), "spo_ma_trpo_linesearch_sums")
                return tr._ls_sums.tolist()
            lines += table("(a) one candidate evaluation and its host read (wall time, launch to synchronize)", timed(candidate, a.calls, a.warmup))
            actor.theta.copy_(theta_old)
        snap = B.Snapshot(pol, tr)
        steps = {}

        def update(knob):
            tr.trpo_update(sample)
            steps[knob] = dict(tr.last_step_info)
        times = timed(update, a.calls, a.warmup, before=snap.restore)
        assert steps["1"] == steps["0"], steps
        n = steps["1"]["accepted_step"] + 1 if steps["1"]["accepted_step"] >= 0 else int(tr.config["searching_steps"])
        lines += table(f"{title}, same start state every call; optim_case {steps['1']['optim_case']}, {n} line-search candidate(s) on both routes",
                       times, note=f" = {n} candidate(s)")
    os.environ.pop("SPO_MA_LS_FUSED", None)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
