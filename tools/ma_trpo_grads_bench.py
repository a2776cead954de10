"""MACPO's two surrogate gradients: the fused pair (spo_ma_trpo_grads, SPO_MA_GRADS_FUSED=1) against the default, spo_ma_actor_loss +
spo_ma_backward once per gradient.

    python tools/ma_trpo_grads_bench.py [--rows 10000] [--calls 32] [--warmup 4] [--out FILE]
        (a) the gradient pair alone on kept activations -- _surrogate_grads_fused against two _surrogate_grad calls -- and (b), (c)
        one MACPO_Trainer.trpo_update per call in the host-driven and the sharded form at the mamujoco configuration (hidden 128,
        layer_N = 1, obs 48, act 6; the set-up of tools/macpo_dp_bench.py), the two routes alternating call by call in one process,
        every trpo_update from the same parameters, optimiser state and PopArt statistics; both routes must take the same case and
        accept the same step.  Median and minimum per route; a gain is claimed only where it exceeds three times the larger
        median-to-minimum spread (the table of tools/ma_ls_eval_bench.py)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import macpo_dp_bench as B  # noqa: E402  (also puts the package on sys.path)
from ma_ls_eval_bench import table  # noqa: E402

KNOB = "SPO_MA_GRADS_FUSED"
ROUTES = (("fused pair (SPO_MA_GRADS_FUSED=1)", "1"), ("loss + backward per gradient (default)", "0"))


def timed(fn, calls, warmup, before=None):
    import torch
    times = {name: [] for name, _ in ROUTES}
    for k in range(warmup + calls):
        for name, knob in ROUTES:
            os.environ[KNOB] = knob
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(knob)
            torch.cuda.synchronize()
            if k >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.calls >= 32, "medians of at least 32 calls"
    import torch
    arch = torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    before = os.environ.get(KNOB)
    lines = [f"# python tools/ma_trpo_grads_bench.py --rows {a.rows} --calls {a.calls} --warmup {a.warmup}",
             f"# {a.rows} rows, hidden 128, layer_N 1, obs 48 / act 6; {arch}; routes alternating call by call"]
    for title, sharded in (("(b) one MACPO_Trainer.trpo_update, host-driven form", False), ("(c) one MACPO_Trainer.trpo_update, sharded form at world size 1", True)):
        pol, tr, sample = B.build(a.rows, sharded)
        actor = pol.actor
        assert actor.trpo_grads_supported()
        snap = B.Snapshot(pol, tr)
        steps = {}

        def update(knob):
            tr.trpo_update(sample)
            steps[knob] = dict(tr.last_step_info)
        times = timed(update, a.calls, a.warmup, before=snap.restore)
        assert steps["1"] == steps["0"], steps
        if not sharded:
            snap.restore()
            f = lambda t: t.float().contiguous()
            obs, act, old_lp = f(sample[1]), f(sample[4]), f(sample[9])
            adv, cadv, factor, active = (f(sample[k]).reshape(-1) for k in (10, 16, 12, 8))
            mean, saved = actor.net_forward(obs, keep=True)

            def pair(knob):
                if knob == "1":
                    tr._surrogate_grads_fused(saved, mean, act, old_lp, adv, cadv, factor)
                else:
                    tr._surrogate_grad(saved, mean, act, old_lp, adv, factor, active)
                    tr._surrogate_grad(saved, mean, act, old_lp, cadv, factor, active)
            lines += table("(a) the gradient pair alone on kept activations (wall time, launch to synchronize)", timed(pair, a.calls, a.warmup))
        lines += table(f"{title}, same start state every call; optim_case {steps['1']['optim_case']}, accepted step "
                       f"{steps['1']['accepted_step']} on both routes", times)
    os.environ.pop(KNOB, None) if before is None else os.environ.__setitem__(KNOB, before)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
