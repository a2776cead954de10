"""Row-chunk CPO kernels (csrc/cpo_rows.hip) against the chunked wide path (SPO_CPO_ROWS=0), alternating in one process:
medians (minima) of 48 calls per primitive and of one whole policy_update at 4096 x 128 rows.  Prints the table."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "safe-policy-optimization_amd"), os.path.join(ROOT, "tests")]
SHAPES = [(60, 8, [128, 128]), (72, 2, [128, 128]), (128, 16, [128, 128, 128])]
N, T, CALLS = 4096, 128, 48


def timed(fn, calls):
    out = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def main():
    from test_gpu_cpo_obs128 import _cpo_problem
    dev = torch.device("cuda:0")
    print(f"rows {N * T}; us per call: median (min) of {CALLS}; policy_update: of 6")
    for D, A, hidden in SHAPES:
        engs = {}
        for knob in ("1", "0"):
            os.environ["SPO_CPO_ROWS"] = knob
            engs[knob] = _cpo_problem(D, A, hidden, N, T, dev, seed=3, expect_new_path=False)[2]
        on = engs["1"]._actor_on_row_group_kernels
        v = torch.randn(engs["1"].Pa, device=dev)
        rows = {}
        for name, calls in (("surrogate_grad", CALLS), ("fvp", CALLS), ("linesearch", CALLS), ("policy_update", 6)):
            for knob, e in engs.items():
                d = e.buffer.data
                th0 = e.theta_actor.clone()
                e.snapshot_old_distribution()
                fn = {"surrogate_grad": lambda: e._surrogate_grad_local(d["adv_r"], -1.0), "fvp": lambda: e._fvp_local(v),
                      "linesearch": lambda: e._linesearch_sums_local(d["adv_r"], d["adv_c"]),
                      "policy_update": lambda: (e.theta_actor.copy_(th0), e.policy_update(-1.0))}[name]
                fn(); torch.cuda.synchronize()
                t = timed(fn, calls)
                rows[(name, knob)] = (statistics.median(t), min(t))
            a, b = rows[(name, "1")], rows[(name, "0")]
            print(f"{D:4d}/{A:<2d} {str(hidden):16s} {name:15s} rows kernels{'' if on else ' (outside the envelope: chunked)'} "
                  f"{a[0]:10.1f} ({a[1]:.1f})   chunked {b[0]:10.1f} ({b[1]:.1f})   ratio {b[0] / a[0]:.2f}", flush=True)


if __name__ == "__main__":
    main()
