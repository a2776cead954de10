"""The update problems of tests/test_gpu_seed_batch_ks.py (no test in here): run r of a (shape, mode) at the feature-split
kernel's dims -- its initialisation, rows, old distribution, shuffles, scalars and optimiser clocks -- built on the CPU from seeds
by tests/klpen_batch_problem.py's make_run (same draws, same oracle), with the shapes and constants of this file.

`python tests/ks_batch_problem.py` prints, per (shape, mode), what the float32 CPU oracle (oracle/restatement.py) finds under the
constants below: how many of the steps have their joint gradient norm above max_grad_norm, the smallest relative distance of a
norm from it, and on how many FOCOPS steps the indicator fraction lies strictly between 0 and 1."""
import numpy as np
import torch

import klpen_batch_problem as K

# (obs, act, batch): the smallest shapes at which each distinct path of the feature-split body is exercised
SHAPES = [
    (376, 17, 64),     # S = 6, ragged last slice of 56, second output tile with one column (HumanoidVelocity)
    (129, 1, 64),      # S = 3, last slice of one feature
    (512, 32, 64),     # S = 8, everything full
    (192, 16, 20),     # S = 3 exact slices, one full output tile, short batch
    (60, 20, 64),      # S = 1, no exchange partner: what act_dim > 16 routes here
]
MODES = K.MODES               # mode -> (actor_loss, actor_only): "focops", "cup2" (the actor alone, its clock ahead), "clip"
CASES = [(s, m) for m in ("clip", "focops", "cup2") for s in SHAPES]
REPLICAS = (1, 3, 8, 9, 16)   # run counts of the bit-exactness test (9 and 16 only up to 256 observations)
GAMMA = K.GAMMA


def slices(shape):
    return (shape[0] + 63) // 64


def max_runs(shape):
    """spo_update_ks_multi_supported's cap, restated: min(16, 8 * (8 // S))."""
    return min(16, 8 * (8 // slices(shape)))


rows, n_steps = K.rows, K.n_steps

# max_grad_norm per (shape, mode), fixed from the float32 oracle (this file run as a script prints the line behind each entry):
# between a quarter and three quarters of the 2 x ceil(M / batch) x max_runs(shape) steps have their joint norm above it -- so
# clipped and unclipped steps are both compared -- and no step's norm lies within 1e-3 (relative) of it.
MAX_GRAD_NORM = {
    # the clipped surrogate:
    ((376, 17, 64), "clip"): 1.9,      # 47 of 96 steps above, nearest 5.2e-3
    ((129, 1, 64), "clip"): 1.06,      # 121 of 192, 5.1e-3
    ((512, 32, 64), "clip"): 1.9,      # 48 of 96, 3.3e-3
    ((192, 16, 20), "clip"): 2.13,     # 83 of 160, 3.0e-3
    ((60, 20, 64), "clip"): 1.39,      # 87 of 192, 2.3e-3
    # FOCOPS (the indicator fraction lies strictly between 0 and 1 on all 96 / 192 / 160 steps of every shape):
    ((376, 17, 64), "focops"): 1.7,    # 50 of 96, 3.1e-3
    ((129, 1, 64), "focops"): 1.09,    # 104 of 192, 3.4e-3
    ((512, 32, 64), "focops"): 2.0,    # 49 of 96, 7.9e-3
    ((192, 16, 20), "focops"): 2.1,    # 78 of 160, 3.2e-3
    ((60, 20, 64), "focops"): 1.4,     # 85 of 192, 3.3e-3
    # CUP's second stage (the norm spans the actor alone):
    ((376, 17, 64), "cup2"): 4.7,      # 48 of 96, 7.8e-3
    ((129, 1, 64), "cup2"): 1.1,       # 104 of 192, 1.0e-2
    ((512, 32, 64), "cup2"): 4.75,     # 52 of 96, 2.3e-3
    ((192, 16, 20), "cup2"): 6.9,      # 78 of 160, 8.6e-3
    ((60, 20, 64), "cup2"): 4.5,       # 94 of 192, 5.6e-3
}


def make_run(shape, mode, r, max_grad_norm=None):
    """Run r of (shape, mode), everything on the CPU.  The runs differ in initialisation, data, old distribution, shuffles,
    pg_coef, kl_bound, lr_factor and both optimiser clocks (klpen_batch_problem.make_run)."""
    return K.make_run(shape, mode, r, MAX_GRAD_NORM[(shape, mode)] if max_grad_norm is None else max_grad_norm)


def survey(shape, mode, max_grad_norm):
    """-> (steps above the bound, steps, smallest relative distance from the bound, FOCOPS steps with 0 < fraction < 1, norms)."""
    norms, fracs = [], []
    for r in range(max_runs(shape)):
        n, f = K.oracle_norms(make_run(shape, mode, r, max_grad_norm))
        norms.append(n); fracs.append(f)
    norms, fracs = np.concatenate(norms), np.concatenate(fracs)
    margin = float(np.min(np.abs(norms / max_grad_norm - 1.0)))
    return int((norms > max_grad_norm).sum()), norms.size, margin, int(((fracs > 0) & (fracs < 1)).sum()), norms


def holds(above, n, margin, mixed, mode):
    return 4 * above >= n and 4 * above <= 3 * n and margin > 1e-3 and (mode != "focops" or mixed == n)


if __name__ == "__main__":
    import sys
    torch.set_num_threads(4)
    for shape, mode in CASES:
        bound = MAX_GRAD_NORM[(shape, mode)]
        above, n, margin, mixed, norms = survey(shape, mode, bound)
        print(f"{shape} {mode}: max_grad_norm {bound}: {above} of {n} steps above it, nearest {margin:.2e} "
              f"(relative), norms {norms.min():.3g} .. {norms.max():.3g}, median {np.median(norms):.4g}"
              + (f", 0 < fraction < 1 on {mixed} steps" if mode == "focops" else "")
              + ("" if holds(above, n, margin, mixed, mode) else "   <-- CONDITION NOT MET"), flush=True)
    sys.exit(0)
