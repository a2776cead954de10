"""Development aid (GPU box): time the KL-penalty minibatch step of the wide path -- FOCOPS's step (focops.py:312-347) and CUP's
actor-only second stage (cup.py:370-386) through safepo.common.engine.WidePPOLagEngine.learning_iter_ex -- at the reference's
default batch of 64 for a few (obs_dim, act_dim, hidden_sizes).  Uses only interfaces that predate the row-group form of this step
(csrc/mlp_rows.hip), so the same file times a checkout from before it:
    python tools/klpen_rows_bench.py [--steps 256] [--repeats 3]
One JSON line: per case the microseconds per minibatch step of every repeat (a host clock around a synchronised pass of `steps`
replayed steps, after a warm-up pass of the same shape), their median and spread, and which path the step took."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safe-policy-optimization_amd"))

CASES = [(60, 8, [128, 128]), (60, 8, [256, 256]), (72, 2, [128, 128])]
BATCH = 64


def one(D, A, hidden, actor_only, steps, repeats):
    from safepo import _abi
    from safepo.common.engine import WidePPOLagEngine
    from safepo.common.model import ActorVCritic
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    pol = ActorVCritic(D, A, hidden_sizes=hidden).to(dev)
    M = BATCH * steps
    cfg = {"hidden_sizes": hidden, "gamma": 0.99, "target_kl": 1e9, "batch_size": BATCH, "learning_iters": 1, "max_grad_norm": 40.0}
    eng = WidePPOLagEngine(pol, 1, M, cfg, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    b = eng.buffer
    for k in ("obs", "act", "target_value_r", "target_value_c"):
        b.data[k].normal_(generator=g)
    b.data["log_prob"].copy_(-A * 0.92 - 0.5 * (b.data["act"] ** 2).sum(-1))
    adv = torch.randn(M, device=dev, generator=g)
    eng.snapshot_old_distribution()
    # old means a little off the current ones, the bound at the median of the rows' KL: the indicator is active on about half of them
    eng.mean_old += 0.05 * torch.randn(eng.mean_old.shape, device=dev, generator=g)
    kl = (0.5 * ((eng.wide.actor_mean(b.data["obs"].view(M, D)) - eng.mean_old) / eng.std_old) ** 2).sum(-1)
    kl_bound = float("inf") if actor_only else float(kl.median())
    pg_coef = -0.37 if actor_only else 1 / 1.5
    perm = torch.randperm(M, device=dev, generator=g).to(torch.int32)
    run = lambda: eng.learning_iter_ex(perm, adv, _abi.ACTOR_LOSS_KL_PENALTY, kl_bound, pg_coef, actor_only)
    losses = run()                                   # warm-up: lazy set-up, the graph capture
    torch.cuda.synchronize()
    assert torch.isfinite(losses[:, 2]).all()
    us = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / steps * 1e6)
    ok = getattr(eng, "_row_group_step_ok", None)
    path = "row-group" if ok is not None and ok(BATCH, _abi.ACTOR_LOSS_KL_PENALTY, actor_only) else "launch-per-network"
    return {"obs_dim": D, "act_dim": A, "hidden_sizes": hidden, "step": "cup_stage2" if actor_only else "focops", "batch": BATCH,
            "steps": steps, "us_per_step": [round(v, 2) for v in us], "median_us": round(sorted(us)[len(us) // 2], 2),
            "spread_us": round(max(us) - min(us), 2), "path": path}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    assert args.steps >= 256, "a timed window is at least 256 steps"
    out = [one(D, A, hidden, ao, args.steps, args.repeats) for D, A, hidden in CASES for ao in (False, True)]
    print(json.dumps(out))
