"""Child process of test_gpu_seed_batch_critic_split.py: SPO_CPO_SPLIT_L2 is read once per process, so the uncached exchange of
the seed-batched split critic fit is exercised in a process of its own.  Runs S runs of one shape through two batched launches and
through single launches (same process, same setting), compares every run bit for bit and prints one JSON line:
    python tests/seed_batch_critic_split_worker.py S D A"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "safe-policy-optimization_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(S, shape):
    import torch
    import test_gpu_seed_batch_critic_split as T
    from safepo import _abi
    lib = _abi.load()
    dev = torch.device("cuda:0")
    want = []
    for r in range(S):
        eng, perms = T._engine(shape, r, dev)
        T._start(eng)
        logs = [T._single_iter(lib, eng, perms[k]) for k in range(2)]
        want.append((T._state(eng), logs))
    built = [T._engine(shape, r, dev) for r in range(S)]
    engs = [e for e, _ in built]
    for e in engs:
        T._start(e)
    T._counters(lib)
    got_logs = [T._multi_iter(lib, engs, [p[k] for _, p in built]) for k in range(2)]
    torch.cuda.synchronize()
    counters = T._counters(lib)
    bad = []
    for r, e in enumerate(engs):
        if int(e.sync_ws[8].item()) or int(e._split_setup()["sync_ws"][8].item()):
            bad.append(f"run {r}: error word set")
        for name, x, y in zip(T.STATE_NAMES, T._state(e), want[r][0]):
            if not torch.equal(x, y):
                bad.append(f"run {r}: {name} differs")
        for k in range(2):
            for h in range(2):
                if not torch.equal(got_logs[k][r][h], want[r][1][k][h]):
                    bad.append(f"run {r}: loss log {h} of launch {k} differs")
    print("RESULT " + json.dumps({"counters": counters, "bad": bad, "l2": os.environ.get("SPO_CPO_SPLIT_L2")}))


if __name__ == "__main__":
    main(int(sys.argv[1]), (int(sys.argv[2]), int(sys.argv[3])))
