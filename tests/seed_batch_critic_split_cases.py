"""The problems of the seed-batched split critic fit's tests, shared by the GPU tests (test_gpu_seed_batch_critic_split.py) and
their CPU companion (test_seed_batch_critic_split_host.py: the clip condition on these very initialisations).

Shapes (obs_dim, act_dim): the default sweep's own class (72 / 2: Car) and the two edges of the KIN = 128 range (65 / 1,
128 / 16).  Every run has M = 3 x 128 rows (three 128-row minibatches, each split into two 64-row halves) and two shuffles.

So that some steps clip and some do not: max_grad_norm 1.0, the value targets of _synthetic_update_problem times 0.6, a stale
actor gradient of ||.||^2 = 0.5 + 0.01 r (the settings of test_gpu_seed_batch_critic.py).  The float32 oracle
(oracle/restatement.CriticFitter, OraclePolicy initialised under torch.manual_seed(100 + r), 17 runs x 6 steps) has joint norms of
0.79-1.60 / 0.73-1.43 / 0.75-1.42 at the three shapes with 49 / 47 / 42 of 102 steps above 1.0, both kinds among runs 0-2; the CPU
companion asserts the condition on ActorVCritic's own initialisation.  Every clipped step rescales the stale norm: the joint
clip's write to stale_sq_io is exercised."""
import torch

SHAPES = [(72, 2), (65, 1), (128, 16)]
BATCH, M = 128, 3 * 128
N_MB = M // BATCH
S_MAX = 17
MAX_GRAD_NORM = 1.0
TARGET_SCALE = {(72, 2): 0.6, (65, 1): 0.6, (128, 16): 0.6}
STALE_SQ0 = 0.5
CFG = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 0.01, "learning_iters": 1}


def stale_sq0(r: int) -> float:
    return STALE_SQ0 + 0.01 * r


def make_policy(shape, r):
    """Run r's ActorVCritic, on the CPU (the GPU tests move it over): the initialisation both sides of the comparison share."""
    from safepo.common.model import ActorVCritic
    D, A = shape
    torch.manual_seed(100 + r)
    pol = ActorVCritic(D, A)
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    return pol


def make_problem(shape, r):
    """(obs, act, logp, tgt_r, tgt_c, adv) of run r, the targets scaled."""
    from test_gpu_parity import _synthetic_update_problem
    D, A = shape
    obs, act, logp, tgt_r, tgt_c, adv = _synthetic_update_problem(M, D, A, seed=1000 + r)
    k = TARGET_SCALE[shape]
    return obs, act, logp, k * tgt_r, k * tgt_c, adv


def make_perms(r, n=2):
    g = torch.Generator().manual_seed(50 + r)
    return [torch.randperm(M, generator=g).to(torch.int32) for _ in range(n)]
