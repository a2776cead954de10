"""The problems of the seed-batched feature-split critic fit's tests (no test in here), shared by the GPU tests
(test_gpu_seed_batch_critic_ks.py) and their CPU companion (test_seed_batch_critic_ks_host.py: the clip condition on these very
initialisations and scalars).

Shapes (obs_dim, act_dim): 129 / 1 (S = 3, the last slice holds one feature), 192 / 16 (three exact slices), 376 / 17
(HumanoidVelocity, S = 6), 448 / 8 (S = 7: one run per XCD label) and 512 / 32 (S = 8).  Batches: 128 (two full 64-column
chunks), 65 (the second chunk holds one column), 64 (one chunk), 100.  Every run has M = 5 * batch + 7 rows -- five full
minibatches and a ragged one of 7 rows -- and two shuffles.

The runs differ in initialisation, rows, targets, shuffles, stale actor-gradient norm, optimiser clock and cfg scalars: run r has
the critic learning rate 1e-3 * (1 + r % 3 / 4) and max_grad_norm MAX_GRAD_NORMS[r % 4] = 0.6 / 1000 / 1.0 / 1.6.  The stale
||actor.grad||^2 is 0.5 + 0.01 r, so the joint norm of any step of run 0 starts above sqrt(0.5) = 0.707 > 0.6: its first step
clips whatever the critics' gradient is, and every clipped step rescales stale_sq_io.  Run 1 (bound 1000) never clips: its
stale_sq_io comes back bit for bit.  So every launch of two or more runs holds both kinds; the CPU companion checks both claims
with the float32 oracle (oracle/restatement.CriticFitter) at every (shape, batch)."""
import torch

SHAPES = [(129, 1), (192, 16), (376, 17), (448, 8), (512, 32)]
BATCHES = (128, 65, 64, 100)
REPLICAS = (1, 3, 8, 9, 16)        # run counts of the bit-exactness test (9 and 16 only where a launch takes that many)
HUMANOID = (376, 17)
MAX_GRAD_NORMS = (0.6, 1000.0, 1.0, 1.6)
TARGET_SCALE = 0.6
STALE_SQ0 = 0.5
M_MAX = 5 * max(BATCHES) + 7
CFG = {"hidden_sizes": [64, 64], "gamma": 0.99, "target_kl": 0.01, "learning_iters": 1}


def slices(D: int) -> int:
    return (D + 63) // 64


def max_runs(D: int) -> int:
    """spo_critic_fit_ks_multi_supported's cap, restated: at most 24 blocks per XCD label, 2 S blocks a run."""
    return min(16, 8 * (24 // (2 * slices(D))))


def rows(batch: int) -> int:
    return 5 * batch + 7


def n_steps(batch: int) -> int:
    return (rows(batch) + batch - 1) // batch


def stale_sq0(r: int) -> float:
    return STALE_SQ0 + 0.01 * r


def max_grad_norm(r: int) -> float:
    return MAX_GRAD_NORMS[r % 4]


def lr_critic(r: int) -> float:
    return 1e-3 * (1.0 + (r % 3) / 4.0)


def adam_step0(r: int) -> int:
    return 3 + 5 * r


def make_policy(shape, r):
    """Run r's ActorVCritic, on the CPU (the GPU tests move it over): the initialisation both sides of a comparison share."""
    from safepo.common.model import ActorVCritic
    D, A = shape
    torch.manual_seed(100 + r)
    pol = ActorVCritic(D, A)
    with torch.no_grad():
        pol.actor.log_std.copy_(torch.randn(A) * 0.2)
    return pol


def make_rows(shape, r, batch):
    """(obs [M, D], tgt_r [M], tgt_c [M]) of run r: the first M = rows(batch) rows of the run's M_MAX rows."""
    D, _ = shape
    g = torch.Generator().manual_seed(1000 + r)
    obs = torch.randn(M_MAX, D, generator=g)
    tgt_r, tgt_c = torch.randn(M_MAX, generator=g), torch.rand(M_MAX, generator=g)
    M = rows(batch)
    return obs[:M].contiguous(), (TARGET_SCALE * tgt_r[:M]).contiguous(), (TARGET_SCALE * tgt_c[:M]).contiguous()


def make_perms(r, batch, n=2):
    g = torch.Generator().manual_seed(50 + r)
    return [torch.randperm(rows(batch), generator=g).to(torch.int32) for _ in range(n)]
