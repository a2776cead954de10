"""FOCOPS (First Order Constrained Optimization in Policy Space): reference safepo/single_agent/focops.py.
The ppo_lag epoch loop with (a) the multiplier bounded by FOCOPS_NU, (b) the actor loss
    ((KL(pi || pi_old) - (1/FOCOPS_LAM) * ratio * adv) * [KL <= target_kl]).mean()          (focops.py:326-337)
evaluated in the persistent update kernel (spo_update_iter_ex, SPO_ACTOR_LOSS_KL_PENALTY).
Data-parallel (torchrun): the split form -- the KL and policy-gradient parts of the actor's gradient and the row sums from
spo_kl_penalty_grad, one all-reduce, spo_clip_adam_ex with the global fraction of rows inside the bound (engine
PPOLagEngine._learning_iter_ex_split; outside the persistent kernels' shapes WidePPOLagEngine._minibatch_step_ex_split).
hidden_sizes other than [64, 64]: the step's gather, forwards, losses and backward passes are ONE launch split over 16-row groups
(spo_wide_kl_penalty_grad_rows, csrc/mlp_rows.hip: the KL part and the policy-gradient part of the actor's gradient in two kinds of
workgroup), combined with the minibatch's fraction in the group sum (spo_wide_kl_penalty_reduce_parts) or, data-parallel, behind
the all-reduce (spo_wide_kl_penalty_combine); beyond 256 rows or one CU's LDS, the launch-per-network step.
"""
from __future__ import annotations

from safepo.single_agent import _first_order
from safepo.utils.config import run_as_script

default_cfg = {
    'hidden_sizes': [64, 64],
    'gamma': 0.99,
    'target_kl': 0.02,
    'batch_size': 64,
    'learning_iters': 40,
    'max_grad_norm': 40.0,
}


def main(args, cfg_env=None):
    return _first_order.run(args, cfg_env, default_cfg, multiplier="adam", clip=0.2, variant="focops")


if __name__ == "__main__":
    run_as_script(main, __file__)
