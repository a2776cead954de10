"""Seed-batched PPO-Lagrangian: S independent runs (own seed, policy, buffer, optimiser state) on one GPU whose minibatch
steps share ONE persistent launch (spo_ppo_lag_update_iter_multi, csrc/update_rs.hip): run r on its own six co-XCD workgroups.
FOCOPS and CUP go through the same group on spo_update_iter_ex_multi (csrc/update.hip: the four-wave step, one workgroup per network).
CPOEngineGroup does the same for the critic fit of the second-order scripts (spo_critic_fit_iter_multi: eight workgroups per run).
Per run nothing changes -- the arithmetic of a step is the single launch's, bit for bit, and every run draws its random numbers
from its own generator state (ReplicaRNG), so run r of a group is the stand-alone run with its seed.

The stand-alone step uses 6 of the card's 256 CUs; collect, GAE and the KL of the early-stop test stay one launch per run on
the one stream.
"""
from __future__ import annotations

import contextlib
import os
import random

import numpy as np
import torch

from safepo import _abi


class ReplicaRNG:
    """The random-number state of one run of a group: Python's `random`, numpy's global generator, torch's CPU generator and --
    with `device` -- that device's default generator, seeded the way a stand-alone run seeds itself (random.seed, np.random.seed,
    torch.manual_seed: single_agent/_first_order.run).  `with rng:` switches the state in and saves it back on the way out;
    whatever is drawn for the run (policy init, env creation and reset, the rollout's noise, the shuffle) is drawn inside."""

    def __init__(self, seed: int, device=None):
        self.seed = int(seed)
        self.device = None if device is None else torch.device(device)
        # the states a stand-alone run has right after seeding.  Python, numpy and torch's CPU generator: built on generators of
        # our own.  The device: its default generator is seeded and put back -- no other device's generator is touched (as
        # torch.manual_seed would), and nothing process-wide is left changed.
        dev_state = None
        if self.device is not None:
            outer = torch.cuda.get_rng_state(self.device)             # (initialises the device's generator if need be)
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            torch.cuda.default_generators[idx].manual_seed(self.seed)
            dev_state = torch.cuda.get_rng_state(self.device)
            torch.cuda.set_rng_state(outer, self.device)
        self._state = (random.Random(self.seed).getstate(), np.random.RandomState(self.seed).get_state(),
                       torch.Generator().manual_seed(self.seed).get_state(), dev_state)
        self._outer = None

    def _capture(self):
        dev = None if self.device is None else torch.cuda.get_rng_state(self.device)
        return random.getstate(), np.random.get_state(), torch.get_rng_state(), dev

    def _restore(self, st) -> None:
        random.setstate(st[0])
        np.random.set_state(st[1])
        torch.set_rng_state(st[2])
        if self.device is not None:
            torch.cuda.set_rng_state(st[3], self.device)

    def __enter__(self):
        assert self._outer is None, "ReplicaRNG is not re-entrant"
        self._outer = self._capture()
        self._restore(self._state)
        return self

    def __exit__(self, *exc):
        self._state = self._capture()
        self._restore(self._outer)
        self._outer = None
        return False


class _EngineGroup:
    """What the groups below share: the runs' generator states and their error words."""

    engines, rngs = (), None

    def __len__(self):
        return len(self.engines)

    def rng(self, i: int):
        """Context of run i's random-number state (a no-op context without rngs)."""
        return self.rngs[i] if self.rngs is not None else contextlib.nullcontext()

    def _adopt(self, name, engines, rngs, base, check_type):
        """The constructor checks both groups share, `name` as the message prefix: per engine check_type(i, e) and world size 1
        (engines of class `base` only: anything else with its methods -- a recording stand-in in a test -- is stepped one by
        one), one shape and device, one ReplicaRNG per engine."""
        e0 = engines[0]
        for i, e in enumerate(engines):
            if isinstance(e, base):
                check_type(i, e)
                if e.comm.world_size != 1:
                    raise _abi.SpoError(f"{name}: data-parallel engines cannot be grouped (world size 1 only)")
            if (e.D, e.A, e.M) != (e0.D, e0.A, e0.M) or e.dev != e0.dev:
                raise _abi.SpoError(f"{name}: engine {i} has obs / act / rows / device {e.D} / {e.A} / {e.M} / {e.dev}, "
                                    f"engine 0 has {e0.D} / {e0.A} / {e0.M} / {e0.dev}")
        if rngs is not None and len(rngs) != len(engines):
            raise ValueError(f"{name}: one ReplicaRNG per engine")
        self.engines, self.rngs = engines, rngs
        self._native = all(isinstance(e, base) for e in engines)
        self.lib = _abi.load() if self._native else None

    def _default_perm_fns(self, perm_fns, who=""):
        """perm_fns with every None replaced by the run's default shuffle, drawn under its ReplicaRNG."""
        es, S = self.engines, len(self.engines)

        def default_perm_fn(i):
            def fn(it):
                with self.rng(i):
                    return torch.randperm(es[i].M, device=es[i].dev).to(torch.int32)
            return fn

        perm_fns = [None] * S if perm_fns is None else list(perm_fns)
        if len(perm_fns) != S:
            raise ValueError(f"{who}one perm_fn (or None) per engine")
        return [f if f is not None else default_perm_fn(i) for i, f in enumerate(perm_fns)]

    def _flags(self, who, perms, active):
        """The active flags of one launch as a list of bools (default: every run), one perm and one flag per engine."""
        S = len(self.engines)
        active = [True] * S if active is None else [bool(x) for x in active]
        if len(perms) != S or len(active) != S:
            raise ValueError(f"{who}: one perm and one active flag per engine")
        return active

    def _perm_and_losses(self, i, perms, active, n_mb, nan_fill=False):
        """Run i's shuffle and its loss rows [n_mb, 3] for one launch -- (None, None) for a run that sits out: it still names
        its own arrays (the table is validated as a whole), but nothing of it is touched."""
        if not active[i] or perms[i] is None:
            return None, None
        dev = self.engines[i].dev
        return (_abi.require_gpu_tensor(perms[i], "perm", torch.int32),
                torch.full((n_mb, 3), float("nan"), dtype=torch.float32, device=dev) if nan_fill
                else torch.empty((n_mb, 3), dtype=torch.float32, device=dev))

    @staticmethod
    def _loss_dict(ls, keys=("loss_r", "loss_c")):
        """A run's per-launch loss rows as the result dict's means (NaN without a launch) and the rows themselves."""
        means = torch.cat(ls, 0).mean(0).tolist() if ls else [float("nan")] * len(keys)
        return {**dict(zip(keys, means)), "losses": ls}

    def check_sync_error(self) -> None:
        """The engine's check_sync_error per run (every run has its own error word); the message names the run."""
        es = self.engines
        if all(torch.is_tensor(getattr(e, "sync_ws", None)) for e in es):
            codes = torch.stack([e.sync_ws[8] for e in es]).cpu().tolist()       # one read for all runs
        else:
            codes = [1] * len(es)
        for i, e in enumerate(es):
            if not codes[i]:
                continue
            try:
                e.check_sync_error()
            except _abi.SpoError as err:
                raise _abi.SpoError(f"replica {i} of {len(es)}: {err}") from None


class PPOLagEngineGroup(_EngineGroup):
    """S ordinary one-GPU PPOLagEngines of one shape (observations, actions, rows, minibatch size) on one device.
    `rngs`: one ReplicaRNG per engine -- the default shuffle of run i is then drawn under rngs[i].
    A group made entirely of one-GPU WidePPOLagEngines whose minibatch step is on the feature-split kernel
    (_feature_split_kernel_ok: hidden [64, 64], up to 512 observations / 32 actions, HumanoidVelocity's 376 / 17) is taken too:
    its learning iterations share one spo_update_iter_ex_ks_multi launch (csrc/update_ks.hip: run r on its own
    3 x ceil(obs_dim / 64) co-XCD workgroups), each bit for bit its own spo_ppo_lag_update_iter_ks / spo_update_iter_ex_ks.
    A third kind: one-GPU WidePPOLagEngines of one shape NONE of which is on the feature-split kernel -- hidden_sizes other than
    [64, 64], act_dim > 32 or obs_dim > 512 --, whose PPO-Lagrangian step is the row-group gradient kernel with the fused
    optimiser (csrc/mlp_rows.hip).  Where _rows_batched holds, the whole minibatches of a learning iteration are replayed from
    one captured graph of spo_wide_rows_step_multi (run r = blockIdx.y of the step's three launches), each run bit for bit its
    own graph-replayed pass; update() only (FOCOPS / CUP step such a group engine by engine).
    `klpen_rows=True` (opt-in): such a row-group group also shares the steps of learning_iter_ex_all -- FOCOPS' step and both of
    CUP's stages -- where _rows_batched_ex holds: one captured graph of spo_wide_rows_ex_step_multi (run r = blockIdx.y of the
    step's five launches) per (batch, kind), each run bit for bit its own graph-replayed learning_iter_ex pass."""

    def __init__(self, engines, rngs=None, klpen_rows=False):
        from safepo.common.engine import PPOLagEngine, WidePPOLagEngine
        engines = list(engines)
        if not engines:
            raise ValueError("PPOLagEngineGroup: no engines")
        # the feature-split form: every engine a WidePPOLagEngine on that kernel (mixed groups are refused below)
        wide = all(type(e) is WidePPOLagEngine for e in engines)
        # the row-group form: every engine a WidePPOLagEngine and none of them on the feature-split kernel
        self._rows = wide and not any(e._feature_split_kernel_ok(e._cfg_struct()) for e in engines)
        self._ks = wide and not self._rows
        self._rows_graphs = {}
        self._klpen_rows = bool(klpen_rows)

        def check_type(i, e):
            if self._rows:
                if e.comm.world_size != 1:
                    raise _abi.SpoError("PPOLagEngineGroup: data-parallel engines cannot be grouped (world size 1 only)")
                if list(e.policy.hidden_sizes) != list(engines[0].policy.hidden_sizes):
                    raise _abi.SpoError(f"PPOLagEngineGroup: engine {i} has hidden_sizes {list(e.policy.hidden_sizes)}, engine 0 has "
                                        f"{list(engines[0].policy.hidden_sizes)}")
            elif self._ks:
                if e.comm.world_size != 1:
                    raise _abi.SpoError("PPOLagEngineGroup: data-parallel engines cannot be grouped (world size 1 only)")
                if not e._feature_split_kernel_ok(e._cfg_struct()):
                    raise _abi.SpoError(f"PPOLagEngineGroup: engine {i} is a WidePPOLagEngine outside the feature-split kernel "
                                        "(hidden [64, 64], obs_dim <= 512, act_dim <= 32, batch <= 64, SPO_WIDE_KS not 0); "
                                        "only those wide engines can be grouped")
            elif type(e) is not PPOLagEngine:
                raise _abi.SpoError(f"PPOLagEngineGroup: engine {i} is a {type(e).__name__}; only the persistent-kernel "
                                    "PPOLagEngine (hidden [64, 64], obs_dim <= 128, act_dim <= 16) can be grouped")

        self._adopt("PPOLagEngineGroup", engines, rngs, PPOLagEngine, check_type)

    # ------------------------------------------------------------------ one learning iteration of every active run
    def batched(self, cfgs=None) -> bool:
        """Does learning_iter_all run as one launch?  Where the two-row-group row-split kernel is the stand-alone form too
        (spo_update_rs_multi_matches_single: the library's own routing answers, nothing of it is repeated here) and all runs
        share the minibatch size.  SPO_FORCE_DP=1 is PPOLagEngine.learning_iter's own switch to the data-parallel entry point."""
        if not self._native:
            return False
        cfgs = cfgs or [e._cfg_struct() for e in self.engines]
        c0 = cfgs[0]
        if any(c.batch != c0.batch for c in cfgs):
            return False
        if self._rows:
            return self._rows_batched(cfgs)
        if self._ks:
            return self._ks_batched(cfgs)
        if os.environ.get("SPO_FORCE_DP", "0") == "1":
            return False
        return bool(self.lib.spo_update_rs_multi_supported(c0.obs_dim, c0.act_dim, c0.batch, len(self.engines))
                    and self.lib.spo_update_rs_multi_matches_single(c0.obs_dim, c0.act_dim, c0.batch))

    def _ks_batched(self, cfgs) -> bool:
        """A group of feature-split WidePPOLagEngines: one spo_update_iter_ex_ks_multi launch where every engine's own step is
        (still: SPO_WIDE_KS is read at every call) on that kernel and the library takes this many runs of the shape
        (spo_update_ks_multi_supported: 16 up to 256 observations, 8 up to 512)."""
        c0 = cfgs[0]
        return (all(e._feature_split_kernel_ok(c) for e, c in zip(self.engines, cfgs))
                and bool(self.lib.spo_update_ks_multi_supported(c0.obs_dim, c0.act_dim, c0.batch, len(self.engines))))

    def _rows_batched(self, cfgs) -> bool:
        """A group of WidePPOLagEngines on the row-group kernel: one spo_wide_rows_step_multi per minibatch step where every
        engine's own pass would be the graph-replayed fused step -- world size 1, wide.rows_grad_ok(batch), the fused optimiser
        on (SPO_WIDE_ROWS_FUSED not 0), 0 < batch <= graph_max_batch with more than two minibatches, not on the feature-split
        kernel (all read at every call, as the engine reads them) -- and the library takes this many runs."""
        es, c0 = self.engines, cfgs[0]
        n_mb = (es[0].M + c0.batch - 1) // max(c0.batch, 1)
        return (os.environ.get("SPO_WIDE_ROWS_FUSED", "1") != "0" and n_mb > 2
                and all(e.comm.world_size == 1 and 0 < c.batch <= e.graph_max_batch and e.wide.rows_grad_ok(c.batch)
                        and not e._feature_split_kernel_ok(c) for e, c in zip(es, cfgs))
                and bool(self.lib.spo_wide_rows_multi_supported(es[0].wide.net_c, es[0].wide.net_a, c0.batch, len(es))))

    def _rows_learning_iter_all(self, cfgs, perms, active):
        """WidePPOLagEngine.learning_iter's graph-replayed pass for the active runs: every run's device clocks from its own host
        step counts (_sync_pow4) and its own PermWindow loaded with its own shuffle, the argument table uploaded once (outside any
        capture), the whole minibatches replayed from ONE captured graph of spo_wide_rows_step_multi (eight steps per graph launch:
        SPO_WIDE_GRAPH_UNROLL, as the engine), the ragged last minibatch through each engine's own eager minibatch_step."""
        from safepo.common.wide import PermWindow
        es, S, e0, lib = self.engines, len(self.engines), self.engines[0], self.lib
        batch, M = int(cfgs[0].batch), e0.M
        n_mb, n_full = (M + batch - 1) // batch, M // batch
        nc, na = e0.wide.net_c, e0.wide.net_a
        ent = self._rows_graphs.get(batch)
        if ent is None:
            ent = self._rows_graphs[batch] = {
                "wins": [PermWindow(M, batch, e.dev) for e in es],
                "loss3": [torch.full((3,), float("nan"), dtype=torch.float32, device=e.dev) for e in es],
                "parts": [e.wide._scratch.setdefault(("parts", batch, False), torch.zeros(
                    int(lib.spo_wide_grad_rows_part_floats(e.wide.P, batch)), dtype=torch.float32, device=e.dev)) for e in es],
                "table": torch.zeros(int(lib.spo_wide_rows_multi_table_bytes(S)), dtype=torch.uint8, device=e0.dev),
                "graphs": None}
        wins = ent["wins"]
        perms64, losses = [None] * S, [None] * S
        reps = (_abi.WideRowsReplica * S)()
        for i, e in enumerate(es):
            r = reps[i]
            r.cfg, r.active = cfgs[i], int(active[i] and perms[i] is not None)
            if not r.active:
                continue
            perms64[i] = _abi.require_gpu_tensor(perms[i], "perm", torch.int32).long()
            losses[i] = torch.empty((n_mb, 3), dtype=torch.float32, device=e.dev)
            e._sync_pow4()
            wins[i].load(perms64[i])
            d, M_ = e.buffer.data, e.M
            r.theta, r.adam_m, r.adam_v = _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v)
            r.grad, r.parts = _abi.ptr(e.flat_grad), _abi.ptr(ent["parts"][i])
            r.obs, r.act, r.logp_old = _abi.ptr(d["obs"]), _abi.ptr(d["act"]), _abi.ptr(d["log_prob"])
            r.target_r, r.target_c, r.adv = _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(e.buffer.adv_mix)
            r.perm, r.cursor_dev, r.pow4_dev = _abi.ptr(wins[i].perm), _abi.ptr(wins[i].cursor), _abi.ptr(e.pow4)
            r.losses3_out, r.scalars4_out = _abi.ptr(ent["loss3"][i]), _abi.ptr(e.scal4)
            r.partial_ws, r.partial_capacity = _abi.ptr(e.loss_partials), e.loss_partials.numel()
            r.loss_log_dev = _abi.ptr(wins[i].loss_log)
        idx = [i for i in range(S) if reps[i].active]
        if not idx:
            return losses
        table = ent["table"]

        def step():
            _abi.check(lib.spo_wide_rows_step_multi(_abi.ptr(table), S, nc, na, batch, _abi.stream_ptr()), "spo_wide_rows_step_multi")

        _abi.check(lib.spo_wide_rows_multi_upload(_abi.ptr(table), reps, S, nc, na, batch, batch, _abi.stream_ptr()),
                   "spo_wide_rows_multi_upload")
        if ent["graphs"] is None:
            # first use: one eager step for the lazy per-kernel set-up, its effects on every taking-part run's parameters / moments /
            # clocks / gradient / cursor undone (as _graphed_pass does for one engine), then the captures
            state = [t for i in idx for t in (es[i].policy.theta, es[i].adam_m, es[i].adam_v, es[i].pow4, es[i].flat_grad, wins[i].cursor)]
            snap = [t.clone() for t in state]
            step()
            for t, b in zip(state, snap):
                t.copy_(b)
            torch.cuda.synchronize(e0.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                step()
            unroll = max(1, int(os.environ.get("SPO_WIDE_GRAPH_UNROLL", "8")))
            g_many = None
            if unroll > 1:
                g_many = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_many, capture_error_mode="thread_local"):
                    for _ in range(unroll):
                        step()
            ent["graphs"] = (g, g_many, unroll)         # (the table, windows, loss and part buffers live in `ent` beside them)
        g, g_many, unroll = ent["graphs"]
        done = 0
        if g_many is not None:
            for _ in range(n_full // unroll):
                g_many.replay()
            done = (n_full // unroll) * unroll
        for _ in range(n_full - done):
            g.replay()
        for i in idx:
            losses[i][:n_full].copy_(wins[i].loss_log[:n_full])
            es[i].adam_step += n_full
            for k in range(n_full, n_mb):               # (the ragged last minibatch: eager, host clocks, as stand-alone)
                es[i].minibatch_step(perms64[i][k * batch:(k + 1) * batch], losses[i][k], cfg=cfgs[i])
        return losses

    def _rows_batched_ex(self, cfgs, actor_loss, actor_only) -> bool:
        """A klpen_rows group on the row-group kernel: one spo_wide_rows_ex_step_multi per minibatch step of learning_iter_ex_all
        where every engine's own pass would be the graph-replayed row-group step -- world size 1, _row_group_step_ok(batch,
        actor_loss, actor_only), 0 < batch <= graph_max_batch with more than two minibatches, not on the feature-split kernel
        (all read at every call, as the engine reads them) -- and the library takes this many runs of the shape and kind."""
        if not self._klpen_rows:
            return False
        es, c0 = self.engines, cfgs[0]
        n_mb = (es[0].M + c0.batch - 1) // max(c0.batch, 1)
        return (n_mb > 2
                and all(e.comm.world_size == 1 and 0 < c.batch <= e.graph_max_batch
                        and e._row_group_step_ok(c.batch, actor_loss, actor_only)
                        and not e._feature_split_kernel_ok(c) for e, c in zip(es, cfgs))
                and bool(self.lib.spo_wide_rows_ex_multi_supported(es[0].wide.net_c, es[0].wide.net_a, c0.batch, int(actor_loss),
                                                                   int(bool(actor_only)), len(es))))

    def _rows_learning_iter_ex_all(self, cfgs, perms, advs, actor_loss, kl_bounds, pg_coefs, actor_only, active):
        """WidePPOLagEngine.learning_iter_ex's graph-replayed pass for the active runs, as _rows_learning_iter_all does it for the
        PPO-Lagrangian step: every run's device clocks from its own host step counts (_sync_pow4) and its own PermWindow loaded
        with its own shuffle, the argument table -- kl_bound, pg_coef and the advantage among its entries, so one capture per
        (batch, kind) serves every epoch -- uploaded once per pass outside any capture, the whole minibatches replayed from ONE
        captured graph of spo_wide_rows_ex_step_multi (eight steps per graph launch: SPO_WIDE_GRAPH_UNROLL, as the engine), the
        ragged last minibatch through each engine's own eager minibatch_step_ex, the host clocks advanced as learning_iter_ex
        advances them."""
        from safepo.common.wide import PermWindow
        es, S, e0, lib = self.engines, len(self.engines), self.engines[0], self.lib
        batch, M = int(cfgs[0].batch), e0.M
        n_mb, n_full = (M + batch - 1) // batch, M // batch
        nc, na = e0.wide.net_c, e0.wide.net_a
        klpen, actor_only = actor_loss == _abi.ACTOR_LOSS_KL_PENALTY, bool(actor_only)
        key = ("ex", batch, int(actor_loss), actor_only)
        ent = self._rows_graphs.get(key)
        if ent is None:
            # (the part buffers are the engines' own for this step: what their stand-alone launches fill)
            def parts_of(e):
                if klpen:
                    return e.wide._scratch.setdefault(("klpen_parts", batch, actor_only), torch.zeros(
                        int(lib.spo_wide_kl_penalty_rows_part_floats(e.wide.P, e.wide.off_ls, batch)), dtype=torch.float32, device=e.dev))
                return e.wide._scratch.setdefault(("parts", batch, False), torch.zeros(
                    int(lib.spo_wide_grad_rows_part_floats(e.wide.P, batch)), dtype=torch.float32, device=e.dev))
            ent = self._rows_graphs[key] = {
                "wins": [PermWindow(M, batch, e.dev) for e in es],
                "loss3": [torch.full((3,), float("nan"), dtype=torch.float32, device=e.dev) for e in es],
                "parts": [parts_of(e) for e in es],
                "table": torch.zeros(int(lib.spo_wide_rows_ex_multi_table_bytes(S)), dtype=torch.uint8, device=e0.dev),
                "graphs": None}
        wins = ent["wins"]
        perms64, losses, keep = [None] * S, [None] * S, []
        reps = (_abi.WideRowsExReplica * S)()
        for i, e in enumerate(es):
            r = reps[i]
            r.cfg, r.active = cfgs[i], int(active[i] and perms[i] is not None)
            if not r.active:
                continue
            perms64[i] = _abi.require_gpu_tensor(perms[i], "perm", torch.int32).long()
            adv = _abi.require_gpu_tensor(advs[i], "adv", torch.float32)
            keep.append(adv)
            losses[i] = torch.full((n_mb, 3), float("nan"), dtype=torch.float32, device=e.dev)
            e._sync_pow4()
            wins[i].load(perms64[i])
            d = e.buffer.data
            r.theta, r.adam_m, r.adam_v = _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v)
            r.grad, r.parts = _abi.ptr(e.flat_grad), _abi.ptr(ent["parts"][i])
            r.obs, r.act, r.logp_old = _abi.ptr(d["obs"]), _abi.ptr(d["act"]), _abi.ptr(d["log_prob"])
            r.target_r, r.target_c, r.adv = _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(adv)
            r.perm, r.cursor_dev, r.pow4_dev = _abi.ptr(wins[i].perm), _abi.ptr(wins[i].cursor), _abi.ptr(e.pow4)
            r.losses3_out, r.scalars4_out = _abi.ptr(ent["loss3"][i]), _abi.ptr(e.scal4)
            r.partial_ws, r.partial_capacity = _abi.ptr(e.loss_partials), e.loss_partials.numel()
            r.loss_log_dev = _abi.ptr(wins[i].loss_log)
            if klpen:
                r.old_mean, r.old_std = _abi.ptr(e.mean_old), _abi.ptr(e.std_old)
                r.kl_bound, r.pg_coef = float(kl_bounds[i]), float(pg_coefs[i])
        idx = [i for i in range(S) if reps[i].active]
        if not idx:
            return losses
        table = ent["table"]

        def step():
            _abi.check(lib.spo_wide_rows_ex_step_multi(_abi.ptr(table), S, nc, na, batch, int(actor_loss), int(actor_only),
                                                       _abi.stream_ptr()), "spo_wide_rows_ex_step_multi")

        _abi.check(lib.spo_wide_rows_ex_multi_upload(_abi.ptr(table), reps, S, nc, na, batch, batch, int(actor_loss), int(actor_only),
                                                     _abi.stream_ptr()), "spo_wide_rows_ex_multi_upload")
        if ent["graphs"] is None:
            # first use: one eager step for the lazy per-kernel set-up, its effects on every taking-part run's parameters / moments /
            # clocks / gradient / cursor undone (as _graphed_pass does for one engine), then the captures
            state = [t for i in idx for t in (es[i].policy.theta, es[i].adam_m, es[i].adam_v, es[i].pow4, es[i].flat_grad, wins[i].cursor)]
            snap = [t.clone() for t in state]
            step()
            for t, b in zip(state, snap):
                t.copy_(b)
            torch.cuda.synchronize(e0.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                step()
            unroll = max(1, int(os.environ.get("SPO_WIDE_GRAPH_UNROLL", "8")))
            g_many = None
            if unroll > 1:
                g_many = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g_many, capture_error_mode="thread_local"):
                    for _ in range(unroll):
                        step()
            ent["graphs"] = (g, g_many, unroll)         # (the table, windows, loss and part buffers live in `ent` beside them)
        g, g_many, unroll = ent["graphs"]
        done = 0
        if g_many is not None:
            for _ in range(n_full // unroll):
                g_many.replay()
            done = (n_full // unroll) * unroll
        for _ in range(n_full - done):
            g.replay()
        for i in idx:
            e = es[i]
            losses[i][:n_full].copy_(wins[i].loss_log[:n_full])
            if actor_only:
                e.adam_step_actor_extra += n_full
            else:
                e.adam_step += n_full
            for k in range(n_full, n_mb):               # (the ragged last minibatch: eager, host clocks, as stand-alone)
                e.minibatch_step_ex(perms64[i][k * batch:(k + 1) * batch], advs[i], losses[i][k], actor_loss, kl_bounds[i], pg_coefs[i],
                                    actor_only, cfg=cfgs[i])
                if actor_only:
                    e.adam_step_actor_extra += 1
                else:
                    e.adam_step += 1
        return losses

    def _launch_ex(self, entry, cfgs, perms, advs, actor_loss, kl_bounds, pg_coefs, actor_only, active, nan_fill=True):
        """One launch of `entry` (spo_update_iter_ex_multi or spo_update_iter_ex_ks_multi) for the active runs; the clocks
        advance as learning_iter_ex advances them.  nan_fill=False: the feature-split PPO-Lagrangian step -- loss rows left
        uninitialised and the actor on the critics' clock, as WidePPOLagEngine.learning_iter launches it."""
        S, e0 = len(self.engines), self.engines[0]
        n_mb = (e0.M + cfgs[0].batch - 1) // cfgs[0].batch
        reps = (_abi.UpdateExReplica * S)()
        losses = [None] * S
        for i, e in enumerate(self.engines):
            d = e.buffer.data
            perm, losses[i] = self._perm_and_losses(i, perms, active, n_mb, nan_fill)
            adv = _abi.require_gpu_tensor(advs[i], "adv", torch.float32)
            r = reps[i]
            r.theta, r.adam_m, r.adam_v = _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v)
            r.adam_step_critics, r.adam_step_actor = e.adam_step, e.adam_step + (e.adam_step_actor_extra if nan_fill else 0)
            r.obs, r.act, r.logp_old = _abi.ptr(d["obs"]), _abi.ptr(d["act"]), _abi.ptr(d["log_prob"])
            r.target_r, r.target_c, r.adv = _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(adv)
            r.perm, r.old_mean, r.old_std = _abi.ptr(perm), _abi.ptr(e.mean_old), _abi.ptr(e.std_old)
            r.kl_bound, r.pg_coef, r.losses_out = float(kl_bounds[i]), float(pg_coefs[i]), _abi.ptr(losses[i])
            r.sync_ws, r.cfg, r.active = _abi.ptr(e.sync_ws), cfgs[i], int(active[i])
        _abi.check(getattr(self.lib, entry)(reps, S, e0.M, int(actor_loss), int(bool(actor_only)), _abi.stream_ptr()), entry)
        for i, e in enumerate(self.engines):
            if active[i]:
                if actor_only:
                    e.adam_step_actor_extra += n_mb
                else:
                    e.adam_step += n_mb
        return losses

    def learning_iter_all(self, perms, active=None):
        """PPOLagEngine.learning_iter(perms[i]) for every run i with active[i] (default: all): one
        spo_ppo_lag_update_iter_multi launch where batched(), else one launch per run -- the same results.  Returns the
        per-minibatch losses [n_mb, 3] per run (None for a run that did not take part)."""
        S = len(self.engines)
        active = self._flags("learning_iter_all", perms, active)
        cfgs = [e._cfg_struct() for e in self.engines] if self._native else None
        if not self.batched(cfgs):
            return [e.learning_iter(perms[i]) if active[i] else None for i, e in enumerate(self.engines)]
        if self._rows:
            return self._rows_learning_iter_all(cfgs, perms, active)
        if self._ks:
            # spo_ppo_lag_update_iter_ks is spo_update_iter_ex_ks with the clipped surrogate on adv_mix and equal clocks
            return self._launch_ex("spo_update_iter_ex_ks_multi", cfgs, perms, [e.buffer.adv_mix for e in self.engines],
                                   _abi.ACTOR_LOSS_CLIP, [float("inf")] * S, [0.0] * S, False, active, nan_fill=False)
        e0 = self.engines[0]
        n_mb = (e0.M + cfgs[0].batch - 1) // cfgs[0].batch
        reps = (_abi.UpdateReplica * S)()
        losses = [None] * S
        for i, e in enumerate(self.engines):
            d, b = e.buffer.data, e.buffer
            perm, losses[i] = self._perm_and_losses(i, perms, active, n_mb)
            r = reps[i]
            r.theta, r.adam_m, r.adam_v, r.adam_step = _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v), e.adam_step
            r.obs, r.act, r.logp_old = _abi.ptr(d["obs"]), _abi.ptr(d["act"]), _abi.ptr(d["log_prob"])
            r.target_r, r.target_c, r.adv = _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(b.adv_mix)
            r.perm, r.losses_out = _abi.ptr(perm), _abi.ptr(losses[i])
            r.sync_ws, r.cfg, r.active = _abi.ptr(e.sync_ws), cfgs[i], int(active[i])
        _abi.check(self.lib.spo_ppo_lag_update_iter_multi(reps, S, e0.M, _abi.stream_ptr()), "spo_ppo_lag_update_iter_multi")
        for i, e in enumerate(self.engines):
            if active[i]:
                e.adam_step += n_mb
        return losses

    # ------------------------------------------------------------------ the epoch's update of every run
    def _read_kls(self, idx) -> list:
        """kl_read() of the runs idx after their kl_launch(): ONE host synchronisation for all of them."""
        es = [self.engines[i] for i in idx]
        if all(torch.is_tensor(getattr(e, "kl_sum", None)) for e in es):
            sums = torch.cat([e.kl_sum.reshape(1) for e in es]).cpu().tolist()
            return [float(s) / float(e.M * e.comm.world_size) for s, e in zip(sums, es)]
        return [e.kl_read() for e in es]

    def update(self, lams, perm_fns=None):
        """PPOLagEngine.update for every run: GAE, the old-distribution snapshot, then learning iterations with KL early
        stopping under the run's own target_kl and learning_iters.  A run that stops sits out the remaining launches; the loop
        ends when none is active.  Per run the order of shuffle draws and KL reads is the stand-alone loop's (the next pass's
        shuffle is drawn before the KL is read, also on the pass that stops).  Returns the list of update()'s dicts."""
        es, S = self.engines, len(self.engines)
        if len(lams) != S:
            raise ValueError("update: one multiplier per engine")
        for e, lam in zip(es, lams):
            e.buffer.compute_gae(lam, e.comm)
            e.snapshot_old_distribution()
        all_losses, stop_iter, kl = self._kl_stopped_loop_all(self._default_perm_fns(perm_fns), [0] * S, self.learning_iter_all,
                                                              draw_ahead=True)
        self.check_sync_error()
        outs = []
        for i, e in enumerate(es):
            e.buffer.reset()
            outs.append({"stop_iter": stop_iter[i], "kl": kl[i], **self._loss_dict(all_losses[i], ("loss_r", "loss_c", "loss_pi"))})
        return outs

    # ------------------------------------------------------------------ FOCOPS / CUP: spo_update_iter_ex of every active run
    def batched_ex(self, actor_loss: int, cfgs=None, actor_only: bool = False) -> bool:
        """Does learning_iter_ex_all run as one launch (spo_update_iter_ex_multi)?  Where the stand-alone spo_update_iter_ex runs
        the four-wave kernel itself (spo_update_ex_multi_matches_single: the library's own routing answers -- always with the
        KL-penalty loss; with the clipped surrogate where the main + helper kernel does not take the launch, i.e. above 64
        observations under default routing) and all runs share the minibatch size."""
        if not self._native:
            return False
        cfgs = cfgs or [e._cfg_struct() for e in self.engines]
        c0 = cfgs[0]
        if any(c.batch != c0.batch for c in cfgs):
            return False
        if self._rows:
            # (without klpen_rows: engine by engine; with it: the table-driven row-group step, spo_wide_rows_ex_step_multi)
            return self._rows_batched_ex(cfgs, actor_loss, actor_only)
        if self._ks:
            return self._ks_batched(cfgs)
        return bool(self.lib.spo_update_ex_multi_supported(c0.obs_dim, c0.act_dim, c0.batch, int(actor_loss), len(self.engines))
                    and self.lib.spo_update_ex_multi_matches_single(c0.obs_dim, c0.act_dim, c0.batch, int(actor_loss)))

    def learning_iter_ex_all(self, perms, advs, actor_loss: int = 0, kl_bounds=None, pg_coefs=None, actor_only: bool = False,
                             active=None):
        """PPOLagEngine.learning_iter_ex(perms[i], advs[i], actor_loss, kl_bounds[i], pg_coefs[i], actor_only) for every run i
        with active[i] (default: all): one spo_update_iter_ex_multi launch where batched_ex(actor_loss), else one launch per
        run -- the same results.  The run's adam_step (or, with actor_only, adam_step_actor_extra) advances exactly as
        learning_iter_ex advances it.  Returns the per-minibatch losses [n_mb, 3] per run (None for a run that sat out)."""
        S = len(self.engines)
        active = [True] * S if active is None else [bool(x) for x in active]
        kl_bounds = [float("inf")] * S if kl_bounds is None else list(kl_bounds)
        pg_coefs = [0.0] * S if pg_coefs is None else list(pg_coefs)
        if not (len(perms) == len(advs) == len(active) == len(kl_bounds) == len(pg_coefs) == S):
            raise ValueError("learning_iter_ex_all: one perm, adv, kl_bound, pg_coef and active flag per engine")
        cfgs = [e._cfg_struct() for e in self.engines] if self._native else None
        if not self.batched_ex(actor_loss, cfgs, actor_only):
            return [e.learning_iter_ex(perms[i], advs[i], actor_loss, kl_bounds[i], pg_coefs[i], actor_only) if active[i] else None
                    for i, e in enumerate(self.engines)]
        if self._rows:
            return self._rows_learning_iter_ex_all(cfgs, perms, advs, actor_loss, kl_bounds, pg_coefs, actor_only, active)
        entry = "spo_update_iter_ex_ks_multi" if self._ks else "spo_update_iter_ex_multi"
        return self._launch_ex(entry, cfgs, perms, advs, actor_loss, kl_bounds, pg_coefs, actor_only, active)

    def _kl_stopped_loop_all(self, perm_fns, it0s, launch, draw_ahead=False):
        """PPOLagEngine._kl_stopped_loop for every run, one `launch(perms, active)` per pass: run i draws the shuffle
        perm_fns[i](it0s[i] + it) at the start of pass `it` and none after it stopped (its own target_kl, its own learning_iters);
        a run that stopped sits out the later launches.  The KLs of a pass are read in one host read.
        draw_ahead: PPOLagEngine.update's order instead -- pass 0's shuffle before the loop, and the next pass's shuffle of every
        run that took part (and has iterations left) BEFORE the pass's KLs are read, so also on the pass whose KL stops the run.
        Returns (losses, stop_iter, kl), each a list over the runs."""
        es, S = self.engines, len(self.engines)
        n_its = [e.cfg["learning_iters"] for e in es]
        active = [n > 0 for n in n_its]
        all_losses, stop_iter, kl = [[] for _ in range(S)], [0] * S, [1.0] * S
        perms = [perm_fns[i](it0s[i]) if active[i] else None for i in range(S)] if draw_ahead else None
        it = 0
        while any(active):
            idx = [i for i in range(S) if active[i]]
            if not draw_ahead:
                perms = [perm_fns[i](it0s[i] + it) if active[i] else None for i in range(S)]
            losses = launch(perms, list(active))
            for i in idx:
                all_losses[i].append(losses[i])
                es[i].kl_launch()
            if draw_ahead:
                for i in idx:
                    perms[i] = perm_fns[i](it0s[i] + it + 1) if it + 1 < n_its[i] else None
            for i, v in zip(idx, self._read_kls(idx)):
                kl[i] = v
                stop_iter[i] += 1
                if v > es[i].cfg["target_kl"] or it + 1 >= n_its[i]:
                    active[i] = False
            it += 1
        return all_losses, stop_iter, kl

    def update_focops(self, lams, perm_fns=None, focops_lam: float = 1.5):
        """PPOLagEngine.update_focops for every run: GAE and the old-distribution snapshot seed by seed, then the KL-stopped
        loop with one spo_update_iter_ex_multi launch per pass.  Returns the list of update_focops()'s dicts."""
        es, S = self.engines, len(self.engines)
        if len(lams) != S:
            raise ValueError("update_focops: one multiplier per engine")
        perm_fns = self._default_perm_fns(perm_fns)
        for e, lam in zip(es, lams):
            e.buffer.compute_gae(lam, e.comm)
            e.snapshot_old_distribution()
        advs = [e.buffer.adv_mix for e in es]
        kl_bounds, pg_coefs = [e.cfg["target_kl"] for e in es], [1.0 / focops_lam] * S
        losses, stop_iter, kl = self._kl_stopped_loop_all(perm_fns, [0] * S, lambda perms, active: self.learning_iter_ex_all(
            perms, advs, _abi.ACTOR_LOSS_KL_PENALTY, kl_bounds, pg_coefs, False, active))
        self.check_sync_error()
        outs = []
        for i, e in enumerate(es):
            e.buffer.reset()
            outs.append({"stop_iter": stop_iter[i], "kl": kl[i], **self._loss_dict(losses[i], ("loss_r", "loss_c", "loss_pi"))})
        return outs

    def update_cup(self, lams, perm_fns=None, cup_lambda: float = 0.95):
        """PPOLagEngine.update_cup for every run: stage one (clipped surrogate on adv_r) for all runs, the second snapshot run by
        run, then stage two (the actor alone, KL penalty) -- run i's shuffle index going on from its own stage-one stop_iter.
        A stage is one launch per pass where batched_ex says so for its loss, else one launch per run per pass (under default
        routing: stage one up to 64 observations, which the stand-alone run puts on the main + helper kernel)."""
        es, S = self.engines, len(self.engines)
        if len(lams) != S:
            raise ValueError("update_cup: one multiplier per engine")
        perm_fns = self._default_perm_fns(perm_fns)
        for e in es:
            e.buffer.compute_gae(0.0, e.comm)              # lambda 0: adv_mix == adv_r exactly (cup.py:285)
            e.snapshot_old_distribution()
        adv_r = [e.buffer.adv_mix for e in es]
        losses, stop_iter, kl = self._kl_stopped_loop_all(perm_fns, [0] * S, lambda perms, active: self.learning_iter_ex_all(
            perms, adv_r, _abi.ACTOR_LOSS_CLIP, None, None, False, active))
        for e in es:
            e.snapshot_old_distribution()                  # cup.py:355-358
        coefs = [(1 - e.cfg["gamma"] * cup_lambda) / (1 - e.cfg["gamma"]) for e in es]
        adv_c = [e.buffer.data["adv_c"] for e in es]
        pg_coefs = [-float(lam) * coef for lam, coef in zip(lams, coefs)]
        losses2, stop_iter2, kl2 = self._kl_stopped_loop_all(perm_fns, stop_iter, lambda perms, active: self.learning_iter_ex_all(
            perms, adv_c, _abi.ACTOR_LOSS_KL_PENALTY, [float("inf")] * S, pg_coefs, True, active))
        self.check_sync_error()
        outs = []
        for i, e in enumerate(es):
            e.buffer.reset()
            outs.append({"stop_iter": stop_iter[i], "second_stage_stop_iter": stop_iter2[i], "kl": kl2[i], "kl_first_stage": kl[i],
                         **self._loss_dict(losses[i], ("loss_r", "loss_c", "loss_pi")), "second_stage_losses": losses2[i]})
        return outs


class CPOEngineGroup(_EngineGroup):
    """S one-GPU CPOEngines (cpo, pcpo, rcpo, trpo_lag, trpo, natural_pg) of one shape on one device whose critic fits share ONE
    persistent launch per iteration (spo_critic_fit_iter_multi, csrc/update_rs.hip): run r on its own eight co-XCD workgroups
    (2 critics x 4 row groups), each bit for bit its own spo_critic_fit_iter.  The full-batch actor updates already fill the
    GPU and stay one run after the other.  `rngs`: one ReplicaRNG per engine -- run i's default shuffle is drawn under rngs[i].
    `split_form=True` also admits WideCPOEngines whose critics are on the persistent kernel at 65-128 observations (up to 32):
    their two-replica split critic fits share one launch per iteration (spo_critic_fit_iter_split_multi, csrc/update.hip: run r
    on its own four co-XCD workgroups), each bit for bit its own spo_critic_fit_iter_split; see batched_split().
    `ks_form=True` also admits WideCPOEngines at 129-512 observations with hidden [64, 64] (HumanoidVelocity's 376 / 17), whose
    critic fit runs on the feature-split kernel: their critic fits share one launch per iteration
    (spo_critic_fit_iter_ks_multi, csrc/update_ks.hip: run r on its own 2 x ceil(obs_dim / 64) workgroups of XCD label r mod 8;
    up to 16 runs up to 384 observations, 8 up to 512), each bit for bit its own spo_critic_fit_iter_ks; see batched_ks()."""

    KS_MIN_OBS, KS_MAX_OBS = _abi.MAX_OBS + 1, 512      # above the persistent two-critic kernel, inside the feature-split kernel

    def __init__(self, engines, rngs=None, split_form=False, ks_form=False):
        from safepo.single_agent.cpo import CPOEngine, WideCPOEngine
        engines = list(engines)
        if not engines:
            raise ValueError("CPOEngineGroup: no engines")
        self.split_form, self.ks_form = bool(split_form), bool(ks_form)

        def takes_split(e):
            return (self.split_form and type(e) is WideCPOEngine and getattr(e, "_critics_on_persistent_kernel", False)
                    and 65 <= e.D <= _abi.MAX_OBS)

        def takes_ks(e):
            return (self.ks_form and type(e) is WideCPOEngine and not getattr(e, "_critics_on_persistent_kernel", False)
                    and self.KS_MIN_OBS <= e.D <= self.KS_MAX_OBS and list(e.policy.hidden_sizes) == [64, 64])

        self._takes_ks = takes_ks
        # the split form's launch holds up to 32 runs (four workgroups each) at 65-128 observations; the feature-split form what
        # 24 workgroups per XCD leave of its 2 x ceil(obs_dim / 64) a run (spo_critic_fit_ks_multi_supported); everything else 24
        if takes_ks(engines[0]):
            lib = _abi.load()
            cap = max(n for n in range(1, _abi.KS_MAX_REPLICAS + 1) if lib.spo_critic_fit_ks_multi_supported(engines[0].D, 1, n))
        else:
            cap = _abi.CRITIC_SPLIT_MAX_REPLICAS if takes_split(engines[0]) else _abi.RS_CRITIC_MAX_REPLICAS
        if len(engines) > cap:
            raise _abi.SpoError(f"CPOEngineGroup: {len(engines)} engines; at most {cap} critic fits share a launch")

        def check_type(i, e):
            if not (takes_split(e) or takes_ks(e)) and type(e) is not CPOEngine:
                raise _abi.SpoError(f"CPOEngineGroup: engine {i} is a {type(e).__name__}; only the persistent-kernel "
                                    "CPOEngine (hidden [64, 64], obs_dim <= 64, act_dim <= 16) can be grouped")

        self._adopt("CPOEngineGroup", engines, rngs, CPOEngine, check_type)

    def batched(self, cfgs=None) -> bool:
        """Does critic_fit_all run one launch per iteration?  Where the four-row-group row-split kernel is the stand-alone
        form too (spo_critic_fit_multi_matches_single: the library's own routing answers; SPO_UPDATE_FORM < 3 says no), no
        engine takes its two-replica split form (SPO_CPO_SPLIT=force) and all runs share the minibatch size."""
        if not self._native:
            return False
        cfgs = cfgs or [e._cfg_struct() for e in self.engines]
        c0 = cfgs[0]
        if any(c.batch != c0.batch for c in cfgs):
            return False
        if not (self.lib.spo_critic_fit_multi_supported(c0.obs_dim, c0.act_dim, c0.batch, len(self.engines))
                and self.lib.spo_critic_fit_multi_matches_single(c0.obs_dim, c0.act_dim, c0.batch)):
            return False
        return all(e._split_setup() is None for e in self.engines)

    def _fit_iter(self, entry, who, perms, active):
        """One launch of `entry` (spo_critic_fit_iter_multi or spo_critic_fit_iter_ks_multi: one table type) for the active runs."""
        S, e0 = len(self.engines), self.engines[0]
        active = self._flags(who, perms, active)
        cfgs = [e._cfg_struct() for e in self.engines]
        n_mb = (e0.M + cfgs[0].batch - 1) // cfgs[0].batch
        reps = (_abi.CriticFitReplica * S)()
        losses = [None] * S
        for i, e in enumerate(self.engines):
            d = e.buffer.data
            perm, losses[i] = self._perm_and_losses(i, perms, active, n_mb)
            r = reps[i]
            r.theta, r.adam_m, r.adam_v, r.adam_step = _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v), e.adam_step
            r.obs, r.target_r, r.target_c = _abi.ptr(d["obs"]), _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"])
            r.perm, r.losses_out, r.stale_sq_io = _abi.ptr(perm), _abi.ptr(losses[i]), _abi.ptr(e.stale_sq)
            r.sync_ws, r.cfg, r.active = _abi.ptr(e.sync_ws), cfgs[i], int(active[i])
        _abi.check(getattr(self.lib, entry)(reps, S, e0.M, _abi.stream_ptr()), entry)
        for i, e in enumerate(self.engines):
            if active[i]:
                e.adam_step += n_mb
        return losses

    def fit_iter_all(self, perms, active=None):
        """One critic-fit iteration (ceil(M / batch) minibatch steps) of every run i with active[i] in ONE launch; adam_step
        advances per run.  Returns the losses [n_mb, 3] per run (columns 0, 1 are written; None for a run that sat out)."""
        return self._fit_iter("spo_critic_fit_iter_multi", "fit_iter_all", perms, active)

    def _fit_loop(self, perm_fns, fit_iter):
        """learning_iters iterations per run (a run with fewer sits out the later launches), one fit_iter(perms, active) each,
        every iteration's shuffle drawn before its launch.  Returns the critics' loss columns per run and iteration."""
        S = len(self.engines)
        n_its = [e.cfg["learning_iters"] for e in self.engines]
        all_losses = [[] for _ in range(S)]
        for it in range(max(n_its)):
            active = [it < n for n in n_its]
            perms = [perm_fns[i](it) if active[i] else None for i in range(S)]
            losses = fit_iter(perms, active)
            for i in range(S):
                if active[i]:
                    all_losses[i].append(losses[i][:, :2])
        return all_losses

    def _backup(self):
        """Every run's critics, moments, stale norm and adam_step before a critic fit that restores them on an exchange error."""
        return [(e.policy.theta.clone(), e.adam_m.clone(), e.adam_v.clone(), e.stale_sq.clone(), e.adam_step) for e in self.engines]

    def _restore(self, backups) -> None:
        for e, b in zip(self.engines, backups):
            e.sync_ws[8] = 0
            e.policy.theta.copy_(b[0]); e.adam_m.copy_(b[1]); e.adam_v.copy_(b[2]); e.stale_sq.copy_(b[3])
            e.adam_step = b[4]

    # ------------------------------------------------------------------ the two-replica split form (65-128 observations)
    def batched_split(self) -> bool:
        """Does critic_fit_all run the split critic fits of all runs as one launch per iteration
        (spo_critic_fit_iter_split_multi)?  Only in a group built with split_form=True, where every run steps through
        minibatches of 128 rows that divide its rows, the library has the form for this shape and run count
        (spo_critic_fit_split_multi_supported) and every engine's own critic_fit would take the split form too
        (_split_setup() returns its state: the exchange regions and the second replica's arrays)."""
        if not (self.split_form and self._native):
            return False
        es = self.engines
        if any(int(e.cfg.get("batch_size", 0)) != 128 for e in es) or es[0].M % 128 != 0:
            return False
        if not self.lib.spo_critic_fit_split_multi_supported(es[0].D, 64, len(es)):
            return False
        return all(e._split_setup() is not None for e in es)

    @staticmethod
    def _split_cfg(e):
        """What WideCPOEngine hands the stand-alone split launch: act_dim capped at MAX_ACT (the critics' layout is act-free),
        64 rows per half."""
        cfg = e._cfg_struct()
        cfg.act_dim = min(cfg.act_dim, _abi.MAX_ACT)
        cfg.batch = 64
        return cfg

    def fit_iter_split_all(self, perms, active=None):
        """One iteration of CPOEngine._critic_fit_split's loop for every run i with active[i] in ONE launch: the shuffle cut
        into its 64-column halves, both replicas stepped, the run's step tag and adam_step advanced.  Returns (l0 + l1) * 0.5
        per run ([n_mb, 3], columns 0 and 1 are written; None for a run that sat out)."""
        S, e0 = len(self.engines), self.engines[0]
        active = self._flags("fit_iter_split_all", perms, active)
        n_mb, half = e0.M // 128, e0.M // 2
        reps = (_abi.CriticFitSplitReplica * S)()
        halves = [None] * S
        for i, e in enumerate(self.engines):
            r = reps[i]
            r.cfg, r.active = self._split_cfg(e), int(active[i])
            if not active[i]:
                continue                                    # (a run that sits out names nothing: nothing of it is touched)
            st, d = e._split_setup(), e.buffer.data
            perm = _abi.require_gpu_tensor(perms[i], "perm", torch.int32).view(n_mb, 128)
            p0, p1 = perm[:, :64].contiguous().view(-1), perm[:, 64:].contiguous().view(-1)
            l0 = torch.empty((n_mb, 3), dtype=torch.float32, device=e.dev)
            l1 = torch.empty_like(l0)
            halves[i] = (p0, p1, l0, l1)
            r.theta0, r.adam_m0, r.adam_v0 = _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v)
            r.theta1, r.adam_m1, r.adam_v1 = _abi.ptr(st["theta1"]), _abi.ptr(st["m1"]), _abi.ptr(st["v1"])
            r.adam_step = e.adam_step
            r.obs, r.target_r, r.target_c = _abi.ptr(d["obs"]), _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"])
            r.perm0, r.perm1 = _abi.ptr(p0), _abi.ptr(p1)
            r.stale_sq_io0, r.stale_sq_io1 = _abi.ptr(e.stale_sq), _abi.ptr(st["stale1"])
            r.losses0, r.losses1 = _abi.ptr(l0), _abi.ptr(l1)
            r.sync_ws0, r.sync_ws1 = _abi.ptr(e.sync_ws), _abi.ptr(st["sync_ws"])
            r.regions2[0], r.regions2[1] = st["regions"][0], st["regions"][1]
            r.step0 = st["step"] & 0xFFFFFFFF
        _abi.check(self.lib.spo_critic_fit_iter_split_multi(reps, S, half, _abi.stream_ptr()), "spo_critic_fit_iter_split_multi")
        losses = [None] * S
        for i, e in enumerate(self.engines):
            if active[i]:
                e._split_setup()["step"] += n_mb
                e.adam_step += n_mb
                losses[i] = (halves[i][2] + halves[i][3]) * 0.5
        return losses

    def _critic_fit_all_split(self, perm_fns):
        """critic_fit_all where batched_split(): CPOEngine._critic_fit_split for every run, one launch per iteration.  An
        exchange error (a workgroup of the launch was not resident) is not degraded to another form: every run's state is
        restored and the error raised, naming the run."""
        es, S = self.engines, len(self.engines)
        sts = [e._split_setup() for e in es]
        backups = self._backup()
        for e, st in zip(es, sts):                      # the second replica starts as a copy of the first
            st["theta1"].copy_(e.policy.theta); st["m1"].copy_(e.adam_m); st["v1"].copy_(e.adam_v); st["stale1"].copy_(e.stale_sq)
        all_losses = self._fit_loop(perm_fns, self.fit_iter_split_all)
        # WideCPOEngine.check_sync_error is a no-op: both error words of every run, one host read
        words = [e.sync_ws[8] for e in es] + [st["sync_ws"][8] for st in sts]
        codes = [int(c) & 0xFFFFFFFF for c in torch.stack([w.to(torch.int64) for w in words]).cpu().tolist()]
        bad = [i for i in range(S) if codes[i] | codes[S + i]]
        if bad:
            for st in sts:
                st["sync_ws"][8] = 0
            self._restore(backups)
            i = bad[0]
            raise _abi.SpoError(f"replica {i} of {S}: split critic fit: exchange error {codes[i] | codes[S + i]} (the workgroups of "
                                "the seed-batched launch were not all resident); every run's critics, moments and stale norm are "
                                "restored to the start of this critic fit")
        return [self._loss_dict(ls) for ls in all_losses]

    # ------------------------------------------------------------------ the feature-split form (129-512 observations)
    def batched_ks(self) -> bool:
        """Does critic_fit_all run the feature-split critic fits of all runs as one launch per iteration
        (spo_critic_fit_iter_ks_multi)?  Only in a group built with ks_form=True, where every engine's own critic_fit would
        take the feature-split kernel too (_feature_split_critic_fit_ok: hidden [64, 64], one GPU, not SPO_WIDE_KS=0), all
        runs share the minibatch size and the library has the form for this shape and run count
        (spo_critic_fit_ks_multi_supported)."""
        if not (self.ks_form and self._native):
            return False
        es = self.engines
        if not all(self._takes_ks(e) for e in es):
            return False
        cfgs = [e._cfg_struct() for e in es]
        if any(c.batch != cfgs[0].batch for c in cfgs):
            return False
        if not all(e._feature_split_critic_fit_ok(c) for e, c in zip(es, cfgs)):
            return False
        return bool(self.lib.spo_critic_fit_ks_multi_supported(es[0].D, cfgs[0].batch, len(es)))

    def fit_iter_ks_all(self, perms, active=None):
        """One iteration of WideCPOEngine.critic_fit's feature-split loop for every run i with active[i] in ONE launch;
        adam_step advances per run.  Returns the losses [n_mb, 3] per run (columns 0, 1 are written; None for a run that sat
        out)."""
        return self._fit_iter("spo_critic_fit_iter_ks_multi", "fit_iter_ks_all", perms, active)

    def _critic_fit_all_ks(self, perm_fns):
        """critic_fit_all where batched_ks(): the feature-split loop of WideCPOEngine.critic_fit for every run, one launch per
        iteration; after the loop every run's error word (one host read for all) and the rescale of its stale actor-gradient
        vector to the norm the kernel carried.  An exchange error is not degraded to another form: every run's critics,
        moments, stale norm and adam_step are restored to the start of this critic fit (the stale vector has not been touched
        yet) and the error raised, naming the run."""
        es, S = self.engines, len(self.engines)
        backups = self._backup()
        all_losses = self._fit_loop(perm_fns, self.fit_iter_ks_all)
        codes = [int(c) & 0xFFFFFFFF for c in torch.stack([e.sync_ws[8].to(torch.int64) for e in es]).cpu().tolist()]
        bad = [i for i in range(S) if codes[i]]
        if bad:
            self._restore(backups)
            i = bad[0]
            raise _abi.SpoError(f"replica {i} of {S}: feature-split critic fit: exchange error {codes[i]} (the inter-workgroup "
                                "exchange of the seed-batched launch timed out); every run's critics, moments and stale norm are "
                                "restored to the start of this critic fit")
        outs = []
        for e, b, ls in zip(es, backups, all_losses):
            e.flat_grad[e.ls_off:].mul_(torch.sqrt(e.stale_sq / b[3].clamp_min(1e-38)))
            outs.append(self._loss_dict(ls))
        return outs

    def critic_fit_all(self, perm_fns=None):
        """CPOEngine.critic_fit for every run: learning_iters iterations each (a run with fewer sits out the later launches),
        every iteration's shuffle drawn per run -- under its ReplicaRNG by default -- before that iteration's launch, as the
        stand-alone loop draws it.  Where batched_split() (a split_form group at 65-128 observations): the same loop on the
        two-replica split form.  Where batched_ks() (a ks_form group at 129-512 observations): the same loop on the
        feature-split kernel.  Where none of them: each engine's own critic_fit, one after the other -- the same results.
        Returns the list of critic_fit()'s dicts."""
        perm_fns = self._default_perm_fns(perm_fns, "critic_fit_all: ")
        if self.batched_split():
            return self._critic_fit_all_split(perm_fns)
        if self.batched_ks():
            return self._critic_fit_all_ks(perm_fns)
        if not self.batched():
            return [e.critic_fit(perm_fns[i]) for i, e in enumerate(self.engines)]
        all_losses = self._fit_loop(perm_fns, self.fit_iter_all)
        self.check_sync_error()
        return [self._loss_dict(ls) for ls in all_losses]
