"""GPU tests of the single-run update launches' scratch blocks: one block per (device, stream) in a StreamTable
(csrc/stream_table.h), made at the stream's first launch, refused under capture, freed by spo_update_scratch_release.  Four forms
keep such a block:
  hs     spo_update_iter_ex, clipped loss    update.hip, the main + helper kernel's backup rows and norm granules
  rs     spo_ppo_lag_update_iter             update_rs.hip, the row-split kernel's exchange slots (and its staging block)
  ks     spo_ppo_lag_update_iter_ks          update_ks.hip, the feature-split kernel's exchange slots, two slices
  split  spo_critic_fit_iter_split           update.hip, the cached exchange regions of the one-grid split critic fit
Every launch here is the same launch from the same start state, so every comparison is bit for bit.  The shapes are the
smallest that reach each table: two minibatch steps of 8 rows at obs_dim 4 (hs, rs) and 70 (ks), and the smallest case of
tests/seed_batch_critic_split_cases.py (split).  No test provokes a timeout of an exchange; the capture is never replayed."""
import faulthandler
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_rs_stage as RS  # noqa: E402
import test_gpu_seed_batch_critic_split as SP  # noqa: E402
import seed_batch_critic_split_cases as C  # noqa: E402
import ks_batch_problem as KS  # noqa: E402

TIME_LIMIT_S = 120
BATCH, M = 8, 16                      # two minibatch steps
MAX_GRAD_NORM, SCALE = 1.0, 0.7
FORMS = ("hs", "rs", "ks", "split")
REFUSED_BY = {"hs": "update kernel", "rs": "row-split update kernel", "ks": "feature-split update kernel", "split": "split critic fit"}


@pytest.fixture(autouse=True)
def _time_limit_and_routing(monkeypatch):
    for k in ("SPO_RS_OBS128", "SPO_RS_SAFE", "SPO_KS_SAFE", "SPO_RS_L1_PIPE", "SPO_FORCE_DP", "SPO_RS_STAGE", "SPO_RS_STAGE_MAX_MB",
              "SPO_CPO_SPLIT", "SPO_CPO_SPLIT_FORM"):
        monkeypatch.delenv(k, raising=False)
    assert int(os.environ.get("SPO_UPDATE_FORM", "3")) >= 3, "SPO_UPDATE_FORM selects an older form in this process: unset it"
    assert os.environ.get("SPO_WIDE_KS", "1") != "0" and os.environ.get("SPO_CPO_SPLIT_L2", "1") != "0"
    faulthandler.dump_traceback_later(TIME_LIMIT_S, exit=True, file=sys.__stderr__)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


class _Form:
    """One engine of a form with its start state: launch() is the form's entry on the current stream, from wherever the state
    is; result() is everything the launch wrote."""

    def __init__(self, name, dev):
        from safepo import _abi
        self.name, self.lib = name, _abi.load()
        rng = torch.get_rng_state()
        if name in ("hs", "rs"):
            assert self.lib.spo_update_rs_supported(4, 2, BATCH, 3) == 1
            self.eng = RS._engine(4, 2, BATCH, M, MAX_GRAD_NORM, SCALE, dev)
        elif name == "ks":
            # 70 observations: two slices.  The engines route this shape to the row-split kernel, so the entry is called directly
            # (launch below) on a plain engine's parameters and buffer.
            assert KS.slices((70, 2, BATCH)) == 2 and self.lib.spo_ks_supported(70, 2, BATCH) == 1
            self.eng = RS._engine(70, 2, BATCH, M, MAX_GRAD_NORM, SCALE, dev)
        else:
            self.eng, perms = SP._engine(C.SHAPES[1], 0, dev)           # (65, 1): the smallest of the split fit's shapes
            self.perm = perms[0]
            SP._start(self.eng)
        if name != "split":
            self.perm = torch.randperm(M, generator=torch.Generator().manual_seed(9)).to(torch.int32).to(dev)
        torch.set_rng_state(rng)
        torch.cuda.synchronize()
        self.start = self.state()
        self.clocks = (self.eng.adam_step, getattr(self.eng, "adam_step_actor_extra", 0))

    def state(self):
        e = self.eng
        return SP._state(e) if self.name == "split" else (e.policy.theta.clone(), e.adam_m.clone(), e.adam_v.clone())

    def restore(self):
        e = self.eng
        live = ((e.policy.theta, e.adam_m, e.adam_v, e.stale_sq) + tuple(e._split_setup()[k] for k in ("theta1", "m1", "v1", "stale1"))
                if self.name == "split" else (e.policy.theta, e.adam_m, e.adam_v))
        for t, s in zip(live, self.start):
            t.copy_(s)
        e.adam_step = self.clocks[0]                       # (the split form's exchange tag st["step"] carries on: tags never repeat)
        if hasattr(e, "adam_step_actor_extra"):
            e.adam_step_actor_extra = self.clocks[1]
        torch.cuda.synchronize()

    def launch(self):
        e = self.eng
        if self.name == "hs":
            return (e.learning_iter_ex(self.perm, e.buffer.adv_mix.view(-1), 0),)
        if self.name == "split":
            return SP._single_iter(self.lib, e, self.perm)
        if self.name == "ks":
            from safepo import _abi
            d, cfg = e.buffer.data, e._cfg_struct()
            losses = torch.empty(((M + BATCH - 1) // BATCH, 3), dtype=torch.float32, device=e.dev)
            _abi.check(self.lib.spo_ppo_lag_update_iter_ks(
                _abi.ptr(e.policy.theta), _abi.ptr(e.adam_m), _abi.ptr(e.adam_v), e.adam_step, _abi.ptr(d["obs"]), _abi.ptr(d["act"]),
                _abi.ptr(d["log_prob"]), _abi.ptr(d["target_value_r"]), _abi.ptr(d["target_value_c"]), _abi.ptr(e.buffer.adv_mix),
                _abi.ptr(self.perm), M, cfg, _abi.ptr(losses), _abi.ptr(e.sync_ws), _abi.stream_ptr()), "spo_ppo_lag_update_iter_ks")
            return (losses,)
        return (e.learning_iter(self.perm),)

    def run_on(self, stream):
        """restore, launch on `stream`, wait -> state + losses; no error word may be set."""
        self.restore()
        with torch.cuda.stream(stream):
            losses = self.launch()
        torch.cuda.synchronize()
        self.assert_no_error_word()
        out = self.state() + tuple(x.clone() for x in losses)
        assert all(torch.isfinite(t).all() for t in out), self.name
        return out

    def assert_no_error_word(self):
        words = [self.eng.sync_ws] + ([self.eng._split_setup()["sync_ws"]] if self.name == "split" else [])
        assert all(int(w[8].item()) & 0xFFFFFFFF == 0 for w in words), f"{self.name}: error word set"


_FORMS = {}


def _form(name, dev):
    if name not in _FORMS:
        _FORMS[name] = _Form(name, dev)
    return _FORMS[name]


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for i, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), f"{what}: tensor {i} differs in {int((x != y).sum())} of {x.numel()} entries"


def _release(lib, stream):
    torch.cuda.synchronize()
    return int(lib.spo_update_scratch_release(stream.cuda_stream, 0))


@pytest.mark.parametrize("name", FORMS)
def test_block_is_released_and_made_again(dev, name):
    f = _form(name, dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    assert s1.cuda_stream != s2.cuda_stream
    kept2 = f.run_on(s2)                                   # the second stream's block
    kept1 = f.run_on(s1)
    assert not torch.equal(kept1[0], f.start[0])           # (the launch did something)
    _assert_same(kept1, kept2, f"{name}: the same launch on two streams")
    assert _release(f.lib, s1) >= 1
    assert _release(f.lib, s1) == 0
    _assert_same(f.run_on(s1), kept1, f"{name}: after release, on a new block")
    _assert_same(f.run_on(s2), kept2, f"{name}: the other stream's block after the release")
    assert _release(f.lib, s2) >= 1                        # it was still there
    assert _release(f.lib, s2) == 0
    assert _release(f.lib, s1) >= 1 and _release(f.lib, s1) == 0


def test_first_launch_under_capture_is_refused(dev):
    from safepo import _abi
    forms = [_form(name, dev) for name in FORMS]
    for f in forms:
        f.restore()
    s = torch.cuda.Stream(dev)                             # has not launched before: no form holds a block for it
    x = torch.zeros(8, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    msgs = {}
    with torch.cuda.graph(graph, stream=s):                # (captured, never replayed)
        x.add_(1.0)
        for f in forms:
            try:
                f.launch()
                msgs[f.name] = "not refused"
            except _abi.SpoError as e:
                msgs[f.name] = str(e)
    torch.cuda.synchronize()
    # every form meets the refusal of its OWN table (the split fit runs on its default four-wave kernel here -- SPO_CPO_SPLIT_FORM
    # is unset -- so it holds no main + helper block and split_local_for's refusal is the one it reaches)
    for f in forms:
        assert f"(rc=-1): {REFUSED_BY[f.name]}: first launch on a stream under capture" in msgs[f.name], (f.name, msgs[f.name])
        _assert_same(f.state(), f.start, f"{f.name}: refused under capture")
        f.assert_no_error_word()
    assert float(x.sum().item()) == 0.0
    for f in forms:                                        # the next ordinary launch on that stream
        out = f.run_on(s)
        assert not torch.equal(out[0], f.start[0])
    assert _release(forms[0].lib, s) >= len(FORMS)
    assert _release(forms[0].lib, s) == 0
