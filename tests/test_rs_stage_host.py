"""CPU tests (no GPU) of the staged minibatch inputs of the row-split update kernel (csrc/update_rs.hip): the entry points are
declared, exported and bound, and spo_rs_stage_bytes follows the record formula of include/safepo_hip.h -- and is 0 where the
staged form does not apply."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("spo_rs_stage_bytes", "spo_debug_rs_last_staged", "spo_debug_rs_stage")
SHAPES = [(60, 8), (64, 16), (17, 3), (1, 1)]                                  # (obs_dim, act_dim)
BATCHES = [(64, 64 * 3 + 5), (64, 37), (40, 40 * 2 + 9), (32, 32 * 2)]         # (batch, M)


def record_bytes(D):
    """x[64][KIN] + xT[KIN][64] + act[64][16] + logp_old, adv, tgt_r, tgt_c [64], floats; KIN = 16 / 32 / 64."""
    kin = 16 if D <= 16 else 32 if D <= 32 else 64
    return 4 * (2 * 64 * kin + 64 * 16 + 4 * 64)


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from safepo import _abi
    return _abi.load(g.LIB)


@pytest.fixture(autouse=True)
def _default_rows(monkeypatch):
    assert os.environ.get("SPO_RS_ROWS", "32") != "16", "SPO_RS_ROWS=16 selects the four-row-group form in this process: unset it"


def test_symbols_declared_exported_and_bound(lib):
    from safepo import _abi
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "safepo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(spo_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _abi.PROTOTYPES, name
        assert hasattr(lib, name), name


def test_record_is_a_multiple_of_256_bytes_and_the_benchmark_size():
    assert record_bytes(60) == 37888
    assert all(record_bytes(D) % 256 == 0 for D in range(1, 65))


@pytest.mark.parametrize("D,A", SHAPES)
@pytest.mark.parametrize("batch,M", BATCHES)
def test_stage_bytes_equals_the_record_formula(lib, D, A, batch, M):
    nsteps = (M + batch - 1) // batch
    assert lib.spo_rs_stage_bytes(D, A, batch, M) == nsteps * record_bytes(D)


def test_stage_bytes_at_the_benchmark_size(lib):
    assert lib.spo_rs_stage_bytes(60, 8, 64, 4096 * 128) == 8192 * 37888          # 310 MB per launch


def test_stage_bytes_is_zero_where_the_form_does_not_apply(lib):
    f = lib.spo_rs_stage_bytes
    assert f(65, 8, 64, 640) == 0 and f(128, 8, 64, 640) == 0                      # KIN = 128: in-kernel gather
    assert f(60, 8, 65, 650) == 0 and f(60, 8, 128, 1280) == 0                     # four row groups: the critic fit's minibatches
    assert f(60, 4, 128, 128 * 9 + 13) == 0                                        # ... with its usual arguments
    assert f(0, 8, 64, 640) == 0 and f(60, 0, 64, 640) == 0 and f(60, 17, 64, 640) == 0
    assert f(60, 8, 0, 640) == 0 and f(60, 8, 64, 0) == 0
    assert f(64, 16, 64, 1) == record_bytes(64) and f(1, 1, 1, 3) == 3 * record_bytes(1)
