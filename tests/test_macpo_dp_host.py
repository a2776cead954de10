"""Host side of data-parallel MACPO (no GPU): the global advantage statistics, the bindings of the two new kernels' entry
points, and the config key that forces the sharded form."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _TwoShardComm:
    """all_reduce_sum_ of a job whose other ranks' contributions are known: adds the tensors of `others` to the caller's."""
    world_size, rank = 2, 0

    def __init__(self, others):
        self.others, self.calls = list(others), 0

    def all_reduce_sum_(self, t):
        self.calls += 1
        for o in self.others:
            t.add_(o)
        return t


@pytest.mark.parametrize("shape,split", [((7, 8, 1), 3), ((6, 8, 1), 4), ((2, 2, 1), 1)])
def test_global_mean_std_is_torch_mean_std_of_the_concatenation(shape, split):
    from safepo.multi_agent.macpo import adv_sums, global_mean_std
    g = torch.Generator().manual_seed(11)
    full = 3.0 + 2.0 * torch.randn(*shape, generator=g)
    a, b = full[:, :split].contiguous(), full[:, split:].contiguous()
    comm = _TwoShardComm([adv_sums(b)])
    mean, std = global_mean_std(a, comm)
    assert comm.calls == 1 and mean.dtype == std.dtype == torch.float32
    # float32 results of float64 sums against torch's own float32 reductions, whose error is relative to the size of the data
    atol = 1e-6 * float(full.abs().mean())
    torch.testing.assert_close(mean, torch.mean(full), rtol=1e-6, atol=atol)
    torch.testing.assert_close(std, torch.std(full), rtol=1e-6, atol=atol)
    m64, s64 = full.double().mean(), full.double().std()
    assert abs(float(mean) - float(m64)) <= 2 ** -23 * abs(float(m64)) and abs(float(std) - float(s64)) <= 2 ** -23 * float(s64)
    # the other rank arrives at the same numbers
    mean_b, std_b = global_mean_std(b, _TwoShardComm([adv_sums(a)]))
    assert torch.equal(mean, mean_b) and torch.equal(std, std_b)


def test_global_mean_std_single_rank_is_plain_statistics():
    from safepo.multi_agent.macpo import global_mean_std
    from safepo.parallel import Comm
    x = torch.randn(5, 4, 1, generator=torch.Generator().manual_seed(2))
    mean, std = global_mean_std(x, Comm.single())
    atol = 1e-6 * float(x.abs().mean())
    torch.testing.assert_close(mean, x.mean(), rtol=1e-6, atol=atol)
    torch.testing.assert_close(std, x.std(), rtol=1e-6, atol=atol)


def test_macpo_dp_entry_points_declared_and_bound():
    from safepo import _abi
    header = open(os.path.join(ROOT, "include", "safepo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    P = ctypes.c_void_p
    want = {"spo_ma_trpo_linesearch_sums": 17, "spo_ma_cg_init": 8, "spo_ma_cg_update": 9}
    for name, nargs in want.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert decl, f"{name} is not declared in include/safepo_hip.h"
        assert len(decl.group(1).split(",")) == nargs, name
        res, args = _abi.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == nargs, name
        assert args[-1] is P, f"{name}: the stream comes last"
    ls = _abi.PROTOTYPES["spo_ma_trpo_linesearch_sums"][1]
    assert ls[2] is ctypes.c_float and ls[3] is ctypes.c_float and ls[11] is ctypes.c_int64 and ls[12] is ctypes.c_int
    assert _abi.PROTOTYPES["spo_ma_cg_init"][1][6] is ctypes.c_int64
    up = _abi.PROTOTYPES["spo_ma_cg_update"][1]
    assert up[6] is ctypes.c_int64 and up[7] is ctypes.c_float
    for macro, value in (("SPO_MA_LS_WS_DOUBLES", _abi.MA_LS_WS_DOUBLES), ("SPO_MA_CG_WS_DOUBLES", _abi.MA_CG_WS_DOUBLES)):
        assert int(re.search(r"#define " + macro + r" (\d+)", header).group(1)) == value
    # each entry names the reference lines it replaces
    assert "macpo.py:329-366" in header and "macpo.py:168-185" in header


def test_macpo_sharded_form_defaults_to_off():
    from safepo.multi_agent import macpo
    from safepo.utils.config import multi_agent_args
    assert macpo.default_cfg["macpo_sharded_form"] is False
    _, _, cfg = multi_agent_args("macpo", ["--num-envs", "8"])
    assert cfg["macpo_sharded_form"] is False
    assert "macpo_sharded_form" not in __import__("safepo.multi_agent.mappolag", fromlist=["default_cfg"]).default_cfg
