"""CPU: the online occupancy grid's host side -- configuration keys, the slot -> cell bijection's
stride, the rolling slot ranges, the C ABI's argument checks (no kernel launches, no GPU) and the
OnlineGrid state round trip on CPU tensors."""
import ctypes
import math
import os
import re

import pytest
import torch

from march_support import lib, restored_keys

os.environ.setdefault("NERF_AMD_NO_ARGV", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nerf_grid_update_points", "nerf_grid_update_apply", "nerf_grid_update_threshold")
LEGO = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))


@pytest.fixture()
def task_arg():
    """cfg.task_arg with the keys this file touches restored afterwards."""
    from src.config import cfg
    with restored_keys(cfg.task_arg, ("train_renderer", "train_grid", "grid_update")) as ta:
        yield ta


# --------------------------------------------------------------------------------------
# configuration
# --------------------------------------------------------------------------------------
def test_defaults_are_in_the_config(task_arg):
    from src.models.nerf.renderer.online_grid import DEFAULTS, grid_update_settings
    assert task_arg.train_grid == "file" and task_arg.train_renderer == "hierarchical"
    assert dict(task_arg.grid_update) == DEFAULTS == {"interval": 16, "warmup_updates": 16, "period": 4,
                                                      "decay": 0.95, "seed": 0}
    assert grid_update_settings(task_arg) == DEFAULTS
    task_arg.pop("grid_update")  # a configuration without the node: the same defaults
    assert grid_update_settings(task_arg) == DEFAULTS


def test_train_grid_key_is_validated(task_arg, tmp_path, monkeypatch):
    from src.train.trainers.nerf import NetworkWrapper
    monkeypatch.chdir(tmp_path)
    # the default (file) keeps today's error of the accelerated step without its grid file
    task_arg.train_renderer = "accelerated"
    with pytest.raises(FileNotFoundError, match="occupancy_grid.py"):
        NetworkWrapper(None)
    task_arg.train_grid = "live"
    with pytest.raises(ValueError, match="train_grid must be one of"):
        NetworkWrapper(None)
    task_arg.train_grid = "online"
    task_arg.train_renderer = "hierarchical"
    with pytest.raises(ValueError, match="train_renderer: accelerated"):
        NetworkWrapper(None)
    # online + accelerated needs no file and owns a grid of the configured resolution
    task_arg.train_renderer = "accelerated"
    w = NetworkWrapper(None)
    g = w.online_grid
    assert g is not None and g.res == int(task_arg.occupancy_grid_res) == 128
    assert g.threshold == float(task_arg.occupancy_grid_threshold)
    assert (g.interval, g.warmup_updates, g.period, g.decay, g.seed) == (16, 16, 4, 0.95, 0)
    assert g.updates == 0 and g.steps == 0 and g.grid.dtype == torch.uint8 and bool(g.grid.all())
    assert not (tmp_path / "logs").exists()
    # file mode owns none
    task_arg.train_grid = "file"
    task_arg.train_renderer = "hierarchical"
    assert NetworkWrapper(None).online_grid is None


@pytest.mark.parametrize("key,value,match", [
    ("interval", 0, "interval must be an integer >= 1"), ("interval", 2.5, "interval must be an integer"),
    ("warmup_updates", 0, "warmup_updates must be an integer >= 1"), ("period", -1, "period must be an integer >= 1"),
    ("decay", 0.0, r"decay must be in \(0, 1\]"), ("decay", 1.5, r"decay must be in \(0, 1\]"),
    ("decay", "fast", r"decay must be in \(0, 1\]"), ("seed", -3, "seed must be an integer >= 0"),
    ("every", 4, "unknown key")])
def test_grid_update_keys_are_validated(task_arg, key, value, match):
    from src.models.nerf.renderer.online_grid import grid_update_settings
    task_arg.grid_update = {key: value}
    with pytest.raises(ValueError, match=match):
        grid_update_settings(task_arg)


# --------------------------------------------------------------------------------------
# the bijection and the cadence
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [2, 8, 33, 100, 128])
def test_stride_is_coprime_and_golden(res):
    from nerf_amd import ops
    C = res ** 3
    a = ops.grid_update_stride(res)
    assert 0 < a < C and math.gcd(a, C) == 1
    assert abs(a - 0.618 * C) <= max(2.0, 0.01 * C)  # of the order of 0.618 res^3
    if res <= 33:  # a bijection, checked outright
        assert sorted((s * a) % C for s in range(C)) == list(range(C))


def test_rolling_ranges_partition_the_slots():
    """res 33 (C = 35,937 = 4 * 8,984 + 1), period 4: `period` consecutive post-warm-up updates."""
    from nerf_amd import ops
    res, period, warm = 33, 4, 3
    C = res ** 3
    assert C % period != 0
    for k in range(warm):
        assert ops.grid_update_slots(k, res, warm, period) == (0, C)
    for first in (warm, warm + 1, warm + 6):
        seen = []
        for k in range(first, first + period):
            s0, n = ops.grid_update_slots(k, res, warm, period)
            assert 0 <= s0 and n > 0 and s0 + n <= C
            seen.append((s0, n))
        seen.sort()
        assert seen[0][0] == 0 and sum(n for _, n in seen) == C
        for (a0, an), (b0, _) in zip(seen, seen[1:]):
            assert a0 + an == b0
    # more ranges than cells: the surplus ranges are empty, never negative
    assert [ops.grid_update_slots(k, 2, 0, 16)[1] for k in range(16)] == [1] * 8 + [0] * 8


def test_step_cadence_counts_its_own_steps():
    """step() updates at the grid's own steps 0, interval, 2 interval, ...: update 0 precedes the first march."""
    from src.models.nerf.renderer.online_grid import OnlineGrid
    g = OnlineGrid(8, 1.0, LEGO, interval=4, warmup_updates=2, period=4)
    calls = []
    g.update = lambda packer, dtype: (calls.append(g.steps), setattr(g, "updates", g.updates + 1))
    fired = [g.step(None, "fp32") for _ in range(9)]
    assert fired == [True, False, False, False, True, False, False, False, True]
    assert calls == [0, 4, 8] and g.updates == 3 and g.steps == 9


# --------------------------------------------------------------------------------------
# C ABI
# --------------------------------------------------------------------------------------
def test_header_and_signatures_have_the_new_entry_points(lib):
    from nerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_amd.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name
        assert hasattr(lib, name)
    assert re.search(r"\bint64_t\s+nerf_grid_update_workspace_bytes\s*\(", text)
    assert lib.nerf_abi_version() == 4


def test_argument_errors_and_noops_without_gpu(lib):
    from nerf_amd import ops
    from nerf_amd._lib import check
    bbox = ctypes.cast((ctypes.c_float * 6)(-1.5, -1.5, -1.5, 1.5, 1.5, 1.5), ctypes.c_void_p)
    d = ctypes.c_void_p(16)  # never dereferenced: the argument checks come first
    A = ops.grid_update_stride(128)
    C = 128 ** 3

    def points(res=128, bb=bbox, a=A, b=0, s0=0, n=64, cells=d, pts=d):
        return lib.nerf_grid_update_points(res, bb, a, b, 0, 0, s0, n, cells, pts, None)

    for bad, match in ((dict(res=1), "res must be"), (dict(res=2000), "res must be"), (dict(n=-1), "n must be"),
                       (dict(bb=None), "bbox"), (dict(s0=-1), "slots"), (dict(s0=C - 10), "slots"),
                       (dict(a=0), "coprime"), (dict(a=C), "coprime"), (dict(a=A + 1 if A % 2 else A), "coprime"),
                       (dict(b=C), "coprime"), (dict(cells=None), "null pointer"), (dict(pts=None), "null pointer")):
        assert points(**bad) == -22, bad
        with pytest.raises(RuntimeError, match=match):
            check(points(**bad), "nerf_grid_update_points")
    assert points(n=0, cells=None, pts=None) == 0  # n == 0: no launch
    assert points(s0=C, n=0, cells=None, pts=None) == 0

    def apply(cells=d, raw=d, n=64, res=128, density=d):
        return lib.nerf_grid_update_apply(cells, raw, n, res, 0.95, density, None)

    for bad, match in ((dict(res=1), "res must be"), (dict(n=-5), "n must be"), (dict(cells=None), "null pointer"),
                       (dict(raw=None), "null pointer"), (dict(density=None), "null pointer")):
        assert apply(**bad) == -22, bad
        with pytest.raises(RuntimeError, match=match):
            check(apply(**bad), "nerf_grid_update_apply")
    assert apply(cells=None, raw=None, n=0, density=None) == 0

    def threshold(density=d, res=128, ws=d, grid=d, stats=d):
        return lib.nerf_grid_update_threshold(density, res, 1.0, ws, grid, stats, None)

    for bad, match in ((dict(res=0), "res must be"), (dict(density=None), "null pointer"), (dict(ws=None), "null pointer"),
                       (dict(grid=None), "null pointer"), (dict(stats=None), "null pointer")):
        assert threshold(**bad) == -22, bad
        with pytest.raises(RuntimeError, match=match):
            check(threshold(**bad), "nerf_grid_update_threshold")
    assert lib.nerf_grid_update_workspace_bytes(1) == -1
    for res in (2, 33, 128, 1024):
        assert lib.nerf_grid_update_workspace_bytes(res) >= 8 * min(1024, -(-res ** 3 // 256))


def test_ops_reject_cpu_tensors():
    from nerf_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.grid_update_points(8, LEGO, 0, 8, 0, device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.grid_update_apply(torch.zeros(8, 8, 8), torch.zeros(4, dtype=torch.int32), torch.zeros(4, 4), 0.95)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.grid_update_threshold(torch.zeros(8, 8, 8), torch.zeros(8, 8, 8, dtype=torch.uint8), 1.0,
                                  torch.zeros(8192, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32))


# --------------------------------------------------------------------------------------
# state
# --------------------------------------------------------------------------------------
def test_state_round_trip_on_cpu(tmp_path):
    from src.models.nerf.renderer.online_grid import OnlineGrid
    kw = dict(interval=8, warmup_updates=3, period=5, decay=0.9, seed=11)
    bbox = [[-1.3, -0.4, 0.1], [0.7, 1.9, 2.3]]
    a = OnlineGrid(9, 0.5, bbox, **kw)
    g = torch.Generator().manual_seed(2)
    a.density = torch.rand(9, 9, 9, generator=g)
    a.grid = (a.density > 0.4).to(torch.uint8)
    a.updates, a.steps = 7, 50
    path = str(tmp_path / "occupancy_grid_state.pt")
    torch.save(a.state_dict(), path)
    b = OnlineGrid(9, 0.5, bbox, **kw)
    b.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))  # plain data: no unpickled code
    assert torch.equal(a.density, b.density) and torch.equal(a.grid, b.grid)
    assert b.density.dtype == torch.float32 and b.grid.dtype == torch.uint8
    assert (b.updates, b.steps) == (7, 50) and b.slots() == a.slots()
    b.density[0, 0, 0] = 5.0  # a copy, not the file's storage shared with a
    assert float(a.density[0, 0, 0]) != 5.0
    assert a.occupancy_bool().dtype == torch.bool and torch.equal(a.occupancy_bool(), a.density > 0.4)
    # a state written under other settings is refused, naming the setting
    for other, match in ((dict(kw, period=4), "period"), (dict(kw, seed=0), "seed")):
        with pytest.raises(ValueError, match=match):
            OnlineGrid(9, 0.5, bbox, **other).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="res"):
        OnlineGrid(8, 0.5, bbox, **kw).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="bbox"):
        OnlineGrid(9, 0.5, LEGO, **kw).load_state_dict(a.state_dict())
