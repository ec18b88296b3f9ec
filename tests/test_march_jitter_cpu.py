"""CPU: jittered march steps (task_arg.train_march_jitter) -- the six new entry points in the header
and the ctypes table, the argument checks of nerf_march_jitter (no launch, no GPU), the tensor checks
of ops' t_shift argument, and the configuration key's default and validation."""
import ctypes
import os
import re

import pytest

from march_support import _declared, built_lib as lib, restored_keys

os.environ.setdefault("NERF_AMD_NO_ARGV", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# new entry point -> the entry point whose signature it extends by `const float* t_shift` (before the stream)
SHIFTED = {
    "nerf_march_gather_shift": "nerf_march_gather",
    "nerf_march_composite_shift": "nerf_march_composite_used",
    "nerf_march_segments_shift": "nerf_march_segments",
    "nerf_march_seg_composite_fwd_shift": "nerf_march_seg_composite_fwd",
    "nerf_march_seg_composite_bwd_shift": "nerf_march_seg_composite_bwd",
}


def test_header_and_signature_table_have_the_six_symbols(lib):
    from nerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_amd.h")).read(), flags=re.S)
    params = _declared(text, "nerf_march_jitter")
    assert params == ["int64_t N", "float step_size", "uint64_t seed", "uint64_t offset", "float* t_shift",
                      "hipStream_t stream"]
    res, args = _lib.SIGNATURES["nerf_march_jitter"]
    assert res is ctypes.c_int and len(args) == len(params)
    assert args[:4] == [ctypes.c_int64, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64]
    assert hasattr(lib, "nerf_march_jitter")
    for new, old in SHIFTED.items():
        p_new, p_old = _declared(text, new), _declared(text, old)
        assert p_new == p_old[:-1] + ["const float* t_shift", "hipStream_t stream"], new
        res, args = _lib.SIGNATURES[new]
        res_old, args_old = _lib.SIGNATURES[old]
        assert res is res_old is ctypes.c_int and len(args) == len(p_new), new
        assert args == args_old[:-1] + [ctypes.c_void_p, ctypes.c_void_p], new
        assert hasattr(lib, new), new
    assert lib.nerf_abi_version() == 4  # additions do not bump it


def test_jitter_argument_errors_without_gpu(lib):
    from nerf_amd._lib import check
    d = ctypes.c_void_p(16)  # never dereferenced: the argument checks come first
    assert lib.nerf_march_jitter(0, 0.005, 1, 2, None, None) == 0  # N == 0: a no-op, null allowed
    assert lib.nerf_march_jitter(0, 0.005, 1, 2, d, None) == 0
    for n, ptr, match in ((64, None, "t_shift is null"), (-1, d, "N must be"), (-1, None, "N must be")):
        assert lib.nerf_march_jitter(n, 0.005, 1, 2, ptr, None) == -22, (n, ptr)
        with pytest.raises(RuntimeError, match=match):
            check(lib.nerf_march_jitter(n, 0.005, 1, 2, ptr, None), "nerf_march_jitter")


def test_t_shift_is_checked_before_the_device():
    import torch
    from nerf_amd import ops
    rays = torch.zeros(4, 6)
    grid = torch.ones(8, 8, 8, dtype=torch.bool)
    with pytest.raises(ValueError, match="n must be"):
        ops.march_jitter(-1, 0.005, 0, 0, "cpu")
    for bad, exc in ((torch.zeros(4, dtype=torch.float64), TypeError), (torch.zeros(4, dtype=torch.int32), TypeError),
                     ([0.0] * 4, TypeError), (torch.zeros(5), ValueError), (torch.zeros(4, 1), ValueError),
                     (torch.zeros(8)[::2], ValueError)):
        with pytest.raises(exc, match="t_shift"):
            ops.march(None, rays, 2.0, 6.0, grid, t_shift=bad)
        with pytest.raises(exc, match="t_shift"):
            ops.march_grad(None, rays, 2.0, 6.0, grid, t_shift=bad)
        with pytest.raises(exc, match="t_shift"):
            ops.march_segments(rays, torch.arange(2.0, 6.0, 0.005), grid.to(torch.uint8), None,
                               torch.zeros(5, dtype=torch.int32), 0, t_shift=bad)


@pytest.fixture()
def task_arg():
    from src.config import cfg
    with restored_keys(cfg.task_arg, ("train_renderer", "train_grid", "train_march_jitter")) as ta:
        yield ta


def test_config_key_default_and_validation(task_arg, tmp_path, monkeypatch):
    from src.models.nerf.renderer.volume_renderer import march_jitter_setting
    from src.train.trainers.nerf import NetworkWrapper
    monkeypatch.chdir(tmp_path)
    assert task_arg.train_march_jitter is False  # in the shipped configuration, off
    assert march_jitter_setting(task_arg) is False
    assert NetworkWrapper(None).march_jitter is False
    node = task_arg.pop("train_march_jitter")  # a configuration without the key: off as well
    try:
        assert march_jitter_setting(task_arg) is False and NetworkWrapper(None).march_jitter is False
    finally:
        task_arg.train_march_jitter = node
    assert task_arg.get("train_renderer", "hierarchical") == "hierarchical"
    task_arg.train_march_jitter = True
    with pytest.raises(ValueError, match="train_march_jitter"):
        NetworkWrapper(None)  # the hierarchical step has no march to jitter
    for bad in ("true", "yes", 1, 0.5):
        task_arg.train_march_jitter = bad
        with pytest.raises(ValueError, match="train_march_jitter"):
            march_jitter_setting(task_arg)
        task_arg.train_renderer = "accelerated"
        with pytest.raises(ValueError, match="train_march_jitter"):
            NetworkWrapper(None)
        task_arg.train_renderer = "hierarchical"
    # accelerated + true is accepted: the key is read before the grid file is looked for
    task_arg.train_march_jitter = True
    task_arg.train_renderer = "accelerated"
    with pytest.raises(FileNotFoundError, match="occupancy_grid.py"):
        NetworkWrapper(None)
