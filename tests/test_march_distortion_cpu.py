"""CPU: the distortion loss of the training march (task_arg.distortion_loss_weight) -- the two new entry
points in the header and the ctypes table, their argument checks (no launch, no GPU), and the
configuration key's default and validation."""
import ctypes
import os
import re

import pytest

from march_support import _declared, built_lib as lib, restored_keys

os.environ.setdefault("NERF_AMD_NO_ARGV", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "distortion_loss_weight"


def test_header_and_signature_table_have_the_two_symbols(lib):
    from nerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_amd.h")).read(), flags=re.S)
    fwd_shift = _declared(text, "nerf_march_seg_composite_fwd_shift")
    bwd_shift = _declared(text, "nerf_march_seg_composite_bwd_shift")
    fwd, bwd = _declared(text, "nerf_march_seg_composite_fwd_dist"), _declared(text, "nerf_march_seg_composite_bwd_dist")
    # the _shift arguments, then the new ones, the stream last
    assert fwd == fwd_shift[:-1] + ["float inv_range", "float* dist", "double* totals", "hipStream_t stream"]
    assert bwd == (bwd_shift[:11] + ["const float* t_shift", "float inv_range", "const float* g_dist",
                                     "const double* totals", "float* g_raw", "hipStream_t stream"])
    assert bwd_shift[11:] == ["float* g_raw", "const float* t_shift", "hipStream_t stream"]
    for name, params in (("nerf_march_seg_composite_fwd_dist", fwd), ("nerf_march_seg_composite_bwd_dist", bwd)):
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        assert args[params.index("float inv_range")] is ctypes.c_float, name
        assert hasattr(lib, name), name
    # the entry points every existing caller uses keep their signatures
    assert len(_lib.SIGNATURES["nerf_march_seg_composite_fwd_shift"][1]) == len(fwd_shift) == 13
    assert len(_lib.SIGNATURES["nerf_march_seg_composite_bwd_shift"][1]) == len(bwd_shift) == 14
    assert lib.nerf_abi_version() == 4  # additions do not bump it


def _fwd(lib, N, seg_off, inv_range, dist, totals):
    d = ctypes.c_void_p(16)  # never dereferenced: the argument checks come first
    return lib.nerf_march_seg_composite_fwd_dist(d, d, N, d, seg_off, d, 0.005, 1, d, d, d, None, inv_range, dist,
                                                 totals, None)


def _bwd(lib, N, seg_off, inv_range, totals):
    d = ctypes.c_void_p(16)
    return lib.nerf_march_seg_composite_bwd_dist(d, d, N, d, seg_off, d, 0.005, 1, d, d, d, None, inv_range, d, totals,
                                                 d, None)


def test_argument_errors_without_gpu(lib):
    from nerf_amd._lib import check
    d = ctypes.c_void_p(16)
    assert _fwd(lib, 0, d, 0.25, d, d) == 0  # N == 0: a no-op
    assert _fwd(lib, 0, d, 0.25, None, None) == 0
    assert _bwd(lib, 0, d, 0.25, d) == 0
    assert _bwd(lib, 0, d, 0.25, None) == 0
    cases = ((None, 0.25, d, d, "seg_off is null"), (d, 0.25, None, d, "dist is null"),
             (d, 0.25, d, None, "totals is null"), (d, 0.0, d, d, "inv_range"), (d, -0.25, d, d, "inv_range"),
             (d, float("nan"), d, d, "inv_range"), (d, float("inf"), d, d, "inv_range"))
    for seg_off, inv_range, dist, totals, match in cases:
        assert _fwd(lib, 4, seg_off, inv_range, dist, totals) == -22, match
        with pytest.raises(RuntimeError, match=match):
            check(_fwd(lib, 4, seg_off, inv_range, dist, totals), "nerf_march_seg_composite_fwd_dist")
        if dist is None:
            continue  # (the backward has no dist argument; its cotangent may be null)
        assert _bwd(lib, 4, seg_off, inv_range, totals) == -22, match
        with pytest.raises(RuntimeError, match=match):
            check(_bwd(lib, 4, seg_off, inv_range, totals), "nerf_march_seg_composite_bwd_dist")
    assert _fwd(lib, -1, d, 0.25, d, d) == -22 and _bwd(lib, -1, d, 0.25, d) == -22
    with pytest.raises(RuntimeError, match="N must be"):
        check(_fwd(lib, -1, d, 0.25, d, d), "nerf_march_seg_composite_fwd_dist")


def test_march_grad_checks_the_range_before_the_device():
    import torch
    from nerf_amd import ops
    rays = torch.zeros(4, 6)
    grid = torch.ones(8, 8, 8, dtype=torch.bool)
    with pytest.raises(ValueError, match="far > near"):
        ops.march_grad(None, rays, 6.0, 6.0, grid, distortion=True)


@pytest.fixture()
def task_arg():
    from src.config import cfg
    with restored_keys(cfg.task_arg, ("train_renderer", "train_grid", "distortion_loss_weight")) as ta:
        yield ta


def test_config_key_default_and_validation(task_arg, tmp_path, monkeypatch):
    from src.models.nerf.renderer.volume_renderer import distortion_loss_setting
    from src.train.trainers.nerf import NetworkWrapper
    monkeypatch.chdir(tmp_path)
    assert task_arg[KEY] == 0.0 and isinstance(task_arg[KEY], float)  # in the shipped configuration, off
    assert distortion_loss_setting(task_arg) == 0.0
    assert task_arg.get("train_renderer", "hierarchical") == "hierarchical"
    assert NetworkWrapper(None).distortion_weight == 0.0  # 0.0 with the hierarchical renderer constructs
    node = task_arg.pop(KEY)  # a configuration without the key: off as well
    try:
        assert distortion_loss_setting(task_arg) == 0.0 and NetworkWrapper(None).distortion_weight == 0.0
    finally:
        task_arg[KEY] = node
    task_arg[KEY] = 0.01
    assert distortion_loss_setting(task_arg) == 0.01
    with pytest.raises(ValueError, match=KEY):
        NetworkWrapper(None)  # the hierarchical step has no march weights to regularise
    for bad in (-1, -1e-3, "x", "0.01", True, False, float("nan"), float("inf")):
        task_arg[KEY] = bad
        with pytest.raises(ValueError, match=KEY):
            distortion_loss_setting(task_arg)
        for renderer in ("accelerated", "hierarchical"):
            task_arg.train_renderer = renderer
            with pytest.raises(ValueError, match=KEY):
                NetworkWrapper(None)
        task_arg.train_renderer = "hierarchical"
    # accelerated + a positive weight is accepted: the key is read before the grid file is looked for
    task_arg[KEY] = 0.01
    task_arg.train_renderer = "accelerated"
    with pytest.raises(FileNotFoundError, match="occupancy_grid.py"):
        NetworkWrapper(None)
