"""CPU: the march-gradient fixture (tests/golden/golden_march_grad.npz), the oracle against it,
and the C ABI of the differentiable march (declarations, ctypes signatures, argument errors: no
kernel launches, no GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from march_support import g2, lib, mg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ("nerf_march_composite_used", "nerf_march_segments", "nerf_march_seg_composite_fwd",
       "nerf_march_seg_composite_bwd")
TAGS = ("mg_rgb", "mg_all")


def test_fixture_keys_and_shapes(mg):
    from nerf_amd import ops
    assert str(mg["source"]) in ("reference", "oracle")
    assert mg["gt"].shape == (256, 3) and mg["gt"].dtype == np.float32
    np.testing.assert_array_equal(mg["gt"], torch.rand(256, 3, generator=torch.Generator().manual_seed(1)).numpy())
    for tag in TAGS:
        assert mg[f"{tag}_loss"].shape == () and float(mg[f"{tag}_loss"]) > 0
        assert int(mg[f"{tag}_queried"]) == 13382
        assert [str(n) for n in mg[f"{tag}_names"]] == [f"model_fine.{n}" for n in ops.NET_PARAM_NAMES]
        assert mg[f"{tag}_norms"].shape == (24,) and mg[f"{tag}_absmax"].shape == (24,)
        assert mg[f"{tag}_sel_idx"].shape == (24, 64) and mg[f"{tag}_sel_val"].shape == (24, 64)
        assert (mg[f"{tag}_norms"] > 0).all() and (mg[f"{tag}_absmax"] > 0).all()
        assert int(mg[f"{tag}_coarse_tensors_with_grad"]) == 0
        assert mg[f"{tag}_rgb_map_f"].shape == (256, 3) and mg[f"{tag}_depth_map_f"].shape == (256,)
    assert float(mg["mg_all_loss"]) > float(mg["mg_rgb_loss"])


def test_oracle_reproduces_mg_rgb(mg, g2):
    """The oracle's render_accelerated differentiates as it stands: its loss and the 24 fine-net
    gradient norms against the fixture (the forward maps against golden_v2's march too)."""
    from oracle import nerf_oracle as O
    z = np.load(os.path.join(HERE, "golden", "trained_v2.npz"), allow_pickle=False)
    params = {k: torch.from_numpy(z[k]).clone().requires_grad_(True) for k in z.files}
    grid = torch.from_numpy(np.unpackbits(g2["bake128_packed"])[: 128 ** 3].reshape(128, 128, 128).astype(bool))
    r = O.render_accelerated(O.split_params(params, "model_fine"), torch.from_numpy(g2["march_rays"]), 2.0, 6.0, grid,
                             torch.from_numpy(g2["march_t_table"]))
    assert r["n_queried"] == int(mg["mg_rgb_queried"]) == int(g2["march_queried"])
    loss = torch.nn.functional.mse_loss(r["rgb_map_f"], torch.from_numpy(mg["gt"]))
    loss.backward()
    np.testing.assert_allclose(float(loss.detach()), float(mg["mg_rgb_loss"]), rtol=1e-6)
    for i, name in enumerate(mg["mg_rgb_names"]):
        g = params[str(name)].grad
        np.testing.assert_allclose(float(torch.linalg.vector_norm(g.double())), mg["mg_rgb_norms"][i], rtol=1e-5,
                                   err_msg=str(name))
    for k, p in params.items():
        if k.startswith("model."):
            assert p.grad is None, k


def test_header_and_signatures_have_the_new_entry_points():
    from nerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_amd.h")).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared"
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name


def test_new_symbols_are_exported_and_the_abi_version_stays(lib):
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.nerf_abi_version() == 4


def test_argument_errors_without_gpu(lib):
    from nerf_amd._lib import check
    bbox = ctypes.cast((ctypes.c_float * 6)(-1.5, -1.5, -1.5, 1.5, 1.5, 1.5), ctypes.c_void_p)
    dummy = ctypes.c_void_p(16)  # never dereferenced: the argument checks come first
    assert lib.nerf_march_segments(dummy, 4, dummy, 800, dummy, 128, None, bbox, None, dummy, dummy, dummy, None) == -22
    with pytest.raises(RuntimeError, match="seg_off"):
        check(lib.nerf_march_segments(dummy, 4, dummy, 800, dummy, 128, None, bbox, None, dummy, dummy, dummy, None),
              "nerf_march_segments")
    assert lib.nerf_march_segments(dummy, 4, dummy, 70000, dummy, 128, None, bbox, dummy, dummy, dummy, dummy,
                                   None) == -22
    with pytest.raises(RuntimeError, match="65536"):
        check(lib.nerf_march_segments(dummy, 4, dummy, 70000, dummy, 128, None, bbox, dummy, dummy, dummy, dummy, None),
              "nerf_march_segments")
    with pytest.raises(RuntimeError, match="bad arguments"):
        check(lib.nerf_march_segments(dummy, -1, dummy, 800, dummy, 128, None, bbox, dummy, dummy, dummy, dummy, None),
              "nerf_march_segments")
    with pytest.raises(RuntimeError, match="bad arguments"):
        check(lib.nerf_march_segments(dummy, 4, dummy, 800, dummy, 128, None, None, dummy, dummy, dummy, dummy, None),
              "nerf_march_segments")
    for fn, n_tail in ((lib.nerf_march_seg_composite_fwd, 3), (lib.nerf_march_seg_composite_bwd, 4)):
        tail = [dummy] * n_tail + [None]
        assert fn(dummy, dummy, 4, dummy, None, dummy, 0.005, 1, *tail) == -22
        with pytest.raises(RuntimeError, match="seg_off"):
            check(fn(dummy, dummy, 4, dummy, None, dummy, 0.005, 1, *tail), "seg composite")
        with pytest.raises(RuntimeError, match="N must be"):
            check(fn(dummy, dummy, -1, dummy, dummy, dummy, 0.005, 1, *tail), "seg composite")
    # N == 0 is a no-op (no launch)
    assert lib.nerf_march_seg_composite_fwd(None, None, 0, None, dummy, None, 0.005, 1, None, None, None, None) == 0
    assert lib.nerf_march_segments(None, 0, None, 800, None, 128, None, bbox, dummy, None, None, None, None) == 0


def test_train_renderer_key_is_validated():
    """task_arg.train_renderer: hierarchical (default) | accelerated; anything else is refused, and
    accelerated without its grid file raises naming occupancy_grid.py (no GPU needed)."""
    os.environ.setdefault("NERF_AMD_NO_ARGV", "1")
    from src.config import cfg
    from src.train.trainers.nerf import NetworkWrapper
    assert cfg.task_arg.get("train_renderer", "hierarchical") == "hierarchical"
    old = cfg.task_arg.get("train_renderer", None)
    cwd = os.getcwd()
    try:
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            os.chdir(d)
            cfg.task_arg.train_renderer = "accelerated"
            with pytest.raises(FileNotFoundError, match="occupancy_grid.py"):
                NetworkWrapper(None)
            cfg.task_arg.train_renderer = "fast"
            with pytest.raises(ValueError, match="train_renderer"):
                NetworkWrapper(None)
    finally:
        os.chdir(cwd)
        if old is None:
            cfg.task_arg.pop("train_renderer", None)
        else:
            cfg.task_arg.train_renderer = old
