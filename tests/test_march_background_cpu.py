"""CPU: random background colours for the training march (task_arg.train_background) -- the three new
entry points in the header and the ctypes table, their argument checks (no launch, no GPU), the checks of
the ``bg`` tensor, the configuration key's default and validation, and the identity the white case of
nerf_raygen_rgba rests on: the separately rounded fp32 blend onto bg = 1 is the loader's white composite."""
import ctypes
import os
import re

import numpy as np
import pytest

from march_support import _declared, blend_f32, built_lib as lib, restored_keys

os.environ.setdefault("NERF_AMD_NO_ARGV", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = "train_background"
FWD, BWD, RAYGEN = "nerf_march_seg_composite_fwd_bg", "nerf_march_seg_composite_bwd_bg", "nerf_raygen_rgba"


def test_header_and_signature_table_have_the_three_symbols(lib):
    from nerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_amd.h")).read(), flags=re.S)
    # each _bg signature is the _dist one plus the colours, placed before the stream
    for name, like in ((FWD, "nerf_march_seg_composite_fwd_dist"), (BWD, "nerf_march_seg_composite_bwd_dist")):
        got, dist = _declared(text, name), _declared(text, like)
        assert got == dist[:-1] + ["const float* bg", "hipStream_t stream"], name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args == _lib.SIGNATURES[like][1][:-1] + [ctypes.c_void_p] * 2, name
        assert hasattr(lib, name), name
    # nerf_raygen's arguments with the RGBA images in the place of images, the colours in after them and out last
    ray, rgba = _declared(text, "nerf_raygen"), _declared(text, RAYGEN)
    i = ray.index("const float* images")
    assert rgba == (ray[:i] + ["const float* images_rgba", "const float* bg_in"] + ray[i + 1:-1]
                    + ["float* bg_out", "hipStream_t stream"])
    res, args = _lib.SIGNATURES[RAYGEN]
    assert res is ctypes.c_int and len(args) == len(rgba) == len(_lib.SIGNATURES["nerf_raygen"][1]) + 2
    assert args[:9] == _lib.SIGNATURES["nerf_raygen"][1][:9] and hasattr(lib, RAYGEN)
    # the entry points every existing caller uses keep their signatures
    assert len(_lib.SIGNATURES["nerf_raygen"][1]) == len(ray) == 14
    assert len(_lib.SIGNATURES["nerf_march_seg_composite_fwd_dist"][1]) == 16
    assert len(_lib.SIGNATURES["nerf_march_seg_composite_bwd_dist"][1]) == 17
    assert lib.nerf_abi_version() == 4  # additions do not bump it


D = ctypes.c_void_p(16)  # never dereferenced: the argument checks come first


def _fwd(lib, N, seg_off=D, inv_range=0.25, dist=D, totals=D, bg=D, rays=D, rgb=D):
    return lib.nerf_march_seg_composite_fwd_bg(D, rays, N, D, seg_off, D, 0.005, 1, rgb, D, D, None, inv_range, dist,
                                               totals, bg, None)


def _bwd(lib, N, seg_off=D, inv_range=0.25, totals=D, bg=D, rays=D):
    return lib.nerf_march_seg_composite_bwd_bg(D, rays, N, D, seg_off, D, 0.005, 1, D, D, D, None, inv_range, D, totals,
                                               D, bg, None)


def _raygen(lib, R, c2w=D, images=D, rays=D, rgb=D, offset=3, n_img=2, H=4, W=4):
    return lib.nerf_raygen_rgba(c2w, n_img, H, W, 5.0, None, R, 7, offset, images, None, rays, rgb, None, None, None)


def test_argument_errors_without_gpu(lib):
    from nerf_amd._lib import check
    # the compositing pair: N == 0 is a no-op with and without the colours and the distortion outputs
    for bg in (D, None):
        assert _fwd(lib, 0, bg=bg) == 0 and _fwd(lib, 0, dist=None, totals=None, bg=bg) == 0
        assert _bwd(lib, 0, bg=bg) == 0 and _bwd(lib, 0, totals=None, bg=bg) == 0
    for bg in (D, None):  # a null bg forwards to the existing entry points: the same errors
        assert _fwd(lib, -1, bg=bg) == -22 and _bwd(lib, -1, bg=bg) == -22
        with pytest.raises(RuntimeError, match="N must be"):
            check(_fwd(lib, -1, bg=bg), FWD)
        for call in (_fwd, _bwd):
            assert call(lib, 4, seg_off=None, bg=bg) == -22
            with pytest.raises(RuntimeError, match="seg_off is null"):
                check(call(lib, 4, seg_off=None, bg=bg), FWD)
            assert call(lib, 4, rays=None, bg=bg) == -22
            with pytest.raises(RuntimeError, match="null pointer"):
                check(call(lib, 4, rays=None, bg=bg), FWD)
            # with the distortion outputs: inv_range is checked ...
            for bad in (0.0, -0.25, float("nan"), float("inf")):
                assert call(lib, 4, inv_range=bad, bg=bg) == -22
                with pytest.raises(RuntimeError, match="inv_range"):
                    check(call(lib, 4, inv_range=bad, bg=bg), FWD)
        assert _fwd(lib, 4, totals=None, bg=bg) == -22  # dist without its totals
        with pytest.raises(RuntimeError, match="totals is null"):
            check(_fwd(lib, 4, totals=None, bg=bg), FWD)
        assert _fwd(lib, 4, rgb=None, dist=None, totals=None, inv_range=0.0, bg=bg) == -22  # ... and not without them:
        with pytest.raises(RuntimeError, match="null pointer"):   # (this error is the outputs', not inv_range's)
            check(_fwd(lib, 4, rgb=None, dist=None, totals=None, inv_range=0.0, bg=bg), FWD)
        assert _bwd(lib, 4, rays=None, totals=None, inv_range=float("nan"), bg=bg) == -22
        with pytest.raises(RuntimeError, match="null pointer"):
            check(_bwd(lib, 4, rays=None, totals=None, inv_range=float("nan"), bg=bg), BWD)
    with pytest.raises(RuntimeError, match=FWD):  # (the message names the entry point that was called)
        check(_fwd(lib, 4, seg_off=None), FWD)
    with pytest.raises(RuntimeError, match=BWD):
        check(_bwd(lib, 4, seg_off=None), BWD)
    # ray generation
    assert _raygen(lib, 0) == 0 and _raygen(lib, 0, images=None, rays=None, rgb=None) == 0  # R == 0: a no-op
    for kw, match in (({"images": None}, "null pointer"), ({"rays": None}, "null pointer"),
                      ({"rgb": None}, "null pointer"), ({"c2w": None}, "null pointer"),
                      ({"offset": 1 << 63}, "offset must be < 2\\^63"), ({"offset": (1 << 64) - 1}, "offset"),
                      ({"images": ctypes.c_void_p(20)}, "16-byte aligned"), ({"n_img": 0}, "bad sizes"),
                      ({"H": 0}, "bad sizes")):
        assert _raygen(lib, 8, **kw) == -22, kw
        with pytest.raises(RuntimeError, match=match):
            check(_raygen(lib, 8, **kw), RAYGEN)
    assert _raygen(lib, -1) == -22


def test_ops_check_the_colours_before_the_device():
    import torch
    from nerf_amd import ops
    rays = torch.zeros(4, 6)
    grid = torch.ones(8, 8, 8, dtype=torch.bool)
    for bad in (torch.zeros(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float16),
                torch.zeros(4, 3, dtype=torch.int32), np.zeros((4, 3), np.float32), [[0.0] * 3] * 4):
        with pytest.raises(TypeError, match="bg must be a float32 tensor"):
            ops.march_grad(None, rays, 2.0, 6.0, grid, bg=bad)
    for bad in (torch.zeros(4), torch.zeros(3, 3), torch.zeros(5, 3), torch.zeros(4, 4), torch.zeros(4, 1),
                torch.zeros(1, 3), torch.zeros(4, 3, 1), torch.zeros(3, 4).t(), torch.zeros(4, 6)[:, :3]):
        with pytest.raises(ValueError, match="bg must be contiguous \\[4,3\\]"):
            ops.march_grad(None, rays, 2.0, 6.0, grid, bg=bad)
    with pytest.raises(ValueError, match="bg is on"):
        ops.march_grad(None, rays, 2.0, 6.0, grid, bg=torch.zeros(4, 3, device="meta"))
    with pytest.raises(TypeError, match="bg must be"):  # the autograd function checks it as well
        ops._MarchSegComposite.apply(torch.zeros(0, 4), rays, torch.zeros(8), torch.zeros(5, dtype=torch.int32),
                                     torch.zeros(0, dtype=torch.int32), 0.005, True, None, None,
                                     torch.zeros(4, 3, dtype=torch.float64))
    # raygen: the colours need the RGBA images
    c2w = torch.eye(4)[None]
    with pytest.raises(ValueError, match="images_rgba"):
        ops.raygen(c2w, 4, 4, 5.0, n_rays=4, want_bg=True)
    with pytest.raises(ValueError, match="images_rgba"):
        ops.raygen(c2w, 4, 4, 5.0, n_rays=4, images=torch.zeros(1, 4, 4, 3), bg=torch.zeros(4, 3))
    with pytest.raises(ValueError, match="not both"):
        ops.raygen(c2w, 4, 4, 5.0, n_rays=4, images=torch.zeros(1, 4, 4, 3), images_rgba=torch.zeros(1, 4, 4, 4))
    with pytest.raises(ValueError, match=r"\[n_img,H,W,4\]"):
        ops.raygen(c2w, 4, 4, 5.0, n_rays=4, images_rgba=torch.zeros(1, 4, 4, 3))
    with pytest.raises(ValueError, match=r"bg must be \[4,3\]"):
        ops.raygen(c2w, 4, 4, 5.0, n_rays=4, images_rgba=torch.zeros(1, 4, 4, 4), bg=torch.zeros(5, 3))


@pytest.fixture()
def task_arg():
    from src.config import cfg
    with restored_keys(cfg.task_arg, ("train_renderer", "train_grid", "train_background")) as ta:
        yield ta


def test_config_key_default_and_validation(task_arg, tmp_path, monkeypatch):
    from src.models.nerf.renderer.volume_renderer import train_background_setting
    from src.train.trainers.nerf import NetworkWrapper
    monkeypatch.chdir(tmp_path)
    assert task_arg[KEY] == "white"  # in the shipped configuration, off
    assert train_background_setting(task_arg) == "white"
    assert task_arg.get("train_renderer", "hierarchical") == "hierarchical"
    assert NetworkWrapper(None).train_background == "white"  # white with the hierarchical renderer constructs
    node = task_arg.pop(KEY)  # a configuration without the key: white as well
    try:
        assert train_background_setting(task_arg) == "white" and NetworkWrapper(None).train_background == "white"
    finally:
        task_arg[KEY] = node
    task_arg[KEY] = "random"
    assert train_background_setting(task_arg) == "random"
    with pytest.raises(ValueError, match=KEY):
        NetworkWrapper(None)  # the hierarchical compositor has no colour per ray
    for bad in ("black", "Random", "WHITE", "", 1, 0, True, False, 0.5, ["random"]):
        task_arg[KEY] = bad
        with pytest.raises(ValueError, match=KEY):
            train_background_setting(task_arg)
        for renderer in ("accelerated", "hierarchical"):
            task_arg.train_renderer = renderer
            with pytest.raises(ValueError, match=KEY):
                NetworkWrapper(None)
        task_arg.train_renderer = "hierarchical"
    # accelerated + random is accepted: the key is read before the grid file is looked for
    task_arg[KEY] = "random"
    task_arg.train_renderer = "accelerated"
    with pytest.raises(FileNotFoundError, match="occupancy_grid.py"):
        NetworkWrapper(None)


def test_dataset_needs_alpha_in_random_mode(task_arg):
    import torch
    from src.datasets.nerf.blender import Dataset
    from src.datasets.nerf.synthetic import make_scene, make_scene_rgba
    rgba, poses, focal = make_scene_rgba(2, 8, 8, "cpu")
    rgb, poses3, focal3 = make_scene(2, 8, 8, "cpu")
    assert rgba.shape == (2, 8, 8, 4) and torch.equal(poses, poses3) and focal == focal3
    a = rgba[..., 3]
    assert bool(((a == 0) | (a == 1)).all()) and 0 < float(a.mean()) < 1  # hits and background
    assert torch.equal(rgba[..., :3] * rgba[..., 3:] + (1.0 - rgba[..., 3:]), rgb)  # make_scene, bit for bit
    # white: an alpha channel is composited away, as the loader does; nothing is kept of it
    for ds in (Dataset.from_arrays(rgba, poses, focal), Dataset.from_arrays(rgba[..., :3], poses, focal, alpha=a)):
        assert ds.images_rgba is None and torch.equal(ds.images, rgb) and ds.n_img == 2
    assert torch.equal(Dataset.from_arrays(rgb, poses, focal).images, rgb)
    task_arg[KEY] = "random"
    with pytest.raises(ValueError, match="alpha"):
        Dataset.from_arrays(rgb, poses, focal)  # a train split without alpha
    for ds in (Dataset.from_arrays(rgba, poses, focal), Dataset.from_arrays(rgba[..., :3], poses, focal, alpha=a)):
        assert torch.equal(ds.images_rgba, rgba) and ds._images is None  # one copy of the pixels ...
        assert torch.equal(ds.images, rgb) and ds.n_img == 2 and (ds.H, ds.W) == (8, 8)  # ... images on demand
    test = Dataset.from_arrays(rgb, poses, focal, split="test")  # the test split never draws: no alpha needed
    assert test.images_rgba is None and torch.equal(test.images, rgb)
    assert Dataset.from_arrays(rgba, poses, focal, split="test").images_rgba is None


def test_loaders_on_a_png(tmp_path):
    from PIL import Image
    from src.datasets.nerf.blender import load_png_rgb, load_png_rgba
    px = _rgba_fixture()
    Image.fromarray(px, "RGBA").save(str(tmp_path / "a.png"))
    Image.fromarray(px[..., :3].copy(), "RGB").save(str(tmp_path / "b.png"))
    a = load_png_rgba(str(tmp_path / "a.png"))
    assert a.dtype == np.float32 and a.shape == (16, 16, 4)
    np.testing.assert_array_equal(a, px.astype(np.float32) / 255.0)
    np.testing.assert_array_equal(a[..., :3] * a[..., -1:] + (1.0 - a[..., -1:]), load_png_rgb(str(tmp_path / "a.png")))
    with pytest.raises(ValueError, match="no alpha channel"):
        load_png_rgba(str(tmp_path / "b.png"))


def _rgba_fixture():
    """16 x 16 RGBA uint8: random colours; alpha 0 on a quarter, 255 on a quarter, random between on the rest."""
    rng = np.random.default_rng(11)
    px = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    px[:4, :, 3] = 0
    px[4:8, :, 3] = 255
    px[8:, :, 3] = rng.integers(1, 255, (8, 16), dtype=np.uint8)
    assert (px[..., 3] == 0).any() and (px[..., 3] == 255).any() and ((px[..., 3] > 0) & (px[..., 3] < 255)).any()
    return px


def test_white_composite_identity():
    """fmul(1 - a, 1) is 1 - a exactly, so on bg = 1 the blend is load_png_rgb's expression bit for bit: what
    lets nerf_raygen_rgba with bg_in = ones stand in for nerf_raygen on the white-composited images."""
    a = _rgba_fixture().astype(np.float32) / 255.0
    loader = a[..., :3] * a[..., -1:] + (1.0 - a[..., -1:])  # load_png_rgb, blender.py
    assert loader.dtype == np.float32
    got = blend_f32(a, np.ones(3, np.float32))
    np.testing.assert_array_equal(got.view(np.uint32), loader.view(np.uint32))
    # (and it is a blend: transparent pixels are white, opaque ones their colour, bit for bit)
    np.testing.assert_array_equal(got[:4], np.ones((4, 16, 3), np.float32))
    np.testing.assert_array_equal(got[4:8], a[4:8, :, :3])
    # any other colour moves the transparent pixels only by that colour
    bg = np.array([0.2, 0.5, 0.8], np.float32)
    np.testing.assert_array_equal(blend_f32(a, bg)[:4], np.broadcast_to(bg, (4, 16, 3)))
    np.testing.assert_array_equal(blend_f32(a, bg)[4:8], a[4:8, :, :3])
