"""Random background colours for the training march on the GPU (task_arg.train_background: random).

nerf_raygen_rgba draws a colour per ray and blends the straight-alpha ground truth onto it; the BG
instantiations of the segment compositing kernels (nerf_march_seg_composite_fwd_bg / _bwd_bg) composite the
prediction onto the same colour:  rgb_r = sum_k w_k c_k + (1 - acc_r) bg_r,  g_acc' = g_acc - g_rgb . bg_r.

Checked here: the ray generation against nerf_raygen and a numpy Philox / blend, bit for bit; the kernels
against fp64 (march_support's long-segment case, test_gpu_march_distortion.py's too: segments that cross the
backward's 64-chunk register window, alpha == 1 points, surplus tails), with and without the distortion term and
the per-ray shift; the identities with the white / black entry points, bit for bit; that a white floater in front of a
transparent pixel gets a density gradient (the point of the key); ops.march_grad(bg=) on the trained fixture
net; the renderer, the dataset and the trainer; and that a step trains.
"""
import os

import numpy as np
import pytest
import torch

from march_support import (ALPHA_ONE, INV_RANGE, LONG, MAPS, STEP, _batch, _dist_double_sum, _dist_prefix, _flat_grad,
                           _march_grad, _per_segment_bound, _trained_net, _trainer, _write_grid, blend_f32, fp32_cfg,
                           g2, long_segment_case, trained_grid)

pytestmark = pytest.mark.gpu

os.environ.setdefault("NERF_AMD_NO_ARGV", "1")
KEY = "train_background"


# --------------------------------------------------------------------------------------
# 1. ray generation
# --------------------------------------------------------------------------------------
def _philox_xyz(n, seed, offset):
    """Philox-4x32-10, key (seed lo, seed hi), counter (idx lo, idx hi, offset lo, offset hi | 0x80000000) --
    the pixel draw's counter with the top bit flipped: words 0, 1, 2 (test_gpu_march_jitter's word 0, extended)."""
    mask = np.uint64(0xFFFFFFFF)
    sh = np.uint64(32)
    idx = np.arange(n, dtype=np.uint64)
    c = [idx & mask, idx >> sh, np.full(n, offset & 0xFFFFFFFF, dtype=np.uint64),
         np.full(n, (offset >> 32) | 0x80000000, dtype=np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]  # 32 x 32 -> 64 bits: no overflow
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & mask, (p0 >> sh) ^ c[3] ^ k1, p0 & mask]
        k0 = (k0 + np.uint64(0x9E3779B9)) & mask
        k1 = (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack([(w >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24) for w in c[:3]], 1)


def _rgba_images():
    """3 images of 8 x 8, float32 of uint8 / 255 like the loader's; alpha 0, 1 and values between."""
    rng = np.random.default_rng(3)
    px = rng.integers(0, 256, (3, 8, 8, 4), dtype=np.uint8)
    px[:, :2, :, 3] = 0
    px[:, 2:4, :, 3] = 255
    return px.astype(np.float32) / 255.0


@pytest.mark.parametrize("seed,offset", [(12345, 4), ((1 << 40) + 7919 * 3 + 1, (1 << 62) + (1 << 33) + 9)])
def test_ray_generation(cuda, seed, offset):
    from nerf_amd import ops
    from src.datasets.nerf.synthetic import view_poses
    H = W = 8
    focal, R = 11.5, 1000
    c2w = view_poses(3, 2).to(cuda)
    rgba = _rgba_images()
    img = torch.from_numpy(rgba).to(cuda)
    flat = rgba.reshape(-1, 4)
    rays0, none0, pix0 = ops.raygen(c2w, H, W, focal, n_rays=R, seed=seed, offset=offset, want_pix=True)
    rays1, rgb1, pix1, bg1 = ops.raygen(c2w, H, W, focal, n_rays=R, seed=seed, offset=offset, want_pix=True,
                                        images_rgba=img, want_bg=True)
    assert none0 is None and torch.equal(pix1, pix0) and torch.equal(rays1, rays0)  # the same rays, bit for bit
    pix = pix0.cpu().numpy()
    assert pix.min() >= 0 and pix.max() < 3 * H * W and len(np.unique(pix)) > 150  # (of 192: all three images)
    bg = bg1.cpu().numpy()
    want_bg = _philox_xyz(R, seed, offset)
    assert want_bg.dtype == np.float32 and want_bg.shape == (R, 3)
    np.testing.assert_array_equal(bg, want_bg)  # exact
    assert bg.min() >= 0.0 and bg.max() < 1.0 and len(np.unique(bg)) > 2990  # a stream in [0, 1)
    np.testing.assert_array_equal(rgb1.cpu().numpy().view(np.uint32), blend_f32(flat[pix], bg).view(np.uint32))
    # want_bg off: the same draw, not returned
    rays2, rgb2, pix2, none2 = ops.raygen(c2w, H, W, focal, n_rays=R, seed=seed, offset=offset, images_rgba=img)
    assert none2 is None and pix2 is None and torch.equal(rgb2, rgb1) and torch.equal(rays2, rays0)
    # bg_in = ones: nerf_raygen on the white-composited images (test_march_background_cpu: the numpy identity)
    white = torch.from_numpy(rgba[..., :3] * rgba[..., -1:] + (1.0 - rgba[..., -1:])).to(cuda)
    _, rgb_w, _ = ops.raygen(c2w, H, W, focal, n_rays=R, seed=seed, offset=offset, images=white)
    ones = torch.ones(R, 3, device=cuda)
    rays3, rgb3, _, bg3 = ops.raygen(c2w, H, W, focal, n_rays=R, seed=seed, offset=offset, images_rgba=img, bg=ones,
                                     want_bg=True)
    assert torch.equal(rgb3, rgb_w) and torch.equal(bg3, ones) and torch.equal(rays3, rays0)
    # an injected bg_in comes back in bg_out, and is what the blend used
    inj = torch.rand(R, 3, generator=torch.Generator().manual_seed(9)).to(cuda)
    inj[0], inj[1] = 0.0, 1.0
    _, rgb4, _, bg4 = ops.raygen(c2w, H, W, focal, n_rays=R, seed=seed, offset=offset, images_rgba=img, bg=inj,
                                 want_bg=True)
    assert torch.equal(bg4, inj)
    np.testing.assert_array_equal(rgb4.cpu().numpy().view(np.uint32),
                                  blend_f32(flat[pix], inj.cpu().numpy()).view(np.uint32))
    # pixel ids given: every pixel once, in reverse -- the rays of nerf_raygen, the colours drawn per ray index
    given = torch.arange(3 * H * W - 1, -1, -1, device=cuda)
    rays_g0, _, _ = ops.raygen(c2w, H, W, focal, pix=given)
    rays_g, rgb_g, pix_g, bg_g = ops.raygen(c2w, H, W, focal, pix=given, seed=seed, offset=offset, images_rgba=img,
                                            want_pix=True, want_bg=True)
    assert torch.equal(rays_g, rays_g0) and torch.equal(pix_g, given)
    np.testing.assert_array_equal(bg_g.cpu().numpy(), want_bg[:3 * H * W])
    np.testing.assert_array_equal(rgb_g.cpu().numpy().view(np.uint32),
                                  blend_f32(flat[::-1], want_bg[:3 * H * W]).view(np.uint32))
    # another offset: other colours; the same offset: the same colours
    _, _, _, bg5 = ops.raygen(c2w, H, W, focal, n_rays=R, seed=seed, offset=offset + 1, images_rgba=img, want_bg=True)
    _, _, _, bg6 = ops.raygen(c2w, H, W, focal, n_rays=R, seed=seed, offset=offset, images_rgba=img, want_bg=True)
    assert not torch.equal(bg5, bg1) and torch.equal(bg6, bg1)
    np.testing.assert_array_equal(bg5.cpu().numpy(), _philox_xyz(R, seed, offset + 1))
    # no rays
    e = ops.raygen(c2w, H, W, focal, n_rays=0, seed=seed, offset=offset, images_rgba=img, want_bg=True)
    assert e[0].shape == (0, 6) and e[1].shape == (0, 3) and e[3].shape == (0, 3)
    with pytest.raises(RuntimeError, match="offset must be < 2\\^63"):
        ops.raygen(c2w, H, W, focal, n_rays=4, seed=seed, offset=1 << 63, images_rgba=img)


# --------------------------------------------------------------------------------------
# 2. the segment kernels against fp64
# --------------------------------------------------------------------------------------
BLACK, WHITE = 5, 8  # the rays whose colour is exactly (0,0,0) / (1,1,1): segments of 65 and 800 points


def _colours(n):
    bg = torch.rand(n, 3, generator=torch.Generator().manual_seed(21))
    bg[BLACK] = 0.0
    bg[WHITE] = 1.0
    return bg


def _shifts(n):
    s = (torch.rand(n, generator=torch.Generator().manual_seed(22)) * STEP).to(torch.float32)
    s[0] = 0.0
    return s


def _reference(c, bg, t_shift):
    """fp64 on the CPU, out of place: test_gpu_march_distortion's compositor with rgb composited onto bg[r]; the
    depths are the kernel's (one rounded fp32 add of the ray's shift); the distortion by its O(n^2) definition,
    by the prefix-sum form (shown equal to it there) on the two long segments."""
    raw = c["raw"].double().requires_grad_(True)
    off = c["seg_off"].tolist()
    rgb, depth, acc, dist = [], [], [], []
    for r in range(c["N"]):
        sl = slice(off[r], off[r + 1])
        st = c["out_step"][sl].long()
        valid = (st >= 0).double()
        col = torch.sigmoid(raw[sl, :3])
        sigma = torch.relu(raw[sl, 3])
        d = STEP * torch.linalg.vector_norm(c["rays"][r, 3:6].double())
        alpha = (1.0 - torch.exp(-sigma * d)) * valid
        T = torch.cat([torch.ones(1, dtype=torch.float64), torch.cumprod(1.0 - alpha, 0)[:-1]])
        w = T * alpha
        t = c["t_table"][st.clamp(min=0)]
        t = (t if t_shift is None else t + t_shift[r]).double()
        a = w.sum()
        rgb.append((w[:, None] * col).sum(0) + (1.0 - a) * bg[r].double())
        depth.append((w * t).sum())
        acc.append(a)
        dist.append(_dist_prefix(w, t) if r in LONG else _dist_double_sum(w, t))
    rgb, depth, acc, dist = torch.stack(rgb), torch.stack(depth), torch.stack(acc), torch.stack(dist)
    g_rgb, g_depth, g_acc, g_dist = (x.double() for x in c["cot"])
    three = (rgb * g_rgb).sum() + (depth * g_depth).sum() + (acc * g_acc).sum()
    (g_three,) = torch.autograd.grad(three, raw, retain_graph=True)
    (g_all,) = torch.autograd.grad(three + (dist * g_dist).sum(), raw)
    return dict(rgb=rgb.detach(), depth=depth.detach(), acc=acc.detach(), dist=dist.detach(), g_three=g_three,
                g_all=g_all)


@pytest.fixture(scope="module")
def segment_case():
    c = long_segment_case()
    assert c["lens"][BLACK] == 65 and c["lens"][WHITE] == 800
    c["bg"], c["shift"] = _colours(c["N"]), _shifts(c["N"])
    c["ref"] = {s: _reference(c, c["bg"], c["shift"] if s else None) for s in (False, True)}  # computed once, shared
    return c


def _apply(c, cuda, white, dist=False, t_shift=None, bg=None):
    from nerf_amd import ops
    raw = c["raw"].to(cuda).requires_grad_(True)
    maps = ops._MarchSegComposite.apply(raw, c["rays"].to(cuda), c["t_table"].to(cuda), c["seg_off"].to(cuda),
                                        c["out_step"].to(cuda), STEP, white,
                                        None if t_shift is None else t_shift.to(cuda), INV_RANGE if dist else None,
                                        None if bg is None else bg.to(cuda))
    return raw, maps


def _grad(c, cuda, raw, maps):
    cot = [x.to(cuda) for x in c["cot"]][:len(maps)]
    (g,) = torch.autograd.grad(list(maps), [raw], cot)
    return g


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("dist", [False, True])
def test_background_kernels_against_fp64(cuda, segment_case, dist, shift):
    c, ref = segment_case, segment_case["ref"][shift]
    raw, maps = _apply(c, cuda, True, dist, c["shift"] if shift else None, c["bg"])
    assert len(maps) == (4 if dist else 3)
    g = _grad(c, cuda, raw, maps).cpu()
    assert bool(torch.isfinite(g).all())
    errs = {k: float((m.detach().cpu().double() - ref[k]).abs().max()) for k, m in zip(("rgb", "depth", "acc"), maps)}
    worst = _per_segment_bound(c, g, ref["g_all" if dist else "g_three"], "bg")
    print(f"\ndist {dist}, shift {shift}: max |error| rgb {errs['rgb']:.3e}, depth {errs['depth']:.3e}, acc "
          f"{errs['acc']:.3e}; g_raw worst error / segment's largest {worst:.3e}")
    # the bounds of test_gpu_march_distortion (all within the 1e-4 of the fp32 contract)
    assert errs["rgb"] <= 1e-5 and errs["acc"] <= 1e-5 and errs["depth"] <= 5e-5, errs
    if dist:
        d, rd = maps[3].detach().cpu().double(), ref["dist"]
        print(f"dist max rel err {float(((d - rd).abs() / rd.abs().clamp(min=1e-300)).max()):.3e}")
        assert bool(((d - rd).abs() <= 1e-4 * rd.abs() + 1e-12).all())
    # the colours reached the kernel: an empty segment is its colour, and the result is not the white one
    assert c["lens"][0] == 0 and torch.equal(maps[0][0].detach().cpu(), c["bg"][0])
    _, white_maps = _apply(c, cuda, True, dist, c["shift"] if shift else None)
    assert not torch.equal(white_maps[0], maps[0])
    assert torch.equal(white_maps[1], maps[1]) and torch.equal(white_maps[2], maps[2])  # depth, acc: untouched
    if dist:
        assert torch.equal(white_maps[3], maps[3])
    # exact zeros: after an alpha == 1 point, on surplus points
    off = c["seg_off"].tolist()
    for seg, pos in ALPHA_ONE:
        tail = g[off[seg] + pos + 1:off[seg + 1]]
        assert tail.numel() > 0 and bool((tail == 0).all()), seg
    assert bool((g[c["out_step"] < 0] == 0).all())


# --------------------------------------------------------------------------------------
# 3. identities, bit for bit
# --------------------------------------------------------------------------------------
def _direct(c, cuda, white, bg, dist, t_shift=None):
    """nerf_march_seg_composite_fwd_bg / _bwd_bg called as they are (bg may be None: a null pointer)."""
    from nerf_amd._lib import check, lib, ptr
    N = c["N"]
    dev = {k: c[k].to(cuda).contiguous() for k in ("raw", "rays", "t_table", "seg_off", "out_step")}
    cot = [x.to(cuda).contiguous() for x in c["cot"]]
    bg = None if bg is None else bg.to(cuda).contiguous()
    t_shift = None if t_shift is None else t_shift.to(cuda)
    rgb, depth, acc = torch.empty(N, 3, device=cuda), torch.empty(N, device=cuda), torch.empty(N, device=cuda)
    dmap = torch.empty(N, device=cuda) if dist else None
    totals = torch.empty(N, 2, device=cuda, dtype=torch.float64) if dist else None
    g_raw = torch.empty_like(dev["raw"])
    s = torch.cuda.current_stream(cuda).cuda_stream
    inv = INV_RANGE if dist else float("nan")  # (not looked at without the distortion outputs)
    head = (ptr(dev["raw"]), ptr(dev["rays"]), N, ptr(dev["t_table"]), ptr(dev["seg_off"]), ptr(dev["out_step"]),
            STEP, int(white))
    check(lib().nerf_march_seg_composite_fwd_bg(*head, ptr(rgb), ptr(depth), ptr(acc), ptr(t_shift), inv, ptr(dmap),
                                                ptr(totals), ptr(bg), s), "fwd_bg")
    check(lib().nerf_march_seg_composite_bwd_bg(*head, ptr(cot[0]), ptr(cot[1]), ptr(cot[2]), ptr(t_shift), inv,
                                                ptr(cot[3]) if dist else None, ptr(totals), ptr(g_raw), ptr(bg), s),
          "bwd_bg")
    torch.cuda.synchronize()
    return [rgb, depth, acc] + ([dmap] if dist else []), g_raw


def _same(a, b):
    (maps_a, g_a), (maps_b, g_b) = a, b
    assert len(maps_a) == len(maps_b)
    for x, y in zip(maps_a, maps_b):
        assert torch.equal(x.detach(), y.detach())
    assert float(g_a.abs().max()) > 0 and torch.equal(g_a, g_b)


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("dist", [False, True])
def test_identities_bit_for_bit(cuda, segment_case, dist, shift):
    c = segment_case
    sh = c["shift"] if shift else None
    ones, zeros = torch.ones(c["N"], 3), torch.zeros(c["N"], 3)
    existing = {}
    for white in (False, True):  # the existing entry points, through ops
        raw, maps = _apply(c, cuda, white, dist, sh)
        existing[white] = (list(maps), _grad(c, cuda, raw, maps))
    assert not torch.equal(existing[True][0][0], existing[False][0][0])
    assert not torch.equal(existing[True][1], existing[False][1])
    for white in (False, True):
        _same(_direct(c, cuda, white, ones, dist, sh), existing[True])    # bg = 1 is white = 1 ...
        _same(_direct(c, cuda, white, zeros, dist, sh), existing[False])  # ... bg = 0 is white = 0, whatever `white`
        _same(_direct(c, cuda, white, None, dist, sh), existing[white])   # a null bg: the existing entry points
    _same(_direct(c, cuda, False, c["bg"], dist, sh), _direct(c, cuda, True, c["bg"], dist, sh))
    raw, maps = _apply(c, cuda, True, dist, sh, c["bg"])  # ops with the colours makes the same two calls
    _same((list(maps), _grad(c, cuda, raw, maps)), _direct(c, cuda, True, c["bg"], dist, sh))


def test_launches(cuda, segment_case):
    """With the colours one forward and one backward launch, as without; without them the names they had."""
    from nerf_amd import ops
    c = segment_case
    kt = ops.KERNEL_TIMES
    old = (kt.enabled, kt.detail)
    kt.enabled = kt.detail = True
    names = {}
    try:
        for key, (dist, bg) in {"plain": (False, None), "dist": (True, None), "bg": (False, c["bg"]),
                                "bg_dist": (True, c["bg"])}.items():
            kt.reset()
            raw, maps = _apply(c, cuda, True, dist, None, bg)
            _grad(c, cuda, raw, maps)
            names[key] = [p[0] for p in kt.pending]
    finally:
        kt.enabled, kt.detail = old
        kt.reset()
    assert names["plain"] == ["march_seg_composite_fwd", "march_seg_composite_bwd"]
    assert names["dist"] == ["march_seg_composite_fwd_dist", "march_seg_composite_bwd_dist"]
    assert names["bg"] == names["bg_dist"] == ["march_seg_composite_fwd_bg", "march_seg_composite_bwd_bg"]


# --------------------------------------------------------------------------------------
# 4. the white floater gets a gradient
# --------------------------------------------------------------------------------------
def _floater(cuda, bg, white=True, cot=None):
    """One ray, a 3-point segment: point 0 white (colour logits +20: c is 1 in fp32) with sigma logit 1, the two
    points behind it empty.  The ground truth is the background itself (an a = 0 pixel).  -> d MSE / d raw (or
    the gradient under the cotangent ``cot`` of rgb), the cotangent of rgb."""
    from nerf_amd import ops
    raw = torch.tensor([[20.0, 20.0, 20.0, 1.0], [0.3, -0.2, 0.1, -1.0], [-0.5, 0.4, 0.2, -1.0]],
                       device=cuda, requires_grad=True)
    rays = torch.tensor([[0.0, 0.0, 4.0, 0.0, 0.0, -1.0]], device=cuda)
    t_table = torch.arange(2.0, 6.0, 0.005).to(cuda)
    seg_off = torch.tensor([0, 3], dtype=torch.int32, device=cuda)
    out_step = torch.tensor([100, 200, 300], dtype=torch.int32, device=cuda)
    args = [raw, rays, t_table, seg_off, out_step, STEP, white, None, None]
    gt = torch.ones(1, 3, device=cuda)
    if bg is not None:
        gt = torch.tensor([bg], device=cuda)
        args.append(gt.clone())
    rgb = ops._MarchSegComposite.apply(*args)[0]
    if cot is None:
        rgb.retain_grad()
        torch.nn.functional.mse_loss(rgb, gt).backward()
        return raw.grad.cpu(), rgb.grad.cpu()
    g_rgb = torch.tensor([cot], device=cuda)
    (g,) = torch.autograd.grad([rgb], [raw], [g_rgb])
    return g.cpu(), g_rgb.cpu()


def test_white_floater_gets_a_gradient(cuda):
    # on white the floater is invisible: its density gets no gradient, under the MSE and under any cotangent
    for cot in (None, (0.3, -0.7, 0.5)):
        g, g_rgb = _floater(cuda, None, cot=cot)
        print(f"\nwhite: d / d raw[0,3] = {float(g[0, 3]):.3e}, largest rgb cotangent {float(g_rgb.abs().max()):.3e}")
        assert abs(float(g[0, 3])) <= 1e-7 * float(g_rgb.abs().max())
    assert float(g_rgb.abs().max()) > 0.69  # (the second pass: a cotangent that is not small)
    # on a colour it costs loss: the gradient is positive (descent lowers sigma) and matches fp64
    bg = (0.2, 0.5, 0.8)
    g, g_rgb = _floater(cuda, bg)
    raw3 = torch.tensor(1.0, dtype=torch.float64, requires_grad=True)
    alpha = 1.0 - torch.exp(-torch.relu(raw3) * np.float64(np.float32(STEP)))  # |d| = 1
    c0 = torch.sigmoid(torch.tensor([20.0] * 3, dtype=torch.float64))
    b = torch.tensor(bg, dtype=torch.float32).double()
    pred = alpha * c0 + (1.0 - alpha) * b
    ((pred - b) ** 2).mean().backward()
    want = float(raw3.grad)
    print(f"bg {bg}: d MSE / d raw[0,3] = {float(g[0, 3]):.6e} (fp64 {want:.6e}), largest rgb cotangent "
          f"{float(g_rgb.abs().max()):.3e}")
    assert want > 0 and float(g[0, 3]) > 0
    assert abs(float(g[0, 3]) - want) <= 1e-4 * want
    assert bool((g[1:, 3] == 0).all())  # (the empty points: relu's zero side)


# --------------------------------------------------------------------------------------
# 5. ops.march_grad(bg=) on the trained fixture net and its own bake
# --------------------------------------------------------------------------------------
@pytest.fixture()
def bg_cfg():
    """cfg with the keys the tests below set restored afterwards."""
    yield from fp32_cfg(("train_renderer", "train_grid", "point_budget", "mlp_dtype", "perturb", "chunk_size",
                         "train_rays", "distortion_loss_weight", "train_march_jitter", "train_background"))


@pytest.fixture()
def fixture_net(cuda, bg_cfg, g2, trained_grid):
    """The trained fixture net, its optimizer (the flat gradient), the 256 march rays, a ground truth, colours."""
    from src.train.optimizer import make_optimizer
    net = _trained_net(cuda)
    opt = make_optimizer(bg_cfg, net)
    rays = torch.from_numpy(g2["march_rays"]).to(cuda)
    t_table = torch.from_numpy(g2["march_t_table"]).to(cuda)
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(1)).to(cuda)
    bg = torch.rand(256, 3, generator=torch.Generator().manual_seed(2)).to(cuda)
    return {"net": net, "opt": opt, "rays": rays, "t_table": t_table, "gt": gt, "bg": bg,
            "grid": trained_grid.to(cuda)}


def test_march_grad_with_the_colours(cuda, fixture_net):
    f = fixture_net
    mse = torch.nn.functional.mse_loss
    plain = _march_grad(f, f["rays"])
    out = _march_grad(f, f["rays"], bg=f["bg"])
    assert out["n_queried"] == plain["n_queried"] == 13382
    assert torch.equal(out["depth_map_f"], plain["depth_map_f"]) and torch.equal(out["acc_map_f"], plain["acc_map_f"])
    assert not torch.equal(out["rgb_map_f"], plain["rgb_map_f"]) and out["rgb_map_f"].requires_grad
    flat = _flat_grad(f, mse(out["rgb_map_f"], f["gt"]))
    got = {k: p.grad.detach().clone() for k, p in f["net"].named_parameters()}
    # the comparison run: no background in the kernels, the colours composed in torch
    black = _march_grad(f, f["rays"], white_bkgd=False)
    rgb = black["rgb_map_f"] + (1.0 - black["acc_map_f"])[:, None] * f["bg"]
    np.testing.assert_allclose(out["rgb_map_f"].detach().cpu().numpy(), rgb.detach().cpu().numpy(), rtol=0, atol=1e-6)
    _flat_grad(f, mse(rgb, f["gt"]))
    worst, moved = (0.0, ""), 0
    for k, p in f["net"].named_parameters():
        want = p.grad.detach()
        big = float(want.abs().max())
        if k.startswith("model."):  # the coarse net is not part of the graph
            assert big == 0.0 and float(got[k].abs().max()) == 0.0, k
            continue
        err = float((got[k] - want).abs().max())
        assert big > 0 and err <= 1e-4 * big, (k, err, big)
        worst = max(worst, (err / big, k))
        moved += 1
    print(f"\nlargest entry error {worst[0]:.3e} of its tensor's largest ({worst[1]}), {moved} tensors")
    # bit-reproducible
    again = _march_grad(f, f["rays"], bg=f["bg"])
    assert torch.equal(again["rgb_map_f"], out["rgb_map_f"])
    assert float(flat.abs().max()) > 0 and torch.equal(_flat_grad(f, mse(again["rgb_map_f"], f["gt"])), flat)
    # with the distortion term and a shift as well: the same rgb as the sum of the parts says
    both = _march_grad(f, f["rays"], bg=f["bg"], distortion=True)
    assert torch.equal(both["rgb_map_f"], out["rgb_map_f"]) and both["dist_map_f"].shape == (256,)
    assert torch.equal(both["dist_map_f"], _march_grad(f, f["rays"], distortion=True)["dist_map_f"])


def test_march_grad_colours_under_the_point_budget(cuda, fixture_net):
    f = fixture_net
    mse = torch.nn.functional.mse_loss
    capped = _march_grad(f, f["rays"], bg=f["bg"], max_points=6000, t_table=None)
    kept = capped["rays_kept"]
    assert 0 < kept < 256 and capped["rgb_map_f"].shape == (256, 3)
    direct = _march_grad(f, f["rays"][:kept], bg=f["bg"][:kept].clone(), t_table=None)
    for m in MAPS:
        assert torch.equal(capped[m][:kept], direct[m]), m
    g_capped = _flat_grad(f, mse(capped["rgb_map_f"][:kept], f["gt"][:kept]))
    g_direct = _flat_grad(f, mse(direct["rgb_map_f"], f["gt"][:kept]))
    assert float(g_direct.abs().max()) > 0 and torch.equal(g_capped, g_direct)
    # the dropped rows: pass A's values (the configured background), no graph
    white = _march_grad(f, f["rays"], max_points=6000, t_table=None)
    for m in MAPS:
        assert torch.equal(capped[m][kept:], white[m][kept:]), m
    capped = _march_grad(f, f["rays"], bg=f["bg"], max_points=6000, t_table=None)  # (a fresh graph)
    g_dropped = _flat_grad(f, (capped["rgb_map_f"][kept:] * 3.0).sum() + 0.0 * capped["rgb_map_f"][:kept].sum())
    assert float(g_dropped.abs().max()) == 0.0


# --------------------------------------------------------------------------------------
# 6. renderer, dataset, trainer
# --------------------------------------------------------------------------------------
def test_chunked_step_equals_unchunked(cuda, bg_cfg, g2, trained_grid):
    from src.models.nerf.renderer.volume_renderer import Renderer
    cfg = bg_cfg
    cfg.task_arg[KEY] = "random"
    net = _trained_net(cuda)
    rays = np.concatenate([g2["march_rays"], g2["march_rays"][:44][::-1]])  # 300 rays
    bg = torch.rand(300, 3, generator=torch.Generator().manual_seed(4))
    outs = []
    for chunk in (4096, 128):  # one chunk, then three
        cfg.task_arg.chunk_size = chunk
        r = Renderer(net)
        r.set_occupancy_grid(trained_grid, cuda)
        outs.append(r.render_accelerated(_batch(rays, cuda, bg=bg)))
    whole, parts = outs
    assert parts["n_queried"] == whole["n_queried"] and whole["rgb_map_f"].requires_grad
    for m in MAPS:
        assert parts[m].shape[0] == 300 and torch.equal(parts[m], whole[m]), m
    # the two copies of a ray were composited onto their own colours
    assert torch.equal(whole["acc_map_f"][:44], whole["acc_map_f"][256:].flip(0))
    assert not torch.equal(whole["rgb_map_f"][:44], whole["rgb_map_f"][256:].flip(0))
    with pytest.raises(ValueError, match=KEY):  # the key on and no colours in the batch
        r.render_accelerated(_batch(rays, cuda))
    cfg.task_arg[KEY] = "white"  # the key off: the colours are not looked at
    assert torch.equal(r.render_accelerated(_batch(rays, cuda, bg=bg))["rgb_map_f"],
                       r.render_accelerated(_batch(rays, cuda))["rgb_map_f"])


def test_dataset_draws_colours(cuda, bg_cfg):
    from nerf_amd import ops
    from src.datasets.nerf.blender import Dataset
    from src.datasets.nerf.synthetic import make_scene, make_scene_rgba
    ta = bg_cfg.task_arg
    ta.train_rays = 512
    rgba, poses, focal = make_scene_rgba(4, 16, 16, cuda)
    assert torch.equal(rgba[..., :3] * rgba[..., 3:] + (1.0 - rgba[..., 3:]), make_scene(4, 16, 16, cuda)[0])
    torch.manual_seed(0)
    off = Dataset.from_arrays(rgba, poses, focal)  # the key off: no colours anywhere
    item = off[0]
    assert "bg" not in item and off.images_rgba is None and len(off.sample_batch()) == 2
    ta[KEY] = "random"
    torch.manual_seed(0)
    a = Dataset.from_arrays(rgba, poses, focal)
    torch.manual_seed(0)
    b = Dataset.from_arrays(rgba, poses, focal)
    first, second, other = a[0], a[0], b[0]
    for it in (first, second, other):
        assert it["bg"].shape == (1, 512, 3) and it["rgbs"].shape == (1, 512, 3) and it["rays"].shape == (1, 512, 6)
        assert float(it["bg"].min()) >= 0.0 and float(it["bg"].max()) < 1.0
    assert torch.equal(item["rays"], first["rays"])  # the same rays as with the key off
    assert not torch.equal(first["bg"], second["bg"]) and not torch.equal(first["rays"], second["rays"])
    for k in ("bg", "rgbs", "rays"):  # two datasets of one seed agree
        assert torch.equal(first[k], other[k]), k
    # rgbs is the blend of the gathered pixels
    _, _, pix = ops.raygen(poses, 16, 16, focal, n_rays=512, seed=a.seed, offset=1, want_pix=True)
    px = rgba.reshape(-1, 4)[pix].cpu().numpy()
    assert 0 < float(px[:, 3].mean()) < 1  # hits and background
    np.testing.assert_array_equal(first["rgbs"][0].cpu().numpy().view(np.uint32),
                                  blend_f32(px, first["bg"][0].cpu().numpy()).view(np.uint32))
    # the test split never draws: the white composite, no colours
    test = Dataset.from_arrays(rgba, poses, focal, split="test")
    it = test[1]
    assert "bg" not in it and test.images_rgba is None
    assert torch.equal(it["rgbs"][0], make_scene(4, 16, 16, cuda)[0][1].reshape(-1, 3))


def test_trainer_key_on_off_and_validation(cuda, bg_cfg, g2, trained_grid, tmp_path, monkeypatch):
    from nerf_amd import ops
    cfg = bg_cfg
    ta = cfg.task_arg
    _write_grid(tmp_path, monkeypatch, trained_grid)
    ta.train_renderer = "accelerated"
    ta.train_grid = "file"
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(1))
    bg = torch.rand(256, 3, generator=torch.Generator().manual_seed(2))
    batch = _batch(g2["march_rays"], cuda, gt)
    # the key off -- "white", absent, or white with colours in the batch: the same step, bit for bit, no bg anywhere
    runs = []
    for mode in ("white", "absent", "white+bg"):
        node = ta.pop(KEY) if mode == "absent" else None
        if mode != "absent":
            ta[KEY] = "white"
        try:
            net, trainer, opt = _trainer(cfg, cuda)
            assert trainer.network.train_background == "white"
            b = dict(batch)
            if mode == "white+bg":
                b["bg"] = bg.to(cuda)[None]
            out, loss, stats = trainer.train_step(b, opt)
            torch.cuda.synchronize()
        finally:
            if node is not None:
                ta[KEY] = node
        assert set(stats) == {"loss_f", "total_loss"} and "bg" not in out
        runs.append((float(loss.detach()), out["rgb_map_f"].detach().clone(),
                     [p.detach().clone() for p in net.parameters()]))
    for other in runs[1:]:
        assert other[0] == runs[0][0] and torch.equal(other[1], runs[0][1])
        for p, q in zip(other[2], runs[0][2]):
            assert torch.equal(p, q)
    # the key on: the colours reach the compositor, the step moves the fine net, a batch without colours is an error
    ta[KEY] = "random"
    net, trainer, opt = _trainer(cfg, cuda)
    assert trainer.network.train_background == "random"
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    out, loss, stats = trainer.train_step(dict(batch, bg=bg.to(cuda)[None]), opt)
    torch.cuda.synchronize()
    assert set(stats) == {"loss_f", "total_loss"} and bool(torch.isfinite(loss))
    assert not torch.equal(out["rgb_map_f"].detach(), runs[0][1]) and float(loss.detach()) != runs[0][0]
    moved = 0
    for k, p in net.named_parameters():
        if k.startswith("model."):
            assert torch.equal(p.detach(), before[k]), k
        else:
            moved += int(not torch.equal(p.detach(), before[k]))
    assert moved > 0
    with pytest.raises(ValueError, match="batch\\['bg'\\]"):
        trainer.train_step(dict(batch), opt)
    # with a point budget, jitter and the distortion term at once
    ta.point_budget = {"target": 8192, "max_points": 4096}
    ta.train_march_jitter = True
    ta.distortion_loss_weight = 0.01
    net_b, budgeted, opt_b = _trainer(cfg, cuda)
    out_b, loss_b, stats_b = budgeted.train_step(dict(batch, bg=bg.to(cuda)[None]), opt_b)
    assert set(stats_b) == {"loss_f", "loss_dist", "total_loss", "rays", "points"} and bool(torch.isfinite(loss_b))
    assert 0 < out_b["rays_kept"] < 256 and "t_shift" in out_b
    ta.point_budget = {"target": 0}
    ta.train_march_jitter = False
    ta.distortion_loss_weight = 0.0
    # validation: under no_grad the configured (white) background, whatever the key and the batch say
    from src.models.nerf.renderer.volume_renderer import Renderer
    net = _trained_net(cuda)
    r = Renderer(net)
    r.set_occupancy_grid(trained_grid, cuda)
    with torch.no_grad():
        inf = r.render_accelerated(_batch(g2["march_rays"], cuda, bg=bg))
        ref = ops.march(net.model_fine.packer(), torch.from_numpy(g2["march_rays"]).to(cuda), 2.0, 6.0,
                        r.occupancy_grid, step_size=float(ta.render_step_size),
                        t_thresh=float(ta.transmittance_threshold), bbox=r._bbox_tuple(),
                        white_bkgd=bool(ta.white_bkgd), dtype=net.mlp_dtype)
        val, _, vstats = trainer.network(dict(batch))  # (no colours needed without grad)
    assert bool(ta.white_bkgd) and inf["n_queried"] == ref["n_queried"]
    for m in MAPS:
        assert torch.equal(inf[m], ref[m]), m
    assert "rgb_map_c" in val and set(vstats) == {"loss_c", "loss_f", "total_loss"}


# --------------------------------------------------------------------------------------
# 7. it trains
# --------------------------------------------------------------------------------------
def test_it_trains_on_random_backgrounds(cuda, bg_cfg, g2, trained_grid, tmp_path, monkeypatch):
    """test_it_trains_with_jitter's procedure with this key on: rgb_linear.bias + 1, 256 rays, 12 steps (lr 5e-4,
    clip 40); the ground truth is the unperturbed net's own no-grad march without a background, composited here
    onto the colours the batch carries."""
    from nerf_amd import ops
    from src.models.nerf.renderer.volume_renderer import Renderer
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    cfg = bg_cfg
    ta = cfg.task_arg
    _write_grid(tmp_path, monkeypatch, trained_grid)
    ta.train_renderer = "accelerated"
    ta.train_grid = "file"
    ta[KEY] = "random"
    assert float(cfg.train.lr) == 5e-4
    net = _trained_net(cuda)
    rays = torch.from_numpy(g2["march_rays"]).to(cuda)
    bg = torch.rand(256, 3, generator=torch.Generator().manual_seed(2)).to(cuda)
    r = Renderer(net)
    r.set_occupancy_grid(trained_grid, cuda)
    with torch.no_grad():
        clean = ops.march(net.model_fine.packer(), rays, 2.0, 6.0, r.occupancy_grid,
                          step_size=float(ta.render_step_size), t_thresh=float(ta.transmittance_threshold),
                          bbox=r._bbox_tuple(), white_bkgd=False, dtype=net.mlp_dtype)
        gt = clean["rgb_map_f"] + (1.0 - clean["acc_map_f"])[:, None] * bg
        assert 0.05 < float((1.0 - clean["acc_map_f"]).mean()) < 0.95  # the colours show through on part of the rays
        net.model_fine.rgb_linear.bias += 1.0
    trainer = make_trainer(cfg, net)
    assert trainer.clip_value == 40.0
    opt = make_optimizer(cfg, net)
    batch = _batch(rays, cuda, gt, bg)
    losses = []
    for _ in range(12):
        out, loss, _ = trainer.train_step(dict(batch), opt)
        losses.append(float(loss.detach()))
    print("\nlosses:", " ".join(f"{v:.6f}" for v in losses))
    assert losses[11] < 0.25 * losses[0], losses
