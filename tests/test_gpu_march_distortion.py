"""The distortion loss of the training march on the GPU (task_arg.distortion_loss_weight).

The DIST instantiations of the segment compositing kernels (nerf_march_seg_composite_fwd_dist /
_bwd_dist) return, next to rgb / depth / acc, the distortion of each ray's weights

    dist_r = inv_range * ( sum_i sum_j w_i w_j |t_i - t_j|  +  (step_size / 3) * sum_i w_i^2 ).

Checked here: value and gradient against the O(n^2) definition in fp64 (segments that cross the
backward's 64-chunk register window included), known values, that nothing else moves, the per-ray shift,
ops.march_grad(distortion=True) end to end on the trained fixture net, and the training step.
"""
import os

import numpy as np
import pytest
import torch

from march_support import (ALPHA_ONE, INV_RANGE, LONG, MAPS, STEP, _dist_double_sum, _dist_prefix, _flat_grad,
                           _march_grad, _per_segment_bound, _trained_net, _write_grid, fp32_cfg, g2,
                           long_segment_case, trained_grid)

pytestmark = pytest.mark.gpu

os.environ.setdefault("NERF_AMD_NO_ARGV", "1")


# --------------------------------------------------------------------------------------
# 1. against the definition in fp64
# --------------------------------------------------------------------------------------
def _segment_reference(c, white):
    """fp64 on the CPU, out of place: the compositor of test_gpu_march_grad's reference, and the distortion by
    its O(n^2) definition -- by the prefix-sum form on the two long segments, after that form has been shown
    equal to the definition (value and gradient, 1e-12 relative) on every shorter one."""
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
        t = c["t_table"][st.clamp(min=0)].double()
        a = w.sum()
        rgb.append((w[:, None] * col).sum(0) + ((1.0 - a) if white else 0.0))
        depth.append((w * t).sum())
        acc.append(a)
        if r in LONG:
            dist.append(_dist_prefix(w, t))
            continue
        dist.append(_dist_double_sum(w, t))
        if white or off[r + 1] - off[r] < 2:
            continue
        # the prefix-sum form against the definition, value and gradient w.r.t. the weights (of the points that
        # have a depth: a surplus point's weight is the constant 0)
        wl = w.detach().clone().requires_grad_(True)
        v2, vp = _dist_double_sum(wl, t), _dist_prefix(wl, t)
        (g2,), (gp,) = torch.autograd.grad(v2, wl), torch.autograd.grad(vp, wl)
        v2, vp, keep = v2.detach(), vp.detach(), st >= 0
        assert abs(float(v2 - vp)) <= 1e-12 * abs(float(v2)), (r, float(v2), float(vp))
        assert float((g2 - gp)[keep].abs().max()) <= 1e-12 * float(g2[keep].abs().max()), r
    rgb, depth, acc, dist = torch.stack(rgb), torch.stack(depth), torch.stack(acc), torch.stack(dist)
    g_rgb, g_depth, g_acc, g_dist = (x.double() for x in c["cot"])
    (g_only,) = torch.autograd.grad((dist * g_dist).sum(), raw, retain_graph=True)
    (g_three,) = torch.autograd.grad((rgb * g_rgb).sum() + (depth * g_depth).sum() + (acc * g_acc).sum(), raw,
                                     retain_graph=True)
    return dict(rgb=rgb.detach(), depth=depth.detach(), acc=acc.detach(), dist=dist.detach(), g_only=g_only,
                g_three=g_three, g_all=g_only + g_three)


@pytest.fixture(scope="module")
def segment_case():
    c = long_segment_case()
    c["ref"] = {white: _segment_reference(c, white) for white in (False, True)}  # computed once, shared
    return c


def _apply(c, cuda, white, dist=True, t_shift=None, t_table=None):
    from nerf_amd import ops
    raw = c["raw"].to(cuda).requires_grad_(True)
    args = [raw, c["rays"].to(cuda), (c["t_table"] if t_table is None else t_table).to(cuda), c["seg_off"].to(cuda),
            c["out_step"].to(cuda), STEP, white]
    if dist:
        args += [t_shift, INV_RANGE]
    elif t_shift is not None:
        args += [t_shift]
    return raw, ops._MarchSegComposite.apply(*args)


@pytest.mark.parametrize("white", [False, True])
def test_distortion_kernels_against_fp64(cuda, segment_case, white):
    c, ref = segment_case, segment_case["ref"][white]
    raw, (rgb, depth, acc, dist) = _apply(c, cuda, white)
    cot = [x.to(cuda) for x in c["cot"]]
    (g_only,) = torch.autograd.grad([dist], [raw], [cot[3]], retain_graph=True)
    (g_all,) = torch.autograd.grad([rgb, depth, acc, dist], [raw], cot)
    d, rd = dist.detach().cpu().double(), ref["dist"]
    rel = ((d - rd).abs() / rd.abs().clamp(min=1e-300)).max()
    print(f"\nwhite {white}: dist in [{float(rd.min()):.3e}, {float(rd.max()):.3e}], max rel err {float(rel):.3e}")
    assert bool((rd[[i for i in range(c['N']) if i % 2 == 0 and c['lens'][i] > 60]] > 1e-4).all())  # not negligible
    assert bool(((d - rd).abs() <= 1e-4 * rd.abs() + 1e-12).all()), ((d - rd).abs() / rd.abs().clamp(min=1e-30))
    assert bool(torch.isfinite(g_only).all()) and bool(torch.isfinite(g_all).all())
    w_only = _per_segment_bound(c, g_only.cpu(), ref["g_only"], "dist alone")
    w_all = _per_segment_bound(c, g_all.cpu(), ref["g_all"], "all four")
    print(f"g_raw worst error / segment's largest: dist alone {w_only:.3e}, all four outputs {w_all:.3e}")
    # the three maps and their gradient, the two long segments included: the bounds of test_segment_kernels_against_fp64
    np.testing.assert_allclose(rgb.detach().cpu().numpy(), ref["rgb"].numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(acc.detach().cpu().numpy(), ref["acc"].numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(depth.detach().cpu().numpy(), ref["depth"].numpy(), rtol=0, atol=5e-5)
    raw3, maps3 = _apply(c, cuda, white, dist=False)
    (g_three,) = torch.autograd.grad(list(maps3), [raw3], cot[:3])
    np.testing.assert_allclose(g_three.cpu().numpy(), ref["g_three"].numpy(), rtol=1e-4, atol=1e-5)
    # exact zeros: after an alpha == 1 point, on surplus points, on an empty segment
    off = c["seg_off"].tolist()
    for g in (g_only.cpu(), g_all.cpu()):
        for seg, pos in ALPHA_ONE:
            tail = g[off[seg] + pos + 1:off[seg + 1]]
            assert tail.numel() > 0 and bool((tail == 0).all()), seg
        assert bool((g[c["out_step"] < 0] == 0).all())
    assert c["lens"][0] == 0 and float(dist[0].detach()) == 0.0


# --------------------------------------------------------------------------------------
# 2. known values
# --------------------------------------------------------------------------------------
def test_known_values(cuda):
    from nerf_amd import ops
    # ray 0: one point at alpha exactly 1 (w = 1: dist = inv_range * step / 3); ray 1: empty; ray 2: an alpha == 1
    # point in the middle and a surplus tail
    seg_off = torch.tensor([0, 1, 1, 7], dtype=torch.int32, device=cuda)
    out_step = torch.tensor([17, 3, 9, 20, 31, 40, -1], dtype=torch.int32, device=cuda)
    raw = torch.tensor([[0.3, -0.2, 0.1, 1e4]] + [[0.1, 0.2, 0.3, s] for s in (30.0, 50.0, 1e4, 60.0, 70.0, 80.0)],
                       device=cuda).requires_grad_(True)
    rays = torch.tensor([[0.0, 0.0, 4.0, 0.0, 0.0, -1.0]] * 3, device=cuda)
    t_table = torch.arange(2.0, 6.0, 0.005).to(cuda)
    rgb, depth, acc, dist = ops._MarchSegComposite.apply(raw, rays, t_table, seg_off, out_step, STEP, True, None,
                                                         INV_RANGE)
    want = np.float32(np.float64(np.float32(INV_RANGE)) * np.float64(np.float32(STEP)) / 3.0)
    assert float(acc[0]) == 1.0
    assert abs(float(dist[0]) - float(want)) <= float(np.spacing(want)), (float(dist[0]), float(want))
    assert float(dist[1]) == 0.0 and float(dist[2]) > 0.0
    (g,) = torch.autograd.grad(dist.sum(), raw)
    g = g.cpu()
    assert bool(torch.isfinite(g).all())
    assert float(g[1:3, 3].abs().min()) > 0      # before the alpha == 1 point: a gradient
    assert bool((g[4:] == 0).all())              # after it, and on the surplus point: exactly 0
    # no segment at all: dist is 0 and nothing is differentiated
    raw0 = torch.zeros(0, 4, device=cuda, requires_grad=True)
    out0 = ops._MarchSegComposite.apply(raw0, rays, t_table, torch.zeros(4, dtype=torch.int32, device=cuda),
                                        out_step[:0], STEP, True, None, INV_RANGE)
    assert bool((out0[3] == 0).all()) and bool((out0[2] == 0).all())
    (g0,) = torch.autograd.grad(out0[3].sum(), raw0)
    assert g0.shape == (0, 4)


# --------------------------------------------------------------------------------------
# 3. nothing else moves
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [False, True])
def test_the_other_maps_and_launches_are_unchanged(cuda, segment_case, white):
    from nerf_amd import ops
    c = segment_case
    cot = [x.to(cuda) for x in c["cot"]]
    kt = ops.KERNEL_TIMES
    old = (kt.enabled, kt.detail)
    kt.enabled = kt.detail = True
    try:
        kt.reset()
        raw3, maps3 = _apply(c, cuda, white, dist=False)
        (g3,) = torch.autograd.grad(list(maps3), [raw3], cot[:3])
        names3 = [p[0] for p in kt.pending]
        kt.reset()
        raw4, maps4 = _apply(c, cuda, white)
        (g4,) = torch.autograd.grad(list(maps4[:3]), [raw4], cot[:3])  # no cotangent on dist
        names4 = [p[0] for p in kt.pending]
        units = {p[0]: p[1] for p in kt.pending}
    finally:
        kt.enabled, kt.detail = old
        kt.reset()
    assert len(maps3) == 3 and names3 == ["march_seg_composite_fwd", "march_seg_composite_bwd"]
    assert len(maps4) == 4 and names4 == ["march_seg_composite_fwd_dist", "march_seg_composite_bwd_dist"]
    M, N = c["raw"].shape[0], c["N"]
    assert units == {"march_seg_composite_fwd_dist": 20 * M + 68 * N, "march_seg_composite_bwd_dist": 56 * M + 68 * N}
    for a, b in zip(maps3, maps4):
        assert torch.equal(a, b)
    assert float(g3.abs().max()) > 0 and torch.equal(g3, g4)


# --------------------------------------------------------------------------------------
# 4. the per-ray shift
# --------------------------------------------------------------------------------------
def test_a_constant_shift_is_the_shifted_table(cuda, segment_case):
    c = segment_case
    shift = torch.full((c["N"],), 0.0037)
    cot = [x.to(cuda) for x in c["cot"]]
    raw_s, maps_s = _apply(c, cuda, True, t_shift=shift.to(cuda))
    raw_t, maps_t = _apply(c, cuda, True, t_table=c["t_table"] + shift[0])  # (rounded entry by entry, as the kernel adds)
    raw_0, maps_0 = _apply(c, cuda, True)
    for a, b in zip(maps_s, maps_t):
        assert torch.equal(a, b)
    assert not torch.equal(maps_s[1], maps_0[1])  # (the shift does reach the kernel)
    (g_s,) = torch.autograd.grad(list(maps_s), [raw_s], cot)
    (g_t,) = torch.autograd.grad(list(maps_t), [raw_t], cot)
    assert float(g_s.abs().max()) > 0 and torch.equal(g_s, g_t)


# --------------------------------------------------------------------------------------
# 5. end to end: ops.march_grad(distortion=True) on the trained fixture net and its own bake
# --------------------------------------------------------------------------------------
@pytest.fixture()
def dist_cfg():
    """cfg with the keys the tests below set restored afterwards."""
    yield from fp32_cfg(("train_renderer", "train_grid", "point_budget", "mlp_dtype", "perturb", "chunk_size",
                         "train_rays", "distortion_loss_weight"))


@pytest.fixture()
def fixture_net(cuda, dist_cfg, g2, trained_grid):
    """The trained fixture net, its optimizer (the flat gradient), the 256 march rays, a ground truth."""
    from src.train.optimizer import make_optimizer
    net = _trained_net(cuda)
    opt = make_optimizer(dist_cfg, net)
    rays = torch.from_numpy(g2["march_rays"]).to(cuda)
    t_table = torch.from_numpy(g2["march_t_table"]).to(cuda)
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(1)).to(cuda)
    return {"net": net, "opt": opt, "rays": rays, "t_table": t_table, "gt": gt, "grid": trained_grid.to(cuda)}


def test_march_grad_with_the_map(cuda, fixture_net):
    f = fixture_net
    mse = torch.nn.functional.mse_loss
    plain = _march_grad(f, f["rays"])
    assert "dist_map_f" not in plain
    g_mse = _flat_grad(f, mse(plain["rgb_map_f"], f["gt"]))
    out = _march_grad(f, f["rays"], distortion=True)
    d = out["dist_map_f"]
    assert d.shape == (256,) and d.dtype == torch.float32 and d.requires_grad
    assert bool(torch.isfinite(d).all()) and bool((d >= 0).all()) and float(d.max()) > 0
    assert out["n_queried"] == plain["n_queried"] == 13382
    for m in MAPS:
        assert torch.equal(out[m], plain[m]), m
    g_dist = _flat_grad(f, d.mean())
    assert float(g_dist.abs().max()) > 0
    flats = []
    for _ in range(2):
        o = _march_grad(f, f["rays"], distortion=True)
        flats.append(_flat_grad(f, mse(o["rgb_map_f"], f["gt"]) + 0.01 * o["dist_map_f"].mean()))
    assert torch.equal(flats[0], flats[1])  # bit-reproducible
    want = g_mse.double() + 0.01 * g_dist.double()
    err = float((flats[0].double() - want).abs().max())
    print(f"\nmean dist {float(d.mean()):.4e}; |grad| MSE {float(g_mse.abs().max()):.3e}, dist "
          f"{float(g_dist.abs().max()):.3e}; combined against the sum: {err:.3e}")
    assert err <= 1e-4 * float(want.abs().max())


def test_chunks_and_the_point_budget(cuda, fixture_net, trained_grid):
    from src.models.nerf.renderer.volume_renderer import Renderer
    f = fixture_net
    from src.config import cfg
    ta = cfg.task_arg
    r = Renderer(f["net"])
    r.set_occupancy_grid(trained_grid, cuda)
    batch = {"rays": f["rays"][None], "near": torch.tensor([2.0], device=cuda), "far": torch.tensor([6.0], device=cuda)}
    assert "dist_map_f" not in r.render_accelerated(dict(batch))  # weight 0: today's keys
    ta.distortion_loss_weight = 0.01
    whole = r.render_accelerated(dict(batch))
    direct = _march_grad(f, f["rays"], distortion=True, t_table=None)  # (the renderer's own table)
    assert torch.equal(whole["dist_map_f"], direct["dist_map_f"])
    ta.chunk_size = 96  # three chunks
    parts = r.render_accelerated(dict(batch))
    assert parts["dist_map_f"].shape == (256,) and torch.equal(parts["dist_map_f"], whole["dist_map_f"])
    with torch.no_grad():  # a no-grad caller never computes it
        assert "dist_map_f" not in r.render_accelerated(dict(batch))
    capped = _march_grad(f, f["rays"], distortion=True, max_points=6000, t_table=None)
    kept = capped["rays_kept"]
    assert 0 < kept < 256 and capped["dist_map_f"].shape == (256,)
    assert torch.equal(capped["dist_map_f"][:kept], direct["dist_map_f"][:kept])
    assert bool((capped["dist_map_f"][kept:] == 0).all())
    g_dropped = _flat_grad(f, (capped["dist_map_f"][kept:] * 3.0).sum() + 0.0 * capped["dist_map_f"][:kept].sum())
    assert float(g_dropped.abs().max()) == 0.0


# --------------------------------------------------------------------------------------
# 6. the training step
# --------------------------------------------------------------------------------------
def test_training_step_with_the_loss(cuda, dist_cfg, g2, trained_grid, tmp_path, monkeypatch):
    from nerf_amd import ops
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    cfg = dist_cfg
    ta = cfg.task_arg
    net = _trained_net(cuda)
    _write_grid(tmp_path, monkeypatch, trained_grid)
    ta.train_renderer = "accelerated"
    ta.train_grid = "file"
    ta.distortion_loss_weight = 0.01
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(1))
    batch = {"rays": torch.from_numpy(g2["march_rays"]).to(cuda)[None], "near": ops.device_scalar(2.0, cuda),
             "far": ops.device_scalar(6.0, cuda), "rgbs": gt.to(cuda)[None]}
    trainer = make_trainer(cfg, net)
    assert trainer.network.distortion_weight == 0.01
    opt = make_optimizer(cfg, net)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    out, loss, stats = trainer.train_step(dict(batch), opt)
    torch.cuda.synchronize()
    assert set(stats) == {"loss_f", "loss_dist", "total_loss"}
    assert out["dist_map_f"].shape == (256,) and float(stats["loss_dist"]) > 0
    np.testing.assert_allclose(float(stats["loss_dist"]), float(out["dist_map_f"].detach().mean()), rtol=1e-6)
    np.testing.assert_allclose(float(stats["total_loss"]), float(stats["loss_f"]) + 0.01 * float(stats["loss_dist"]),
                               rtol=3e-7)
    assert float(loss.detach()) == float(stats["total_loss"])
    moved = 0
    for k, p in net.named_parameters():
        if k.startswith("model."):  # the coarse net is not evaluated: its bits stay
            assert torch.equal(p.detach(), before[k]), k
        else:
            moved += int(not torch.equal(p.detach(), before[k]))
    assert moved > 0
    with torch.no_grad():  # validation is untouched
        ret, _, vstats = trainer.network(dict(batch))
    assert "dist_map_f" not in ret and set(vstats) == {"loss_c", "loss_f", "total_loss"}
    # with a point budget: the mean over the kept rows, the budget's stats next to it
    ta.point_budget = {"target": 8192, "max_points": 4096}
    budgeted = make_trainer(cfg, net)
    out_b, loss_b, stats_b = budgeted.train_step(dict(batch), opt)
    assert set(stats_b) == {"loss_f", "loss_dist", "total_loss", "rays", "points"}
    k = out_b["rays_kept"]
    assert 0 < k < 256 and bool((out_b["dist_map_f"][k:] == 0).all())
    np.testing.assert_allclose(float(stats_b["loss_dist"]), float(out_b["dist_map_f"][:k].detach().mean()), rtol=1e-6)
    np.testing.assert_allclose(float(stats_b["total_loss"]),
                               float(stats_b["loss_f"]) + 0.01 * float(stats_b["loss_dist"]), rtol=3e-7)
    # the weight 0.0: today's keys
    ta.point_budget = {"target": 0}
    ta.distortion_loss_weight = 0.0
    plain = make_trainer(cfg, net)
    out_p, _, stats_p = plain.train_step(dict(batch), opt)
    assert set(stats_p) == {"loss_f", "total_loss"} and "dist_map_f" not in out_p
