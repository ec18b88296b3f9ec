"""The online occupancy grid on the GPU (task_arg.train_grid "online"): the three update kernels
against NumPy restatements, the OnlineGrid's composition and cadence, render quality against the
baked grid, the training step against the file-mode step, a from-scratch run, save and load.
"""
import os

import numpy as np
import pytest
import torch

from march_support import _batch, fp32_cfg, g2

pytestmark = pytest.mark.gpu

os.environ.setdefault("NERF_AMD_NO_ARGV", "1")
HERE = os.path.dirname(os.path.abspath(__file__))
LEGO = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
SKEW = ((-1.3, -0.4, 0.1), (0.7, 1.9, 2.3))
BBOXES = {"lego": LEGO, "skew": SKEW}
RES = [2, 8, 33, 128]


@pytest.fixture(scope="module")
def baked_grid(g2):
    return torch.from_numpy(np.unpackbits(g2["bake128_packed"])[: 128 ** 3].reshape(128, 128, 128).astype(bool))


def _trained_state():
    z = np.load(os.path.join(HERE, "golden", "trained_v2.npz"), allow_pickle=False)
    return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.fixture()
def online_cfg():
    """cfg with the keys the tests below set restored afterwards."""
    yield from fp32_cfg(("train_renderer", "train_grid", "grid_update", "mlp_dtype", "perturb", "train_rays",
                         "occupancy_grid_res", "occupancy_grid_threshold", "chunk_size"))


def _net(cuda, state=None):
    from src.models.nerf.network import Network
    torch.manual_seed(0)
    net = Network()
    if state is not None:
        net.load_state_dict(state, strict=True)
    return net.to(cuda)


@pytest.fixture()
def trained(cuda, online_cfg):
    return online_cfg, _net(cuda, _trained_state())


def _cell_ijk(cells, res):
    c = cells.long()
    return torch.stack([c // (res * res), (c // res) % res, c % res], 1)


# --------------------------------------------------------------------------------------
# 1. points
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("bbox", sorted(BBOXES))
@pytest.mark.parametrize("res", RES)
def test_points_full_visit(cuda, res, bbox):
    from nerf_amd import ops
    bb = BBOXES[bbox]
    C = res ** 3
    cells, pts = ops.grid_update_points(res, bb, 0, C, update=3, seed=5, device=cuda)
    assert cells.dtype == torch.int32 and cells.shape == (C,) and pts.shape == (C, 3)
    # every cell exactly once
    assert torch.equal(cells.long().sort().values, torch.arange(C, device=cuda))
    # the march's own lookup puts EVERY point in its cell
    ijk = _cell_ijk(cells, res)
    idx, _ = ops.grid_index(pts, None, res, bb)
    assert torch.equal(idx, ijk)
    # inside the bbox; the last index of an axis sits on the face
    mn, mx = (torch.tensor(v, device=cuda) for v in bb)
    assert bool((pts >= mn).all()) and bool((pts <= mx).all())
    face = ijk == res - 1
    assert torch.equal(pts[face], mx.expand(C, 3)[face])
    # the same (seed, update) twice: the same bits
    cells2, pts2 = ops.grid_update_points(res, bb, 0, C, update=3, seed=5, device=cuda)
    assert torch.equal(cells, cells2) and torch.equal(pts, pts2)
    # another update index, or another seed, moves the points and not the cells
    for kw in (dict(update=4, seed=5), dict(update=3, seed=6)):
        cells3, pts3 = ops.grid_update_points(res, bb, 0, C, device=cuda, **kw)
        assert torch.equal(cells, cells3)
        moved = (pts3 != pts)[~face]
        assert float(moved.float().mean()) > 0.99, kw
    # a range of slots is that range of the full visit (the draw is counted by the slot)
    s0, n = C // 3, max(1, C // 5)
    cells4, pts4 = ops.grid_update_points(res, bb, s0, n, update=3, seed=5, device=cuda)
    assert torch.equal(cells4, cells[s0:s0 + n]) and torch.equal(pts4, pts[s0:s0 + n])
    if res == 128:
        # the centre fall-back is the exception (the plain formula misses its cell on < 0.01 % of the
        # coordinates): fewer than 1 % of the points sit at their cell's centre on all three axes
        # (the centre in NumPy float32, IEEE operation by operation as the kernel computes it)
        lo, hi = (np.asarray(v, np.float32) for v in bb)
        i32 = ijk.cpu().numpy().astype(np.float32)
        centre = lo + ((i32 + np.float32(0.5)) / np.float32(res - 1)) * (hi - lo)
        assert centre.dtype == np.float32
        at_centre = int((pts.cpu().numpy() == centre).all(1).sum())
        ext = mx - mn
        print(f"\nres {res} {bbox}: {at_centre} of {C} points at the centre on all three axes")
        assert at_centre < 0.01 * C
        # and the jitter is a uniform draw over the cell: the mean offset of 6e6 draws is 0.5 +- 1.2e-4 (1 sigma)
        u = ((pts - mn) / ext * float(res - 1) - ijk.float())[~face]
        assert abs(float(u.double().mean()) - 0.5) < 0.01


def test_consecutive_slots_land_far_apart(cuda):
    """A ~ 0.618 res^3: neighbouring slots are ~0.6 of the grid apart along x, not neighbouring cells."""
    from nerf_amd import ops
    res = 128
    cells, _ = ops.grid_update_points(res, LEGO, 0, 4096, update=0, device=cuda)
    ix = _cell_ijk(cells, res)[:, 0]
    assert float((ix[1:] - ix[:-1]).abs().float().mean()) > res / 4


# --------------------------------------------------------------------------------------
# 2. rolling coverage
# --------------------------------------------------------------------------------------
def test_rolling_updates_cover_every_cell_once(cuda):
    from src.models.nerf.renderer.online_grid import OnlineGrid
    g = OnlineGrid(33, 1.0, LEGO, cuda, warmup_updates=2, period=4)
    C = 33 ** 3
    for k in range(2):
        assert g.slots(k) == (0, C)
    for first in (2, 5):
        cells = torch.cat([g.points(k)[0] for k in range(first, first + 4)])
        assert cells.numel() == C
        assert torch.equal(cells.long().sort().values, torch.arange(C, device=cuda))


# --------------------------------------------------------------------------------------
# 3. apply
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,s0,n", [(33, 777, 10001), (2, 0, 8), (128, 0, 128 ** 3)])
def test_apply_against_numpy(cuda, res, s0, n):
    from nerf_amd import ops
    C = res ** 3
    g = torch.Generator().manual_seed(res)
    density = torch.rand(res, res, res, generator=g) * 3.0
    density[torch.rand(res, res, res, generator=g) < 0.3] = 0.0
    raw = torch.randn(n, 4, generator=g) * 3.0  # about half of raw[:, 3] negative
    raw[0, 3] = -7.0
    cells, _ = ops.grid_update_points(res, LEGO, s0, n, update=0, device=cuda)
    d_gpu = density.to(cuda)
    out = ops.grid_update_apply(d_gpu, cells, raw.to(cuda), 0.95)
    assert out is d_gpu
    c = cells.cpu().numpy()
    d = density.numpy().reshape(-1)
    want = d.copy()
    want[c] = np.maximum((d[c] * np.float32(0.95)).astype(np.float32), np.maximum(raw.numpy()[:, 3], np.float32(0)))
    got = d_gpu.cpu().numpy().reshape(-1)
    np.testing.assert_array_equal(got, want)
    untouched = np.ones(C, bool)
    untouched[c] = False
    assert untouched.sum() == C - n
    assert got[untouched].tobytes() == d[untouched].tobytes()
    assert (want[c] >= 0).all() and float(want[c[0]]) == float(np.float32(d[c[0]] * np.float32(0.95)))


# --------------------------------------------------------------------------------------
# 4. threshold
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,branch", [(1.0, "mean"), (4.0, "threshold")])
@pytest.mark.parametrize("res", [33, 128])
def test_threshold(cuda, res, scale, branch):
    from nerf_amd import ops
    thr = 1.0
    g = torch.Generator().manual_seed(100 + res)
    density = torch.rand(res, res, res, generator=g) * scale
    density[torch.rand(res, res, res, generator=g) < 0.2] = 0.0
    mean64 = float(density.double().mean())
    assert (mean64 < thr) == (branch == "mean")
    d = density.to(cuda)
    runs = []
    for _ in range(2):
        grid = torch.full((res, res, res), 7, dtype=torch.uint8, device=cuda)
        stats = ops.grid_update_threshold(d, grid, thr)
        runs.append((grid, stats.clone()))
    grid, stats = runs[0]
    mean, count = ops.grid_update_stats(stats)
    print(f"\nres {res} {branch}: mean {mean!r} fp64 {mean64!r} occupied {count}")
    assert abs(mean - mean64) <= 1e-6 * mean64
    cut = min(np.float32(thr), np.float32(mean))
    assert float(stats.cpu()[1:2].view(torch.float32)[0]) == float(cut)
    assert (float(cut) == thr) == (branch == "threshold")
    want = density.numpy() > cut
    np.testing.assert_array_equal(grid.cpu().numpy(), want.astype(np.uint8))
    assert count == int(grid.sum()) == int(want.sum()) and 0 < count < res ** 3
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(d.cpu(), density)  # the density is read only


# --------------------------------------------------------------------------------------
# 5. composition: one full update == its parts
# --------------------------------------------------------------------------------------
def test_update_equals_its_parts(cuda, trained):
    from nerf_amd import ops
    from src.models.nerf.renderer.online_grid import OnlineGrid
    cfg, net = trained
    packer = net.model_fine.packer()
    res, thr = 128, 1.0
    g = OnlineGrid(res, thr, LEGO, cuda, seed=4)
    cells, pts = g.points()
    assert cells.numel() == res ** 3
    with torch.no_grad():
        raw = ops.mlp(packer, pts, None, 1, None, "fp32", density_only=True)
    sigma = raw[:, 3].clamp_min(0).cpu().numpy()
    want = np.zeros(res ** 3, np.float32)
    want[cells.cpu().numpy()] = np.maximum(np.float32(0) * np.float32(g.decay), sigma)
    g.update(packer, "fp32")
    assert g.updates == 1 and g.last_points == res ** 3
    np.testing.assert_array_equal(g.density.cpu().numpy().reshape(-1), want)
    mean, count = ops.grid_update_stats(g.stats)
    assert abs(mean - float(want.astype(np.float64).mean())) <= 1e-6 * mean
    occ = want > min(np.float32(thr), np.float32(mean))
    np.testing.assert_array_equal(g.grid.cpu().numpy().reshape(-1), occ.astype(np.uint8))
    assert count == int(occ.sum())
    m, frac = g.summary()
    assert m == mean and frac == count / res ** 3 and 0.0 < frac < 1.0


# --------------------------------------------------------------------------------------
# 6. render quality: the online grid against the baked one, both against the all-ones grid
# --------------------------------------------------------------------------------------
def test_render_quality_against_the_baked_grid(cuda, trained, g2, baked_grid):
    """max|rgb - rgb_all_ones| over golden_v2's 256 march_rays on the trained fixture net, fp32: the online grid
    after its 16 warm-up updates may be off by at most twice what the baked grid (the reference's method: any of
    a voxel's eight corners) is, floored at the 1e-4 contract; the factor 2 is for one jittered sample per cell
    against eight corners.  Measured on an MI355X: baked 3.504e-2, online 3.730e-2; points queried 123,219
    (all ones), 13,382 (baked, 158,188 cells occupied), 10,623 (online, 130,846 cells)."""
    from nerf_amd import ops
    from src.models.nerf.renderer.online_grid import OnlineGrid
    cfg, net = trained
    packer = net.model_fine.packer()
    rays = torch.from_numpy(g2["march_rays"]).to(cuda)
    t_table = torch.from_numpy(g2["march_t_table"]).to(cuda)
    g = OnlineGrid(128, float(cfg.task_arg.occupancy_grid_threshold), LEGO, cuda)  # the default schedule
    assert g.warmup_updates == 16
    for _ in range(g.warmup_updates):
        g.update(packer, "fp32")
    assert g.updates == g.warmup_updates and g.slots() != (0, 128 ** 3)
    grids = {"ones": torch.ones(128, 128, 128, dtype=torch.bool), "baked": baked_grid, "online": g.grid}
    out = {k: ops.march(packer, rays, 2.0, 6.0, v, t_table=t_table, dtype="fp32") for k, v in grids.items()}
    err = {k: float((out[k]["rgb_map_f"] - out["ones"]["rgb_map_f"]).abs().max()) for k in ("baked", "online")}
    print(f"\nmax|rgb - rgb_all_ones|: baked {err['baked']:.3e} online {err['online']:.3e}; n_queried: ones "
          f"{out['ones']['n_queried']} baked {out['baked']['n_queried']} online {out['online']['n_queried']}; "
          f"occupied: baked {int(baked_grid.sum())} online {int(g.grid.sum())}")
    assert out["online"]["n_queried"] < out["ones"]["n_queried"]
    assert err["online"] <= max(2.0 * err["baked"], 1e-4), err


# --------------------------------------------------------------------------------------
# 7. a step at which no update fires == the file-mode step given that grid
# --------------------------------------------------------------------------------------
def test_step_equals_the_file_mode_step(cuda, trained, g2, tmp_path, monkeypatch):
    from nerf_amd import ops
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    from src.train.trainers.nerf import occupancy_grid_path
    cfg, net = trained
    monkeypatch.chdir(tmp_path)
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(1))
    batch = _batch(g2["march_rays"], cuda, gt, device_scalar=True)
    cfg.task_arg.train_renderer = "accelerated"
    cfg.task_arg.train_grid = "online"
    online = make_trainer(cfg, net)
    grid = online.network.online_grid
    opt = make_optimizer(cfg, net)
    online.forward_backward(dict(batch), opt)  # the grid's step 0: update 0, then the march (weights unchanged)
    assert (grid.updates, grid.steps) == (1, 1) and grid.device == cuda
    assert online.network.renderer.occupancy_grid is grid.grid  # handed over as it is
    snap = opt.flat_param.clone()
    _, loss_on, stats_on = online.train_step(dict(batch), opt)  # step 1: no update fires
    assert (grid.updates, grid.steps) == (1, 2)
    grad_on = opt.flat_grad.clone()
    after_on = opt.flat_param.clone()
    assert set(stats_on) == {"loss_f", "total_loss"} and float(grad_on.abs().max()) > 0
    online.network.save_grid(str(tmp_path / "model"))
    # the same weights and fresh moments, the file-mode step on the grid the online trainer wrote
    with torch.no_grad():
        opt.flat_param.copy_(snap)
        opt.flat_m.zero_()
        opt.flat_v.zero_()
    opt._step = 0
    ops.params_updated()
    cfg.task_arg.train_grid = "file"
    filed = make_trainer(cfg, net)
    assert filed.network.online_grid is None and os.path.exists(occupancy_grid_path())
    assert filed.network.renderer.occupancy_grid.dtype == torch.bool
    assert torch.equal(filed.network.renderer.occupancy_grid, grid.grid.bool())
    _, loss_file, _ = filed.train_step(dict(batch), opt)
    assert float(loss_file.detach()) == float(loss_on.detach())
    assert torch.equal(opt.flat_grad, grad_on)
    assert torch.equal(opt.flat_param, after_on)
    # validation in online mode goes through the march with the live grid (and does not count as a step)
    with torch.no_grad():
        ret, _, vstats = online.network(dict(batch))
    assert set(vstats) == {"loss_f", "total_loss"} and "rgb_map_c" not in ret and "n_queried" in ret
    assert (grid.updates, grid.steps) == (1, 2)


# --------------------------------------------------------------------------------------
# 8. from scratch
# --------------------------------------------------------------------------------------
SCRATCH_STEPS = 480  # 30 x interval


def test_from_scratch(cuda, online_cfg):
    """Seed-0 init, the procedural scene, 1024 rays a step, fp32, the default schedule: the grid prunes
    without collapsing (an over-pruned grid renders the all-white image) and the net learns through it -- the
    held-out PSNR, rendered through the march with the live grid, beats the all-white image's by more than 3 dB
    (the bar of test_gpu_training.py).  Measured on an MI355X after 480 steps (6.6 s): 13.0 % of the cells
    occupied, 21.29 dB against 8.16 dB; mean loss per 16 steps 0.114 -> 0.0081."""
    from nerf_amd import ops
    from src.datasets.nerf.blender import Dataset
    from src.datasets.nerf.synthetic import camera_rays, make_scene, psnr, shade, view_poses
    from src.models import make_network
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    from src.utils.camera import focal_for
    cfg = online_cfg
    ta = cfg.task_arg
    ta.train_rays = 1024
    ta.train_renderer = "accelerated"
    ta.train_grid = "online"
    imgs, poses, focal = make_scene(100, 100, 100, cuda, seed=0)
    ds = Dataset.from_arrays(imgs, poses, focal)
    torch.manual_seed(0)
    net = make_network(cfg).to(cuda)
    trainer = make_trainer(cfg, net)
    grid = trainer.network.online_grid
    interval = grid.interval
    assert SCRATCH_STEPS % interval == 0 and interval == 16
    opt = make_optimizer(cfg, net)
    losses = []
    for _ in range(SCRATCH_STEPS):
        rays, rgbs = ds.sample_batch()
        _, loss, _ = trainer.train_step({"rays": rays[None], "rgbs": rgbs[None], "near": ops.device_scalar(2.0, cuda),
                                         "far": ops.device_scalar(6.0, cuda)}, opt)
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu().numpy()
    assert (grid.steps, grid.updates) == (SCRATCH_STEPS, SCRATCH_STEPS // interval)
    _, frac = grid.summary()
    ev = view_poses(2, seed=1).to(cuda)
    ps, white = [], []
    with torch.no_grad():
        for k in range(ev.shape[0]):
            o, d = camera_rays(ev[k], 100, 100, focal_for(100))
            gt = shade(o, d)
            ret, _, _ = trainer.network({"rays": torch.cat([o, d], -1), "rgbs": gt, "near": ops.device_scalar(2.0, cuda),
                                         "far": ops.device_scalar(6.0, cuda)})
            ps.append(psnr(ret["rgb_map_f"], gt))
            white.append(psnr(torch.ones_like(gt), gt))
    curve = [float(losses[i:i + interval].mean()) for i in range(0, SCRATCH_STEPS, interval)]
    print(f"\nfrom scratch, {SCRATCH_STEPS} steps: occupied {frac:.4f}; held-out PSNR {np.mean(ps):.2f} dB, all-white "
          f"{np.mean(white):.2f} dB; mean loss per {interval} steps: " + " ".join(f"{v:.4f}" for v in curve))
    assert 0.0 < frac < 1.0
    assert curve[-1] < curve[0]
    assert np.mean(ps) > np.mean(white) + 3.0


# --------------------------------------------------------------------------------------
# 9. save and load
# --------------------------------------------------------------------------------------
def test_save_and_load(cuda, trained, g2, tmp_path, monkeypatch):
    from src.models.nerf.renderer.volume_renderer import Renderer
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    from src.train.trainers.nerf import GRID_STATE_FILE, occupancy_grid_path
    cfg, net = trained
    monkeypatch.chdir(tmp_path)
    ta = cfg.task_arg
    ta.train_renderer = "accelerated"
    ta.train_grid = "online"
    ta.occupancy_grid_res = 33
    ta.grid_update = {"interval": 2, "warmup_updates": 1, "period": 4}
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(1))
    batch = _batch(g2["march_rays"], cuda, gt, device_scalar=True)
    a = make_trainer(cfg, net)
    opt = make_optimizer(cfg, net)
    for _ in range(3):  # updates at the grid's steps 0 (full) and 2 (rolling)
        a.train_step(dict(batch), opt)
    ga = a.network.online_grid
    assert (ga.res, ga.updates, ga.steps) == (33, 2, 3)
    model_dir = str(tmp_path / "trained_model")
    a.network.save_grid(model_dir)
    assert sorted(os.listdir(model_dir)) == [GRID_STATE_FILE]
    b = make_trainer(cfg, net)  # fresh objects
    gb = b.network.online_grid
    assert gb is not ga and gb.updates == 0
    assert b.network.load_grid(model_dir) is True
    assert (gb.updates, gb.steps) == (2, 3)
    assert torch.equal(gb.density.cpu(), ga.density.cpu()) and torch.equal(gb.grid.cpu(), ga.grid.cpu())
    # one further update from equal weights: equal grids, bit for bit
    packer = net.model_fine.packer()
    ga.update(packer, "fp32")
    gb.to(cuda).update(packer, "fp32")
    assert gb.updates == ga.updates == 3
    assert torch.equal(gb.density, ga.density) and torch.equal(gb.grid, ga.grid)
    assert not torch.equal(gb.density.cpu(), torch.load(os.path.join(model_dir, GRID_STATE_FILE),
                                                        weights_only=True)["density"])  # (it did move)
    # the bool file the trainer wrote loads through the renderer, as run.py evaluate does
    saved = torch.load(occupancy_grid_path(), map_location="cpu", weights_only=True)
    assert saved.dtype == torch.bool and saved.shape == (33, 33, 33)
    r = Renderer(net)
    r.load_occupancy_grid(occupancy_grid_path())
    assert r.occupancy_grid.dtype == torch.bool and r.resolution == 33
    assert torch.equal(r.occupancy_grid.cpu(), saved)
    # a file-mode wrapper has nothing to save or load
    ta.train_grid = "file"
    c = make_trainer(cfg, net)
    assert c.network.load_grid(model_dir) is False
