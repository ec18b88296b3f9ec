"""The point budget on the GPU (task_arg.point_budget): nerf_march_budget against NumPy, the capped
differentiable march (ops.march_grad(max_points=)) against the uncapped one bit for bit, the budgeted
training step, a from-scratch run whose ray count follows the pruning grid, save and resume.
"""
import os

import numpy as np
import pytest
import torch

from march_support import (MAPS, _batch, _flat_grad, _loss, _march_grad, _trained_net, _write_grid, fixture_net,
                           fp32_cfg, g2, trained_grid)

pytestmark = pytest.mark.gpu

os.environ.setdefault("NERF_AMD_NO_ARGV", "1")
INT32_MAX = 2 ** 31 - 1


def formula(n_rays, n_queried, target, min_rays=1024, max_rays=32768, granularity=256):
    """The controller's formula, restated."""
    want = max_rays if n_queried == 0 else (target * n_rays) // n_queried
    want = min(max(want, n_rays // 2), 2 * n_rays)
    return min(max((want // granularity) * granularity, min_rays), max_rays)


@pytest.fixture()
def budget_cfg():
    """cfg with the keys the tests below set restored afterwards."""
    yield from fp32_cfg(("train_renderer", "train_grid", "grid_update", "point_budget", "mlp_dtype", "perturb",
                         "train_rays", "occupancy_grid_res", "occupancy_grid_threshold", "chunk_size"))


# --------------------------------------------------------------------------------------
# 1. the kernel against NumPy
# --------------------------------------------------------------------------------------
def _numpy_cut(used, budget):
    P = np.concatenate([[0], np.cumsum(used, dtype=np.int64)])
    n_keep = int(np.searchsorted(P, budget, "right") - 1)
    m_keep = int(P[n_keep])
    seg = np.where(np.arange(P.size) <= n_keep, P, m_keep)
    return seg, n_keep, m_keep


def _counts(N):
    """[0, 800] with runs of zeros: random ones, one at each end, and one around the middle (a cut there has
    zeros on both sides)."""
    rng = np.random.default_rng(N)
    used = rng.integers(0, 801, size=N).astype(np.int32)
    for _ in range(max(1, N // 50)):
        a = int(rng.integers(0, max(N, 1)))
        used[a:a + int(rng.integers(1, 9))] = 0
    if N >= 16:
        used[:2] = 0
        used[-3:] = 0
        used[N // 2 - 2:N // 2 + 3] = 0
        used[N // 2 - 3] = 800
        used[N // 2 + 3] = 1
    elif N:
        used[-1] = 7  # (a total of 0 would leave nothing to cut)
    return used


def _check_budget(cuda, used, budget):
    from nerf_amd import ops
    seg, keep = ops.march_budget(torch.from_numpy(used).to(cuda), budget)
    want_seg, n_keep, m_keep = _numpy_cut(used, budget)
    assert seg.dtype == torch.int32 and seg.shape == (used.size + 1,)
    assert keep.tolist() == [n_keep, m_keep], (used.size, budget)
    np.testing.assert_array_equal(seg.cpu().numpy().astype(np.int64), want_seg, err_msg=f"N {used.size} B {budget}")
    return n_keep, m_keep


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 1023, 1024, 1025, 70001])
def test_budget_kernel_against_numpy(cuda, N):
    used = _counts(N)
    P = np.concatenate([[0], np.cumsum(used, dtype=np.int64)])
    total = int(P[-1])
    budgets = {0, 1, total - 1, total, total + 1, INT32_MAX}
    for r in sorted({N // 2, N // 2 + 1, N // 3, N - 1, N, min(N, 1), min(N, 1024), min(N, 1025)}):
        if 0 <= r <= N:  # (N // 2 sits inside the run of zeros: P[r - 1] == P[r] == P[r + 1])
            budgets |= {int(P[r]) - 1, int(P[r]), int(P[r]) + 1}
    cuts = set()
    for b in sorted(v for v in budgets if 0 <= v <= INT32_MAX):
        cuts.add(_check_budget(cuda, used, b)[0])
    lead = int(np.argmax(used > 0)) if N else 0  # budget 0 keeps the leading rays without points
    assert min(cuts) == lead and N in cuts
    if N >= 16:
        assert N // 2 + 3 in cuts  # budget P[N // 2]: the zeros after the cut are kept, the 1 after them is not
        assert len(cuts) >= 6


def test_budget_kernel_totals_above_2_31(cuda):
    """3,000,000 rays of 800 points: the total, 2.4e9, does not fit in int32; everything written does."""
    from nerf_amd import ops
    N = 3_000_000
    used = torch.full((N,), 800, dtype=torch.int32, device=cuda)
    seg, keep = ops.march_budget(used, INT32_MAX)
    n_keep = INT32_MAX // 800
    assert keep.tolist() == [n_keep, n_keep * 800]
    want = np.minimum(np.arange(N + 1, dtype=np.int64), n_keep) * 800
    got = seg.cpu().numpy()
    assert int(got.min()) >= 0
    np.testing.assert_array_equal(got.astype(np.int64), want)
    # and a budget the whole array stays under by far: a cut in the first tile, the rest filled
    seg, keep = ops.march_budget(used, 799)
    assert keep.tolist() == [0, 0] and int(seg.abs().max()) == 0


def test_budget_kernel_writes_into_spare_slots(cuda):
    """keep may alias two int64 slots of a larger tensor (the march's stats): its neighbours are untouched."""
    from nerf_amd import ops
    used = torch.tensor([3, 0, 5, 7], dtype=torch.int32, device=cuda)
    stats = torch.tensor([11, 12, -1, -1, 15], dtype=torch.int64, device=cuda)
    seg, keep = ops.march_budget(used, 9, keep=stats[2:4])
    assert stats.tolist() == [11, 12, 3, 8, 15] and seg.tolist() == [0, 3, 3, 8, 8]
    seg, keep = ops.march_budget(torch.zeros(5, dtype=torch.int32, device=cuda), 0)  # nothing to cut: every ray kept
    assert keep.tolist() == [5, 0] and seg.tolist() == [0] * 6
    with pytest.raises(RuntimeError, match="budget must be in"):
        ops.march_budget(used, -1)
    with pytest.raises(TypeError, match="int32"):
        ops.march_budget(used.long(), 9)


# --------------------------------------------------------------------------------------
# 2. march_grad(max_points=) on the trained fixture net and its own bake
# --------------------------------------------------------------------------------------
def test_a_cap_above_everything_changes_nothing(cuda, fixture_net):
    f = fixture_net
    plain = _march_grad(f, f["rays"], "fp32")
    g_plain = _flat_grad(f, _loss(plain, f["gt"]))
    capped = _march_grad(f, f["rays"], "fp32", max_points=INT32_MAX)
    g_capped = _flat_grad(f, _loss(capped, f["gt"]))
    assert "rays_kept" not in plain and "n_points" not in plain  # (the uncapped result is today's)
    assert capped["rays_kept"] == 256 and capped["n_points"] == capped["n_queried"] == plain["n_queried"] == 13382
    for k in MAPS + ("n_evaluated", "rounds"):
        assert torch.equal(capped[k], plain[k]) if torch.is_tensor(plain[k]) else capped[k] == plain[k], k
    assert float(g_plain.abs().max()) > 0 and torch.equal(g_capped, g_plain)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3", "bf16x3f", "bf16"])
def test_a_cap_of_6000_points(cuda, fixture_net, dtype):
    """Rows and gradient of the kept rays are those of an uncapped march_grad on rays[:rays_kept] alone, bit for
    bit (the same kernels on the same points at the same positions); the other rows are the no-grad march's."""
    from nerf_amd import ops
    f = fixture_net
    B = 6000
    packer = f["net"].model_fine.packer()
    nograd = ops.march(packer, f["rays"], 2.0, 6.0, f["grid"], t_table=f["t_table"], dtype=dtype,
                       k_schedule=(12, 24, 48, 96, 192, 384, 768), return_used=True)
    _, n_keep, m_keep = _numpy_cut(nograd["ray_used"].cpu().numpy(), B)
    capped = _march_grad(f, f["rays"], dtype, max_points=B)
    kept = capped["rays_kept"]
    print(f"\n{dtype}: {capped['n_queried']} points queried, cap {B}: {kept} rays kept with {capped['n_points']} points")
    assert capped["n_points"] <= B and 0 < kept < 256
    assert (kept, capped["n_points"]) == (n_keep, m_keep)
    assert capped["n_queried"] == nograd["n_queried"] == int(nograd["ray_used"].sum())
    for m in MAPS:
        assert capped[m].shape[0] == 256
        assert torch.equal(capped[m][kept:].detach(), nograd[m][kept:]), m
    g_capped = _flat_grad(f, _loss(capped, f["gt"], kept))
    # a cotangent on the dropped rows alone reaches no parameter
    again = _march_grad(f, f["rays"], dtype, max_points=B)
    g_dropped = _flat_grad(f, sum((again[m][kept:] * 3.0).sum() for m in MAPS))
    assert float(g_dropped.abs().max()) == 0.0
    alone = _march_grad(f, f["rays"][:kept], dtype)
    assert alone["n_queried"] == capped["n_points"]
    for m in MAPS:
        assert torch.equal(capped[m][:kept].detach(), alone[m].detach()), m
    g_alone = _flat_grad(f, _loss(alone, f["gt"][:kept]))
    assert float(g_alone.abs().max()) > 0 and torch.equal(g_capped, g_alone)


def test_a_cap_below_the_steps_is_refused(cuda, fixture_net):
    f = fixture_net
    assert f["t_table"].numel() == 800
    with pytest.raises(ValueError, match="max_points"):
        _march_grad(f, f["rays"], "fp32", max_points=799)
    out = _march_grad(f, f["rays"], "fp32", max_points=800)  # the smallest cap: at least one ray is kept
    assert out["rays_kept"] >= 1 and out["n_points"] <= 800
    none = _march_grad(f, f["rays"][:0], "fp32", max_points=800)  # no rays
    assert none["rays_kept"] == 0 and none["n_points"] == 0 and none["rgb_map_f"].shape == (0, 3)


# --------------------------------------------------------------------------------------
# 3. the budgeted training step
# --------------------------------------------------------------------------------------
def test_training_step_with_a_budget(cuda, budget_cfg, g2, trained_grid, tmp_path, monkeypatch):
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    cfg = budget_cfg
    ta = cfg.task_arg
    net = _trained_net(cuda)
    _write_grid(tmp_path, monkeypatch, trained_grid)
    ta.train_renderer = "accelerated"
    ta.train_grid = "file"
    ta.point_budget = {"target": 8192, "max_points": 4096}
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(1))
    batch = _batch(g2["march_rays"], cuda, gt, device_scalar=True)
    trainer = make_trainer(cfg, net)
    budget = trainer.network.ray_budget
    assert budget.rays == 4096 and budget.max_points == 4096 and trainer.network.online_grid is None
    opt = make_optimizer(cfg, net)
    before = opt.flat_param.clone()
    out, loss, stats = trainer.train_step(dict(batch), opt)
    torch.cuda.synchronize()
    assert set(stats) == {"loss_f", "total_loss", "rays", "points"}
    assert stats["rays"].dtype == stats["points"].dtype == torch.float32
    assert float(stats["rays"]) == 256.0 and 0 < float(stats["points"]) <= 4096
    assert float(stats["points"]) == out["n_points"] and 0 < out["rays_kept"] < 256 and out["n_queried"] == 13382
    assert out["rgb_map_f"].shape == (256, 3)
    assert (budget.rays, budget.observations) == (formula(256, out["n_queried"], 8192), 1)
    assert not torch.equal(opt.flat_param, before) and bool(torch.isfinite(loss))
    # the loss is the MSE over the kept rows
    k = out["rays_kept"]
    want = torch.nn.functional.mse_loss(out["rgb_map_f"][:k].detach(), gt.to(cuda)[:k])
    np.testing.assert_allclose(float(loss.detach()), float(want), rtol=1e-6)
    # validation is untouched (file mode without grad: the hierarchical render) and is no observation
    with torch.no_grad():
        ret, _, vstats = trainer.network(dict(batch))
    assert "rgb_map_c" in ret and set(vstats) == {"loss_c", "loss_f", "total_loss"} and budget.observations == 1
    # chunk_size does not split a budgeted step
    ta.chunk_size = 64
    out2, _, _ = trainer.train_step(dict(batch), opt)
    assert out2["rgb_map_f"].shape == (256, 3) and 0 < out2["n_points"] <= 4096 and budget.observations == 2
    # the same step with the budget off: today's stats
    ta.chunk_size = 4096
    ta.point_budget = {"target": 0}
    plain = make_trainer(cfg, net)
    assert plain.network.ray_budget is None
    out3, _, stats3 = plain.train_step(dict(batch), opt)
    assert set(stats3) == {"loss_f", "total_loss"} and "rays_kept" not in out3


def test_the_loader_draws_the_next_batch_at_the_new_count(cuda, budget_cfg, trained_grid, tmp_path, monkeypatch):
    """With a loader the wrapper sets dataset.batch_rays, and Trainer.train_step's prefetch -- called after the
    forward -- already draws the new count."""
    from src.datasets.make_dataset import BatchLoader
    from src.datasets.nerf.blender import Dataset
    from src.datasets.nerf.synthetic import view_poses
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    from src.utils.camera import focal_for
    cfg = budget_cfg
    ta = cfg.task_arg
    net = _trained_net(cuda)
    _write_grid(tmp_path, monkeypatch, trained_grid)
    ta.train_renderer = "accelerated"
    ta.train_grid = "file"
    ta.train_rays = 512
    ta.point_budget = {"target": 16384, "min_rays": 256}
    images = torch.rand(4, 64, 64, 3, generator=torch.Generator().manual_seed(7)).to(cuda)
    ds = Dataset.from_arrays(images, view_poses(4, seed=3).to(cuda), focal_for(64))
    loader = BatchLoader(ds, 3)
    trainer = make_trainer(cfg, net, loader)
    opt = make_optimizer(cfg, net)
    assert ds.batch_rays == trainer.network.ray_budget.rays == 512
    it = iter(loader)
    first = next(it)
    assert first["rays"].shape[1] == 512
    out, _, _ = trainer.train_step(trainer.prepare(first), opt, prefetch=lambda: next(it, None))
    want = formula(512, out["n_queried"], 16384, min_rays=256)
    assert want != 512  # (the test would show nothing otherwise)
    assert ds.batch_rays == trainer.network.ray_budget.rays == want
    assert trainer.prefetched["rays"].shape[1] == want


# --------------------------------------------------------------------------------------
# 4. from scratch: the ray count follows the pruning grid
# --------------------------------------------------------------------------------------
SCRATCH_STEPS = 160


def test_from_scratch_the_ray_count_follows_the_grid(cuda, budget_cfg):
    """The from-scratch setup of test_gpu_grid_update.py (procedural 100x100 scene, seed-0 init, online grid, fp32)
    with target 65536, max_points 98304, min_rays 256, from 1024 rays: the cap holds at every step, every count is
    the formula of the step before, and the count grows while the grid prunes and the loss falls.
    Measured on an MI355X (2.5 s), means per 16 steps:
      rays             320 256 256 256 256 256 256 272 288 336
      points queried   124585 96188 59700 44659 43871 42494 39595 39389 40452 44128
      points (capped)  97829 95280 59700 44659 43871 42494 39595 39389 40452 44128
      rays kept        251 254 256 256 256 256 256 272 288 336
      loss             0.1145 0.0780 0.0453 0.0402 0.0359 0.0293 0.0276 0.0248 0.0229 0.0219
    the cap dropped rays in 14 steps, all among the first 32.  A ray costs ~390 points at first (1024 -> 512 -> 256
    rays, the floor) and ~130 by step 100, where 65536 // 130 crosses 512 and the count starts to leave the floor:
    the last 16 steps are at 256 or 512 rays (mean 336 against the first 16 steps' 320 = (1024 + 512 + 14 * 256) / 16).
    The run is deterministic (integer controller, fixed-order gradient sums), so the comparison is not a matter of
    luck, but its margin is one step at 512 rays."""
    from nerf_amd import ops
    from src.datasets.nerf.blender import Dataset
    from src.datasets.nerf.synthetic import make_scene
    from src.models import make_network
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    cfg = budget_cfg
    ta = cfg.task_arg
    ta.train_rays = 1024
    ta.train_renderer = "accelerated"
    ta.train_grid = "online"
    ta.point_budget = {"target": 65536, "max_points": 98304, "min_rays": 256}
    imgs, poses, focal = make_scene(100, 100, 100, cuda, seed=0)
    ds = Dataset.from_arrays(imgs, poses, focal)
    torch.manual_seed(0)
    net = make_network(cfg).to(cuda)
    trainer = make_trainer(cfg, net)
    budget = trainer.network.ray_budget
    assert budget.rays == 1024
    opt = make_optimizer(cfg, net)
    rays_n, queried, points, kept, losses = [], [], [], [], []
    for _ in range(SCRATCH_STEPS):
        n = budget.rays
        rays, rgbs = ds.sample_batch(n_rays=n)
        out, loss, stats = trainer.train_step({"rays": rays[None], "rgbs": rgbs[None],
                                               "near": ops.device_scalar(2.0, cuda),
                                               "far": ops.device_scalar(6.0, cuda)}, opt)
        assert rays.shape[0] == n == int(stats["rays"])
        rays_n.append(n)
        queried.append(out["n_queried"])
        points.append(int(stats["points"]))
        kept.append(out["rays_kept"])
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu().numpy()
    assert bool(np.isfinite(losses).all())

    def per16(v):
        return [float(np.mean(v[i:i + 16])) for i in range(0, SCRATCH_STEPS, 16)]

    print(f"\nfrom scratch with a point budget, {SCRATCH_STEPS} steps; per 16 steps:"
          f"\n  rays    " + " ".join(f"{v:.0f}" for v in per16(rays_n)) +
          f"\n  queried " + " ".join(f"{v:.0f}" for v in per16(queried)) +
          f"\n  points  " + " ".join(f"{v:.0f}" for v in per16(points)) +
          f"\n  kept    " + " ".join(f"{v:.0f}" for v in per16(kept)) +
          f"\n  loss    " + " ".join(f"{v:.4f}" for v in per16(losses)) +
          f"\n  steps in which the cap dropped rays: {sum(k < n for k, n in zip(kept, rays_n))}")
    assert max(points) <= 98304 and min(points) >= 0
    assert all(p <= q for p, q in zip(points, queried)) and all(0 < k <= n for k, n in zip(kept, rays_n))
    for i in range(1, SCRATCH_STEPS):
        assert rays_n[i] == formula(rays_n[i - 1], queried[i - 1], 65536, min_rays=256), i
    assert budget.observations == SCRATCH_STEPS
    assert np.mean(rays_n[-16:]) > np.mean(rays_n[:16])
    assert losses[-16:].mean() < losses[:16].mean()


# --------------------------------------------------------------------------------------
# 5. save and resume
# --------------------------------------------------------------------------------------
def test_save_and_resume(cuda, budget_cfg, g2, tmp_path, monkeypatch):
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    from src.train.trainers.nerf import BUDGET_STATE_FILE, GRID_STATE_FILE
    cfg = budget_cfg
    ta = cfg.task_arg
    monkeypatch.chdir(tmp_path)
    net = _trained_net(cuda)
    ta.train_renderer = "accelerated"
    ta.train_grid = "online"
    ta.train_rays = 2048
    ta.occupancy_grid_res = 33
    ta.grid_update = {"interval": 2, "warmup_updates": 1, "period": 4}
    ta.point_budget = {"target": 8192, "max_points": 4096}
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(1))
    batch = _batch(g2["march_rays"], cuda, gt, device_scalar=True)
    a = make_trainer(cfg, net)
    opt = make_optimizer(cfg, net)
    assert a.network.ray_budget.rays == 2048
    out, _, _ = a.train_step(dict(batch), opt)
    rays = a.network.ray_budget.rays
    assert rays == formula(256, out["n_queried"], 8192) != 2048
    model_dir = str(tmp_path / "trained_model")
    a.network.save_grid(model_dir)
    assert sorted(os.listdir(model_dir)) == sorted([GRID_STATE_FILE, BUDGET_STATE_FILE])
    b = make_trainer(cfg, net)  # fresh objects
    assert b.network.ray_budget.rays == 2048 and b.network.ray_budget.observations == 0
    assert b.network.load_grid(model_dir) is True
    assert (b.network.ray_budget.rays, b.network.ray_budget.observations) == (rays, 1)
    # without the file: the count is train_rays
    c = make_trainer(cfg, net)
    assert c.network.load_grid(str(tmp_path / "nothing_here")) is False
    assert (c.network.ray_budget.rays, c.network.ray_budget.observations) == (2048, 0)
    # file mode saves and restores the count too (there is no grid state to write)
    ta.train_grid = "file"
    d = make_trainer(cfg, net)  # (logs/<cfg name>/occupancy_grid.pt: the online trainer wrote it)
    d.network.ray_budget.observe(8192, 8192 * 4)  # 2048 rays wanted, half of 8192 is 4096
    other = str(tmp_path / "file_mode")
    d.network.save_grid(other)
    assert os.listdir(other) == [BUDGET_STATE_FILE]
    e = make_trainer(cfg, net)
    assert e.network.load_grid(other) is False and e.network.ray_budget.rays == d.network.ray_budget.rays == 4096
    assert e.network.ray_budget.observations == 1
