"""Data-parallel training with a point budget (task_arg.point_budget) on two ranks.

Two processes share cuda:0 over gloo, as in test_gpu_dp_grid.py.  Each rank draws its own rays and
follows its OWN ray count (its RayBudget observes its own march; no collective carries the count), so
the counts may differ between the ranks; the gradient all-reduce averages the ranks' mean gradients,
so after every step the weights are bit-identical, and with them the online grids.
"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from march_support import _free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STEPS = 3
TARGET, CAP, MIN_RAYS = 32768, 49152, 256


def _formula(n_rays, n_queried):
    want = 32768 if n_queried == 0 else (TARGET * n_rays) // n_queried
    want = min(max(want, n_rays // 2), 2 * n_rays)
    return min(max((want // 256) * 256, MIN_RAYS), 32768)


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), NERF_AMD_NO_ARGV="1")
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "nerf-replication_amd")]
    try:
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.cuda.set_device(0)
        from nerf_amd import ops
        from src.config import cfg
        from src.datasets.nerf.blender import Dataset
        from src.datasets.nerf.synthetic import view_poses
        from src.models.nerf.network import Network
        from src.train.optimizer import make_optimizer
        from src.train.trainers.make_trainer import make_trainer
        from src.utils.camera import focal_for
        dev = torch.device("cuda", 0)
        ta = cfg.task_arg
        ta.perturb = 0
        ta.mlp_dtype = "fp32"
        ta.train_rays = 1024
        ta.train_renderer = "accelerated"
        ta.train_grid = "online"
        ta.occupancy_grid_res = 64
        ta.grid_update = {"interval": 2, "warmup_updates": 2, "period": 4}
        ta.point_budget = {"target": TARGET, "max_points": CAP, "min_rays": MIN_RAYS}
        z = np.load(os.path.join(HERE, "golden", "trained_v2.npz"), allow_pickle=False)
        torch.manual_seed(0)
        net = Network()
        net.load_state_dict({k: torch.from_numpy(z[k]) for k in z.files}, strict=True)
        net = net.to(dev)
        trainer = make_trainer(cfg, net)
        opt = make_optimizer(cfg, net)
        budget = trainer.network.ray_budget
        images = torch.rand(4, 128, 128, 3, generator=torch.Generator().manual_seed(7)).to(dev)
        ds = Dataset.from_arrays(images, view_poses(4, seed=3).to(dev), focal_for(128))
        grid = trainer.network.online_grid
        counts, same_params, first = [], [], None
        for _ in range(STEPS):
            n = budget.rays
            rays, rgbs = ds.sample_batch(n_rays=n)
            if first is None:
                first = rays.cpu()
            out, _, stats = trainer.train_step({"rays": rays[None], "rgbs": rgbs[None],
                                                "near": ops.device_scalar(2.0, dev),
                                                "far": ops.device_scalar(6.0, dev)}, opt)
            assert rays.shape[0] == n and budget.rays == _formula(n, out["n_queried"])
            assert out["n_points"] <= CAP and int(stats["points"]) == out["n_points"]
            counts.append([n, out["n_queried"], out["rays_kept"]])
            mine = opt.flat_param.cpu()
            every = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(every, mine)
            same_params.append(all(torch.equal(every[0], e) for e in every[1:]))
        torch.cuda.synchronize()
        same = {}
        for k, t in {"rays": first, "density": grid.density.cpu(), "grid": grid.grid.cpu()}.items():
            every = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(every, t)
            same[k] = all(torch.equal(every[0], e) for e in every[1:])
        q.put((rank, same, same_params, counts, (grid.updates, grid.steps), float(grid.grid.float().mean()), None))
        dist.destroy_process_group()
    except Exception:  # noqa: BLE001 - reported to the parent
        import traceback
        q.put((rank, None, None, None, None, None, traceback.format_exc()))


def test_two_ranks_follow_their_own_counts():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=240) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert sorted(r[0] for r in res) == [0, 1]
    for rank, same, same_params, counts, counters, occupied, err in sorted(res, key=lambda r: r[0]):
        assert err is None, err
        print(f"\nrank {rank}: (rays, points queried, rays kept) per step {counts}")
        assert counters == (2, STEPS)  # updates at the grid's steps 0 and 2
        assert not same["rays"]  # each rank drew its own rays
        assert same_params == [True] * STEPS, (rank, same_params)  # after every step
        assert same["density"] and same["grid"], (rank, same)
        assert 0.0 < occupied < 1.0
        assert counts[0][0] == 1024 and all(0 < k <= n for n, _, k in counts)
        assert all(n % 256 == 0 and MIN_RAYS <= n <= 32768 for n, _, _ in counts)
    # (the ranks' counts MAY differ -- each follows its own rays -- and nothing above needed them equal)
    for p in procs:
        assert p.exitcode == 0
