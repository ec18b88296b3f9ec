"""CPU, world_size 2 (gloo): the data-parallel step's collective semantics.

Each rank holds a flat gradient (FusedAdam.flat_grad's role); allreduce_grads and the
per-net GradBuckets (started from backward, remainder in finish) must leave every rank
with the mean; broadcast_params must give every rank rank-0's weights
(DistributedDataParallel's construction broadcast, trainer.py:15-22 of the reference); the
tile-split renderer must reproduce a single-process render.
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from march_support import _free_port


class _FakeRenderer:
    """rgb / depth / acc as fixed functions of each ray (the split/gather logic under test)."""

    def __init__(self):
        self.seen = []

    def render(self, batch):
        r = batch["rays"].reshape(-1, 6)
        self.seen.append(r[:, 0].clone())
        return {"rgb_map_f": r[:, :3] * 2.0, "depth_map_f": r[:, 3] + 1.0, "acc_map_f": r[:, 4],
                "n_queried": int(r.shape[0])}

    render_accelerated = render


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      NERF_AMD_NO_ARGV="1")
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "nerf-replication_amd")]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from src.train.trainers.trainer import allreduce_grads, broadcast_params

    class Opt:
        pass

    opt = Opt()
    opt.flat_grad = torch.arange(10, dtype=torch.float32) * (rank + 1)
    allreduce_grads(opt)
    opt_grad_plain = opt.flat_grad.tolist()
    lin = torch.nn.Linear(4, 3)
    torch.nn.init.constant_(lin.weight, float(rank))
    broadcast_params(lin)
    # per-net buckets: one slice reported from "backward", the rest reduced in finish()
    from src.train.trainers.trainer import GradBuckets
    opt.flat_grad = torch.arange(10, dtype=torch.float32) * (rank + 1)
    bk = GradBuckets()
    bk._hook(opt.flat_grad[2:6])
    bk.finish(opt)
    bucket_grad = opt.flat_grad.tolist()
    # a two-chunk training step (train_rays = 2 x chunk_size): each net's MLP runs once per
    # chunk, its bucket must fire once, after the LAST chunk's backward (ops.PackedMLP
    # pending count), and the bucketed average must equal the plain flat average
    from nerf_amd.ops import PackedMLP
    coarse = PackedMLP([torch.zeros(1)] * 24)
    fine = PackedMLP([torch.zeros(1)] * 24)
    flat = torch.zeros(10)
    opt.flat_grad = flat
    bk = GradBuckets()
    bk.attach([coarse, fine])
    bk.begin()
    g = torch.Generator().manual_seed(100 + rank)
    parts = {k: torch.randn(n, generator=g) for k, n in (("c1", 6), ("c2", 6), ("f1", 4), ("f2", 4))}
    for _ in range(2):  # forward: chunk 1 then chunk 2, coarse then fine
        coarse.forward_started()
        fine.forward_started()
    fired = []
    # backward in reverse: chunk 2 (fine, coarse), then chunk 1 (fine, coarse)
    for key, pk, sl in (("f2", fine, slice(6, 10)), ("c2", coarse, slice(0, 6)), ("f1", fine, slice(6, 10)),
                        ("c1", coarse, slice(0, 6))):
        flat[sl] += parts[key]
        fired.append(pk.backward_done(flat[sl]))
    n_works = len(bk.works)
    bk.finish(opt)
    local = torch.cat([parts["c1"] + parts["c2"], parts["f1"] + parts["f2"]])
    plain = local.clone()
    dist.all_reduce(plain)
    plain /= world
    two_chunk_ok = fired == [False, False, True, True] and n_works == 2 and torch.allclose(flat, plain, atol=1e-6)
    # rank-distinct ray streams (the reference's fix_random makes every rank draw the same
    # rays, blender.py:126 + train.py:25-28; here the Philox seeds differ per rank)
    from src.datasets.nerf.blender import Dataset
    torch.manual_seed(0)  # identical torch seed on every rank, as fix_random would set
    ds = Dataset.from_arrays(torch.zeros(1, 2, 2, 3), torch.eye(4)[None], 1.0)
    from src.models.nerf.renderer.volume_renderer import Renderer
    seeds = torch.tensor([ds.seed & 0xFFFFFFFF, Renderer(None)._seed & 0xFFFFFFFF], dtype=torch.int64)
    all_seeds = [torch.zeros_like(seeds) for _ in range(world)]
    dist.all_gather(all_seeds, seeds)
    seeds_distinct = len({tuple(s.tolist()) for s in all_seeds}) == world
    # tile-split inference: 1001 rays over the ranks in interleaved 256-ray blocks (rank r
    # renders blocks r, r + W, ...), gathered everywhere in ray order
    from src.utils.dist_render import interleaved_index, render_distributed
    rays = torch.arange(1001 * 6, dtype=torch.float32).reshape(1, 1001, 6)
    full = _FakeRenderer().render({"rays": rays})
    fr = _FakeRenderer()
    got = render_distributed(fr, {"rays": rays})
    ok = all(torch.equal(got[k], full[k]) for k in ("rgb_map_f", "depth_map_f", "acc_map_f"))
    mine = interleaved_index(1001, rank, world)
    ok = ok and len(fr.seen) == 1 and torch.equal(fr.seen[0], rays[0, mine, 0])
    ok = ok and int(mine[0]) == 256 * rank and (mine // 256 % world == rank).all().item()
    q.put((rank, opt_grad_plain, float(lin.weight.sum()), bucket_grad, ok and got["n_queried"] == 1001,
           two_chunk_ok, seeds_distinct))
    dist.destroy_process_group()


def test_two_rank_gradient_average_and_broadcast():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    expect = [1.5 * i for i in range(10)]
    for rank, grad, wsum, bucket_grad, render_ok, two_chunk_ok, seeds_distinct in res:
        assert grad == pytest.approx(expect)
        assert wsum == 0.0  # rank 0's weights everywhere
        assert bucket_grad == pytest.approx(expect)  # bucketed + remainder == one flat average
        assert render_ok  # tile-split render == single-process render
        assert two_chunk_ok  # one bucket per net after its last chunk; == the flat average
        assert seeds_distinct  # every rank draws its own rays


def test_interleaved_split_balances_a_central_workload():
    """SURVEY.md 8e / render_accelerated: the march's work sits in the rows that cross the
    occupied cells.  With the work of an 800x800 frame concentrated in its central rows, the
    busiest of 8 ranks gets <= 2 % above the mean share by interleaved blocks, against >= 2x by
    contiguous row blocks; every ray is rendered exactly once."""
    from src.utils.dist_render import interleaved_index, shard_bounds
    H = W = 800
    n, world = H * W, 8
    row = torch.arange(n) // W
    work = torch.exp(-((row.float() - 400.0) / 120.0) ** 2)  # central rows hold the occupied cells
    mean = float(work.sum()) / world
    idx = [interleaved_index(n, r, world) for r in range(world)]
    assert torch.equal(torch.sort(torch.cat(idx)).values, torch.arange(n))
    inter = max(float(work[i].sum()) for i in idx) / mean
    contig = max(float(work[slice(*shard_bounds(n, r, world))].sum()) for r in range(world)) / mean
    assert inter <= 1.02 and contig >= 2.0, (inter, contig)


class _EmptyAwareRenderer(_FakeRenderer):
    """As the reference Renderer.render: no rays -> {} (it must never be asked, though)."""

    def render(self, batch):
        r = batch["rays"].reshape(-1, 6)
        if r.shape[0] == 0:
            self.empty_calls = getattr(self, "empty_calls", 0) + 1
            return {}
        out = super().render(batch)
        out["render_time"] = 0.5 + dist.get_rank()
        return out

    render_accelerated = render


def _small_image_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      NERF_AMD_NO_ARGV="1")
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "nerf-replication_amd")]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from src.utils.dist_render import render_distributed
    results = []
    # 2 rays on 3 ranks (one rank has nothing), 5 rays, a 40x40 view (< 256 * (W - 1) rays)
    for n in (2, 5, 1600, 1001):
        rays = torch.arange(n * 6, dtype=torch.float32).reshape(1, n, 6)
        full = _FakeRenderer().render({"rays": rays})
        fr = _EmptyAwareRenderer()
        got = render_distributed(fr, {"rays": rays}, accelerated=(n == 5))
        ok = all(torch.equal(got[k], full[k]) for k in ("rgb_map_f", "depth_map_f", "acc_map_f"))
        ok = ok and got["n_queried"] == n and got["render_time"] == 0.5 + (world - 1 if n >= world else 1)
        ok = ok and getattr(fr, "empty_calls", 0) == 0 and len(fr.seen) == (1 if (n >= world or rank < n) else 0)
        results.append((n, ok))
    q.put((rank, results))
    dist.destroy_process_group()


def test_small_image_split_no_rank_idle_and_no_deadlock():
    """256-ray blocks leave ranks without rays on images of <= 256 (W - 1) rays;
    the reference renderer returns {} for zero rays and such a rank would skip the gathers the
    others block in.  Blocks shrink so every rank renders when n >= W; when n < W the empty
    rank skips rendering and joins the gathers with empty parts."""
    world = 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_small_image_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, results in res:
        assert all(ok for _, ok in results), (rank, results)


def test_ray_block_shrinks_for_small_images():
    from src.utils.dist_render import RAY_BLOCK, interleaved_index, ray_block
    assert ray_block(640000, 8) == RAY_BLOCK
    for n, world in ((1600, 8), (7, 8), (8, 8), (2049, 8), (1, 1)):
        b = ray_block(n, world)
        idx = [interleaved_index(n, r, world, b) for r in range(world)]
        assert torch.equal(torch.sort(torch.cat(idx)).values, torch.arange(n))
        if n >= world:
            assert min(i.numel() for i in idx) >= 1, (n, world, b)


def _fake_bake_slab(res):
    """A deterministic 'bake' of voxel slab (x0, x1): cell (x, y, z) occupied iff (7x + 3y + z) % 5 == 0."""
    def f(slab):
        x0, x1 = slab
        x, y, z = torch.meshgrid(torch.arange(x0, x1), torch.arange(res), torch.arange(res), indexing="ij")
        return (7 * x + 3 * y + z) % 5 == 0
    return f


def _bake_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      NERF_AMD_NO_ARGV="1")
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "nerf-replication_amd")]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from src.utils.dist_render import bake_distributed, shard_bounds
    res = 10
    seen = []
    fake = _fake_bake_slab(res)

    def slab(sl):
        seen.append(tuple(sl))
        return fake(sl)
    got = bake_distributed(slab, res)
    full = fake((0, res))
    q.put((rank, bool(torch.equal(got, full)), seen, shard_bounds(res, rank, world)))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_grid_bake_voxel_slabs_all_gathered(world):
    """SURVEY.md 8e grid bake: each rank bakes only its own x-slab (sizes differ by at most one;
    res 10 over 3 ranks pads the all-gather), and every rank ends with the full grid."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_bake_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok, seen, bounds in res:
        assert ok
        assert seen == [tuple(bounds)]  # the rank baked its own slab and nothing else
