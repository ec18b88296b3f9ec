"""World-2 gloo (CPU): the data-parallel gradient of a training step through the grid march
(task_arg.train_renderer "accelerated").  Only the fine net runs, in one or several chunks, so
only its bucket fires from the backward; GradBuckets.finish must all-reduce the coarse range
too (zero on every rank) and leave every rank with the average of the flat gradient."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from march_support import _free_port


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      NERF_AMD_NO_ARGV="1")
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "nerf-replication_amd")]
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nerf_amd.ops import PackedMLP
    from src.train.trainers.trainer import GradBuckets

    class Opt:
        pass

    results = []
    for chunks in (1, 3):
        coarse = PackedMLP([torch.zeros(1)] * 24)
        fine = PackedMLP([torch.zeros(1)] * 24)
        # the coarse slice [0, 6) carries a rank-dependent left-over that only finish() can average
        flat = torch.cat([torch.full((6,), float(rank + 1)), torch.zeros(4)])
        opt = Opt()
        opt.flat_grad = flat
        bk = GradBuckets()
        bk.attach([coarse, fine])
        bk.begin()
        g = torch.Generator().manual_seed(7 + rank)
        parts = [torch.randn(4, generator=g) for _ in range(chunks)]
        for _ in range(chunks):  # the fine net's forward, once per chunk; the coarse net never runs
            fine.forward_started()
        fired = []
        for p in reversed(parts):
            flat[6:] += p
            fired.append(fine.backward_done(flat[6:]))
        n_works = len(bk.works)
        local = torch.cat([torch.full((6,), float(rank + 1)), sum(parts)])
        bk.finish(opt)
        plain = local.clone()
        dist.all_reduce(plain)
        plain /= world
        results.append(fired == [False] * (chunks - 1) + [True] and n_works == 1 and coarse.pending == 0
                       and torch.allclose(flat, plain, atol=1e-6) and torch.equal(flat[:6], torch.full((6,), 1.5)))
    q.put((rank, results))
    dist.destroy_process_group()


def test_only_the_fine_bucket_fires_and_finish_reduces_the_coarse_range():
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
    assert sorted(r for r, _ in res) == [0, 1]
    for rank, results in res:
        assert results == [True, True], (rank, results)
