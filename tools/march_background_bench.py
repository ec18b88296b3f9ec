"""What random background colours (task_arg.train_background: random) cost the accelerated training step.

    python tools/march_background_bench.py [--steps 48] [--tiers fp32,bf16x3f] [--out profiles/r13/random_background.json]

One process, the trained fixture net (tests/golden/trained_v2.npz) and its res-128 bake, the golden_v2
``rays4096`` rays, as tools/march_jitter_bench.py: ``Trainer.train_step`` of the accelerated mode with the key
off and on, interleaved in blocks of 4 steps, each step between two HIP events, median after a warm-up.  Each
mode steps its own copy of the net with the learning rate at 0 (every launch of the step runs, Adam included,
and the weights stay: a net that trains changes its point count within tens of steps, by a different amount
per target, and the cost of a step is its points -- so both modes march the fixture net's own 77,887 points):
off towards golden_v2's ``grad4096_gt`` (on white), on towards the same target moved onto the batch's colours,
gt - (1 - acc)(1 - bg) with the fixture net's own fp32 acc of those rays.  And the kernels alone, HIP events
around blocks of 100 launches into preallocated outputs: the segment compositing pair on that batch's own
segments (the fixture net's raw values) through the ``_bg`` entry points with a null and a non-null ``bg`` (the
BG = false / true instantiations), and ray generation, 4,096 drawn rays of 8 procedural 100 x 100 views,
nerf_raygen against nerf_raygen_rgba.  The result is merged into --out under "background_step" /
"background_kernels".
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "nerf-replication_amd"))
os.environ.setdefault("NERF_AMD_NO_ARGV", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def blocks_us(fn, reps=12, per=100):
    """median us per call of fn over `reps` blocks of `per` back-to-back calls (the first two blocks dropped)"""
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per):
            fn()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    return round(statistics.median(1000.0 * x.elapsed_time(y) / per for x, y in ev[2:]), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tiers", default="fp32,bf16x3f")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "random_background.json"))
    a = ap.parse_args()
    from nerf_amd import ops
    from nerf_amd._lib import check, lib, ptr
    from src.config import cfg
    from src.datasets.nerf.synthetic import make_scene_rgba
    from src.models.nerf.network import Network
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer

    dev = torch.device("cuda:0")
    gold = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(gold, "trained_v2.npz"), allow_pickle=False)
    state = {k: torch.from_numpy(z[k]) for k in z.files}
    g2 = np.load(os.path.join(gold, "golden_v2.npz"), allow_pickle=False)
    grid = torch.from_numpy(np.unpackbits(g2["bake128_packed"])[: 128 ** 3].reshape(128, 128, 128).astype(bool))
    rays = torch.from_numpy(g2["rays4096"]).to(dev)
    gt = torch.from_numpy(g2["grad4096_gt"]).reshape(-1, 3).to(dev)
    bg = torch.rand(rays.shape[0], 3, generator=torch.Generator().manual_seed(2)).to(dev)
    ta = cfg.task_arg
    ta.perturb = 0
    ta.train_renderer = "hierarchical"
    ta.train_background = "white"

    def stack(dtype):
        torch.manual_seed(0)
        net = Network()
        net.load_state_dict(state, strict=True)
        net = net.to(dev)
        net.mlp_dtype = dtype
        trainer = make_trainer(cfg, net)
        trainer.network.train_renderer = "accelerated"  # (the grid handed over directly: no logs/ file)
        trainer.network.renderer.set_occupancy_grid(grid, dev)
        opt = make_optimizer(cfg, net)
        for group in opt.param_groups:
            group["lr"] = 0.0
        return net, trainer, opt

    with torch.no_grad():  # the targets: on white as given; on the colours, what shows through by the net's own acc
        acc = ops.march(stack("fp32")[0].model_fine.packer(), rays, 2.0, 6.0, grid, dtype="fp32")["acc_map_f"]
        targets = {"white": gt, "random": gt - (1.0 - acc)[:, None] * (1.0 - bg)}
    batches = {m: {"rays": rays[None], "rgbs": t[None], "bg": bg[None], "near": ops.device_scalar(2.0, dev),
                   "far": ops.device_scalar(6.0, dev)} for m, t in targets.items()}

    steps = {}
    for dtype in a.tiers.split(","):
        ta.mlp_dtype = dtype
        stacks = {m: stack(dtype) for m in ("white", "random")}
        events = {m: [] for m in stacks}
        queried = {m: [] for m in stacks}
        done = -a.warmup
        while done < a.steps:
            for m, (_, trainer, opt) in stacks.items():
                ta.train_background = m  # (the renderer reads the key at every step)
                trainer.network.train_background = m
                for _ in range(4):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out, _, _ = trainer.train_step(dict(batches[m]), opt)
                    e1.record()
                    if done >= 0:
                        events[m].append((e0, e1))
                        queried[m].append(out["n_queried"])
            done += 4
        ta.train_background = "white"
        torch.cuda.synchronize()
        ms = {m: [x.elapsed_time(y) for x, y in v] for m, v in events.items()}
        steps[dtype] = {"ms_per_step_median": {m: round(statistics.median(v), 4) for m, v in ms.items()},
                        "ms_per_step_min": {m: round(min(v), 4) for m, v in ms.items()},
                        "n_queried_median": {m: int(statistics.median(v)) for m, v in queried.items()},
                        "timed_steps": len(ms["white"])}
        print("step", dtype, json.dumps(steps[dtype]), flush=True)
        del stacks
        torch.cuda.empty_cache()

    # ---- the kernels alone ---------------------------------------------------------------------------
    torch.manual_seed(0)
    net = Network()
    net.load_state_dict(state, strict=True)
    net = net.to(dev)
    packer = net.model_fine.packer()
    with torch.no_grad():  # the batch's own segments, as ops.march_grad lays them out
        out, walk = ops._march(packer, rays, 2.0, 6.0, grid, step_size=0.005, t_thresh=1e-4, bbox=ops.SCENE_BBOX,
                               white_bkgd=True, dtype="fp32", t_table=None,
                               k_schedule=(12, 24, 48, 96, 192, 384, 768), round_bytes=1 << 31, use_macro=True,
                               return_used=True)
        rays_c, t_tab, _, g8, _, macro, vd = walk
        N, M = rays_c.shape[0], out["n_queried"]
        seg_off = torch.zeros(N + 1, dtype=torch.int32, device=dev)
        seg_off[1:] = torch.cumsum(out["ray_used"], 0, dtype=torch.int32)
        out_ray, out_step, out_pts = ops.march_segments(rays_c, t_tab, g8, macro, seg_off, M)
        raw = ops.mlp(packer, out_pts, vd, 1, out_ray, "fp32").reshape(-1, 4).contiguous()
    rgb, depth, acc = (torch.empty(N, 3, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev))
    dist, totals = torch.empty(N, device=dev), torch.empty(N, 2, device=dev, dtype=torch.float64)
    g_rgb, g_raw = torch.randn(N, 3, device=dev), torch.empty_like(raw)
    s = torch.cuda.current_stream(dev).cuda_stream
    head = (ptr(raw), ptr(rays_c), N, ptr(t_tab), ptr(seg_off), ptr(out_step), 0.005, 1)
    L = lib()
    kernels = {"rays": N, "points": M,
               "timing": "HIP events around 100 back-to-back launches into preallocated outputs, median of 10 blocks"}
    for name, b in (("white", None), ("bg", bg)):
        for dn, (d, t) in (("", (None, None)), ("_dist", (dist, totals))):
            def fwd():
                check(L.nerf_march_seg_composite_fwd_bg(*head, ptr(rgb), ptr(depth), ptr(acc), None, 0.25, ptr(d),
                                                        ptr(t), ptr(b), s), "fwd")

            def bwd():
                check(L.nerf_march_seg_composite_bwd_bg(*head, ptr(g_rgb), None, None, None, 0.25, None, ptr(t),
                                                        ptr(g_raw), ptr(b), s), "bwd")
            fwd()
            kernels[f"seg_fwd{dn}_{name}_us"] = blocks_us(fwd)
            kernels[f"seg_bwd{dn}_{name}_us"] = blocks_us(bwd)
    imgs, poses, focal = make_scene_rgba(8, 100, 100, dev)
    white = (imgs[..., :3] * imgs[..., 3:] + (1.0 - imgs[..., 3:])).contiguous()
    o_rays, o_rgb, o_bg = torch.empty(N, 6, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, 3, device=dev)
    count = [0]

    def raygen():
        count[0] += 1
        check(L.nerf_raygen(ptr(poses), 8, 100, 100, float(focal), None, N, 1234, count[0], ptr(white), ptr(o_rays),
                            ptr(o_rgb), None, s), "raygen")

    def raygen_rgba():
        count[0] += 1
        check(L.nerf_raygen_rgba(ptr(poses), 8, 100, 100, float(focal), None, N, 1234, count[0], ptr(imgs), None,
                                 ptr(o_rays), ptr(o_rgb), None, ptr(o_bg), s), "raygen_rgba")
    kernels["raygen_us"] = blocks_us(raygen)
    kernels["raygen_rgba_us"] = blocks_us(raygen_rgba)
    print("kernels", json.dumps(kernels), flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    result.update(device=torch.cuda.get_device_name(0), background_kernels=kernels,
                  background_step={"rays": int(rays.shape[0]), "warmup": a.warmup,
                                   "timing": "HIP events around Trainer.train_step, key off / on interleaved in "
                                             "blocks of 4, median; learning rate 0 (the nets stay, both "
                                             "modes march the same points)", "tiers": steps})
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
