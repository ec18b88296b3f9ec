"""What the distortion loss (task_arg.distortion_loss_weight) costs the accelerated training step.

    python tools/march_distortion_bench.py [--steps 48] [--weight 0.01] [--tiers fp32,bf16x3f]
                                           [--out profiles/r11/distortion.json]

One process, the trained fixture net (tests/golden/trained_v2.npz) and its res-128 bake, the golden_v2
``rays4096`` batch, as tools/march_jitter_bench.py: ``Trainer.train_step`` of the accelerated mode with the
weight 0 and --weight, interleaved in blocks of 4 steps, each step between two HIP events, median after a
warm-up (each mode trains its own copy of the net); and the two segment compositing kernels' own times with
and without the distortion (ops.kernel_timer's HIP events around each launch of ops.march_grad's forward and
backward on the same batch, median of --steps).  The result is merged into --out under "step_cost" /
"kernels".  ``--only-plain`` times the weight-0 step alone and prints one JSON line (the A/B of two builds
in alternating processes).
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

SEG_KERNELS = ("march_seg_composite_fwd", "march_seg_composite_bwd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--weight", type=float, default=0.01)
    ap.add_argument("--tiers", default="fp32,bf16x3f")
    ap.add_argument("--only-plain", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "distortion.json"))
    a = ap.parse_args()
    from nerf_amd import ops
    from src.config import cfg
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
    batch = {"rays": rays[None], "rgbs": gt[None], "near": ops.device_scalar(2.0, dev),
             "far": ops.device_scalar(6.0, dev)}
    ta = cfg.task_arg
    ta.perturb = 0
    ta.train_renderer = "hierarchical"
    has_key = not a.only_plain  # (--only-plain also runs on a build from before the key)
    weights = {"plain": 0.0} if a.only_plain else {"plain": 0.0, "distortion": a.weight}

    def stack(dtype, weight):
        torch.manual_seed(0)
        net = Network()
        net.load_state_dict(state, strict=True)
        net = net.to(dev)
        net.mlp_dtype = dtype
        trainer = make_trainer(cfg, net)
        trainer.network.train_renderer = "accelerated"  # (the grid handed over directly: no logs/ file)
        trainer.network.renderer.set_occupancy_grid(grid, dev)
        if has_key:
            trainer.network.distortion_weight = weight
        return net, trainer, make_optimizer(cfg, net)

    steps = {}
    for dtype in a.tiers.split(","):
        ta.mlp_dtype = dtype
        stacks = {m: stack(dtype, w) for m, w in weights.items()}
        events = {m: [] for m in stacks}
        dist = []
        done = -a.warmup
        while done < a.steps:
            for m, (_, trainer, opt) in stacks.items():
                if has_key:
                    ta.distortion_loss_weight = weights[m]  # (the renderer reads the key at every step)
                for _ in range(4):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out, _, stats = trainer.train_step(dict(batch), opt)
                    e1.record()
                    assert ("dist_map_f" in out) == (weights[m] > 0) == ("loss_dist" in stats)
                    if done >= 0:
                        events[m].append((e0, e1))
                        if "loss_dist" in stats:
                            dist.append(stats["loss_dist"])
            done += 4
        if has_key:
            ta.distortion_loss_weight = 0.0
        torch.cuda.synchronize()
        ms = {m: [x.elapsed_time(y) for x, y in v] for m, v in events.items()}
        steps[dtype] = {"ms_per_step_median": {m: round(statistics.median(v), 4) for m, v in ms.items()},
                        "ms_per_step_min": {m: round(min(v), 4) for m, v in ms.items()},
                        "timed_steps": len(ms["plain"])}
        if dist:
            steps[dtype]["loss_dist_first_last"] = [float(dist[0]), float(dist[-1])]
        print("step", dtype, json.dumps(steps[dtype]), flush=True)
        del stacks
        torch.cuda.empty_cache()
    if a.only_plain:
        print("PLAIN " + json.dumps({t: v["ms_per_step_median"]["plain"] for t, v in steps.items()}), flush=True)
        return

    # the two kernels alone, with and without the distortion: the same points either way
    torch.manual_seed(0)
    net = Network()
    net.load_state_dict(state, strict=True)
    net = net.to(dev)
    packer = net.model_fine.packer()
    kt = ops.KERNEL_TIMES
    per = {}
    for rep in range(a.warmup + a.steps):
        for mode in ("plain", "distortion"):
            kt.enabled = kt.detail = True
            kt.reset()
            out = ops.march_grad(packer, rays, 2.0, 6.0, grid.to(dev), dtype="fp32", distortion=mode == "distortion")
            loss = torch.nn.functional.mse_loss(out["rgb_map_f"], gt)
            if mode == "distortion":
                loss = loss + a.weight * out["dist_map_f"].mean()
            loss.backward()
            net.zero_grad()
            torch.cuda.synchronize()
            summary = kt.summary()
            kt.enabled = kt.detail = False
            if rep >= a.warmup:
                for name, (n, t_ms, units) in summary.items():
                    if name.startswith(SEG_KERNELS):
                        per.setdefault(name, []).append((1000.0 * t_ms / n, units // n))
    kt.reset()
    kernels = {name: {"us_median": round(statistics.median(x[0] for x in v), 2), "bytes": v[0][1],
                      "points": int(out["n_queried"]), "rays": int(rays.shape[0])} for name, v in sorted(per.items())}
    print("kernels", json.dumps(kernels), flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    result.update(device=torch.cuda.get_device_name(0), kernels=kernels,
                  step_cost={"rays": int(rays.shape[0]), "warmup": a.warmup, "weight": a.weight,
                             "timing": "HIP events around Trainer.train_step, weight 0 / --weight interleaved in "
                                       "blocks of 4, median", "tiers": steps})
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
