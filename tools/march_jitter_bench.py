"""What jittered march steps (task_arg.train_march_jitter) cost the accelerated training step.

    python tools/march_jitter_bench.py [--steps 48] [--tiers fp32,bf16x3f] [--out profiles/r10/march_jitter.json]

One process, the trained fixture net (tests/golden/trained_v2.npz) and its res-128 bake, the golden_v2
``rays4096`` batch, as tools/march_train_bench.py: ``Trainer.train_step`` of the accelerated mode with the
key off and on, interleaved in blocks of 4 steps, each step between two HIP events, median after a warm-up
(each mode trains its own copy of the net); and the jitter launch alone (ops.march_jitter, 4,096 rays), HIP
events around blocks of 100 launches.  The result is merged into --out under "jittered_step" /
"jitter_launch".
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tiers", default="fp32,bf16x3f")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "march_jitter.json"))
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

    def stack(dtype):
        torch.manual_seed(0)
        net = Network()
        net.load_state_dict(state, strict=True)
        net = net.to(dev)
        net.mlp_dtype = dtype
        trainer = make_trainer(cfg, net)
        trainer.network.train_renderer = "accelerated"  # (the grid handed over directly: no logs/ file)
        trainer.network.renderer.set_occupancy_grid(grid, dev)
        return net, trainer, make_optimizer(cfg, net)

    steps = {}
    for dtype in a.tiers.split(","):
        ta.mlp_dtype = dtype
        stacks = {m: stack(dtype) for m in ("fixed", "jittered")}
        events = {m: [] for m in stacks}
        queried = {m: [] for m in stacks}
        done = -a.warmup
        while done < a.steps:
            for m, (_, trainer, opt) in stacks.items():
                ta.train_march_jitter = m == "jittered"  # (the renderer reads the key at every step)
                for _ in range(4):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out, _, _ = trainer.train_step(dict(batch), opt)
                    e1.record()
                    assert ("t_shift" in out) == (m == "jittered")
                    if done >= 0:
                        events[m].append((e0, e1))
                        queried[m].append(out["n_queried"])
            done += 4
        ta.train_march_jitter = False
        torch.cuda.synchronize()
        ms = {m: [x.elapsed_time(y) for x, y in v] for m, v in events.items()}
        steps[dtype] = {"ms_per_step_median": {m: round(statistics.median(v), 4) for m, v in ms.items()},
                        "ms_per_step_min": {m: round(min(v), 4) for m, v in ms.items()},
                        "n_queried_median": {m: int(statistics.median(v)) for m, v in queried.items()},
                        "timed_steps": len(ms["fixed"])}
        print("step", dtype, json.dumps(steps[dtype]), flush=True)
        del stacks
        torch.cuda.empty_cache()

    blocks = []
    for rep in range(12):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(100):
            ops.march_jitter(4096, 0.005, 1234, 4 * (100 * rep + k), dev)
        e1.record()
        blocks.append((e0, e1))
    torch.cuda.synchronize()
    us = [1000.0 * x.elapsed_time(y) / 100 for x, y in blocks[2:]]
    launch = {"rays": 4096, "us_per_launch_median": round(statistics.median(us), 3),
              "timing": "HIP events around 100 back-to-back launches (allocation of the output included), 10 blocks"}
    print("jitter launch", json.dumps(launch), flush=True)

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}
    result.update(device=torch.cuda.get_device_name(0), jitter_launch=launch,
                  jittered_step={"rays": int(rays.shape[0]), "warmup": a.warmup,
                                 "timing": "HIP events around Trainer.train_step, key off / on interleaved in "
                                           "blocks of 4, median", "tiers": steps})
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
