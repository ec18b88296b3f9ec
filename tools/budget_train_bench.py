"""The point budget (task_arg.point_budget): does a ray count that follows the occupancy buy
training rays per second, and PSNR at equal training time, over the fixed train_rays?

    python tools/budget_train_bench.py [--tiers fp32,bf16x3f] [--out profiles/r9/point_budget.json]

One process, the procedural scene (src/datasets/nerf/synthetic.py), seed-0 init, train_grid online,
per MLP tier:

run A   fixed ``--rays`` (4096) rays per step, ``--steps`` (2000) steps.
run B   point_budget.target ``--target`` (262144; the cap at its default, twice the target), from the
        same ray count, for the same TRAINING TIME as run A: it stops at the first time check (every
        ``--check`` steps) at which its time in training steps has reached run A's.

Time is the time in training steps: HIP events on the compute stream around blocks of ``--check``
steps, summed; the held-out renders are outside the blocks.  Both runs are made here, in this
process, one after the other, after a throwaway warm-up of both modes (code objects, allocator);
nothing is copied from an earlier file.  Per checkpoint (every ``--every`` steps, and at the end):
seconds in training, step, the last step's rays / points queried / points differentiated / rays
kept, held-out PSNR of 4 views of 100x100 through the march with the live grid.  Over the run: mean
rays per second, mean ms per step, the steps in which the cap dropped rays, and (run B) the ray count
of every 16th step.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "nerf-replication_amd"))
os.environ.setdefault("NERF_AMD_NO_ARGV", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiers", default="fp32,bf16x3f")
    ap.add_argument("--steps", type=int, default=2000, help="run A: training steps")
    ap.add_argument("--every", type=int, default=250, help="steps between held-out renders")
    ap.add_argument("--check", type=int, default=25, help="steps per timed block (run B checks its time after each)")
    ap.add_argument("--rays", type=int, default=4096, help="run A's rays per step, run B's first count")
    ap.add_argument("--target", type=int, default=262144, help="run B: point_budget.target")
    ap.add_argument("--warmup", type=int, default=20, help="throwaway steps per mode before the runs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r9", "point_budget.json"))
    a = ap.parse_args()
    if a.every % a.check or a.steps % a.check:
        ap.error("--every and --steps must be multiples of --check")
    from nerf_amd import ops
    from src.config import cfg
    from src.datasets.nerf.blender import Dataset
    from src.datasets.nerf.synthetic import camera_rays, make_scene, psnr, shade, view_poses
    from src.models import make_network
    from src.models.nerf.renderer.ray_budget import DEFAULTS
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    from src.utils.camera import focal_for

    dev = torch.device("cuda:0")
    ta = cfg.task_arg
    near, far = ops.device_scalar(2.0, dev), ops.device_scalar(6.0, dev)
    imgs, poses, focal = make_scene(100, 100, 100, dev, seed=0)
    ev_poses = view_poses(4, seed=1).to(dev)
    held = []
    for k in range(ev_poses.shape[0]):
        o, d = camera_rays(ev_poses[k], 100, 100, focal_for(100))
        held.append((torch.cat([o, d], -1), shade(o, d)))
    white_db = float(np.mean([psnr(torch.ones_like(g), g) for _, g in held]))
    budget_node = dict(DEFAULTS, target=a.target)
    result = {"command": " ".join([os.path.basename(sys.executable)] + sys.argv),
              "device": torch.cuda.get_device_name(0),
              "timing": "HIP events on the compute stream around blocks of --check training steps, summed; "
                        "held-out renders excluded; both runs in this process after a warm-up of both modes",
              "scene": "procedural, 100 views of 100x100; held-out: 4 views", "all_white_psnr_db": round(white_db, 3),
              "run_A": {"rays": a.rays, "steps": a.steps}, "run_B": {"point_budget": budget_node}, "tiers": {}}
    ta.train_rays = a.rays
    ta.train_renderer, ta.train_grid = "accelerated", "online"

    def run(dtype, budgeted, steps=None, seconds=None):
        """steps: that many; seconds: until the time in training reaches it."""
        ta.mlp_dtype = dtype
        ta.perturb = 1
        ta.point_budget = dict(budget_node) if budgeted else {"target": 0}
        torch.manual_seed(0)
        net = make_network(cfg).to(dev)
        trainer = make_trainer(cfg, net)
        opt = make_optimizer(cfg, net)
        ds = Dataset.from_arrays(imgs, poses, focal)
        budget = trainer.network.ray_budget
        assert (budget is not None) == budgeted

        def heldout():
            ta.perturb = 0
            with torch.no_grad():
                ps = [psnr(trainer.network({"rays": rr, "rgbs": g, "near": near, "far": far})[0]["rgb_map_f"], g)
                      for rr, g in held]
            ta.perturb = 1
            return float(np.mean(ps))

        curve, traj = [], []
        step, train_s, total_rays, dropped = 0, 0.0, 0, 0
        while (steps is not None and step < steps) or (seconds is not None and train_s < seconds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.check):
                n = budget.rays if budgeted else a.rays
                r, c = ds.sample_batch(n_rays=n)
                out, _, _ = trainer.train_step({"rays": r[None], "rgbs": c[None], "near": near, "far": far}, opt)
                kept = out.get("rays_kept", n)
                total_rays += n
                dropped += kept < n
                if budgeted and step % 16 == 0:
                    traj.append(n)
                step += 1
            e1.record()
            e1.synchronize()
            train_s += e0.elapsed_time(e1) / 1000.0
            done = (steps is not None and step >= steps) or (seconds is not None and train_s >= seconds)
            if step % a.every == 0 or done:
                curve.append({"step": step, "train_seconds": round(train_s, 3), "rays": n,
                              "points_queried": out["n_queried"], "points": out.get("n_points", out["n_queried"]),
                              "rays_kept": kept, "psnr_db": round(heldout(), 3)})
        _, frac = trainer.network.online_grid.summary()
        rec = {"steps": step, "train_seconds": round(train_s, 3), "rays_per_second_mean": round(total_rays / train_s, 1),
               "ms_per_step_mean": round(1000.0 * train_s / step, 4), "rays_per_step_mean": round(total_rays / step, 1),
               "steps_the_cap_dropped_rays": int(dropped), "occupied_fraction_final": round(frac, 4),
               "psnr_db_final": curve[-1]["psnr_db"], "curve": curve}
        if budgeted:
            rec["rays_every_16th_step"] = traj
        del net, trainer, opt
        torch.cuda.empty_cache()
        return rec

    for dtype in a.tiers.split(","):
        for budgeted in (False, True):  # (thrown away: code objects loaded, the allocator's blocks sized)
            run(dtype, budgeted, steps=max(a.check, a.warmup // a.check * a.check))
        rec_a = run(dtype, False, steps=a.steps)
        print("A", dtype, json.dumps({k: v for k, v in rec_a.items() if k != "curve"}), flush=True)
        rec_b = run(dtype, True, seconds=rec_a["train_seconds"])
        print("B", dtype, json.dumps({k: v for k, v in rec_b.items() if k not in ("curve", "rays_every_16th_step")}),
              flush=True)
        result["tiers"][dtype] = {
            "A_fixed_rays": rec_a, "B_point_budget": rec_b,
            "B_over_A": {"rays_per_second": round(rec_b["rays_per_second_mean"] / rec_a["rays_per_second_mean"], 4),
                         "psnr_db_at_equal_time": round(rec_b["psnr_db_final"] - rec_a["psnr_db_final"], 3),
                         "train_seconds": round(rec_b["train_seconds"] / rec_a["train_seconds"], 4)}}
    ta.point_budget = {"target": 0}
    ta.train_renderer, ta.train_grid = "hierarchical", "file"

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
