"""The online occupancy grid (task_arg.train_grid "online"): what its update costs, and how a
from-scratch run through the march converges against the hierarchical one.

    python tools/grid_train_bench.py [--tiers fp32,bf16x3f] [--out profiles/r8/online_grid.json]
    python tools/grid_train_bench.py --jitter [--out profiles/r10/march_jitter.json]
    python tools/grid_train_bench.py --distortion 0.001,0.01 [--out profiles/r11/distortion.json]
    python tools/grid_train_bench.py --background random [--out profiles/r13/random_background.json]

One process, HIP events on the compute stream, medians.

update      res 128, the trained fixture net (tests/golden/trained_v2.npz): a full update (every cell)
            and a rolling one (1 / period of the cells), per MLP tier.
step        Trainer.train_step on the golden_v2 ``rays4096`` batch from the trained fixture net, online
            mode (its own grid, past the warm-up: one rolling update per ``interval`` steps, the block's
            time divided by ``interval``) against the file-mode accelerated step on the fixture's baked
            grid, in interleaved blocks of ``interval`` steps.  Each mode trains its own copy of the net;
            the target is the fixture net's own march of those rays, so the net -- and with it the online
            grid -- stays the trained scene while the steps are timed.
convergence the procedural scene (src/datasets/nerf/synthetic.py), seed-0 init, the same ray stream:
            online-accelerated against hierarchical, held-out PSNR (4 views of 100x100; the online run
            rendered through the march with its live grid, the hierarchical one with render()) against
            the wall-clock spent in training steps (evaluation excluded), per tier.
--jitter    the convergence part alone, online-accelerated with task_arg.train_march_jitter off and on
            (same scene, seed, ray stream, steps and tiers), merged into --out under "convergence".
--distortion W[,W...]  the convergence part alone, online-accelerated with task_arg.distortion_loss_weight 0 and
            each W (same scene, seed, ray stream, steps and tiers), merged into --out under "convergence".
--background random  the convergence part alone, online-accelerated with task_arg.train_background white and
            random (the same scene with its alpha channel, seed, ray stream, steps and tiers; the held-out
            views stay composited on white), merged into --out under "convergence".
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "nerf-replication_amd"))
os.environ.setdefault("NERF_AMD_NO_ARGV", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

TIERS = ("fp32", "bf16x3", "bf16x3f", "bf16")


def med(v):
    return round(statistics.median(v), 4)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return e0, e1, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiers", default=",".join(TIERS))
    ap.add_argument("--convergence-tiers", default="fp32,bf16x3f")
    ap.add_argument("--reps", type=int, default=10, help="timed updates per kind and tier")
    ap.add_argument("--blocks", type=int, default=6, help="timed blocks of `interval` steps per mode")
    ap.add_argument("--steps", type=int, default=2000, help="convergence: training steps per run")
    ap.add_argument("--every", type=int, default=250, help="convergence: steps between held-out renders")
    ap.add_argument("--rays", type=int, default=4096, help="convergence: rays per step")
    ap.add_argument("--jitter", action="store_true",
                    help="convergence only: online-accelerated with train_march_jitter off and on")
    ap.add_argument("--distortion", default=None, metavar="W[,W...]",
                    help="convergence only: online-accelerated with distortion_loss_weight 0 and each W")
    ap.add_argument("--background", default=None, choices=("random",),
                    help="convergence only: online-accelerated with train_background white and random")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dist_weights = [float(w) for w in a.distortion.split(",")] if a.distortion else []
    if a.jitter + bool(dist_weights) + bool(a.background) > 1:
        ap.error("--jitter, --distortion and --background are separate runs")
    if any(not w > 0 for w in dist_weights):
        ap.error("--distortion takes positive weights (the run with the weight 0 is always made)")
    conv_only = a.jitter or bool(dist_weights) or bool(a.background)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", *(("r10", "march_jitter.json") if a.jitter else
                                                 ("r11", "distortion.json") if dist_weights else
                                                 ("r13", "random_background.json") if a.background else
                                                 ("r8", "online_grid.json")))
    from nerf_amd import ops
    from src.config import cfg
    from src.datasets.nerf.blender import Dataset
    from src.datasets.nerf.synthetic import camera_rays, make_scene, make_scene_rgba, psnr, shade, view_poses
    from src.models import make_network
    from src.models.nerf.network import Network
    from src.models.nerf.renderer.online_grid import DEFAULTS, OnlineGrid
    from src.models.nerf.renderer.volume_renderer import Renderer
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    from src.utils.camera import focal_for

    dev = torch.device("cuda:0")
    ta = cfg.task_arg
    gold = os.path.join(ROOT, "tests", "golden")
    z = np.load(os.path.join(gold, "trained_v2.npz"), allow_pickle=False)
    state = {k: torch.from_numpy(z[k]) for k in z.files}
    g2 = np.load(os.path.join(gold, "golden_v2.npz"), allow_pickle=False)
    baked = torch.from_numpy(np.unpackbits(g2["bake128_packed"])[: 128 ** 3].reshape(128, 128, 128).astype(bool))
    rays = torch.from_numpy(g2["rays4096"]).to(dev)
    near, far = ops.device_scalar(2.0, dev), ops.device_scalar(6.0, dev)
    bbox = (tuple(cfg.train_dataset.scene_bbox[0]), tuple(cfg.train_dataset.scene_bbox[1]))
    interval = int(DEFAULTS["interval"])
    result = {"device": torch.cuda.get_device_name(0), "grid_update": dict(DEFAULTS), "res": 128,
              "timing": "HIP events on the compute stream, medians", "update": {}, "step": {}, "convergence": {}}

    def fixture_net(dtype):
        torch.manual_seed(0)
        net = Network()
        net.load_state_dict(state, strict=True)
        net = net.to(dev)
        net.mlp_dtype = dtype
        return net

    def reset_modes():
        ta.train_renderer, ta.train_grid = "hierarchical", "file"

    with torch.no_grad():  # the step's target: the fixture net's own march through its baked grid
        gt = ops.march(fixture_net("fp32").model_fine.packer(), rays, 2.0, 6.0, baked, dtype="fp32")["rgb_map_f"]
    batch = {"rays": rays[None], "rgbs": gt[None], "near": near, "far": far}

    # ---- update cost ---------------------------------------------------------------------------------
    ta.perturb = 0
    for dtype in () if conv_only else a.tiers.split(","):
        packer = fixture_net(dtype).model_fine.packer()
        g = OnlineGrid(128, float(ta.occupancy_grid_threshold), bbox, dev, **DEFAULTS)
        for _ in range(2):
            g.update(packer, dtype)  # (warm: packs the weights, sizes the allocator's blocks)
        ev = {"full": [], "rolling": []}
        for kind in ev:
            for _ in range(a.reps):
                g.updates = 0 if kind == "full" else g.warmup_updates + (g.updates % g.period)
                e0, e1, _ = event_ms(lambda: g.update(packer, dtype))
                ev[kind].append((e0, e1, g.last_points))
        torch.cuda.synchronize()
        result["update"][dtype] = {k: {"ms_median": med([x.elapsed_time(y) for x, y, _ in v]), "points": v[-1][2]}
                                   for k, v in ev.items()}
        print("update", dtype, json.dumps(result["update"][dtype]), flush=True)

    # ---- the step, online (amortised) against file mode ----------------------------------------------
    for dtype in () if conv_only else a.tiers.split(","):
        ta.mlp_dtype = dtype
        stacks = {}
        for mode in ("file", "online"):
            net = fixture_net(dtype)
            ta.train_renderer, ta.train_grid = ("accelerated", "online") if mode == "online" else ("hierarchical", "file")
            trainer = make_trainer(cfg, net)
            if mode == "file":  # (the grid handed over directly: no logs/ file in a benchmark)
                trainer.network.train_renderer = "accelerated"
                trainer.network.renderer.set_occupancy_grid(baked, dev)
            stacks[mode] = (net, trainer, make_optimizer(cfg, net))
        reset_modes()
        grid = stacks["online"][1].network.online_grid.to(dev)
        for _ in range(grid.warmup_updates):  # past the warm-up: the timed blocks hold one rolling update each
            grid.update(stacks["online"][0].model_fine.packer(), dtype)
        grid.steps = 0
        for mode, (_, trainer, opt) in stacks.items():
            for _ in range(interval):
                trainer.train_step(dict(batch), opt)
        torch.cuda.synchronize()
        blocks = {m: [] for m in stacks}
        queried = {m: [] for m in stacks}
        for _ in range(a.blocks):
            for mode, (_, trainer, opt) in stacks.items():
                def run():
                    for _ in range(interval):
                        out, _, _ = trainer.train_step(dict(batch), opt)
                        queried[mode].append(out["n_queried"])
                e0, e1, _ = event_ms(run)
                blocks[mode].append((e0, e1))
        torch.cuda.synchronize()
        ms = {m: [x.elapsed_time(y) / interval for x, y in v] for m, v in blocks.items()}
        _, frac = grid.summary()
        result["step"][dtype] = {
            "rays": int(rays.shape[0]), "interval": interval,
            "ms_per_step_median": {m: med(v) for m, v in ms.items()},
            "ratio_online_over_file": round(statistics.median(ms["online"]) / statistics.median(ms["file"]), 4),
            "n_queried_median": {m: int(statistics.median(v)) for m, v in queried.items()},
            "occupied_fraction": {"file": round(float(baked.float().mean()), 4), "online": round(frac, 4)},
            "updates_in_timed_blocks": a.blocks}
        print("step", dtype, json.dumps(result["step"][dtype]), flush=True)
        del stacks
        torch.cuda.empty_cache()

    # ---- convergence from scratch --------------------------------------------------------------------
    # (with --background the views keep their alpha; composited on white they are make_scene's bit for bit)
    imgs, poses, focal = (make_scene_rgba if a.background else make_scene)(100, 100, 100, dev, seed=0)
    ev_poses = view_poses(4, seed=1).to(dev)
    held = []
    for k in range(ev_poses.shape[0]):
        o, d = camera_rays(ev_poses[k], 100, 100, focal_for(100))
        held.append((torch.cat([o, d], -1), shade(o, d)))
    white_db = float(np.mean([psnr(torch.ones_like(g), g) for _, g in held]))
    ta.train_rays = a.rays
    for dtype in a.convergence_tiers.split(","):
        result["convergence"][dtype] = {"rays_per_step": a.rays, "steps": a.steps, "all_white_psnr_db": round(white_db, 3)}
        modes = ("online_accelerated", "online_accelerated_jitter") if a.jitter else ("online_accelerated",
                                                                                      "hierarchical")
        if dist_weights:
            modes = ("online_accelerated",) + tuple(f"online_accelerated_distortion_{w:g}" for w in dist_weights)
        if a.background:
            modes = ("online_accelerated", "online_accelerated_background_random")
        for mode in modes:
            ta.mlp_dtype = dtype
            ta.train_background = "random" if mode.endswith("_background_random") else "white"
            ta.perturb = 1
            ta.train_march_jitter = mode == "online_accelerated_jitter"
            ta.distortion_loss_weight = float(mode.rsplit("_", 1)[1]) if "_distortion_" in mode else 0.0
            ta.train_renderer, ta.train_grid = ("accelerated", "online") if mode != "hierarchical" else ("hierarchical",
                                                                                                         "file")
            torch.manual_seed(0)
            net = make_network(cfg).to(dev)
            trainer = make_trainer(cfg, net)
            opt = make_optimizer(cfg, net)
            ds = Dataset.from_arrays(imgs, poses, focal)  # same seed: the same ray stream in both modes
            plain = Renderer(net)

            def heldout():
                ta.perturb = 0
                ps = []
                with torch.no_grad():
                    for rr, g in held:
                        b = {"rays": rr, "rgbs": g, "near": near, "far": far}
                        out = trainer.network(b)[0] if mode != "hierarchical" else plain.render(b)
                        ps.append(psnr(out["rgb_map_f"], g))
                ta.perturb = 1
                return float(np.mean(ps))

            curve, train_s, queried = [], 0.0, []
            for s0 in range(0, a.steps, a.every):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(min(a.every, a.steps - s0)):
                    r, c, *bg = ds.sample_batch()
                    b = {"rays": r[None], "rgbs": c[None], "near": near, "far": far}
                    if bg:
                        b["bg"] = bg[0][None]
                    out, _, _ = trainer.train_step(b, opt)
                torch.cuda.synchronize()
                train_s += time.perf_counter() - t0
                if "n_queried" in out:
                    queried.append(out["n_queried"])
                curve.append({"step": min(s0 + a.every, a.steps), "train_seconds": round(train_s, 3),
                              "psnr_db": round(heldout(), 3)})
            rec = {"curve": curve, "ms_per_step_mean": round(1000.0 * train_s / a.steps, 4)}
            if mode != "hierarchical":
                _, frac = trainer.network.online_grid.summary()
                rec.update(occupied_fraction_final=round(frac, 4), n_queried_at_checkpoints=queried)
            result["convergence"][dtype][mode] = rec
            print("convergence", dtype, mode, json.dumps(rec), flush=True)
            del net, trainer, opt
            torch.cuda.empty_cache()
    reset_modes()
    ta.train_march_jitter = False
    ta.distortion_loss_weight = 0.0
    ta.train_background = "white"

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    if conv_only:  # the file also holds the cost measurements of other tools: only this part is replaced
        conv = result["convergence"]
        result = json.load(open(a.out)) if os.path.exists(a.out) else {}
        result.update(device=torch.cuda.get_device_name(0), convergence=conv)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
