"""The training step through the occupancy-grid march against the hierarchical one.

    python tools/march_train_bench.py [--steps 24] [--warmup 5] [--out profiles/r7/march_train.json] [--lib PATH]

One process, the trained fixture net (tests/golden/trained_v2.npz) and its res-128 bake, the
golden_v2 ``rays4096`` batch.  For each MLP tier (fp32, bf16x3, bf16x3f, bf16) it times
``Trainer.train_step`` with ``task_arg.train_renderer`` hierarchical and accelerated, interleaved
(blocks of 4 steps, alternating, so clock drift hits both alike), each step between two HIP events on
the compute stream, after a warm-up; the figure is the median over the timed steps.  The two modes
train their own copy of the net (the steps update the weights).

For the accelerated step it also reports n_queried / n_evaluated and the split into pass A (the
no-grad march), the segment gather (prefix sum + nerf_march_segments), the MLP forward, the segment
compositing, and in the backward the compositing and the MLP (dX + dW): pass A and the gather between
events around the ops calls, the kernels from ops.KERNEL_TIMES; medians over ``--split-reps`` runs.
And an A/B of pass A's k_schedule (its rounds are launch-bound at 4096 rays): forward + backward of
ops.march_grad under several schedules, interleaved; the steps above run the renderer's own
(TRAIN_K_SCHEDULE of volume_renderer.py, or task_arg.train_k_schedule).
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

TIERS = ("fp32", "bf16x3", "bf16x3f", "bf16")
# pass A's k_schedule A/B: the inference default, two coarser ones (k96 = Renderer's TRAIN_K_SCHEDULE), one round
SCHEDULES = {"inference": (12, 24, 48, 96, 192, 384, 768), "k48": (48, 96, 192, 384, 768), "k96": (96, 384, 768),
             "k800": (800,)}


def med(v):
    return round(statistics.median(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--split-reps", type=int, default=10)
    ap.add_argument("--tiers", default=",".join(TIERS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r7", "march_train.json"))
    ap.add_argument("--lib", default=None, help="alternative build of libnerf_amd.so")
    a = ap.parse_args()
    from nerf_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    from nerf_amd import ops
    from src.config import cfg
    from src.models.nerf.network import Network
    from src.models.nerf.renderer.volume_renderer import TRAIN_K_SCHEDULE
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
    cfg.task_arg.perturb = 0
    cfg.task_arg.train_renderer = "hierarchical"
    result = {"device": torch.cuda.get_device_name(0), "rays": int(rays.shape[0]), "steps": a.steps,
              "train_k_schedule": list(TRAIN_K_SCHEDULE),
              "warmup": a.warmup, "timing": "HIP events around Trainer.train_step, interleaved blocks of 4, median",
              "tiers": {}}

    def stack(mode, dtype):
        torch.manual_seed(0)
        net = Network()
        net.load_state_dict(state, strict=True)
        net = net.to(dev)
        net.mlp_dtype = dtype
        trainer = make_trainer(cfg, net)
        if mode == "accelerated":  # (the grid handed over directly: no logs/ file in a benchmark)
            trainer.network.train_renderer = "accelerated"
            trainer.network.renderer.set_occupancy_grid(grid, dev)
        return net, trainer, make_optimizer(cfg, net)

    def timed_step(trainer, opt):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out, _, _ = trainer.train_step(dict(batch), opt)
        e1.record()
        return e0, e1, out

    for dtype in a.tiers.split(","):
        cfg.task_arg.mlp_dtype = dtype
        stacks = {m: stack(m, dtype) for m in ("hierarchical", "accelerated")}
        for m, (_, trainer, opt) in stacks.items():
            for _ in range(a.warmup):
                trainer.train_step(dict(batch), opt)
        torch.cuda.synchronize()
        events = {m: [] for m in stacks}
        counts = []
        done = 0
        while done < a.steps:
            for m, (_, trainer, opt) in stacks.items():
                for _ in range(4):
                    e0, e1, out = timed_step(trainer, opt)
                    events[m].append((e0, e1))
                    if m == "accelerated":
                        counts.append((out["n_queried"], out["n_evaluated"]))
            done += 4
        torch.cuda.synchronize()
        ms = {m: [x.elapsed_time(y) for x, y in v] for m, v in events.items()}
        tier = {"ms_per_step_median": {m: med(v) for m, v in ms.items()},
                "ms_per_step_min": {m: round(min(v), 4) for m, v in ms.items()},
                "ratio_accelerated_over_hierarchical": round(statistics.median(ms["accelerated"])
                                                             / statistics.median(ms["hierarchical"]), 4),
                "n_queried": int(statistics.median(c[0] for c in counts)),
                "n_evaluated": int(statistics.median(c[1] for c in counts))}

        # ---- the accelerated step's split, on the accelerated copy at its current weights
        net, trainer, opt = stacks["accelerated"]
        packer = net.model_fine.packer()
        r = trainer.network.renderer
        ta = cfg.task_arg
        kw = dict(step_size=float(ta.render_step_size), t_thresh=float(ta.transmittance_threshold),
                  bbox=r._bbox_tuple(), white_bkgd=bool(ta.white_bkgd), dtype=dtype)
        split = {}
        ops.KERNEL_TIMES.enabled = ops.KERNEL_TIMES.detail = True
        for rep in range(a.split_reps + 2):
            ops.KERNEL_TIMES.reset()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            opt.zero_grad()
            ev[0].record()
            with torch.no_grad():
                out, walk = ops._march(packer, rays, 2.0, 6.0, r.occupancy_grid, t_table=None,
                                       k_schedule=TRAIN_K_SCHEDULE, round_bytes=1 << 31, use_macro=True,
                                       return_used=True, **kw)
            ev[1].record()
            rays_c, t_tab, _, g8, _, macro, vd = walk
            seg_off = torch.zeros(rays_c.shape[0] + 1, dtype=torch.int32, device=dev)
            seg_off[1:] = torch.cumsum(out["ray_used"], 0, dtype=torch.int32)
            out_ray, out_step, out_pts = ops.march_segments(rays_c, t_tab, g8, macro, seg_off, out["n_queried"],
                                                            kw["bbox"])
            ev[2].record()
            raw = ops.mlp(packer, out_pts, vd, 1, out_ray, dtype)
            rgb, _, _ = ops._MarchSegComposite.apply(raw, rays_c, t_tab, seg_off, out_step, kw["step_size"], True)
            _, _, total = ops.mse_pair(rgb, None, gt)
            with ops.direct_grad():
                total.backward()
            torch.cuda.synchronize()
            if rep < 2:
                continue
            kt = {k: v[1] for k, v in ops.KERNEL_TIMES.summary().items()}
            parts = {"pass_a": ev[0].elapsed_time(ev[1]), "gather": ev[1].elapsed_time(ev[2]),
                     "mlp_forward": kt.get("mlp_fwd_train", 0.0),
                     "composite": kt.get("march_seg_composite_fwd", 0.0),
                     "composite_backward": kt.get("march_seg_composite_bwd", 0.0),
                     "mlp_backward": kt.get("mlp_bwd_dx", 0.0) + kt.get("mlp_bwd_dw", 0.0)}
            for k, v in parts.items():
                split.setdefault(k, []).append(v)
            split.setdefault("rounds_launched", []).append(out["rounds_launched"])
        ops.KERNEL_TIMES.enabled = ops.KERNEL_TIMES.detail = False
        ops.KERNEL_TIMES.reset()
        tier["accelerated_split_ms"] = {k: med(v) for k, v in split.items()}

        # ---- pass A's k_schedule, forward + backward of ops.march_grad, interleaved
        ab = {k: [] for k in SCHEDULES}
        for rep in range(a.split_reps + 2):
            for name, sched in SCHEDULES.items():
                opt.zero_grad()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                o = ops.march_grad(packer, rays, 2.0, 6.0, r.occupancy_grid, k_schedule=sched, **kw)
                _, _, total = ops.mse_pair(o["rgb_map_f"], None, gt)
                with ops.direct_grad():
                    total.backward()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    ab[name].append((e0.elapsed_time(e1), o["n_evaluated"], o["rounds_launched"]))
        tier["k_schedule_ab"] = {k: {"schedule": list(SCHEDULES[k]), "fwd_bwd_ms_median": med([x[0] for x in v]),
                                     "n_evaluated": v[-1][1], "rounds_launched": v[-1][2]} for k, v in ab.items()}
        result["tiers"][dtype] = tier
        print(dtype, json.dumps(tier), flush=True)
        del stacks
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
