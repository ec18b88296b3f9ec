"""What the mesh export costs: the density field against the surface extraction.

    python tools/mesh_bench.py [--res 128,256] [--tiers fp32,bf16] [--reps 9] [--out profiles/r15/mesh.json]

One process, one GPU, the trained fixture net (tests/golden/trained_v2.npz, fine net) on the lego box at level
32.  Per resolution: ops.mesh_field per MLP tier, and on the fp32 field the three stages of ops.mesh_extract
(classify kernel, the two torch.cumsum scans with their subtractions, emit kernel), each between two HIP
events, median of --reps after two warm-up rounds; ops.mesh_extract as a whole (with its host read) on a host
clock around a synchronise.  The kernels' algorithmic bytes (what they must read and write, from the shapes
and V, F) over their time is given as a fraction of the 6.3 TB/s a device copy reaches.
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

COPY_BYTES_PER_S = 6.3e12
LEVEL = 32.0


def event_ms(fn, reps, warmup=2):
    """(median ms, min ms, last result) of fn between two HIP events."""
    out = None
    for _ in range(warmup):
        out = fn()
    ev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return round(statistics.median(ms), 4), round(min(ms), 4), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", default="128,256")
    ap.add_argument("--tiers", default="fp32,bf16")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "mesh.json"))
    a = ap.parse_args()
    from nerf_amd import ops

    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "trained_v2.npz"), allow_pickle=False)
    packer = ops.PackedMLP([torch.from_numpy(z[f"model_fine.{n}"]).to(dev) for n in ops.NET_PARAM_NAMES])
    box = ops.SCENE_BBOX
    result = {"device": torch.cuda.get_device_name(0), "level": LEVEL, "net": "trained_v2 fine", "reps": a.reps,
              "timing": "HIP events around each stage, median (min) of reps after 2 warm-up rounds; extract_total_ms "
                        "is a host clock around ops.mesh_extract and a synchronise (it holds the one host read)",
              "copy_bytes_per_s": COPY_BYTES_PER_S, "resolutions": {}}
    for N in (int(r) for r in a.res.split(",")):
        shape = (N, N, N)
        P, C = N ** 3, (N - 1) ** 3
        row = {"points": P, "field_ms": {}}
        for tier in a.tiers.split(","):
            med, lo, _ = event_ms(lambda: ops.mesh_field(packer, shape, box, tier), a.reps)
            row["field_ms"][tier] = {"median": med, "min": lo}
        field = ops.mesh_field(packer, shape, box, "fp32")
        c_med, c_min, (mask, vcount, tcount) = event_ms(lambda: ops.mesh_classify(field, LEVEL), a.reps)
        s_med, s_min, (voff, toff, totals) = event_ms(lambda: ops.mesh_scan(vcount, tcount), a.reps)
        V, F = totals.tolist()
        e_med, e_min, _ = event_ms(lambda: ops.mesh_emit(field, LEVEL, box, mask, voff, toff, V, F), a.reps)
        wall = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.mesh_extract(field, LEVEL, box)
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
        classify_bytes = 4 * P + P + 4 * P + 4 * C
        emit_bytes = 4 * P + P + 8 * P + 8 * C + 12 * V + 12 * F
        row.update(V=V, F=F,
                   classify_ms={"median": c_med, "min": c_min}, scan_ms={"median": s_med, "min": s_min},
                   emit_ms={"median": e_med, "min": e_min},
                   extract_stages_ms=round(c_med + s_med + e_med, 4),
                   extract_total_ms={"median": round(statistics.median(wall), 4), "min": round(min(wall), 4)},
                   classify_bytes=classify_bytes, emit_bytes=emit_bytes,
                   classify_fraction_of_copy=round(classify_bytes / (c_med * 1e-3) / COPY_BYTES_PER_S, 4),
                   emit_fraction_of_copy=round(emit_bytes / (e_med * 1e-3) / COPY_BYTES_PER_S, 4))
        result["resolutions"][str(N)] = row
        print(N, json.dumps(row), flush=True)
        del field, mask, vcount, tcount, voff, toff
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
