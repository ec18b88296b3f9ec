"""The occupancy grid of a training run, maintained from the live fine net
(``task_arg.train_grid: online``), so that ``train_renderer: accelerated`` can start from random
weights instead of a grid baked from a finished model.

State: a fp32 density per cell, in the march's (ix*res + iy)*res + iz order, and the uint8
occupancy the march reads (handed to the renderer as it is: no per-step conversion).  An update
  1. draws one jittered point inside each visited cell (nerf_grid_update_points),
  2. runs the density-only fused MLP on them, without grad, at the net's mlp_dtype,
  3. density[cell] = max(density[cell] * decay, relu(sigma))            (nerf_grid_update_apply),
  4. occupancy = density > min(threshold, mean(density))                (nerf_grid_update_threshold).
Cells are visited through a fixed bijection of [0, res^3), so a cell appears at most once per
update; the first ``warmup_updates`` updates visit every cell, later ones a rolling 1/period of
them.  ``step()`` is called once per training step and updates every ``interval`` steps, counted
by the grid itself (Trainer.global_step restarts at 0 on resume); update 0 runs before the first
march, so an all-occupied grid is never marched.  Seed, points and weights are the same on every
data-parallel rank, so every rank holds the same grid bit for bit with no collective.
"""
import torch

from nerf_amd import ops

DEFAULTS = {"interval": 16, "warmup_updates": 16, "period": 4, "decay": 0.95, "seed": 0}
SETTINGS = ("res", "threshold", "bbox", "interval", "warmup_updates", "period", "decay", "seed")


def grid_update_settings(task_arg) -> dict:
    """task_arg.grid_update.{interval, warmup_updates, period, decay, seed}, validated."""
    node = task_arg.get("grid_update", None) or {}
    unknown = sorted(set(node) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"task_arg.grid_update: unknown key(s) {unknown} (known: {sorted(DEFAULTS)})")
    out = {k: node.get(k, v) for k, v in DEFAULTS.items()}
    for k in ("interval", "warmup_updates", "period"):
        if isinstance(out[k], bool) or not isinstance(out[k], int) or out[k] < 1:
            raise ValueError(f"task_arg.grid_update.{k} must be an integer >= 1, got {out[k]!r}")
    if isinstance(out["seed"], bool) or not isinstance(out["seed"], int) or out["seed"] < 0:
        raise ValueError(f"task_arg.grid_update.seed must be an integer >= 0, got {out['seed']!r}")
    if isinstance(out["decay"], bool) or not isinstance(out["decay"], (int, float)) or not 0.0 < out["decay"] <= 1.0:
        raise ValueError(f"task_arg.grid_update.decay must be in (0, 1], got {out['decay']!r}")
    out["decay"] = float(out["decay"])
    return out


class OnlineGrid:
    def __init__(self, res, threshold, bbox, device="cpu", interval=16, warmup_updates=16, period=4, decay=0.95,
                 seed=0):
        self.res = int(res)
        if self.res < 2:
            raise ValueError(f"OnlineGrid: res must be >= 2, got {res}")
        self.threshold = float(threshold)
        self.bbox = (tuple(float(v) for v in bbox[0]), tuple(float(v) for v in bbox[1]))
        self.interval, self.warmup_updates, self.period = int(interval), int(warmup_updates), int(period)
        self.decay, self.seed = float(decay), int(seed)
        self.stride = ops.grid_update_stride(self.res)
        self.updates = 0  # updates done
        self.steps = 0    # training steps seen
        self.last_points = 0
        device = torch.device(device)
        r = self.res
        self.density = torch.zeros(r, r, r, dtype=torch.float32, device=device)
        self.grid = torch.ones(r, r, r, dtype=torch.uint8, device=device)
        self.workspace = None
        self.stats = None

    @property
    def device(self):
        return self.density.device

    def to(self, device):
        device = torch.device(device)
        if device != self.density.device:
            self.density = self.density.to(device)
            self.grid = self.grid.to(device)
            self.workspace = self.stats = None
        return self

    def slots(self, update=None):
        """(s0, n) of update ``update`` (default: the next one)."""
        return ops.grid_update_slots(self.updates if update is None else update, self.res, self.warmup_updates,
                                     self.period)

    def points(self, update=None):
        """cells [n] int32, pts [n,3] of update ``update`` (default: the next one)."""
        k = self.updates if update is None else int(update)
        s0, n = self.slots(k)
        return ops.grid_update_points(self.res, self.bbox, s0, n, k, self.seed, self.device, self.stride)

    def update(self, packer, dtype):
        """One update from the fine net's packed weights (the four steps of the module docstring)."""
        dev = self.device
        if self.workspace is None:
            self.workspace = torch.empty(ops.lib().nerf_grid_update_workspace_bytes(self.res), dtype=torch.uint8,
                                         device=dev)
            self.stats = torch.zeros(4, dtype=torch.int32, device=dev)
        cells, pts = self.points()
        self.last_points = int(cells.numel())
        if cells.numel():
            with torch.no_grad():
                raw = ops.mlp(packer, pts, None, 1, None, dtype, density_only=True)
            ops.grid_update_apply(self.density, cells, raw, self.decay)
        ops.grid_update_threshold(self.density, self.grid, self.threshold, self.workspace, self.stats)
        self.updates += 1

    def step(self, packer, dtype) -> bool:
        """Once per training step, before its march; True when it updated."""
        fired = self.steps % self.interval == 0
        if fired:
            self.update(packer, dtype)
        self.steps += 1
        return fired

    def summary(self):
        """(mean density, occupied fraction) of the last update -- a host read, for logging."""
        if self.stats is None:
            return 0.0, 1.0
        mean, occ = ops.grid_update_stats(self.stats)
        return mean, occ / float(self.res ** 3)

    def occupancy_bool(self):
        """The occupancy in the format of occupancy_grid.pt: a CPU bool [res,res,res]."""
        return self.grid.bool().cpu()

    def state_dict(self):
        sd = {k: getattr(self, k) for k in SETTINGS}
        sd["bbox"] = [list(self.bbox[0]), list(self.bbox[1])]
        sd.update(updates=self.updates, steps=self.steps, density=self.density.detach().cpu().clone(),
                  grid=self.grid.detach().cpu().clone())
        return sd

    def load_state_dict(self, sd):
        mine = self.state_dict()
        for k in SETTINGS:
            a, b = mine[k], sd[k]
            same = [list(map(float, v)) for v in a] == [list(map(float, v)) for v in b] if k == "bbox" else a == b
            if not same:
                raise ValueError(f"occupancy grid state: {k} is {b!r} in the file but {a!r} in this run's configuration")
        if tuple(sd["density"].shape) != (self.res,) * 3 or tuple(sd["grid"].shape) != (self.res,) * 3:
            raise ValueError("occupancy grid state: density / grid are not [res,res,res]")
        self.density = sd["density"].to(device=self.device, dtype=torch.float32).contiguous().clone()
        self.grid = sd["grid"].to(device=self.device, dtype=torch.uint8).contiguous().clone()
        self.updates, self.steps = int(sd["updates"]), int(sd["steps"])
