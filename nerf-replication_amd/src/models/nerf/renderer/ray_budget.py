"""The ray count of a training step that follows the occupancy (``task_arg.point_budget``), so that
the points a step of ``train_renderer: accelerated`` composites stay near a target.

``task_arg.train_rays`` fixes the rays of a step, but the cost and the memory of the accelerated step
follow the points the march composites, and those fall by more than 3x while the grid prunes.  With
``point_budget.target > 0`` the trainer observes every step's (rays marched, points queried) and
draws the next batch with

    want = max_rays                     if n_queried == 0 else (target * n_rays) // n_queried
    want = min(max(want, n_rays // 2), 2 * n_rays)            # at most a factor 2 per step
    next = min(max((want // granularity) * granularity, min_rays), max_rays)

rays -- integers only, so the trajectory is the same on every host.  ``max_points`` (0: twice the
target) is the hard cap of the differentiable pass of one step (ops.march_grad(max_points=)): rays
past it are marched but dropped from the loss.  No smoothing beyond the factor 2: the mean over
thousands of rays is steady, and the grid changes it only every ``grid_update.interval`` steps.

Pure Python (no torch): the controller is a few integers.
"""
import math

DEFAULTS = {"target": 0, "max_points": 0, "min_rays": 1024, "max_rays": 32768, "granularity": 256}


def march_steps(near, far, step_size) -> int:
    """Steps of the march's t table, torch.arange(near, far, step_size): ceil((far - near) / step) in double."""
    return int(math.ceil((float(far) - float(near)) / float(step_size)))


def point_budget_settings(task_arg) -> dict:
    """task_arg.point_budget.{target, max_points, min_rays, max_rays, granularity}, validated."""
    node = task_arg.get("point_budget", None) or {}
    unknown = sorted(set(node) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"task_arg.point_budget: unknown key(s) {unknown} (known: {sorted(DEFAULTS)})")
    out = {k: node.get(k, v) for k, v in DEFAULTS.items()}
    for k, low in (("target", 0), ("max_points", 0), ("min_rays", 1), ("max_rays", 1), ("granularity", 1)):
        if isinstance(out[k], bool) or not isinstance(out[k], int) or out[k] < low:
            raise ValueError(f"task_arg.point_budget.{k} must be an integer >= {low}, got {out[k]!r}")
    for k in ("min_rays", "max_rays"):
        if out[k] % out["granularity"]:
            raise ValueError(f"task_arg.point_budget.{k} must be a multiple of granularity "
                             f"({out['granularity']}), got {out[k]}")
    if out["min_rays"] > out["max_rays"]:
        raise ValueError(f"task_arg.point_budget.min_rays ({out['min_rays']}) exceeds max_rays ({out['max_rays']})")
    return out


class RayBudget:
    def __init__(self, target, max_points=0, min_rays=1024, max_rays=32768, granularity=256, train_rays=4096,
                 n_steps=0):
        """``n_steps``: the march's step count -- one ray alone can need that many points, so a smaller
        cap could keep no ray at all (ops.march_grad refuses it)."""
        s = point_budget_settings({"point_budget": dict(target=target, max_points=max_points, min_rays=min_rays,
                                                        max_rays=max_rays, granularity=granularity)})
        if s["target"] < 1:
            raise ValueError(f"task_arg.point_budget.target must be >= 1 for a RayBudget, got {target!r}")
        self.target, self.min_rays, self.max_rays, self.granularity = (s[k] for k in ("target", "min_rays", "max_rays",
                                                                                      "granularity"))
        self.max_points = s["max_points"] or 2 * self.target
        if self.max_points < int(n_steps):
            raise ValueError(f"task_arg.point_budget.max_points ({self.max_points}) is below the march's "
                             f"{int(n_steps)} steps: one ray alone can need that many points")
        if self.max_points > 2 ** 31 - 1:
            raise ValueError(f"task_arg.point_budget.max_points ({self.max_points}) exceeds 2^31 - 1")
        self.rays = self._clamp(int(train_rays))
        self.observations = 0

    @classmethod
    def from_config(cls, task_arg):
        """The controller of a configuration, or None when point_budget.target is 0 (off)."""
        s = point_budget_settings(task_arg)
        if s["target"] == 0:
            return None
        renderer = str(task_arg.get("train_renderer", "hierarchical") or "hierarchical")
        if renderer != "accelerated":
            raise ValueError("task_arg.point_budget.target > 0 budgets the points of train_renderer: accelerated; "
                             f"with train_renderer: {renderer} the points per ray are fixed")
        n_steps = march_steps(task_arg.get("near", 2.0), task_arg.get("far", 6.0),
                              task_arg.get("render_step_size", 0.005))
        return cls(train_rays=int(task_arg.get("train_rays", 4096)), n_steps=n_steps, **s)

    def _clamp(self, want):
        g = self.granularity
        return min(max((want // g) * g, self.min_rays), self.max_rays)

    def observe(self, n_rays, n_queried):
        """One training step marched ``n_rays`` rays and queried ``n_queried`` points -> the next ray count."""
        n_rays, n_queried = int(n_rays), int(n_queried)
        want = self.max_rays if n_queried == 0 else (self.target * n_rays) // n_queried
        want = min(max(want, n_rays // 2), 2 * n_rays)
        self.rays = self._clamp(want)
        self.observations += 1
        return self.rays

    def state_dict(self):
        return {"rays": self.rays, "observations": self.observations}

    def load_state_dict(self, sd):
        rays = int(sd["rays"])
        if rays != self._clamp(rays):
            raise ValueError(f"ray budget state: {rays} rays is not a count this run's point_budget allows "
                             f"(min_rays {self.min_rays}, max_rays {self.max_rays}, granularity {self.granularity})")
        self.rays, self.observations = rays, int(sd["observations"])
