"""Drop-in ``loss_module`` (reference: src/train/trainers/nerf.py:6-50).

NetworkWrapper(net, train_loader).forward(batch) -> (ret, loss, {loss_c, loss_f, total_loss})
with loss = MSE(rgb_map_c, gt) + MSE(rgb_map_f, gt).  Like the reference it builds its
Renderer from this module path directly (nerf.py:3,10), so the drop-in renderer must live
at src.models.nerf.renderer.volume_renderer.

``task_arg.train_renderer: accelerated`` (default ``hierarchical``: the above) trains the fine
net through the occupancy-grid march instead (Renderer.render_accelerated under autograd):
loss = MSE(rgb_map_f, gt), stats {loss_f, total_loss}; the coarse net is not evaluated and
receives a zero gradient.  The grid comes from logs/<cfg name>/occupancy_grid.pt (what
occupancy_grid.py writes and run.py evaluate loads); a missing file is an error, never a
fall-back to the hierarchical render.  Without grad (validation) forward() keeps render().

``task_arg.train_grid: online`` (default ``file``: the above; only with ``train_renderer:
accelerated``) needs no grid file: the module owns an OnlineGrid for the FINE net (the net the
march queries; the coarse net is not trained in this mode), updated from the live weights every
``task_arg.grid_update.interval`` steps, so a run can start from random weights.  Validation
(no grad) then also goes through render_accelerated with the live grid -- an untrained coarse
net would make render()'s importance sampling meaningless -- with stats {loss_f, total_loss}.
save_grid() / load_grid() write and read the grid beside the checkpoints (train.py).

``task_arg.point_budget.target > 0`` (default 0: off; only with ``train_renderer: accelerated``, either
``train_grid``) lets the ray count follow the occupancy: the module owns a RayBudget (``.ray_budget``),
every training forward marches its whole batch as one call capped at ``max_points`` differentiated
points (rays past the cap are marched but left out of the loss: MSE over the first ``rays_kept`` rows),
reports stats {loss_f, total_loss, rays, points}, observes (rays marched, points queried) and sets the
loader's dataset.batch_rays, so the batch Trainer.train_step prefetches next has the new count.  Without
a loader the caller reads ``.ray_budget.rays``.  Validation is untouched.  Data parallel: every rank
follows its own count with no collective, so the all-reduce averages per-rank MEAN gradients of
different ray counts (each rank weighs 1 / world, not its rays); the online grids stay bit-identical
(they depend on the weights only).  save_grid() / load_grid() also carry the count
(<model_dir>/ray_budget_state.pt).

``task_arg.train_march_jitter: true`` (default false; only with ``train_renderer: accelerated``, either
``train_grid``, with or without a point budget) shifts every ray's march steps by a random fraction of a
step in each training forward (Renderer._render_accelerated_grad; ret["t_shift"]).  Validation and every
other no-grad march keep the fixed steps.  The renderer's seed contains the rank, so ranks draw different
shifts; the stream restarts with the renderer's call counter on resume, as the ``perturb`` stream does.

``task_arg.distortion_loss_weight: W`` (float >= 0, default 0.0; positive only with ``train_renderer:
accelerated``, either ``train_grid``, with or without a point budget or jitter) adds Mip-NeRF 360's
distortion of each ray's compositing weights to the training loss: loss = MSE + W * mean(dist_map_f),
the mean over the rays the MSE runs over (the first ``rays_kept`` under a point budget), stats gain
``loss_dist`` (the unweighted mean).  Per rank, like the MSE: no collective.  Exactly 0 computes nothing:
every launch, output and stats key is what it was.  Validation never computes it.

``task_arg.train_background: random`` (default ``white``; only with ``train_renderer: accelerated``, either
``train_grid``, with or without a point budget, jitter or the distortion term) trains on a fresh random
background colour per ray and step: the train dataset keeps the alpha channel and its batch carries ``bg``
[N,3] and ``rgbs`` already composited onto it (nerf_raygen_rgba); the training march composites its
prediction onto the same colours (Renderer._render_accelerated_grad -> ops.march_grad(bg=)), so density where
the image is transparent costs loss whatever its colour.  The loss itself is unchanged (``gt`` arrives
blended).  A batch without ``bg`` is an error.  Validation, evaluation and every other no-grad march keep the
configured background.  With ``white`` every launch, output and stats key is what it was.
"""
import os

import torch
import torch.nn as nn

from nerf_amd import ops

from src.config import cfg
from src.models.nerf.renderer.online_grid import OnlineGrid, grid_update_settings
from src.models.nerf.renderer.ray_budget import RayBudget
from src.models.nerf.renderer.volume_renderer import (Renderer, distortion_loss_setting, march_jitter_setting,
                                                        train_background_setting)

TRAIN_RENDERERS = ("hierarchical", "accelerated")
TRAIN_GRIDS = ("file", "online")
GRID_STATE_FILE = "occupancy_grid_state.pt"
BUDGET_STATE_FILE = "ray_budget_state.pt"


def occupancy_grid_path():
    """logs/<cfg name>/occupancy_grid.pt, as run.py's evaluate builds it (run.py:85-87)."""
    from src.config.config import args
    name = os.path.splitext(os.path.basename(args.cfg_file))[0]
    return os.path.join("logs", name, "occupancy_grid.pt")


class NetworkWrapper(nn.Module):
    def __init__(self, net, train_loader=None):
        super().__init__()
        self.net = net
        self.train_loader = train_loader
        self.renderer = Renderer(self.net)
        self.loss_fn = nn.MSELoss()
        self.train_renderer = str(cfg.task_arg.get("train_renderer", "hierarchical") or "hierarchical")
        if self.train_renderer not in TRAIN_RENDERERS:
            raise ValueError(f"task_arg.train_renderer must be one of {TRAIN_RENDERERS}, got {self.train_renderer!r}")
        self.train_grid = str(cfg.task_arg.get("train_grid", "file") or "file")
        if self.train_grid not in TRAIN_GRIDS:
            raise ValueError(f"task_arg.train_grid must be one of {TRAIN_GRIDS}, got {self.train_grid!r}")
        self.march_jitter = march_jitter_setting(cfg.task_arg)
        if self.march_jitter and self.train_renderer != "accelerated":
            raise ValueError("task_arg.train_march_jitter: true jitters the steps of train_renderer: accelerated; "
                             f"with train_renderer: {self.train_renderer} the samples follow task_arg.perturb")
        self.distortion_weight = distortion_loss_setting(cfg.task_arg)
        if self.distortion_weight > 0.0 and self.train_renderer != "accelerated":
            raise ValueError("task_arg.distortion_loss_weight > 0 regularises the weights of train_renderer: "
                             f"accelerated; with train_renderer: {self.train_renderer} there is no such term")
        self.train_background = train_background_setting(cfg.task_arg)
        if self.train_background == "random" and self.train_renderer != "accelerated":
            raise ValueError("task_arg.train_background: random composites train_renderer: accelerated onto a colour "
                             f"per ray; with train_renderer: {self.train_renderer} the background is white_bkgd's")
        self.ray_budget = RayBudget.from_config(cfg.task_arg)  # (None: point_budget.target 0, the fixed train_rays)
        if self.ray_budget is not None:
            self.renderer.max_points = self.ray_budget.max_points
            self._publish_rays()  # (train_rays clamped and rounded to the budget's bounds)
        self.online_grid = None
        if self.train_grid == "online":
            if self.train_renderer != "accelerated":
                raise ValueError("task_arg.train_grid: online maintains the grid of train_renderer: accelerated; "
                                 f"with train_renderer: {self.train_renderer} there is no grid to maintain")
            ta = cfg.task_arg
            self.online_grid = OnlineGrid(int(ta.get("occupancy_grid_res", 128)),
                                          float(ta.get("occupancy_grid_threshold", 1.0)),
                                          cfg.train_dataset.scene_bbox, **grid_update_settings(ta))
        elif self.train_renderer == "accelerated":
            path = occupancy_grid_path()
            if not os.path.exists(path):
                raise FileNotFoundError(
                    f"train_renderer: accelerated needs the occupancy grid {path}: bake it first with "
                    "occupancy_grid.py (there is no fall-back to the hierarchical render in training)")
            self.renderer.load_occupancy_grid(path)

    def _live_grid(self, device):
        """The online grid on the rays' device, installed in the renderer (its uint8 tensor itself)."""
        grid = self.online_grid.to(device)
        self.renderer.set_live_grid(grid.grid)
        return grid

    def save_grid(self, model_dir):
        """Online mode, beside a checkpoint: logs/<cfg name>/occupancy_grid.pt in occupancy_grid.py's bool
        format (run.py evaluate and render_video.py load it) and <model_dir>/occupancy_grid_state.pt
        (density, counters, settings: what a resumed run continues from); a no-op in file mode.  With a
        point budget also <model_dir>/ray_budget_state.pt (the ray count a resumed run continues at)."""
        if self.ray_budget is not None:
            os.makedirs(model_dir, exist_ok=True)
            torch.save(self.ray_budget.state_dict(), os.path.join(model_dir, BUDGET_STATE_FILE))
        if self.online_grid is None:
            return
        path = occupancy_grid_path()
        os.makedirs(os.path.dirname(path), exist_ok=True)
        torch.save(self.online_grid.occupancy_bool(), path)
        os.makedirs(model_dir, exist_ok=True)
        torch.save(self.online_grid.state_dict(), os.path.join(model_dir, GRID_STATE_FILE))

    def load_grid(self, model_dir):
        """Resume: the state save_grid wrote, when it is there.  True when the grid was loaded.  The ray
        budget's count is read the same way; without its file the run starts from train_rays."""
        path = os.path.join(model_dir, BUDGET_STATE_FILE)
        if self.ray_budget is not None and os.path.exists(path):
            self.ray_budget.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
            self._publish_rays()
            print(f"load ray budget state: {path} ({self.ray_budget.rays} rays)")
        path = os.path.join(model_dir, GRID_STATE_FILE)
        if self.online_grid is None or not os.path.exists(path):
            return False
        self.online_grid.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
        print(f"load occupancy grid state: {path}")
        return True

    def _publish_rays(self):
        """The budget's ray count to the loader's dataset: the next batch drawn has that many rays."""
        if self.train_loader is not None:
            self.train_loader.dataset.batch_rays = self.ray_budget.rays

    def _march_loss(self, ret, gt, kept=None):
        """MSE(rgb_map_f, gt) over the first ``kept`` rays (all of them when None), plus the weighted mean
        distortion when the renderer returned the map -> (total, stats)."""
        rgb, gt = (ret["rgb_map_f"], gt) if kept is None else (ret["rgb_map_f"][:kept], gt[:kept])
        loss_f, _, total = ops.mse_pair(rgb, None, gt)
        if "dist_map_f" not in ret:
            return total, {"loss_f": loss_f, "total_loss": total}
        dist = ret["dist_map_f"] if kept is None else ret["dist_map_f"][:kept]
        loss_dist = dist.mean()
        total = total + self.distortion_weight * loss_dist
        return total, {"loss_f": loss_f, "loss_dist": loss_dist.detach(), "total_loss": total}

    def _budgeted_step(self, batch, gt):
        """The training forward under a point budget: one capped march, the loss over the kept rays, then the
        observation of ALL marched rays (the dropped ones were marched too) that sets the next count."""
        ret = self.renderer.render_accelerated(batch)
        kept, n = ret["rays_kept"], ret["rgb_map_f"].shape[0]
        total, stats = self._march_loss(ret, gt, kept)
        self.ray_budget.observe(n, ret["n_queried"])
        self._publish_rays()
        # (host tensors: a device scalar per step would be a blocking pageable copy, ops.device_scalar)
        stats.update(rays=torch.tensor(float(n)), points=torch.tensor(float(ret["n_points"])))
        return ret, total, stats

    def forward(self, batch):
        gt = batch["rgbs"].reshape(-1, 3) if batch["rgbs"].dim() == 3 else batch["rgbs"]
        budgeted = self.ray_budget is not None and torch.is_grad_enabled()
        if self.train_background == "random" and torch.is_grad_enabled() and batch.get("bg") is None:
            raise ValueError("task_arg.train_background: random needs batch['bg'] (the colours the ground truth was "
                             "composited onto); the train dataset adds it under this key")
        if self.online_grid is not None:
            grid = self._live_grid(batch["rays"].device)
            fine = self.net.model_fine
            if torch.is_grad_enabled():
                grid.step(fine.packer(), self.net.mlp_dtype)  # (may update; update 0 precedes the first march)
            elif grid.updates == 0:  # validation before any training step: never march the all-ones grid
                grid.update(fine.packer(), self.net.mlp_dtype)
        if budgeted:
            return self._budgeted_step(batch, gt)
        if self.online_grid is not None or (self.train_renderer == "accelerated" and torch.is_grad_enabled()):
            # the fine net through the grid march; the MSE and its backward in one launch each
            # (ops.mse_pair with no second image)
            ret = self.renderer.render_accelerated(batch)
            total, stats = self._march_loss(ret, gt)
            return ret, total, stats
        ret = self.renderer.render(batch)
        if "rgb_map_f" in ret and ret["rgb_map_c"].is_cuda and cfg.task_arg.get("fuse_mse", True):
            # both MSEs and their sum in one launch, the backward in one (ops.mse_pair)
            loss_c, loss_f, total = ops.mse_pair(ret["rgb_map_c"], ret["rgb_map_f"], gt)
            return ret, total, {"loss_c": loss_c, "loss_f": loss_f, "total_loss": total}
        loss_c = self.loss_fn(ret["rgb_map_c"], gt)
        stats = {"loss_c": loss_c}
        if "rgb_map_f" in ret:
            loss_f = self.loss_fn(ret["rgb_map_f"], gt)
            total = loss_c + loss_f
            stats["loss_f"] = loss_f
        else:
            total = loss_c
        stats["total_loss"] = total
        return ret, total, stats
