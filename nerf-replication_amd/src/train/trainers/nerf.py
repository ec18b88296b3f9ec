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
"""
import os

import torch
import torch.nn as nn

from nerf_amd import ops

from src.config import cfg
from src.models.nerf.renderer.volume_renderer import Renderer

TRAIN_RENDERERS = ("hierarchical", "accelerated")


def occupancy_grid_path():
    """logs/<cfg name>/occupancy_grid.pt, as run.py's evaluate builds it (run.py:85-87)."""
    from src.config.config import args
    name = os.path.splitext(os.path.basename(args.cfg_file))[0]
    return os.path.join("logs", name, "occupancy_grid.pt")


class NetworkWrapper(nn.Module):
    def __init__(self, net, train_loader=None):
        super().__init__()
        self.net = net
        self.renderer = Renderer(self.net)
        self.loss_fn = nn.MSELoss()
        self.train_renderer = str(cfg.task_arg.get("train_renderer", "hierarchical") or "hierarchical")
        if self.train_renderer not in TRAIN_RENDERERS:
            raise ValueError(f"task_arg.train_renderer must be one of {TRAIN_RENDERERS}, got {self.train_renderer!r}")
        if self.train_renderer == "accelerated":
            path = occupancy_grid_path()
            if not os.path.exists(path):
                raise FileNotFoundError(
                    f"train_renderer: accelerated needs the occupancy grid {path}: bake it first with "
                    "occupancy_grid.py (there is no fall-back to the hierarchical render in training)")
            self.renderer.load_occupancy_grid(path)

    def forward(self, batch):
        gt = batch["rgbs"].reshape(-1, 3) if batch["rgbs"].dim() == 3 else batch["rgbs"]
        if self.train_renderer == "accelerated" and torch.is_grad_enabled():
            # the fine net through the grid march; the MSE and its backward in one launch each
            # (ops.mse_pair with no second image)
            ret = self.renderer.render_accelerated(batch)
            loss_f, _, total = ops.mse_pair(ret["rgb_map_f"], None, gt)
            return ret, total, {"loss_f": loss_f, "total_loss": total}
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
