"""Mesh export: the density iso-surface of a trained net as a PLY (reference: src/utils/mesh_utils.py:8-46
and the ``level`` / ``resolution`` keys its config reserves for it).

    python extract_mesh.py --cfg_file configs/nerf/lego.yaml [level 32.0 resolution 256]

sigma = relu(raw[3]) of the fine net (task_arg.mesh_net: coarse for the coarse one) on the
resolution^3 lattice of train_dataset.scene_bbox by the density-only fused MLP, then the surface
sigma == level by marching tetrahedra on the GPU (nerf_amd.ops.mesh_extract); written to
logs/<cfg name>/mesh.ply (binary little-endian, indexed triangles, normals pointing out of the dense
side).  Single process: under ``torch.distributed.run`` rank 0 works and the others return.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402,F401

from src.config import cfg, args  # noqa: E402
from src.config.config import apply_gpus  # noqa: E402


def main():
    from src.models import make_network
    from src.utils.mesh_utils import extract_mesh_from_net, mesh_settings
    from src.utils.net_utils import load_network

    level, res, net = mesh_settings(cfg)
    if int(os.environ.get("RANK", "0")) != 0:
        return
    if "LOCAL_RANK" in os.environ:
        torch.cuda.set_device(int(os.environ["LOCAL_RANK"]))
    else:
        apply_gpus(cfg)
    network = make_network(cfg).cuda()
    load_network(network, cfg.trained_model_dir, epoch=cfg.test.epoch)
    network.eval()
    b = cfg.train_dataset.scene_bbox
    name = os.path.splitext(os.path.basename(args.cfg_file))[0]
    path = os.path.join("logs", name, "mesh.ply")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    times = {}
    verts, faces = extract_mesh_from_net(network, level, (b[0], b[1]), path, res, net, times)
    print(f"{net} net, level {level:g}, {res}^3 lattice: {len(verts)} vertices, {len(faces)} faces "
          f"(field {times['field'] * 1e3:.1f} ms, extraction {times['extract'] * 1e3:.1f} ms)")
    print(f"Saved mesh to: {path}")
    print("Done.")


if __name__ == "__main__":
    main()
