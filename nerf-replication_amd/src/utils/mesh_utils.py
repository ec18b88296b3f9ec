"""Mesh export (reference: src/utils/mesh_utils.py:8-46, extract_mesh).

``extract_mesh(queryfn, level, bbox, output_path, N)`` keeps the reference's signature and its
``queryfn`` contract (CUDA points [n,3] -> [..., C], density in channel 0), samples the same N^3
lattice (both bbox faces included; per axis, where the reference uses the x extent on all three) and
writes a PLY.  What differs: the field is evaluated in large device slabs without a host copy per
batch, the surface is extracted on the GPU by marching tetrahedra (nerf_amd.ops.mesh_extract; the
reference's skimage ``marching_cubes_lewiner`` and ``np.int`` no longer exist, and trimesh is not
needed), and the vertices are the world coordinates of the sampled lattice (the reference places them
with spacing size / N about the bbox centre although it sampled with size / (N - 1) from the corner).
``extract_mesh_from_net`` is the fast path over the fused density-only MLP.

Out of scope: vertex colours and normals, simplification, removing floater components, culling the
lattice by the occupancy grid, multi-GPU slabs.
"""
import math
import time

import numpy as np
import torch

PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {V}\nproperty float x\nproperty float y\n"
              "property float z\nelement face {F}\nproperty list uchar int vertex_indices\nend_header\n")
_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_ply(path, verts, faces) -> None:
    """Binary little-endian PLY: ``float x y z`` per vertex, ``list uchar int vertex_indices`` per
    triangle (the layout trimesh exports)."""
    v = np.ascontiguousarray(np.asarray(verts).reshape(-1, 3), dtype="<f4")
    f = np.asarray(faces).reshape(-1, 3)
    rec = np.empty(len(f), _FACE)
    rec["n"] = 3
    rec["v"] = f
    with open(path, "wb") as out:
        out.write(PLY_HEADER.format(V=len(v), F=len(f)).encode("ascii"))
        out.write(v.tobytes())
        out.write(rec.tobytes())


def read_ply(path):
    """(verts float32 [V,3], faces int32 [F,3]) of a file in write_ply's layout."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    if lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: only binary_little_endian 1.0 is read, got {lines[1]!r}")
    counts = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("element ")}
    props = [ln for ln in lines if ln.startswith("property ")]
    if props != [ln for ln in PLY_HEADER.split("\n") if ln.startswith("property ")]:
        raise ValueError(f"{path}: unexpected properties {props}")
    V, F = counts["vertex"], counts["face"]
    body = end + len(b"end_header\n")
    if len(data) != body + 12 * V + _FACE.itemsize * F:
        raise ValueError(f"{path}: {len(data) - body} bytes of data for {V} vertices and {F} faces")
    verts = np.frombuffer(data, "<f4", 3 * V, body).reshape(V, 3).astype(np.float32)
    rec = np.frombuffer(data, _FACE, F, body + 12 * V)
    if F and not (rec["n"] == 3).all():
        raise ValueError(f"{path}: a face is not a triangle")
    return verts, rec["v"].astype(np.int32).reshape(F, 3)


def mesh_settings(cfg):
    """(level, resolution, mesh_net) of a configuration: the reference's top-level ``level`` and
    ``resolution`` and this build's ``task_arg.mesh_net``; each bad value raises naming its key."""
    level, res = cfg.get("level", 32.0), cfg.get("resolution", 256)
    if isinstance(level, bool) or not isinstance(level, (int, float)) or not math.isfinite(level):
        raise ValueError(f"level must be a finite number, got {level!r}")
    if isinstance(res, bool) or not isinstance(res, int) or res < 2:
        raise ValueError(f"resolution must be an integer >= 2, got {res!r}")
    net = cfg.task_arg.get("mesh_net", "fine")
    if net not in ("fine", "coarse"):
        raise ValueError(f"task_arg.mesh_net must be 'fine' or 'coarse', got {net!r}")
    return float(level), int(res), net


def _bbox(bbox):
    b = np.asarray(bbox, dtype=np.float64).reshape(2, 3)
    return tuple(map(float, b[0])), tuple(map(float, b[1]))


def _finish(verts, faces, output_path):
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    write_ply(output_path, v, f)
    return v, f


def extract_mesh(queryfn, level, bbox, output_path="test.ply", N=256):
    """The reference's entry: the iso-surface ``queryfn(points)[..., 0] == level`` on the N^3 lattice of
    ``bbox`` -> (verts float32 [V,3], faces int32 [F,3]) as numpy arrays, written to ``output_path``."""
    from nerf_amd import ops
    bbox = _bbox(bbox)
    N = int(N)
    planes = max(1, ops.MESH_MLP_POINTS // (N * N))
    density = torch.empty(N, N, N, dtype=torch.float32, device="cuda")
    with torch.no_grad():
        for x0 in range(0, N, planes):
            x1 = min(N, x0 + planes)
            out = queryfn(ops.mesh_lattice((N, N, N), bbox, x0, x1))[..., 0]
            density[x0:x1] = out.detach().reshape(x1 - x0, N, N)
    return _finish(*ops.mesh_extract(density, level, bbox), output_path)


def extract_mesh_from_net(network, level, bbox, output_path="test.ply", N=256, net="fine", times=None):
    """extract_mesh over the fused density-only MLP of ``network`` (sigma = relu(raw[3]) of its fine or
    coarse net at the network's mlp_dtype).  ``times`` (a dict) receives the seconds of the field and of
    the extraction."""
    from nerf_amd import ops
    if net not in ("fine", "coarse"):
        raise ValueError(f"net must be 'fine' or 'coarse', got {net!r}")
    bbox = _bbox(bbox)
    N = int(N)
    model = network.model_fine if net == "fine" else network.model
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    field = ops.mesh_field(model.packer(), (N, N, N), bbox, network.mlp_dtype)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    verts, faces = ops.mesh_extract(field, level, bbox)
    torch.cuda.synchronize()
    if times is not None:
        times.update(field=t1 - t0, extract=time.perf_counter() - t1)
    return _finish(verts, faces, output_path)
