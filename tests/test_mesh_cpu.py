"""CPU: the mesh export's interface (header, ctypes signatures, PLY I/O, settings) and the properties of
its algorithm, held by the numpy restatement (tests/mesh_numpy.py) on analytic fields 32 + 40 (r - dist)
at level 32: exact vertex and face counts, a closed and consistently oriented surface, the Euler
characteristic, and a positive volume just below the solid's (an inscribed polyhedron)."""
import os
import re

import numpy as np
import pytest

import mesh_numpy as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerf_amd.h")
MESH_SYMBOLS = ("nerf_mesh_lattice", "nerf_mesh_classify", "nerf_mesh_emit")


def test_mesh_symbols_are_declared_and_bound():
    from nerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in MESH_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", text), f"{name} is not declared in nerf_amd.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.lib()
        for name in MESH_SYMBOLS:
            assert hasattr(lib, name), name
        assert lib.nerf_abi_version() == 4  # additions do not bump it


def test_mesh_argument_errors_are_reported_without_gpu():
    from nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = _lib.lib()
    with pytest.raises(RuntimeError, match="at least 2"):
        _lib.check(lib.nerf_mesh_lattice(None, 1, 4, 4, 0, 1, None, None), "nerf_mesh_lattice")
    with pytest.raises(RuntimeError, match="2\\^31"):
        _lib.check(lib.nerf_mesh_classify(None, 2048, 2048, 2048, 32.0, None, None, None, None), "nerf_mesh_classify")
    with pytest.raises(RuntimeError, match="finite"):
        _lib.check(lib.nerf_mesh_classify(None, 4, 4, 4, float("nan"), None, None, None, None), "nerf_mesh_classify")
    with pytest.raises(RuntimeError, match="null"):
        _lib.check(lib.nerf_mesh_emit(None, None, 4, 4, 4, float("inf"), None, None, None, 1, 1, None, None, None),
                   "nerf_mesh_emit")


def test_mesh_ops_reject_cpu_tensors():
    import torch
    from nerf_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.mesh_extract(torch.zeros(4, 4, 4), 32.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.mesh_lattice((4, 4, 4), device="cpu")


@pytest.mark.parametrize("V,F", [(0, 0), (1, 0), (7, 5), (1000, 2001)])
def test_ply_round_trip(tmp_path, V, F):
    from src.utils.mesh_utils import read_ply, write_ply
    rng = np.random.default_rng(V + F)
    verts = rng.standard_normal((V, 3)).astype(np.float32)
    if V:
        verts[0] = [np.float32(-0.0), np.float32(1e-42), np.float32(3.4e38)]  # signed zero, a denormal, near max
    faces = rng.integers(0, max(V, 1), (F, 3)).astype(np.int32)
    path = tmp_path / "m.ply"
    write_ply(path, verts, faces)
    data = open(path, "rb").read()
    head = data[:data.index(b"end_header\n")].decode("ascii")
    assert head.startswith("ply\nformat binary_little_endian 1.0\n")
    assert f"element vertex {V}\nproperty float x\nproperty float y\nproperty float z\n" in head
    assert f"element face {F}\nproperty list uchar int vertex_indices\n" in head
    assert len(data) == len(head) + len("end_header\n") + 12 * V + 13 * F
    v, f = read_ply(path)
    assert v.dtype == np.float32 and v.shape == (V, 3) and f.dtype == np.int32 and f.shape == (F, 3)
    assert v.tobytes() == verts.tobytes() and f.tobytes() == faces.tobytes()


def test_read_ply_refuses_other_files(tmp_path):
    from src.utils.mesh_utils import read_ply
    p = tmp_path / "x.ply"
    p.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nelement face 0\nend_header\n")
    with pytest.raises(ValueError, match="binary_little_endian"):
        read_ply(p)
    p.write_bytes(b"not a ply")
    with pytest.raises(ValueError, match="not a PLY"):
        read_ply(p)


def test_default_cfg_carries_the_reference_keys():
    from src.config.config import default_cfg
    from src.utils.mesh_utils import mesh_settings
    c = default_cfg()
    assert c.level == 32.0 and c.resolution == 256
    assert mesh_settings(c) == (32.0, 256, "fine")
    c.task_arg.mesh_net = "coarse"
    c.level, c.resolution = 5, 2
    assert mesh_settings(c) == (5.0, 2, "coarse")


@pytest.mark.parametrize("key,value,match", [
    ("resolution", 1, "resolution"), ("resolution", 0, "resolution"), ("resolution", 64.5, "resolution"),
    ("resolution", "big", "resolution"), ("level", float("nan"), "level"), ("level", float("inf"), "level"),
    ("level", "high", "level"), ("level", None, "level"), ("task_arg.mesh_net", "both", "task_arg.mesh_net"),
    ("task_arg.mesh_net", "", "task_arg.mesh_net")])
def test_bad_settings_raise_and_name_the_key(key, value, match):
    from src.config.config import default_cfg
    from src.utils.mesh_utils import mesh_settings
    c = default_cfg()
    node = c
    for part in key.split(".")[:-1]:
        node = node[part]
    node[key.split(".")[-1]] = value
    with pytest.raises(ValueError, match=match):
        mesh_settings(c)


def test_triangle_table_is_one_parity_per_permutation_and_case():
    """The winding the restatement derives from the geometry is a fixed parity: an odd permutation's
    triangles are the even ones with their last two edges swapped, and complementing the inside set
    gives the same surface with the opposite winding."""
    def odd(p):
        return sum(1 for i in range(3) for j in range(i) if p[j] > p[i]) % 2

    def canon(tris):
        return sorted(tuple(t[k:] + t[:k]) for t in tris for k in [t.index(min(t))])

    base = M.TABLE[0]
    for pi, perm in enumerate(M.PERMS):
        for case in range(16):
            want = base[case] if not odd(perm) else [[t[0], t[2], t[1]] for t in base[case]]
            assert M.TABLE[pi][case] == want, (perm, case)
            n = bin(case).count("1")
            assert len(M.TABLE[pi][case]) == (0, 1, 2, 1, 0)[n]
    for case in (1, 2, 4, 8):  # one inside vertex against three: the same triangle, reversed
        a, b = base[case], base[15 - case]
        assert canon(a) == canon([[t[0], t[2], t[1]] for t in b]), case


def test_lattice_samples_both_bbox_faces():
    for shape, bbox in (((2, 2, 2), M.LEGO_BOX), ((9, 12, 17), M.BOX_B), ((33, 33, 33), M.LEGO_BOX)):
        pts = M.lattice(shape, bbox)
        assert pts.dtype == np.float32 and pts.shape == (shape[0] * shape[1] * shape[2], 3)
        assert pts[0].tolist() == [np.float32(v) for v in bbox[0]]
        assert np.allclose(pts[-1], bbox[1], rtol=0, atol=1e-6)
        grid = pts.reshape(*shape, 3)
        assert (np.diff(grid[:, 0, 0, 0]) > 0).all() and (np.diff(grid[0, 0, :, 2]) > 0).all()
        assert np.array_equal(M.lattice(shape, bbox, 1, 2), grid[1:2].reshape(-1, 3))


@pytest.mark.parametrize("name", list(M.CASES))
def test_restatement_on_analytic_fields(name):
    shape, bbox, build, V, F, chi, solid, lower = M.CASES[name]
    field = build(shape, bbox)
    assert field.dtype == np.float32 and not (field == np.float32(M.LEVEL)).any()  # no value on the level
    verts, faces = M.extract(field, M.LEVEL, bbox)
    t = M.topology(verts, faces)
    ratio = t["volume"] / solid if solid else None
    print(f"\n{name}: V {t['V']} F {t['F']} chi {t['chi']} closed {t['closed']} volume ratio {ratio}")
    assert verts.dtype == np.float32 and faces.dtype == np.int32
    assert (t["V"], t["F"]) == (V, F)  # a property of the algorithm, not a measurement
    assert t["closed"] and t["chi"] == chi and t["degenerate"] == 0
    assert t["volume"] > 0  # the normals point outwards
    assert faces.min() >= 0 and faces.max() == V - 1 and len(np.unique(faces)) == V  # welded, no orphan
    lo, hi = np.asarray(bbox, np.float32)
    assert (verts >= lo).all() and (verts <= hi).all()
    if solid:
        assert ratio <= 1.0  # an inscribed polyhedron cannot exceed the solid
    if lower:
        assert ratio >= lower


def test_restatement_edge_cases():
    box = M.LEGO_BOX
    one = np.full((2, 2, 2), 0.0, np.float32)
    one[0, 0, 0] = 64.0
    v, f = M.extract(one, M.LEVEL, box)
    assert len(v) == 7 and len(f) == 6  # the seven edges of the corner, one triangle per tetrahedron
    assert np.array_equal(np.unique(v), np.float32([-1.5, 0.0]))
    for fill in (0.0, 64.0):
        v, f = M.extract(np.full((3, 4, 5), fill, np.float32), M.LEVEL, box)
        assert v.shape == (0, 3) and f.shape == (0, 3)
    cut = M.sphere_field((9, 9, 9), box, 1.7)
    v, f = M.extract(cut, M.LEVEL, box)
    t = M.topology(v, f)
    assert t["F"] > 0 and not t["closed"]  # cut by the lattice boundary: open
    octa = M.octahedron_field((9, 9, 9), ((-4, -4, -4), (4, 4, 4)))
    assert (octa == np.float32(M.LEVEL)).any()
    v, f = M.extract(octa, M.LEVEL, ((-4, -4, -4), (4, 4, 4)))
    assert np.isfinite(v).all() and M.topology(v, f)["degenerate"] > 0
