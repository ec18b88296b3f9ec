"""GPU: the mesh export kernels (csrc/mesh.hip) against the numpy restatement (tests/mesh_numpy.py).

The vertex array must be the restatement's bit for bit and in its order (ids are lattice order, then
edge type); the faces must be the same oriented triangles as a multiset (their order and the rotation
of a triple are the implementation's choice).  The topology of the analytic fields is asserted on the
kernels' own output.  Then the layers above: ops.mesh_field on the trained fixture net,
mesh_utils.extract_mesh / extract_mesh_from_net, the PLY they write, and the extract_mesh.py entry
point."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_numpy as M

from march_support import trained_state

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "nerf-replication_amd")
_REF = {}


def _ref(key, field, bbox):
    """The restatement's mesh of a field, computed once per key and left unchanged."""
    if key not in _REF:
        v, f = M.extract(field, M.LEVEL, bbox)
        v.setflags(write=False)
        f.setflags(write=False)
        _REF[key] = (v, f)
    return _REF[key]


def _gpu(field, bbox, cuda, level=M.LEVEL):
    from nerf_amd import ops
    v, f = ops.mesh_extract(torch.from_numpy(np.ascontiguousarray(field)).to(cuda), level, bbox)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    assert v.shape[1:] == (3,) and f.shape[1:] == (3,)
    return v.cpu().numpy(), f.cpu().numpy()


def _assert_same(got, want):
    (v, f), (rv, rf) = got, want
    assert v.shape == rv.shape and f.shape == rf.shape, (v.shape, rv.shape, f.shape, rf.shape)
    assert v.tobytes() == rv.tobytes(), f"{int((v.view(np.int32) != rv.view(np.int32)).sum())} vertex words differ"
    assert np.array_equal(M.canonical_faces(f), M.canonical_faces(rf))


# ---------------------------------------------------------------------------------------------
# lattice
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,bbox,slab", [((2, 2, 2), M.LEGO_BOX, None), ((9, 12, 17), M.BOX_B, None),
                                             ((33, 33, 33), M.LEGO_BOX, None), ((33, 33, 33), M.LEGO_BOX, (3, 7))])
def test_lattice_is_the_restatement_bit_for_bit(cuda, shape, bbox, slab):
    from nerf_amd import ops
    x0, x1 = slab or (0, shape[0])
    got = ops.mesh_lattice(shape, bbox, x0, x1, device=cuda) if slab else ops.mesh_lattice(shape, bbox, device=cuda)
    want = M.lattice(shape, bbox, x0, x1)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert got.cpu().numpy().tobytes() == want.tobytes()


def test_lattice_argument_errors(cuda):
    from nerf_amd import ops
    assert ops.mesh_lattice((4, 4, 4), M.LEGO_BOX, 2, 2, device=cuda).shape == (0, 3)
    with pytest.raises(ValueError, match="x-planes"):
        ops.mesh_lattice((4, 4, 4), M.LEGO_BOX, 3, 5, device=cuda)
    with pytest.raises(ValueError, match="at least 2"):
        ops.mesh_lattice((4, 1, 4), M.LEGO_BOX, device=cuda)


# ---------------------------------------------------------------------------------------------
# extraction: the analytic fields of the table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(M.CASES))
def test_extract_analytic_fields(cuda, name):
    shape, bbox, build, V, F, chi, solid, lower = M.CASES[name]
    field = build(shape, bbox)
    got = _gpu(field, bbox, cuda)
    _assert_same(got, _ref(name, field, bbox))
    t = M.topology(*got)  # on the kernels' own output
    ratio = t["volume"] / solid if solid else None
    print(f"\n{name}: V {t['V']} F {t['F']} chi {t['chi']} closed {t['closed']} volume ratio {ratio}")
    assert (t["V"], t["F"], t["chi"]) == (V, F, chi)
    assert t["closed"] and t["degenerate"] == 0 and t["volume"] > 0
    if solid:
        assert ratio <= 1.0
    if lower:
        assert ratio >= lower


# ---------------------------------------------------------------------------------------------
# edge cases, each against the restatement
# ---------------------------------------------------------------------------------------------
def _noise(shape, seed):
    """Values scattered about the level: every tetrahedron case of every permutation occurs."""
    f = (np.random.default_rng(seed).standard_normal(shape) * 20.0 + 32.0).astype(np.float32)
    assert not (f == np.float32(M.LEVEL)).any()
    return f


def _one_corner():
    f = np.zeros((2, 2, 2), np.float32)
    f[0, 0, 0] = 64.0
    return f


OCTA_BOX = ((-4.0, -4.0, -4.0), (4.0, 4.0, 4.0))
EDGE_FIELDS = {
    "one_corner": (M.LEGO_BOX, _one_corner),
    "far_corner": (M.BOX_B, lambda: 64.0 - _one_corner()[::-1, ::-1, ::-1]),  # inside everywhere but at (1,1,1)
    "cut_sphere": (M.LEGO_BOX, lambda: M.sphere_field((9, 9, 9), M.LEGO_BOX, 1.7)),
    "octahedron": (OCTA_BOX, lambda: M.octahedron_field((9, 9, 9), OCTA_BOX)),
    "noise_5x7x3": (M.BOX_B, lambda: _noise((5, 7, 3), 1)),
    "noise_65x2x2": (M.BOX_B, lambda: _noise((65, 2, 2), 2)),
    "noise_2x3x70": (M.BOX_T, lambda: _noise((2, 3, 70), 3)),
    "noise_19x11x23": (M.BOX_T, lambda: _noise((19, 11, 23), 4)),
}


@pytest.mark.parametrize("name", list(EDGE_FIELDS))
def test_extract_edge_cases(cuda, name):
    bbox, build = EDGE_FIELDS[name]
    field = build()
    got = _gpu(field, bbox, cuda)
    want = _ref(name, field, bbox)
    _assert_same(got, want)
    assert np.isfinite(got[0]).all()
    if name == "one_corner":
        assert len(got[0]) == 7 and len(got[1]) == 6
    if name == "cut_sphere":
        t = M.topology(*got)
        assert t["F"] > 0 and not t["closed"]  # the surface leaves the lattice: open, but bit-equal
    if name == "octahedron":
        assert (field == np.float32(M.LEVEL)).any() and M.topology(*got)["degenerate"] > 0
    if name.startswith("noise"):
        assert len(got[0]) > 0 and got[1].min() == 0 and got[1].max() == len(got[0]) - 1


@pytest.mark.parametrize("fill", [0.0, 64.0])
def test_uniform_field_gives_an_empty_mesh_and_an_empty_ply(cuda, tmp_path, fill):
    from src.utils.mesh_utils import extract_mesh, read_ply
    v, f = _gpu(np.full((5, 7, 3), fill, np.float32), M.BOX_B, cuda)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    path = tmp_path / "empty.ply"
    v, f = extract_mesh(lambda p: torch.full((p.shape[0], 2), fill, device=p.device), M.LEVEL, M.LEGO_BOX, str(path), N=6)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    rv, rf = read_ply(path)
    assert rv.shape == (0, 3) and rf.shape == (0, 3)


def test_two_runs_give_the_same_bytes(cuda):
    field = _noise((33, 17, 40), 5)
    a, b = _gpu(field, M.BOX_T, cuda), _gpu(field, M.BOX_T, cuda)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_bad_fields_raise(cuda):
    from nerf_amd import ops
    field = torch.from_numpy(M.sphere_field((9, 9, 9), M.LEGO_BOX, 0.9)).to(cuda)
    for bad in (float("nan"), float("inf")):
        f = field.clone()
        f[4, 5, 6] = bad
        with pytest.raises(ValueError, match="NaN or an infinity"):
            ops.mesh_extract(f, M.LEVEL, M.LEGO_BOX)
    with pytest.raises(ValueError, match="level"):
        ops.mesh_extract(field, float("nan"), M.LEGO_BOX)
    with pytest.raises(TypeError, match="float32"):
        ops.mesh_extract(field.double(), M.LEVEL, M.LEGO_BOX)
    with pytest.raises(ValueError, match="at least 2"):
        ops.mesh_extract(field[:1], M.LEVEL, M.LEGO_BOX)


# ---------------------------------------------------------------------------------------------
# the trained fixture net: field, mesh, PLY, entry point
# ---------------------------------------------------------------------------------------------
N_NET = 48


@pytest.fixture(scope="module")
def fine_packer(cuda, trained_state):
    from nerf_amd import ops
    return ops.PackedMLP([trained_state[f"model_fine.{n}"].to(cuda) for n in ops.NET_PARAM_NAMES])


@pytest.fixture(scope="module")
def net_field(cuda, fine_packer):
    """sigma of the fine net on the 48^3 lego lattice in ONE density-only MLP call, and the restatement's mesh."""
    from nerf_amd import ops
    with torch.no_grad():
        pts = ops.mesh_lattice((N_NET,) * 3, M.LEGO_BOX, device=cuda)
        raw = ops.mlp(fine_packer, pts, None, 1, None, "fp32", density_only=True)
        field = torch.relu(raw[:, 3]).reshape(N_NET, N_NET, N_NET)
    return field, _ref("net48", field.cpu().numpy(), M.LEGO_BOX)


def test_mesh_field_on_the_trained_net(cuda, fine_packer, net_field):
    from nerf_amd import ops
    field, (rv, rf) = net_field
    for planes in (None, 5, 48):
        got = ops.mesh_field(fine_packer, (N_NET,) * 3, M.LEGO_BOX, "fp32", slab_planes=planes)
        assert got.dtype == torch.float32 and tuple(got.shape) == (N_NET,) * 3
        assert torch.equal(got, field), planes
    v, f = ops.mesh_extract(field, M.LEVEL, M.LEGO_BOX)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    print(f"\ntrained fine net, {N_NET}^3, level {M.LEVEL}: V {len(v)} F {len(f)}")
    assert len(v) > 0 and len(f) > 0
    assert (v >= -1.5).all() and (v <= 1.5).all()
    _assert_same((v, f), (rv, rf))


def test_extract_mesh_with_a_queryfn(cuda, fine_packer, net_field, tmp_path):
    from nerf_amd import ops
    from src.utils.mesh_utils import extract_mesh, read_ply
    _, want = net_field
    calls = []

    def queryfn(p):  # the reference's contract: CUDA points [n,3] -> [..., C], density in channel 0
        assert p.is_cuda and p.shape[1] == 3
        calls.append(p.shape[0])
        raw = ops.mlp(fine_packer, p, None, 1, None, "fp32", density_only=True)
        return torch.stack([torch.relu(raw[:, 3]), raw[:, 0]], -1)

    path = tmp_path / "q.ply"
    v, f = extract_mesh(queryfn, M.LEVEL, [[-1.5, -1.5, -1.5], [1.5, 1.5, 1.5]], str(path), N=N_NET)
    assert sum(calls) == N_NET ** 3 and max(calls) <= ops.MESH_MLP_POINTS
    assert isinstance(v, np.ndarray) and v.dtype == np.float32 and f.dtype == np.int32
    _assert_same((v, f), want)
    rv, rf = read_ply(path)
    assert rv.tobytes() == v.tobytes() and rf.tobytes() == f.tobytes()


def _run_entry(tmp_path, extra):
    env = {k: v for k, v in os.environ.items() if k != "NERF_AMD_NO_ARGV"}
    r = subprocess.run([sys.executable, os.path.join(PKG, "extract_mesh.py"), "--cfg_file", "configs/nerf/lego.yaml",
                        "trained_model_dir", str(tmp_path / "model"), "resolution", "32"] + extra,
                       cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    return r


def test_extract_mesh_entry_point(cuda, trained_state, tmp_path):
    """`python extract_mesh.py --cfg_file configs/nerf/lego.yaml resolution 32` on a fixture checkpoint writes
    logs/lego/mesh.ply = extract_mesh_from_net's arrays; task_arg.mesh_net coarse gives another valid mesh."""
    from src.models.nerf.network import Network
    from src.utils.mesh_utils import extract_mesh_from_net, read_ply
    mdir = tmp_path / "model" / "nerf_replication" / "lego" / "nerf"
    mdir.mkdir(parents=True)
    torch.save({"net": trained_state, "epoch": 9}, mdir / "latest.pth")
    net = Network()
    net.load_state_dict(trained_state, strict=True)
    net = net.to(cuda).eval()
    meshes = {}
    for which, extra in (("fine", []), ("coarse", ["task_arg.mesh_net", "coarse"])):
        r = _run_entry(tmp_path, extra)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "vertices" in r.stdout and "field" in r.stdout and "extraction" in r.stdout, r.stdout[-1000:]
        got = read_ply(tmp_path / "logs" / "lego" / "mesh.ply")
        want = extract_mesh_from_net(net, M.LEVEL, M.LEGO_BOX, str(tmp_path / f"{which}.ply"), 32, which)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), which
        assert len(got[0]) > 0 and len(got[1]) > 0 and got[1].min() >= 0 and got[1].max() < len(got[0])
        meshes[which] = got
    assert meshes["fine"][0].tobytes() != meshes["coarse"][0].tobytes()
