"""numpy restatement of the mesh export (csrc/mesh.hip; DESIGN.md 4 "Mesh export"): marching
tetrahedra on the Kuhn split of a density lattice, float32 throughout, one rounded op at a time.

Shared by tests/test_mesh_cpu.py (the properties of the algorithm on analytic fields) and
tests/test_gpu_mesh.py (the kernels against it, bit for bit).  Nothing here comes from the kernels:
the triangle table is derived below from the geometry of each tetrahedron case.

  lattice   coordinate i on axis a = mn[a] + float(i) * h[a],  h[a] = (mx[a] - mn[a]) / float(n[a] - 1)
  inside    field >= level
  edges     point p owns p -> p + d for the seven d of EDGE_DIRS that stay in the lattice; an edge
            crosses when its ends differ in "inside" and then carries one vertex, interpolated
            from the owner end: t = (level - f0) / (f1 - f0), v = x0 + t * (x1 - x0)
  ids       vert_off[p] + popcount(mask[p] & ((1 << type) - 1)): lattice order, then edge type
  faces     per cube the six tetrahedra p, p + e_a, p + e_a + e_b, p + (1,1,1) of the axis
            permutations (a, b, c); 1 or 2 triangles per tetrahedron, wound so that the right-hand
            normal points from inside to outside
"""
import itertools

import numpy as np

F = np.float32
EDGE_DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
EDGE_TYPE = {d: t for t, d in enumerate(EDGE_DIRS)}
PERMS = tuple(itertools.permutations(range(3)))


def tet_path(perm):
    """The four path vertices of a permutation's tetrahedron as integer offsets from the cube origin."""
    v = [np.zeros(3, np.int64)]
    for a in perm:
        w = v[-1].copy()
        w[a] += 1
        v.append(w)
    return v


def _case_triangles(case):
    """The triangles of one inside set as triples of tetrahedron edges (i, j), before winding."""
    S = [i for i in range(4) if case >> i & 1]
    O = [i for i in range(4) if not case >> i & 1]
    if len(S) == 1:
        return [[(S[0], j) for j in O]]
    if len(S) == 3:
        return [[(j, O[0]) for j in S]]
    if len(S) == 2:
        (i, j), (k, l) = S, O
        return [[(i, k), (i, l), (j, l)], [(i, k), (j, l), (j, k)]]
    return []


def _build_table():
    """TABLE[perm][case] -> list of triangles, each three sorted tetrahedron edges (i < j), wound by a
    geometric test on the unit cube with every crossing at its edge's midpoint: the normal
    (b - a) x (c - a) must point from the inside vertices' centroid to the outside vertices'."""
    table = []
    for perm in PERMS:
        path = [p.astype(np.float64) for p in tet_path(perm)]
        row = []
        for case in range(16):
            tris = []
            S = [path[i] for i in range(4) if case >> i & 1]
            O = [path[i] for i in range(4) if not case >> i & 1]
            for tri in _case_triangles(case):
                tri = [tuple(sorted(e)) for e in tri]
                a, b, c = [(path[i] + path[j]) / 2 for i, j in tri]
                out = np.mean(O, axis=0) - np.mean(S, axis=0)
                s = float(np.dot(np.cross(b - a, c - a), out))
                assert abs(s) > 1e-9
                tris.append(tri if s > 0 else [tri[0], tri[2], tri[1]])
            row.append(tris)
        table.append(row)
    return table


TABLE = _build_table()


def lattice_axis(mn, mx, n):
    """float32 coordinates of one axis: fadd(mn, fmul(float(i), h))."""
    mn, mx = F(mn), F(mx)
    h = F(F(mx - mn) / F(n - 1))
    return (mn + (np.arange(n, dtype=F) * h).astype(F)).astype(F)


def lattice(shape, bbox, x0=0, x1=None):
    """float32 [(x1 - x0) * ny * nz, 3]: the points of the x-planes [x0, x1), z fastest."""
    x1 = shape[0] if x1 is None else x1
    ax = [lattice_axis(bbox[0][a], bbox[1][a], shape[a]) for a in range(3)]
    g = np.stack(np.meshgrid(ax[0][x0:x1], ax[1], ax[2], indexing="ij"), -1)
    return np.ascontiguousarray(g.reshape(-1, 3), dtype=F)


def _popcount(x):
    x = x.astype(np.int64)
    return sum((x >> k) & 1 for k in range(8))


def extract(field, level, bbox):
    """-> verts float32 [V,3], faces int32 [F,3] of the float32 [nx,ny,nz] field."""
    field = np.ascontiguousarray(field, dtype=F)
    nx, ny, nz = shape = field.shape
    level = F(level)
    inside = field >= level
    ax = [lattice_axis(bbox[0][a], bbox[1][a], shape[a]) for a in range(3)]

    def lo(d):  # the owners of the edges p -> p + d
        return tuple(slice(0, shape[a] - d[a]) for a in range(3))

    def hi(d):
        return tuple(slice(d[a], shape[a]) for a in range(3))

    mask = np.zeros(shape, np.int64)
    for t, d in enumerate(EDGE_DIRS):
        mask[lo(d)] |= (inside[lo(d)] != inside[hi(d)]).astype(np.int64) << t
    count = _popcount(mask)
    off = np.cumsum(count.reshape(-1)).reshape(shape) - count  # exclusive, lattice order
    V = int(count.sum())
    verts = np.zeros((V, 3), F)
    for t, d in enumerate(EDGE_DIRS):
        own = np.zeros(shape, bool)
        own[lo(d)] = (mask[lo(d)] >> t & 1).astype(bool)
        idx = np.argwhere(own)
        if not len(idx):
            continue
        f0 = field[own]
        f1 = field[tuple((idx + np.array(d)).T)]
        tt = (F(level - f0) / (f1 - f0).astype(F)).astype(F)
        ids = off[own] + _popcount(mask[own] & ((1 << t) - 1))
        for a in range(3):
            x0 = ax[a][idx[:, a]]
            x1 = ax[a][idx[:, a] + d[a]]
            verts[ids, a] = (x0 + (tt * (x1 - x0).astype(F)).astype(F)).astype(F)

    def vid(base, v_from, v_to):  # ids of the edges (cube origin + v_from) -> (cube origin + v_to)
        q = tuple((base + v_from).T)
        t = EDGE_TYPE[tuple(int(x) for x in v_to - v_from)]
        return off[q] + _popcount(mask[q] & ((1 << t) - 1))

    faces = []
    for pi, perm in enumerate(PERMS):
        path = tet_path(perm)
        case = np.zeros(tuple(n - 1 for n in shape), np.int64)
        for i, v in enumerate(path):
            case |= inside[tuple(slice(v[a], shape[a] - 1 + v[a]) for a in range(3))].astype(np.int64) << i
        for c in range(1, 15):
            base = np.argwhere(case == c)
            if not len(base):
                continue
            for tri in TABLE[pi][c]:
                faces.append(np.stack([vid(base, path[i], path[j]) for i, j in tri], -1))
    faces = np.concatenate(faces).astype(np.int32) if faces else np.zeros((0, 3), np.int32)
    return verts, faces


# ---------------------------------------------------------------------------------------------
# mesh properties (fp64 / integer; used on the restatement's and on the kernels' output alike)
# ---------------------------------------------------------------------------------------------
def canonical_faces(faces):
    """Each triple rotated so that its smallest id comes first, then the rows sorted: equal for two
    face arrays that hold the same oriented triangles in any order and rotation."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if not len(f):
        return f
    k = np.argmin(f, axis=1)
    r = np.stack([f[np.arange(len(f)), (k + s) % 3] for s in range(3)], -1)
    return r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]


def topology(verts, faces):
    """dict: V, F, E, chi, closed (every undirected edge in exactly two faces, every directed edge once
    and its reverse present), volume (signed, fp64), degenerate (faces of zero area or a repeated id)."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    key = de[:, 0] * (len(v) + 1) + de[:, 1]
    rkey = de[:, 1] * (len(v) + 1) + de[:, 0]
    ue = np.sort(de, axis=1)
    _, ucount = np.unique(ue[:, 0] * (len(v) + 1) + ue[:, 1], return_counts=True)
    directed_once = len(np.unique(key)) == len(key)
    reversed_present = bool(np.isin(rkey, key).all())
    closed = bool(len(f) > 0 and (ucount == 2).all() and directed_once and reversed_present)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    volume = float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    return {"V": len(v), "F": len(f), "E": len(ucount), "chi": len(v) - len(ucount) + len(f), "closed": closed,
            "volume": volume, "degenerate": int((area2 == 0).sum())}


# ---------------------------------------------------------------------------------------------
# the analytic fields of the tests: 32 + 40 * (r - dist) at level 32, fp64 on the float32 lattice
# ---------------------------------------------------------------------------------------------
LEVEL = 32.0
LEGO_BOX = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))


def _xyz(shape, bbox):
    return lattice(shape, bbox).astype(np.float64).reshape(*shape, 3)


def sphere_field(shape, bbox, r, centre=(0.0, 0.0, 0.0)):
    d = np.linalg.norm(_xyz(shape, bbox) - np.asarray(centre, np.float64), axis=-1)
    return (32.0 + 40.0 * (r - d)).astype(F)


def torus_field(shape, bbox, R, r):
    p = _xyz(shape, bbox)
    d = np.sqrt((np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - R) ** 2 + p[..., 2] ** 2)
    return (32.0 + 40.0 * (r - d)).astype(F)


def two_spheres_field(shape, bbox):
    return np.maximum(sphere_field(shape, bbox, 0.5, (0.7, 0, 0)), sphere_field(shape, bbox, 0.45, (-0.7, 0, 0)))


def octahedron_field(shape, bbox):
    """32 + 6 - (|x| + |y| + |z|): integer values on an integer lattice, some equal to the level."""
    p = _xyz(shape, bbox)
    return (32.0 + 6.0 - np.abs(p).sum(-1)).astype(F)


SPHERE_VOLUME = 4.0 / 3.0 * np.pi * 0.9 ** 3
TORUS_VOLUME = 2.0 * np.pi ** 2 * 0.9 * 0.3 ** 2
BOX_B = ((-1.5, -1.0, -2.0), (1.5, 1.25, 1.0))
BOX_T = ((-1.5, -1.5, -0.75), (1.5, 1.5, 0.75))

# name -> (shape, bbox, field builder, expected V, F, chi, solid volume or None, lower volume bound or None)
CASES = {
    "sphere9": ((9, 9, 9), LEGO_BOX, lambda s, b: sphere_field(s, b, 0.9), 326, 648, 2, SPHERE_VOLUME, 0.90),
    "sphere17": ((17, 17, 17), LEGO_BOX, lambda s, b: sphere_field(s, b, 0.9), 1262, 2520, 2, SPHERE_VOLUME, 0.97),
    "sphere33": ((33, 33, 33), LEGO_BOX, lambda s, b: sphere_field(s, b, 0.9), 5210, 10416, 2, SPHERE_VOLUME, 0.99),
    "sphere_box": ((9, 12, 17), BOX_B, lambda s, b: sphere_field(s, b, 0.8, (0, 0, -0.5)), 658, 1312, 2,
                   4.0 / 3.0 * np.pi * 0.8 ** 3, None),
    "torus": ((25, 25, 13), BOX_T, lambda s, b: torus_field(s, b, 0.9, 0.3), 3060, 6120, 0, TORUS_VOLUME, None),
    "two_spheres": ((17, 17, 17), LEGO_BOX, two_spheres_field, 736, 1464, 4, None, None),
}
