// Mesh export (include/nerf_amd.h "mesh"; DESIGN.md 4 "Mesh export"): the level set of a density lattice as an
// indexed, welded, consistently oriented triangle mesh, by marching tetrahedra on the Kuhn split.
//
// Every lattice cube is cut into the six tetrahedra p, p + e_a, p + e_a + e_b, p + (1,1,1), one per permutation
// (a, b, c) of the axes.  Their edges are the seven directions MESH_EDGE_CORNER below; lattice point p owns the
// edges p -> p + d that stay in the lattice, a crossing edge carries one vertex, and a vertex id is
//   vert_off[p] + popcount(mask[p] & ((1 << type) - 1)),
// so welding is a prefix sum over the points (the caller's) -- no hash, no sort, no atomic, and the output is a pure
// function of the field.  One thread per lattice point, z fastest: the loads of a wave are 64 consecutive floats of
// up to four z-rows, the stores follow the offsets in the same order.
#include "grid_common.h"
#include "nerf_amd.h"
#include <math.h>

namespace nerf {

struct MeshDims {
  int n[3];  // nx, ny, nz
};

// corner c of the cube at p is p + (c & 1, c >> 1 & 1, c >> 2 & 1); the edge of type t runs from corner 0 to
// corner MESH_EDGE_CORNER[t]: d = (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1)
__device__ constexpr int MESH_EDGE_CORNER[7] = {1, 2, 4, 3, 5, 6, 7};
// the inverse, three bits per corner difference: type = MESH_TYPE_OF >> 3 * (ci ^ cj) & 7
constexpr unsigned MESH_TYPE_OF = (0u << 3) | (1u << 6) | (3u << 9) | (2u << 12) | (4u << 15) | (5u << 18) | (6u << 21);

// The triangles of a tetrahedron with path vertices 0..3 and inside bits `case` (bit i: vertex i is inside), for an
// even permutation: bits 0-1 the count, then 12 bits per triangle, 4 per edge (i | j << 2, i < j).  One inside
// vertex i: the edges (i, j) to the outside; three: the edges (j, k) to the outside vertex k; two, S = {i < j} and
// O = {k < l}: the quad (i,k), (i,l), (j,l), (j,k) split along (i,k)-(j,l).  Each is wound so that its right-hand
// normal points from the inside to the outside; an odd permutation mirrors the tetrahedron, so its triangles swap
// their last two edges.  (tests/mesh_numpy.py derives the same table from the geometry.)
__device__ constexpr unsigned MESH_TRI[16] = {0x0000000u, 0x0003211u, 0x0002751u, 0x2763722u, 0x0003a61u, 0x3a53392u,
                                              0x2393b52u, 0x0003b71u, 0x00037b1u, 0x3793a12u, 0x3b12792u, 0x00027a1u,
                                              0x3363662u, 0x0003651u, 0x0002311u, 0x0000000u};
// the permutations in lexicographic order as (a, b) and their parity
__device__ constexpr int MESH_PERM_A[6] = {0, 0, 1, 1, 2, 2};
__device__ constexpr int MESH_PERM_B[6] = {1, 2, 0, 2, 0, 1};
__device__ constexpr int MESH_PERM_ODD[6] = {0, 1, 1, 0, 0, 1};

__device__ __forceinline__ float mesh_coord(const BBox& b, const MeshDims& d, int a, int i) {
  const float h = fdiv(fsub(b.mx[a], b.mn[a]), (float)(d.n[a] - 1));
  return fadd(b.mn[a], fmul((float)i, h));
}

// point index -> (ix, iy, iz); P < 2^31
__device__ __forceinline__ void mesh_decode(const MeshDims& d, unsigned p, int i[3]) {
  const unsigned q = p / (unsigned)d.n[2];
  i[2] = (int)(p - q * (unsigned)d.n[2]);
  i[0] = (int)(q / (unsigned)d.n[1]);
  i[1] = (int)(q - (unsigned)i[0] * (unsigned)d.n[1]);
}

__device__ __forceinline__ int64_t mesh_corner_offset(const MeshDims& d, int c) {
  return (int64_t)(c & 1) * d.n[1] * d.n[2] + (int64_t)(c >> 1 & 1) * d.n[2] + (c >> 2 & 1);
}

// the field at the eight corners of p's cube; a corner outside the lattice repeats p's own value, so that its edge
// never crosses.  -> the inside bits (bit c: v[c] >= level)
__device__ __forceinline__ unsigned mesh_corners(const float* __restrict__ field, const MeshDims& d, int64_t p,
                                                 const int i[3], float level, float v[8]) {
  unsigned in = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bool ok = (!(c & 1) || i[0] + 1 < d.n[0]) && (!(c & 2) || i[1] + 1 < d.n[1]) && (!(c & 4) || i[2] + 1 < d.n[2]);
    v[c] = ok ? field[p + mesh_corner_offset(d, c)] : v[0];  // (corner 0 is p itself)
    in |= (unsigned)(v[c] >= level) << c;
  }
  return in;
}

__device__ __forceinline__ bool mesh_is_cube(const MeshDims& d, const int i[3]) {
  return i[0] + 1 < d.n[0] && i[1] + 1 < d.n[1] && i[2] + 1 < d.n[2];
}
__device__ __forceinline__ int64_t mesh_cube_index(const MeshDims& d, const int i[3]) {
  return ((int64_t)i[0] * (d.n[1] - 1) + i[1]) * (d.n[2] - 1) + i[2];
}

// inside bits of the path vertices of permutation k
__device__ __forceinline__ unsigned mesh_case(unsigned in, int k) {
  const int c1 = 1 << MESH_PERM_A[k], c2 = c1 | 1 << MESH_PERM_B[k];
  return (in & 1) | (in >> c1 & 1) << 1 | (in >> c2 & 1) << 2 | (in >> 7 & 1) << 3;
}

// ---- lattice points of the x-planes [x0, x1) ----
__global__ void mesh_lattice_kernel(MeshDims d, BBox b, int x0, int64_t count, float* __restrict__ pts) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  int i[3];
  mesh_decode(d, (unsigned)(t + (int64_t)x0 * d.n[1] * d.n[2]), i);
#pragma unroll
  for (int a = 0; a < 3; ++a) pts[t * 3 + a] = mesh_coord(b, d, a, i[a]);
}

// ---- crossing edges per point, triangles per cube ----
__global__ void mesh_classify_kernel(const float* __restrict__ field, MeshDims d, int64_t P, float level,
                                     uint8_t* __restrict__ edge_mask, int32_t* __restrict__ vert_count,
                                     int32_t* __restrict__ tri_count) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  int i[3];
  mesh_decode(d, (unsigned)p, i);
  float v[8];
  const unsigned in = mesh_corners(field, d, p, i, level, v);
  unsigned mask = 0;
#pragma unroll
  for (int t = 0; t < 7; ++t) mask |= ((in >> MESH_EDGE_CORNER[t] ^ in) & 1u) << t;
  edge_mask[p] = (uint8_t)mask;
  vert_count[p] = __popc(mask);
  if (!mesh_is_cube(d, i)) return;
  int n = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) n += (int)(MESH_TRI[mesh_case(in, k)] & 3u);
  tri_count[mesh_cube_index(d, i)] = n;
}

// ---- the vertices a point owns and the faces of its cube ----
struct MeshEmitArgs {
  const float* field;
  MeshDims d;
  BBox b;
  int64_t P;
  float level;
  const uint8_t* edge_mask;
  const int64_t* vert_off;
  const int64_t* tri_off;
  int64_t n_verts, n_faces;  // the sizes of verts / faces: nothing is written past them
  float* verts;
  int32_t* faces;
};

__global__ void mesh_emit_kernel(MeshEmitArgs a) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.P) return;
  const MeshDims d = a.d;
  int i[3];
  mesh_decode(d, (unsigned)p, i);
  float v[8];
  const unsigned in = mesh_corners(a.field, d, p, i, a.level, v);
  if (in == 0u || in == 255u) return;  // no crossing edge and no face here (an outside corner repeats v[0])

  const unsigned mask = a.edge_mask[p];
  if (mask) {
    int64_t o = a.vert_off[p];
#pragma unroll
    for (int t = 0; t < 7; ++t) {
      if (!(mask >> t & 1u)) continue;
      const int c = MESH_EDGE_CORNER[t];
      const float s = fdiv(fsub(a.level, v[0]), fsub(v[c], v[0]));  // from the owner end
      if (o < a.n_verts) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float x0 = mesh_coord(a.b, d, k, i[k]), x1 = mesh_coord(a.b, d, k, i[k] + (c >> k & 1));
          a.verts[o * 3 + k] = fadd(x0, fmul(s, fsub(x1, x0)));
        }
      }
      ++o;
    }
  }

  if (!mesh_is_cube(d, i)) return;
  int64_t o = a.tri_off[mesh_cube_index(d, i)];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const int c1 = 1 << MESH_PERM_A[k], c2 = c1 | 1 << MESH_PERM_B[k];
    const unsigned corners = (unsigned)c1 << 3 | (unsigned)c2 << 6 | 7u << 9;  // path vertex j -> cube corner
    const unsigned w = MESH_TRI[mesh_case(in, k)];
    const int n = (int)(w & 3u);
    for (int tri = 0; tri < n; ++tri) {
      const unsigned code = w >> (2 + 12 * tri);
      int32_t id[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const unsigned ci = corners >> 3 * (code >> 4 * e & 3u) & 7u;        // the owner end (i < j on the path)
        const unsigned cj = corners >> 3 * (code >> (4 * e + 2) & 3u) & 7u;
        const unsigned type = MESH_TYPE_OF >> 3 * (ci ^ cj) & 7u;
        const int64_t q = p + mesh_corner_offset(d, (int)ci);
        id[e] = (int32_t)(a.vert_off[q] + __popc((unsigned)a.edge_mask[q] & ((1u << type) - 1u)));
      }
      if (o < a.n_faces) {
        a.faces[o * 3 + 0] = id[0];
        a.faces[o * 3 + 1] = id[MESH_PERM_ODD[k] ? 2 : 1];
        a.faces[o * 3 + 2] = id[MESH_PERM_ODD[k] ? 1 : 2];
      }
      ++o;
    }
  }
}

static int mesh_dims(const char* who, int nx, int ny, int nz, MeshDims* d, int64_t* P) {
  NERF_REQUIRE(nx >= 2 && ny >= 2 && nz >= 2, "%s: every lattice axis needs at least 2 points, got %d x %d x %d", who,
               nx, ny, nz);
  const int64_t yz = (int64_t)ny * nz;
  NERF_REQUIRE(yz <= INT32_MAX && (int64_t)nx <= INT32_MAX / yz, "%s: nx * ny * nz must be below 2^31", who);
  *d = MeshDims{{nx, ny, nz}};
  *P = (int64_t)nx * yz;
  return 0;
}

}  // namespace nerf

// ======================================================================================
// C-ABI
// ======================================================================================
using namespace nerf;

extern "C" {

int nerf_mesh_lattice(const float* bbox_host, int nx, int ny, int nz, int x0, int x1, float* pts, hipStream_t stream) {
  MeshDims d;
  int64_t P;
  if (int rc = mesh_dims("nerf_mesh_lattice", nx, ny, nz, &d, &P)) return rc;
  NERF_REQUIRE(bbox_host && 0 <= x0 && x0 <= x1 && x1 <= nx, "nerf_mesh_lattice: bad bbox or x-planes [%d, %d)", x0,
               x1);
  if (x0 == x1) return 0;
  NERF_REQUIRE(pts, "nerf_mesh_lattice: null pointer");
  const int64_t count = (int64_t)(x1 - x0) * ny * nz;
  hipLaunchKernelGGL(mesh_lattice_kernel, grid1(count), dim3(256), 0, stream, d, make_bbox(bbox_host), x0, count, pts);
  return check_launch("nerf_mesh_lattice");
}

int nerf_mesh_classify(const float* field, int nx, int ny, int nz, float level, uint8_t* edge_mask,
                       int32_t* vert_count, int32_t* tri_count, hipStream_t stream) {
  MeshDims d;
  int64_t P;
  if (int rc = mesh_dims("nerf_mesh_classify", nx, ny, nz, &d, &P)) return rc;
  NERF_REQUIRE(isfinite(level), "nerf_mesh_classify: level must be finite");
  NERF_REQUIRE(field && edge_mask && vert_count && tri_count, "nerf_mesh_classify: null pointer");
  hipLaunchKernelGGL(mesh_classify_kernel, grid1(P), dim3(256), 0, stream, field, d, P, level, edge_mask, vert_count,
                     tri_count);
  return check_launch("nerf_mesh_classify");
}

int nerf_mesh_emit(const float* field, const float* bbox_host, int nx, int ny, int nz, float level,
                   const uint8_t* edge_mask, const int64_t* vert_off, const int64_t* tri_off, int64_t n_verts,
                   int64_t n_faces, float* verts, int32_t* faces, hipStream_t stream) {
  MeshDims d;
  int64_t P;
  if (int rc = mesh_dims("nerf_mesh_emit", nx, ny, nz, &d, &P)) return rc;
  NERF_REQUIRE(isfinite(level) && bbox_host, "nerf_mesh_emit: level must be finite and bbox non-null");
  NERF_REQUIRE(n_verts >= 0 && n_verts <= INT32_MAX && n_faces >= 0, "nerf_mesh_emit: vertex ids are int32");
  if (n_verts == 0 && n_faces == 0) return 0;
  NERF_REQUIRE(field && edge_mask && vert_off && tri_off && (verts || !n_verts) && (faces || !n_faces),
               "nerf_mesh_emit: null pointer");
  MeshEmitArgs a{field, d, make_bbox(bbox_host), P, level, edge_mask, vert_off, tri_off, n_verts, n_faces, verts, faces};
  hipLaunchKernelGGL(mesh_emit_kernel, grid1(P), dim3(256), 0, stream, a);
  return check_launch("nerf_mesh_emit");
}

}  // extern "C"
