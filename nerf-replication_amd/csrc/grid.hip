// Occupancy grid on gfx950: cell lookup, baking and the online update.  The march that reads the
// grid is march.hip; what the two share is grid_common.h.
//
// Reference semantics (echo636/nerf-replication):
//   world_to_grid_indices   src/models/nerf/renderer/volume_renderer.py:261-265
//   grid bake               occupancy_grid.py:15-80
#include "grid_common.h"

namespace nerf {

struct GridIndexArgs {
  const float* pts;
  int64_t M;
  BBox bb;
  int res;
  const uint8_t* grid;
  int64_t* idx;
  uint8_t* occ;
};

__global__ void grid_index_kernel(GridIndexArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.M) return;
  int ix = grid_axis(a.pts[i * 3 + 0], a.bb.mn[0], a.bb.mx[0], a.res);
  int iy = grid_axis(a.pts[i * 3 + 1], a.bb.mn[1], a.bb.mx[1], a.res);
  int iz = grid_axis(a.pts[i * 3 + 2], a.bb.mn[2], a.bb.mx[2], a.res);
  if (a.idx) {
    a.idx[i * 3 + 0] = ix;
    a.idx[i * 3 + 1] = iy;
    a.idx[i * 3 + 2] = iz;
  }
  if (a.occ) a.occ[i] = a.grid[((int64_t)ix * a.res + iy) * a.res + iz];
}

// ------------------------------------------------------------------------------------
// bake
// ------------------------------------------------------------------------------------
// A bake covers the voxel slab x in [x0, x1) (the whole grid: [0, res)); point and grid
// indices are slab-relative.
struct BakeArgs {
  int res;
  BBox bb;
  int dedup;   // 1: (x1-x0+1)(res+1)^2 lattice points; 0: (x1-x0) res^2 x 8 corners
  int x0, x1;
  float* pts;
};

__device__ __forceinline__ float voxel_size(const BBox& bb, int k, int res) {
  return fdiv(fsub(bb.mx[k], bb.mn[k]), (float)res);
}

__global__ void bake_points_kernel(BakeArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nx = a.x1 - a.x0;
  if (a.dedup) {
    const int64_t n = (int64_t)(a.res + 1);
    if (i >= (nx + 1) * n * n) return;
    const int L[3] = {a.x0 + (int)(i / (n * n)), (int)((i / n) % n), (int)(i % n)};
#pragma unroll
    for (int k = 0; k < 3; ++k)
      a.pts[i * 3 + k] = fadd(a.bb.mn[k], fmul((float)L[k], voxel_size(a.bb, k, a.res)));
  } else {
    const int64_t n = (int64_t)a.res;
    if (i >= nx * n * n * 8) return;
    const int64_t v = i >> 3;
    const int c = (int)(i & 7);  // meshgrid 'ij' over the 2x2x2 corner offsets
    const int idx[3] = {a.x0 + (int)(v / (n * n)), (int)((v / n) % n), (int)(v % n)};
    const int off[3] = {(c >> 2) & 1, (c >> 1) & 1, c & 1};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float vs = voxel_size(a.bb, k, a.res);
      const float base = fadd(a.bb.mn[k], fmul((float)idx[k], vs));
      a.pts[i * 3 + k] = fadd(base, off[k] ? vs : 0.f);
    }
  }
}

struct BakeReduceArgs {
  const float* raw;  // [P,4] (slab points)
  int res, dedup;
  int x0, x1;
  float threshold;
  uint8_t* grid;     // [x1 - x0][res][res]
};

__global__ void bake_reduce_kernel(BakeReduceArgs a) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = a.res;
  if (v >= (int64_t)(a.x1 - a.x0) * n * n) return;
  const int x = (int)(v / (n * n)), y = (int)((v / n) % n), z = (int)(v % n);
  bool occ = false;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    int64_t p;
    if (a.dedup) {
      const int64_t m = n + 1;
      p = ((int64_t)(x + ((c >> 2) & 1)) * m + (y + ((c >> 1) & 1))) * m + (z + (c & 1));
    } else {
      p = v * 8 + c;
    }
    const float s = a.raw[p * 4 + 3];
    const float sigma = s > 0.f ? s : 0.f;  // relu(raw[..., 3])
    occ |= sigma > a.threshold;
  }
  a.grid[v] = occ ? 1 : 0;
}

// ------------------------------------------------------------------------------------
// online grid update (training from scratch through the march)
// ------------------------------------------------------------------------------------
// The trainer keeps a fp32 density per cell and re-derives the uint8 occupancy the march reads.
// An update visits the slots [s0, s0 + n) of the bijection pi(s) = (s A + B) mod res^3 (A coprime
// to res^3): a cell appears at most once per update, so no atomics and no dependence on arrival
// order.  One jittered point per visited cell, INSIDE the cell of the march's own lookup
// (grid_axis): cell i < res - 1 covers the normalised coordinate [i / (res-1), (i+1) / (res-1)),
// cell res - 1 only the bbox face (and, clamped, everything beyond it), so it is sampled at the face.
struct UpdatePointsArgs {
  int64_t s0, n;
  int res;
  BBox bb;
  uint64_t A, B, C;  // C = res^3 < 2^31, A, B < C: s A + B < 2^63
  uint64_t seed, update;
  int32_t* cells;    // [n]
  float* pts;        // [n,3]
};

// mn + ((i + u) / (res-1)) (mx - mn) does not always round-trip through grid_axis in fp32 (a
// coordinate an ulp below a cell boundary lands in the neighbour); the cell's centre does, so the
// index is re-evaluated on the coordinate produced and the centre taken when it differs.
__device__ __forceinline__ float update_coord(int i, float u, float mn, float mx, int res) {
  if (i >= res - 1) return mx;
  const float ext = fsub(mx, mn), rm1 = (float)(res - 1);
  const float p = fadd(mn, fmul(fdiv(fadd((float)i, u), rm1), ext));
  if (grid_axis(p, mn, mx, res) == i) return p;
  return fadd(mn, fmul(fdiv(fadd((float)i, 0.5f), rm1), ext));
}

__global__ void update_points_kernel(UpdatePointsArgs a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t slot = (uint64_t)(a.s0 + i);
  const uint64_t cell = (slot * a.A + a.B) % a.C;
  const int64_t r = a.res;
  const int idx[3] = {(int)(cell / (uint64_t)(r * r)), (int)((cell / (uint64_t)r) % (uint64_t)r),
                      (int)(cell % (uint64_t)r)};
  const uint4 c = make_uint4((uint32_t)slot, (uint32_t)(slot >> 32), (uint32_t)a.update, (uint32_t)(a.update >> 32));
  const uint4 rnd = philox(c, make_uint2((uint32_t)a.seed, (uint32_t)(a.seed >> 32)));
  const float u[3] = {u01(rnd.x), u01(rnd.y), u01(rnd.z)};
  a.cells[i] = (int32_t)cell;
#pragma unroll
  for (int k = 0; k < 3; ++k) a.pts[i * 3 + k] = update_coord(idx[k], u[k], a.bb.mn[k], a.bb.mx[k], a.res);
}

// density[cell] = max(density[cell] * decay, relu(raw[slot, 3])); cells not visited are untouched
__global__ void update_apply_kernel(const int32_t* cells, const float* raw, int64_t n, int64_t C, float decay,
                                    float* density) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t c = cells[i];
  if (c < 0 || c >= C) return;  // (not a cell of this grid: nothing is written)
  const float4 rw = *(const float4*)(raw + i * 4);
  const float sigma = rw.w > 0.f ? rw.w : 0.f;
  density[c] = fmaxf(fmul(density[c], decay), sigma);
}

// mean of the density: two levels, each in a fixed order (a block's threads walk the array with a
// fixed stride and add in double; lanes, then waves, then the blocks' partial sums combine in a
// fixed tree), the launches ordered by the stream -- the same bits every run.
constexpr int UPD_BLOCKS = 1024;
struct UpdateStats { float mean, cut; int32_t occupied, pad; };

__device__ __forceinline__ double block_sum_d(double v, double* lds) {  // 256 threads; the total on thread 0
  v = wave_sum_d(v);
  if (lane_id() == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

__global__ void __launch_bounds__(256) update_mean_partial_kernel(const float* density, int64_t C, int nblocks,
                                                                  double* partial) {
  __shared__ double lds[4];
  double s = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < C; i += (int64_t)nblocks * 256) s += (double)density[i];
  s = block_sum_d(s, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(256) update_mean_final_kernel(const double* partial, int nblocks, int64_t C,
                                                                float threshold, UpdateStats* stats) {
  __shared__ double lds[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 256) s += partial[i];
  s = block_sum_d(s, lds);
  if (threadIdx.x == 0) {
    const float mean = (float)(s / (double)C);
    stats->mean = mean;
    stats->cut = fminf(threshold, mean);
    stats->occupied = 0;
    stats->pad = 0;
  }
}

// grid[c] = density[c] > min(threshold, mean); the occupied count by integer adds (order-free)
__global__ void __launch_bounds__(256) update_threshold_kernel(const float* density, int64_t C, UpdateStats* stats,
                                                               uint8_t* grid) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float cut = stats->cut;
  bool occ = false;
  if (c < C) {
    occ = density[c] > cut;
    grid[c] = occ ? 1 : 0;
  }
  const unsigned long long m = __ballot(occ);
  if (lane_id() == 0 && m) atomicAdd(&stats->occupied, __popcll(m));
}

}  // namespace nerf

// ======================================================================================
// C-ABI
// ======================================================================================
using namespace nerf;

extern "C" {

int nerf_grid_index(const float* pts, int64_t M, const float* bbox_host, int res, const uint8_t* grid,
                    int64_t* idx_out, uint8_t* occ_out, hipStream_t stream) {
  NERF_REQUIRE(M >= 0 && res > 1 && bbox_host, "nerf_grid_index: bad arguments");
  if (M == 0) return 0;
  NERF_REQUIRE(pts && (idx_out || occ_out), "nerf_grid_index: null pointer");
  NERF_REQUIRE(!occ_out || grid, "nerf_grid_index: occupancy needs the grid");
  GridIndexArgs a{pts, M, make_bbox(bbox_host), res, grid, idx_out, occ_out};
  hipLaunchKernelGGL(grid_index_kernel, grid1(M), dim3(256), 0, stream, a);
  return check_launch("nerf_grid_index");
}

int64_t nerf_bake_num_points_slab(int res, int dedup, int x0, int x1) {
  const int64_t n = res, nx = x1 - x0;
  if (res <= 0 || x0 < 0 || x1 > res || nx < 0) return -1;
  if (nx == 0) return 0;
  return dedup ? (nx + 1) * (n + 1) * (n + 1) : nx * n * n * 8;
}
int64_t nerf_bake_num_points(int res, int dedup) { return nerf_bake_num_points_slab(res, dedup, 0, res); }

int nerf_bake_points_slab(int res, const float* bbox_host, int dedup, int x0, int x1, float* pts,
                          hipStream_t stream) {
  NERF_REQUIRE(res > 0 && bbox_host && 0 <= x0 && x0 <= x1 && x1 <= res, "nerf_bake_points: bad arguments");
  if (x0 == x1) return 0;
  NERF_REQUIRE(pts, "nerf_bake_points: null pointer");
  BakeArgs a{res, make_bbox(bbox_host), dedup, x0, x1, pts};
  hipLaunchKernelGGL(bake_points_kernel, grid1(nerf_bake_num_points_slab(res, dedup, x0, x1)), dim3(256), 0, stream,
                     a);
  return check_launch("nerf_bake_points");
}
int nerf_bake_points(int res, const float* bbox_host, int dedup, float* pts, hipStream_t stream) {
  return nerf_bake_points_slab(res, bbox_host, dedup, 0, res, pts, stream);
}

int nerf_bake_reduce_slab(const float* raw, int res, int dedup, int x0, int x1, float threshold, uint8_t* grid,
                          hipStream_t stream) {
  NERF_REQUIRE(res > 0 && 0 <= x0 && x0 <= x1 && x1 <= res, "nerf_bake_reduce: bad arguments");
  if (x0 == x1) return 0;
  NERF_REQUIRE(raw && grid, "nerf_bake_reduce: null pointer");
  BakeReduceArgs a{raw, res, dedup, x0, x1, threshold, grid};
  hipLaunchKernelGGL(bake_reduce_kernel, grid1((int64_t)(x1 - x0) * res * res), dim3(256), 0, stream, a);
  return check_launch("nerf_bake_reduce");
}
int nerf_bake_reduce(const float* raw, int res, int dedup, float threshold, uint8_t* grid, hipStream_t stream) {
  return nerf_bake_reduce_slab(raw, res, dedup, 0, res, threshold, grid, stream);
}

// ---- online grid update ----
static uint64_t gcd_u64(uint64_t a, uint64_t b) {
  while (b) {
    const uint64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

constexpr int UPDATE_MAX_RES = 1290;  // res^3 < 2^31: cell ids are int32, s A + B stays below 2^63

int nerf_grid_update_points(int res, const float* bbox_host, uint64_t stride_a, uint64_t offset_b, uint64_t seed,
                            uint64_t update, int64_t s0, int64_t n, int32_t* cells, float* pts, hipStream_t stream) {
  NERF_REQUIRE(res >= 2 && res <= UPDATE_MAX_RES, "nerf_grid_update_points: res must be in [2, %d]", UPDATE_MAX_RES);
  NERF_REQUIRE(n >= 0, "nerf_grid_update_points: n must be >= 0");
  NERF_REQUIRE(bbox_host, "nerf_grid_update_points: bbox is null");
  const uint64_t C = (uint64_t)res * res * res;
  NERF_REQUIRE(s0 >= 0 && (uint64_t)s0 + (uint64_t)n <= C, "nerf_grid_update_points: slots [s0, s0 + n) must lie in [0, res^3)");
  NERF_REQUIRE(stride_a > 0 && stride_a < C && offset_b < C && gcd_u64(stride_a, C) == 1,
               "nerf_grid_update_points: the stride must be in (0, res^3) and coprime to res^3, the offset below res^3");
  if (n == 0) return 0;
  NERF_REQUIRE(cells && pts, "nerf_grid_update_points: null pointer");
  UpdatePointsArgs a{s0, n, res, make_bbox(bbox_host), stride_a, offset_b, C, seed, update, cells, pts};
  hipLaunchKernelGGL(update_points_kernel, grid1(n), dim3(256), 0, stream, a);
  return check_launch("nerf_grid_update_points");
}

int nerf_grid_update_apply(const int32_t* cells, const float* raw, int64_t n, int res, float decay, float* density,
                           hipStream_t stream) {
  NERF_REQUIRE(res >= 2 && res <= UPDATE_MAX_RES, "nerf_grid_update_apply: res must be in [2, %d]", UPDATE_MAX_RES);
  NERF_REQUIRE(n >= 0, "nerf_grid_update_apply: n must be >= 0");
  if (n == 0) return 0;
  NERF_REQUIRE(cells && raw && density, "nerf_grid_update_apply: null pointer");
  hipLaunchKernelGGL(update_apply_kernel, grid1(n), dim3(256), 0, stream, cells, raw, n, (int64_t)res * res * res,
                     decay, density);
  return check_launch("nerf_grid_update_apply");
}

int64_t nerf_grid_update_workspace_bytes(int res) {
  if (res < 2 || res > UPDATE_MAX_RES) return -1;
  return (int64_t)UPD_BLOCKS * (int64_t)sizeof(double);
}

// stats (device, 16 bytes): float mean, float min(threshold, mean), int32 occupied cells, int32 0
int nerf_grid_update_threshold(const float* density, int res, float threshold, void* workspace, uint8_t* grid,
                               void* stats, hipStream_t stream) {
  NERF_REQUIRE(res >= 2 && res <= UPDATE_MAX_RES, "nerf_grid_update_threshold: res must be in [2, %d]", UPDATE_MAX_RES);
  NERF_REQUIRE(density && workspace && grid && stats, "nerf_grid_update_threshold: null pointer");
  const int64_t C = (int64_t)res * res * res;
  const int nblocks = (int)((C + 255) / 256 < UPD_BLOCKS ? (C + 255) / 256 : UPD_BLOCKS);
  hipLaunchKernelGGL(update_mean_partial_kernel, dim3(nblocks), dim3(256), 0, stream, density, C, nblocks,
                     (double*)workspace);
  if (int e = check_launch("nerf_grid_update_threshold (partial sums)")) return e;
  hipLaunchKernelGGL(update_mean_final_kernel, dim3(1), dim3(256), 0, stream, (const double*)workspace, nblocks, C,
                     threshold, (UpdateStats*)stats);
  if (int e = check_launch("nerf_grid_update_threshold (mean)")) return e;
  hipLaunchKernelGGL(update_threshold_kernel, grid1(C), dim3(256), 0, stream, density, C, (UpdateStats*)stats, grid);
  return check_launch("nerf_grid_update_threshold");
}

}  // extern "C"
