// Fused NeRF MLP: the packed-weight layout and the pack kernels.
#pragma once
#include "mlp_policy.h"

namespace nerf {
namespace mlp {

// ------------------------------------------------------------------------------------
// packed-weight layout (1 KiB chunks, lane-linear: chunk[lane][16 B])
//   forward unit u: fwd_unit_tiles(u) * CH weight chunks, then 1 bias chunk (32 fp32)
//   backward unit u: bwd_unit_tiles(u) * CH weight chunks
// ------------------------------------------------------------------------------------
// DIR 0: forward units, 1: dX-chain units, 2: 16-row forward units (PBF3W)
// DIR 3: 16-row dX units (PF32W / PBF3W)
// DIR 4: the 16-row forward units of DIR 2 computed from the DIR 0 pack of PF32 (the wide fp32 forward, PF32W):
//        the two 16-row units 2n, 2n + 1 of a layer are the row halves of 32-row unit n and share its chunks
constexpr int DIR_F32W = 4;
__host__ __device__ constexpr int num_units(int dir) {
  return dir == 0 ? NUNIT_FWD : dir == 1 ? NUNIT_BWD : (dir == 2 || dir == DIR_F32W) ? NUNIT_FWD16 : NUNIT_BWD16;
}
// DIR 4: the 32-row unit (of DIR 0) that holds 16-row unit u, and the 16-row units of a 32-row unit
__host__ __device__ constexpr int f32w_unit32(int u) {
  const int L = fwd16_unit_layer(u);
  return fwd_unit_first(L) + ((u - fwd16_unit_first(L)) >> 1);
}
__host__ __device__ constexpr int f32w_unit16_first(int u32) {
  const int L = fwd_unit_layer(u32);
  return fwd16_unit_first(L) + 2 * (u32 - fwd_unit_first(L));
}
__host__ __device__ constexpr int f32w_unit16_count(int u32) {
  const int L = fwd_unit_layer(u32);
  return L == LRGB || (L == LFA && u32 - fwd_unit_first(L) == 8) ? 1 : 2;  // (all-padding row halves are skipped)
}
__host__ __device__ constexpr int fwd_unit_chunks(int u, int ch) { return fwd_unit_tiles(u) * ch + 1; }
__host__ __device__ constexpr int fwd16_unit_chunks(int u, int ch) { return fwd16_unit_tiles(u) * ch + 1; }
__host__ __device__ constexpr int fwd16_unit_chunk_off(int u, int ch) { return fwd16_unit_tile_off(u) * ch + u; }
__host__ __device__ constexpr int fwd_unit_chunk_off(int u, int ch) { return fwd_unit_tile_off(u) * ch + u; }
__host__ __device__ constexpr int bwd_unit_chunks(int u, int ch) { return bwd_unit_tiles(u) * ch; }
__host__ __device__ constexpr int bwd_unit_chunk_off(int u, int ch) { return bwd_unit_tile_off(u) * ch; }
__host__ __device__ constexpr int bwd16_unit_chunks(int u, int ch) { return bwd16_unit_tiles(u) * ch; }
__host__ __device__ constexpr int bwd16_unit_chunk_off(int u, int ch) { return bwd16_unit_tile_off(u) * ch; }
__host__ __device__ constexpr int64_t total_chunks(int ch, int dir) {
  return dir == 0 ? (int64_t)FWD_TILES * ch + NUNIT_FWD
       : dir == 1 ? (int64_t)BWD_TILES * ch
       : dir == 2 ? (int64_t)FWD16_TILES * ch + NUNIT_FWD16
       : (int64_t)BWD16_TILES * ch;
}

struct ParamPtrs { const float* p[NPARAM]; };

// first chunk of every unit (+ the end), evaluated at compile time and passed by value:
// the unit of a chunk is then a scan of kernel arguments, not a runtime walk of the
// constexpr layout functions (which are loops)
struct UnitOffsets { int off[NUNIT_MAX + 1]; };
template <int CH, int DIR>
constexpr UnitOffsets unit_offsets() {
  UnitOffsets t{};
  const int nu = num_units(DIR);
  for (int u = 0; u <= nu; ++u)
    t.off[u] = DIR == 0 ? fwd_unit_chunk_off(u, CH) : DIR == 1 ? bwd_unit_chunk_off(u, CH)
             : DIR == 2 ? fwd16_unit_chunk_off(u, CH) : bwd16_unit_chunk_off(u, CH);
  return t;
}

// one thread per 16-B lane slot of one chunk
// The sources of packed lane-chunk i (chunk i >> 6, lane i & 63): weight(e, wp, idx, c) for each of its
// E elements (wp = -1: a zero element; else element idx of parameter wp, split part c of P::cvt_c), or, on
// a forward unit's bias chunk, bias(e, wp, idx) for its 4 fp32 values.
template <class P, int DIR, class Weight, class Bias>
__device__ __forceinline__ void pack_sources(int64_t i, const UnitOffsets& uo, Weight&& weight, Bias&& bias) {
  const int lane = (int)(i & 63);
  const int chunk = (int)(i >> 6);
  const int r = lane & 31, h = lane >> 5;
  const int nunit = num_units(DIR);
  int u = 0;
  for (int k = 1; k < nunit; ++k) u += uo.off[k] <= chunk ? 1 : 0;
  const int within = chunk - uo.off[u];
  if constexpr (DIR == 2) {
    // 16-row unit (PBF3W, PF32W): lane l = r16 + 16 g holds weight row r16 of the unit, the E features
    // P::feat16(c, g, e) of K-block t, split part P::part16(c) (PBF3W: all 8 features of lane group g, chunk
    // c = 0 the hi, 1 the lo halves; PF32W: the 4 features 16 c + 4 g + e).  Bias chunk: lanes 0..3 hold
    // rows 4 lane + e (the accumulator's rows of lane group g = lane), rest zero.
    const int L = fwd16_unit_layer(u), m = u - fwd16_unit_first(L);
    const int w = fwd16_out_weight(L, m);
    if (within == fwd16_unit_tiles(u) * P::CH) {
      for (int e = 0; e < 4; ++e) {
        const int row = lane * 4 + e;
        const bool ok = lane < 4 && row < fwd16_out_valid(L, m);
        bias(e, ok ? w + 1 : -1, (int64_t)(fwd16_out_row0(L, m) + row));
      }
      return;
    }
    const int t = within / P::CH, c = within % P::CH, r16 = lane & 15, g = lane >> 4;
#pragma unroll
    for (int e = 0; e < P::E; ++e) {
      const int f = P::feat16(c, g, e);
      const bool ok = r16 < fwd16_out_valid(L, m) && f < fwd_in_valid(L, t);
      weight(e, ok ? w : -1,
             ok ? (int64_t)(fwd16_out_row0(L, m) + r16) * weight_K(w) + fwd_in_colbase(L, t) + f : (int64_t)0,
             P::part16(c));
    }
    return;
  }
  if constexpr (DIR == 3) {
    // 16-row dX unit (PF32W / PBF3W): half m & 1 of W^T output tile m >> 1 of stage s.  Lane l = r16 + 16 g holds
    // A[i][p] = W[p][i] for dX row i = the forward in-feature bwd_out_colbase + 16 (m & 1) + r16 and the E forward
    // out-features p = row0 + P::feat16(c, g, e) of input K-block t (forward output tile t of the stage's layer)
    const int s = bwd16_unit_stage(u), m = u - bwd16_unit_first(s), L = bwd_fwd_layer(s);
    const int t = within / P::CH, c = within % P::CH, r16 = lane & 15, g = lane >> 4;
    const int w = fwd_out_weight(L, t), i = bwd_out_colbase(s, m >> 1) + 16 * (m & 1) + r16;
#pragma unroll
    for (int e = 0; e < P::E; ++e) {
      const int f = P::feat16(c, g, e);
      const bool ok = f < fwd_out_valid(L, t);
      weight(e, ok ? w : -1, ok ? (int64_t)(fwd_out_row0(L, t) + f) * weight_K(w) + i : (int64_t)0, P::part16(c));
    }
    return;
  }
  if (DIR == 0 && within == fwd_unit_tiles(u) * P::CH) {
    // bias chunk: lanes 0..7 hold the 32 biases of the unit's output rows, rest zero
    const int L = fwd_unit_layer(u), n = u - fwd_unit_first(L);
    const int wp = fwd_out_weight(L, n);
    for (int e = 0; e < 4; ++e) {
      const int row = lane * 4 + e;
      const bool ok = lane < 8 && row < fwd_out_valid(L, n);
      bias(e, ok ? wp + 1 : -1, (int64_t)(fwd_out_row0(L, n) + row));
    }
    return;
  }
  const int t = within / P::CH, c = within % P::CH;
#pragma unroll
  for (int e = 0; e < P::E; ++e) {
    const int rho = P::rho_of(c, e);
    const int ar = acc_row(rho, h);
    int wp = -1;
    int64_t idx = 0;
    if (DIR == 0) {
      const int L = fwd_unit_layer(u), n = u - fwd_unit_first(L);
      const int w = fwd_out_weight(L, n);
      const int row = fwd_out_row0(L, n) + r, col = fwd_in_colbase(L, t) + ar;
      if (r < fwd_out_valid(L, n) && ar < fwd_in_valid(L, t)) wp = w, idx = (int64_t)row * weight_K(w) + col;
    } else {
      // A[i = forward in-feature (r)][p = forward out-feature of forward tile t (ar)]
      const int s = bwd_unit_stage(u), j = u - bwd_unit_first(s), L = bwd_fwd_layer(s);
      const int w = fwd_out_weight(L, t);
      const int row = fwd_out_row0(L, t) + ar, col = bwd_out_colbase(s, j) + r;
      if (ar < fwd_out_valid(L, t)) wp = w, idx = (int64_t)row * weight_K(w) + col;
    }
    weight(e, wp, idx, c);
  }
}

// direct pack (any parameter layout): one thread per lane-chunk, the sources walked on the device
template <class P, int DIR>
__global__ void pack_kernel(ParamPtrs prm, UnitOffsets uo, char* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total_chunks(P::CH, DIR) * 64) return;
  char* dst = out + i * 16;
  typename P::Store vals[P::E];
  bool is_bias = false;
  pack_sources<P, DIR>(
      i, uo,
      [&](int e, int wp, int64_t idx, int c) { vals[e] = P::cvt_c(wp < 0 ? 0.f : prm.p[wp][idx], c); },
      [&](int e, int wp, int64_t idx) {
        is_bias = true;
        ((float*)dst)[e] = wp < 0 ? 0.f : prm.p[wp][idx];
      });
  if (is_bias) return;
#pragma unroll
  for (int e = 0; e < P::E; ++e) ((typename P::Store*)dst)[e] = vals[e];
}

// Pack plan (r5): the sources of every packed element, built once per (policy, direction, device) by
// pack_plan_kernel, so that the per-step repack of a net whose 24 parameters lie back to back (FusedAdam's
// flat buffer) is one gather (pack_gather_kernel: ~30 instructions per lane-chunk instead of the ~2,000 of
// the unit / layer walk above, bit-identical).  Entry: bits 0-23 the element's offset in the net's flat
// parameters, bits 24-26 the split part c; PLAN_ZERO a zero element; PLAN_BIAS in entry E - 1 marks a
// bias lane-chunk whose entries 0-3 are fp32 values (E = 8 policies; fp32's E = 4 stores floats anyway).
constexpr uint32_t PLAN_ZERO = 0xFFFFFFFFu;
constexpr uint32_t PLAN_BIAS = 0xFE000000u;
template <class P, int DIR>
__global__ void pack_plan_kernel(UnitOffsets uo, uint32_t* plan) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total_chunks(P::CH, DIR) * 64) return;
  uint32_t* pl = plan + i * P::E;
  auto code = [](int wp, int64_t idx, int c) {
    return wp < 0 ? PLAN_ZERO : (uint32_t)(param_offset(wp) + idx) | ((uint32_t)c << 24);
  };
  bool is_bias = false;
  uint32_t ent[P::E];
  pack_sources<P, DIR>(
      i, uo, [&](int e, int wp, int64_t idx, int c) { ent[e] = code(wp, idx, c); },
      [&](int e, int wp, int64_t idx) {
        is_bias = true;
        ent[e] = code(wp, idx, 0);
      });
  if (is_bias)
    for (int e = 4; e < P::E; ++e) ent[e] = e == P::E - 1 ? PLAN_BIAS : PLAN_ZERO;
  for (int e = 0; e < P::E; ++e) pl[e] = ent[e];
}
template <class P>
__global__ void pack_gather_kernel(const float* __restrict__ flat, const uint32_t* __restrict__ plan, char* out,
                                   int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t ent[P::E];
#pragma unroll
  for (int q = 0; q < P::E / 4; ++q) {
    const uint4 v = ((const uint4*)(plan + i * P::E))[q];
    ent[4 * q] = v.x, ent[4 * q + 1] = v.y, ent[4 * q + 2] = v.z, ent[4 * q + 3] = v.w;
  }
  char* dst = out + i * 16;
  if (P::E == 8 && ent[P::E - 1] == PLAN_BIAS) {
    float f[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = ent[e] == PLAN_ZERO ? 0.f : flat[ent[e] & 0xFFFFFFu];
    *(float4*)dst = make_float4(f[0], f[1], f[2], f[3]);
    return;
  }
  typename P::Store vals[P::E];
#pragma unroll
  for (int e = 0; e < P::E; ++e)
    vals[e] = P::cvt_c(ent[e] == PLAN_ZERO ? 0.f : flat[ent[e] & 0xFFFFFFu], (int)((ent[e] >> 24) & 7u));
  static_assert(sizeof(vals) == 16, "a lane-chunk is 16 bytes");
  *(uint4*)dst = __builtin_bit_cast(uint4, vals);
}

}  // namespace mlp
}  // namespace nerf
