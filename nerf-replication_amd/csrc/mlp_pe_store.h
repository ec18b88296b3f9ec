// Fused NeRF MLP: positional encoding into register tiles, the training stores' layout, the ReLU masks.
#pragma once
#include "mlp_schedule.h"

namespace nerf {
namespace mlp {

// ------------------------------------------------------------------------------------
// positional encoding straight into accumulator-layout tiles
// (freq.py:7-32: [x, sin(2^k x), cos(2^k x)]_k; feature 3 + 6k + {0..2 sin, 3..5 cos})
// ------------------------------------------------------------------------------------
// feature f of an nfreq-band encoding -> (kind, coordinate, band, cos?)
//   kind 0: zero (padding), 1: the raw coordinate, 2: sin/cos(x_dim * 2^k)
struct PeFeat { int kind, dim, k, cos; };
__host__ __device__ constexpr PeFeat pe_feat(int f, int nfreq, int nvalid) {
  if (f >= nvalid) return PeFeat{0, 0, 0, 0};
  if (f < 3) return PeFeat{1, f, 0, 0};
  const int g = f - 3, k = g / 6, r = g % 6;
  if (k >= nfreq) return PeFeat{0, 0, 0, 0};
  return PeFeat{2, r % 3, k, r >= 3 ? 1 : 0};
}

// sin or cos of x * 2^k, three forms (P::PE):
//   PE_FAST (bf16): the angle in revolutions, x * (2^k / 2pi) + (cos ? 1/4 : 0), reduced
//     exactly enough in f64 (|x 2^k| < 2^13 rad keeps ~40 fractional bits), then v_sin_f32 on
//     [0,1) revolutions -- far inside bf16 resolution.
//   PE_LIBM (fp32, the parity path): one libm sincosf of the exact fp32 product x * 2^k (as
//     torch computes x * 2.**k, then sin/cos).  Its large-argument path costs ~140
//     instructions per value, 3-5 % of the fp32 forward, but the cheaper forms below move the
//     4096-ray fine-net L0 gradient 3e-4 from the reference's (a correctly rounded f64 sin
//     does too; libm sincosf: 5e-5, tools/grad_margin.py) against the 1e-4 contract: the fine
//     net's highest PE band amplifies sample-position ulps 512x.
//   PE_POLY (bf16x3, whose own products carry ~1e-5 relative error): the f64 revolution
//     reduction to the nearest quarter turn, t = q/4 + f with |f| <= 1/8, and a Cephes
//     sinf / cosf polynomial of theta = 2 pi f in fp32, chosen and signed by q mod 4:
//     branch-free, ~20 VALU, within 1.6 ulp of sin/cos (forward 12 % faster than libm).
enum PeMode { PE_FAST = 0, PE_LIBM = 1, PE_POLY = 2 };
__device__ __forceinline__ float sin_rev_poly(double t) {
  const double q = __builtin_rint(4.0 * t);
  const double f = __builtin_fma(q, -0.25, t);
  const float th = (float)(f * 6.283185307179586476925286766559);
  const float z = th * th;
  const float s = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z,
                                                -1.6666654611e-1f) * z, th, th);
  const float c = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z,
                                                4.166664568298827e-2f) * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
  const int qi = (int)q;
  const float r = (qi & 1) ? c : s;
  return (qi & 2) ? -r : r;
}

template <int MODE>
__device__ __forceinline__ float pe_trig(float x, double scale_rev, float scale_rad, double phase, bool is_cos) {
  if constexpr (MODE == PE_LIBM) {
    float s, c;
    sincosf(x * scale_rad, &s, &c);
    return is_cos ? c : s;
  } else {
    const double t = __builtin_fma((double)x, scale_rev, phase);
    if constexpr (MODE == PE_FAST) return __builtin_amdgcn_sinf((float)(t - __builtin_floor(t)));
    else return sin_rev_poly(t);
  }
}

// positional encoding straight into accumulator-layout tiles (freq.py:7-32:
// [x, sin(2^k x), cos(2^k x)]_k, feature 3 + 6k + {0..2 sin, 3..5 cos}).  Register rho of
// lane l holds feature 32 tile + acc_row(rho, l >> 5): the two lane halves differ by 4
// features, so each register selects between two compile-time feature descriptors.
template <class P, int TILE, int NFREQ, int NVALID>
__device__ __forceinline__ void pe_tile(typename P::Tile& t, int h, float x0, float x1, float x2) {
  constexpr double INV2PI = 0.15915494309189533576888376337251;
  float vals[16];
  sfor<16>([&](auto rr) {
    constexpr int rho = decltype(rr)::value;
    constexpr PeFeat A = pe_feat(32 * TILE + acc_row(rho, 0), NFREQ, NVALID);
    constexpr PeFeat B = pe_feat(32 * TILE + acc_row(rho, 1), NFREQ, NVALID);
    float v;
    if constexpr (A.kind == 0 && B.kind == 0) {
      v = 0.f;
    } else {
      const int dim = h ? B.dim : A.dim;
      const float x = dim == 0 ? x0 : dim == 1 ? x1 : x2;
      float trig = 0.f;
      if constexpr (A.kind == 2 || B.kind == 2) {
        constexpr int ka = A.kind == 2 ? A.k : (B.kind == 2 ? B.k : 0);
        constexpr int kb = B.kind == 2 ? B.k : ka;
        const int k = h ? kb : ka;
        const bool is_cos = h ? (B.cos != 0) : (A.cos != 0);
        const double srev = INV2PI * (double)(1 << k);
        trig = pe_trig<P::PE>(x, srev, (float)(1 << k), is_cos ? 0.25 : 0.0, is_cos);
      }
      const int kind = h ? B.kind : A.kind;
      v = kind == 2 ? trig : kind == 1 ? x : 0.f;
    }
    if constexpr (P::KIND == K_BF16X3) vals[rho] = v;
    else P::set(t, rho, v);  // (fp32: element-wise keeps the forward's register allocation)
  });
  if constexpr (P::KIND == K_BF16X3) P::pack16(t, vals);
}

// KiB offset of chunk c of tile tau of 32-sample block b in a store of `ntiles` tiles.
// Block-major: one block's tiles are contiguous (a dW job reads a few contiguous runs per
// block instead of one 1-2 KiB piece from each of up to 18 distant tile planes).
__host__ __device__ constexpr int64_t tile_kib(int64_t nblk, int ntiles, int tau, int64_t b, int c, int ch) {
  return (b * ntiles + tau) * ch + c;
}
// KiB stride between consecutive blocks of one tile
__host__ __device__ constexpr int64_t block_stride_kib(int ntiles, int ch) {
  return (int64_t)ntiles * ch;
}

// fragment-native store of one finished tile (mlp_tables.h, "Training stores"): CH
// lane-linear 16-byte stores per lane, each wave-instruction writes 1 KiB contiguous
//
// The training stores (activations, dZ, masks: written once, read once by a later kernel,
// gigabytes per launch) are nontemporal.  Measured per launch at 524,288 samples
// (tools/mlp_bench.py --libs, interleaved): nt takes the training forward 5.22 -> 4.94 ms
// (fp32), 0.737 -> 0.667 (bf16), 2.38 -> 2.02 (bf16x3) and dX 4.49 -> 4.35 / 0.692 -> 0.626 /
// 1.92 -> 1.78 against plain stores; sc1 gained as much on fp32 and less on bf16.
template <int OFF>
__device__ __forceinline__ void store16(uint4* p, uint4 v) {
  if constexpr (NERF_DIAG_NO_STORE) return;
  const u32x4 w = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(w, (u32x4*)p + OFF / 16);
}
// SCH: chunks stored per tile (P::CH; 2 for a bf16x3 tile stored as its bf16 hi half, the
// bf16 tile-block layout)
template <class P, int SCH = P::CH>
__device__ __forceinline__ void store_tile(void* base, int64_t nblk, int ntiles, int tau, int64_t wblock, int lane,
                                           const typename P::Tile& t) {
  uint4* dst = (uint4*)base + tile_kib(nblk, ntiles, tau, wblock, 0, SCH) * 64 + lane;
  sfor<SCH>([&](auto cc) {
    constexpr int c = decltype(cc)::value;
    store16<c * 1024>(dst, P::chunk(t, c));
  });
}


// ReLU masks of the training forward, read by the dX chain: per 32-sample wave block,
// MASK_GROUPS x 64 lanes x 16 B; group l < 8 = layer l's 8 output tiles (tile n -> dword
// n >> 1, bit 8 (n & 1) + mask_bit(rho)), group 8 = the view layer's 4 tiles.  One 16-byte
// store per lane per layer.
__device__ __forceinline__ uint4* mask_slot(void* masks, int64_t wblock, int grp, int lane) {
  return (uint4*)masks + (wblock * MASK_GROUPS + grp) * 64 + lane;
}

// The bf16x3 forwards and the wide fp32 one hold their position-encoding tiles X from L0 to the
// skip input of L5 instead of recomputing them there (bf16x3: its f64-reduced polynomial sin/cos):
// bit-identical, inference forward 1.526 -> 1.498 ms, bf16x3f training forward 1.688 -> 1.668,
// bf16x3 1.872 -> 1.845 at 524,288 samples (r4).  fp32 / bf16 recompute (their register budgets)
template <class P> __host__ __device__ constexpr bool keep_pe() {
  return P::KIND == K_BF16X3 || P::KIND == K_BF16X3W || P::KIND == K_F32W;
}

}  // namespace mlp
}  // namespace nerf
