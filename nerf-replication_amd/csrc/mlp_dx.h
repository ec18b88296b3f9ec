// Fused NeRF MLP: the dX chain (DxWave, DxWave16).
#pragma once
#include "mlp_fwd.h"

namespace nerf {
namespace mlp {

// ------------------------------------------------------------------------------------
// backward dX chain: W^T products + ReLU masks, 32 samples per wave, storing every
// layer's output gradient (pre-activation dZ) fragment-native for the dW GEMMs.
// Stages (mlp_tables.h BStage): bRGB -> dZv, bV -> dfeature, bFA -> dZ7, b7..b1 -> dZ6..dZ0.
// ------------------------------------------------------------------------------------
// (dz tile, mask group or -1) of output tile j of dX stage s
__host__ __device__ constexpr int bwd_dz_tile(int s, int j) {
  return s == B_RGB ? ZT_V + j : s == B_V ? ZT_F + j : s == B_FA ? ZT_H + 56 + j : ZT_H + 8 * (bwd_fwd_layer(s) - 1) + j;
}
__host__ __device__ constexpr int bwd_mask_group(int s) {
  return s == B_RGB ? 8 : s == B_V ? -1 : s == B_FA ? 7 : bwd_fwd_layer(s) - 1;
}

struct DxArgs {
  const char* wpack_t;  // W^T chunks
  const float* d_raw;   // [M,4]
  int64_t M, nblk;
  const void* masks;    // [nblk][MASK_GROUPS][64] x 16 B
  void* dz;             // [ZT_TILES][nblk] tile-blocks
};

template <class P>
struct DxWave {
  using Tile = typename P::Tile;
  static constexpr int CH = P::CH;
  using GT = GroupTable<1, false, P::CH>;
  static_assert(finish_schedule_violation<P, 1, false>() == 0,
                "finish placement (NERF_FINISH_PARTS_* / NERF_FINISH_DELAY) reads a tile pair before its finish part "
                "writes it, or reads a reassigned pend (FinishSchedule)");

  const DxArgs& a;
  uint32_t lds_base;
  int lane, wave, h;
  int64_t wblock, m;
  Tile G, DA, Ha[8], Hb[8];
  uint4 mk[MASK_GROUPS];
  f32x16 pend;      // finished accumulator awaiting its deferred finish (group_body)
  DmaLean dl;

  __device__ __forceinline__ DxWave(const DxArgs& args, const uint4* smem) : a(args) {
    lds_base = (uint32_t)(uintptr_t)(lds_void*)smem;
    lane = threadIdx.x & 63;
    wave = threadIdx.x >> 6;
    h = lane >> 5;
    wblock = (int64_t)blockIdx.x * P::WAVES + wave;
    m = wblock * 32 + (lane & 31);
    dl = DmaLean{a.wpack_t, (uint32_t)(lane * 16 + wave * 1024),
                 (uint32_t)__builtin_amdgcn_readfirstlane(lds_base + (uint32_t)wave * 1024u),
                 (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)wave)};
  }

  template <int g> __device__ __forceinline__ void fetch() {
    constexpr Group Gr = GT::t.g[g];
    fetch_group_lean<P, Gr.c0, Gr.nch, (g % NSLOT) * SLOT_CAP * 1024>(dl);
  }
  template <int g, int i> __device__ __forceinline__ void fetch_piece() {
    constexpr Group Gr = GT::t.g[g];
    fetch_piece_lean<P, Gr.c0, Gr.nch, (g % NSLOT) * SLOT_CAP * 1024, i>(dl);
  }
  static __host__ __device__ constexpr int unit_stores(int) { return CH; }

  // register tile slot S (TileSlot: Ha/Hb ping-pong, seeds G / DA); stage s reads
  // slot<bwd_in_slot(s, t)>, its finish writes slot<bwd_out_slot(s, j)>
  template <int S> __device__ __forceinline__ Tile& slot() {
    if constexpr (S >= TS_HA && S < TS_HB) return Ha[S - TS_HA];
    else if constexpr (S >= TS_HB && S < TS_X) return Hb[S - TS_HB];
    else if constexpr (S == TS_G) return G;
    else {
      static_assert(S == TS_DA, "dX tile slot");
      return DA;
    }
  }
  template <int s, int t> __device__ __forceinline__ const Tile& in_tile_S() { return slot<bwd_in_slot(s, t)>(); }
  static __host__ __device__ constexpr int dz_tile(int s, int j) { return bwd_dz_tile(s, j); }
  static __host__ __device__ constexpr int mask_group(int s) { return bwd_mask_group(s); }
  static __host__ __device__ constexpr int group_stores(int g) {
    int s = 0;
    for (int u = 0; u < NUNIT_BWD; ++u)
      if (finished_in_group<1, false, P::CH, cross_finish<P, 1>()>(g, u)) s += CH;
    return s;
  }

  // ---- group_body hooks
  template <int u, int t> __device__ __forceinline__ const Tile& in_tile() {
    return in_tile_S<bwd_unit_stage(u), t>();
  }
  template <int u> __device__ __forceinline__ void prefetch() {}
  template <int u> __device__ __forceinline__ void init(f32x16& acc) {
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  }
  // part p of NP of unit u's finish: register pairs [8p/NP, 8(p+1)/NP) masked by the forward's
  // ReLU bits into the output-gradient tile (in place); the last part stores the tile
  template <int u, int p> __device__ __forceinline__ void finish_part(const f32x16& acc) {
    constexpr int s = bwd_unit_stage(u), j = u - bwd_unit_first(s);
    constexpr int mg = mask_group(s);
    constexpr int NP = finish_parts<P>();
    constexpr int K0 = 8 * p / NP, K1 = 8 * (p + 1) / NP;
    uint32_t w = 0xFFFFFFFFu;  // this tile's bits at mask_bit(rho) (bf16: + 8 for an odd tile)
    if constexpr (mg >= 0) {
      w = (j >> 1) == 0 ? mk[mg].x : (j >> 1) == 1 ? mk[mg].y : (j >> 1) == 2 ? mk[mg].z : mk[mg].w;
      if constexpr (P::KIND != K_BF16) w >>= 8 * (j & 1);
    }
    // bf16: bits b, 16 + b of pair k (b = k + 8 (j & 1)) -> 0xFFFF / 0 halves: each 16-bit half shifted
    // so its bit lands on bit 15, then arithmetic-shifted back (v_pk_lshlrev_b16 + v_pk_ashrrev_i16;
    // was shift, and, v_mul_u32_u24: 2,614 VALU instead of 3,158 in the dX, 0.591 -> 0.587 ms, r5)
    auto half_mask = [&](auto kk) {
      constexpr unsigned short SH = 15 - decltype(kk)::value - 8 * (j & 1);
      const u16x2 t = __builtin_bit_cast(u16x2, w) << (u16x2){SH, SH};
      return __builtin_bit_cast(uint32_t, __builtin_bit_cast(i16x2, t) >> (i16x2){15, 15});
    };
    Tile& out = slot<bwd_out_slot(s, j)>();
    sfor<K1 - K0>([&](auto kk) {
      constexpr int k = K0 + decltype(kk)::value;
      if constexpr (P::KIND == K_BF16) {
        uint32_t d = pack_bf16(acc[2 * k], acc[2 * k + 1]);
        if constexpr (mg >= 0) d &= half_mask(std::integral_constant<int, k>{});
        P::set_dword(out, k, d);
      } else {  // (bf16x3: the same half masks on the split hi / lo pairs measured 1.3 % slower, r5)
        const float y0 = ((w >> mask_bit(2 * k)) & 1u) ? acc[2 * k] : 0.f;
        const float y1 = ((w >> mask_bit(2 * k + 1)) & 1u) ? acc[2 * k + 1] : 0.f;
        P::set_pair(out, k, y0, y1);
      }
    });
    if constexpr (p == NP - 1) store_tile<P>(a.dz, a.nblk, ZT_TILES, dz_tile(s, j), wblock, lane, out);
  }

  template <int g> __device__ __forceinline__ void step() {
    constexpr int NG = GT::t.n;
    if constexpr (g + PF < NG && dma_spread<P>() == 0) fetch<g + PF>();
    const uint32_t slot = lds_base + (uint32_t)((g % NSLOT) * SLOT_CAP * 1024);
    group_body<P, 1, false, g>(*this, lds_ptr(slot + (uint32_t)(lane * 16)));
    constexpr int N = dma_spread<P>() > 0
        ? handoff_vmcnt_spread<P, 1, false>(g, [](int u) constexpr { return unit_stores(u); })
        : handoff_vmcnt<P, 1, false>(g, [](int i) constexpr { return group_stores(i); }, 2 * CH);
    if constexpr (g + 1 < NG) wait_barrier<N>();
  }

  __device__ __forceinline__ void run() {
    // output gradients of rgb_linear (rows 0..2) and alpha_linear (row 0): lanes 0..31
    const float4 gr = m < a.M ? *(const float4*)(a.d_raw + m * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < MASK_GROUPS; ++i) mk[i] = *mask_slot((void*)a.masks, wblock, i, lane);
    sfor<(PF < GT::t.n ? PF : GT::t.n)>([&](auto gg) { fetch<decltype(gg)::value>(); });
#pragma unroll
    for (int rho = 0; rho < 16; ++rho) {
      P::set(G, rho, (h == 0 && rho < 3) ? (rho == 0 ? gr.x : rho == 1 ? gr.y : gr.z) : 0.f);
      P::set(DA, rho, (h == 0 && rho == 0) ? gr.w : 0.f);
    }
    store_tile<P>(a.dz, a.nblk, ZT_TILES, ZT_RGB, wblock, lane, G);
    store_tile<P>(a.dz, a.nblk, ZT_TILES, ZT_A, wblock, lane, DA);
    {
      constexpr int N0 = [] {
        int n = 2 * CH;
        for (int j = 1; j < PF && j < GT::t.n; ++j) n += group_dma<P, 1, false>(j);
        return n;
      }();
      wait_barrier<N0>();
    }
#pragma unroll
    for (int i = 0; i < MASK_GROUPS; ++i) {
      settle(mk[i].x);
      settle(mk[i].y);
      settle(mk[i].z);
      settle(mk[i].w);
    }
    sfor<GT::t.n>([&](auto gg) { step<decltype(gg)::value>(); });
  }
};

// ------------------------------------------------------------------------------------
// The wide dX (round 6, PF32W / PBF3W): DxWave's W^T chain over 16-row units (DIR 3) on the 16x16 MFMAs, 16
// samples per wave, 8 waves per workgroup, two per SIMD.  The same register trick as FwdWave16 (a 16-row output
// tile IS half of the next stage's K-block), the forward's ReLU masks read from the old-layout lane of this
// lane's sample and half (lold), and the dZ stores in the old tile-block layout (the dW is unchanged): lane
// (s, g)'s four values of output tile m are old lane lold's registers 4 (2 (m & 1) + (g >> 1)) + e.
// ------------------------------------------------------------------------------------
template <class P>
struct DxWave16 {
  using Tile = typename P::Tile;
  using Acc = f32x4;
  static constexpr bool F32 = P::KIND == K_F32W, B16 = P::KIND == K_BF16W;
  static_assert(wide_kind<P>(), "DxWave16: PF32W, PBF3W or PBF16W");
  static constexpr int CH = P::CH;
  static constexpr int SCH = B16 ? 2 : 4;   // chunks of a stored dZ tile-block (fp32, bf16x3 hi + lo, bf16)
  static constexpr int SST = B16 || F32 ? 1 : 2;  // stores per output tile: 16-byte (fp32), hi [+ lo] 8-byte
  using GT = GroupTable<3, false, P::CH>;
  static_assert(finish_schedule_violation<P, 3, false>() == 0,
                "finish placement (NERF_FINISH_PARTS_* / NERF_FINISH_DELAY) reads a tile pair before its finish part "
                "writes it, or reads a reassigned pend (FinishSchedule)");

  const DxArgs& a;
  uint32_t lds_base;
  int lane, wave, s, g;
  int64_t m, wb32;
  uint32_t st_off, lold, gsh;
  Tile G, DA, Ha[8], Hb[8];
  uint4 mk[MASK_GROUPS];
  Acc pend;
  DmaLean dl;

  __device__ __forceinline__ DxWave16(const DxArgs& args, const uint4* smem) : a(args) {
    lds_base = (uint32_t)(uintptr_t)(lds_void*)smem;
    lane = threadIdx.x & 63;
    wave = threadIdx.x >> 6;
    s = lane & 15;
    g = lane >> 4;
    m = ((int64_t)blockIdx.x * P::WAVES + wave) * 16 + s;
    wb32 = (int64_t)blockIdx.x * (P::WAVES / 2) + (wave >> 1);
    lold = 16u * (uint32_t)(wave & 1) + (uint32_t)s + 32u * (uint32_t)(g & 1);
    st_off = 16u * lold + (F32 ? 1024u : 8u) * (uint32_t)(g >> 1);
    gsh = 2u * (uint32_t)(g >> 1);
    dl = DmaLean{a.wpack_t, (uint32_t)(lane * 16 + wave * 1024),
                 (uint32_t)__builtin_amdgcn_readfirstlane(lds_base + (uint32_t)wave * 1024u),
                 (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)wave)};
  }

  template <int gi> __device__ __forceinline__ void fetch() {
    constexpr Group Gr = GT::t.g[gi];
    fetch_group_lean<P, Gr.c0, Gr.nch, (gi % NSLOT) * SLOT_CAP * 1024>(dl);
  }
  template <int gi, int i> __device__ __forceinline__ void fetch_piece() {
    constexpr Group Gr = GT::t.g[gi];
    fetch_piece_lean<P, Gr.c0, Gr.nch, (gi % NSLOT) * SLOT_CAP * 1024, i>(dl);
  }
  static __host__ __device__ constexpr int unit_stores(int) { return SST; }
  static __host__ __device__ constexpr int group_stores(int gi) {
    int n = 0;
    for (int u = 0; u < NUNIT_BWD16; ++u)
      if (finished_in_group<3, false, P::CH, cross_finish<P, 3>()>(gi, u)) n += SST;
    return n;
  }
  template <int S> __device__ __forceinline__ Tile& slot() {
    if constexpr (S >= TS_HA && S < TS_HB) return Ha[S - TS_HA];
    else if constexpr (S >= TS_HB && S < TS_X) return Hb[S - TS_HB];
    else if constexpr (S == TS_G) return G;
    else {
      static_assert(S == TS_DA, "dX tile slot");
      return DA;
    }
  }
  static __host__ __device__ constexpr int stage_of(int u) { return bwd16_unit_stage(u); }

  // half hf of the 32-feature dZ tile tau (old layout): fp32 values v[4 hf .. 4 hf + 3], or the bf16x3 hi / lo dwords
  // 2 hf, 2 hf + 1 (8 bytes each, lo 2 KiB after hi)
  __device__ __forceinline__ void store_half(int tau, int hf, const Tile& t) {
    if constexpr (F32) {
      char* base = (char*)a.dz + (((wb32 * ZT_TILES + tau) * SCH + 2 * hf) << 10) + st_off;
      store16<0>((uint4*)base, make_uint4(__float_as_uint(t.v[4 * hf]), __float_as_uint(t.v[4 * hf + 1]),
                                          __float_as_uint(t.v[4 * hf + 2]), __float_as_uint(t.v[4 * hf + 3])));
    } else {
      char* base = (char*)a.dz + (((wb32 * ZT_TILES + tau) * SCH + hf) << 10) + st_off;
      store8(base, get_dword(t.hi, 2 * hf), get_dword(t.hi, 2 * hf + 1));
      if constexpr (!B16) store8(base + 2048, get_dword(t.lo, 2 * hf), get_dword(t.lo, 2 * hf + 1));
    }
  }

  // ---- group_body hooks
  template <int u, int t> __device__ __forceinline__ const Tile& in_tile() {
    return slot<bwd_in_slot(stage_of(u), t)>();
  }
  template <int u> __device__ __forceinline__ void prefetch() {}
  template <int u> __device__ __forceinline__ void init(Acc& acc) {
    acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
  }
  // part p of NP of unit u (half m & 1 of output tile j = m >> 1 of stage st): its register pairs masked by the
  // forward's ReLU bits into the output-gradient K-block (in place); the last part stores
  template <int u, int p> __device__ __forceinline__ void finish_part(const Acc& acc) {
    constexpr int st = stage_of(u), mu = u - bwd16_unit_first(st), j = mu >> 1, hf = mu & 1;
    constexpr int mg = bwd_mask_group(st);
    constexpr int NP = finish_parts<P>();
    constexpr int K0 = 2 * p / NP, K1 = 2 * (p + 1) / NP;
    uint32_t w = 0xFFFFFFFFu;
    if constexpr (mg >= 0) {
      // value e (pair k = e >> 1, element e & 1) of this lane: old register rho = 4 (2 hf + (g >> 1)) + e of old
      // tile j, mask bit 8 (j & 1) + (rho >> 1) + 16 (rho & 1) = [k + 16 (e & 1)] << (8 (j & 1) + 4 hf + gsh)
      const uint32_t d = (j >> 1) == 0 ? mk[mg].x : (j >> 1) == 1 ? mk[mg].y : (j >> 1) == 2 ? mk[mg].z : mk[mg].w;
      w = d >> ((uint32_t)(8 * (j & 1) + 4 * hf) + gsh);
    }
    Tile& out = slot<bwd_out_slot(st, j)>();
    sfor<K1 - K0>([&](auto kk) {
      constexpr int k = K0 + decltype(kk)::value;
      const float y0 = ((w >> k) & 1u) ? acc[2 * k] : 0.f;
      const float y1 = ((w >> (16 + k)) & 1u) ? acc[2 * k + 1] : 0.f;
      if constexpr (F32) {
        out.v[4 * hf + 2 * k] = y0;
        out.v[4 * hf + 2 * k + 1] = y1;
      } else if constexpr (B16) {
        set_dword8(out.hi, 2 * hf + k, pack_bf16(y0, y1));
      } else {
        const uint32_t hw = pack_bf16(y0, y1);
        const uint32_t lw = pack_bf16(y0 - __uint_as_float(hw << 16), y1 - __uint_as_float(hw & 0xffff0000u));
        set_dword8(out.hi, 2 * hf + k, hw);
        set_dword8(out.lo, 2 * hf + k, lw);
      }
    });
    if constexpr (p == NP - 1) store_half(bwd_dz_tile(st, j), hf, out);
  }

  template <int gi> __device__ __forceinline__ void step() {
    constexpr int NG = GT::t.n;
    if constexpr (gi + PF < NG && dma_spread<P>() == 0) fetch<gi + PF>();
    const uint32_t sl = lds_base + (uint32_t)((gi % NSLOT) * SLOT_CAP * 1024);
    group_body<P, 3, false, gi>(*this, lds_ptr(sl + (uint32_t)(lane * 16)));
    constexpr int N = dma_spread<P>() > 0
        ? handoff_vmcnt_spread<P, 3, false>(gi, [](int u) constexpr { return unit_stores(u); })
        : handoff_vmcnt<P, 3, false>(gi, [](int i) constexpr { return group_stores(i); }, 4 * SST);
    if constexpr (gi + 1 < NG) wait_barrier<N>();
  }

  // the seed tiles: K-block 0 of d rgb (features 0..2) and of d alpha (feature 0), element e of lane group g =
  // feature k16_feat(g, e): lane group 0's elements 0..2 / 0
  __device__ __forceinline__ void seed(Tile& t, float v0, float v1, float v2) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = 0.f;
    if (g == 0) v[0] = v0, v[1] = v1, v[2] = v2;
    if constexpr (F32) {
#pragma unroll
      for (int e = 0; e < 8; ++e) t.v[e] = v[e];
    } else {
      uint32_t hw[4], lw[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        hw[k] = pack_bf16(v[2 * k], v[2 * k + 1]);
        lw[k] = pack_bf16(v[2 * k] - __uint_as_float(hw[k] << 16), v[2 * k + 1] - __uint_as_float(hw[k] & 0xffff0000u));
      }
      t.hi = __builtin_bit_cast(bf16x8, make_uint4(hw[0], hw[1], hw[2], hw[3]));
      if constexpr (!B16) t.lo = __builtin_bit_cast(bf16x8, make_uint4(lw[0], lw[1], lw[2], lw[3]));
    }
  }

  __device__ __forceinline__ void run() {
    const float4 gr = m < a.M ? *(const float4*)(a.d_raw + m * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < MASK_GROUPS; ++i) mk[i] = *mask_slot((void*)a.masks, wb32, i, (int)lold);
    sfor<(PF < GT::t.n ? PF : GT::t.n)>([&](auto gg) { fetch<decltype(gg)::value>(); });
    seed(G, gr.x, gr.y, gr.z);
    seed(DA, gr.w, 0.f, 0.f);
    store_half(ZT_RGB, 0, G);
    store_half(ZT_RGB, 1, G);
    store_half(ZT_A, 0, DA);
    store_half(ZT_A, 1, DA);
    {
      constexpr int N0 = [] {
        int n = 4 * SST;
        for (int j = 1; j < PF && j < GT::t.n; ++j) n += group_dma<P, 3, false>(j);
        return n;
      }();
      wait_barrier<N0>();
    }
#pragma unroll
    for (int i = 0; i < MASK_GROUPS; ++i) {
      settle(mk[i].x);
      settle(mk[i].y);
      settle(mk[i].z);
      settle(mk[i].w);
    }
    sfor<GT::t.n>([&](auto gg) { step<decltype(gg)::value>(); });
  }
};

template <class P>
using DxWaveOf = std::conditional_t<wide_kind<P>(), DxWave16<P>, DxWave<P>>;

template <class P>
__global__ void __launch_bounds__(P::WAVES * 64) dx_kernel(DxArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 smem_u4[];
  DxWaveOf<P> w(a, smem_u4);
  w.run();
}

}  // namespace mlp
}  // namespace nerf
