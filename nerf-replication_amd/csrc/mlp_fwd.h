// Fused NeRF MLP: the forward kernels (FwdWave: 32 samples per wave; FwdWave16: the wide 16-sample waves).
#pragma once
#include "mlp_dma.h"
#include "mlp_pe_store.h"

namespace nerf {
namespace mlp {

// ------------------------------------------------------------------------------------
// forward: one wave = 32 samples through all 11 layers; activations stay in registers
// (feature-major accumulator layout = the next layer's B operand).
// ------------------------------------------------------------------------------------
struct FwdArgs {
  const char* wpack;
  const float* pts;          // [M,3]
  const float* dirs;         // [ndir,3] unit view directions
  const int32_t* dir_index;  // [M] or null (then dir = m / samples_per_dir)
  int samples_per_dir;
  int64_t M;
  int64_t nblk;              // 32-sample blocks of the stores (M padded to M_ALIGN) / 32
  float* raw;                // [M,4]
  void* act;                 // [AT_TILES][nblk] tile-blocks or null
  void* masks;               // [nblk][MASK_GROUPS][64] x 16 B or null
  const int32_t* M_dev;      // persistent inference launch: M = min(*M_dev, M_cap), read on the device
  int64_t M_cap;
};

// HALF (bf16x3 only): the training stores keep each tile's bf16 hi half in the bf16 layout
// (2 chunks per tile-block) for a bf16 backward -- the "bf16x3f" tier: bf16x3 outputs, bf16
// gradients.  hi = RNE bf16 of the fp32-class value, exactly what a bf16 forward stores.
template <class P, bool STORE, bool DENSITY, bool PERSIST = false, bool HALF = false>
struct FwdWave {
  using Tile = typename P::Tile;
  static constexpr int CH = P::CH;
  static_assert(!HALF || (P::KIND == K_BF16X3 && STORE), "half stores: bf16x3 training forward only");
  static_assert(finish_schedule_violation<P, 0, DENSITY>() == 0,
                "finish placement (NERF_FINISH_PARTS_* / NERF_FINISH_DELAY) reads a tile pair before its finish part "
                "writes it, or reads a reassigned pend (FinishSchedule)");
  static constexpr int SCH = HALF ? 2 : P::CH;  // chunks stored per tile
  using GT = GroupTable<0, DENSITY, P::CH>;

  const FwdArgs& a;
  uint32_t lds_base;
  int lane, wave, h;
  int64_t wblock, m;
  float px, py, pz, dx, dy, dz;
  Tile X[2], D, Ha[8], Hb[8];
  uint32_t mw[4];
  uint32_t one16;   // 0x00010001 in an SGPR, opaque to hipcc (nonzero_bf16x2)
  float alpha, rgb0, rgb1, rgb2;
  lds_cu4* wb;      // current group's slot + 16 h (bias reads)
  uint4 bias[4];
  f32x16 pend;      // finished accumulator awaiting its deferred finish (group_body)
  DmaLean dl;

  __device__ __forceinline__ FwdWave(const FwdArgs& args, const uint4* smem, int64_t blk, int tid) : a(args) {
    lds_base = (uint32_t)(uintptr_t)(lds_void*)smem;
    lane = tid & 63;
    wave = tid >> 6;
    h = lane >> 5;
    wblock = blk * P::WAVES + wave;
    m = wblock * 32 + (lane & 31);
    one16 = opaque_one16();
    dl = DmaLean{a.wpack, (uint32_t)(lane * 16 + wave * 1024),
                 (uint32_t)__builtin_amdgcn_readfirstlane(lds_base + (uint32_t)wave * 1024u),
                 (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)wave)};
  }

  template <int g> __device__ __forceinline__ void fetch() {
    constexpr Group G = GT::t.g[g];
    fetch_group_lean<P, G.c0, G.nch, (g % NSLOT) * SLOT_CAP * 1024>(dl);
  }
  template <int g, int i> __device__ __forceinline__ void fetch_piece() {
    constexpr Group G = GT::t.g[g];
    fetch_piece_lean<P, G.c0, G.nch, (g % NSLOT) * SLOT_CAP * 1024, i>(dl);
  }

  // register tile slot S (TileSlot: Ha/Hb ping-pong, PE tiles X / D); layer L reads
  // slot<fwd_in_slot(L, t)>, its finish writes slot<fwd_out_slot(L, n)>
  template <int S> __device__ __forceinline__ Tile& slot() {
    if constexpr (S >= TS_HA && S < TS_HB) return Ha[S - TS_HA];
    else if constexpr (S >= TS_HB && S < TS_X) return Hb[S - TS_HB];
    else if constexpr (S == TS_X || S == TS_X + 1) return X[S - TS_X];
    else {
      static_assert(S == TS_D, "forward tile slot");
      return D;
    }
  }
  template <int L, int t> __device__ __forceinline__ const Tile& in_tile_L() {
    return slot<fwd_in_slot(L, t)>();
  }

  // vector-memory stores issued by unit u's finish
  static __host__ __device__ constexpr int unit_stores(int u) {
    if (!STORE) return 0;
    const int L = fwd_unit_layer(u), n = u - fwd_unit_first(L);
    if (L == LFA) return n < 8 ? SCH : 0;
    if (L == LRGB) return 0;
    return SCH + (n == fwd_out_tiles(L) - 1 ? 1 : 0);  // + the layer's mask store
  }
  static __host__ __device__ constexpr int group_stores(int g) {
    int s = 0;
    for (int u = 0; u < NUNIT_FWD; ++u)
      if (finished_in_group<0, DENSITY, P::CH, cross_finish<P, 0>()>(g, u)) s += unit_stores(u);
    return s;
  }

  // part p of NP of unit (L, n)'s finish: register pairs [8p/NP, 8(p+1)/NP) into the output
  // tile (in place), their mask bits; the last part stores the tile (and the layer's masks)
  template <int L, int n, int p> __device__ __forceinline__ void finish_L_part(const f32x16& acc) {
    constexpr int NP = finish_parts<P>();
    constexpr int K0 = 8 * p / NP, K1 = 8 * (p + 1) / NP;
    constexpr bool LASTP = p == NP - 1;
    if constexpr (L <= L7 || L == LV) {
      Tile& out = slot<fwd_out_slot(L, n)>();
      uint32_t bits = 0;  // this tile's mask bits (mask_bit layout)
      sfor<K1 - K0>([&](auto kk) {
        constexpr int k = K0 + decltype(kk)::value;
        const float a0 = acc[2 * k], a1 = acc[2 * k + 1];
        if constexpr (P::KIND == K_BF16) {
          // bf16: pack the pair first, then ReLU on the packed pair (one VALU for both); the mask
          // bits k / 16 + k from the packed result (v_pk_min_u16 + v_lshl_or_b32 per pair, as the bf16x3 path,
          // instead of per-value compares and selects)
          const uint32_t d = relu_bf16x2(pack_bf16(a0, a1));
          if constexpr (STORE) bits |= nonzero_bf16x2(d, one16) << k;
          P::set_dword(out, k, d);
        } else {
          // ReLU as an integer max on the float bits (negative floats are negative ints)
          const int y0 = max(__float_as_int(a0), 0), y1 = max(__float_as_int(a1), 0);
          if constexpr (STORE && P::KIND == K_BF16X3) {
            // bit k / 16 + k = the pair's hi halves non-zero: the same bits as y > 0, since RNE keeps
            // every positive fp32 above 2^-134 non-zero in bf16 (pre-activations that small do not occur)
            bits |= nonzero_bf16x2(pack_bf16(__int_as_float(y0), __int_as_float(y1)), one16) << k;
          } else if constexpr (STORE) {
            bits |= min((uint32_t)y0, 1u) << mask_bit(2 * k);
            bits |= min((uint32_t)y1, 1u) << mask_bit(2 * k + 1);
          }
          P::set_pair(out, k, __int_as_float(y0), __int_as_float(y1));
        }
      });
      if constexpr (STORE) {
        if constexpr (K0 == 0 && (n & 1) == 0) mw[n >> 1] = bits;
        else mw[n >> 1] |= bits << (8 * (n & 1));
        if constexpr (LASTP) {
          store_tile<P, SCH>(a.act, a.nblk, AT_TILES, (L == LV ? AT_V : AT_H + 8 * L) + n, wblock, lane, out);
          if constexpr (n == fwd_out_tiles(L) - 1)
            store16<0>(mask_slot(a.masks, wblock, L == LV ? 8 : L, lane),
                       make_uint4(mw[0], mw[1], L == LV ? 0u : mw[2], L == LV ? 0u : mw[3]));
        }
      }
    } else if constexpr (L == LFA) {
      if constexpr (n < 8) {  // feature_linear: no activation
        Tile& out = slot<fwd_out_slot(L, n)>();
        sfor<K1 - K0>([&](auto kk) {
          constexpr int k = K0 + decltype(kk)::value;
          P::set_pair(out, k, acc[2 * k], acc[2 * k + 1]);
        });
        if constexpr (STORE && LASTP) store_tile<P, SCH>(a.act, a.nblk, AT_TILES, AT_F + n, wblock, lane, out);
      } else if constexpr (p == 0) {
        alpha = acc[0];  // alpha_linear: output row 0 = register 0 of lanes 0..31
      }
    } else if constexpr (p == 0) {  // LRGB: rows 0..2 = registers 0..2 of lanes 0..31
      rgb0 = acc[0];
      rgb1 = acc[1];
      rgb2 = acc[2];
    }
  }

  // ---- group_body hooks
  template <int u> static __host__ __device__ constexpr int group_of() {
    int g = 0;
    while (!(GT::t.g[g].u0 <= u && u < GT::t.g[g].u0 + GT::t.g[g].n)) ++g;
    return g;
  }
  template <int u, int t> __device__ __forceinline__ const Tile& in_tile() {
    return in_tile_L<fwd_unit_layer(u), t>();
  }
  // the unit's bias chunk (rows 8q + 4h + {0..3} = lane 2q + h) is the MFMA chain's
  // initial accumulator; it is read one unit ahead
  template <int u> __device__ __forceinline__ void prefetch() {
    constexpr int L = fwd_unit_layer(u);
    constexpr int BOFF = unit_chunk_off<0>(u, CH) - GT::t.g[group_of<u>()].c0 + fwd_in_tiles(L) * CH;
#pragma unroll
    for (int q = 0; q < 4; ++q) bias[q] = as_uint4(wb[BOFF * 64 + 2 * q]);
  }
  template <int u> __device__ __forceinline__ void init(f32x16& acc) {
    constexpr int L = fwd_unit_layer(u), n = u - fwd_unit_first(L);
    if constexpr (L == L5 && n == 0 && !keep_pe<P>()) {  // PE recomputed for the skip instead of held through L1..L4
      settle(px);  // opaque to hipcc: it would otherwise CSE this with the L0 tiles and hold them
      settle(py);
      settle(pz);
      pe_tile<P, 0, 10, 63>(X[0], h, px, py, pz);
      pe_tile<P, 1, 10, 63>(X[1], h, px, py, pz);
    }
    if constexpr (L == LV && n == 0) {
      settle(dx);
      settle(dy);
      settle(dz);
      pe_tile<P, 0, 4, 27>(D, h, dx, dy, dz);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      acc[4 * q + 0] = __uint_as_float(bias[q].x);
      acc[4 * q + 1] = __uint_as_float(bias[q].y);
      acc[4 * q + 2] = __uint_as_float(bias[q].z);
      acc[4 * q + 3] = __uint_as_float(bias[q].w);
    }
  }
  template <int u, int p> __device__ __forceinline__ void finish_part(const f32x16& acc) {
    constexpr int L = fwd_unit_layer(u), n = u - fwd_unit_first(L);
    finish_L_part<L, n, p>(acc);
  }

  template <int g> __device__ __forceinline__ void step() {
    constexpr int NG = GT::t.n;
    if constexpr (g + PF < NG && dma_spread<P>() == 0) fetch<g + PF>();
    const uint32_t slot = lds_base + (uint32_t)((g % NSLOT) * SLOT_CAP * 1024);
    wb = lds_ptr(slot + (uint32_t)(h * 16));
    group_body<P, 0, DENSITY, g>(*this, lds_ptr(slot + (uint32_t)(lane * 16)));
    constexpr int N = dma_spread<P>() > 0
        ? handoff_vmcnt_spread<P, 0, DENSITY>(g, [](int u) constexpr { return unit_stores(u); })
        : handoff_vmcnt<P, 0, DENSITY>(g, [](int i) constexpr { return group_stores(i); }, STORE ? 3 * SCH : 0);
    if constexpr (g + 1 < NG) wait_barrier<N>();
  }

  __device__ __forceinline__ void run() {
#if NERF_DIAG_STAMPS
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
#endif
    const int64_t ms = m < a.M ? m : a.M - 1;
    px = a.pts[ms * 3 + 0];
    py = a.pts[ms * 3 + 1];
    pz = a.pts[ms * 3 + 2];
    dx = dy = dz = 0.f;
    if constexpr (!DENSITY) {
      const int64_t di = a.dir_index ? (int64_t)a.dir_index[ms] : ms / a.samples_per_dir;
      dx = a.dirs[di * 3 + 0];
      dy = a.dirs[di * 3 + 1];
      dz = a.dirs[di * 3 + 2];
    }
    sfor<(PF < GT::t.n ? PF : GT::t.n)>([&](auto gg) { fetch<decltype(gg)::value>(); });
    pe_tile<P, 0, 10, 63>(X[0], h, px, py, pz);
    pe_tile<P, 1, 10, 63>(X[1], h, px, py, pz);
    if constexpr (STORE) {
      Tile Dt;
      pe_tile<P, 0, 4, 27>(Dt, h, dx, dy, dz);
      store_tile<P, SCH>(a.act, a.nblk, AT_TILES, AT_X, wblock, lane, X[0]);
      store_tile<P, SCH>(a.act, a.nblk, AT_TILES, AT_X + 1, wblock, lane, X[1]);
      store_tile<P, SCH>(a.act, a.nblk, AT_TILES, AT_D, wblock, lane, Dt);
    }
    {  // group 0 landed: younger = the DMAs of groups 1 .. PF - 1 and the PE stores
      constexpr int N0 = [] {
        int n = STORE ? 3 * SCH : 0;
        for (int j = 1; j < PF && j < GT::t.n; ++j) n += group_dma<P, 0, DENSITY>(j);
        return n;
      }();
      wait_barrier<N0>();
    }
#if NERF_DIAG_STAMPS
    const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
#endif
    settle(dx);
    settle(dy);
    settle(dz);
    sfor<GT::t.n>([&](auto gg) { step<decltype(gg)::value>(); });
    if (h == 0 && m < a.M)
      *(float4*)(a.raw + m * 4) = DENSITY ? make_float4(0.f, 0.f, 0.f, alpha) : make_float4(rgb0, rgb1, rgb2, alpha);
#if NERF_DIAG_STAMPS
    // (diagnostic only) wave 0 lane 0 of each workgroup overwrites raw rows 0-1 of its block:
    // hw id, xcc id, entry / prologue-done / end (s_memrealtime)
    const uint64_t t2 = __builtin_amdgcn_s_memrealtime();
    if (wave == 0 && lane == 0) {
      uint32_t* d = (uint32_t*)(a.raw + (wblock * 32) * 4);
      d[0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
      d[1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
      d[2] = (uint32_t)t0, d[3] = (uint32_t)(t0 >> 32);
      d[4] = (uint32_t)t1, d[5] = (uint32_t)(t1 >> 32);
      d[6] = (uint32_t)t2, d[7] = (uint32_t)(t2 >> 32);
    }
#endif
  }
};

// ------------------------------------------------------------------------------------
// The wide bf16x3 forward (round 6, PBF3W): one wave = 16 samples on v_mfma_f32_16x16x32_bf16, 8 waves
// per workgroup, two per SIMD.  The bf16x3 forward of the 32x32 kernels above holds 32 samples' hi / lo
// activation tiles per wave in ~370 registers -- one wave per SIMD, so nothing feeds the matrix pipe
// while a wave runs its epilogue (ReLU, hi / lo split, masks, stores) or waits on LDS; with 16 samples
// a wave needs ~200 registers and the two waves of a SIMD overlap each other's epilogues and waits.
// Same weight ring (2 x 72 KiB LDS slots, LDS-DMA one group ahead, counted hand-offs) and group
// pipeline (group_body, finish parts, spread DMA) over 16-row units (DIR 2).
//
// Training stores go to the 32x32 fragment layout the dX / dW kernels read (mlp_tables.h "Training
// stores"): a 32-sample tile-block spans the two waves of a SIMD pair (wave & 1 = its half of the
// samples) and two 16-row output tiles (old chunk c = tile m & 1).  Old lane L = sample (L & 31) + 32 h
// holds features 16 c + 4 h + {0..3} then 16 c + 8 + 4 h + {0..3}: exactly the 4 rows of this kernel's
// lane (s, g = h) and of lane (s, g = h + 2) -- so every lane writes its 8 bytes (4 bf16) with one
// global_store_dwordx2 at 16 L + 8 (g >> 1), no exchange.  The ReLU-mask bits of old lane L come from the
// lanes l and l + 32 of one wave: combined with one v_permlane32_swap per mask dword at the layer's end.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void store8(char* p, uint32_t lo, uint32_t hi) {
  if constexpr (NERF_DIAG_NO_STORE) return;
  typedef unsigned int u32x2v __attribute__((ext_vector_type(2)));
  __builtin_nontemporal_store((u32x2v){lo, hi}, (u32x2v*)p);  // (plain stores measured: 1.536 -> 1.561 ms, r6)
}
__device__ __forceinline__ uint32_t get_dword(const bf16x8& v, int k) {
  const uint4 u = __builtin_bit_cast(uint4, v);
  return k == 0 ? u.x : k == 1 ? u.y : k == 2 ? u.z : u.w;
}
__device__ __forceinline__ void set_dword8(bf16x8& v, int k, uint32_t d) {
  uint4 u = __builtin_bit_cast(uint4, v);
  if (k == 0) u.x = d;
  else if (k == 1) u.y = d;
  else if (k == 2) u.z = d;
  else u.w = d;
  v = __builtin_bit_cast(bf16x8, u);
}
// position encoding of K-block TILE in the wide B-operand layout: element e of lane group g is feature
// 32 TILE + P::fwd_feat(g, e) (PBF3W: k16_feat, PF32W: f32w_feat); the same fp32 values as pe_tile<PBF3>
// (PE_POLY), split hi / lo, or as pe_tile<PF32> (PE_LIBM)
template <class T> __device__ __forceinline__ T sel4(int g, T a0, T a1, T a2, T a3) {
  return (g & 2) ? ((g & 1) ? a3 : a2) : ((g & 1) ? a1 : a0);  // (branch-free selects on the lane group)
}
template <class P, int TILE, int NFREQ, int NVALID>
__device__ __forceinline__ void pe_kblock(typename P::Tile& t, int g, float x0, float x1, float x2) {
  constexpr double INV2PI = 0.15915494309189533576888376337251;
  float v[8];
  sfor<8>([&](auto ee) {
    constexpr int e = decltype(ee)::value;
    constexpr PeFeat F0 = pe_feat(32 * TILE + P::fwd_feat(0, e), NFREQ, NVALID);
    constexpr PeFeat F1 = pe_feat(32 * TILE + P::fwd_feat(1, e), NFREQ, NVALID);
    constexpr PeFeat F2 = pe_feat(32 * TILE + P::fwd_feat(2, e), NFREQ, NVALID);
    constexpr PeFeat F3 = pe_feat(32 * TILE + P::fwd_feat(3, e), NFREQ, NVALID);
    // every candidate is chosen at compile time; only the lane group selects among them
    const float c0 = F0.dim == 0 ? x0 : F0.dim == 1 ? x1 : x2, c1 = F1.dim == 0 ? x0 : F1.dim == 1 ? x1 : x2;
    const float c2 = F2.dim == 0 ? x0 : F2.dim == 1 ? x1 : x2, c3 = F3.dim == 0 ? x0 : F3.dim == 1 ? x1 : x2;
    const float x = sel4(g, c0, c1, c2, c3);
    float trig = 0.f;
    if constexpr (F0.kind == 2 || F1.kind == 2 || F2.kind == 2 || F3.kind == 2) {
      if constexpr (P::PE == PE_LIBM) {  // (PF32W: sincosf of the exact fp32 x * 2^k, as PF32's pe_tile)
        const float srad = sel4(g, (float)(1 << F0.k), (float)(1 << F1.k), (float)(1 << F2.k), (float)(1 << F3.k));
        const bool is_cos = sel4(g, F0.cos != 0, F1.cos != 0, F2.cos != 0, F3.cos != 0);
        trig = pe_trig<PE_LIBM>(x, 0.0, srad, 0.0, is_cos);
      } else {
        const double srev = sel4(g, INV2PI * (double)(1 << F0.k), INV2PI * (double)(1 << F1.k),
                                 INV2PI * (double)(1 << F2.k), INV2PI * (double)(1 << F3.k));
        const double ph = sel4(g, F0.cos ? 0.25 : 0.0, F1.cos ? 0.25 : 0.0, F2.cos ? 0.25 : 0.0, F3.cos ? 0.25 : 0.0);
        trig = pe_trig<PE_POLY>(x, srev, 0.f, ph, false);
      }
    }
    v[e] = sel4(g, F0.kind == 2 ? trig : F0.kind == 1 ? x : 0.f, F1.kind == 2 ? trig : F1.kind == 1 ? x : 0.f,
                F2.kind == 2 ? trig : F2.kind == 1 ? x : 0.f, F3.kind == 2 ? trig : F3.kind == 1 ? x : 0.f);
  });
  if constexpr (P::KIND == K_F32W) {
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
    t.lo = __builtin_bit_cast(bf16x8, make_uint4(lw[0], lw[1], lw[2], lw[3]));
  }
}

template <class P, bool STORE, bool DENSITY, bool PERSIST = false, bool HALF = false>
struct FwdWave16 {
  using Tile = typename P::Tile;
  using Acc = f32x4;
  static constexpr bool F32 = P::KIND == K_F32W;
  static_assert(wide_kind<P>() && (!HALF || (!F32 && STORE)), "FwdWave16: PBF3W (HALF: bf16x3f stores) or PF32W");
  static_assert(!F32 || (STORE && !PERSIST), "PF32W: the training forward only");
  static constexpr int CH = P::CH;
  static constexpr int SCH = HALF ? 2 : 4;  // chunks of a stored tile-block: bf16 hi (bf16x3f), hi + lo, or fp32
  // stores per output tile: PBF3W one 8-byte store per half (hi [+ lo]); PF32W one 16-byte store
  static constexpr int SST = F32 ? 1 : HALF ? 1 : 2;
  // (r6, measured and removed: the two 16-row tiles of one old tile stored together, one 16-byte store per lane
  // with the halves exchanged by v_permlane32_swap -- bit-identical, bf16x3f training forward 1.502 -> 1.573 ms,
  // bf16x3 1.660 -> 1.769; profiles/r6/pair_store_ab.json)
  static constexpr int PRO_ST = NERF_DIAG_NO_ACT ? 0 : 6 * SST;  // the prologue's PE stores (3 K-blocks x 2 halves)
  // the units' layout in the pack and the slots: DIR 2, or (PF32W) DIR 4 -- the same 16-row units over PF32's pack
  static constexpr int DIR = sched_dir<P, 2>();
  static_assert(!F32 || (P::CH == 2 && PF32::CH == 4), "a PF32W step is two of PF32's four chunks");
  using GT = GroupTable<DIR, DENSITY, P::CH>;
  static_assert(finish_schedule_violation<P, 2, DENSITY>() == 0,
                "finish placement (NERF_FINISH_PARTS_* / NERF_FINISH_DELAY) reads a tile pair before its finish part "
                "writes it, or reads a reassigned pend (FinishSchedule)");

  const FwdArgs& a;
  uint32_t lds_base;
  int lane, wave, s, g;
  int64_t m;        // this lane's sample
  int64_t wb32;     // the 32-sample block of the training stores
  uint32_t st_off;  // byte offset of this lane's 8 bytes in a 1-KiB chunk of the stores (PF32W: its 16 bytes,
                    // + 1 KiB (g >> 1): chunk 2 (mt & 1) + (g >> 1) of the fp32 tile-block)
  uint32_t lold;    // old-layout lane of the mask store: sample (16 (wave & 1) + s) + 32 (g & 1)
  uint32_t gsh;     // 2 (g >> 1): offset of this lane's mask bits among an old register pair group (PF32W: 16 (g >> 1))
  uint32_t a_off;   // byte offset of this lane's A operand in a chunk: 16 lane, or (PF32W) its 8 bytes of PF32's slot
                    // (row f32w_row(lane & 15), half g & 1): 16 (32 (g & 1) + row) + 8 (g >> 1)
  float px, py, pz, dx, dy, dz;
  Tile X[2], D, Ha[8], Hb[8];
  uint32_t mw[4];
  uint32_t one16;
  float alpha, rgb0, rgb1, rgb2;
  lds_cu4* wbg;     // current group's slot + 16 g (bias reads; PF32W: + 16 (g & 1) + 4 (g >> 1))
  uint4 bias;
  Acc pend;
  DmaLean dl;

  __device__ __forceinline__ FwdWave16(const FwdArgs& args, const uint4* smem, int64_t blk, int tid) : a(args) {
    lds_base = (uint32_t)(uintptr_t)(lds_void*)smem;
    lane = tid & 63;
    wave = tid >> 6;
    s = lane & 15;
    g = lane >> 4;
    m = (blk * P::WAVES + wave) * 16 + s;
    wb32 = blk * (P::WAVES / 2) + (wave >> 1);
    const uint32_t sb = 16u * (uint32_t)(wave & 1) + (uint32_t)s;
    lold = sb + 32u * (uint32_t)(g & 1);
    st_off = 16u * lold + (F32 ? 1024u : 8u) * (uint32_t)(g >> 1);
    gsh = (F32 ? 16u : 2u) * (uint32_t)(g >> 1);
    // f32w_row(a) of a = lane & 15 (mlp_tables.h), bit by bit: 8 (a >> 1 & 1) + 4 (a >> 2 & 1) + 2 (a & 1) + (a >> 3)
    const uint32_t arow = 8u * ((uint32_t)(s >> 1) & 1u) + 4u * ((uint32_t)(s >> 2) & 1u) + 2u * ((uint32_t)s & 1u) +
                          ((uint32_t)s >> 3);
    a_off = F32 ? 16u * (32u * (uint32_t)(g & 1) + arow) + 8u * (uint32_t)(g >> 1) : 16u * (uint32_t)lane;
    one16 = opaque_one16();
    dl = DmaLean{a.wpack, (uint32_t)(lane * 16 + wave * 1024),
                 (uint32_t)__builtin_amdgcn_readfirstlane(lds_base + (uint32_t)wave * 1024u),
                 (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)wave)};
  }

  template <int gi> __device__ __forceinline__ void fetch() {
    constexpr Group G = GT::t.g[gi];
    fetch_group_lean<P, G.c0, G.nch, (gi % NSLOT) * SLOT_CAP * 1024>(dl);
  }
  template <int gi, int i> __device__ __forceinline__ void fetch_piece() {
    constexpr Group G = GT::t.g[gi];
    fetch_piece_lean<P, G.c0, G.nch, (gi % NSLOT) * SLOT_CAP * 1024, i>(dl);
  }
  template <int S> __device__ __forceinline__ Tile& slot() {
    if constexpr (S >= TS_HA && S < TS_HB) return Ha[S - TS_HA];
    else if constexpr (S >= TS_HB && S < TS_X) return Hb[S - TS_HB];
    else if constexpr (S == TS_X || S == TS_X + 1) return X[S - TS_X];
    else {
      static_assert(S == TS_D, "forward tile slot");
      return D;
    }
  }
  template <int u> static __host__ __device__ constexpr int layer_of() { return fwd16_unit_layer(u); }
  template <int u> static __host__ __device__ constexpr int tile_of() { return u - fwd16_unit_first(fwd16_unit_layer(u)); }

  // vector-memory stores issued by unit u's finish
  static __host__ __device__ constexpr int unit_stores(int u) {
    if (!STORE) return 0;
    const int L = fwd16_unit_layer(u), mt = u - fwd16_unit_first(L);
    constexpr int ST = NERF_DIAG_NO_ACT ? 0 : SST, MS = NERF_DIAG_NO_MASK ? 0 : 1;
    if (L == LFA) return mt < 16 ? ST : 0;
    if (L == LRGB) return 0;
    return ST + (mt == fwd16_out_tiles(L) - 1 ? MS : 0);  // + the layer's mask store
  }
  static __host__ __device__ constexpr int group_stores(int gi) {
    int n = 0;
    for (int u = 0; u < NUNIT_FWD16; ++u)
      if (finished_in_group<DIR, DENSITY, P::CH, cross_finish<P, DIR>()>(gi, u)) n += unit_stores(u);
    return n;
  }
  // the training stores of one 32-feature tile (a K-block, or the two 16-row tiles that fill it): old
  // tile tau, 8 bytes of chunk c (hi) [and c + 2 (lo)] at this lane's slot
  __device__ __forceinline__ void store_half(int tau, int c, uint32_t h0, uint32_t h1, uint32_t l0, uint32_t l1) {
    if constexpr (NERF_DIAG_NO_ACT) return;
    char* base = (char*)a.act + (((wb32 * AT_TILES + tau) * SCH + c) << 10) + st_off;
    store8(base, h0, h1);
    if constexpr (!HALF) store8(base + 2048, l0, l1);
  }
  // PF32W: output-tile half hf of fp32 tile tau (values v[4 hf + e]).  Value e is feature 16 hf + f32w_feat(g, e) =
  // old register rho = 4 (2 hf + (e >> 1)) + 2 (e & 1) + (g >> 1) of old lane lold: lanes (s, g) and (s, g ^ 2) --
  // l and l ^ 32 -- hold elements {0, 2} and {1, 3} of the same two 16-byte pieces, chunks 2 hf and 2 hf + 1.  Two
  // v_permlane32_swap (on copies: the K-block keeps its order for the next layer's MFMAs) give the lower lane
  // the whole of piece 2 hf and the upper one the whole of 2 hf + 1 = chunk 2 hf + (g >> 1), st_off's.
  __device__ __forceinline__ void store_f32(int tau, int hf, const Tile& t) {
    if constexpr (NERF_DIAG_NO_ACT) return;
    char* base = (char*)a.act + (((wb32 * AT_TILES + tau) * SCH + 2 * hf) << 10) + st_off;
    const auto r0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(t.v[4 * hf]), __float_as_uint(t.v[4 * hf + 2]),
                                                     false, false);
    const auto r1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(t.v[4 * hf + 1]), __float_as_uint(t.v[4 * hf + 3]),
                                                     false, false);
    store16<0>((uint4*)base, make_uint4(r0[0], r0[1], r1[0], r1[1]));
  }
  __device__ __forceinline__ void store_kblock(int tau, const Tile& t) {
    if constexpr (F32) {
      store_f32(tau, 0, t);
      store_f32(tau, 1, t);
    } else {
      store_half(tau, 0, get_dword(t.hi, 0), get_dword(t.hi, 1), get_dword(t.lo, 0), get_dword(t.lo, 1));
      store_half(tau, 1, get_dword(t.hi, 2), get_dword(t.hi, 3), get_dword(t.lo, 2), get_dword(t.lo, 3));
    }
  }

  // ---- group_body hooks
  template <int u> static __host__ __device__ constexpr int group_of() {
    int gi = 0;
    while (!(GT::t.g[gi].u0 <= u && u < GT::t.g[gi].u0 + GT::t.g[gi].n)) ++gi;
    return gi;
  }
  template <int u, int t> __device__ __forceinline__ const Tile& in_tile() {
    return slot<fwd_in_slot(layer_of<u>(), t)>();
  }
  // the unit's bias chunk (rows 4 g + {0..3} = lane g) is the MFMA chain's initial accumulator, read one unit ahead
  // (PF32W: PF32's bias chunk of the 32-row unit holds row r at float r; rows 16 (mt & 1) + f32w_row(4 g + e) =
  // floats 16 (mt & 1) + 4 (g & 1) + (g >> 1) + {0, 2, 8, 10})
  template <int u> __device__ __forceinline__ void prefetch() {
    if constexpr (F32) {
      constexpr int u32 = f32w_unit32(u);
      constexpr int BOFF = fwd_unit_chunk_off(u32, PF32::CH) - GT::t.g[group_of<u>()].c0 + fwd_in_tiles(layer_of<u>()) * PF32::CH;
      typedef __attribute__((address_space(3))) const uint32_t lds_cu1;
      lds_cu1* bp = (lds_cu1*)wbg + BOFF * 256 + 16 * (tile_of<u>() & 1);
      bias = make_uint4(bp[0], bp[2], bp[8], bp[10]);
    } else {
      constexpr int BOFF = unit_chunk_off<2>(u, CH) - GT::t.g[group_of<u>()].c0 + fwd_in_tiles(layer_of<u>()) * CH;
      bias = as_uint4(wbg[BOFF * 64]);
    }
  }
  template <int u> __device__ __forceinline__ void init(Acc& acc) {
    constexpr int L = layer_of<u>(), mt = tile_of<u>();
    if constexpr (L == L5 && mt == 0 && !keep_pe<P>()) {
      settle(px);
      settle(py);
      settle(pz);
      pe_kblock<P, 0, 10, 63>(X[0], g, px, py, pz);
      pe_kblock<P, 1, 10, 63>(X[1], g, px, py, pz);
    }
    if constexpr (L == LV && mt == 0) {
      settle(dx);
      settle(dy);
      settle(dz);
      pe_kblock<P, 0, 4, 27>(D, g, dx, dy, dz);
    }
    acc[0] = __uint_as_float(bias.x);
    acc[1] = __uint_as_float(bias.y);
    acc[2] = __uint_as_float(bias.z);
    acc[3] = __uint_as_float(bias.w);
  }
  // part p of NP of output tile mt's finish: its register pairs [2p/NP, 2(p+1)/NP) into half mt & 1 of the
  // output K-block (in place), their mask bits; the last part stores (and the layer's last tile the masks)
  template <int u, int p> __device__ __forceinline__ void finish_part(const Acc& acc) {
    constexpr int L = layer_of<u>(), mt = tile_of<u>();
    constexpr int NP = finish_parts<P>();
    constexpr int K0 = 2 * p / NP, K1 = 2 * (p + 1) / NP;
    constexpr bool LASTP = p == NP - 1;
    if constexpr (L <= L7 || L == LV || (L == LFA && mt < 16)) {
      constexpr bool RELU = L != LFA;  // feature_linear: no activation
      constexpr int Q = 2 * (mt & 1);   // the K-block dwords of this tile: Q, Q + 1
      Tile& out = slot<fwd_out_slot(L, mt >> 1)>();
      uint32_t bits = 0;
      sfor<K1 - K0>([&](auto kk) {
        constexpr int k = K0 + decltype(kk)::value;
        float y0 = acc[2 * k], y1 = acc[2 * k + 1];
        if constexpr (RELU) {
          y0 = __int_as_float(max(__float_as_int(y0), 0));
          y1 = __int_as_float(max(__float_as_int(y1), 0));
        }
        if constexpr (F32) {
          // bits 2k, 2k + 1: the pair's values non-zero (after the ReLU: > 0)
          if constexpr (STORE && RELU && !NERF_DIAG_NO_MASK)
            bits |= (min((uint32_t)__float_as_int(y0), 1u) | (min((uint32_t)__float_as_int(y1), 1u) << 1)) << (2 * k);
          out.v[2 * Q + 2 * k] = y0;
          out.v[2 * Q + 2 * k + 1] = y1;
        } else {
          const uint32_t hw = pack_bf16(y0, y1);
          const uint32_t lw = pack_bf16(y0 - __uint_as_float(hw << 16), y1 - __uint_as_float(hw & 0xffff0000u));
          if constexpr (STORE && RELU && !NERF_DIAG_NO_MASK) bits |= nonzero_bf16x2(hw, one16) << k;  // (as PBF3)
          set_dword8(out.hi, Q + k, hw);
          set_dword8(out.lo, Q + k, lw);
        }
      });
      if constexpr (STORE) {
        constexpr int n = mt >> 1, d = mt >> 2;  // old 32-row tile, its mask dword
        if constexpr (RELU && !NERF_DIAG_NO_MASK) {
          // value 2k + j of this lane = old register rho = 4 (2 (mt & 1) + (g >> 1)) + 2k + j of old tile n, old
          // lane half h = g & 1: mask bit 8 (n & 1) + (rho >> 1) + 16 (rho & 1) = [bit k / 16 + k] << (C + gsh)
          // (PF32W: value e = old register rho = 4 (2 (mt & 1) + (e >> 1)) + 2 (e & 1) + (g >> 1), so rho >> 1 =
          // 4 (mt & 1) + e and rho & 1 = g >> 1: [bit e] << (C + 16 (g >> 1)))
          constexpr uint32_t C = 8 * (n & 1) + 4 * (mt & 1);
          const uint32_t b = bits << (C + gsh);
          if constexpr ((mt & 3) == 0 && p == 0) mw[d] = b;
          else mw[d] |= b;
        }
        if constexpr (LASTP) {
          constexpr int tau = (L == LV ? AT_V : L == LFA ? AT_F : AT_H + 8 * L) + n;
          if constexpr (F32) store_f32(tau, mt & 1, out);
          else store_half(tau, mt & 1, get_dword(out.hi, Q), get_dword(out.hi, Q + 1), get_dword(out.lo, Q),
                          get_dword(out.lo, Q + 1));
          if constexpr (RELU && !NERF_DIAG_NO_MASK && mt == fwd16_out_tiles(L) - 1) {
            // old lane L gets its bits from lanes l and l + 32 (g = h, h + 2): OR in the partner's dwords; lanes l
            // and l + 32 then hold the same 16 bytes for the same old lane and both store them
            constexpr int ND = L == LV ? 2 : 4;
            uint32_t full[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int q = 0; q < ND; ++q) {
              const auto r = __builtin_amdgcn_permlane32_swap(mw[q], mw[q], false, false);
              full[q] = mw[q] | (lane < 32 ? r[1] : r[0]);
            }
            store16<0>((uint4*)((char*)a.masks + ((wb32 * MASK_GROUPS + (L == LV ? 8 : L)) * 64 + lold) * 16),
                       make_uint4(full[0], full[1], full[2], full[3]));
          }
        }
      }
    } else if constexpr (L == LFA) {  // the alpha row: row 0 = register 0 of lane group 0
      if constexpr (p == 0) alpha = acc[0];
    } else if constexpr (p == 0) {    // LRGB: rows 0..2 = registers 0..2 of lane group 0
      if constexpr (F32) {
        // rows f32w_row(4 g + e): 0 and 2 in registers 0, 1 of lane group 0, 1 in register 0 of lane group 2
        static_assert(f32w_row(0) == 0 && f32w_row(8) == 1 && f32w_row(1) == 2, "the rgb rows of the wide fp32 unit");
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[0]), __float_as_uint(acc[0]), false, false);
        rgb0 = acc[0];
        rgb1 = __uint_as_float(r[1]);  // (lanes < 32: the value of lane + 32)
        rgb2 = acc[1];
      } else {
        rgb0 = acc[0];
        rgb1 = acc[1];
        rgb2 = acc[2];
      }
    }
  }

  template <int gi> __device__ __forceinline__ void step() {
    constexpr int NG = GT::t.n;
    if constexpr (gi + PF < NG && dma_spread<P>() == 0) fetch<gi + PF>();
    const uint32_t sl = lds_base + (uint32_t)((gi % NSLOT) * SLOT_CAP * 1024);
    wbg = lds_ptr(sl + (F32 ? 16u * (uint32_t)(g & 1) + 4u * (uint32_t)(g >> 1) : 16u * (uint32_t)g));
    group_body<P, DIR, DENSITY, gi>(*this, lds_ptr(sl + a_off));
    constexpr int N = dma_spread<P>() > 0
        ? handoff_vmcnt_spread<P, DIR, DENSITY>(gi, [](int u) constexpr { return unit_stores(u); })
        : handoff_vmcnt<P, DIR, DENSITY>(gi, [](int i) constexpr { return group_stores(i); }, STORE ? PRO_ST : 0);
    if constexpr (gi + 1 < NG) wait_barrier<N>();
  }

  __device__ __forceinline__ void run() {
    const int64_t ms = m < a.M ? m : a.M - 1;
    px = a.pts[ms * 3 + 0];
    py = a.pts[ms * 3 + 1];
    pz = a.pts[ms * 3 + 2];
    dx = dy = dz = 0.f;
    if constexpr (!DENSITY) {
      const int64_t di = a.dir_index ? (int64_t)a.dir_index[ms] : ms / a.samples_per_dir;
      dx = a.dirs[di * 3 + 0];
      dy = a.dirs[di * 3 + 1];
      dz = a.dirs[di * 3 + 2];
    }
    sfor<(PF < GT::t.n ? PF : GT::t.n)>([&](auto gg) { fetch<decltype(gg)::value>(); });
    pe_kblock<P, 0, 10, 63>(X[0], g, px, py, pz);
    pe_kblock<P, 1, 10, 63>(X[1], g, px, py, pz);
    if constexpr (STORE) {
      Tile Dt;
      pe_kblock<P, 0, 4, 27>(Dt, g, dx, dy, dz);
      store_kblock(AT_X, X[0]);
      store_kblock(AT_X + 1, X[1]);
      store_kblock(AT_D, Dt);
    }
    {  // group 0 landed: younger = the DMAs of groups 1 .. PF - 1 and the PE stores (3 K-blocks x 2 halves)
      constexpr int N0 = [] {
        int n = STORE ? PRO_ST : 0;
        for (int j = 1; j < PF && j < GT::t.n; ++j) n += group_dma<P, DIR, DENSITY>(j);
        return n;
      }();
      wait_barrier<N0>();
    }
    settle(dx);
    settle(dy);
    settle(dz);
    sfor<GT::t.n>([&](auto gg) { step<decltype(gg)::value>(); });
    if (g == 0 && m < a.M)
      *(float4*)(a.raw + m * 4) = DENSITY ? make_float4(0.f, 0.f, 0.f, alpha) : make_float4(rgb0, rgb1, rgb2, alpha);
  }
};

template <class P, bool STORE, bool DENSITY, bool PERSIST, bool HALF>
using FwdWaveOf = std::conditional_t<wide_kind<P>(), FwdWave16<P, STORE, DENSITY, PERSIST, HALF>,
                                     FwdWave<P, STORE, DENSITY, PERSIST, HALF>>;

// PERSIST (inference only): the sample count is read on the device (a.M_dev, e.g. the grid
// march's gather count: no host round trip sizes the launch) and a grid of one wave of
// workgroups loops over the sample blocks; the barrier at the end of each block keeps the next
// block's prologue DMA out of the ring slot still being read.
template <class P, bool STORE, bool DENSITY, bool PERSIST, bool HALF = false>
__global__ void __launch_bounds__(P::WAVES * 64) fwd_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 smem_u4[];
  if constexpr (!PERSIST) {
    FwdWaveOf<P, STORE, DENSITY, false, HALF> w(a, smem_u4, blockIdx.x, threadIdx.x);
    w.run();
  } else {
    static_assert(!STORE, "the persistent forward is inference only");
    const int64_t cnt = a.M_dev[0];
    FwdArgs b = a;
    b.M = cnt < a.M_cap ? cnt : a.M_cap;
    for (int64_t blk = blockIdx.x; blk * samples_per_block<P>() < b.M; blk += gridDim.x) {
      // the thread id, laundered per block: every lane-dependent address (the weight DMA sources,
      // the LDS read bases) is then recomputed inside the body, as in the one-block kernel,
      // instead of being hoisted out of the loop and held in registers across it (spills)
      int tid = threadIdx.x;
      asm volatile("" : "+v"(tid));
      FwdWaveOf<P, STORE, DENSITY, true, false> w(b, smem_u4, blk, tid);
      w.run();
      __syncthreads();
    }
  }
}

}  // namespace mlp
}  // namespace nerf
