// Fused NeRF MLP: the dW / db kernel, its work items' layout and the ordered reduce.
#pragma once
#include "mlp_pe_store.h"

namespace nerf {
namespace mlp {

// ------------------------------------------------------------------------------------
// dW / db: C[n][k] += sum_m dz[n][m] act[k][m] (K = samples), one pass over the stores.
//
// Ten jobs, each reading every tile it needs once per 32-sample block (159 tile-blocks per
// block for the whole net):
//   J0..J7  pts_linears.l: 8 dZ_l tiles x (2 | 8 | 10) act tiles; wave w owns n-tile w
//   J8      feature_linear (8 dF x 8 h7) + alpha_linear (dA x h7): wave w also owns the
//           alpha row against h7 tile w
//   J9      views_linears (4 dZv x [8 feature, PE(dir)]) on waves 0..3 + rgb_linear
//           (d rgb x hv tile w-4) on waves 4..7
// Work items = (job, contiguous block range) sized to equal bytes, as many as there are
// CUs (nerf_mlp_dw_items), so the single wave of workgroups ends together.  Per block, a
// job's tile-blocks (fragment-native, mlp_tables.h) stream into an LDS ring with LDS-DMA
// and are read back transposed (ds_read_b64_tr_b16): row i of a fragment <-> feature
// acc_row(i & 15, i >> 4).  Each item adds its partial sums with fp32 atomics.
// ------------------------------------------------------------------------------------
constexpr int DW_WAVES = 8;
constexpr int DW_SLOTS = 18;  // most tile-blocks one job reads per block
constexpr int NDWJOB = 10;
enum DwKind { DW_REG = 0, DW_FA = 1, DW_VR = 2 };

struct DwJobDesc {
  int kind, kt;     // kind; k-tiles per wave (REG / FA trunk / VR view waves)
  int nd, na;       // dz tiles, act tiles (LDS slots [0, nd) then [nd, nd + na))
  int dz[9];        // dz tile ids
  int act[13];      // act tile ids
};
__host__ __device__ constexpr DwJobDesc dw_job_desc(int j) {
  DwJobDesc d{};
  if (j < 8) {
    d.kind = DW_REG;
    d.kt = gemm_k_tiles(j);
    d.nd = 8;
    d.na = d.kt;
    for (int n = 0; n < 8; ++n) d.dz[n] = ZT_H + 8 * j + n;
    for (int t = 0; t < d.kt; ++t) d.act[t] = gemm_act_tile(j, t);
  } else if (j == 8) {
    d.kind = DW_FA;
    d.kt = 8;
    d.nd = 9;
    d.na = 8;
    for (int n = 0; n < 8; ++n) d.dz[n] = ZT_F + n;
    d.dz[8] = ZT_A;
    for (int t = 0; t < 8; ++t) d.act[t] = AT_H + 56 + t;
  } else {
    d.kind = DW_VR;
    d.kt = 9;
    d.nd = 5;
    d.na = 13;
    for (int n = 0; n < 4; ++n) d.dz[n] = ZT_V + n;
    d.dz[4] = ZT_RGB;
    for (int t = 0; t < 8; ++t) d.act[t] = AT_F + t;
    d.act[8] = AT_D;
    for (int t = 0; t < 4; ++t) d.act[9 + t] = AT_V + t;
  }
  return d;
}
__host__ __device__ constexpr int dw_job_tiles(int j) { return dw_job_desc(j).nd + dw_job_desc(j).na; }

// LDS ring depth: 4 x 36 KiB (bf16), 2 x 72 KiB (fp32)
constexpr int DW_NBUF_BF16 = 4;
template <class P> __host__ __device__ constexpr int dw_nbuf() { return P::KIND == K_BF16 ? DW_NBUF_BF16 : 2; }
__host__ __device__ constexpr int perm_row(int i) { return acc_row(i & 15, i >> 4); }

// work items: segment s = items [item_off[s], item_off[s + 1]) of job job_of[s]
// (item_off[NDWJOB] = total); segments are ordered longest item first
struct DwArgs {
  const void* dz;
  const void* act;
  int64_t nblk;       // 32-sample blocks in the stores
  float* grad;        // flat [NET_PARAMS], accumulated
  int item_off[NDWJOB + 1];
  int job_of[NDWJOB];
  float* partial;     // per-item partial sums (deterministic mode, dw_reduce_kernel) or null (atomics)
};

// Deterministic mode: every work item writes its accumulators, fragment-native, to its own
// slice of `partial` -- per wave DW_PSLOTS tiles (acc[0..9] -> 0..9, acc2 -> 10) of 64 lanes x
// 16 floats, then 128 floats of row sums (dbias lanes 0..63, dbias2 lanes 0..63) -- and
// dw_reduce_kernel adds the items of each job in item order: the same sum on every run.
constexpr int DW_PSLOTS = 11;
constexpr int DW_PWAVE = DW_PSLOTS * 1024 + 128;   // floats per wave
constexpr int DW_PITEM = DW_WAVES * DW_PWAVE;      // floats per item

// s_waitcnt vmcnt(n) for a wave-uniform runtime n in [0, 63] (n is a multiple of G here)
__device__ __forceinline__ void wait_vmcnt_rt(int n) {
#define NERF_VMW(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
  switch (n) {
    NERF_VMW(0) NERF_VMW(1) NERF_VMW(2) NERF_VMW(3) NERF_VMW(4) NERF_VMW(5) NERF_VMW(6) NERF_VMW(7)
    NERF_VMW(8) NERF_VMW(9) NERF_VMW(10) NERF_VMW(11) NERF_VMW(12) NERF_VMW(13) NERF_VMW(14) NERF_VMW(15)
    NERF_VMW(16) NERF_VMW(17) NERF_VMW(18)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
#undef NERF_VMW
}

typedef __attribute__((ext_vector_type(4))) short short4_t;
typedef __attribute__((address_space(3))) short4_t lds_short4;

// bf16 LDS swizzle of the dW ring.  A stored chunk is 64 lane-linear 16-B pieces; the
// transposed fragment read below touches pieces p = 16 a + b with b in {q, q + 4} (+ 8 for
// lanes 32..63), a in {s, s + 2}, of both chunks of a tile at once -- 16 of the 64 banks
// as stored.  Piece p of chunk c is placed at slot 16 a + (b + 4 (a >> 1) + 8 c) mod 16
// instead (the DMA's per-lane source address does the permutation for free), which makes
// every ds_read_b64_tr_b16 conflict-free.
__host__ __device__ constexpr int dw_swz(int c, int p) {
  return 16 * (p >> 4) + (((p & 15) + 4 * ((p >> 4) >> 1) + 8 * c) & 15);
}
__host__ __device__ constexpr int dw_unswz(int c, int slot) {
  return 16 * (slot >> 4) + (((slot & 15) - 4 * ((slot >> 4) >> 1) - 8 * c) & 15);
}

// bf16: the 8-sample K fragment (samples 16 s + 8 h + [0, 8)) of row (lane & 31)
__device__ __forceinline__ bf16x8 dw_frag_bf16(const char* tile, int s, int lane) {
  const int l16 = lane & 15, G = lane >> 4;
  const int hp = G & 1, h = G >> 1, q = l16 >> 2, pp = l16 & 3;
  const int c = pp >> 1, p = 16 * s + 8 * h + q + 32 * hp;
  const char* base = tile + c * 1024 + (pp & 1) * 8;
  short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4*)(base + dw_swz(c, p) * 16));
  short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4*)(base + dw_swz(c, p + 4) * 16));
  typedef __attribute__((ext_vector_type(8))) short short8_t;
  short8_t v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  return __builtin_bit_cast(bf16x8, v);
}
// fp32 LDS swizzle of the dW ring.  The K = 2 fragment read below has the 32 lanes of one
// ds_read_b32 bank group touch pieces p in {2 s + h, 2 s + h + 32} of all 4 chunks (dword
// rho & 3 of each): as stored, those 8 pieces sit at the same (slot mod 8), i.e. on 4 of the
// 32 banks -- an 8-way conflict.  Piece p of chunk c is placed at slot
// (p & ~7) | ((p + 2 c + (p >> 5)) & 7) instead, which puts the 8 pieces on 8 distinct
// (slot mod 8) and every read conflict-free.
__host__ __device__ constexpr int dw_swz_f32(int c, int p) { return (p & ~7) | ((p + 2 * c + (p >> 5)) & 7); }
__host__ __device__ constexpr int dw_unswz_f32(int c, int q) { return (q & ~7) | ((q - 2 * c - (q >> 5)) & 7); }

// fp32: the K = 2 fragment (sample 2 s + h) of row (lane & 31).  With s = 4 a + b, the slot
// dw_swz_f32(c, 2 s + h + 32 hp) = 8 a + 32 hp + ((2 b + h + 2 c + hp) & 7): the per-lane part
// depends on s & 3 only.  A tile region's four per-lane bases (F32Base) are laundered through
// empty asm, so every read is one ds_read_b32 at base + immediate (tile * 4 KiB + 128 a).
__device__ __forceinline__ uint32_t dw_f32_lane_off(int lane, int b) {
  const int rho = lane & 15, hp = (lane >> 4) & 1, h = lane >> 5, c = rho >> 2;
  const int sw = 2 * c + hp;  // (the swizzle)
  return (uint32_t)(c * 1024 + 512 * hp + 16 * ((2 * b + h + sw) & 7) + 4 * (rho & 3));
}
struct F32Base { uint32_t b[4]; };
__device__ __forceinline__ F32Base f32_base(uint32_t region, const uint32_t (&lane_off)[4]) {
  F32Base r;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    r.b[b] = region + lane_off[b];
    settle(r.b[b]);
  }
  return r;
}
typedef __attribute__((address_space(3))) const float lds_cf;
template <int IMM>
__device__ __forceinline__ float f32_frag(const F32Base& B, int s) {
  static_assert(IMM >= 0 && IMM + 128 * 3 < 65536, "ds_read offset is 16 bits");
  return *(lds_cf*)(uintptr_t)(B.b[s & 3] + (uint32_t)(IMM + 128 * (s >> 2)));
}
// step after which the fp32 K loop issues the next block's DMA, waves 4..7 DW_FETCH_SPLIT steps later
// (after step 1 / step 5: 5.05 -> 4.95 ms at 524k samples)
constexpr int DW_FETCH_STEP = 1;
constexpr int DW_FETCH_SPLIT = 4;

// one K step (16 samples) of C += A B^T for A = LDS tile `at`, bf16 / bf16x3 (the fp32 K loop of dw_job reads its
// fragments through f32_frag)
template <class P>
__device__ __forceinline__ f32x16 dw_mma(const char* at, const char* bt, int s, int lane, f32x16 acc) {
  if constexpr (P::KIND == K_BF16) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(dw_frag_bf16(at, s, lane), dw_frag_bf16(bt, s, lane), acc, 0, 0, 0);
  } else {  // tile-block = hi (2 KiB) then lo (2 KiB)
    static_assert(P::KIND == K_BF16X3, "dw_mma: bf16 or bf16x3");
    const bf16x8 ah = dw_frag_bf16(at, s, lane), al = dw_frag_bf16(at + 2048, s, lane);
    const bf16x8 bh = dw_frag_bf16(bt, s, lane), bl = dw_frag_bf16(bt + 2048, s, lane);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
  }
}
template <class P>
__device__ __forceinline__ float dw_rowsum(const char* at, int s, int lane) {
  const bf16x8 v = dw_frag_bf16(at, s, lane);
  float r = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) r += (float)v[e];
  if constexpr (P::KIND == K_BF16X3) {
    const bf16x8 l = dw_frag_bf16(at + 2048, s, lane);
    float q = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) q += (float)l[e];
    r += q;
  }
  return r;
}

// add a 32 x 32 accumulator tile into weight WP at rows 32 ntile + perm, columns col0 +
// perm (valid rows < nvalid, valid columns < cvalid of the tile).  The layout functions
// are loops: every use sits in a constant expression.
template <int WP>
__device__ __forceinline__ void dw_flush(float* grad, int ntile, int nvalid, int col0, int cvalid, const f32x16& acc,
                                         int lane) {
  constexpr int64_t OFF = param_offset(WP);
  constexpr int K = weight_K(WP);
  float* gw = grad + OFF;
  const int h = lane >> 5, colf = perm_row(lane & 31);
  if (colf >= cvalid) return;
#pragma unroll
  for (int rho = 0; rho < 16; ++rho) {
    const int n = 32 * ntile + perm_row(acc_row(rho, h));
    if (n < nvalid) atomicAdd(gw + (int64_t)n * K + col0 + colf, acc[rho]);
  }
}
template <int WPB>
__device__ __forceinline__ void dw_flush_bias(float* grad, int ntile, int nvalid, float dbias, int lane) {
  constexpr int64_t OFF = param_offset(WPB);
  dbias += __shfl_xor(dbias, 32, 64);
  const int n = 32 * ntile + perm_row(lane & 31);
  if (lane < 32 && n < nvalid) atomicAdd(grad + OFF + n, dbias);
}

// LDS slot of job tile q (q < nd: dz tile q, else act tile q - nd): the act tiles come first,
// so a K step's act-tile reads are one per-lane base + immediates below 64 KiB
__host__ __device__ constexpr int dw_slot(const DwJobDesc& d, int q) { return q < d.nd ? d.na + q : q - d.nd; }

// dW's tile stream is read exactly once (each tile-block by one work item), so it is loaded nt
// (bf16 dW 0.957 -> 0.926 ms, bf16x3 2.05 -> 2.02 at 524,288 samples; fp32 unchanged)
// global_load_lds_dwordx4 with a uniform 64-bit base (SGPR pair) + per-lane 32-bit offset
// (the SADDR form: one VGPR per fetch stream instead of a 64-bit address pair)
__device__ __forceinline__ void glds16_saddr(const void* sbase, uint32_t voff, uint32_t lds_wave_base) {
  uint32_t saved;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
               : "=&s"(saved) : "v"(voff), "s"(sbase), "s"(__builtin_amdgcn_readfirstlane(lds_wave_base)) : "memory");
}

// a wave-uniform pointer made visibly uniform (SGPR pair) to the compiler
__device__ __forceinline__ const char* uniform_ptr(const char* p) {
  const uint64_t v = (uint64_t)(uintptr_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (const char*)(uintptr_t)(((uint64_t)hi << 32) | lo);
}

template <class P, int J>
__device__ __forceinline__ void dw_job(const DwArgs& a, int64_t b_begin, int64_t b_end, char* lds) {
  constexpr DwJobDesc JD = dw_job_desc(J);
  constexpr int TB = P::CH * 1024;            // tile-block bytes
  constexpr int BUF = DW_SLOTS * TB;          // one stage of the ring
  constexpr int NT = JD.nd + JD.na;
  constexpr int NCHUNK = NT * P::CH;
  constexpr int G = (NCHUNK + DW_WAVES - 1) / DW_WAVES;  // DMA per wave per block (uniform)
  constexpr int NBUF = dw_nbuf<P>(), D = NBUF - 1;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;  // (kept divergent to the compiler: uniform branching spills)

  // DMA streams, resolved once (a table lookup inside the loop would be a compiler-visible
  // load, whose wait drains the ring): uniform tile base (block 0) + per-lane piece offset
  const char* sb[G];
  uint32_t voff[G];
  uint32_t dst[G];
  int64_t bstride[G];
#pragma unroll
  for (int i = 0; i < G; ++i) {
    const int k = cmin(wave + DW_WAVES * i, NCHUNK - 1);
    const int q = k / P::CH, c = k % P::CH;
    const bool is_dz = q < JD.nd;
    int tau = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t == q) tau = t < JD.nd ? JD.dz[t] : JD.act[t - JD.nd];
    const int ntiles = is_dz ? ZT_TILES : AT_TILES;
    // swizzled rings (bf16x3: chunks 2, 3 are the lo tile, swizzled as chunks 0, 1)
    const int piece = P::KIND != K_F32 ? dw_unswz(c & 1, lane) : dw_unswz_f32(c, lane);
    sb[i] = uniform_ptr((const char*)(is_dz ? a.dz : a.act) + tile_kib(a.nblk, ntiles, tau, 0, c, P::CH) * 1024);
    voff[i] = (uint32_t)(piece * 16);
    bstride[i] = block_stride_kib(ntiles, P::CH) * 1024;
    int slot = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t == q) slot = dw_slot(JD, t);
    dst[i] = (uint32_t)(slot * TB + c * 1024);
  }
  const uint32_t lds_base = (uint32_t)(uintptr_t)(lds_void*)lds;
  auto fetch = [&](int64_t b, int buf) {
#pragma unroll
    for (int i = 0; i < G; ++i)
      glds16_saddr(uniform_ptr(sb[i] + b * bstride[i]), voff[i], lds_base + (uint32_t)(buf * BUF) + dst[i]);
  };

  // wave roles
  //   REG: dz tile w x act tiles 0 .. kt;  FA: + alpha (dz tile 8) x act tile w
  //   VR: waves 0..3 dz tile w x act tiles 0 .. 9; waves 4..7 d rgb (dz tile 4) x act tile 9 + (w - 4)
  const bool vr_rgb = JD.kind == DW_VR && wave >= 4;
  const int n_q = vr_rgb ? 4 : wave;         // dz tile of this wave
  const int n_lds = JD.na + n_q;             // its LDS slot
  f32x16 acc[10], acc2;
#pragma unroll
  for (int t = 0; t < 10; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc2[i] = 0.f;
  float dbias = 0.f, dbias2 = 0.f;
  uint32_t lane_off[4];
#pragma unroll
  for (int bb = 0; bb < 4; ++bb) lane_off[bb] = dw_f32_lane_off(lane, bb);

  for (int d = 0; d < D; ++d)
    if (b_begin + d < b_end) fetch(b_begin + d, d);
  int buf = 0;
  for (int64_t b = b_begin; b < b_end; ++b) {
    const int younger = (int)min((int64_t)(D - 1), b_end - 1 - b);
    wait_vmcnt_rt(G * younger);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    // fp32: the next block's DMA is issued inside the K loop (DW_FETCH_STEP), the two waves of a SIMD
    // (w, w + 4) at different steps, so its ~70 issue slots overlap the partner's MFMAs
    const int fbuf = buf == 0 ? NBUF - 1 : buf - 1;
    if (P::KIND != K_F32 && b + D < b_end) fetch(b + D, fbuf);
    const char* tiles = lds + buf * BUF;
    if constexpr (P::KIND == K_F32) {
      // 16 K steps, fully unrolled, software-pipelined one step deep: step s + 1's fragments
      // (the dz fragment, the k-tiles' act fragments, the alpha pair) are read before step
      // s's MFMAs issue, fenced by sched_barrier so hipcc keeps that order (on its own it read
      // two fragments, waited lgkmcnt(0), issued two MFMAs: every LDS latency exposed).
      // Every read is one of four per-lane bases (s & 3) + an immediate (< 64 KiB).
      constexpr int KT = JD.kind == DW_VR ? 9 : JD.kt;
      constexpr int NF = 1 + KT + (JD.kind == DW_FA ? 2 : 0);
      const uint32_t region = lds_base + (uint32_t)(buf * BUF);
      const F32Base Bn = f32_base(region + (uint32_t)(n_lds * TB), lane_off);
      // act tiles: all of them from slot 0 (immediates t * 4 KiB), or the rgb wave's one
      const F32Base Ba = f32_base(region + (uint32_t)(vr_rgb ? (9 + wave - 4) * TB : 0), lane_off);
      F32Base Bal{}, Bw{};
      if constexpr (JD.kind == DW_FA) {
        Bal = f32_base(region + (uint32_t)((JD.na + 8) * TB), lane_off);
        Bw = f32_base(region + (uint32_t)(wave * TB), lane_off);
      }
      float fr[2][NF];
      auto rd = [&](auto ss, float (&f)[NF]) {
        constexpr int s = decltype(ss)::value;
        constexpr int SOFF = 128 * (s >> 2);
        f[0] = f32_frag<SOFF>(Bn, s & 3);
        if (!vr_rgb) {
          sfor<KT>([&](auto tt) {
            constexpr int t = decltype(tt)::value;
            f[1 + t] = f32_frag<t * TB + SOFF>(Ba, s & 3);
          });
        } else {
          f[1] = f32_frag<SOFF>(Ba, s & 3);
        }
        if constexpr (JD.kind == DW_FA) {
          f[KT + 1] = f32_frag<SOFF>(Bal, s & 3);
          f[KT + 2] = f32_frag<SOFF>(Bw, s & 3);
        }
      };
      auto mm = [&](const float (&f)[NF]) {
        dbias += f[0];
        if (!vr_rgb) {
          sfor<KT>([&](auto tt) {
            constexpr int t = decltype(tt)::value;
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(f[0], f[1 + t], acc[t], 0, 0, 0);
          });
        } else {
          acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(f[0], f[1], acc[0], 0, 0, 0);
        }
        if constexpr (JD.kind == DW_FA) {
          if (wave == 0) dbias2 += f[KT + 1];
          acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(f[KT + 1], f[KT + 2], acc2, 0, 0, 0);
        }
      };
      rd(std::integral_constant<int, 0>{}, fr[0]);
      const bool fhi = wave >= 4;
      sfor<16>([&](auto ss) {
        constexpr int s = decltype(ss)::value;
        if constexpr (s + 1 < 16) rd(std::integral_constant<int, s + 1>{}, fr[(s + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        mm(fr[s & 1]);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (s == DW_FETCH_STEP) {
          if (!fhi && b + D < b_end) fetch(b + D, fbuf);
          __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (s == DW_FETCH_STEP + DW_FETCH_SPLIT) {
          if (fhi && b + D < b_end) fetch(b + D, fbuf);
          __builtin_amdgcn_sched_barrier(0);
        }
      });
    } else {  // bf16 / bf16x3: 2 K steps of 16 samples
      const char* nt = tiles + n_lds * TB;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (!vr_rgb) {
          dbias += dw_rowsum<P>(nt, s, lane);
#pragma unroll
          for (int t = 0; t < JD.kt; ++t) acc[t] = dw_mma<P>(nt, tiles + t * TB, s, lane, acc[t]);
        } else {
          dbias += dw_rowsum<P>(nt, s, lane);
          acc[0] = dw_mma<P>(nt, tiles + (9 + (wave - 4)) * TB, s, lane, acc[0]);
        }
        if constexpr (JD.kind == DW_FA) {
          const char* at = tiles + (JD.na + 8) * TB;
          if (wave == 0) dbias2 += dw_rowsum<P>(at, s, lane);
          acc2 = dw_mma<P>(at, tiles + wave * TB, s, lane, acc2);
        }
      }
    }
    buf = buf == NBUF - 1 ? 0 : buf + 1;
  }

  if (a.partial) {  // deterministic: the item's sums to its own slice (dw_reduce_kernel adds them)
    float* pw = a.partial + ((int64_t)blockIdx.x * DW_WAVES + wave) * DW_PWAVE;
    auto put = [&](int slot, const f32x16& v) {
      float* d = pw + slot * 1024 + lane * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q) *(float4*)(d + q * 256) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    };
    constexpr int NACC = JD.kind == DW_VR ? 9 : JD.kt;
    if (!vr_rgb) {
      sfor<NACC>([&](auto tt) { put(decltype(tt)::value, acc[decltype(tt)::value]); });
    } else {
      put(0, acc[0]);
    }
    if constexpr (JD.kind == DW_FA) put(10, acc2);
    pw[DW_PSLOTS * 1024 + lane] = dbias;
    pw[DW_PSLOTS * 1024 + 64 + lane] = dbias2;
    return;
  }
  // flush (state_dict layout: weight [N][K] row-major)
  if constexpr (JD.kind == DW_REG) {
    constexpr int WP = gemm_weight(J);
    sfor<JD.kt>([&](auto tt) {
      constexpr int t = decltype(tt)::value;
      constexpr int C0 = gemm_col0(J, t), CV = gemm_col_valid(J, t);
      dw_flush<WP>(a.grad, wave, 256, C0, CV, acc[t], lane);
    });
    dw_flush_bias<WP + 1>(a.grad, wave, 256, dbias, lane);
  } else if constexpr (JD.kind == DW_FA) {
#pragma unroll
    for (int t = 0; t < 8; ++t) dw_flush<P_FW>(a.grad, wave, 256, 32 * t, 32, acc[t], lane);
    dw_flush_bias<P_FB>(a.grad, wave, 256, dbias, lane);
    dw_flush<P_AW>(a.grad, 0, 1, 32 * wave, 32, acc2, lane);
    if (wave == 0) dw_flush_bias<P_AB>(a.grad, 0, 1, dbias2, lane);
  } else {
    if (!vr_rgb) {
#pragma unroll
      for (int t = 0; t < 9; ++t) dw_flush<P_VW>(a.grad, wave, 128, 32 * t, t < 8 ? 32 : 27, acc[t], lane);
      dw_flush_bias<P_VB>(a.grad, wave, 128, dbias, lane);
    } else {
      dw_flush<P_RW>(a.grad, 0, 3, 32 * (wave - 4), 32, acc[0], lane);
      if (wave == 4) dw_flush_bias<P_RB>(a.grad, 0, 3, dbias, lane);
    }
  }
}

template <class P>
__global__ void __launch_bounds__(DW_WAVES * 64) dw_kernel(DwArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint4 smem_u4[];
  char* lds = (char*)smem_u4;
  const int item = blockIdx.x;
  int seg = 0;
#pragma unroll
  for (int k = 1; k < NDWJOB; ++k) seg += a.item_off[k] <= item ? 1 : 0;
  const int n_items = a.item_off[seg + 1] - a.item_off[seg], i = item - a.item_off[seg];
  const int j = a.job_of[seg];
  const int64_t b_begin = a.nblk * i / n_items, b_end = a.nblk * (i + 1) / n_items;
  switch (j) {
    case 0: dw_job<P, 0>(a, b_begin, b_end, lds); break;
    case 1: dw_job<P, 1>(a, b_begin, b_end, lds); break;
    case 2: dw_job<P, 2>(a, b_begin, b_end, lds); break;
    case 3: dw_job<P, 3>(a, b_begin, b_end, lds); break;
    case 4: dw_job<P, 4>(a, b_begin, b_end, lds); break;
    case 5: dw_job<P, 5>(a, b_begin, b_end, lds); break;
    case 6: dw_job<P, 6>(a, b_begin, b_end, lds); break;
    case 7: dw_job<P, 7>(a, b_begin, b_end, lds); break;
    case 8: dw_job<P, 8>(a, b_begin, b_end, lds); break;
    default: dw_job<P, 9>(a, b_begin, b_end, lds); break;
  }
}

// flat-gradient index of element (wave w, slot t, lane, register rho) of job J's partial
// accumulators, or -1 (padding / unused): the inverse of the dw_flush / dw_flush_bias maps.
// Slot DW_PSLOTS holds the row sums: q = element (0..127) -- q < 32: dbias of lanes q and
// q + 32 (returned for q only; the caller adds both), 64 <= q < 96: dbias2 likewise.
template <int J>
__device__ __forceinline__ int64_t dw_param_index(int w, int t, int lane, int rho) {
  constexpr DwJobDesc JD = dw_job_desc(J);
  const int h = lane >> 5, colf = perm_row(lane & 31), nrow = perm_row(acc_row(rho, h));
  if constexpr (JD.kind == DW_REG) {
    constexpr int WP = gemm_weight(J);
    if (t >= JD.kt) return -1;
    const int c0 = gemm_col0(J, t), cv = gemm_col_valid(J, t);
    if (colf >= cv) return -1;
    return param_offset(WP) + (int64_t)(32 * w + nrow) * weight_K(WP) + c0 + colf;
  } else if constexpr (JD.kind == DW_FA) {
    if (t < 8) return param_offset(P_FW) + (int64_t)(32 * w + nrow) * 256 + 32 * t + colf;
    if (t == 10 && nrow < 1) return param_offset(P_AW) + 32 * w + colf;
    return -1;
  } else {
    if (w < 4) {
      if (t >= 9 || colf >= (t < 8 ? 32 : 27)) return -1;
      return param_offset(P_VW) + (int64_t)(32 * w + nrow) * 283 + 32 * t + colf;
    }
    if (t == 0 && nrow < 3) return param_offset(P_RW) + (int64_t)nrow * 128 + 32 * (w - 4) + colf;
    return -1;
  }
}
template <int J>
__device__ __forceinline__ int64_t dw_bias_index(int w, int q) {
  constexpr DwJobDesc JD = dw_job_desc(J);
  const int n = perm_row(q & 31);
  if (q < 32) {
    if constexpr (JD.kind == DW_REG) return param_offset(gemm_weight(J) + 1) + 32 * w + n;
    else if constexpr (JD.kind == DW_FA) return param_offset(P_FB) + 32 * w + n;
    else {
      if (w < 4) return param_offset(P_VB) + 32 * w + n;
      return (w == 4 && n < 3) ? param_offset(P_RB) + n : -1;
    }
  }
  if (q >= 64 && q < 96 && JD.kind == DW_FA && w == 0 && n < 1) return param_offset(P_AB);
  return -1;
}

struct DwReduceArgs {
  const float* partial;
  float* grad;
  int item_off[NDWJOB + 1];
  int job_of[NDWJOB];
};

// one thread per (segment, wave, partial element); sums the segment's items in order
template <int J>
__device__ __forceinline__ void dw_reduce_job(const DwReduceArgs& a, int i0, int n, int w, int e) {
  int64_t idx;
  bool bias = e >= DW_PSLOTS * 1024;
  if (!bias) {
    const int t = e >> 10, r = e & 1023, q = r >> 8, lane = (r >> 2) & 63, rho = 4 * q + (r & 3);
    idx = dw_param_index<J>(w, t, lane, rho);
  } else {
    idx = dw_bias_index<J>(w, e - DW_PSLOTS * 1024);
  }
  if (idx < 0) return;
  const float* p = a.partial + ((int64_t)i0 * DW_WAVES + w) * DW_PWAVE + e;
  // row sums: lanes q and q + 32 of one item
  auto item = [&](int i) { const float* pi = p + (int64_t)i * DW_PITEM; return bias ? pi[0] + pi[32] : pi[0]; };
  // the items in order, 8 loads in flight (a one-load-per-iteration loop made the reduce a chain of n
  // dependent round trips: 21 us per launch at ~25 items per job)
  float sum = 0.f;
  int i = 0;
  for (; i + 8 <= n; i += 8) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = item(i + k);
#pragma unroll
    for (int k = 0; k < 8; ++k) sum += v[k];
  }
  for (; i < n; ++i) sum += item(i);
  a.grad[idx] += sum;
}

#if !defined(NERF_MLP_PREC)  // non-template: defined in the C-ABI translation unit only
__global__ void dw_reduce_kernel(DwReduceArgs a) {
  const int seg = blockIdx.y;
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)DW_WAVES * DW_PWAVE) return;
  const int w = (int)(g / DW_PWAVE), e = (int)(g % DW_PWAVE);
  const int i0 = a.item_off[seg], n = a.item_off[seg + 1] - i0;
  switch (a.job_of[seg]) {
    case 0: dw_reduce_job<0>(a, i0, n, w, e); break;
    case 1: dw_reduce_job<1>(a, i0, n, w, e); break;
    case 2: dw_reduce_job<2>(a, i0, n, w, e); break;
    case 3: dw_reduce_job<3>(a, i0, n, w, e); break;
    case 4: dw_reduce_job<4>(a, i0, n, w, e); break;
    case 5: dw_reduce_job<5>(a, i0, n, w, e); break;
    case 6: dw_reduce_job<6>(a, i0, n, w, e); break;
    case 7: dw_reduce_job<7>(a, i0, n, w, e); break;
    case 8: dw_reduce_job<8>(a, i0, n, w, e); break;
    default: dw_reduce_job<9>(a, i0, n, w, e); break;
  }
}
#endif

}  // namespace mlp
}  // namespace nerf
