// Fused NeRF MLP: the precision policies (PF32 .. PBF16W), mask-bit and ReLU helpers.
#pragma once
#include "common.h"
#include "mlp_knobs.h"
#include "mlp_tables.h"

namespace nerf {
namespace mlp {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;

// registers 2k, 2k+1 of an fp32 accumulator as one packed bf16 pair (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){lo, hi}, bf16x2));
}

// ------------------------------------------------------------------------------------
// precision policies
// ------------------------------------------------------------------------------------
enum PKind { K_F32 = 0, K_BF16 = 1, K_BF16X3 = 2, K_BF16X6 = 3, K_BF16X3W = 4, K_F32W = 5, K_BF16W = 6 };

struct PF32 {
  static constexpr int KIND = K_F32;
  using Acc = f32x16;     // one 32x32 accumulator tile
  static constexpr int SPW = 32;  // samples per wave
  static constexpr int CH = 4;     // 1 KiB chunks per 32-feature input tile
  static constexpr int E = 4;      // elements per lane per chunk
  static constexpr int WAVES = 4;  // one wave per SIMD (<= 512 VGPR+AGPR)
  static constexpr int ESIZE = 4;
  static constexpr int SPL = 4;    // samples per 16-B lane load (dW GEMM)
  static constexpr int PE = 1;  // PE_LIBM: the fp32 parity path (pe_trig)
  using Store = float;
  struct Tile { float v[16]; };
  // (a packed 16-byte slot holds its four weights in the order rho 4c + 0, 2, 1, 3 -- rho_of below: the wide fp32
  // forward, PF32W, then reads its pair of one slot as 8 aligned bytes; here the order is a renaming of a's fields)
  static __device__ __forceinline__ f32x16 mma(uint4 a, const Tile& b, int c, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), b.v[4 * c + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), b.v[4 * c + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), b.v[4 * c + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), b.v[4 * c + 3], acc, 0, 0, 0);
    return acc;
  }
  static __device__ __forceinline__ void set(Tile& t, int rho, float x) { t.v[rho] = x; }
  // a whole tile from its 16 register values
  static __device__ __forceinline__ void pack16(Tile& t, const float (&v)[16]) {
#pragma unroll
    for (int rho = 0; rho < 16; ++rho) t.v[rho] = v[rho];
  }
  static __device__ __forceinline__ float get(const Tile& t, int rho) { return t.v[rho]; }
  static __device__ __forceinline__ Store cvt(float x) { return x; }
  // packed weight element e of chunk c: accumulator register (k order) and stored value
  static __host__ __device__ constexpr int rho_of(int c, int e) { return c * E + (e == 1 ? 2 : e == 2 ? 1 : e); }
  static __device__ __forceinline__ Store cvt_c(float x, int) { return x; }
  static __device__ __forceinline__ f32x16 mma_k(uint4 a, uint4 b, f32x16 acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    return acc;
  }
  static __device__ __forceinline__ float lsum(uint4 a) {
    return ((__uint_as_float(a.x) + __uint_as_float(a.y)) + __uint_as_float(a.z)) + __uint_as_float(a.w);
  }
  static __device__ __forceinline__ uint4 chunk(const Tile& t, int c) {
    return make_uint4(__float_as_uint(t.v[4 * c]), __float_as_uint(t.v[4 * c + 1]), __float_as_uint(t.v[4 * c + 2]),
                      __float_as_uint(t.v[4 * c + 3]));
  }
  // registers 2k, 2k + 1 of a tile (the finish writes a tile pair by pair)
  static __device__ __forceinline__ void set_pair(Tile& t, int k, float x0, float x1) {
    t.v[2 * k] = x0;
    t.v[2 * k + 1] = x1;
  }
};

struct PBF16 {
  static constexpr int KIND = K_BF16;
  using Acc = f32x16;     // one 32x32 accumulator tile
  static constexpr int SPW = 32;  // samples per wave
  static constexpr int CH = 2;
  static constexpr int E = 8;
  static constexpr int WAVES = 8;  // two waves per SIMD (<= 256 VGPR)
  static constexpr int ESIZE = 2;
  static constexpr int SPL = 8;
  static constexpr int PE = 0;  // PE_FAST: rounded to bf16 anyway
  using Store = __bf16;
  struct Tile { bf16x8 b[2]; };
  static __device__ __forceinline__ f32x16 mma(uint4 a, const Tile& b, int c, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), b.b[c], acc, 0, 0, 0);
  }
  static __device__ __forceinline__ void set(Tile& t, int rho, float x) { t.b[rho >> 3][rho & 7] = (__bf16)x; }
  static __device__ __forceinline__ void pack16(Tile& t, const float (&v)[16]) {
    uint32_t d[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = pack_bf16(v[2 * k], v[2 * k + 1]);
    t.b[0] = __builtin_bit_cast(bf16x8, make_uint4(d[0], d[1], d[2], d[3]));
    t.b[1] = __builtin_bit_cast(bf16x8, make_uint4(d[4], d[5], d[6], d[7]));
  }
  static __device__ __forceinline__ float get(const Tile& t, int rho) { return (float)t.b[rho >> 3][rho & 7]; }
  static __device__ __forceinline__ Store cvt(float x) { return (__bf16)x; }
  static __host__ __device__ constexpr int rho_of(int c, int e) { return c * E + e; }
  static __device__ __forceinline__ Store cvt_c(float x, int) { return (__bf16)x; }
  static __device__ __forceinline__ f32x16 mma_k(uint4 a, uint4 b, f32x16 acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
  }
  static __device__ __forceinline__ float lsum(uint4 a) {
    bf16x8 v = __builtin_bit_cast(bf16x8, a);
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += (float)v[i];
    return s;
  }
  static __device__ __forceinline__ uint4 chunk(const Tile& t, int c) { return __builtin_bit_cast(uint4, t.b[c]); }
  // packed pair k (registers 2k, 2k + 1) = dword k & 3 of chunk k >> 2
  static __device__ __forceinline__ void set_dword(Tile& t, int k, uint32_t d) {
    uint4 v = __builtin_bit_cast(uint4, t.b[k >> 2]);
    if ((k & 3) == 0) v.x = d;
    else if ((k & 3) == 1) v.y = d;
    else if ((k & 3) == 2) v.z = d;
    else v.w = d;
    t.b[k >> 2] = __builtin_bit_cast(bf16x8, v);
  }
  static __device__ __forceinline__ void set_pair(Tile& t, int k, float x0, float x1) {
    set_dword(t, k, pack_bf16(x0, x1));
  }
};

// bf16x3: every fp32 operand x is split x = hi + lo (hi = bf16(x), lo = bf16(x - hi), 16
// significant bits together) and a product is hi*hi + hi*lo + lo*hi on the bf16 MFMA with fp32
// accumulation -- 3 bf16 MFMAs (96 cycles) per K = 16 step instead of 8 fp32 ones (512 cycles),
// at ~1e-5 relative error per dot product (fp32-class; the fp32 parity tests hold at 1e-4).
// Weights: chunks 0, 1 = hi of k 0-7 / 8-15, chunks 2, 3 = lo.  Tiles hold hi and lo (16
// VGPRs, as fp32), stored as 4 KiB tile-blocks (hi 2 KiB then lo 2 KiB).
struct PBF3 {
  static constexpr int KIND = K_BF16X3;
  using Acc = f32x16;     // one 32x32 accumulator tile
  static constexpr int SPW = 32;  // samples per wave
  static constexpr int CH = 4;
  static constexpr int E = 8;
  static constexpr int WAVES = 4;  // one wave per SIMD (16-VGPR tiles)
  static constexpr int ESIZE = 4;
  static constexpr int SPL = 8;
  static constexpr int PE = 2;  // PE_POLY: fp32-accurate to 1.6 ulp, then split
  using Store = __bf16;
  struct Tile { bf16x8 hi[2], lo[2]; };
  static __device__ __forceinline__ f32x16 mma(uint4 a, const Tile& b, int c, f32x16 acc) {
    const bf16x8 av = __builtin_bit_cast(bf16x8, a);
    if (c < 2) {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, b.hi[c], acc, 0, 0, 0);
      return __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, b.lo[c], acc, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, b.hi[c - 2], acc, 0, 0, 0);
  }
  static __device__ __forceinline__ void set(Tile& t, int rho, float x) {
    const __bf16 h = (__bf16)x;
    t.hi[rho >> 3][rho & 7] = h;
    t.lo[rho >> 3][rho & 7] = (__bf16)(x - (float)h);
  }
  // packed pairs: hi = v_cvt_pk_bf16_f32, its fp32 value by a shift / mask, lo = the
  // residuals' pair (same values as set(), 4 VALU per pair instead of element inserts)
  static __device__ __forceinline__ void pack16(Tile& t, const float (&v)[16]) {
    uint32_t hw[8], lw[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      hw[k] = pack_bf16(v[2 * k], v[2 * k + 1]);
      lw[k] = pack_bf16(v[2 * k] - __uint_as_float(hw[k] << 16), v[2 * k + 1] - __uint_as_float(hw[k] & 0xffff0000u));
    }
    t.hi[0] = __builtin_bit_cast(bf16x8, make_uint4(hw[0], hw[1], hw[2], hw[3]));
    t.hi[1] = __builtin_bit_cast(bf16x8, make_uint4(hw[4], hw[5], hw[6], hw[7]));
    t.lo[0] = __builtin_bit_cast(bf16x8, make_uint4(lw[0], lw[1], lw[2], lw[3]));
    t.lo[1] = __builtin_bit_cast(bf16x8, make_uint4(lw[4], lw[5], lw[6], lw[7]));
  }
  static __device__ __forceinline__ float get(const Tile& t, int rho) {
    return (float)t.hi[rho >> 3][rho & 7] + (float)t.lo[rho >> 3][rho & 7];
  }
  static __host__ __device__ constexpr int rho_of(int c, int e) { return (c & 1) * E + e; }
  static __device__ __forceinline__ Store cvt_c(float x, int c) {
    const __bf16 h = (__bf16)x;
    return c < 2 ? h : (__bf16)(x - (float)h);
  }
  static __device__ __forceinline__ uint4 chunk(const Tile& t, int c) {
    return __builtin_bit_cast(uint4, c < 2 ? t.hi[c] : t.lo[c - 2]);
  }
  static __device__ __forceinline__ void put(bf16x8& dst, int q, uint32_t d) {
    uint4 v = __builtin_bit_cast(uint4, dst);
    if (q == 0) v.x = d;
    else if (q == 1) v.y = d;
    else if (q == 2) v.z = d;
    else v.w = d;
    dst = __builtin_bit_cast(bf16x8, v);
  }
  // registers 2k, 2k + 1 split into hi / lo pairs (the values pack16 gives)
  static __device__ __forceinline__ void set_pair(Tile& t, int k, float x0, float x1) {
    const uint32_t hw = pack_bf16(x0, x1);
    const uint32_t lw = pack_bf16(x0 - __uint_as_float(hw << 16), x1 - __uint_as_float(hw & 0xffff0000u));
    put(t.hi[k >> 2], k & 3, hw);
    put(t.lo[k >> 2], k & 3, lw);
  }

};

// bf16x6 (inference forward only, round 5): every fp32 operand split exactly into three bf16,
// x = hi + mid + lo (24 significant bits), and the six products hh, hm, mh, hl, lh, mm accumulated in
// fp32 on the bf16 MFMA (the dropped ml, lm, ll are < 2^-24 relative): at least as accurate as an fp32
// GEMM, at 6 bf16 MFMAs (192 cycles) per K = 16 step instead of 8 fp32 ones (512).  The render of the
// bf16x3 tiers evaluates its COARSE net with it (Network.mlp_dtype_for): a split-bf16 coarse net moves
// importance samples across CDF bins.  Activations stay fp32 in registers (16
// VGPRs per tile, as PF32) and are split when a K half is used (12 VGPRs live at a time): the chunk
// order hi, mid, lo of K half 0, then of K half 1, so the split of one half is reused by its three
// chunks.  Weights: chunk 3q + p = part p (hi / mid / lo) of K half q.
struct PBF6 {
  static constexpr int KIND = K_BF16X6;
  using Acc = f32x16;     // one 32x32 accumulator tile
  static constexpr int SPW = 32;  // samples per wave
  static constexpr int CH = 6;
  static constexpr int E = 8;
  static constexpr int WAVES = 4;  // one wave per SIMD (16-VGPR fp32 tiles)
  static constexpr int ESIZE = 4;
  static constexpr int SPL = 8;
  static constexpr int PE = 2;  // PE_POLY: fp32-accurate to 1.6 ulp
  using Store = __bf16;
  struct Tile { float v[16]; };
  struct Split { bf16x8 h, m, l; };
  // K half q (registers 8q .. 8q + 7) as three bf16x8 parts
  static __device__ __forceinline__ Split split(const Tile& t, int q) {
    uint32_t hw[4], mw[4], lw[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float x0 = t.v[8 * q + 2 * k], x1 = t.v[8 * q + 2 * k + 1];
      hw[k] = pack_bf16(x0, x1);
      const float r0 = x0 - __uint_as_float(hw[k] << 16), r1 = x1 - __uint_as_float(hw[k] & 0xffff0000u);
      mw[k] = pack_bf16(r0, r1);
      lw[k] = pack_bf16(r0 - __uint_as_float(mw[k] << 16), r1 - __uint_as_float(mw[k] & 0xffff0000u));
    }
    return Split{__builtin_bit_cast(bf16x8, make_uint4(hw[0], hw[1], hw[2], hw[3])),
                 __builtin_bit_cast(bf16x8, make_uint4(mw[0], mw[1], mw[2], mw[3])),
                 __builtin_bit_cast(bf16x8, make_uint4(lw[0], lw[1], lw[2], lw[3]))};
  }
  static __device__ __forceinline__ f32x16 mma(uint4 a, const Tile& b, int c, f32x16 acc) {
    const bf16x8 av = __builtin_bit_cast(bf16x8, a);
    const int q = c / 3, p = c % 3;
    const Split x = split(b, q);  // (identical for the three chunks of a half: CSE'd)
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, x.h, acc, 0, 0, 0);
    if (p == 2) return acc;                                                  // lo . hi
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, x.m, acc, 0, 0, 0);   // . mid
    if (p == 1) return acc;
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, x.l, acc, 0, 0, 0);  // hi . lo
  }
  static __device__ __forceinline__ void set(Tile& t, int rho, float x) { t.v[rho] = x; }
  static __device__ __forceinline__ void pack16(Tile& t, const float (&v)[16]) {
#pragma unroll
    for (int rho = 0; rho < 16; ++rho) t.v[rho] = v[rho];
  }
  static __device__ __forceinline__ float get(const Tile& t, int rho) { return t.v[rho]; }
  static __host__ __device__ constexpr int rho_of(int c, int e) { return (c / 3) * E + e; }
  static __device__ __forceinline__ Store cvt_c(float x, int c) {
    const __bf16 h = (__bf16)x;
    const float r = x - (float)h;
    const __bf16 m = (__bf16)r;
    return c % 3 == 0 ? h : c % 3 == 1 ? m : (__bf16)(r - (float)m);
  }
  static __device__ __forceinline__ void set_pair(Tile& t, int k, float x0, float x1) {
    t.v[2 * k] = x0;
    t.v[2 * k + 1] = x1;
  }
};

// bf16x3 on v_mfma_f32_16x16x32_bf16 (round 6, the "wide" bf16x3 forward: 16 samples per wave, 8
// waves per workgroup = two per SIMD, so that one wave's epilogue runs beside the other's MFMAs).  The
// same arithmetic as PBF3 -- every fp32 operand split x = hi + lo, products hi*hi + hi*lo + lo*hi with
// fp32 accumulation -- on 16-row units (mlp_tables.h fwd16_*).  A chunk is 16 weight rows x one 32-feature
// K-block: chunk 0 the hi halves, chunk 1 the lo halves; a Tile is one K-block of the B operand (8 hi +
// 8 lo bf16 per lane, 8 VGPRs), the accumulator 4 fp32.  Forward only: the bf16x3 dX / dW and the bf16
// backward of bf16x3f read its training stores, which it writes in the 32x32 fragment layout.
struct PBF3W {
  static constexpr int KIND = K_BF16X3W;
  using Acc = f32x4;
  static constexpr int SPW = 16;
  static constexpr int CH = 2;
  static constexpr int E = 8;
  static constexpr int WAVES = 8;
  static constexpr int ESIZE = 4;
  static constexpr int SPL = 8;
  static constexpr int PE = 2;  // PE_POLY, as PBF3
  using Store = __bf16;
  struct Tile { bf16x8 hi, lo; };
  static __device__ __forceinline__ f32x4 mma(uint4 a, const Tile& b, int c, f32x4 acc) {
    const bf16x8 av = __builtin_bit_cast(bf16x8, a);
    if (c == 0) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b.hi, acc, 0, 0, 0);
      return __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b.lo, acc, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, b.hi, acc, 0, 0, 0);
  }
  static __host__ __device__ constexpr int rho_of(int, int e) { return e; }  // (a chunk reads the whole K-block)
  static __device__ __forceinline__ Store cvt_c(float x, int c) {
    const __bf16 h = (__bf16)x;
    return c == 0 ? h : (__bf16)(x - (float)h);
  }
  // packed weight element e of chunk c, lane group g: feature k16_feat(g, e) of the K-block, split part c
  static __host__ __device__ constexpr int feat16(int, int g, int e) { return k16_feat(g, e); }
  static __host__ __device__ constexpr int part16(int c) { return c; }
  // forward B operand: the feature of a K-block in register e of lane group g
  static __host__ __device__ constexpr int fwd_feat(int g, int e) { return k16_feat(g, e); }
};

// The wide fp32 TRAINING forward (round 6, PF32W): the PBF3W structure on v_mfma_f32_16x16x4_f32 -- one wave =
// 16 samples, 8 waves per workgroup, two per SIMD (the 32x32x2 fp32 forward holds 32 samples' fp32 tiles in
// ~450 registers: one wave per SIMD).  A K-block (32 features x 16 samples) is 8 MFMAs, and a 16x16 output tile
// mt (rows 4 g + e in lane group g) IS registers 4 (mt & 1) + e of the next layer's K-block mt >> 1.
//
// The FORWARD (round 7) sums in PF32's order and is bit-identical to it -- raw, stored activations, masks.  Both
// f32 MFMAs are a k-ordered fmaf chain (the 32x32x2 over its two lane halves, the 16x16x4 over its four lane
// groups), so MFMA j's B operand in lane (s, g) is feature f32w_feat(g, j) (mlp_tables.h): positions 4 j + g of
// PF32's K sequence 0,4,1,5,2,6,3,7, 8,12,...  The weight rows of a 16-row unit are permuted to match (f32w_row),
// which costs nothing: the kernel reads PF32's own forward pack (DIR 0, no second pack) and the permutation is
// which bytes a lane fetches.  PF32's 16-byte slot (row r, half h, chunk b) holds rho = 4b + 0, 2, 1, 3; lane
// (r16, g) needs rho 4b + (g >> 1) and 4b + 2 + (g >> 1) of half g & 1 for MFMAs 2b, 2b + 1: one aligned
// ds_read_b64 at 16 (32 (g & 1) + row) + 8 (g >> 1) of the chunk.  A step (t, c) is the four MFMAs 4c .. 4c + 3 =
// PF32's chunks 2c, 2c + 1.  (The two lane groups of a half-wave read the same 8 bytes of the slots of both
// halves h: a 2-way LDS bank conflict, 4 LDS cycles per read instead of 2 -- 16 cycles per 256 MFMA cycles and
// wave.  It is inherent in a 16-byte slot that PF32 reads whole)
//
// The wide dX keeps its own DIR 3 pack and K order, feat16 = 16 c + 4 g + e (it flips no ReLU branch).
// The training forward only -- renders keep the 32x32 PF32 kernels (a follow-up with its own measurement).
struct PF32W {
  static constexpr int KIND = K_F32W;
  using Acc = f32x4;
  static constexpr int SPW = 16;
  static constexpr int CH = 2;
  static constexpr int E = 4;
  static constexpr int WAVES = 8;
  static constexpr int ESIZE = 4;
  static constexpr int SPL = 4;
  static constexpr int PE = 1;  // PE_LIBM, as PF32
  using Store = float;
  struct Tile { float v[8]; };
  static __device__ __forceinline__ f32x4 mma(uint4 a, const Tile& b, int c, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), b.v[4 * c + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), b.v[4 * c + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), b.v[4 * c + 2], acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), b.v[4 * c + 3], acc, 0, 0, 0);
  }
  static __host__ __device__ constexpr int rho_of(int c, int e) { return 4 * c + e; }
  static __device__ __forceinline__ Store cvt_c(float x, int) { return x; }
  static __host__ __device__ constexpr int feat16(int c, int g, int e) { return 16 * c + 4 * g + e; }  // (the dX pack)
  static __host__ __device__ constexpr int part16(int) { return 0; }
  static __host__ __device__ constexpr int fwd_feat(int g, int e) { return f32w_feat(g, e); }  // (the forward: PF32's order)
};
// The wide bf16 dX (round 6, PBF16W): the bf16 dX of the bf16 and bf16x3f tiers on v_mfma_f32_16x16x32_bf16 over the
// 16-row W^T units -- PBF3W's layout with the hi half only (one 1 KiB chunk per K-block).
struct PBF16W {
  static constexpr int KIND = K_BF16W;
  using Acc = f32x4;
  static constexpr int SPW = 16;
  static constexpr int CH = 1;
  static constexpr int E = 8;
  static constexpr int WAVES = 8;
  static constexpr int ESIZE = 2;
  static constexpr int SPL = 8;
  static constexpr int PE = 0;
  using Store = __bf16;
  struct Tile { bf16x8 hi; };
  static __device__ __forceinline__ f32x4 mma(uint4 a, const Tile& b, int, f32x4 acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), b.hi, acc, 0, 0, 0);
  }
  static __host__ __device__ constexpr int rho_of(int, int e) { return e; }
  static __device__ __forceinline__ Store cvt_c(float x, int) { return (__bf16)x; }
  static __host__ __device__ constexpr int feat16(int, int g, int e) { return k16_feat(g, e); }
  static __host__ __device__ constexpr int part16(int) { return 0; }
};
template <class P> __host__ __device__ constexpr bool wide_kind() {
  return P::KIND == K_BF16X3W || P::KIND == K_F32W || P::KIND == K_BF16W;
}

// ReLU-mask bit of accumulator register rho of a tile: the tile's 16 bits sit at positions
// (rho >> 1) + 16 (rho & 1) of a dword (bf16 pair k = registers 2k, 2k+1 -> bits k, 16 + k),
// and two tiles n, n + 1 share one dword, the odd one shifted up by 8.
__host__ __device__ constexpr int mask_bit(int rho) { return (rho >> 1) + 16 * (rho & 1); }

typedef __attribute__((ext_vector_type(2))) short i16x2;
typedef __attribute__((ext_vector_type(2))) unsigned short u16x2;
// ReLU of a bf16 pair: sign-magnitude bf16 ordered as int16 -> v_pk_max_i16 with 0
// (relu(bf16(x)) == bf16(relu(x)): rounding keeps the sign)
__device__ __forceinline__ uint32_t relu_bf16x2(uint32_t d) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(i16x2, d), (i16x2){0, 0}));
}
// 1 in each half that is non-zero: v_pk_min_u16 with `one` = 0x00010001, which the caller holds in an
// SGPR laundered through an empty asm (no instruction) -- hipcc then emits the one v_pk_min_u16 itself;
// knowing the operand is 1 it rewrites min(x, 1) into a compare and a select per half.
// Round 6: this WAS an inline-asm v_pk_min_u16.  hipcc's hazard recognizer does not model the MFMA
// hazards of an inline-asm VGPR write: with finish parts 2 it allocated the asm's output to v1, a dead
// lane of the rgb unit's accumulator v[0:15] whose MFMA had issued one instruction earlier and still
// had its write of v[0:15] pending -- the MFMA's late write-back replaced the mask bits on some runs
// (the round-5 "masks differ run to run" finding; tools/mfma_war_scan.py: asm write 1 wait state after
// the MFMA, against >= 13 for every compiler-placed write).  No VGPR-writing inline asm is left in the
// MFMA kernels (tools/asm_check.py fails one).
__device__ __forceinline__ uint32_t nonzero_bf16x2(uint32_t d, uint32_t one) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, d), __builtin_bit_cast(u16x2, one)));
}
__device__ __forceinline__ uint32_t opaque_one16() {
  uint32_t one = 0x00010001u;
  asm("" : "+s"(one));
  return one;
}

template <class P> __host__ __device__ constexpr int samples_per_block() { return P::WAVES * P::SPW; }
inline constexpr int M_ALIGN = 256;  // activation stores are padded to this many samples

}  // namespace mlp
}  // namespace nerf
