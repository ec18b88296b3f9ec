// Fused NeRF MLP: the weight stream's groups, steps, finish parts and DMA spread, their compile-time
// proof (FinishSchedule) and the group runner (group_body).
#pragma once
#include "mlp_pack.h"

#include <type_traits>
#include <utility>

namespace nerf {
namespace mlp {

// ------------------------------------------------------------------------------------
// weight stream.  The packed units (one 32-row output tile of one layer, forward; one
// 32-row output tile of one dX stage, backward) are cut into GROUPS of consecutive units
// of one layer/stage that fit one LDS slot (<= SLOT_CAP KiB).  A 2-slot ring is filled by
// LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction) one group ahead, so a
// workgroup meets one barrier per group (4 hidden-layer units = 64 MFMAs per wave in
// bf16) instead of one per unit.
//
// The DMA is issued from inline asm, invisible to hipcc's waitcnt bookkeeping, and the
// group hand-off is a counted `s_waitcnt vmcnt(N)` + s_barrier where N = the vector-memory
// instructions this wave issued after the next group's DMA (the group's activation /
// gradient stores).  Loads, stores and LDS-DMA retire in issue order on one counter
// (MI355X_MICROARCH.md), so the wait covers the DMA and never the stores.  No
// compiler-visible global load may sit between a DMA and its wait (its compiler wait
// would drain the ring): all such loads are in the prologue.
// ------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void lds_void;

// every younger-than-N vector memory op of this wave may still be in flight; all LDS ops
// done; then the workgroup barrier.  "memory": no LDS/global access crosses it.
template <int N>
__device__ __forceinline__ void wait_barrier() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

// hand a loaded value to an empty asm right after a prologue wait: hipcc then places its
// own wait for the load there (already satisfied) instead of at the first use in the main
// loop, where it would also drain the in-flight weight DMA
__device__ __forceinline__ void settle(float& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void settle(uint32_t& x) { asm volatile("" : "+v"(x)); }

template <int... I, class F>
__device__ __forceinline__ void sfor_impl(std::integer_sequence<int, I...>, F&& f) {
  (f(std::integral_constant<int, I>{}), ...);
}
// compile-time unrolled loop: f(std::integral_constant<int, i>) for i in [0, N)
template <int N, class F>
__device__ __forceinline__ void sfor(F&& f) {
  sfor_impl(std::make_integer_sequence<int, N>{}, f);
}

__host__ __device__ constexpr int cmin(int a, int b) { return a < b ? a : b; }

// (a 3-slot ring of 48 KiB slots, DMA two groups ahead, measured slower everywhere in round 4:
// profiles/r4/pipeline_experiments.json)
constexpr int NSLOT = 2;       // ring slots; the DMA runs one group ahead
constexpr int SLOT_CAP = 72;   // KiB (1 KiB chunks) per slot: 144 KiB of the 160 KiB LDS
constexpr int PF = NSLOT - 1;
constexpr int GROUP_MAX = 8;   // units per group

struct Group { int u0, n, c0, nch; };  // first unit, units, first chunk, chunks

// DIR 0: forward units (DENSITY: trunk + alpha only, occupancy_grid.py:60 reads raw[...,3]);
// DIR 1: dX-chain units; DIR 2: 16-row forward units (PBF3W)
template <int DIR, bool DENSITY>
__host__ __device__ constexpr bool unit_used(int u) {
  return DIR == 1 || DIR == 3 || !DENSITY ||
         (DIR == 0 ? (u < fwd_unit_first(LFA) || u == fwd_unit_first(LFA) + 8)
                   : (u < fwd16_unit_first(LFA) || u == fwd16_unit_first(LFA) + 16));
}
template <int DIR> __host__ __device__ constexpr int unit_seg(int u) {
  return DIR == 0 ? fwd_unit_layer(u) : DIR == 1 ? bwd_unit_stage(u)
       : (DIR == 2 || DIR == DIR_F32W) ? fwd16_unit_layer(u) : bwd16_unit_stage(u);
}
template <int DIR> __host__ __device__ constexpr int unit_chunks(int u, int ch) {
  return DIR == 0 ? fwd_unit_chunks(u, ch) : DIR == 1 ? bwd_unit_chunks(u, ch)
       : DIR == 2 ? fwd16_unit_chunks(u, ch) : bwd16_unit_chunks(u, ch);
}
template <int DIR> __host__ __device__ constexpr int unit_chunk_off(int u, int ch) {
  return DIR == 0 ? fwd_unit_chunk_off(u, ch) : DIR == 1 ? bwd_unit_chunk_off(u, ch)
       : DIR == 2 ? fwd16_unit_chunk_off(u, ch) : bwd16_unit_chunk_off(u, ch);
}

// greedy grouping: consecutive used units of one segment while the slot has room
template <int DIR, bool DENSITY, int CH>
struct Groups {
  Group g[NUNIT_MAX];
  int n;
  __host__ __device__ constexpr Groups() : g(), n(0) {
    if (DIR == DIR_F32W) {
      // PF32's own groups (its pack, its slots, its chunk count), each 32-row unit as its one or two 16-row units
      const Groups<0, DENSITY, PF32::CH> T0{};
      for (int i = 0; i < T0.n; ++i) {
        Group G{f32w_unit16_first(T0.g[i].u0), 0, T0.g[i].c0, T0.g[i].nch};
        for (int j = 0; j < T0.g[i].n; ++j) G.n += f32w_unit16_count(T0.g[i].u0 + j);
        g[n++] = G;
      }
      return;
    }
    const int NU = num_units(DIR);
    int u = 0;
    while (u < NU) {
      if (!unit_used<DIR, DENSITY>(u)) {
        ++u;
        continue;
      }
      Group G{u, 0, unit_chunk_off<DIR>(u, CH), 0};
      const int seg = unit_seg<DIR>(u);
      while (u < NU && unit_used<DIR, DENSITY>(u) && (NERF_GROUP_ACROSS || unit_seg<DIR>(u) == seg) &&
             G.n < GROUP_MAX &&
             G.nch + unit_chunks<DIR>(u, CH) <= SLOT_CAP) {
        G.nch += unit_chunks<DIR>(u, CH);
        ++G.n;
        ++u;
      }
      g[n++] = G;
    }
  }
};
template <int DIR, bool DENSITY, int CH>
struct GroupTable {
  static constexpr Groups<DIR, DENSITY, CH> t{};
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const u32x4 lds_cu4;
__device__ __forceinline__ uint4 as_uint4(u32x4 v) { return make_uint4(v.x, v.y, v.z, v.w); }

// per-lane LDS base of a unit's chunks (lane-linear: + 16 lane bytes), laundered through
// an empty asm: every read of the unit is then this one VGPR + an immediate offset
// (< 64 KiB).  Left visible, hipcc materialises one address VGPR per distinct chunk offset
// of both ring slots and keeps them all live across the unrolled kernel.
__device__ __forceinline__ lds_cu4* lds_ptr(uint32_t byte_addr) {
  settle(byte_addr);
  return (lds_cu4*)(uintptr_t)byte_addr;
}

// The MFMA steps of a group as one flat compile-time list: step k = (unit j of the group,
// input tile t, chunk c), in execution order.  A group's body is straight-line code over
// it with the A operand (weights, LDS) prefetched PD steps ahead across unit boundaries
// -- hipcc on its own keeps one ds_read in flight and waits lgkmcnt(0) before every MFMA.

// DMA wave-instructions (1 KiB global_load_lds each) per wave for group g (fetch_group_lean)
template <class P, int DIR, bool DENSITY>
__host__ __device__ constexpr int group_dma_units(int g) {
  return (GroupTable<DIR, DENSITY, P::CH>::t.g[g].nch + P::WAVES - 1) / P::WAVES;
}
template <class P, int DIR, bool DENSITY>
__host__ __device__ constexpr int group_dma(int g) {
  return group_dma_units<P, DIR, DENSITY>(g);
}
// vmcnt of the hand-off at the end of group g (group g + 1's DMA must have landed): the
// wave's vector-memory ops younger than that DMA = the DMAs of groups g + 2 .. g + PF and
// the stores of the iterations g + 1 - PF .. g (each issued after its iteration's DMA), plus
// the prologue's stores when group g + 1 was fetched in the prologue.
template <class P, int DIR, bool DENSITY, class StoresFn>
__host__ __device__ constexpr int handoff_vmcnt(int g, StoresFn stores, int prologue_stores) {
  const int NG = GroupTable<DIR, DENSITY, P::CH>::t.n;
  int n = 0;
  for (int j = g + 2; j <= g + PF && j < NG; ++j) n += group_dma<P, DIR, DENSITY>(j);
  for (int i = (g + 1 - PF > 0 ? g + 1 - PF : 0); i <= g; ++i) n += stores(i);
  if (g + 1 < PF) n += prologue_stores;
  return n;
}

struct Step { int j, u, t, c, off, kin, len; bool first, last; };
template <int DIR> __host__ __device__ constexpr int unit_tiles(int u) {
  return DIR == 0 ? fwd_unit_tiles(u) : DIR == 1 ? bwd_unit_tiles(u)
       : (DIR == 2 || DIR == DIR_F32W) ? fwd16_unit_tiles(u) : bwd16_unit_tiles(u);
}
template <int DIR, bool DENSITY, int CH>
__host__ __device__ constexpr int group_steps(int g) {
  const Group G = GroupTable<DIR, DENSITY, CH>::t.g[g];
  int n = 0;
  for (int j = 0; j < G.n; ++j) n += unit_tiles<DIR>(G.u0 + j) * CH;
  return n;
}
template <int DIR, bool DENSITY, int CH>
__host__ __device__ constexpr Step group_step(int g, int k) {
  const Group G = GroupTable<DIR, DENSITY, CH>::t.g[g];
  for (int j = 0; j < G.n; ++j) {
    const int u = G.u0 + j, n = unit_tiles<DIR>(u) * CH;
    if (k < n) {
      const int t = k / CH, c = k % CH;
      if (DIR == DIR_F32W) {
        // off in 256-byte units: PF32's chunks 2c, 2c + 1 of tile t of the 32-row unit, + 256 B for its upper 16 rows
        const int u32 = f32w_unit32(u), hi = (u - fwd16_unit_first(fwd16_unit_layer(u))) & 1;
        const int ch = fwd_unit_chunk_off(u32, PF32::CH) - G.c0 + PF32::CH * t + 2 * c;
        return Step{j, u, t, c, 4 * ch + hi, k, n, k == 0, k == n - 1};
      }
      return Step{j, u, t, c, unit_chunk_off<DIR>(u, CH) - G.c0 + k, k, n, k == 0, k == n - 1};
    }
    k -= n;
  }
  return Step{-1, -1, 0, 0, 0, 0, 0, false, false};
}
// A-operand prefetch distance in steps and the finish delay (mlp_knobs.h: NERF_PREFETCH_*, NERF_FINISH_DELAY*)
template <class P> __host__ __device__ constexpr int prefetch_depth() {
  return P::KIND == K_F32 ? NERF_PREFETCH_F32 : P::KIND == K_F32W ? NERF_PREFETCH_F32W : NERF_PREFETCH_BF16;  // a bf16 / bf16x3 step is 1-2 short MFMAs
}
constexpr int FINISH_DELAY = NERF_FINISH_DELAY;

// Cross-group finish: the last unit of a group is finished after the barrier.  Not in the
// bf16x3 forward: a finished accumulator carried over the barrier (plus the hi / lo split of
// the finish) takes it past 512 VGPRs (139 spilled); finished in-group it needs none.
// (r5: with the lean DMA and packed masks the bf16x3 forward fits cross-group finish without spills, 372
// VGPRs, but it is not faster: bf16x3f training forward 1.609 vs 1.599 ms)
template <class P, int DIR> __host__ __device__ constexpr bool cross_finish() {
  return !(P::KIND == K_BF16X3 && DIR == 0);
}
// the unit finished inside group g: (first, last] = units whose finish is issued in g.
// With cross_finish() the last unit of a group is finished FINISH_DELAY steps into the
// next group (after the barrier), so no group ends in a VALU burst that every wave of the
// workgroup runs at once; its stores then count against the next group's hand-off.
template <int DIR, bool DENSITY, int CH, bool CROSS>
__host__ __device__ constexpr bool finished_in_group(int g, int u) {
  const auto& T = GroupTable<DIR, DENSITY, CH>::t;
  const Group G = T.g[g];
  const int last = G.u0 + G.n - 1;
  if (!CROSS) return u >= G.u0 && u <= last;
  const bool prev = g > 0 && u == T.g[g - 1].u0 + T.g[g - 1].n - 1;
  return prev || (u >= G.u0 && (u < last || (u == last && g + 1 == T.n)));
}

// Finish parts.  A unit's epilogue (ReLU, mask bits, pack / hi-lo split, stores: ~60-110
// instructions) issued as one run stalls the matrix pipe of a one-wave-per-SIMD kernel (fp32,
// bf16x3) for the whole run: nothing else feeds it (the gfx950 assembly of the bf16x3
// training forward had 70 % of its non-MFMA instructions in 138 runs of > 20 between two
// MFMAs).  With NP parts, part p (register pairs [8p/NP, 8(p+1)/NP)) is issued FINISH_DELAY + p
// steps into the next unit, clamped to that unit's last step; the last part stores.
// Any value is checked at compile time: FinishSchedule (below) static_asserts that no MFMA reads a tile pair
// before the part that writes it.  (Round 5 saw NERF_FINISH_PARTS_BF16 = 2 / 8 write masks / dZ that differed
// run to run.  Parts 8 is that clamping hazard and no longer compiles; parts 2 was an inline-asm VGPR write
// racing an MFMA write-back (nonzero_bf16x2), fixed for every placement.  Round 6, tools/race_diag.py,
// profiles/r6/race_diag_*.json: bf16 parts 2 / 4 and bf16x3 parts 4 / 8 bit-identical, run to run and to
// each other.)
template <class P> __host__ __device__ constexpr int finish_parts() {
  return P::KIND == K_F32 ? NERF_FINISH_PARTS_F32 : P::KIND == K_BF16 ? NERF_FINISH_PARTS_BF16
       : P::KIND == K_BF16X3W ? NERF_FINISH_PARTS_BF3W : P::KIND == K_F32W ? NERF_FINISH_PARTS_F32W
       : P::KIND == K_BF16W ? NERF_FINISH_PARTS_BF16W : NERF_FINISH_PARTS_BF3;
}
// DMA spread.  0: the next group's LDS-DMA pieces (up to 18 per wave, ~7 instructions each)
// are issued as one burst at the group's start; S > 0: piece i at step i (NS / S) / NF of the
// group's NS steps, i.e. inside the first 1/S of the group (they must land before its end).
template <class P> __host__ __device__ constexpr int dma_spread() {
  return PF != 1 ? 0 : P::KIND == K_F32 ? NERF_DMA_SPREAD_F32 : P::KIND == K_BF16 ? NERF_DMA_SPREAD_BF16
       : P::KIND == K_BF16X3W ? NERF_DMA_SPREAD_BF3W : P::KIND == K_F32W ? NERF_DMA_SPREAD_F32W
       : P::KIND == K_BF16W ? NERF_DMA_SPREAD_BF16W : NERF_DMA_SPREAD_BF3;
}

// step (in group g) at which part p of unit u's finish is issued, or -1 when u is not
// finished in g
template <class P, int DIR, bool DENSITY>
__host__ __device__ constexpr int part_step(int g, int u, int p) {
  const auto& T = GroupTable<DIR, DENSITY, P::CH>::t;
  const Group G = T.g[g];
  if (!finished_in_group<DIR, DENSITY, P::CH, cross_finish<P, DIR>()>(g, u)) return -1;
  const int NS = group_steps<DIR, DENSITY, P::CH>(g);
  if (u == G.u0 + G.n - 1) return NS - 1;  // the group's last unit, finished in-group: at its last step
  const int js = u < G.u0 ? 0 : u - G.u0 + 1;  // the unit after u (this group's first, or u + 1)
  int start = 0;
  for (int j = 0; j < js; ++j) start += unit_tiles<DIR>(G.u0 + j) * P::CH;
  const int len = unit_tiles<DIR>(G.u0 + js) * P::CH;
  const int d = (P::KIND == K_BF16W ? NERF_FINISH_DELAY_BF16W : FINISH_DELAY) + p;
  return start + (d < len - 1 ? d : len - 1);
}
// step (in group g) of the i-th of the next group's NF DMA pieces (dma_spread > 0)
template <class P, int DIR, bool DENSITY>
__host__ __device__ constexpr int dma_piece_step(int g, int i) {
  const int NS = group_steps<DIR, DENSITY, P::CH>(g);
  const int NF = group_dma_units<P, DIR, DENSITY>(g + 1);
  const int S = dma_spread<P>() > 0 ? dma_spread<P>() : 1;  // (instantiated, never evaluated, for a spread of 0)
  const int front = (NS + S - 1) / S;
  return i * front / NF;
}
// vmcnt of the hand-off at the end of group g when the next group's DMA is spread over
// group g: the stores issued at or after the step of its last piece (a step issues its DMA
// pieces first, then its MFMAs, then any finish parts)
template <class P, int DIR, bool DENSITY, class StoresFn>
__host__ __device__ constexpr int handoff_vmcnt_spread(int g, StoresFn unit_stores) {
  if (g + 1 >= GroupTable<DIR, DENSITY, P::CH>::t.n) return 0;  // (the last group: no hand-off)
  const int last = dma_piece_step<P, DIR, DENSITY>(g, group_dma_units<P, DIR, DENSITY>(g + 1) - 1);
  const int NU = num_units(DIR);
  int n = 0;
  for (int u = 0; u < NU; ++u) {
    const int s = part_step<P, DIR, DENSITY>(g, u, finish_parts<P>() - 1);
    if (s >= last) n += unit_stores(u);
  }
  return n;
}

// ------------------------------------------------------------------------------------
// Register tile slots and the finish-schedule check (r6).
//
// A wave's B-operand tiles live in registers: the activation / gradient ping-pong arrays Ha[0..7]
// and Hb[0..7], the encodings X[0..1] and D (forward) and the output-gradient seeds G and DA (dX).
// Every unit reads its input tiles from slots and its finish parts write its output tile, pair by
// pair, IN PLACE into a slot -- which the next layer's first unit reads.  The two tables below
// are the kernels' own (FwdWave::in_tile / DxWave::in_tile and the finishes go through them), so
// the schedule model below checks the code that runs.
//
// The race found in round 5 (bf16 finish parts 2 / 8: masks / dZ that differed between two runs
// of one launch) is this hand-off.  A finish part is issued FINISH_DELAY + p steps into the next
// unit, CLAMPED to that unit's last step, and within a step the finish runs after the MFMA.
// Where the next unit has few input tiles -- LRGB after LV (4 tiles), the dX stage bV after
// bRGB (4 tiles) -- eight parts land at steps 3..7 of an 8-step unit, and the parts writing
// pairs 3..7 of tile 3 come after the MFMAs that read them (steps 6 and 7).  Those MFMAs read the
// slot's OLD registers: in the forward the previous layer's values (deterministic, wrong), in the
// dX chain Hb[3] before its first write (uninitialised registers: different on every run).  The
// ISA-level hand-off check could not see it: it is a register dependence the program order
// itself gets wrong, not a memory-counter one.  finish_schedule_ok() below simulates every
// group's steps and fails the build of any placement where an MFMA reads a pair before its
// producer's part (or a later producer's part overwrites it first), or a part reads `pend` after
// it was reassigned.
// ------------------------------------------------------------------------------------
enum TileSlot { TS_HA = 0, TS_HB = 8, TS_X = 16, TS_D = 18, TS_G = 19, TS_DA = 20, TS_NONE = -1 };
__host__ __device__ constexpr bool finish_slot(int s) { return s >= TS_HA && s < TS_X; }  // written by finishes
// forward layer L: input tile t, output tile n
__host__ __device__ constexpr int fwd_in_slot(int L, int t) {
  return L == L0 ? TS_X + t
       : L == L5 ? (t < 2 ? TS_X + t : TS_HA + t - 2)
       : L == LV ? (t < 8 ? TS_HA + t : (int)TS_D)
       : L == LRGB ? TS_HB + t
       : (L == L1 || L == L3 || L == L7) ? TS_HA + t
       : TS_HB + t;  // L2, L4, L6, LFA
}
__host__ __device__ constexpr int fwd_out_slot(int L, int n) {
  return L == LRGB || (L == LFA && n == 8) ? (int)TS_NONE  // (rgb / alpha: scalars)
       : (L == L0 || L == L2 || L == L4 || L == L6 || L == LFA) ? TS_HA + n
       : TS_HB + n;  // L1, L3, L5, L7, LV
}
// dX stage s: input tile t, output tile j
__host__ __device__ constexpr int bwd_in_slot(int s, int t) {
  return s == B_RGB ? (int)TS_G
       : s == B_V ? TS_HB + t
       : s == B_FA ? (t < 8 ? TS_HA + t : (int)TS_DA)
       : (s == B_7 || s == B_5 || s == B_3 || s == B_1) ? TS_HB + t
       : TS_HA + t;  // B_6, B_4, B_2
}
__host__ __device__ constexpr int bwd_out_slot(int s, int j) {
  return (s == B_RGB || s == B_FA || s == B_6 || s == B_4 || s == B_2) ? TS_HB + j : TS_HA + j;
}
template <int DIR> __host__ __device__ constexpr int unit_in_slot(int u, int t) {
  return DIR == 0 ? fwd_in_slot(fwd_unit_layer(u), t)
       : DIR == 1 ? bwd_in_slot(bwd_unit_stage(u), t)
       : (DIR == 2 || DIR == DIR_F32W) ? fwd_in_slot(fwd16_unit_layer(u), t)
       : bwd_in_slot(bwd16_unit_stage(u), t);
}
// 16-row unit (DIR 2): output tile m fills half m & 1 (elements 4 (m & 1) .. + 3) of K-block slot m >> 1
template <int DIR> __host__ __device__ constexpr int unit_out_slot(int u) {
  return DIR == 0 ? fwd_out_slot(fwd_unit_layer(u), u - fwd_unit_first(fwd_unit_layer(u)))
       : DIR == 1 ? bwd_out_slot(bwd_unit_stage(u), u - bwd_unit_first(bwd_unit_stage(u)))
       : (DIR == 2 || DIR == DIR_F32W) ? fwd_out_slot(fwd16_unit_layer(u), (u - fwd16_unit_first(fwd16_unit_layer(u))) >> 1)
       : bwd_out_slot(bwd16_unit_stage(u), (u - bwd16_unit_first(bwd16_unit_stage(u))) >> 1);
}
// the register pairs of its slot a unit's finish writes (a 32x32 tile: all 8; a 16-row unit: 2 of a K-block's 4)
template <int DIR> __host__ __device__ constexpr int unit_out_pairs(int u) {
  return (DIR == 2 || DIR == DIR_F32W) ? (((u - fwd16_unit_first(fwd16_unit_layer(u))) & 1) ? 0xC : 0x3)
       : DIR == 3 ? (((u - bwd16_unit_first(bwd16_unit_stage(u))) & 1) ? 0xC : 0x3) : 0xFF;
}
// register pairs (bit k = registers 2k, 2k + 1) of a tile that MFMA chunk c reads / finish part p writes
template <class P> __host__ __device__ constexpr int chunk_pairs(int c) {
  int m = 0;
  for (int e = 0; e < P::E; ++e) {
    const int rho = P::rho_of(c, e);
    if (rho < 16) m |= 1 << (rho >> 1);
  }
  return m;
}
// pairs of an output tile: 8 (32x32 accumulator, 16 registers), 2 (16x16, 4 registers)
template <class P> __host__ __device__ constexpr int tile_pairs() { return wide_kind<P>() ? 2 : 8; }
template <class P> __host__ __device__ constexpr int part_pairs(int p) {
  constexpr int NP = finish_parts<P>(), TP = tile_pairs<P>();
  int m = 0;
  for (int k = TP * p / NP; k < TP * (p + 1) / NP; ++k) m |= 1 << k;
  return m;
}
// the pairs of its slot part p of unit u writes
template <class P, int DIR> __host__ __device__ constexpr int part_write_pairs(int u, int p) {
  return DIR < 2 ? part_pairs<P>(p) : part_pairs<P>(p) << (unit_out_pairs<DIR>(u) == 0xC ? 2 : 0);
}
// Positions in the straight-line schedule: 4 * (global step) + phase, the phases of one step in
// group_body's order: 0 DMA pieces, 1 pend / init + MFMA, 2 the previous unit's finish parts, 3 the
// group's last unit (finished in-group, or parked in `pend` for the next group).
// finish_schedule_violation() is 0 when the schedule is sound; else a code naming the first
// violation: 1 an MFMA reads a pair before its producer's part writes it (or reads a slot no unit
// wrote), 2 a later producer's part overwrites the pair before the read, 3 a part reads `pend`
// after it was reassigned, 4 a finish part is never issued.
template <class P, int DIR, bool DENSITY>
struct FinishSchedule {
  static constexpr int NU = num_units(DIR);
  static constexpr int NP = finish_parts<P>();
  int pos[NUNIT_MAX][8];   // position of part p of unit u (-1: none)
  int pend_at[NUNIT_MAX];  // position at which `pend` takes unit u (-1)
  int violation;
  __host__ __device__ constexpr FinishSchedule() : pos(), pend_at(), violation(0) {
    const auto& T = GroupTable<DIR, DENSITY, P::CH>::t;
    for (int u = 0; u < NU; ++u) {
      pend_at[u] = -1;
      for (int p = 0; p < 8; ++p) pos[u][p] = -1;
    }
    int base = 0;
    for (int g = 0; g < T.n; ++g) {
      const Group G = T.g[g];
      const int NS = group_steps<DIR, DENSITY, P::CH>(g);
      const int last = G.u0 + G.n - 1;
      // units finished in g: the previous group's last unit (cross-group finish) and G's own
      for (int u = (g > 0 ? T.g[g - 1].u0 + T.g[g - 1].n - 1 : G.u0); u <= last; ++u)
        for (int p = 0; p < NP; ++p) {
          const int st = part_step<P, DIR, DENSITY>(g, u, p);
          if (st >= 0) pos[u][p] = 4 * (base + st) + (u == last ? 3 : 2);
        }
      for (int j = 1, k = unit_tiles<DIR>(G.u0) * P::CH; j < G.n; k += unit_tiles<DIR>(G.u0 + j) * P::CH, ++j)
        pend_at[G.u0 + j - 1] = 4 * (base + k) + 1;  // (the first step of unit j)
      if (!finished_in_group<DIR, DENSITY, P::CH, cross_finish<P, DIR>()>(g, last)) pend_at[last] = 4 * (base + NS - 1) + 3;
      base += NS;
    }
    violation = check();
  }
  __host__ __device__ constexpr int check() const {
    const auto& T = GroupTable<DIR, DENSITY, P::CH>::t;
    int out[NUNIT_MAX] = {}, opairs[NUNIT_MAX] = {}, pw[NUNIT_MAX][8] = {}, next_w[NUNIT_MAX][8] = {};
    int ntiles[NUNIT_MAX] = {}, in_slot[NUNIT_MAX][10] = {};  // (precomputed: the unit walks are loops)
    for (int u = 0; u < NU; ++u) {
      ntiles[u] = unit_tiles<DIR>(u);
      for (int t = 0; t < ntiles[u]; ++t) in_slot[u][t] = unit_in_slot<DIR>(u, t);
      out[u] = unit_used<DIR, DENSITY>(u) ? unit_out_slot<DIR>(u) : (int)TS_NONE;
      opairs[u] = finish_slot(out[u]) ? unit_out_pairs<DIR>(u) : 0;
      for (int p = 0; p < NP; ++p) pw[u][p] = part_write_pairs<P, DIR>(u, p);
    }
    {  // next_w[u][q]: the next unit after u that writes pair q of u's slot (-1: none)
      int seen[TS_X][8] = {};
      for (int sl = 0; sl < TS_X; ++sl)
        for (int q = 0; q < 8; ++q) seen[sl][q] = -1;
      for (int u = NU - 1; u >= 0; --u)
        for (int q = 0; q < 8; ++q) {
          next_w[u][q] = -1;
          if ((opairs[u] >> q) & 1) {
            next_w[u][q] = seen[out[u]][q];
            seen[out[u]][q] = u;
          }
        }
    }
    for (int u = 0; u < NU; ++u) {
      if (!unit_used<DIR, DENSITY>(u)) continue;
      for (int p = 0; p < NP; ++p) {
        if (pos[u][p] < 0) return 4;
        if ((pos[u][p] & 3) == 3) continue;  // finished in-group from `acc`
        // `pend` holds u from pend_at[u] until the next unit's assignment
        if (pend_at[u] < 0 || pend_at[u] >= pos[u][p]) return 3;
        for (int v = u + 1; v < NU; ++v)
          if (pend_at[v] >= 0 && pend_at[v] < pos[u][p]) return 3;
      }
    }
    // writer[slot][pair]: the last unit (in unit order, before the reading unit) that writes the pair
    int writer[TS_X][8] = {};
    for (int sl = 0; sl < TS_X; ++sl)
      for (int q = 0; q < 8; ++q) writer[sl][q] = -1;
    int base = 0, done = 0;  // (writer holds the units < done, in unit order)
    for (int g = 0; g < T.n; ++g) {
      const Group G = T.g[g];
      for (int j = 0; j < G.n; ++j) {
        const int u = G.u0 + j;
        for (; done < u; ++done)
          for (int q = 0; q < 8; ++q)
            if ((opairs[done] >> q) & 1) writer[out[done]][q] = done;
        const int nt = ntiles[u];
        for (int t = 0; t < nt; ++t) {
          const int slot = in_slot[u][t];
          if (!finish_slot(slot)) {
            base += P::CH;
            continue;
          }
          for (int c = 0; c < P::CH; ++c, ++base) {
            const int rpos = 4 * base + 1, cp = chunk_pairs<P>(c);
            for (int q = 0; q < 8; ++q) {
              if (!((cp >> q) & 1)) continue;
              const int prod = writer[slot][q];
              if (prod < 0) return 1;
              const int nv = next_w[prod][q];
              for (int p = 0; p < NP; ++p) {
                if (((pw[prod][p] >> q) & 1) && pos[prod][p] >= rpos) return 1;
                // the next unit writing the pair must not write it before this read
                if (nv >= 0 && ((pw[nv][p] >> q) & 1) && pos[nv][p] >= 0 && pos[nv][p] < rpos) return 2;
              }
            }
          }
        }
      }
    }
    return 0;
  }
};
// (PF32W's 16-row forward units, DIR 2, run over PF32's pack: their groups and steps are DIR 4's)
template <class P, int DIR> __host__ __device__ constexpr int sched_dir() {
  return P::KIND == K_F32W && DIR == 2 ? DIR_F32W : DIR;
}
template <class P, int DIR, bool DENSITY> __host__ __device__ constexpr int finish_schedule_violation() {
  return FinishSchedule<P, sched_dir<P, DIR>(), DENSITY>{}.violation;
}

// the A operand of one step from the current slot (wl: this lane's base in it; OFF: Step::off).  DIR 4: the 8 bytes
// of this lane's half of two of PF32's 16-byte slots, chunks 2c and 2c + 1 (OFF in 256-byte units)
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// (Relaxed wavefront-scope atomic loads: two plain ds_read_b64, 2 LDS cycles each on 64 banks, 4 with this layout's
// 2-way conflict, and no memory-model wait behind them.  Plain loads hipcc pairs into ds_read2st64_b64 /
// ds_read2_b64, which bank on 32 and take twice the LDS cycles; volatile ones it follows with lgkmcnt(0) each,
// which undoes the prefetch.)
typedef __attribute__((address_space(3))) uint64_t lds_u64;
template <int DIR, int OFF>
__device__ __forceinline__ uint4 load_a(lds_cu4* wl) {
  if constexpr (DIR == DIR_F32W) {
    lds_u64* p = (lds_u64*)wl;
    const uint64_t lo = __hip_atomic_load(p + OFF * 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    const uint64_t hi = __hip_atomic_load(p + OFF * 32 + 128, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
  } else {
    return as_uint4(wl[OFF * 64]);
  }
}

// W: the wave object; it provides in_tile<u, t>(), prefetch<u>() (issue unit u's side
// reads one unit ahead), init<u>(acc) (initial accumulator), finish_part<u, p>(acc),
// fetch_piece<g, i>() (the i-th DMA piece of group g) and a pending accumulator `pend` that
// carries a finished chain to its deferred finish
template <class P, int DIR, bool DENSITY, int g, class W>
__device__ __forceinline__ void group_body(W& w, lds_cu4* wl) {
  constexpr int NS = group_steps<DIR, DENSITY, P::CH>(g);
  constexpr int PDP = prefetch_depth<P>();
  constexpr int NP = finish_parts<P>();
  constexpr auto& T = GroupTable<DIR, DENSITY, P::CH>::t;
  constexpr Group G = T.g[g];
  constexpr int PREV_U = g > 0 ? T.g[g - 1].u0 + T.g[g - 1].n - 1 : -1;  // previous group's last unit
  constexpr bool SPREAD = dma_spread<P>() > 0 && g + 1 < T.n;
  constexpr int NF = SPREAD ? group_dma_units<P, DIR, DENSITY>(g + 1) : 0;
  uint4 ring[PDP];
  sfor<(NS < PDP ? NS : PDP)>([&](auto kk) {
    constexpr int k = decltype(kk)::value;
    constexpr Step S = group_step<DIR, DENSITY, P::CH>(g, k);
    ring[k] = load_a<DIR, S.off>(wl);
  });
  w.template prefetch<G.u0>();
  typename P::Acc acc;
  sfor<NS>([&](auto kk) {
    constexpr int k = decltype(kk)::value;
    constexpr Step S = group_step<DIR, DENSITY, P::CH>(g, k);
    if constexpr (SPREAD) {
      sfor<NF>([&](auto ii) {
        if constexpr (dma_piece_step<P, DIR, DENSITY>(g, decltype(ii)::value) == k)
          w.template fetch_piece<g + 1, decltype(ii)::value>();
      });
    }
    const uint4 a = ring[k % PDP];
    if constexpr (k + PDP < NS) {
      constexpr Step N = group_step<DIR, DENSITY, P::CH>(g, k + PDP);
      ring[k % PDP] = load_a<DIR, N.off>(wl);
    }
    // (PF32W forward, 240 of its 256 VGPRs: hipcc sinks each prefetched read to just before its MFMAs and waits
    // lgkmcnt(0) there.  No MFMA or LDS read may cross this point -- 0x276: VALU, SALU, VMEM, LDS writes may --
    // so the reads of step k + PDP are in flight over the MFMAs of step k.)
    if constexpr (DIR == DIR_F32W) __builtin_amdgcn_sched_barrier(0x276);
    if constexpr (S.first) {
      if constexpr (S.j > 0) w.pend = acc;
      w.template init<S.u>(acc);
      if constexpr (S.j + 1 < G.n) w.template prefetch<S.u + 1>();
    }
    acc = P::mma(a, w.template in_tile<S.u, S.t>(), S.c, acc);
    constexpr int U_BEFORE = S.j > 0 ? S.u - 1 : PREV_U;
    if constexpr (U_BEFORE >= 0) {
      sfor<NP>([&](auto pp) {
        if constexpr (part_step<P, DIR, DENSITY>(g, U_BEFORE, decltype(pp)::value) == k)
          w.template finish_part<U_BEFORE, decltype(pp)::value>(w.pend);
      });
    }
    if constexpr (S.last && S.j == G.n - 1) {
      if constexpr (finished_in_group<DIR, DENSITY, P::CH, cross_finish<P, DIR>()>(g, S.u))
        sfor<NP>([&](auto pp) { w.template finish_part<S.u, decltype(pp)::value>(acc); });
      else w.pend = acc;
    }
  });
}

}  // namespace mlp
}  // namespace nerf
