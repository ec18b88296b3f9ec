// Fused NeRF MLP: the LDS-DMA pieces of the weight ring.
#pragma once
#include "mlp_schedule.h"

namespace nerf {
namespace mlp {

// DMA piece I of a wave for a group of NCH chunks starting at chunk C0 into the slot at SLOT_OFF: every wave
// issues exactly group_dma_units pieces (the last chunk is re-copied by the surplus waves -- identical bytes),
// so the count a later wait needs is a compile-time constant.
//
// The lean form (the only one; the earlier piece saved and restored M0 and computed a 64-bit address per
// lane).  Wave w's piece I is chunk w + WAVES I, so with the per-lane VGPR vlane = 16 lane + 1024 w and the wave-uniform swave = LDS base + 1024 w held for the
// whole kernel, the piece's global offset and LDS address are those plus compile-time constants:
// `s_add_u32 m0` (the LDS destination), `s_nop 0` (the wait state an M0 write needs before an
// LDS-DMA) and the DMA in the SADDR form on the packed-weight base; the per-lane offset vlane + GOFF is
// a v_add_u32 that hipcc places itself (4 instructions per piece; round 5 put the v_add_u32 inside
// the asm, as the m0 wait state, for 3).  Round 6: no VGPR is written inside inline asm any more --
// hipcc's hazard recognizer does not cover an asm VGPR write that lands on a register an in-flight
// MFMA still writes or reads as SrcC (the mask race, nonzero_bf16x2 in mlp_policy.h); a compiler-placed
// v_add_u32 gets its wait states.  M0 is not saved: no compiler code of these kernels touches it
// (tools/asm_check.py checks the emitted code; M0 is a reserved register, so clang ignores it in a
// clobber list -- "-Winline-asm: reserved registers on the clobber list may not be preserved").  s_add_u32 writes SCC: declared
// clobbered too (without it hipcc kept a comparison in SCC across the statement and the last group's
// surplus-wave selection went wrong -- the rgb bias chunk was never copied).  A surplus wave of the
// last piece (w + WAVES I > NCH - 1) re-copies its previous piece instead: the same bytes to the same
// place.
struct DmaLean {
  const void* gbase;  // packed weights (kernel argument: SGPR pair)
  uint32_t vlane;     // 16 lane + 1024 wave
  uint32_t swave;     // LDS byte address of the ring + 1024 wave (wave-uniform)
  uint32_t wave_u;    // wave (wave-uniform)
};
template <class P, int C0, int NCH, int SLOT_OFF, int I>
__device__ __forceinline__ void fetch_piece_lean(const DmaLean& d) {
  if constexpr (NERF_DIAG_NO_DMA) return;
  constexpr int NU = (NCH + P::WAVES - 1) / P::WAVES;
  constexpr uint32_t GOFF = (uint32_t)(C0 + P::WAVES * I) * 1024u, LOFF = (uint32_t)(SLOT_OFF + P::WAVES * I * 1024);
  static_assert(NCH % P::WAVES == 0 || NU >= 2, "a one-piece group with surplus waves");
  if constexpr (I + 1 < NU || NCH % P::WAVES == 0) {
    const uint32_t voff = d.vlane + GOFF;
    asm volatile("s_add_u32 m0, %1, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %3"
                 :: "v"(voff), "s"(d.swave), "i"(LOFF), "s"(d.gbase) : "memory", "scc");
  } else {
    const uint32_t adj = d.wave_u + P::WAVES * I > (uint32_t)(NCH - 1) ? (uint32_t)P::WAVES * 1024u : 0u;
    const uint32_t voff = d.vlane + (GOFF - adj);
    asm volatile("s_add_u32 m0, %1, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %3"
                 :: "v"(voff), "s"(d.swave - adj), "i"(LOFF), "s"(d.gbase) : "memory", "scc");
  }
}
// issue the whole DMA of a group (group_dma_units pieces per wave)
template <class P, int C0, int NCH, int SLOT_OFF>
__device__ __forceinline__ void fetch_group_lean(const DmaLean& d) {
  constexpr int NU = (NCH + P::WAVES - 1) / P::WAVES;
  sfor<NU>([&](auto ii) { fetch_piece_lean<P, C0, NCH, SLOT_OFF, decltype(ii)::value>(d); });
}

}  // namespace mlp
}  // namespace nerf
