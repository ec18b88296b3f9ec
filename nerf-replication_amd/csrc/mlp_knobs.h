// Fused NeRF MLP: every -DNERF_* build knob of the MLP kernels, its default and what was measured at it, and the
// knob policy that says which of them may be set at all.  Included first by every mlp_*.h header.
//
// Knob policy (round 6).  Schedule knobs -- NERF_FINISH_PARTS_*, NERF_FINISH_DELAY*, NERF_PREFETCH_*,
// NERF_DMA_SPREAD_*, NERF_GROUP_ACROSS -- may take any value: every placement they produce is proven at compile
// time (FinishSchedule's static_assert in FwdWave / FwdWave16 / DxWave / DxWave16; the hand-off vmcnt counts are
// computed from the same tables and tools/asm_check.py checks them on the emitted code).  The kernel selectors
// NERF_BF3_WIDE, NERF_F32_WIDE and NERF_*_WIDE_DX choose between verified kernels.  NERF_DIAG_* (and NERF_DW_DIAG)
// are diagnostic builds only (results meaningless).  Every other tuning knob the kernels once had is retired: the
// code no longer branches on it, its verified value is a named constant where it is used, and defining the macro to
// anything else fails the build (the last section of this file).
#pragma once

// ------------------------------------------------------------------------------------
// diagnostic builds
// ------------------------------------------------------------------------------------
// (NERF_DIAG_NO_DMA / NERF_DIAG_NO_STORE: diagnostic timing builds only -- the weight stream or
// the training stores left out, results meaningless -- to price them in the kernels' time)
#ifndef NERF_DIAG_NO_DMA
#define NERF_DIAG_NO_DMA 0
#endif
#ifndef NERF_DIAG_NO_STORE
#define NERF_DIAG_NO_STORE 0
#endif
// (NERF_DIAG_NO_MASK / NERF_DIAG_NO_ACT: the wide forward without its mask bits / without its activation stores)
#ifndef NERF_DIAG_NO_MASK
#define NERF_DIAG_NO_MASK 0
#endif
#ifndef NERF_DIAG_NO_ACT
#define NERF_DIAG_NO_ACT 0
#endif
// (NERF_DIAG_STAMPS: diagnostic only -- the forward overwrites two raw rows per workgroup with its CU id and
// entry / prologue-done / end timestamps, tools/wg_stamps.py)
#ifndef NERF_DIAG_STAMPS
#define NERF_DIAG_STAMPS 0
#endif

// ------------------------------------------------------------------------------------
// schedule knobs (mlp_schedule.h: Groups, prefetch_depth, part_step, finish_parts, dma_spread)
// ------------------------------------------------------------------------------------
#ifndef NERF_GROUP_ACROSS
#define NERF_GROUP_ACROSS 1    // groups may span layers: every group fills its slot
#endif

// A-operand prefetch distance in steps (a bf16 step is one 32-cycle MFMA, an fp32 step four
// 64-cycle ones) and how many steps into unit j + 1 the finish of unit j is issued (its
// VALU then interleaves with unit j + 1's MFMAs instead of stalling the wave)
#ifndef NERF_PREFETCH_BF16
#define NERF_PREFETCH_BF16 3
#endif
#ifndef NERF_PREFETCH_F32
#define NERF_PREFETCH_F32 2  // (fp32 training forward 4.99 / 4.94 / 5.08 ms at 1 / 2 / 3 steps ahead)
#endif
#ifndef NERF_FINISH_DELAY
#define NERF_FINISH_DELAY 3
#endif
#ifndef NERF_PREFETCH_F32W
#define NERF_PREFETCH_F32W 2  // (a PF32W step is four 32-cycle MFMAs)
#endif

// (the wide bf16 dX, one chunk per K-block: the dX stage bV reads bRGB's last output K-block at its step 3, so its
// finish runs 1 step into bV's first unit -- with 3 FinishSchedule refuses the build)
#ifndef NERF_FINISH_DELAY_BF16W
#define NERF_FINISH_DELAY_BF16W 1
#endif

// finish parts per unit (mlp_schedule.h, "Finish parts")
#ifndef NERF_FINISH_PARTS_F32
#define NERF_FINISH_PARTS_F32 1  // (fp32: 8 parts + spread DMA measured 4.88 -> 5.05 ms, training forward)
#endif
#ifndef NERF_FINISH_PARTS_BF16
#define NERF_FINISH_PARTS_BF16 4  // with NERF_DMA_SPREAD_BF16 3: bf16 inference forward 0.517 -> 0.488 ms,
#endif                            // dX 0.619 -> 0.609 at 524,288 samples (r4; 8 parts: no gain)
#ifndef NERF_FINISH_PARTS_BF3
#define NERF_FINISH_PARTS_BF3 8  // with NERF_DMA_SPREAD_BF3 3: bf16x3 forward 1.70 -> 1.58 ms, training
#endif                           // forward 1.97 -> 1.88, dX 1.73 -> 1.65 at 524,288 samples (r4)
#ifndef NERF_FINISH_PARTS_BF3W
#define NERF_FINISH_PARTS_BF3W 2  // (a 16x16 tile's 2 register pairs)
#endif
#ifndef NERF_FINISH_PARTS_F32W
#define NERF_FINISH_PARTS_F32W 2
#endif
#ifndef NERF_FINISH_PARTS_BF16W
#define NERF_FINISH_PARTS_BF16W 2
#endif

// DMA spread (mlp_schedule.h, "DMA spread"): 0 one burst at the group's start, S > 0 over its first 1/S
#ifndef NERF_DMA_SPREAD_F32
#define NERF_DMA_SPREAD_F32 0
#endif
#ifndef NERF_DMA_SPREAD_BF16
#define NERF_DMA_SPREAD_BF16 3
#endif
#ifndef NERF_DMA_SPREAD_BF3
#define NERF_DMA_SPREAD_BF3 3
#endif
#ifndef NERF_DMA_SPREAD_BF3W
#define NERF_DMA_SPREAD_BF3W 3
#endif
#ifndef NERF_DMA_SPREAD_F32W
#define NERF_DMA_SPREAD_F32W 3
#endif
#ifndef NERF_DMA_SPREAD_BF16W
#define NERF_DMA_SPREAD_BF16W 3
#endif

// ------------------------------------------------------------------------------------
// kernel selectors (mlp.hip: PBF3F, PF32T, PF32X, PBF16X, PBF3X), each 0 or 1; every kernel they select compiles
// under FinishSchedule and is listed in tools/asm_check.py
// ------------------------------------------------------------------------------------
// The bf16x3 forward (training, bf16x3f training with bf16 stores, inference, density, persistent): the wide
// 16x16x32 kernel (PBF3W, round 6) or, with -DNERF_BF3_WIDE=0, the 32x32x16 one (PBF3) for A/B builds.  The
// bf16x3 backward (dX / dW, and its W^T pack) is PBF3's either way: both forwards write the same stores.
#ifndef NERF_BF3_WIDE
#define NERF_BF3_WIDE 1
#endif

// The fp32 TRAINING forward: the wide 16x16x4 kernel (PF32W) or, with -DNERF_F32_WIDE=0, PF32's 32x32x2 one; the
// inference forwards -- renders, the march, the bake -- are PF32 either way.  Both read the one fp32 forward pack
// (PF32's DIR 0 layout) and produce the same bits: the wide kernel feeds the matrix pipe PF32's K sequence
// (struct PF32W; tests/test_gpu_f32_wide_forward.py compares raw, activations and masks bitwise), so the fp32
// gradient contract and the full-frame fixtures hold for it by construction.  (Round 6's wide forward summed in
// its own order, k16_feat: 4.9 % faster than PF32's, but the order flipped the ReLU branch of 5.6e-7 of the
// pre-activations and moved the 4,096-ray fine-net L0 bias gradient 9.4e-4 from the reference's against the
// contract's 1e-4 -- it was never the default and is gone.)  nerf_mlp_fwd's flags bit 2 runs PF32's training
// forward whatever the default: the reference of the bitwise test and the A/B arm of tools/mlp_bench.py.
#ifndef NERF_F32_WIDE
#define NERF_F32_WIDE 1
#endif

// The dX of fp32 and bf16x3: the wide 16x16 kernels (DxWave16 over 16-row units, round 6) or, with
// -DNERF_F32_WIDE_DX=0 / -DNERF_BF3_WIDE_DX=0, the 32x32 ones; their W^T packs follow (bwd_layout).  The dZ they
// store is the same old-layout tile-block list either way (the dW is unchanged).
#ifndef NERF_F32_WIDE_DX
#define NERF_F32_WIDE_DX 1
#endif
#ifndef NERF_BF3_WIDE_DX
#define NERF_BF3_WIDE_DX 1
#endif
// (the bf16 dX stays the 32x32 kernel: the wide one, PBF16W, reads a 1 KiB weight chunk per single 16x16x32 MFMA --
// twice the LDS bytes per flop of the 32x32 kernel's, which already ran two waves per SIMD -- and measured slower,
// bf16 dX 0.596 -> 0.747 ms, bf16x3f's 0.564 -> 0.724, profiles/r6/wide_dx_bf16_ab.json; -DNERF_BF16_WIDE_DX=1)
#ifndef NERF_BF16_WIDE_DX
#define NERF_BF16_WIDE_DX 0
#endif
static_assert((NERF_BF3_WIDE == 0 || NERF_BF3_WIDE == 1) && (NERF_F32_WIDE == 0 || NERF_F32_WIDE == 1) &&
                  (NERF_F32_WIDE_DX == 0 || NERF_F32_WIDE_DX == 1) && (NERF_BF3_WIDE_DX == 0 || NERF_BF3_WIDE_DX == 1) &&
                  (NERF_BF16_WIDE_DX == 0 || NERF_BF16_WIDE_DX == 1),
              "NERF_*_WIDE*: 0 or 1");

// ------------------------------------------------------------------------------------
// retired knobs: each is pinned to the value the tests verified (the constant named on the right holds it);
// a -D of any other value fails here
// ------------------------------------------------------------------------------------
#define NERF_PINNED(K, V) static_assert((K) == (V), #K ": only the verified value " #V " is allowed (mlp.hip knob policy)");
#ifdef NERF_PACKED_MASK
NERF_PINNED(NERF_PACKED_MASK, 1)  // mlp_fwd.h finish_L_part: mask bits from the packed bf16 pair
#endif
#ifdef NERF_DMA_LEAN
NERF_PINNED(NERF_DMA_LEAN, 1)  // mlp_dma.h: fetch_piece is the lean form
#endif
#ifdef NERF_KEEP_PE_BF3
NERF_PINNED(NERF_KEEP_PE_BF3, 1)  // mlp_pe_store.h keep_pe()
#endif
#ifdef NERF_DW_NBUF_BF16
NERF_PINNED(NERF_DW_NBUF_BF16, 4)  // mlp_dw.h DW_NBUF_BF16
#endif
#ifdef NERF_DW_SWZ_F32
NERF_PINNED(NERF_DW_SWZ_F32, 1)  // mlp_dw.h dw_swz_f32: the fp32 ring is always swizzled
#endif
#ifdef NERF_DW_F32_PIPE
NERF_PINNED(NERF_DW_F32_PIPE, 1)  // mlp_dw.h dw_job: the pipelined fp32 K loop is the only one
#endif
#ifdef NERF_DW_FETCH_STEP
NERF_PINNED(NERF_DW_FETCH_STEP, 1)  // mlp_dw.h DW_FETCH_STEP
#endif
#ifdef NERF_DW_FETCH_SPLIT
NERF_PINNED(NERF_DW_FETCH_SPLIT, 4)  // mlp_dw.h DW_FETCH_SPLIT
#endif
#ifdef NERF_DW_DMA_NT
NERF_PINNED(NERF_DW_DMA_NT, 1)  // mlp_dw.h glds16_saddr: the dW stream is loaded nt
#endif
#ifdef NERF_DW_BALANCE_MFMA
NERF_PINNED(NERF_DW_BALANCE_MFMA, 1)  // (the fp32 MFMA / fetch cost model: replaced by the measured table)
#endif
#ifdef NERF_DW_LAT_CYCLES
NERF_PINNED(NERF_DW_LAT_CYCLES, 4000)
#endif
#ifdef NERF_DW_ITEMS_PER_CU
NERF_PINNED(NERF_DW_ITEMS_PER_CU, 2)  // mlp.hip DW_ITEMS_PER_CU_F32
#endif
#ifdef NERF_DW_COST_TABLE
NERF_PINNED(NERF_DW_COST_TABLE, 1)  // mlp.hip dw_job_cost: the measured fp32 table
#endif
#ifdef NERF_DW_COST_TABLE_BF
NERF_PINNED(NERF_DW_COST_TABLE_BF, 1)  // mlp.hip dw_job_cost: the measured bf16x3 table
#endif
#undef NERF_PINNED
