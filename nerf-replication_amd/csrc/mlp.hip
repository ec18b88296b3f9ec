// Fused NeRF MLP on gfx950 MFMA: positional encoding + 8x256 trunk (skip@4) + alpha /
// feature / view branch, forward and backward.
//
// Replaces the ATen op sequence of Network.forward / NeRF.forward
// (src/models/nerf/network.py:49-74, 171-192; encoders src/models/encoding/freq.py:7-32)
// and its autograd backward.
//
// Kernels:
//   pack_kernel   fp32 nn.Linear weights -> lane-linear A-operand chunks (W for the
//                 forward, W^T for the dX chain) + per-unit bias chunks
//   fwd_kernel    one wave = 32 samples through all 11 layers; activations never leave
//                 registers; weights stream through a 2-slot LDS ring filled by
//                 global_load_lds, one unit (one 32-row output tile of one layer) per slot.
//                 The training variant also stores every layer input feature-major and
//                 the ReLU masks.
//   dx_kernel     the dX chain (W^T products + ReLU masks), 32 samples per wave, storing
//                 every layer's output gradient feature-major
//   dw_kernel     dW/db = dz . act^T, a K = samples GEMM per layer; per-item partial sums
//                 reduced in a fixed order (dw_reduce_kernel), or fp32 atomics
//
// Source map.  This file is the translation unit the Makefile compiles (once per precision and kernel family,
// -DNERF_MLP_PREC / -DNERF_MLP_PART, and once for the C ABI) and the one tests and tools include under
// NERF_MLP_DEVICE_ONLY (the device side only).  It holds the launchers, the explicit instantiations and the
// extern "C" functions; the device side is in flat headers, each including what it depends on:
//   mlp_knobs.h     every -DNERF_* knob: default, measurement, and the knob policy
//   mlp_tables.h    the network's layout tables (units, tiles, stores)
//   mlp_policy.h    the precision policies PF32 .. PBF16W, mask-bit and ReLU helpers
//   mlp_pack.h      packed-weight layout, pack_kernel, pack_plan_kernel, pack_gather_kernel
//   mlp_schedule.h  groups, steps, finish parts, DMA spread, FinishSchedule, group_body
//   mlp_dma.h       the LDS-DMA pieces of the weight ring
//   mlp_pe_store.h  positional encoding into tiles, the training stores' layout, masks
//   mlp_fwd.h       FwdArgs, FwdWave, FwdWave16, fwd_kernel
//   mlp_dx.h        DxArgs, DxWave, DxWave16, dx_kernel
//   mlp_dw.h        the dW jobs, dw_kernel, dw_reduce_kernel
#include "mlp_dx.h"
#include "mlp_dw.h"

#include <mutex>

#ifndef NERF_MLP_DEVICE_ONLY
#if defined(NERF_MLP_PREC) != defined(NERF_MLP_PART)
#error "mlp.hip: define NERF_MLP_PREC and NERF_MLP_PART together (a kernel unit, csrc/Makefile) or neither (the C-ABI unit)"
#endif
// ======================================================================================
// launchers
// ======================================================================================
using namespace nerf;
using namespace nerf::mlp;

template <class P> static constexpr size_t fwd_lds_bytes() { return (size_t)NSLOT * SLOT_CAP * 1024; }
template <class P> static constexpr size_t dx_lds_bytes() { return (size_t)NSLOT * SLOT_CAP * 1024; }
template <class P> static constexpr size_t dw_lds_bytes() { return (size_t)dw_nbuf<P>() * DW_SLOTS * P::CH * 1024; }

template <class K>
static void allow_lds(K kernel, size_t bytes) {
  if (bytes > 65536) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

template <class P, bool STORE, bool DENSITY, bool HALF = false>
static void launch_fwd(const FwdArgs& a, hipStream_t stream) {
  static const bool lds_ok = (allow_lds(fwd_kernel<P, STORE, DENSITY, false, HALF>, fwd_lds_bytes<P>()), true);
  (void)lds_ok;
  const int spb = samples_per_block<P>();
  dim3 grid((unsigned)(STORE ? a.nblk * 32 / spb : (a.M + spb - 1) / spb));
  hipLaunchKernelGGL((fwd_kernel<P, STORE, DENSITY, false, HALF>), grid, dim3(P::WAVES * 64), fwd_lds_bytes<P>(),
                     stream, a);
}

// persistent inference forward: one wave of workgroups (every CU x its resident workgroups),
// fewer when M_cap needs fewer blocks
template <class P>
static void launch_fwd_persist(const FwdArgs& a, hipStream_t stream) {
  auto kern = fwd_kernel<P, false, false, true>;
  static const int resident = [&] {
    allow_lds(kern, fwd_lds_bytes<P>());
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void*)kern, P::WAVES * 64, fwd_lds_bytes<P>()) !=
            hipSuccess || per <= 0)
      per = 1;
    return cus * per;
  }();
  const int64_t spb = samples_per_block<P>(), need = (a.M_cap + spb - 1) / spb;
  dim3 grid((unsigned)(need < resident ? need : resident));
  hipLaunchKernelGGL(kern, grid, dim3(P::WAVES * 64), fwd_lds_bytes<P>(), stream, a);
}

template <class P>
static void launch_dx(const DxArgs& x, int64_t ldm, hipStream_t stream) {
  static const bool lds_ok = (allow_lds(dx_kernel<P>, dx_lds_bytes<P>()), true);
  (void)lds_ok;
  hipLaunchKernelGGL((dx_kernel<P>), dim3((unsigned)(ldm / samples_per_block<P>())), dim3(P::WAVES * 64),
                     dx_lds_bytes<P>(), stream, x);
}

template <class P>
static void launch_fwd_any(const FwdArgs& a, bool store, bool density, hipStream_t stream) {
  if (store) launch_fwd<P, true, false>(a, stream);
  else if (density) launch_fwd<P, false, true>(a, stream);
  else launch_fwd<P, false, false>(a, stream);
}

// Every kernel launch of one precision, instantiated in that precision's translation unit
// (mlp.hip compiled with -DNERF_MLP_PREC=0 fp32 / 1 bf16 / 2 bf16x3, csrc/Makefile); the C-ABI
// unit (no NERF_MLP_PREC) only declares them, so the three precisions compile in parallel.
namespace nerf {
namespace mlp {
// the pack plan of (P, dir) on the device that holds the parameters: built on first use (one launch, then a
// stream sync), kept for the process; null if it cannot be allocated, or while the stream is being captured
// (the build syncs), and the caller falls back to pack_kernel.  The device comes from the parameter pointer,
// not the current device (a net on cuda:1 packed while cuda:0 is current), and the build runs under a device
// guard on that device.  (round 6)
static_assert(NET_PARAMS < (1 << 24), "a plan entry holds a 24-bit parameter offset");
// the packed-weight layout of a policy's forward: 32-row units (0), or the 16-row units of PBF3W (2)
template <class P> static constexpr int fwd_layout() { return wide_kind<P>() ? 2 : 0; }
// ... and of its dX: 32-row units (1), or the 16-row units of PF32W / PBF3W (3)
template <class P> static constexpr int bwd_layout() { return wide_kind<P>() ? 3 : 1; }
template <class P, class F> static void with_layout(int dir, F&& f) {  // f(integral_constant<layout>)
  if (dir == 1) {
    f(std::integral_constant<int, bwd_layout<P>()>{});
  } else {
    f(std::integral_constant<int, fwd_layout<P>()>{});
  }
}
template <class P>
static const uint32_t* pack_plan(int dir, const void* params, hipStream_t stream) {
  static std::mutex mu;
  static uint32_t* plans[64][2] = {};
  hipPointerAttribute_t at{};
  if (hipPointerGetAttributes(&at, params) != hipSuccess || at.device < 0 || at.device >= 64) return nullptr;
  const int dev = at.device;
  std::lock_guard<std::mutex> lock(mu);
  uint32_t*& plan = plans[dev][dir];
  if (!plan) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess || (cur != dev && hipSetDevice(dev) != hipSuccess)) return nullptr;
    const int64_t n = total_chunks(P::CH, dir == 0 ? fwd_layout<P>() : bwd_layout<P>()) * 64;
    uint32_t* p = nullptr;
    bool ok = hipMalloc(&p, (size_t)n * P::E * sizeof(uint32_t)) == hipSuccess;
    if (ok) {
      dim3 grid((unsigned)((n + 255) / 256));
      with_layout<P>(dir, [&](auto lay) {
        constexpr int D = decltype(lay)::value;
        hipLaunchKernelGGL((pack_plan_kernel<P, D>), grid, dim3(256), 0, stream, unit_offsets<P::CH, D>(), p);
      });
      ok = hipStreamSynchronize(stream) == hipSuccess;
      if (!ok) (void)hipFree(p);
    }
    if (cur != dev) (void)hipSetDevice(cur);
    if (!ok) return nullptr;
    plan = p;
  }
  return plan;
}
template <class P>
void mlp_pack_impl(const ParamPtrs& prm, int dir, char* dst, hipStream_t stream) {
  const int64_t n = total_chunks(P::CH, dir == 0 ? fwd_layout<P>() : bwd_layout<P>()) * 64;
  dim3 grid((unsigned)((n + 255) / 256));
  // the 24 parameters back to back (FusedAdam's flat buffer): the plan gather (NERF_PACK_PLAN=0: always
  // the direct pack, for A/B timing)
  const char* env = getenv("NERF_PACK_PLAN");
  bool flat = !(env && env[0] == '0');
  for (int k = 1; k < NPARAM; ++k) flat = flat && prm.p[k] == prm.p[0] + param_offset(k);
  if (flat) {
    if (const uint32_t* plan = pack_plan<P>(dir, prm.p[0], stream)) {
      hipLaunchKernelGGL((pack_gather_kernel<P>), grid, dim3(256), 0, stream, prm.p[0], plan, dst, n);
      return;
    }
  }
  with_layout<P>(dir, [&](auto lay) {
    constexpr int D = decltype(lay)::value;
    hipLaunchKernelGGL((pack_kernel<P, D>), grid, dim3(256), 0, stream, prm, unit_offsets<P::CH, D>(), dst);
  });
}
template <class P>
void mlp_fwd_train_impl(const FwdArgs& a, hipStream_t stream) {
  launch_fwd<P, true, false>(a, stream);
}
// the policies the kernel selectors choose (mlp_knobs.h: what each selects, and why these are the defaults)
using PBF3F = std::conditional_t<NERF_BF3_WIDE != 0, PBF3W, PBF3>;         // every bf16x3 forward
using PF32T = std::conditional_t<NERF_F32_WIDE != 0, PF32W, PF32>;         // the fp32 training forward
using PF32X = std::conditional_t<NERF_F32_WIDE_DX != 0, PF32W, PF32>;      // the fp32 dX
using PBF16X = std::conditional_t<NERF_BF16_WIDE_DX != 0, PBF16W, PBF16>;  // the bf16 / bf16x3f dX
using PBF3X = std::conditional_t<NERF_BF3_WIDE_DX != 0, PBF3W, PBF3>;      // the bf16x3 dX
// bf16x3 forward, bf16 (hi-half) stores for the bf16 backward
void mlp_fwd_train_half_impl(const FwdArgs& a, hipStream_t stream);
#if defined(NERF_MLP_PREC) && NERF_MLP_PREC == 2 && NERF_MLP_PART == 4
void mlp_fwd_train_half_impl(const FwdArgs& a, hipStream_t stream) { launch_fwd<PBF3F, true, false, true>(a, stream); }
#endif
// the three inference forwards, one translation unit each (parts 1, 5, 6)
template <class P>
void mlp_fwd_plain_impl(const FwdArgs& a, hipStream_t stream) { launch_fwd<P, false, false>(a, stream); }
template <class P>
void mlp_fwd_density_impl(const FwdArgs& a, hipStream_t stream) { launch_fwd<P, false, true>(a, stream); }
template <class P>
void mlp_fwd_persist_impl(const FwdArgs& a, hipStream_t stream) { launch_fwd_persist<P>(a, stream); }
template <class P>
void mlp_fwd_infer_impl(const FwdArgs& a, bool density, hipStream_t stream) {
  if (a.M_dev) mlp_fwd_persist_impl<P>(a, stream);
  else if (density) mlp_fwd_density_impl<P>(a, stream);
  else mlp_fwd_plain_impl<P>(a, stream);
}
template <class P>
void mlp_dx_impl(const DxArgs& x, int64_t ldm, hipStream_t stream) {
  launch_dx<P>(x, ldm, stream);
}
template <class P>
void mlp_dw_impl(const DwArgs& w, dim3 grid, hipStream_t stream) {
  allow_lds(dw_kernel<P>, dw_lds_bytes<P>());
  hipLaunchKernelGGL((dw_kernel<P>), grid, dim3(DW_WAVES * 64), dw_lds_bytes<P>(), stream, w);
}
// explicit instantiations, split further by part (-DNERF_MLP_PART: 0 training forward, 1 inference forward,
// 2 dX + pack, 3 dW, 4 the bf16x3f / the wide fp32 training forward, 5 density-only forward, 6 persistent
// inference forward) so that no translation unit holds more than one or two of the large straight-line kernels
#define NERF_MLP_I_PACK(EXT, P) EXT template void mlp_pack_impl<P>(const ParamPtrs&, int, char*, hipStream_t);
#define NERF_MLP_I_FWDT(EXT, P) EXT template void mlp_fwd_train_impl<P>(const FwdArgs&, hipStream_t);
#define NERF_MLP_I_FWDI(EXT, P) EXT template void mlp_fwd_plain_impl<P>(const FwdArgs&, hipStream_t);
#define NERF_MLP_I_FWDD(EXT, P) EXT template void mlp_fwd_density_impl<P>(const FwdArgs&, hipStream_t);
#define NERF_MLP_I_FWDP(EXT, P) EXT template void mlp_fwd_persist_impl<P>(const FwdArgs&, hipStream_t);
#define NERF_MLP_I_DX(EXT, P) EXT template void mlp_dx_impl<P>(const DxArgs&, int64_t, hipStream_t);
#define NERF_MLP_I_DW(EXT, P) EXT template void mlp_dw_impl<P>(const DwArgs&, dim3, hipStream_t);
#define NERF_MLP_IMPLS(EXT, P) \
  NERF_MLP_I_PACK(EXT, P) NERF_MLP_I_FWDT(EXT, P) NERF_MLP_I_FWDI(EXT, P) NERF_MLP_I_FWDD(EXT, P) \
  NERF_MLP_I_FWDP(EXT, P) NERF_MLP_I_DX(EXT, P) NERF_MLP_I_DW(EXT, P)
#define NERF_MLP_FWDS(EXT, P) \
  NERF_MLP_I_FWDT(EXT, P) NERF_MLP_I_FWDI(EXT, P) NERF_MLP_I_FWDD(EXT, P) NERF_MLP_I_FWDP(EXT, P)
#if !defined(NERF_MLP_PREC)
NERF_MLP_IMPLS(extern, PF32)
NERF_MLP_I_FWDT(extern, PF32W)
NERF_MLP_I_PACK(extern, PF32W)
NERF_MLP_I_DX(extern, PF32W)
NERF_MLP_I_DX(extern, PBF3W)
NERF_MLP_I_DX(extern, PBF16W)
NERF_MLP_I_PACK(extern, PBF16W)
NERF_MLP_IMPLS(extern, PBF16)
NERF_MLP_I_PACK(extern, PBF3)  // bf16x3: the W^T pack, dX, dW (+ the forward pack when not wide)
NERF_MLP_I_DX(extern, PBF3)
NERF_MLP_I_DW(extern, PBF3)
NERF_MLP_FWDS(extern, PBF3F)
NERF_MLP_I_PACK(extern, PBF3W)
NERF_MLP_I_FWDI(extern, PBF6)  // bf16x6: the inference forward and its pack only
NERF_MLP_I_PACK(extern, PBF6)
#elif NERF_MLP_PREC == 3
#if NERF_MLP_PART == 1
NERF_MLP_I_FWDI(, PBF6)
#elif NERF_MLP_PART == 2
NERF_MLP_I_PACK(, PBF6)
#endif
#else
// NERF_PP: the precision's pack / dW policy, NERF_PP_FWD: its forwards', NERF_PP_DX: its dX's
#if NERF_MLP_PREC == 0
#define NERF_PP PF32
#define NERF_PP_FWD PF32
#define NERF_PP_DX PF32X  // (PF32W unless NERF_F32_WIDE_DX=0)
#elif NERF_MLP_PREC == 1
#define NERF_PP PBF16
#define NERF_PP_FWD PBF16
#define NERF_PP_DX PBF16X  // (PBF16W unless NERF_BF16_WIDE_DX=0)
#else
#define NERF_PP PBF3
#define NERF_PP_FWD PBF3F  // (PBF3W unless NERF_BF3_WIDE=0)
#define NERF_PP_DX PBF3X   // (PBF3W unless NERF_BF3_WIDE_DX=0)
#endif
#if NERF_MLP_PART == 0
NERF_MLP_I_FWDT(, NERF_PP_FWD)
#endif
#if NERF_MLP_PREC == 0 && NERF_MLP_PART == 4
NERF_MLP_I_FWDT(, PF32W)  // (the wide fp32 training forward, a translation unit of its own)
#endif
#if NERF_MLP_PART == 1
NERF_MLP_I_FWDI(, NERF_PP_FWD)
#endif
#if NERF_MLP_PART == 5
NERF_MLP_I_FWDD(, NERF_PP_FWD)
#endif
#if NERF_MLP_PART == 6
NERF_MLP_I_FWDP(, NERF_PP_FWD)
#endif
#if NERF_MLP_PART == 2
NERF_MLP_I_DX(, NERF_PP_DX)
NERF_MLP_I_PACK(, NERF_PP)
#if NERF_MLP_PREC == 2 && (NERF_BF3_WIDE || NERF_BF3_WIDE_DX)
NERF_MLP_I_PACK(, PBF3W)
#endif
#if NERF_MLP_PREC == 0 && NERF_F32_WIDE_DX
NERF_MLP_I_PACK(, PF32W)  // (the W^T pack of the wide dX; the wide forward reads PF32's forward pack)
#endif
#if NERF_MLP_PREC == 1 && NERF_BF16_WIDE_DX
NERF_MLP_I_PACK(, PBF16W)
#endif
#endif
#if NERF_MLP_PART == 3
NERF_MLP_I_DW(, NERF_PP)
#endif
#endif
}  // namespace mlp
}  // namespace nerf

#if !defined(NERF_MLP_PREC)

extern "C" {

int64_t nerf_mlp_net_params(void) { return NET_PARAMS; }
int64_t nerf_mlp_param_offset(int i) { return (i >= 0 && i <= NPARAM) ? param_offset(i) : -1; }

// dtype 3 (bf16x3f) = a bf16x3 forward (its forward pack) whose training stores are bf16, with
// the bf16 backward (its W^T pack, bf16 dZ): every function below maps it to its part
static int fwd_prec(int dtype) { return dtype == 3 ? 2 : dtype; }
static int bwd_prec(int dtype) { return dtype == 3 ? 1 : dtype; }
static int store_prec(int dtype) { return dtype == 3 ? 1 : dtype; }
// dtype 4 (bf16x6) is an inference forward only: its forward pack and nerf_mlp_fwd without flags
static bool train_dtype(int dtype) { return dtype >= 0 && dtype <= 3; }

int64_t nerf_mlp_packed_bytes(int dtype, int dir) {
  if (dtype == 4) return dir == 0 ? total_chunks(PBF6::CH, 0) * 1024 : -1;
  if (!train_dtype(dtype) || (dir != 0 && dir != 1)) return -1;
  const int p = dir == 0 ? fwd_prec(dtype) : bwd_prec(dtype);
  if (p == 2 && dir == 0) return total_chunks(PBF3F::CH, fwd_layout<PBF3F>()) * 1024;  // (the wide bf16x3 forward)
  if (p == 0 && dir == 1) return total_chunks(PF32X::CH, bwd_layout<PF32X>()) * 1024;  // (the fp32 dX)
  if (p == 2 && dir == 1) return total_chunks(PBF3X::CH, bwd_layout<PBF3X>()) * 1024;  // (the bf16x3 dX)
  if (p == 1 && dir == 1) return total_chunks(PBF16X::CH, bwd_layout<PBF16X>()) * 1024;  // (the bf16 dX)
  return total_chunks(p == 1 ? PBF16::CH : PF32::CH, dir) * 1024;  // bf16x3: CH 4 as fp32
}

int64_t nerf_mlp_padded_samples(int64_t M) { return (M + M_ALIGN - 1) / M_ALIGN * M_ALIGN; }
int64_t nerf_mlp_act_bytes(int dtype, int64_t M) {
  if (dtype < 0 || dtype > 3 || M < 0) return -1;
  return (int64_t)A_ROWS * nerf_mlp_padded_samples(M) * (store_prec(dtype) == 1 ? 2 : 4);
}
int64_t nerf_mlp_dz_bytes(int dtype, int64_t M) {
  if (dtype < 0 || dtype > 3 || M < 0) return -1;
  return (int64_t)Z_ROWS * nerf_mlp_padded_samples(M) * (store_prec(dtype) == 1 ? 2 : 4);
}
int64_t nerf_mlp_mask_bytes(int64_t M) { return nerf_mlp_padded_samples(M) / 32 * MASK_GROUPS * 64 * 16; }

int nerf_mlp_pack(const float* const* params, int dtype, void* packed_fwd, void* packed_bwd, hipStream_t stream) {
  NERF_REQUIRE(params != nullptr, "nerf_mlp_pack: params is null");
  NERF_REQUIRE(dtype >= 0 && dtype <= 4,
               "nerf_mlp_pack: dtype must be 0 (f32), 1 (bf16), 2 (bf16x3), 3 (bf16x3f) or 4 (bf16x6), got %d", dtype);
  NERF_REQUIRE(dtype != 4 || packed_bwd == nullptr, "nerf_mlp_pack: dtype 4 (bf16x6) has no backward pack");
  ParamPtrs prm;
  for (int i = 0; i < NPARAM; ++i) {
    NERF_REQUIRE(params[i] != nullptr, "nerf_mlp_pack: params[%d] is null", i);
    prm.p[i] = params[i];
  }
  for (int dir = 0; dir < 2; ++dir) {
    void* dst = dir == 0 ? packed_fwd : packed_bwd;
    if (!dst) continue;
    const int p = dir == 0 ? fwd_prec(dtype) : bwd_prec(dtype);
    if (p == 4) mlp_pack_impl<PBF6>(prm, dir, (char*)dst, stream);
    else if (p == 0 && dir == 1) mlp_pack_impl<PF32X>(prm, dir, (char*)dst, stream);
    else if (p == 0) mlp_pack_impl<PF32>(prm, dir, (char*)dst, stream);  // (every fp32 forward, PF32W's too)
    else if (p == 1 && dir == 1) mlp_pack_impl<PBF16X>(prm, dir, (char*)dst, stream);
    else if (p == 1) mlp_pack_impl<PBF16>(prm, dir, (char*)dst, stream);
    else if (dir == 0) mlp_pack_impl<PBF3F>(prm, dir, (char*)dst, stream);
    else mlp_pack_impl<PBF3X>(prm, dir, (char*)dst, stream);
    if (int e = check_launch("nerf_mlp_pack")) return e;
  }
  return 0;
}

// flags: bit0 = store activations + masks for backward, bit1 = density only, bit2 (dtype 0 with bit0 only) = the
// 32x32 PF32 training forward instead of the default one (the same pack, the same bits)
int nerf_mlp_fwd(const void* packed_fwd, int dtype, const float* pts, const float* viewdirs, int samples_per_dir,
                 const int32_t* dir_index, int64_t M, int flags, float* raw, void* act, uint16_t* masks,
                 hipStream_t stream) {
  NERF_REQUIRE(dtype >= 0 && dtype <= 4, "nerf_mlp_fwd: bad dtype %d", dtype);
  NERF_REQUIRE(dtype != 4 || flags == 0, "nerf_mlp_fwd: dtype 4 (bf16x6) is an inference forward only (flags 0)");
  NERF_REQUIRE(M >= 0, "nerf_mlp_fwd: M < 0");
  if (M == 0) return 0;
  const bool store = flags & 1, density = flags & 2, narrow = flags & 4;
  NERF_REQUIRE(!narrow || (dtype == 0 && store),
               "nerf_mlp_fwd: flags bit 2 (the 32x32 fp32 training forward) needs dtype 0 and bit 0, got dtype %d flags 0x%x",
               dtype, flags);
  NERF_REQUIRE(packed_fwd && pts && raw, "nerf_mlp_fwd: null pointer");
  NERF_REQUIRE(density || viewdirs, "nerf_mlp_fwd: viewdirs required unless density-only");
  NERF_REQUIRE(density || dir_index || samples_per_dir > 0, "nerf_mlp_fwd: samples_per_dir must be > 0");
  NERF_REQUIRE(!store || (act && masks), "nerf_mlp_fwd: store requires act and masks");
  NERF_REQUIRE(!(store && density), "nerf_mlp_fwd: store and density-only are exclusive");
  FwdArgs a{(const char*)packed_fwd, pts, viewdirs, dir_index, samples_per_dir, M,
            nerf_mlp_padded_samples(M) / 32, raw, act, masks};
  if (store) {
    if (dtype == 0 && narrow) mlp_fwd_train_impl<PF32>(a, stream);
    else if (dtype == 0) mlp_fwd_train_impl<PF32T>(a, stream);
    else if (dtype == 1) mlp_fwd_train_impl<PBF16>(a, stream);
    else if (dtype == 2) mlp_fwd_train_impl<PBF3F>(a, stream);
    else mlp_fwd_train_half_impl(a, stream);
  } else {
    if (dtype == 4) mlp_fwd_plain_impl<PBF6>(a, stream);
    else if (dtype == 0) mlp_fwd_infer_impl<PF32>(a, density, stream);
    else if (dtype == 1) mlp_fwd_infer_impl<PBF16>(a, density, stream);
    else mlp_fwd_infer_impl<PBF3F>(a, density, stream);
  }
  return check_launch("nerf_mlp_fwd");
}

// inference forward whose sample count is on the device (min(*M_dev, M_cap)): no host sync sizes
// the launch (the grid march's rounds)
int nerf_mlp_fwd_count(const void* packed_fwd, int dtype, const float* pts, const float* viewdirs, int samples_per_dir,
                       const int32_t* dir_index, const int32_t* M_dev, int64_t M_cap, float* raw, hipStream_t stream) {
  NERF_REQUIRE(dtype >= 0 && dtype <= 3, "nerf_mlp_fwd_count: bad dtype %d", dtype);
  NERF_REQUIRE(M_cap >= 0, "nerf_mlp_fwd_count: M_cap < 0");
  if (M_cap == 0) return 0;
  NERF_REQUIRE(packed_fwd && pts && raw && viewdirs && M_dev, "nerf_mlp_fwd_count: null pointer");
  NERF_REQUIRE(dir_index || samples_per_dir > 0, "nerf_mlp_fwd_count: samples_per_dir must be > 0");
  FwdArgs a{(const char*)packed_fwd, pts, viewdirs, dir_index, samples_per_dir, M_cap, 0, raw, nullptr, nullptr,
            M_dev, M_cap};
  if (dtype == 0) mlp_fwd_infer_impl<PF32>(a, false, stream);
  else if (dtype == 1) mlp_fwd_infer_impl<PBF16>(a, false, stream);
  else mlp_fwd_infer_impl<PBF3F>(a, false, stream);
  return check_launch("nerf_mlp_fwd_count");
}

// work items of the dW launch: at most one per CU (a single wave of workgroups that ends
// together), split across the 10 jobs in proportion to the bytes each reads, at least one
// and at most one per block per job
static int cu_count() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) !=
                                              hipSuccess || n <= 0)
    n = 256;
  return n;
}
// relative cost of one 32-sample block of job j (only the ratios between the jobs of one dtype matter).
// fp32 and bf16x3: each job's measured time with the whole chip to itself (diagnostic build -DNERF_DW_DIAG,
// NERF_DW_ONLY_JOB=j, tools/gpu_dw_jobs.sh; per mille of the L1 job).  For fp32 it replaced a model of MFMA
// cycles and fetch latency that under-priced L5 (measured 1.42x L1, modelled 1.25x) and over-priced the view job
// (0.79x, modelled 1.13x) and L0: dW 4.94 -> 4.72 ms at 524k samples; bf16x3 2.005 -> 1.943 ms.  bf16 dW is
// HBM-bound, its 4-deep ring hides the fetch latency and its jobs all stream HBM at once: the tile-blocks
// streamed (its solo timings, L5 1.73x L1, misprice the shared-bandwidth run: 0.914 -> 0.949 ms).
static int64_t dw_job_cost(int dtype, int j) {
  static constexpr int64_t MEASURED_F32[NDWJOB] = {332, 1000, 1014, 1021, 1018, 1418, 1024, 1012, 1131, 792};
  static constexpr int64_t MEASURED_BF3[NDWJOB] = {552, 1000, 1011, 1004, 1004, 1465, 1003, 1007, 1144, 1044};
  return dtype == 0 ? MEASURED_F32[j] : dtype == 2 ? MEASURED_BF3[j] : dw_job_tiles(j);
}
// fp32: two items per CU (measured -2.5 % over one: the tail of the last items is shorter);
// bf16: one (every extra item re-adds its partial dW with atomics)
constexpr int DW_ITEMS_PER_CU_F32 = 2;
constexpr int64_t DW_MIN_BLOCKS = 8;  // 32-sample blocks per dW work item, at least
static void dw_items(int dtype, int64_t nblk, int item_off[NDWJOB + 1], int job_of[NDWJOB]) {
  static const int cus = cu_count();
  const int target = cus * (dtype == 0 ? DW_ITEMS_PER_CU_F32 : 1);
  int n[NDWJOB];
  int64_t cost = 0;
  for (int j = 0; j < NDWJOB; ++j) cost += dw_job_cost(dtype, j);
  // a small launch (a 64-ray chunk: 128 blocks) gets few items, each of >= DW_MIN_BLOCKS blocks:
  // every item adds a 364 KB partial-sum slice that the ordered reduce reads back
  const int64_t max_items = nblk / DW_MIN_BLOCKS > 1 ? nblk / DW_MIN_BLOCKS : 1;
  int total = 0;
  for (int j = 0; j < NDWJOB; ++j) {
    int64_t k = target * (int64_t)dw_job_cost(dtype, j) / cost;
    n[j] = (int)(k < 1 ? 1 : k > max_items ? max_items : k);
    total += n[j];
  }
  // the remaining CUs go, one at a time, to the job whose items are the longest
  while (total < target) {
    int best = -1;
    double worst = 0.0;  // (worst = 0 only before the first candidate)
    for (int j = 0; j < NDWJOB; ++j) {
      if (n[j] >= max_items) continue;
      const double per = (double)dw_job_cost(dtype, j) / n[j];
      if (per > worst) worst = per, best = j;
    }
    if (best < 0) break;
    ++n[best];
    ++total;
  }
  // longest items first: with more items than CUs, the short ones fill the tail
  for (int j = 0; j < NDWJOB; ++j) job_of[j] = j;
  for (int a = 0; a < NDWJOB; ++a)
    for (int b = a + 1; b < NDWJOB; ++b)
      if ((double)dw_job_cost(dtype, job_of[b]) / n[job_of[b]] > (double)dw_job_cost(dtype, job_of[a]) / n[job_of[a]]) {
        const int t = job_of[a];
        job_of[a] = job_of[b];
        job_of[b] = t;
      }
  item_off[0] = 0;
  for (int s = 0; s < NDWJOB; ++s) item_off[s + 1] = item_off[s] + n[job_of[s]];
#ifdef NERF_DW_DIAG
  // (diagnostic build only) NERF_DW_ONLY_JOB=j: every item to job j, the others skipped
  if (const char* e = getenv("NERF_DW_ONLY_JOB")) {
    const int jj = atoi(e);
    job_of[0] = jj;  // segments 1.. are empty
    for (int s = 1; s <= NDWJOB; ++s) item_off[s] = target;
  }
#endif
}
int64_t nerf_mlp_dw_items(int dtype, int64_t M) {
  if (dtype < 0 || dtype > 3 || M < 0) return -1;
  int off[NDWJOB + 1], job[NDWJOB];
  dw_items(bwd_prec(dtype), nerf_mlp_padded_samples(M) / 32, off, job);
  return off[NDWJOB];
}

// dX chain only: dz (per-layer output gradients, fragment-native tiles) from d_raw + masks
int nerf_mlp_bwd_dx(const void* packed_bwd, int dtype, const float* d_raw, int64_t M, const uint16_t* masks, void* dz,
                    hipStream_t stream) {
  NERF_REQUIRE(dtype >= 0 && dtype <= 3, "nerf_mlp_bwd_dx: bad dtype %d", dtype);
  dtype = bwd_prec(dtype);
  NERF_REQUIRE(M >= 0, "nerf_mlp_bwd_dx: M < 0");
  if (M == 0) return 0;
  NERF_REQUIRE(packed_bwd && d_raw && masks && dz, "nerf_mlp_bwd_dx: null pointer");
  const int64_t ldm = nerf_mlp_padded_samples(M);
  DxArgs x{(const char*)packed_bwd, d_raw, M, ldm / 32, masks, dz};
  if (dtype == 0) mlp_dx_impl<PF32X>(x, ldm, stream);
  else if (dtype == 1) mlp_dx_impl<PBF16X>(x, ldm, stream);
  else mlp_dx_impl<PBF3X>(x, ldm, stream);
  return check_launch("nerf_mlp_bwd_dx");
}

int64_t nerf_mlp_dw_workspace_bytes(int dtype, int64_t M) {
  const int64_t items = nerf_mlp_dw_items(dtype, M);
  return items < 0 ? -1 : items * (int64_t)DW_PITEM * 4;
}

// dW/db only: grad += dz . act^T (grad must be zeroed or hold a running sum).  workspace (nullable,
// nerf_mlp_dw_workspace_bytes): per-item partial sums reduced in a fixed order -- bit-reproducible;
// null: fp32 atomics.
int nerf_mlp_bwd_dw_ws(int dtype, int64_t M, const void* act, const void* dz, float* grad, void* workspace,
                       hipStream_t stream) {
  NERF_REQUIRE(dtype >= 0 && dtype <= 3, "nerf_mlp_bwd_dw: bad dtype %d", dtype);
  dtype = bwd_prec(dtype);
  NERF_REQUIRE(M >= 0, "nerf_mlp_bwd_dw: M < 0");
  if (M == 0) return 0;
  NERF_REQUIRE(act && dz && grad, "nerf_mlp_bwd_dw: null pointer");
  const int64_t nblk = nerf_mlp_padded_samples(M) / 32;
  DwArgs w{dz, act, nblk, grad, {}, {}, (float*)workspace};
  dw_items(dtype, nblk, w.item_off, w.job_of);
  dim3 grid((unsigned)w.item_off[NDWJOB]);
  if (dtype == 0) mlp_dw_impl<PF32>(w, grid, stream);
  else if (dtype == 1) mlp_dw_impl<PBF16>(w, grid, stream);
  else mlp_dw_impl<PBF3>(w, grid, stream);
  if (int e = check_launch("nerf_mlp_bwd_dw")) return e;
  if (workspace) {
    DwReduceArgs r{(const float*)workspace, grad, {}, {}};
    for (int k = 0; k <= NDWJOB; ++k) r.item_off[k] = w.item_off[k];
    for (int k = 0; k < NDWJOB; ++k) r.job_of[k] = w.job_of[k];
    const int64_t per = (int64_t)DW_WAVES * DW_PWAVE;
    hipLaunchKernelGGL(dw_reduce_kernel, dim3((unsigned)((per + 255) / 256), NDWJOB), dim3(256), 0, stream, r);
    return check_launch("nerf_mlp_bwd_dw_reduce");
  }
  return 0;
}
int nerf_mlp_bwd_dw(int dtype, int64_t M, const void* act, const void* dz, float* grad, hipStream_t stream) {
  return nerf_mlp_bwd_dw_ws(dtype, M, act, dz, grad, nullptr, stream);
}

int nerf_mlp_bwd(const void* packed_bwd, int dtype, const float* d_raw, int64_t M, const void* act,
                 const uint16_t* masks, void* dz, float* grad, hipStream_t stream) {
  if (int e = nerf_mlp_bwd_dx(packed_bwd, dtype, d_raw, M, masks, dz, stream)) return e;
  return nerf_mlp_bwd_dw(dtype, M, act, dz, grad, stream);
}

}  // extern "C"
#endif  // !NERF_MLP_PREC
#endif  // NERF_MLP_DEVICE_ONLY
