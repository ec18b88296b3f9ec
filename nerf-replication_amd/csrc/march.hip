// The grid-accelerated ray march on gfx950, with early ray termination, and its differentiable
// second pass (per-ray segments, point budget, jitter, distortion).  The grid itself -- lookup,
// bake, online update -- is grid.hip.
//
// Reference semantics (echo636/nerf-replication):
//   render_accelerated      src/models/nerf/renderer/volume_renderer.py:268-357
//
// The reference marches all alive rays one t-step at a time (800 Python iterations, a
// host sync each).  Here each round lets every alive ray collect its next K occupied
// steps (gather), the fine MLP runs once on all collected points, and a per-ray
// compositor consumes them in t order, stopping exactly where the reference would
// (T < threshold after a queried step).  Points past a ray's termination are evaluated
// but never composited, so outputs are those of the step-by-step march.
#include "grid_common.h"

#include <cmath>
#include <type_traits>

namespace nerf {

struct MarchState {
  float* T;
  float* rgb;
  float* depth;
  float* acc;
  int32_t* next_step;
  uint8_t* alive;     // 1 = still marching
  uint8_t* exhausted; // 1 = gather reached the end of the t table
};

struct MarchGatherArgs {
  const float* rays;  // [N,6]
  int64_t N;
  const float* t_table;
  int n_steps;
  const uint8_t* grid;
  int res;
  const uint8_t* macro;  // [mres^3] 1 = some cell of the 8^3 block occupied (nerf_march_macro), or null
  BBox bb;
  int K;
  int k_low;       // rays with T < t_split gather at most k_low steps (they terminate soon)
  float t_split;
  MarchState st;
  int32_t* counters;   // [0] points reserved, [1] rays alive entering the round
  unsigned long long* evaluated;  // += points written below cap (what the MLP evaluates), or null
  int32_t* out_ray;    // [cap]
  int32_t* out_step;   // [cap]
  float* out_pts;      // [cap,3]
  int32_t* ray_off;    // [N]
  int32_t* ray_cnt;    // [N]
  int64_t cap;
  const float* t_shift;  // [N] per-ray shift of the march steps (nerf_march_jitter), or null: the table as it is
};

// A ray's depth at step s: t_table[s], plus the ray's shift when there is one -- a separately
// rounded add, so a ray shifted by c marches the table t_table + c (rounded entry by entry)
// bit for bit.  Without a shift array there is no add at all.  Every read of the table in the
// march goes through this.  SHIFT is a template parameter of the march's kernels (the launches
// pick the instantiation by t_shift != null), not a test inside the walk: the unshifted kernels
// are the code they were before the shift existed.
template <bool SHIFT>
struct RayT {
  const float* table;
  float shift;
  __device__ __forceinline__ float operator()(int s) const {
    if constexpr (SHIFT) return fadd(table[s], shift);
    else return table[s];
  }
};
template <bool SHIFT>
__device__ __forceinline__ RayT<SHIFT> ray_t(const float* t_table, const float* t_shift, int64_t r) {
  if constexpr (SHIFT) return RayT<SHIFT>{t_table, t_shift[r]};
  else return RayT<SHIFT>{t_table, 0.f};
}

__device__ __forceinline__ bool march_occupied(const MarchGatherArgs& a, const float* ray, float t, float* p,
                                               int* cell) {
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = fadd(ray[k], fmul(t, ray[3 + k]));  // o + t * d
#pragma unroll
  for (int k = 0; k < 3; ++k) cell[k] = grid_axis(p[k], a.bb.mn[k], a.bb.mx[k], a.res);
  return a.grid[((int64_t)cell[0] * a.res + cell[1]) * a.res + cell[2]] != 0;
}

// Empty-cell skip (exact).  The step walk is latency-bound (one dependent grid lookup per
// 0.005 step, ~4.7 steps per cell).  After an EMPTY cell, the steps that provably map to the
// same cell are skipped: along each axis the cell index is a monotone function of p (clamp,
// subtract, divide, multiply, truncate: each monotone in fp32), so its preimage is an interval
// [lo, hi) -- within a few ulps of mn + i w, w = (mx - mn) / (res - 1), open-ended for the
// boundary cells that also hold the clamped outside -- and the computed p = o + t d is monotone
// in t.  Every step whose t is below the first exit of the interval SHRUNK by a margin m is
// therefore in the same empty cell, and is skipped; the walk resumes one step at a time near the
// boundary.  With a per-ray shift (RayT) the steps' depths are fadd(t_table[j], shift): adding a
// constant is monotone in fp32 too, so the shifted depths are still non-decreasing in j and every
// comparison below is made on them, never on the bare table.  m = max(1e-3 w, 2^-18 (|o| +
// t_abs |d| + |mn| + |mx|)), t_abs = max(8, |t| over the shifted table, i.e. at its ends) (a far
// bound past 8 widens the margin with the coordinates): 1e-3 w is ~2.4e-5 at res 128, but
// shrinks as 1/res (2.9e-6 at res 1024), while the fp32 errors of p = o + t d, of the interval
// bounds and of t_exit d are a few ulps of the coordinates' magnitude (~1e-6 for |o| ~ 4, t <= 6
// here): the absolute floor keeps the margin >= 8 such ulps at any resolution.  Returns the next
// step to test (> s).
//
// Two levels: when the whole 8^3 block of cells around an empty cell is empty (the macro grid,
// nerf_march_macro), the interval is the block's -- cells [8 j, 8 j + 7] along each axis, the
// same monotone argument over a union of cells -- so a ray crosses empty space ~8x faster (the
// walk is a chain of dependent lookups: its length, not the lookups, sets a round's gather time).
constexpr int MACRO = 8;
template <class TR>
__device__ __forceinline__ int march_skip_empty(const MarchGatherArgs& a, const TR& tr, const float* ray, int s,
                                                const int* cell, int span) {
  // fp32 with approximate reciprocals: the errors (~1e-6 in p) are far inside the margin.
  // |t| is bounded by the table's ends (it is monotone); 8 is the floor the bound was tested at
  const float t_abs = fmaxf(8.0f, fmaxf(fabsf(tr(0)), fabsf(tr(a.n_steps - 1))));
  float t_exit = 3.0e38f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float d = ray[3 + k];
    const float mn = a.bb.mn[k], w = (a.bb.mx[k] - mn) * (1.0f / (float)(a.res - 1));
    const float mag = fabsf(ray[k]) + t_abs * fabsf(d) + fabsf(mn) + fabsf(a.bb.mx[k]);
    const float m = fmaxf(1e-3f * w, mag * 3.814697265625e-6f);  // 2^-18
    const int lo = cell[k] / span * span, hi = min(lo + span - 1, a.res - 1);  // the interval's cells
    const float rd = __builtin_amdgcn_rcpf(d);
    if (d > 0.0f && hi < a.res - 1) {         // (at max, clamped: stays while p grows)
      t_exit = fminf(t_exit, (mn + (float)(hi + 1) * w - m - ray[k]) * rd);
    } else if (d < 0.0f && lo > 0) {          // (at min, clamped: stays while p falls)
      t_exit = fminf(t_exit, (mn + (float)lo * w + m - ray[k]) * rd);
    }
  }
  // last step j > s with t(j) < t_exit (steps are ~uniform: estimate, then correct)
  const float t0 = tr(s), t1 = tr(a.n_steps > s + 1 ? s + 1 : s);
  int j = s;
  if (t1 > t0 && t_exit > t1) {
    const float est = (t_exit - t0) * __builtin_amdgcn_rcpf(t1 - t0);
    j = s + (int)fminf(est, (float)(a.n_steps - 1 - s)) - 1;
    if (j < s) j = s;
    while (j + 1 < a.n_steps && tr(j + 1) < t_exit) ++j;
    while (j > s && tr(j) >= t_exit) --j;
  }
  return j + 1;
}

// the step after an empty cell: the macro block's exit when the block is empty, else the cell's
template <class TR>
__device__ __forceinline__ int march_next_after_empty(const MarchGatherArgs& a, const TR& tr, const float* ray,
                                                      int s, const int* cell) {
  int span = 1;
  if (a.macro) {
    const int mres = (a.res + MACRO - 1) / MACRO;
    const int64_t j = ((int64_t)(cell[0] / MACRO) * mres + cell[1] / MACRO) * mres + cell[2] / MACRO;
    if (a.macro[j] == 0) span = MACRO;
  }
  return march_skip_empty(a, tr, ray, s, cell, span);
}

// The march's one walk.  From step s: an occupied step goes to on_occupied(step) and counts into n,
// an empty one skips ahead, until n reaches `limit` or the table ends; s is left at the step the walk
// stopped at.  Every kernel that walks a ray does it here, so two walks of a ray from the same step
// visit the same steps.
template <class TR, class N, class F>
__device__ __forceinline__ void march_walk(const MarchGatherArgs& a, const TR& tr, const float* ray, int& s, N& n,
                                           N limit, F&& on_occupied) {
  float p[3];
  int cell[3];
  while (s < a.n_steps && n < limit) {
    if (march_occupied(a, ray, tr(s), p, cell)) {
      on_occupied(s);
      ++n;
      ++s;
    } else {
      s = march_next_after_empty(a, tr, ray, s, cell);
    }
  }
}

// the occupied steps a live ray gathers this round: a ray whose transmittance has already dropped
// is near its termination step, and gathering few steps for it wastes fewer speculative MLP
// evaluations (outputs are unchanged -- the compositor stops where the reference does, and an
// unfinished ray gathers again)
__device__ __forceinline__ int march_quota(const MarchGatherArgs& a, int64_t r) {
  return a.st.T[r] < a.t_split ? (a.k_low < a.K ? a.k_low : a.K) : a.K;
}

template <class TR>
__device__ __forceinline__ void march_put(const MarchGatherArgs& a, const TR& tr, int64_t r, const float* ray,
                                          int64_t at, int s) {
  float p[3];
  const float t = tr(s);
#pragma unroll
  for (int k = 0; k < 3; ++k) p[k] = fadd(ray[k], fmul(t, ray[3 + k]));  // = march_occupied's p
  a.out_ray[at] = (int32_t)r;
  a.out_step[at] = s;
  a.out_pts[at * 3 + 0] = p[0];
  a.out_pts[at * 3 + 1] = p[1];
  a.out_pts[at * 3 + 2] = p[2];
}

// Wave-aggregated reservation of every lane's cnt points (the whole wave calls this; `in`: the lane
// has a ray, `live`: it walked, to step s), with the round's counters and the ray's bookkeeping.
// Returns the ray's slot: its first nwrite points go to pos.. (nwrite = 0 on a lane that has nothing
// to write).
struct MarchSlot { int pos, nwrite; };
__device__ __forceinline__ MarchSlot march_reserve(const MarchGatherArgs& a, int64_t r, bool in, bool live, int cnt,
                                                   int s) {
  const int l = lane_id();
  const int incl = wave_scan_add_i(cnt);
  const int wtotal = __shfl(incl, 63, 64);
  int base = 0;
  if (l == 63 && wtotal > 0) {
    base = atomicAdd(&a.counters[0], wtotal);
    // the positions of this wave's reservation below cap are all written
    const int64_t below = a.cap - (int64_t)base;
    if (a.evaluated && below > 0) atomicAdd(a.evaluated, (unsigned long long)(below < wtotal ? below : wtotal));
  }
  base = __shfl(base, 63, 64);
  const unsigned long long live_mask = __ballot(live);
  if (l == 0 && live_mask) atomicAdd(&a.counters[1], __popcll(live_mask));
  if (!in) return {0, 0};
  if (!live) {
    a.ray_cnt[r] = 0;
    return {0, 0};
  }
  const int pos = base + incl - cnt;
  a.ray_off[r] = pos;
  // out of room: the ray keeps its position and gathers again next round.  The part of its
  // reservation below cap is still written (ray_cnt = -that many: not composited), so that
  // every position below min(points reserved, cap) holds a valid point and ray id -- the MLP
  // launch sized on the device (nerf_mlp_fwd_count) reads exactly that prefix.
  if ((int64_t)pos + cnt > a.cap) {
    const int64_t room = a.cap - (int64_t)pos;
    const int nwrite = (int)(room <= 0 ? 0 : room < cnt ? room : cnt);
    a.ray_cnt[r] = -nwrite;
    return {pos, nwrite};
  }
  a.ray_cnt[r] = cnt;
  a.st.exhausted[r] = (s >= a.n_steps) ? 1 : 0;
  a.st.next_step[r] = s;
  return {pos, cnt};
}

// Two-pass form, first pass: counts and reserves; march_emit_kernel walks again and writes.
template <bool SHIFT>
__global__ void march_gather_kernel(MarchGatherArgs a) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = r < a.N;
  const bool live = in && a.st.alive[r];
  int cnt = 0, s = live ? a.st.next_step[r] : 0;
  const float* ray = a.rays + (in ? r : 0) * 6;
  const RayT<SHIFT> tr = ray_t<SHIFT>(a.t_table, a.t_shift, in ? r : 0);
  if (live) march_walk(a, tr, ray, s, cnt, march_quota(a, r), [](int) {});
  march_reserve(a, r, in, live, cnt, s);
}

// Two-pass variant that keeps the start step: the gather kernel above records counts;
// this kernel writes the points.
struct MarchEmitArgs {
  MarchGatherArgs g;
  const int32_t* start_step;  // [N] step before the gather
};

template <bool SHIFT>
__global__ void march_emit_kernel(MarchEmitArgs e) {
  const MarchGatherArgs& a = e.g;
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.N) return;
  const int c = a.ray_cnt[r];
  const int cnt = c < 0 ? -c : c;  // (< 0: an overflowing ray's points below cap, written only)
  if (cnt == 0) return;
  const float* ray = a.rays + r * 6;
  const RayT<SHIFT> tr = ray_t<SHIFT>(a.t_table, a.t_shift, r);
  const int pos = a.ray_off[r];
  int s = e.start_step[r], k = 0;
  march_walk(a, tr, ray, s, k, cnt, [&](int at) { march_put(a, tr, r, ray, pos + k, at); });
}

// One-pass gather + emit (the default since round 3).  The two-pass form above walks every
// ray twice: once to count its points (the wave's reservation needs every lane's count
// first), once more, with every grid lookup again, to write them (the bf16 trained-net frame:
// 1.4 of 17 ms in emit).  Here the counting walk records where the points are -- as runs of
// consecutive occupied steps, up to MARCH_RUNS per lane in LDS (a run of an occupied cell is
// ~4.7 steps) plus the open one in registers -- and the points are written from the runs
// after the reservation, with no lookups.  A lane whose runs do not fit remembers where its
// first unrecorded run starts and walks again from there for the rest (the same walk: the
// same steps).  Outputs, counters and overflow handling are those of gather + emit.
constexpr int MARCH_RUNS = 16;
constexpr int MARCH_WAVES = 4;  // 256-thread blocks
template <bool SHIFT>
__global__ void __launch_bounds__(256) march_gather_emit_kernel(MarchGatherArgs a) {
  __shared__ uint32_t runs[MARCH_WAVES][MARCH_RUNS][64];  // (start << 16) | length, lane-minor
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int w = threadIdx.x >> 6, l = lane_id();
  const bool in = r < a.N;
  const bool live = in && a.st.alive[r];
  int cnt = 0, s = live ? a.st.next_step[r] : 0;
  const float* ray = a.rays + (in ? r : 0) * 6;
  const RayT<SHIFT> tr = ray_t<SHIFT>(a.t_table, a.t_shift, in ? r : 0);
  int nrun = 0, cur_start = 0, cur_len = 0;  // recorded runs; the open run
  int ovf_step = -1;                           // first unrecorded run's step
  if (live) {
    march_walk(a, tr, ray, s, cnt, march_quota(a, r), [&](int at) {
      if (ovf_step < 0) {
        if (cur_len > 0 && at == cur_start + cur_len && cur_len < 0xFFFF) {
          ++cur_len;
        } else {
          if (cur_len > 0) {
            if (nrun < MARCH_RUNS) {
              runs[w][nrun][l] = ((uint32_t)cur_start << 16) | (uint32_t)cur_len;
              ++nrun;
            } else {  // out of slots: the open run and everything after it are walked again
              ovf_step = cur_start;
            }
          }
          if (ovf_step < 0) {
            cur_start = at;
            cur_len = 1;
          }
        }
      }
    });
  }
  const MarchSlot slot = march_reserve(a, r, in, live, cnt, s);
  const int64_t pos = slot.pos;
  const int nwrite = slot.nwrite;
  // emit: the recorded runs, the open run, then (after a run overflow) the walk again
  int kk = 0;
  for (int i = 0; i < nrun && kk < nwrite; ++i) {
    const uint32_t ru = runs[w][i][l];
    const int st = (int)(ru >> 16), ln = (int)(ru & 0xFFFF);
    for (int j = 0; j < ln && kk < nwrite; ++j, ++kk) march_put(a, tr, r, ray, pos + kk, st + j);
  }
  if (ovf_step < 0) {
    for (int j = 0; j < cur_len && kk < nwrite; ++j, ++kk) march_put(a, tr, r, ray, pos + kk, cur_start + j);
  } else {
    march_walk(a, tr, ray, ovf_step, kk, nwrite, [&](int at) { march_put(a, tr, r, ray, pos + kk, at); });
  }
}

struct MarchCompArgs {
  const float* raw;  // [cap,4]
  const float* rays;
  int64_t N;
  const float* t_table;
  const int32_t* ray_off;
  const int32_t* ray_cnt;
  const int32_t* out_step;
  MarchState st;
  float step_size, t_thresh;
  unsigned long long* consumed;  // += points composited (the reference's MLP queries) or null
  int32_t* ray_used;             // [N] += this ray's points composited this round, or null
  const float* t_shift;          // [N] the gather's per-ray shift, or null
};

// step_size * |d|: the distance between two steps of ray r, for the round compositor and the
// segment compositors alike
__device__ __forceinline__ float ray_step_dist(const float* rays, int64_t r, float step_size) {
  const float* d = rays + r * 6 + 3;
  return fmul(step_size, sqrtf(fadd(fadd(fmul(d[0], d[0]), fmul(d[1], d[1])), fmul(d[2], d[2]))));
}

// Composites a ray's gathered points in step order and stops at T < t_thresh
// (volume_renderer.py:327-341).  Points gathered past that step were evaluated speculatively
// and are dropped; the points composited are exactly the reference's queries (:324).  Returns
// their number.
template <bool SHIFT>
__device__ __forceinline__ int march_composite_ray(const MarchCompArgs& a, int64_t r) {
  const int c = a.ray_cnt[r], off = a.ray_off[r];
  const int cnt = c > 0 ? c : 0;  // (< 0: gathered nothing this round, see march_reserve)
  const RayT<SHIFT> tr = ray_t<SHIFT>(a.t_table, a.t_shift, r);
  const float dist = ray_step_dist(a.rays, r, a.step_size);
  float T = a.st.T[r];
  float cr = a.st.rgb[r * 3 + 0], cg = a.st.rgb[r * 3 + 1], cb = a.st.rgb[r * 3 + 2];
  float dep = a.st.depth[r], acc = a.st.acc[r];
  bool alive = true;
  int used = cnt;
  for (int k = 0; k < cnt; ++k) {
    const float4 rw = *(const float4*)(a.raw + (int64_t)(off + k) * 4);
    const float t = tr(a.out_step[off + k]);
    const float sr = 1.f / (1.f + expf(-rw.x)), sg = 1.f / (1.f + expf(-rw.y)), sb = 1.f / (1.f + expf(-rw.z));
    const float sigma = rw.w > 0.f ? rw.w : 0.f;
    const float alpha = fsub(1.f, expf(-fmul(sigma, dist)));
    const float ta = fmul(T, alpha);
    cr = fadd(cr, fmul(ta, sr));
    cg = fadd(cg, fmul(ta, sg));
    cb = fadd(cb, fmul(ta, sb));
    acc = fadd(acc, ta);
    dep = fadd(dep, fmul(ta, t));
    T = fmul(T, fsub(1.f, alpha));
    if (T < a.t_thresh) {
      alive = false;
      used = k + 1;
      break;
    }
  }
  a.st.T[r] = T;
  a.st.rgb[r * 3 + 0] = cr;
  a.st.rgb[r * 3 + 1] = cg;
  a.st.rgb[r * 3 + 2] = cb;
  a.st.depth[r] = dep;
  a.st.acc[r] = acc;
  if (!alive || a.st.exhausted[r]) a.st.alive[r] = 0;
  return used;
}

// one thread per ray; the points composited are counted into `consumed` and `ray_used`
template <bool SHIFT>
__global__ void march_composite_kernel(MarchCompArgs a) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = r < a.N && a.st.alive[r];
  int used = 0;
  if (live) used = march_composite_ray<SHIFT>(a, r);
  if (a.ray_used && live) a.ray_used[r] += used;
  if (a.consumed) {
    // wave-aggregated count
    int tot = used;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
    if (lane_id() == 0 && tot) atomicAdd(a.consumed, (unsigned long long)tot);
  }
}

// macro occupancy: block (i, j, k) = cells [8 i, 8 i + 8) x [8 j, ..) x [8 k, ..) (clipped at res)
__global__ void march_macro_kernel(const uint8_t* grid, int res, uint8_t* macro) {
  const int mres = (res + MACRO - 1) / MACRO;
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= (int64_t)mres * mres * mres) return;
  const int bi = (int)(b / ((int64_t)mres * mres)), bj = (int)((b / mres) % mres), bk = (int)(b % mres);
  uint8_t any = 0;
  for (int i = bi * MACRO; i < min(bi * MACRO + MACRO, res); ++i)
    for (int j = bj * MACRO; j < min(bj * MACRO + MACRO, res); ++j)
      for (int k = bk * MACRO; k < min(bk * MACRO + MACRO, res); ++k) any |= grid[((int64_t)i * res + j) * res + k];
  macro[b] = any ? 1 : 0;
}

// Jittered steps (training): one shift per ray, uniform in [0, step_size), from the Philox stream
// the stratified sampler draws from (counter = ray, offset; key = seed).  u <= 1 - 2^-24, so the
// rounded product stays below step_size and a shifted ray still samples inside [near, far).  Its
// own launch: both passes of the differentiable march read the same array, and a test can
// inject one.
__global__ void march_jitter_kernel(int64_t N, float step_size, uint64_t seed, uint64_t offset, float* t_shift) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= N) return;
  t_shift[r] = fmul(rng_uniform(seed, offset, (uint64_t)r), step_size);
}

struct MarchInitArgs { MarchState st; int64_t N; };
__global__ void march_init_kernel(MarchInitArgs a) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.N) return;
  a.st.T[r] = 1.f;
  a.st.rgb[r * 3 + 0] = a.st.rgb[r * 3 + 1] = a.st.rgb[r * 3 + 2] = 0.f;
  a.st.depth[r] = 0.f;
  a.st.acc[r] = 0.f;
  a.st.next_step[r] = 0;
  a.st.alive[r] = 1;
  a.st.exhausted[r] = 0;
}

struct MarchFinishArgs { MarchState st; int64_t N; int white; };
__global__ void march_finish_kernel(MarchFinishArgs a) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.N || !a.white) return;
  const float bg = fsub(1.f, a.st.acc[r]);  // rgb += (1 - acc) * 1
#pragma unroll
  for (int k = 0; k < 3; ++k) a.st.rgb[r * 3 + k] = fadd(a.st.rgb[r * 3 + k], bg);
}

// ------------------------------------------------------------------------------------
// differentiable march: per-ray segments (the training step through the grid)
// ------------------------------------------------------------------------------------
// The march above decides, without gradient, how many points each ray composites (ray_used).
// The three kernels below run the differentiable pass over exactly those points: every ray's
// points laid out contiguously in ray order (segment r = [seg_off[r], seg_off[r+1]), the
// exclusive prefix sum of the counts -- no atomic reservation, so the sample order, and with it
// the dW sum order, is the same run to run), composited with no termination test.

// One thread per ray: the gather's walk from step 0 (same skips, same points), the ray's first
// seg_off[r+1] - seg_off[r] occupied steps written at seg_off[r].  A ray with fewer occupied
// steps than its count gets step -1 and its origin in the surplus positions.
template <bool SHIFT>
__global__ void march_segments_kernel(MarchGatherArgs a, const int32_t* seg_off) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.N) return;
  const int64_t pos = seg_off[r];
  const int64_t cnt = (int64_t)seg_off[r + 1] - pos;
  const float* ray = a.rays + r * 6;
  const RayT<SHIFT> tr = ray_t<SHIFT>(a.t_table, a.t_shift, r);
  int64_t k = 0;
  int s = 0;
  march_walk(a, tr, ray, s, k, cnt, [&](int at) { march_put(a, tr, r, ray, pos + k, at); });
  for (; k < cnt; ++k) {
    a.out_ray[pos + k] = (int32_t)r;
    a.out_step[pos + k] = -1;
    a.out_pts[(pos + k) * 3 + 0] = ray[0];
    a.out_pts[(pos + k) * 3 + 1] = ray[1];
    a.out_pts[(pos + k) * 3 + 2] = ray[2];
  }
}

struct SegCompArgs {
  const float* raw;  // [M,4]
  const float* rays;
  int64_t N;
  const float* t_table;
  const int32_t* seg_off;   // [N+1]
  const int32_t* out_step;  // [M] (< 0: a surplus point, weight 0)
  float step_size;
  int white;
  // (an entry point sets what its kernel reads of the rest)
  float* rgb = nullptr;    // forward outputs
  float* depth = nullptr;
  float* acc = nullptr;
  const float* g_rgb = nullptr;  // backward inputs (each nullable = 0)
  const float* g_depth = nullptr;
  const float* g_acc = nullptr;
  float* g_raw = nullptr;  // [M,4]
  const float* t_shift = nullptr;  // [N] the walk's per-ray shift, or null
  // the distortion term (the DIST instantiations alone read these)
  float inv_range = 0.f;        // 1 / (far - near)
  float* dist = nullptr;            // [N] forward output
  double* totals = nullptr;         // [N,2] forward output: the ray's (sum w, sum w t)
  const float* g_dist = nullptr;    // [N] backward input (nullable = 0)
  const double* totals_in = nullptr;  // [N,2] backward input: what the forward wrote
  // the per-ray background colour (the BG instantiations alone read it)
  const float* bg = nullptr;  // [N,3]
};

constexpr int SEG_WAVES = 4;  // rays (waves) per 256-thread block

// alpha of the point at k (lane-private); 0 for a lane past the segment or a surplus point
__device__ __forceinline__ float seg_alpha(const SegCompArgs& a, int64_t k, int64_t end, float dist, int* step) {
  *step = k < end ? a.out_step[k] : -1;
  if (*step < 0) return 0.f;
  const float s = a.raw[k * 4 + 3];
  const float sigma = s > 0.f ? s : 0.f;
  return fsub(1.f, expf(-fmul(sigma, dist)));
}

__device__ __forceinline__ double wave_prod_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v *= __shfl_xor(v, o, 64);
  return v;
}

// prod (1 - alpha) over the 64 points from b (a chunk's transmittance factor; wave-uniform)
__device__ __forceinline__ double seg_chunk_prod(const SegCompArgs& a, int64_t b, int64_t end, float dist) {
  int st;
  const float alpha = seg_alpha(a, b + lane_id(), end, dist, &st);
  return wave_prod_d((double)fsub(1.f, alpha));
}

__device__ __forceinline__ float seg_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// One wave per ray, lanes on consecutive points (raw read as coalesced float4), 64 points a chunk:
// T_k = T_in * prod_{j<k in chunk} (1 - alpha_j) by a product scan across the lanes (in double, as
// the compositor of render()), T_in carried from chunk to chunk; every point of the segment is used.
//
// DIST adds the distortion of the ray's weights (Mip-NeRF 360, on depths normalised by the march's
// range): dist = inv_range (sum_i sum_j w_i w_j |t_i - t_j| + step_size / 3 sum_i w_i^2).  The steps of
// a segment increase, so the double sum is 2 sum_i w_i (t_i Wex_i - Sex_i) with the exclusive prefixes
// Wex_i = sum_{j<i} w_j, Sex_i = sum_{j<i} w_j t_j: two more add scans across the lanes per chunk, in
// double, their totals carried from chunk to chunk like T_in.  The ray's totals (W, S) go out for the
// backward.  DIST is a template parameter like SHIFT: without it the kernel is the code it was.
//
// BG composites onto the ray's own colour bg[r] instead of white: rgb += (1 - acc) * bg[r], whatever
// `white` says.  A third template parameter, for the same reason.
template <bool SHIFT, bool DIST, bool BG>
__global__ void __launch_bounds__(64 * SEG_WAVES) march_seg_fwd_kernel(SegCompArgs a) {
  const int64_t r = (int64_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
  if (r >= a.N) return;  // (wave-uniform)
  const int l = lane_id();
  const int64_t beg = a.seg_off[r], end = a.seg_off[r + 1];
  const float dist = ray_step_dist(a.rays, r, a.step_size);
  const RayT<SHIFT> tr = ray_t<SHIFT>(a.t_table, a.t_shift, r);
  double Tin = 1.0, sr = 0.0, sg = 0.0, sb = 0.0, sd = 0.0, sa = 0.0;
  double Wc = 0.0, Sc = 0.0, sx = 0.0;  // DIST: sum w, sum w t over the chunks before; this lane's share of dist
  for (int64_t b = beg; b < end; b += 64) {
    const int64_t k = b + l;
    int st;
    const float alpha = seg_alpha(a, k, end, dist, &st);
    const double P = wave_scan_mul((double)fsub(1.f, alpha));
    double Pex = __shfl_up(P, 1, 64);
    if (l == 0) Pex = 1.0;
    double wd = 0.0, td = 0.0;  // DIST: this lane's weight and depth (0 past the segment and on a surplus point)
    if (st >= 0) {
      const float4 rw = *(const float4*)(a.raw + k * 4);
      const double w = Tin * Pex * (double)alpha;
      sr += w * (double)seg_sigmoid(rw.x);
      sg += w * (double)seg_sigmoid(rw.y);
      sb += w * (double)seg_sigmoid(rw.z);
      sd += w * (double)tr(st);
      sa += w;
      if constexpr (DIST) {
        wd = w;
        td = (double)tr(st);
      }
    }
    if constexpr (DIST) {
      const double w = wd, t = td, wt = w * t;
      const double Wi = wave_scan_add(w), Si = wave_scan_add(wt);  // inclusive, within the chunk
      const double Wex = Wc + (Wi - w), Sex = Sc + (Si - wt);
      sx += w * (2.0 * (t * Wex - Sex) + (double)a.step_size * (1.0 / 3.0) * w);
      Wc += shfl_d(Wi, 63);
      Sc += shfl_d(Si, 63);
    }
    Tin *= shfl_d(P, 63);
  }
  sr = wave_sum_d(sr);
  sg = wave_sum_d(sg);
  sb = wave_sum_d(sb);
  sd = wave_sum_d(sd);
  sa = wave_sum_d(sa);
  if (l == 0) {
    const float acc = (float)sa;
    if constexpr (BG) {
      const float left = fsub(1.f, acc);  // rgb += (1 - acc) * bg[r]
      a.rgb[r * 3 + 0] = fadd((float)sr, fmul(left, a.bg[r * 3 + 0]));
      a.rgb[r * 3 + 1] = fadd((float)sg, fmul(left, a.bg[r * 3 + 1]));
      a.rgb[r * 3 + 2] = fadd((float)sb, fmul(left, a.bg[r * 3 + 2]));
    } else {
      const float bg = a.white ? fsub(1.f, acc) : 0.f;  // rgb += (1 - acc) * 1
      a.rgb[r * 3 + 0] = fadd((float)sr, bg);
      a.rgb[r * 3 + 1] = fadd((float)sg, bg);
      a.rgb[r * 3 + 2] = fadd((float)sb, bg);
    }
    a.depth[r] = (float)sd;
    a.acc[r] = acc;
  }
  if constexpr (DIST) {
    sx = wave_sum_d(sx);
    if (l == 0) {
      a.dist[r] = (float)((double)a.inv_range * sx);
      a.totals[r * 2 + 0] = Wc;
      a.totals[r * 2 + 1] = Sc;
    }
  }
}

// Backward, division-free.  With v_k = g_rgb . c_k + g_depth t_k + g_acc' (g_acc' = g_acc - sum g_rgb
// on a white background) and R_k = sum_{j>k} w_j v_j / T_{k+1}, obtained without the division from
// R_last = 0, R_{k-1} = alpha_k v_k + (1 - alpha_k) R_k:  dL/dalpha_k = T_k (v_k - R_k), dL/dc_k = w_k g_rgb.
// R is a suffix composition of the affine maps x -> alpha_k v_k + (1 - alpha_k) x: a scan across the
// lanes per chunk, the chunks walked in reverse with R carried.  The chunks' entry transmittances
// come from a forward pre-pass and live in registers: lane j holds chunk j's (the first 64 chunks,
// 4096 points: every ray of an 800-step march) and super-chunk j's (64 chunks each); a later
// super-chunk's chunk entries are recomputed from its own entry when the reverse walk reaches it.
// alpha_k = 1 (exp underflow) zeroes T from k + 1 on: every later gradient is exactly 0, no 0/0.
//
// DIST: v_k gains g_dist d dist / d w_k = g_dist inv_range (2 [(t_k Wex_k - Sex_k) + (Ssuf_k - t_k Wsuf_k)]
// + 2/3 step_size w_k), Wsuf / Ssuf the sums over the points after k.  The reverse walk carries the
// suffix sums of w and w t over the chunks behind it next to C; within a chunk two add scans across the
// lanes give the rest, and a point's exclusive prefix is the forward's saved total minus its inclusive
// suffix, all in double.  No second pre-pass, no state per chunk.
//
// BG: g_acc' = g_acc - g_rgb . bg[r] (the colour is a constant of the step: no gradient of its own).
template <bool SHIFT, bool DIST, bool BG>
__global__ void __launch_bounds__(64 * SEG_WAVES) march_seg_bwd_kernel(SegCompArgs a) {
  const int64_t r = (int64_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
  if (r >= a.N) return;  // (wave-uniform)
  const int l = lane_id();
  const int64_t beg = a.seg_off[r], end = a.seg_off[r + 1];
  if (end <= beg) return;
  const float dist = ray_step_dist(a.rays, r, a.step_size);
  const RayT<SHIFT> tr = ray_t<SHIFT>(a.t_table, a.t_shift, r);
  const double gr = a.g_rgb ? (double)a.g_rgb[r * 3 + 0] : 0.0, gg = a.g_rgb ? (double)a.g_rgb[r * 3 + 1] : 0.0,
               gb = a.g_rgb ? (double)a.g_rgb[r * 3 + 2] : 0.0;
  const double gd = a.g_depth ? (double)a.g_depth[r] : 0.0;
  double gbg;  // g_rgb . background
  if constexpr (BG)
    gbg = gr * (double)a.bg[r * 3 + 0] + gg * (double)a.bg[r * 3 + 1] + gb * (double)a.bg[r * 3 + 2];
  else
    gbg = a.white ? gr + gg + gb : 0.0;
  const double ga = (a.g_acc ? (double)a.g_acc[r] : 0.0) - gbg;
  const int64_t nchunks = (end - beg + 63) / 64, nsuper = (nchunks + 63) / 64;
  double chunkT = 1.0, superT = 1.0;
  {
    double T = 1.0;
    for (int64_t c = 0; c < nchunks; ++c) {
      if (c < 64 && l == (int)c) chunkT = T;
      if ((c & 63) == 0 && (c >> 6) < 64 && l == (int)(c >> 6)) superT = T;
      if (c + 1 < nchunks) T *= seg_chunk_prod(a, beg + c * 64, end, dist);
    }
  }
  double C = 0.0;  // R at the last point of the chunk in hand
  double Wsc = 0.0, Ssc = 0.0, Wtot = 0.0, Stot = 0.0, gx = 0.0;  // DIST: sums over the chunks after; the ray's totals
  if constexpr (DIST) {
    Wtot = a.totals_in[r * 2 + 0];
    Stot = a.totals_in[r * 2 + 1];
    gx = (a.g_dist ? (double)a.g_dist[r] : 0.0) * (double)a.inv_range;
  }
  for (int64_t sc = nsuper - 1; sc >= 0; --sc) {
    const int64_t c0 = sc * 64, c1 = c0 + 64 < nchunks ? c0 + 64 : nchunks;
    double cT = chunkT;  // lane j: T entering chunk c0 + j
    if (sc > 0) {
      double T = 1.0;
      if (sc < 64) {
        T = shfl_d(superT, (int)sc);
      } else {
        for (int64_t c = 0; c < c0; ++c) T *= seg_chunk_prod(a, beg + c * 64, end, dist);
      }
      for (int64_t c = c0; c < c1; ++c) {
        if (l == (int)(c - c0)) cT = T;
        if (c + 1 < c1) T *= seg_chunk_prod(a, beg + c * 64, end, dist);
      }
    }
    for (int64_t c = c1 - 1; c >= c0; --c) {
      const double Tin = shfl_d(cT, (int)(c - c0));
      const int64_t k = beg + c * 64 + l;
      int st;
      const float alpha = seg_alpha(a, k, end, dist, &st);
      const float om = fsub(1.f, alpha);
      const double P = wave_scan_mul((double)om);
      double Pex = __shfl_up(P, 1, 64);
      if (l == 0) Pex = 1.0;
      float4 rw = make_float4(0.f, 0.f, 0.f, 0.f);
      float cx = 0.f, cy = 0.f, cz = 0.f;
      double v = 0.0;
      if (st >= 0) {
        rw = *(const float4*)(a.raw + k * 4);
        cx = seg_sigmoid(rw.x);
        cy = seg_sigmoid(rw.y);
        cz = seg_sigmoid(rw.z);
        v = gr * (double)cx + gg * (double)cy + gb * (double)cz + gd * (double)tr(st) + ga;
      }
      if constexpr (DIST) {
        double w = 0.0, t = 0.0;
        if (st >= 0) {
          w = Tin * Pex * (double)alpha;
          t = (double)tr(st);
        }
        const double wt = w * t;
        const double Wi = wave_scan_add(w), Si = wave_scan_add(wt);  // inclusive, within the chunk
        const double Wct = shfl_d(Wi, 63), Sct = shfl_d(Si, 63);
        const double Wsuf = Wsc + (Wct - Wi), Ssuf = Ssc + (Sct - Si);  // over the points after this one
        const double Wex = Wtot - (Wsuf + w), Sex = Stot - (Ssuf + wt);
        if (st >= 0)
          v += gx * (2.0 * ((t * Wex - Sex) + (Ssuf - t * Wsuf)) + (double)a.step_size * (2.0 / 3.0) * w);
        Wsc += Wct;
        Ssc += Sct;
      }
      // suffix composition: (A, B) of lane i = f_i o f_{i+1} o ... o f_63, f_j(x) = alpha_j v_j + (1 - alpha_j) x
      double A = (double)alpha * v, B = (double)om;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double An = __shfl_down(A, o, 64), Bn = __shfl_down(B, o, 64);
        if (l + o < 64) {
          A += B * An;
          B *= Bn;
        }
      }
      const double An = __shfl_down(A, 1, 64), Bn = __shfl_down(B, 1, 64);
      const double R = l == 63 ? C : An + Bn * C;
      C = shfl_d(A, 0) + shfl_d(B, 0) * C;
      if (k < end) {
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (st >= 0) {
          const double T = Tin * Pex, w = T * (double)alpha;
          const double dalpha = T * (v - R);
          g.x = (float)(w * gr * (double)(cx * (1.f - cx)));
          g.y = (float)(w * gg * (double)(cy * (1.f - cy)));
          g.z = (float)(w * gb * (double)(cz * (1.f - cz)));
          g.w = rw.w > 0.f ? (float)(dalpha * (double)dist * (double)om) : 0.f;
        }
        *(float4*)(a.g_raw + k * 4) = g;
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// point budget: pass A's per-ray counts -> pass B's segment offsets, cut at a point budget
// ------------------------------------------------------------------------------------
// P[r] = sum_{q<r} used[q] (64-bit), n_keep = the largest r with P[r] <= budget, m_keep = P[n_keep];
// seg_off[r] = P[r] up to n_keep and m_keep after it, so the rays past the cut own empty segments.
// One workgroup walks the array in tiles of its size and carries the prefix: lanes scan within a
// wave, the wave totals go through LDS.  No workgroup waits on another (there is only one), the
// loads and stores are coalesced, and at the ray counts of a training step the launch is all it
// costs.  Every value stored is <= budget <= INT32_MAX.
constexpr int BUDGET_THREADS = 1024;
constexpr int BUDGET_WAVES = BUDGET_THREADS / WAVE;

__global__ void __launch_bounds__(BUDGET_THREADS) march_budget_kernel(const int32_t* __restrict__ used, int64_t N,
                                                                      long long budget, int32_t* __restrict__ seg_off,
                                                                      int64_t* __restrict__ keep) {
  __shared__ long long wave_tot[BUDGET_WAVES];
  __shared__ long long cut[2];  // {n_keep, m_keep}; n_keep < 0: every ray so far fits
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
  if (tid == 0) {
    seg_off[0] = 0;
    cut[0] = -1;
    cut[1] = 0;
  }
  __syncthreads();
  long long carry = 0;  // P[base] <= budget
  int64_t base = 0;
  bool found = false;
  for (; base < N && !found; base += BUDGET_THREADS) {
    const int64_t r = base + tid;
    const long long v = r < N ? (long long)used[r] : 0;
    const long long inc = wave_scan_add_i64(v);
    if (lane == WAVE - 1) wave_tot[w] = inc;
    __syncthreads();
    long long pre = carry, tot = 0;
#pragma unroll
    for (int k = 0; k < BUDGET_WAVES; ++k) {
      const long long t = wave_tot[k];
      if (k < w) pre += t;
      tot += t;
    }
    const long long hi = pre + inc, lo = hi - v;  // P[r+1], P[r]
    // the counts are >= 0, so P is monotone and at most one ray straddles the budget: the first dropped one
    if (r < N && hi > budget && lo <= budget) {
      cut[0] = r;
      cut[1] = lo;
    }
    __syncthreads();  // (also orders this tile's reads of wave_tot before the next tile's writes)
    found = cut[0] >= 0;
    if (r < N) seg_off[r + 1] = (int32_t)(hi <= budget ? hi : cut[1]);
    carry += tot;
  }
  if (found) {  // the tiles after the cut: m_keep everywhere, the counts are not read
    const int32_t m = (int32_t)cut[1];
    for (int64_t r = base + tid; r < N; r += BUDGET_THREADS) seg_off[r + 1] = m;
  }
  if (tid == 0) {
    keep[0] = found ? cut[0] : N;
    keep[1] = found ? cut[1] : carry;
  }
}

}  // namespace nerf

// ======================================================================================
// C-ABI
// ======================================================================================
using namespace nerf;

// f(std::true_type) or f(std::false_type): how a launch picks the SHIFT (t_shift != null) or DIST
// instantiation of a kernel template from a run-time flag
template <class F>
static void pick(bool flag, F&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}
#define MARCH_LAUNCH_SHIFT(kernel, t_shift, grid, stream, ...)                                        \
  pick((t_shift) != nullptr, [&](auto S) {                                                            \
    hipLaunchKernelGGL(kernel<decltype(S)::value>, grid, dim3(256), 0, stream, __VA_ARGS__);          \
  })

extern "C" {

// state: T, rgb[3], depth, acc (f32) ; next_step (i32) ; alive, exhausted (u8)
int nerf_march_init(float* T, float* rgb, float* depth, float* acc, int32_t* next_step, uint8_t* alive,
                    uint8_t* exhausted, int64_t N, hipStream_t stream) {
  if (N == 0) return 0;
  NERF_REQUIRE(T && rgb && depth && acc && next_step && alive && exhausted, "nerf_march_init: null pointer");
  MarchInitArgs a{{T, rgb, depth, acc, next_step, alive, exhausted}, N};
  hipLaunchKernelGGL(march_init_kernel, grid1(N), dim3(256), 0, stream, a);
  return check_launch("nerf_march_init");
}

int64_t nerf_march_macro_bytes(int res) {
  if (res <= 1) return -1;
  const int64_t m = (res + MACRO - 1) / MACRO;
  return m * m * m;
}

int nerf_march_macro(const uint8_t* grid, int res, uint8_t* macro, hipStream_t stream) {
  NERF_REQUIRE(res > 1, "nerf_march_macro: bad res");
  NERF_REQUIRE(grid && macro, "nerf_march_macro: null pointer");
  hipLaunchKernelGGL(march_macro_kernel, grid1(nerf_march_macro_bytes(res)), dim3(256), 0, stream, grid, res, macro);
  return check_launch("nerf_march_macro");
}

int nerf_march_jitter(int64_t N, float step_size, uint64_t seed, uint64_t offset, float* t_shift,
                      hipStream_t stream) {
  NERF_REQUIRE(N >= 0, "nerf_march_jitter: N must be >= 0, got %lld", (long long)N);
  if (N == 0) return 0;
  NERF_REQUIRE(t_shift, "nerf_march_jitter: t_shift is null");
  hipLaunchKernelGGL(march_jitter_kernel, grid1(N), dim3(256), 0, stream, N, step_size, seed, offset, t_shift);
  return check_launch("nerf_march_jitter");
}

// The *_shift entry points take the per-ray shift of the march steps (t_shift [N], or null: the
// table as it is); the entry points without it forward a null shift.
//
// counters[0] = points reserved, counters[1] = rays alive entering this round (zero them first);
// evaluated (nullable) += the points written, min(points reserved, cap).
// start_step_scratch: [N] int32 workspace of the two-pass form (gather, then emit walking again),
// or null: the one-pass form (march_gather_emit_kernel, the default).
int nerf_march_gather_shift(const float* rays, int64_t N, const float* t_table, int n_steps, const uint8_t* grid,
                            int res, const uint8_t* macro, const float* bbox_host, int K, int k_low, float t_split,
                            float* T, float* rgb, float* depth, float* acc, int32_t* next_step, uint8_t* alive,
                            uint8_t* exhausted, int32_t* counters, unsigned long long* evaluated,
                            int32_t* start_step_scratch, int32_t* out_ray, int32_t* out_step, float* out_pts,
                            int32_t* ray_off, int32_t* ray_cnt, int64_t cap, const float* t_shift,
                            hipStream_t stream) {
  NERF_REQUIRE(N >= 0 && n_steps >= 0 && K > 0 && res > 1 && bbox_host, "nerf_march_gather: bad arguments");
  NERF_REQUIRE(cap >= K && cap <= INT32_MAX, "nerf_march_gather: need K <= cap <= INT32_MAX (point offsets are int32)");
  if (N == 0) return 0;
  NERF_REQUIRE(k_low > 0, "nerf_march_gather: k_low must be > 0");
  MarchGatherArgs a{rays, N, t_table, n_steps, grid, res, macro, make_bbox(bbox_host), K, k_low, t_split,
                    {T, rgb, depth, acc, next_step, alive, exhausted},
                    counters, evaluated, out_ray, out_step, out_pts, ray_off, ray_cnt, cap, t_shift};
  if (!start_step_scratch) {  // one pass: gather + emit fused (march_gather_emit_kernel)
    NERF_REQUIRE(n_steps < 65536, "nerf_march_gather: the one-pass form needs n_steps < 65536 (16-bit run starts)");
    MARCH_LAUNCH_SHIFT(march_gather_emit_kernel, t_shift, grid1(N), stream, a);
    return check_launch("nerf_march_gather");
  }
  if (hipMemcpyAsync(start_step_scratch, next_step, N * sizeof(int32_t), hipMemcpyDeviceToDevice, stream) !=
      hipSuccess) {
    set_error("nerf_march_gather: hipMemcpyAsync failed");
    return -5;
  }
  MARCH_LAUNCH_SHIFT(march_gather_kernel, t_shift, grid1(N), stream, a);
  if (int e = check_launch("nerf_march_gather")) return e;
  MarchEmitArgs em{a, start_step_scratch};
  MARCH_LAUNCH_SHIFT(march_emit_kernel, t_shift, grid1(N), stream, em);
  return check_launch("nerf_march_emit");
}

int nerf_march_gather(const float* rays, int64_t N, const float* t_table, int n_steps, const uint8_t* grid, int res,
                      const uint8_t* macro, const float* bbox_host, int K, int k_low, float t_split, float* T,
                      float* rgb, float* depth,
                      float* acc,
                      int32_t* next_step, uint8_t* alive, uint8_t* exhausted, int32_t* counters,
                      unsigned long long* evaluated, int32_t* start_step_scratch, int32_t* out_ray, int32_t* out_step,
                      float* out_pts, int32_t* ray_off, int32_t* ray_cnt, int64_t cap, hipStream_t stream) {
  return nerf_march_gather_shift(rays, N, t_table, n_steps, grid, res, macro, bbox_host, K, k_low, t_split, T, rgb,
                                 depth, acc, next_step, alive, exhausted, counters, evaluated, start_step_scratch,
                                 out_ray, out_step, out_pts, ray_off, ray_cnt, cap, nullptr, stream);
}

int nerf_march_composite_shift(const float* raw, const float* rays, int64_t N, const float* t_table,
                               const int32_t* ray_off, const int32_t* ray_cnt, const int32_t* out_step, float* T,
                               float* rgb, float* depth, float* acc, int32_t* next_step, uint8_t* alive,
                               uint8_t* exhausted, float step_size, float t_thresh, unsigned long long* consumed,
                               int32_t* ray_used, const float* t_shift, hipStream_t stream) {
  if (N == 0) return 0;
  MarchCompArgs a{raw, rays, N, t_table, ray_off, ray_cnt, out_step,
                  {T, rgb, depth, acc, next_step, alive, exhausted}, step_size, t_thresh, consumed, ray_used, t_shift};
  MARCH_LAUNCH_SHIFT(march_composite_kernel, t_shift, grid1(N), stream, a);
  return check_launch("nerf_march_composite");
}

int nerf_march_composite_used(const float* raw, const float* rays, int64_t N, const float* t_table,
                              const int32_t* ray_off, const int32_t* ray_cnt, const int32_t* out_step, float* T,
                              float* rgb, float* depth, float* acc, int32_t* next_step, uint8_t* alive,
                              uint8_t* exhausted, float step_size, float t_thresh, unsigned long long* consumed,
                              int32_t* ray_used, hipStream_t stream) {
  return nerf_march_composite_shift(raw, rays, N, t_table, ray_off, ray_cnt, out_step, T, rgb, depth, acc, next_step,
                                    alive, exhausted, step_size, t_thresh, consumed, ray_used, nullptr, stream);
}

int nerf_march_composite(const float* raw, const float* rays, int64_t N, const float* t_table, const int32_t* ray_off,
                         const int32_t* ray_cnt, const int32_t* out_step, float* T, float* rgb, float* depth,
                         float* acc, int32_t* next_step, uint8_t* alive, uint8_t* exhausted, float step_size,
                         float t_thresh, unsigned long long* consumed, hipStream_t stream) {
  return nerf_march_composite_used(raw, rays, N, t_table, ray_off, ray_cnt, out_step, T, rgb, depth, acc, next_step,
                                   alive, exhausted, step_size, t_thresh, consumed, nullptr, stream);
}

int nerf_march_segments_shift(const float* rays, int64_t N, const float* t_table, int n_steps, const uint8_t* grid,
                              int res, const uint8_t* macro, const float* bbox_host, const int32_t* seg_off,
                              int32_t* out_ray, int32_t* out_step, float* out_pts, const float* t_shift,
                              hipStream_t stream) {
  NERF_REQUIRE(N >= 0 && n_steps >= 0 && res > 1 && bbox_host, "nerf_march_segments: bad arguments");
  NERF_REQUIRE(n_steps < 65536, "nerf_march_segments: needs n_steps < 65536 (the one-pass march's step range)");
  NERF_REQUIRE(seg_off, "nerf_march_segments: seg_off is null");
  if (N == 0) return 0;
  NERF_REQUIRE(rays && grid && (t_table || n_steps == 0), "nerf_march_segments: null pointer");
  MarchGatherArgs a{rays, N, t_table, n_steps, grid, res, macro, make_bbox(bbox_host), 0, 0, 0.f,
                    {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr},
                    nullptr, nullptr, out_ray, out_step, out_pts, nullptr, nullptr, 0, t_shift};
  MARCH_LAUNCH_SHIFT(march_segments_kernel, t_shift, grid1(N), stream, a, seg_off);
  return check_launch("nerf_march_segments");
}

int nerf_march_segments(const float* rays, int64_t N, const float* t_table, int n_steps, const uint8_t* grid, int res,
                        const uint8_t* macro, const float* bbox_host, const int32_t* seg_off, int32_t* out_ray,
                        int32_t* out_step, float* out_pts, hipStream_t stream) {
  return nerf_march_segments_shift(rays, N, t_table, n_steps, grid, res, macro, bbox_host, seg_off, out_ray, out_step,
                                   out_pts, nullptr, stream);
}

// The segment compositors (forward / backward, plain / with the distortion term, white / a colour
// per ray) check and launch here.  `name` is the entry point's: it heads every message.  `a` holds what the entry point
// was given, null elsewhere.
static int seg_composite(const char* name, bool bwd, bool dist, const SegCompArgs& a, hipStream_t stream) {
  NERF_REQUIRE(a.N >= 0, "%s: N must be >= 0", name);
  NERF_REQUIRE(a.seg_off, "%s: seg_off is null", name);
  if (dist)
    NERF_REQUIRE(std::isfinite(a.inv_range) && a.inv_range > 0.f, "%s: inv_range must be finite and > 0, got %g", name,
                 (double)a.inv_range);
  if (a.N == 0) return 0;
  if (dist && !bwd) NERF_REQUIRE(a.dist, "%s: dist is null", name);
  if (dist) NERF_REQUIRE(bwd ? (const void*)a.totals_in : (const void*)a.totals, "%s: totals is null", name);
  NERF_REQUIRE(a.rays && (bwd || (a.rgb && a.depth && a.acc)), "%s: null pointer", name);
  const dim3 grid((unsigned)((a.N + SEG_WAVES - 1) / SEG_WAVES)), block(64 * SEG_WAVES);
  pick(a.t_shift != nullptr, [&](auto S) {
    pick(dist, [&](auto D) {
      pick(a.bg != nullptr, [&](auto B) {
        constexpr bool s = decltype(S)::value, d = decltype(D)::value, b = decltype(B)::value;
        if (bwd) hipLaunchKernelGGL((march_seg_bwd_kernel<s, d, b>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((march_seg_fwd_kernel<s, d, b>), grid, block, 0, stream, a);
      });
    });
  });
  return check_launch(name);
}

int nerf_march_seg_composite_fwd_shift(const float* raw, const float* rays, int64_t N, const float* t_table,
                                       const int32_t* seg_off, const int32_t* out_step, float step_size, int white,
                                       float* rgb, float* depth, float* acc, const float* t_shift,
                                       hipStream_t stream) {
  SegCompArgs a{raw, rays, N, t_table, seg_off, out_step, step_size, white};
  a.rgb = rgb, a.depth = depth, a.acc = acc, a.t_shift = t_shift;
  return seg_composite("nerf_march_seg_composite_fwd", false, false, a, stream);
}

int nerf_march_seg_composite_fwd(const float* raw, const float* rays, int64_t N, const float* t_table,
                                 const int32_t* seg_off, const int32_t* out_step, float step_size, int white,
                                 float* rgb, float* depth, float* acc, hipStream_t stream) {
  return nerf_march_seg_composite_fwd_shift(raw, rays, N, t_table, seg_off, out_step, step_size, white, rgb, depth,
                                            acc, nullptr, stream);
}

int nerf_march_seg_composite_bwd_shift(const float* raw, const float* rays, int64_t N, const float* t_table,
                                       const int32_t* seg_off, const int32_t* out_step, float step_size, int white,
                                       const float* g_rgb, const float* g_depth, const float* g_acc, float* g_raw,
                                       const float* t_shift, hipStream_t stream) {
  SegCompArgs a{raw, rays, N, t_table, seg_off, out_step, step_size, white};
  a.g_rgb = g_rgb, a.g_depth = g_depth, a.g_acc = g_acc, a.g_raw = g_raw, a.t_shift = t_shift;
  return seg_composite("nerf_march_seg_composite_bwd", true, false, a, stream);
}

int nerf_march_seg_composite_bwd(const float* raw, const float* rays, int64_t N, const float* t_table,
                                 const int32_t* seg_off, const int32_t* out_step, float step_size, int white,
                                 const float* g_rgb, const float* g_depth, const float* g_acc, float* g_raw,
                                 hipStream_t stream) {
  return nerf_march_seg_composite_bwd_shift(raw, rays, N, t_table, seg_off, out_step, step_size, white, g_rgb, g_depth,
                                            g_acc, g_raw, nullptr, stream);
}

// The same pair with the distortion of the weights (the DIST instantiations): the forward also writes
// dist [N] and the ray's totals (sum w, sum w t) [N,2] fp64, which the backward reads back.
int nerf_march_seg_composite_fwd_dist(const float* raw, const float* rays, int64_t N, const float* t_table,
                                      const int32_t* seg_off, const int32_t* out_step, float step_size, int white,
                                      float* rgb, float* depth, float* acc, const float* t_shift, float inv_range,
                                      float* dist, double* totals, hipStream_t stream) {
  SegCompArgs a{raw, rays, N, t_table, seg_off, out_step, step_size, white};
  a.rgb = rgb, a.depth = depth, a.acc = acc, a.t_shift = t_shift;
  a.inv_range = inv_range, a.dist = dist, a.totals = totals;
  return seg_composite("nerf_march_seg_composite_fwd_dist", false, true, a, stream);
}

int nerf_march_seg_composite_bwd_dist(const float* raw, const float* rays, int64_t N, const float* t_table,
                                      const int32_t* seg_off, const int32_t* out_step, float step_size, int white,
                                      const float* g_rgb, const float* g_depth, const float* g_acc,
                                      const float* t_shift, float inv_range, const float* g_dist,
                                      const double* totals, float* g_raw, hipStream_t stream) {
  SegCompArgs a{raw, rays, N, t_table, seg_off, out_step, step_size, white};
  a.g_rgb = g_rgb, a.g_depth = g_depth, a.g_acc = g_acc, a.g_raw = g_raw, a.t_shift = t_shift;
  a.inv_range = inv_range, a.g_dist = g_dist, a.totals_in = totals;
  return seg_composite("nerf_march_seg_composite_bwd_dist", true, true, a, stream);
}

// The same pair on a background colour per ray, bg [N,3] (the BG instantiations): rgb += (1 - acc) bg[r]
// whatever `white` says, g_acc' = g_acc - g_rgb . bg[r].  A null dist (forward) or totals (backward)
// selects the kernels without the distortion term (inv_range is not read then); a null bg is the
// entry point above, or the _shift one.
int nerf_march_seg_composite_fwd_bg(const float* raw, const float* rays, int64_t N, const float* t_table,
                                    const int32_t* seg_off, const int32_t* out_step, float step_size, int white,
                                    float* rgb, float* depth, float* acc, const float* t_shift, float inv_range,
                                    float* dist, double* totals, const float* bg, hipStream_t stream) {
  if (!bg) {
    if (dist)
      return nerf_march_seg_composite_fwd_dist(raw, rays, N, t_table, seg_off, out_step, step_size, white, rgb, depth,
                                               acc, t_shift, inv_range, dist, totals, stream);
    return nerf_march_seg_composite_fwd_shift(raw, rays, N, t_table, seg_off, out_step, step_size, white, rgb, depth,
                                              acc, t_shift, stream);
  }
  SegCompArgs a{raw, rays, N, t_table, seg_off, out_step, step_size, white};
  a.rgb = rgb, a.depth = depth, a.acc = acc, a.t_shift = t_shift, a.bg = bg;
  if (dist) a.inv_range = inv_range, a.dist = dist, a.totals = totals;
  return seg_composite("nerf_march_seg_composite_fwd_bg", false, dist != nullptr, a, stream);
}

int nerf_march_seg_composite_bwd_bg(const float* raw, const float* rays, int64_t N, const float* t_table,
                                    const int32_t* seg_off, const int32_t* out_step, float step_size, int white,
                                    const float* g_rgb, const float* g_depth, const float* g_acc,
                                    const float* t_shift, float inv_range, const float* g_dist,
                                    const double* totals, float* g_raw, const float* bg, hipStream_t stream) {
  if (!bg) {
    if (totals)
      return nerf_march_seg_composite_bwd_dist(raw, rays, N, t_table, seg_off, out_step, step_size, white, g_rgb,
                                               g_depth, g_acc, t_shift, inv_range, g_dist, totals, g_raw, stream);
    return nerf_march_seg_composite_bwd_shift(raw, rays, N, t_table, seg_off, out_step, step_size, white, g_rgb,
                                              g_depth, g_acc, g_raw, t_shift, stream);
  }
  SegCompArgs a{raw, rays, N, t_table, seg_off, out_step, step_size, white};
  a.g_rgb = g_rgb, a.g_depth = g_depth, a.g_acc = g_acc, a.g_raw = g_raw, a.t_shift = t_shift, a.bg = bg;
  if (totals) a.inv_range = inv_range, a.g_dist = g_dist, a.totals_in = totals;
  return seg_composite("nerf_march_seg_composite_bwd_bg", true, totals != nullptr, a, stream);
}

int nerf_march_budget(const int32_t* ray_used, int64_t N, int64_t budget, int32_t* seg_off, int64_t* keep,
                      hipStream_t stream) {
  NERF_REQUIRE(N >= 0, "nerf_march_budget: N must be >= 0");
  NERF_REQUIRE(budget >= 0 && budget <= (int64_t)INT32_MAX,
               "nerf_march_budget: budget must be in [0, INT32_MAX] (the offsets are int32), got %lld",
               (long long)budget);
  NERF_REQUIRE(seg_off && keep && (ray_used || N == 0), "nerf_march_budget: null pointer");
  hipLaunchKernelGGL(march_budget_kernel, dim3(1), dim3(BUDGET_THREADS), 0, stream, ray_used, N, (long long)budget,
                     seg_off, keep);
  return check_launch("nerf_march_budget");
}

int nerf_march_finish(float* rgb, const float* acc, int64_t N, int white, hipStream_t stream) {
  if (N == 0) return 0;
  MarchFinishArgs a{{nullptr, rgb, nullptr, const_cast<float*>(acc), nullptr, nullptr, nullptr}, N, white};
  hipLaunchKernelGGL(march_finish_kernel, grid1(N), dim3(256), 0, stream, a);
  return check_launch("nerf_march_finish");
}

}  // extern "C"
