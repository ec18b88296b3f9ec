// What grid.hip (lookup, bake, online update) and march.hip (the ray march) share: the scene box,
// the cell index of a coordinate, and the 256-thread launch grid of their entry points.
#pragma once
#include "common.h"

namespace nerf {

struct BBox { float mn[3], mx[3]; };

__device__ __forceinline__ int grid_axis(float p, float mn, float mx, int res) {
  const float c = fminf(fmaxf(p, mn), mx);                  // torch.clamp(p, min, max)
  const float n = fdiv(fsub(c, mn), fsub(mx, mn));          // (p - min) / (max - min)
  return (int)fmul(n, (float)(res - 1));                    // (n * (res - 1)).long()
}

static inline BBox make_bbox(const float* b) {
  BBox bb;
  for (int k = 0; k < 3; ++k) {
    bb.mn[k] = b[k];
    bb.mx[k] = b[3 + k];
  }
  return bb;
}

static inline dim3 grid1(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace nerf
