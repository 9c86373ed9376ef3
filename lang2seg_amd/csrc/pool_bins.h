// The bins of adaptive pooling (nn.AdaptiveAvgPool2d: bin i of n_out over n_in covers [bin_lo, bin_hi), neighbours may share a pixel), and
// the vote of a binary mask's bin.
#pragma once
#include "common.h"

__device__ __forceinline__ int bin_lo(int i, int n_in, int n_out) { return (i * n_in) / n_out; }
__device__ __forceinline__ int bin_hi(int i, int n_in, int n_out) { return ((i + 1) * n_in + n_out - 1) / n_out; }

// one wave counts the set pixels of the bin [y0, y1) x [x0, x1) and decides: 1 where at least half of them are set.  px(yy, xx): the mask's
// pixel (0 / 1), read directly or through a resize table.  The sum is an integer count below 2^24: exact in f32 in any order.
template <class Px>
__device__ __forceinline__ float wave_bin_vote(Px px, int y0, int y1, int x0, int x1, int lane) {
  const int bw = x1 - x0, n = (y1 - y0) * bw;
  float s = 0.f;
  for (int i = lane; i < n; i += 64) s += (float)px(y0 + i / bw, x0 + i % bw);
  s = wave_sum(s);
  return (s / (float)n >= 0.5f) ? 1.f : 0.f;
}
