// Pillow's resampling rules, shared by the kernels that restate a PIL resize (data.hip: the gt masks of the loaders; eval.hip: the
// recovered masks and the gt masks of the evaluation).  Host + device so that the rule is one piece of text.
#pragma once
#include <hip/hip_runtime.h>

// PIL NEAREST source index of output row / column k (Pillow's affine nearest path, oracle/boxes.py nearest_index):
// xo = 0.5 s, then += s in float64, s = n_src / n_out; truncated and clamped to the last source index
__host__ __device__ inline int pil_nearest_src(int k, int n_src, int n_out) {
  const double s = (double)n_src / (double)n_out;
  double xo = 0.5 * s;
  for (int i = 0; i < k; ++i) xo += s;
  const int v = (int)xo;
  return v < n_src - 1 ? v : n_src - 1;
}

// the same walk for a run of consecutive outputs: pil_nearest_src(k) == pil_nearest_at(pil_nearest_xo(k)), and output k + 1's xo is
// output k's + pil_nearest_step (the additions pil_nearest_src makes, one at a time)
__host__ __device__ inline double pil_nearest_step(int n_src, int n_out) { return (double)n_src / (double)n_out; }
__host__ __device__ inline double pil_nearest_xo(int k, int n_src, int n_out) {
  const double s = pil_nearest_step(n_src, n_out);
  double xo = 0.5 * s;
  for (int i = 0; i < k; ++i) xo += s;
  return xo;
}
__host__ __device__ inline int pil_nearest_at(double xo, int n_src) {
  const int v = (int)xo;
  return v < n_src - 1 ? v : n_src - 1;
}

// Pillow's 8-bit BILINEAR resample (libImaging/Resample.c: precompute_coeffs + normalize_coeffs_8bpc) of in_size -> out_size samples,
// box (0, in_size): the taps of output sample xx.  Coefficients in float64 with support = filterscale (the antialiasing path when the
// output is smaller), normalised by their sequential sum, then to fixed point with PRECISION_BITS = 22, rounded away from zero.
#define L2S_PIL_PRECISION_BITS 22
#define L2S_PIL_MAX_TAPS 16          // taps never exceed in_size; the callers resample at most 16 source samples
struct PilTaps {
  int xmin, n;
  int k[L2S_PIL_MAX_TAPS];
};
__host__ __device__ inline void pil_bilinear_taps(int in_size, int out_size, int xx, PilTaps& t) {
#pragma clang fp contract(off)
  const double scale = (double)(float)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double center = 0.0 + (xx + 0.5) * scale;
  const double ss = 1.0 / filterscale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (xmax > L2S_PIL_MAX_TAPS) xmax = L2S_PIL_MAX_TAPS;     // unreachable for in_size <= 16
  double w[L2S_PIL_MAX_TAPS];
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) {
    double a = ((double)(x + xmin) - center + 0.5) * ss;
    if (a < 0.0) a = -a;
    w[x] = a < 1.0 ? 1.0 - a : 0.0;
    ww += w[x];
  }
  for (int x = 0; x < xmax; ++x) {
    const double v = ww != 0.0 ? w[x] / ww : w[x];
    t.k[x] = v < 0 ? (int)(-0.5 + v * (double)(1 << L2S_PIL_PRECISION_BITS)) : (int)(0.5 + v * (double)(1 << L2S_PIL_PRECISION_BITS));
  }
  t.xmin = xmin;
  t.n = xmax;
}
// clip8 of Resample.c: the fixed-point sum (with its 1 << 21 rounding bias) -> uint8
__host__ __device__ inline int pil_clip8(int ss) {
  if (ss >= (1 << L2S_PIL_PRECISION_BITS << 8)) return 255;
  if (ss <= 0) return 0;
  return ss >> L2S_PIL_PRECISION_BITS;
}
