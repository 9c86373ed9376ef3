// Device functions shared by the recurrent step kernels (rnn_step.hip, caption_step.hip, cap_recur.hip; lang.hip takes sigm): the scalar
// pieces, the LSTM cell, the att2in2 gate block and the adaptive-attention cell (adaatt_step.hip) with their backward passes, and the
// workgroup-wide softmax of the attention kernels.
// Every function works on values in registers: the kernel loads the operands and stores the results where its layout wants them.  The
// expressions are the ones the kernels carried inline; the step's gradient bits are pinned by tests/test_topdown_gpu.py.
#pragma once
#include "common.h"

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float dot4(const float4 a, const float4 b, float acc) {
  return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, fmaf(a.w, b.w, acc))));
}
// one wave's partial dot product of row `w` with `x` over n elements (the caller reduces)
template <bool VEC>
__device__ __forceinline__ float row_dot(const float* __restrict__ w, const float* __restrict__ x, int n, int lane, float acc) {
  if (VEC) {
    for (int k = lane * 4; k < n; k += 256) acc = dot4(*(const float4*)(w + k), *(const float4*)(x + k), acc);
  } else {
    for (int k = lane; k < n; k += 64) acc = fmaf(w[k], x[k], acc);
  }
  return acc;
}

// v[q] = p[q * stride + j] and back: the values of unit j in a gate-major array ([gate][unit])
template <int N>
__device__ __forceinline__ void ld_rows(float v[N], const float* p, int stride, int j) {
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] = p[q * stride + j];
}
template <int N>
__device__ __forceinline__ void st_rows(float* p, int stride, int j, const float v[N]) {
#pragma unroll
  for (int q = 0; q < N; ++q) p[q * stride + j] = v[q];
}

// ---- nn.LSTM / nn.LSTMCell, gate order i, f, g, o.  g: the four pre-activations; act: the four activations, saved for backward.
// (Which of the two products of `f * c_prev + i * gg` the compiler fuses into the FMA depends on where the operands come from: with
// c_prev handed over as a value it is f * c_prev in the step kernels, as it was when they carried these lines themselves.)
__device__ __forceinline__ void lstm_cell_fwd(const float g[4], float c_prev, float& c, float& h, float act[4]) {
  const float i = sigm(g[0]), f = sigm(g[1]), gg = tanhf(g[2]), o = sigm(g[3]);
  const float cn = f * c_prev + i * gg;
  c = cn; h = o * tanhf(cn);
  act[0] = i; act[1] = f; act[2] = gg; act[3] = o;
}
// dh / dc_in: the gradients arriving at h and c; dg: the four gate gradients
__device__ __forceinline__ void lstm_cell_bwd(float dh, float dc_in, const float act[4], float c_prev, float c, float dg[4], float& dc_prev) {
  const float i = act[0], f = act[1], gg = act[2], o = act[3];
  const float tc = tanhf(c);
  const float dcn = dc_in + dh * o * (1.f - tc * tc);
  dg[0] = dcn * gg * i * (1.f - i);
  dg[1] = dcn * c_prev * f * (1.f - f);
  dg[2] = dcn * i * (1.f - gg * gg);
  dg[3] = dh * tc * o * (1.f - o);
  dc_prev = dcn * f;
}

// ---- the att2in2 gate block (ATT:449-462).  s: the five sums (in, forget, out gates and the two input transforms), a0 / a1: the a2c
// values of the unit; save: in gate, forget gate, out gate, selector of the max (torch.max(a, b): first wins ties), max, tanh(c)
__device__ __forceinline__ void att2in_gates_fwd(const float s[5], float a0, float a1, float c_prev, float& c, float& h, float save[6]) {
  const float ig = sigm(s[0]), fg = sigm(s[1]), og = sigm(s[2]);
  const float t0 = s[3] + a0, t1 = s[4] + a1;
  const float it = fmaxf(t0, t1);
  const float cn = fg * c_prev + ig * it;
  const float tc = tanhf(cn);
  c = cn; h = og * tc;
  save[0] = ig; save[1] = fg; save[2] = og; save[3] = (t0 >= t1) ? 0.f : 1.f;
  save[4] = it; save[5] = tc;
}
// dhj: recurrent part + this step's output gradient.  ds: gradients of the three gate sums; d0 / d1: of the two input transforms (= of a2c)
__device__ __forceinline__ void att2in_gates_bwd(const float save[6], float dhj, float dc_in, float c_prev, float ds[3], float& d0, float& d1,
                                                 float& dc_prev) {
  const float ig = save[0], fg = save[1], og = save[2], sel = save[3], it = save[4];
  const float tc = save[5];
  const float dcn = dc_in + dhj * og * (1.f - tc * tc);
  ds[0] = dcn * it * ig * (1.f - ig);
  ds[1] = dcn * c_prev * fg * (1.f - fg);
  ds[2] = dhj * tc * og * (1.f - og);
  const float dit = dcn * ig;
  d0 = sel == 0.f ? dit : 0.f; d1 = sel == 0.f ? 0.f : dit;
  dc_prev = dcn * fg;
}

// ---- the adaptive-attention cell (ATT:258-285), row blocks in, forget, out, transform: NOT nn.LSTM's order.  MAXOUT (adaattmo): two transform
// rows and their max without a tanh (torch.max(a, b): first wins ties, as above); otherwise tanh of the one row.  n5: the sentinel gate's sum.
// save: in gate, forget gate, out gate, transform, selector of the max, tanh(c), sigmoid(n5)
template <bool MAXOUT>
__device__ __forceinline__ void adaatt_cell_fwd(const float* s, float n5, float c_prev, float& c, float& h, float& fake, float save[7]) {
  const float ig = sigm(s[0]), fg = sigm(s[1]), og = sigm(s[2]);
  float it, sel = 0.f;
  if (MAXOUT) { it = fmaxf(s[3], s[4]); sel = (s[3] >= s[4]) ? 0.f : 1.f; }
  else it = tanhf(s[3]);
  const float cn = fg * c_prev + ig * it;
  const float tc = tanhf(cn);
  const float sg = sigm(n5);
  c = cn; h = og * tc; fake = sg * tc;
  save[0] = ig; save[1] = fg; save[2] = og; save[3] = it; save[4] = sel; save[5] = tc; save[6] = sg;
}
// dh: recurrent part + d(top_h); dfake: d(fake).  tanh(c) feeds both h and the sentinel.  ds: gradients of the four (five) sums; dn5: of n5
template <bool MAXOUT>
__device__ __forceinline__ void adaatt_cell_bwd(const float save[7], float dh, float dfake, float dc_in, float c_prev, float ds[5], float& dn5,
                                                float& dc_prev) {
  const float ig = save[0], fg = save[1], og = save[2], it = save[3], sel = save[4], tc = save[5], sg = save[6];
  const float dtc = og * dh + sg * dfake;
  const float dcn = dc_in + dtc * (1.f - tc * tc);
  ds[0] = dcn * it * ig * (1.f - ig);
  ds[1] = dcn * c_prev * fg * (1.f - fg);
  ds[2] = dh * tc * og * (1.f - og);
  const float dit = dcn * ig;
  if (MAXOUT) { ds[3] = sel == 0.f ? dit : 0.f; ds[4] = sel == 0.f ? 0.f : dit; }
  else { ds[3] = dit * (1.f - it * it); ds[4] = 0.f; }
  dn5 = dfake * tc * sg * (1.f - sg);
  dc_prev = dcn * fg;
}

// ---- softmax over L <= 256 attention scores, recomputed by every workgroup (256 threads; red: 4 floats): the weight of location
// threadIdx.x (meaningful where threadIdx.x < L)
__device__ __forceinline__ float block_softmax(const float* __restrict__ dots, int L, float* red) {
  const int tid = threadIdx.x;
  const float v = tid < L ? dots[tid] : -INFINITY;
  const float mx = block_max(v, red);
  const float e = tid < L ? expf(v - mx) : 0.f;
  const float sum = block_sum(e, red);
  return e / sum;
}
// its backward, for a workgroup of >= 256 threads (red: one float per wave): dd[l] = w[l] (dw[l] - sum_l w dw) from thread l's wl / dw (0
// beyond L) into ddot[256] (0 beyond L); workgroup 0 also stores it to ddot_out.  Ends with a barrier: ddot is readable on return.
__device__ __forceinline__ void block_softmax_bwd(float wl, float dw, int L, float* ddot, float* red, float* ddot_out) {
  const int tid = threadIdx.x;
  const float dot = block_sum(wl * dw, red);
  const float dd = wl * (dw - dot);
  if (tid < 256) ddot[tid] = tid < L ? dd : 0.f;
  if (blockIdx.x == 0 && tid < L) ddot_out[tid] = dd;
  __syncthreads();
}
