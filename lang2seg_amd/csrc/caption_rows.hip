// The caption branch on ROWS: one row per detection of a sentence (nets/caption_rows.py).  Every kernel here is a merged single-mask
// kernel with a row index in gridDim.y / gridDim.z and the same arithmetic in the same order, so that a row equals what the single-mask
// path computes for it:
//   l2s_masks_to_map          mask_resize_nearest_kernel (decode.hip) + mask_downsample_kernel (misc_kernels.hip) in one launch
//   l2s_adaptive_pool_rows    adaptive_pool_fwd_kernel (misc_kernels.hip)
//   l2s_cap_att_dots_rows     cap_att_dots_kernel (caption_step.hip) without the tanh copy that only backward reads
//   l2s_cap_apply_gates_rows  cap_apply_gates_kernel (caption_step.hip) without `save` / `weight`
//   l2s_decode_pick_rows      the greedy branch of decode_pick_kernel (decode.hip), or the log-probability of a forced token
// The recurrent step stays row-strided rather than one fused workgroup per row: a row reads its own patt [L][AH] and P [L][2R], 1.2 MB at
// the production widths, and one workgroup pulls that through ONE compute unit's L2 port - at rows = 8 that is 8 of 256 ports busy for
// about 8 us a token.  The strided grids spread every row over cdiv(L, 4) / cdiv(R, 16) workgroups and fill the device from one row on.
// Live rows: row r of a call is used iff row0 + r < *count (count: device int32, null = all rows); a dead row is neither read nor
// written, and the grids never depend on *count.
#include "common.h"
#include "../../include/lang2seg_hip.h"
#include "pil_resize.h"
#include "recur.h"
#include <climits>
#include <cmath>

namespace {

constexpr int ROWS_T = 256;

__device__ __forceinline__ bool row_live(int r, int row0, const int* count) { return !count || row0 + r < *count; }
__device__ __forceinline__ int rbin_lo(int i, int n_in, int n_out) { return (i * n_in) / n_out; }
__device__ __forceinline__ int rbin_hi(int i, int n_in, int n_out) { return ((i + 1) * n_in + n_out - 1) / n_out; }

// ---------------------------------------------------------------- l2s_masks_to_map
// Workgroup = one row of map bins of one mask.  The PIL source columns of the whole blob row and the source rows of the bin row go to the
// LDS first (pil_nearest_src is a running float64 sum: every thread walks to its first index once, then steps), then one wave per bin
// counts in mask_downsample_kernel's order.  The sums are integer counts below 2^24: exact in f32 in any order.
__global__ __launch_bounds__(ROWS_T) void masks_to_map_kernel(const uint8_t* __restrict__ masks, int row0, const int* __restrict__ count, int mh, int mw,
                                                              int H, int W, int h, int w, float* out) {
  extern __shared__ int tab[];          // tx[W] | ty[bin rows]
  const int r = blockIdx.y, oy = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (!row_live(r, row0, count)) return;
  const int y0 = rbin_lo(oy, H, h), y1 = rbin_hi(oy, H, h);
  int* tx = tab;
  int* ty = tab + W;
  const bool resize = mh != H || mw != W;
  if (resize) {
    const int chunk = (W + ROWS_T - 1) / ROWS_T, k0 = tid * chunk, k1 = k0 + chunk < W ? k0 + chunk : W;
    if (k0 < k1) {
      const double sx = (double)mw / (double)W;
      double xo = 0.5 * sx;
      for (int i = 0; i < k0; ++i) xo += sx;
      for (int k = k0; k < k1; ++k) {
        const int v = (int)xo;
        tx[k] = v < mw - 1 ? v : mw - 1;
        xo += sx;
      }
    }
    for (int k = y0 + tid; k < y1; k += ROWS_T) ty[k - y0] = pil_nearest_src(k, mh, H);
    __syncthreads();
  }
  const uint8_t* src = masks + (long)r * mh * mw;
  for (int ox = tid >> 6; ox < w; ox += ROWS_T / 64) {
    const int x0 = rbin_lo(ox, W, w), x1 = rbin_hi(ox, W, w);
    const int bw = x1 - x0, n = (y1 - y0) * bw;
    float s = 0.f;
    for (int i = lane; i < n; i += 64) {
      const int yy = y0 + i / bw, xx = x0 + i % bw;
      s += (float)(resize ? src[(long)ty[yy - y0] * mw + tx[xx]] : src[(long)yy * W + xx]);
    }
    s = wave_sum(s);
    if (lane == 0) out[(long)r * h * w + oy * w + ox] = (s / (float)n >= 0.5f) ? 1.f : 0.f;
  }
}

// ---------------------------------------------------------------- l2s_adaptive_pool_rows
// adaptive_pool_fwd_kernel's loop per (channel, bin, row).  Without masks every row is the same pooling: it is summed once (gridDim.z = 1)
// and stored to every live row.
__global__ void adaptive_pool_rows_kernel(const void* x, const float* pm, void* y, int rows, int row0, const int* count, int H, int W, int C, int OH,
                                          int OW, int ldy, int dt) {
  const int bin = blockIdx.y, oy = bin / OW, ox = bin - oy * OW;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.z;
  if (c >= C) return;
  if (pm && !row_live(r, row0, count)) return;
  const int y0 = rbin_lo(oy, H, OH), y1 = rbin_hi(oy, H, OH), x0 = rbin_lo(ox, W, OW), x1 = rbin_hi(ox, W, OW);
  const float* m = pm ? pm + (long)r * H * W : nullptr;
  float s = 0.f;
  for (int yy = y0; yy < y1; ++yy)
    for (int xx = x0; xx < x1; ++xx) {
      float v = ldx(x, ((long)yy * W + xx) * C + c, dt);
      if (m) v *= m[yy * W + xx];
      s += v;
    }
  const float v = s / (float)((y1 - y0) * (x1 - x0));
  const long rs = (long)OH * OW * ldy;
  if (pm) {
    stx(y, r * rs + (long)bin * ldy + c, dt, v);
  } else {
    int n = rows;
    if (count) { n = *count - row0; n = n < 0 ? 0 : (n > rows ? rows : n); }
    for (int q = 0; q < n; ++q) stx(y, q * rs + (long)bin * ldy + c, dt, v);
  }
}

// ---------------------------------------------------------------- the att2in2 step on rows (projected form)
// one wave per (location, row): dots[r][l] = alpha . tanh(patt[r][l] + att_h[r]) + alpha_bias
__global__ __launch_bounds__(256) void cap_att_dots_rows_kernel(const float* __restrict__ patt, const float* __restrict__ att_h, int ld_att_h,
                                                               const float* __restrict__ aw, const float* __restrict__ ab, int row0,
                                                               const int* __restrict__ count, int L, int D, float* dots) {
  const int r = blockIdx.y, l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (l >= L || !row_live(r, row0, count)) return;
  const float* pr = patt + ((long)r * L + l) * D;
  const float* ah = att_h + (long)r * ld_att_h;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s = fmaf(tanhf(pr[d] + ah[d]), aw[d], s);
  s = wave_sum(s);
  if (lane == 0) dots[(long)r * 256 + l] = s + ab[0];
}
// workgroup = 16 units x 16 location groups of one row: the softmax over the row's L dots, the weighted sum of the row's P columns, the gates
__global__ __launch_bounds__(256) void cap_apply_gates_rows_kernel(const float* __restrict__ P, const float* __restrict__ dots, const float* __restrict__ b,
                                                                  const float* __restrict__ s, int ld_s, const float* __restrict__ c_prev, float* c,
                                                                  float* h, int row0, const int* __restrict__ count, int L, int R) {
  __shared__ float w[256];
  __shared__ float red[4];
  __shared__ float p0[16][17], p1[16][17];
  const int r = blockIdx.y, tid = threadIdx.x, dl = tid & 15, lg = tid >> 4;
  if (!row_live(r, row0, count)) return;
  const float wt = block_softmax(dots + (long)r * 256, L, red);
  w[tid] = tid < L ? wt : 0.f;
  __syncthreads();
  const int j = blockIdx.x * 16 + dl;
  float a0 = 0.f, a1 = 0.f;
  if (j < R) {
    const float* q = P + (long)r * L * 2 * R + j;
    for (int l = lg; l < L; l += 16) {
      const float wl = w[l];
      a0 = fmaf(wl, q[(long)l * 2 * R], a0);
      a1 = fmaf(wl, q[(long)l * 2 * R + R], a1);
    }
  }
  p0[lg][dl] = a0; p1[lg][dl] = a1;
  __syncthreads();
  if (lg == 0 && j < R) {
    a0 = b[j]; a1 = b[R + j];
#pragma unroll
    for (int g = 0; g < 16; ++g) { a0 += p0[g][dl]; a1 += p1[g][dl]; }
    float sj[5], sv[6];
    ld_rows<5>(sj, s + (long)r * ld_s, R, j);
    att2in_gates_fwd(sj, a0, a1, c_prev[(long)r * R + j], c[(long)r * R + j], h[(long)r * R + j], sv);
  }
}

// ---------------------------------------------------------------- l2s_decode_pick_rows
__device__ __forceinline__ bool rows_better(float ov, int ok, float bv, int bk) {
  return ok != INT_MAX && ov == ov && (bk == INT_MAX || ov > bv || (ov == bv && ok < bk));
}
__global__ __launch_bounds__(ROWS_T) void decode_pick_rows_kernel(const float* logits, int ld, int V1, int row0, const int* __restrict__ count, int t, int T,
                                                                  const int64_t* forced, int* finished, int64_t* seq, float* logprobs,
                                                                  int64_t* next_token, float* sum) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  __shared__ float wv[4];
  __shared__ int wk[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (!row_live(r, row0, count)) return;
  const float* x = logits + (long)r * ld;
  float m = -INFINITY;
  for (int k = tid; k < V1; k += ROWS_T) m = fmaxf(m, x[k]);
  m = block_max(m, red);
  float s = 0.f;
  for (int k = tid; k < V1; k += ROWS_T) s += expf(x[k] - m);
  s = block_sum(s, red);
  const float ls = logf(s);
  int pick = 0;
  if (forced) {
    const int64_t f = *forced;
    pick = f < 0 ? 0 : (f >= V1 ? V1 - 1 : (int)f);      // (a token outside the table: clamped, never an address)
  } else {
    float bv = 0.f;
    int bk = INT_MAX;
    for (int k = tid; k < V1; k += ROWS_T) {
      const float lp = (x[k] - m) - ls;
      if (rows_better(lp, k, bv, bk)) { bv = lp; bk = k; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int ok = __shfl_xor(bk, o);
      if (rows_better(ov, ok, bv, bk)) { bv = ov; bk = ok; }
    }
    if ((tid & 63) == 0) { wv[tid >> 6] = bv; wk[tid >> 6] = bk; }
    __syncthreads();
    for (int q = 0; q < ROWS_T / 64; ++q)
      if (q == 0 || rows_better(wv[q], wk[q], bv, bk)) { bv = wv[q]; bk = wk[q]; }
    pick = bk == INT_MAX ? 0 : bk;                      // (all NaN: no candidate)
  }
  if (tid == 0) {
    // teacher forcing has no finished rows: the expression is scored to its end (AttModel.forward with the criterion's mask all ones)
    const int fin = (forced || t == 0) ? 0 : finished[r];
    const int tok = fin ? 0 : pick;
    seq[(long)r * T + t] = tok;
    const float lp = fin ? 0.f : (x[pick] - m) - ls;
    logprobs[(long)r * T + t] = lp;
    if (sum) sum[r] = t == 0 ? lp : sum[r] + lp;           // the row's joint log-probability, added up left to right
    next_token[r] = tok;
    finished[r] = fin | (tok == 0);
  }
}

}  // namespace

extern "C" int l2s_masks_to_map(const uint8_t* masks, int rows, int row0, const int* count, int mh, int mw, int H, int W, int Hc, int Wc, float* out,
                                hipStream_t s) {
  if (!masks || !out || rows < 1 || rows > 65535 || row0 < 0 || mh < 1 || mw < 1 || H < 1 || W < 1 || Hc < 1 || Wc < 1 || Hc > 65535 ||
      W > L2S_ROWS_MAX_W || (long)H * W >= (1l << 24))
    return L2S_EINVAL;
  const size_t lds = sizeof(int) * ((size_t)W + (size_t)(H + Hc - 1) / Hc + 2);      // a bin row spans at most ceil(H / Hc) + 1 blob rows
  L2S_LAUNCH(masks_to_map_kernel, dim3(Hc, rows), dim3(ROWS_T), lds, s, masks, row0, count, mh, mw, H, W, Hc, Wc, out);
  return l2s_check_launch();
}

extern "C" int l2s_adaptive_pool_rows(const void* x, const float* pm, void* y, int rows, int row0, const int* count, int H, int W, int C, int OH, int OW,
                                      int ldy, int dtype, hipStream_t s) {
  if (!x || !y || rows < 1 || rows > 65535 || row0 < 0 || H < 1 || W < 1 || C < 1 || OH < 1 || OW < 1 || (long)OH * OW > 65535 || ldy < C ||
      (dtype != 0 && dtype != 1))
    return L2S_EINVAL;
  L2S_LAUNCH(adaptive_pool_rows_kernel, dim3(cdiv(C, 256), OH * OW, pm ? rows : 1), dim3(256), 0, s, x, pm, y, rows, row0, count, H, W, C, OH, OW, ldy,
             dtype);
  return l2s_check_launch();
}

extern "C" int l2s_cap_att_dots_rows(const float* patt, const float* att_h, int ld_att_h, const float* aw, const float* ab, int rows, int row0,
                                     const int* count, int L, int D, float* dots, hipStream_t s) {
  if (!patt || !att_h || !aw || !ab || !dots || rows < 1 || rows > 65535 || row0 < 0 || L < 1 || L > 256 || D < 1 || ld_att_h < D) return L2S_EINVAL;
  L2S_LAUNCH(cap_att_dots_rows_kernel, dim3(cdiv(L, 4), rows), dim3(256), 0, s, patt, att_h, ld_att_h, aw, ab, row0, count, L, D, dots);
  return l2s_check_launch();
}

extern "C" int l2s_cap_apply_gates_rows(const float* P, const float* dots, const float* b_a2c, const float* sums, int ld_sums, const float* c_prev,
                                        float* c, float* h, int rows, int row0, const int* count, int L, int R, hipStream_t s) {
  if (!P || !dots || !b_a2c || !sums || !c_prev || !c || !h || rows < 1 || rows > 65535 || row0 < 0 || L < 1 || L > 256 || R < 1 || R > 1024 ||
      ld_sums < 5 * R)
    return L2S_EINVAL;
  L2S_LAUNCH(cap_apply_gates_rows_kernel, dim3(cdiv(R, 16), rows), dim3(256), 0, s, P, dots, b_a2c, sums, ld_sums, c_prev, c, h, row0, count, L, R);
  return l2s_check_launch();
}

extern "C" int l2s_decode_pick_rows(const float* logits, int ld_logits, int V1, int rows, int row0, const int* count, int t, int T,
                                    const int64_t* forced, int* finished, int64_t* seq, float* logprobs, int64_t* next_token, float* sum,
                                    hipStream_t s) {
  if (!logits || V1 < 1 || ld_logits < V1 || rows < 1 || row0 < 0 || t < 0 || t >= T || !finished || !seq || !logprobs || !next_token) return L2S_EINVAL;
  L2S_LAUNCH(decode_pick_rows_kernel, dim3(rows), dim3(ROWS_T), 0, s, logits, ld_logits, V1, row0, count, t, T, forced, finished, seq, logprobs,
             next_token, sum);
  return l2s_check_launch();
}
