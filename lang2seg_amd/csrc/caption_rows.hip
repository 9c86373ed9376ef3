// The caption branch on ROWS: one row per detection of a sentence (nets/caption_rows.py).  Every kernel here is a merged single-mask
// kernel with a row index in gridDim.y / gridDim.z and the same arithmetic in the same order, so that a row equals what the single-mask
// path computes for it:
//   l2s_masks_to_map          mask_resize_nearest_kernel (decode.hip) + mask_downsample_kernel (misc_kernels.hip) in one launch
//   l2s_adaptive_pool_rows    adaptive_pool_fwd_kernel (misc_kernels.hip)
//   l2s_cap_att_dots_rows     cap_att_dots_kernel (caption_step.hip) without the tanh copy that only backward reads
//   l2s_cap_apply_gates_rows  cap_apply_gates_kernel (caption_step.hip) without `save` / `weight`
//   l2s_cap_att_apply_rows    cap_att_apply_kernel (caption_step.hip) without `weight`
//   l2s_decode_pick_rows      the greedy branch of decode_pick_kernel (decode.hip), or the log-probability of a forced token
// The exception is l2s_lstm_cell_rows, the top-down captioner's nn.LSTMCell on rows: topdown_cell_fwd_kernel's arithmetic with the
// products on MFMA tiles of rows (another summation order, within the forward tolerance of the single-row cell), because the single-row
// kernel streams a whole weight matrix per row.
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
typedef float floatx4 __attribute__((ext_vector_type(4)));

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

// ---------------------------------------------------------------- the top-down step on rows
// l2s_lstm_cell_rows.  The single-row cell (topdown_cell_fwd_kernel) streams a whole weight matrix per row; here the products run as tiles
// of the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32, the lane maps of linear_nt_mfma_kernel in lang.hip: a lane holds A[l%16][l/16] and
// B[l/16][l%16], D rows 4(l/16)+reg, column l%16), so a weight element is fetched once per tile of MT * 16 rows.  Workgroup = CELL_U = 4
// hidden units x MT 16-row tiles: its 16 MFMA columns are the four gate rows of its units (column 4 q + u = gate q of unit u), so it owns
// everything the cell of those units needs and finishes it after one LDS sum; its 4 waves split each segment's K.  At R = 512 that is
// 128 workgroups x cdiv(rows, 32), each pulling 16 weight rows (98 KB of the 1536 columns) and its tile's x rows.
struct RSeg { const float* x; int ldx; const float* w; int ld; int n; };
struct CellR { const float* pre; int ld_pre; const float* pre2; int ld_pre2; const float* add0; const float* add1; RSeg s0, s1;
               const float* c_prev; int ld_cp; float* c; int ld_c; float* h; int ld_h; };
constexpr int CELL_U = 4;

// p[k .. k + 3], zero at and beyond n.  VEC: n % 4 == 0 and p + k is 16-byte aligned, so the four are inside or outside together
template <bool VEC>
__device__ __forceinline__ float4 ld4_upto(const float* __restrict__ p, int k, int n) {
  if (VEC) return k < n ? *(const float4*)(p + k) : make_float4(0.f, 0.f, 0.f, 0.f);
  return make_float4(k < n ? p[k] : 0.f, k + 1 < n ? p[k + 1] : 0.f, k + 2 < n ? p[k + 2] : 0.f, k + 3 < n ? p[k + 3] : 0.f);
}
// one segment's share of wave wv: acc[t] += x rows of tile t (A) . the workgroup's 16 weight rows (B).  xr[t]: the lane's x row, null
// where that row is dead or beyond `rows` (never read: zeros); wr: the lane's weight row.
template <int MT, bool VEC>
__device__ __forceinline__ void cell_rows_seg(const float* const (&xr)[MT], const float* __restrict__ wr, int n, int wv, int kq, floatx4 (&acc)[MT]) {
  const int kper = ((n + 63) / 64) * 16;                  // K range of one wave, a multiple of 16
  const int kb = wv * kper, ke = min(n, kb + kper);
  for (int k = kb; k < ke; k += 16) {
    const int kk = k + 4 * kq;
    const float4 bv = ld4_upto<VEC>(wr, kk, ke);
    float4 av[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) av[t] = xr[t] ? ld4_upto<VEC>(xr[t], kk, ke) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t].x, bv.x, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t].y, bv.y, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t].z, bv.z, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t].w, bv.w, acc[t], 0, 0, 0);
    }
  }
}
template <int MT, bool VEC>
__global__ __launch_bounds__(256) void lstm_cell_rows_kernel(CellR a, int R, int rows, int row0, const int* __restrict__ count) {
  __shared__ float red[4][MT][4][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, j = lane & 15, kq = lane >> 4;
  const int u0 = blockIdx.x * CELL_U, m0 = blockIdx.y * (16 * MT);
  int nlive = rows;                                      // the live rows are the first nlive
  if (count) { nlive = *count - row0; nlive = nlive < 0 ? 0 : (nlive > rows ? rows : nlive); }
  if (m0 >= nlive) return;                               // (the whole workgroup: before any barrier)
  const long wrow = (long)(j >> 2) * R + min(u0 + (j & 3), R - 1);
  floatx4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  if (a.s0.n > 0) {
    const float* xr[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) { const int m = m0 + 16 * t + j; xr[t] = m < nlive ? a.s0.x + (long)m * a.s0.ldx : nullptr; }
    cell_rows_seg<MT, VEC>(xr, a.s0.w + wrow * a.s0.ld, a.s0.n, wv, kq, acc);
  }
  if (a.s1.n > 0) {
    const float* xr[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) { const int m = m0 + 16 * t + j; xr[t] = m < nlive ? a.s1.x + (long)m * a.s1.ldx : nullptr; }
    cell_rows_seg<MT, VEC>(xr, a.s1.w + wrow * a.s1.ld, a.s1.n, wv, kq, acc);
  }
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wv][t][r][lane] = acc[t][r];
  __syncthreads();
  // thread (tile t, row ml, unit u) adds the four waves' shares of its four gates in a fixed order and finishes the cell
  if (tid < 64 * MT) {
    const int t = tid >> 6, ml = (tid & 63) >> 2, u = tid & 3;
    const int m = m0 + 16 * t + ml, unit = u0 + u;
    if (m < nlive && unit < R) {
      float g[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int at = (ml >> 2) * 16 + 4 * q + u;
        float v = ((red[0][t][ml & 3][at] + red[1][t][ml & 3][at]) + red[2][t][ml & 3][at]) + red[3][t][ml & 3][at];
        if (a.pre) v += a.pre[(long)m * a.ld_pre + q * R + unit];
        if (a.pre2) v += a.pre2[(long)m * a.ld_pre2 + q * R + unit];
        if (a.add0) v += a.add0[q * R + unit];
        if (a.add1) v += a.add1[q * R + unit];
        g[q] = v;
      }
      float act[4];
      lstm_cell_fwd(g, a.c_prev[(long)m * a.ld_cp + unit], a.c[(long)m * a.ld_c + unit], a.h[(long)m * a.ld_h + unit], act);
    }
  }
}

// l2s_cap_att_apply_rows: cap_att_apply_kernel (caption_step.hip) per row, cdiv(R, 64) workgroups a row, each recomputing the row's softmax;
// the sum over the locations in that kernel's order (4 location groups, added 0 + 1 + 2 + 3), no `weight` output
__global__ __launch_bounds__(256) void cap_att_apply_rows_kernel(const float* __restrict__ att, const float* __restrict__ dots, float* att_res, int ld_res,
                                                                int row0, const int* __restrict__ count, int L, int D) {
  __shared__ float w[256];
  __shared__ float red[4];
  __shared__ float part[4][64];
  const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  if (!row_live(r, row0, count)) return;
  const float wt = block_softmax(dots + (long)r * 256, L, red);
  if (tid < L) w[tid] = wt;
  __syncthreads();
  const int d = blockIdx.x * 64 + lane;
  const float* ar = att + (long)r * L * D;
  float s = 0.f;
  if (d < D) for (int l = g; l < L; l += 4) s = fmaf(w[l], ar[(long)l * D + d], s);
  part[g][lane] = s;
  __syncthreads();
  if (g == 0 && d < D) att_res[(long)r * ld_res + d] = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
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

static bool rows_seg_ok(const l2s_rows_seg& g, int rows) {
  return g.n == 0 || (g.n > 0 && g.x && g.w && g.ld >= g.n && (g.ldx >= g.n || rows == 1));
}
static bool rows_seg_vec(const l2s_rows_seg& g) {
  return g.n == 0 || !((g.n & 3) || (g.ld & 3) || (g.ldx & 3) || ((uintptr_t)g.x & 15) || ((uintptr_t)g.w & 15));
}
extern "C" int l2s_lstm_cell_rows(const l2s_lstm_rows* a, int R, int rows, int row0, const int* count, hipStream_t s) {
  if (!a || R < 1 || rows < 1 || row0 < 0 || !a->c_prev || !a->c || !a->h || !rows_seg_ok(a->seg[0], rows) || !rows_seg_ok(a->seg[1], rows) ||
      cdiv(rows, 16) > 65535)
    return L2S_EINVAL;
  if (rows > 1 && (a->ld_c_prev < R || a->ld_c < R || a->ld_h < R || (a->pre && a->ld_pre != 0 && a->ld_pre < 4 * R) ||
                   (a->pre2 && a->ld_pre2 != 0 && a->ld_pre2 < 4 * R)))
    return L2S_EINVAL;
  const CellR k{a->pre, a->ld_pre, a->pre2, a->ld_pre2, a->add0, a->add1,
                RSeg{a->seg[0].x, a->seg[0].ldx, a->seg[0].w, a->seg[0].ld, a->seg[0].n},
                RSeg{a->seg[1].x, a->seg[1].ldx, a->seg[1].w, a->seg[1].ld, a->seg[1].n},
                a->c_prev, a->ld_c_prev, a->c, a->ld_c, a->h, a->ld_h};
  const bool vec = rows_seg_vec(a->seg[0]) && rows_seg_vec(a->seg[1]);
  const dim3 g1(cdiv(R, CELL_U), cdiv(rows, 16)), g2(cdiv(R, CELL_U), cdiv(rows, 32));
  if (rows <= 16) {
    if (vec) L2S_LAUNCH((lstm_cell_rows_kernel<1, true>), g1, dim3(256), 0, s, k, R, rows, row0, count);
    else L2S_LAUNCH((lstm_cell_rows_kernel<1, false>), g1, dim3(256), 0, s, k, R, rows, row0, count);
  } else {
    if (vec) L2S_LAUNCH((lstm_cell_rows_kernel<2, true>), g2, dim3(256), 0, s, k, R, rows, row0, count);
    else L2S_LAUNCH((lstm_cell_rows_kernel<2, false>), g2, dim3(256), 0, s, k, R, rows, row0, count);
  }
  return l2s_check_launch();
}

extern "C" int l2s_cap_att_apply_rows(const float* att, const float* dots, float* att_res, int ld_res, int rows, int row0, const int* count, int L,
                                      int R, hipStream_t s) {
  if (!att || !dots || !att_res || rows < 1 || rows > 65535 || row0 < 0 || L < 1 || L > 256 || R < 1 || ld_res < R) return L2S_EINVAL;
  L2S_LAUNCH(cap_att_apply_rows_kernel, dim3(cdiv(R, 64), rows), dim3(256), 0, s, att, dots, att_res, ld_res, row0, count, L, R);
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
