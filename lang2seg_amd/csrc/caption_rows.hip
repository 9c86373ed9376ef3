// The caption branch on ROWS: one row per detection of a sentence (nets/caption_rows.py).  A row entry is the single-mask kernel's own body
// with a row index in gridDim.y / gridDim.z, and lives next to that kernel, so that a row has the bits the single-mask path computes for it:
//   l2s_adaptive_pool_rows                            misc_kernels.hip, adaptive_pool_fwd's second instantiation
//   l2s_cap_att_dots_rows, l2s_cap_apply_gates_rows,
//   l2s_cap_att_apply_rows                            caption_step.hip, the bodies of the train step without what only backward reads
//   l2s_decode_pick_rows                              decode.hip, the greedy decision's two device functions, or a forced token
// What is left here has no single-mask kernel to share a body with:
//   l2s_masks_to_map     mask_resize_nearest_kernel (decode.hip) + mask_downsample_kernel (misc_kernels.hip) in one launch: the bins and the
//                        vote of a bin are pool_bins.h's for both, the pixel is read through the resize tables here
//   l2s_lstm_cell_rows   the top-down captioner's nn.LSTMCell on rows: topdown_cell_fwd_kernel's arithmetic with the products on MFMA tiles
//                        of rows, on purpose (another summation order, within the forward tolerance of the single-row cell), because the
//                        single-row kernel streams a whole weight matrix per row
// The recurrent step stays row-strided rather than one fused workgroup per row: a row reads its own patt [L][AH] and P [L][2R], 1.2 MB at
// the production widths, and one workgroup pulls that through ONE compute unit's L2 port - at rows = 8 that is 8 of 256 ports busy for
// about 8 us a token.  The strided grids spread every row over cdiv(L, 4) / cdiv(R, 16) workgroups and fill the device from one row on.
// Live rows: rows.h.
#include "common.h"
#include "../../include/lang2seg_hip.h"
#include "pil_resize.h"
#include "pool_bins.h"
#include "recur.h"
#include "rows.h"

namespace {

constexpr int ROWS_T = 256;
typedef float floatx4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- l2s_masks_to_map
// Workgroup = one row of map bins of one mask.  The PIL source columns of the whole blob row and the source rows of the bin row go to the
// LDS first (pil_nearest_src is a running float64 sum: every thread walks to its first index once, then steps), then one wave per bin
// votes as in mask_downsample_kernel.
__global__ __launch_bounds__(ROWS_T) void masks_to_map_kernel(const uint8_t* __restrict__ masks, int row0, const int* __restrict__ count, int mh, int mw,
                                                              int H, int W, int h, int w, float* out) {
  extern __shared__ int tab[];          // tx[W] | ty[bin rows]
  const int r = blockIdx.y, oy = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (!row_live(r, row0, count)) return;
  const int y0 = bin_lo(oy, H, h), y1 = bin_hi(oy, H, h);
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
  const auto px = [&](int yy, int xx) { return resize ? src[(long)ty[yy - y0] * mw + tx[xx]] : src[(long)yy * W + xx]; };
  for (int ox = tid >> 6; ox < w; ox += ROWS_T / 64) {
    const float v = wave_bin_vote(px, y0, y1, bin_lo(ox, W, w), bin_hi(ox, W, w), lane);
    if (lane == 0) out[(long)r * h * w + oy * w + ox] = v;
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
__global__ __launch_bounds__(256) void lstm_cell_rows_kernel(CellR a, int R, int rows, int group, int row0, const int* __restrict__ count) {
  __shared__ float red[4][MT][4][64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, j = lane & 15, kq = lane >> 4;
  const int u0 = blockIdx.x * CELL_U, m0 = blockIdx.y * (16 * MT);
  const int nlive = live_rows(rows / group, row0, count) * group;      // group rows per detection (l2s_lstm_cell_groups; 1: a row is a detection)
  if (m0 >= nlive) return;                              // (the whole workgroup: before any barrier)
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
        if (a.pre2) v += a.pre2[(long)(m / group) * a.ld_pre2 + q * R + unit];
        if (a.add0) v += a.add0[q * R + unit];
        if (a.add1) v += a.add1[q * R + unit];
        g[q] = v;
      }
      float act[4];
      lstm_cell_fwd(g, a.c_prev[(long)m * a.ld_cp + unit], a.c[(long)m * a.ld_c + unit], a.h[(long)m * a.ld_h + unit], act);
    }
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

static bool rows_seg_ok(const l2s_rows_seg& g, int rows) {
  return g.n == 0 || (g.n > 0 && g.x && g.w && g.ld >= g.n && (g.ldx >= g.n || rows == 1));
}
static bool rows_seg_vec(const l2s_rows_seg& g) {
  return g.n == 0 || !((g.n & 3) || (g.ld & 3) || (g.ldx & 3) || ((uintptr_t)g.x & 15) || ((uintptr_t)g.w & 15));
}
static int lstm_cell_launch(const l2s_lstm_rows* a, int R, int rows, int group, int row0, const int* count, hipStream_t s) {
  if (!a || R < 1 || rows < 1 || group < 1 || rows % group || row0 < 0 || !a->c_prev || !a->c || !a->h || !rows_seg_ok(a->seg[0], rows) || !rows_seg_ok(a->seg[1], rows) ||
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
    if (vec) L2S_LAUNCH((lstm_cell_rows_kernel<1, true>), g1, dim3(256), 0, s, k, R, rows, group, row0, count);
    else L2S_LAUNCH((lstm_cell_rows_kernel<1, false>), g1, dim3(256), 0, s, k, R, rows, group, row0, count);
  } else {
    if (vec) L2S_LAUNCH((lstm_cell_rows_kernel<2, true>), g2, dim3(256), 0, s, k, R, rows, group, row0, count);
    else L2S_LAUNCH((lstm_cell_rows_kernel<2, false>), g2, dim3(256), 0, s, k, R, rows, group, row0, count);
  }
  return l2s_check_launch();
}
extern "C" int l2s_lstm_cell_rows(const l2s_lstm_rows* a, int R, int rows, int row0, const int* count, hipStream_t s) {
  return lstm_cell_launch(a, R, rows, 1, row0, count, s);
}
// the cell on groups of `group` consecutive rows per detection (beam search on rows): row m is live iff detection m / group is, and pre2
// (the per-detection term: the top-down captioner's fcrow) is read at row m / group; everything else is per row as above
extern "C" int l2s_lstm_cell_groups(const l2s_lstm_rows* a, int R, int rows, int group, int row0, const int* count, hipStream_t s) {
  return lstm_cell_launch(a, R, rows, group, row0, count, s);
}

