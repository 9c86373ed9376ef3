// Every detection against the ground truth, and one detection per rule (model/detect_device.py _JudgeStage), behind l2s_detect_paste
// and the caption branch on rows:
//   l2s_detect_gt_iou   per detection the intersection / union pixel counts of its canvas with the sentence's gt mask (PIL NEAREST
//                       resized as l2s_eval_mask_iou reads it), and its box's hit against the gt box (eval_helpers.h eval_box_hit,
//                       the text l2s_eval_pick uses)
//   l2s_detect_choose   the detector's, the oracle's, the speaker's and the re-ranked choice among a sentence's detections
// All sums are integers (wave shuffles, then integer atomics): no result depends on scheduling.  The only floating point is the box
// hit (float32, fp contract off) and the re-rank key (float64, fp contract off).
#include "common.h"
#include "../../include/lang2seg_hip.h"
#include "eval_helpers.h"
#include <climits>
#include <cmath>

#define SEL_T 256                       // threads of a workgroup
#define SEL_ROWS 32                     // canvas rows of a workgroup
#define SEL_COLS 1024                   // columns whose gt source index a workgroup keeps in the LDS at a time (4 per thread)
#define SEL_WHOLE 8                     // workgroups that share SEL_ROWS rows of the resized gt (row i goes to workgroup i % SEL_WHOLE)
#define SEL_MAX_LAMBDA 8

namespace {

struct SelLambdas {
  float v[SEL_MAX_LAMBDA];
};

// the sum of v over the workgroup, in every thread (integers: exact in any order)
__device__ __forceinline__ int sel_block_sum(int v, int* red) {
  const int t = threadIdx.x;
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();                                  // red's readers of an earlier call
  if ((t & 63) == 0) red[t >> 6] = v;
  __syncthreads();
  int s = 0;
  for (int w = 0; w < SEL_T / 64; ++w) s += red[w];
  return s;
}

// ---------------------------------------------------------------- l2s_detect_gt_iou
// grid (cap + SEL_WHOLE, row blocks).  x = d < cap: SEL_ROWS rows of detection d's box (a canvas is zero outside eval_box_geometry of
// its record's box, and holds rec[d].area set pixels), so U = area + gt_area - I in integers.  x >= cap: every SEL_WHOLE-th of SEL_ROWS
// rows of the resized gt, whose set pixels go to gt_area and to every live detection's U.  out and gt_area are zero on entry.
// The pixels of a workgroup are one flat index space (row, word or column): a box is narrow, a loop over its rows would wait for one
// load after the other.
__global__ __launch_bounds__(SEL_T) void detect_gt_iou_kernel(const uint8_t* canvases, const l2s_det_record* rec, const int* count, int cap,
                                                              int ih, int iw, const uint8_t* gt, int Hs, int Ws, const float* gt_box,
                                                              float im_scale, l2s_det_gt* out, int* gt_area) {
  __shared__ int tx[SEL_COLS];
  __shared__ int ty[SEL_ROWS];
  __shared__ int red[SEL_T / 64];
  const int t = threadIdx.x, d = blockIdx.x;
  int n = count[0];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  const bool whole = d >= cap;                      // the gt's own pixels
  const int slice = whole ? d - cap : 0;
  int x0 = 0, y0 = 0, w = iw, h = ih;
  if (!whole) {
    if (d >= n) {                                   // uniform.  A row behind the count: zeros
      if (blockIdx.y == 0 && t == 0) { l2s_det_gt z; z.I = 0; z.U = 0; z.hit = 0; z.reserved = 0; out[d] = z; }
      return;
    }
    float box[4];
    for (int k = 0; k < 4; ++k) box[k] = rec[d].box[k];
    const EvalGeom g = eval_box_geometry(box, ih, iw);
    x0 = g.x; y0 = g.y; w = g.w; h = g.h;
    // (eval_box_geometry clips the box to the canvas; a guard for any geometry it could return)
    if (x0 < 0 || y0 < 0 || w < 0 || h < 0 || x0 + w > iw || y0 + h > ih) { x0 = 0; y0 = 0; w = iw; h = ih; }
    if (blockIdx.y == 0 && t == 0) {                // the parts of the row that need no pixel
      out[d].hit = eval_box_hit(box, gt_box, im_scale);
      if (rec[d].area) atomicAdd(&out[d].U, rec[d].area);
    }
  }
  const int r0 = y0 + blockIdx.y * SEL_ROWS;
  const int nr = min(SEL_ROWS, y0 + h - r0);
  const int mine = whole ? (nr - slice + SEL_WHOLE - 1) / SEL_WHOLE : nr;      // rows of this workgroup: i = slice + k * SEL_WHOLE
  if (nr <= 0 || mine <= 0 || w <= 0) return;       // uniform
  if (t >= SEL_T - SEL_ROWS) {                      // the last wave: the one with the fewest columns to walk to
    const int i = t - (SEL_T - SEL_ROWS);
    ty[i] = i < nr && (!whole || i % SEL_WHOLE == slice) ? pil_nearest_src(r0 + i, Hs, ih) : 0;
  }
  const double step = pil_nearest_step(Ws, iw);
  const uint8_t* canvas = whole ? nullptr : canvases + (long)d * ih * iw;
  int acc = 0;
  for (int cx = 0; cx < w; cx += SEL_COLS) {
    const int cw = min(SEL_COLS, w - cx);
    __syncthreads();                                // the last chunk's readers
    if (4 * t < cw) {                               // the gt's source column of 4 consecutive columns: one walk
      double xo = pil_nearest_xo(x0 + cx + 4 * t, Ws, iw);
      for (int j = 0; j < 4 && 4 * t + j < cw; ++j) {
        tx[4 * t + j] = pil_nearest_at(xo, Ws);
        xo += step;
      }
    }
    __syncthreads();                                // tx; ty
    if (whole) {
      const int items = mine * cw;
#pragma unroll 4
      for (int q = t; q < items; q += SEL_T) {
        const int k = q / cw, c = q - k * cw;
        acc += gt[(long)ty[slice + k * SEL_WHOLE] * Ws + tx[c]] != 0;
      }
      continue;
    }
    // a row's cw bytes from p on, as aligned 32-bit words; the words that straddle an end are read byte by byte
    const int wpr = cw / 4 + 2;                     // words a row can touch: ceil((head + cw) / 4) with head <= 3
    const int items = nr * wpr;
    for (int q = t; q < items; q += SEL_T) {
      const int i = q / wpr, j = q - i * wpr;
      const uint8_t* p = canvas + (long)(r0 + i) * iw + x0 + cx;
      const int head = (int)((uintptr_t)p & 3);
      if (4 * j >= head + cw) continue;
      const uint8_t* pa = p - head;
      const int lo = 4 * j - head;                  // the column (from cx) of the word's first byte
      uint32_t v = 0;
      if (lo >= 0 && lo + 4 <= cw) {
        v = *(const uint32_t*)(pa + 4 * j);
      } else {
        for (int b = 0; b < 4; ++b)
          if (lo + b >= 0 && lo + b < cw) v |= (uint32_t)pa[4 * j + b] << (8 * b);
      }
      if (v == 0) continue;
      const uint8_t* grow = gt + (long)ty[i] * Ws;
      for (int b = 0; b < 4; ++b)
        if ((v >> (8 * b)) & 0xffu) acc += grow[tx[lo + b]] != 0;
    }
  }
  const int s = sel_block_sum(acc, red);
  if (s == 0) return;
  if (whole) {
    if (t == 0) atomicAdd(gt_area, s);
    for (int k = t; k < n; k += SEL_T) atomicAdd(&out[k].U, s);
  } else if (t == 0) {
    atomicAdd(&out[d].I, s);
    atomicSub(&out[d].U, s);
  }
}

// ---------------------------------------------------------------- l2s_detect_choose
// rule 0 detector, 1 oracle, 2 speaker, 3 + k rerank@lambda_k.  The key of detection d under a rule that has one:
__device__ __forceinline__ double sel_key(int rule, int d, const l2s_det_record* rec, const float* expr, const SelLambdas& lam, double div) {
#pragma clang fp contract(off)
  if (rule == 0) return (double)rec[d].score;
  if (rule == 2) return (double)expr[d];
  const double a = log((double)rec[d].score);
  const double b = (double)lam.v[rule - 3] * (double)expr[d];
  return a + b / div;
}
// one candidate: its index (-1: none), its key (rules with one) or its I / U (the oracle; U = 0 counts as 0 / 1)
struct SelCand {
  int d;
  double key;
  long long I, U;
};
// candidate a is chosen over candidate b: strictly better, or as good with the lower index.  The oracle compares I_a / U_a with
// I_b / U_b exactly, in 64-bit integers
__device__ __forceinline__ bool sel_beats(int rule, const SelCand& a, const SelCand& b) {
  if (b.d < 0) return a.d >= 0;
  if (a.d < 0) return false;
  if (rule == 1) {
    const long long l = a.I * b.U, r = b.I * a.U;
    return l > r || (l == r && a.d < b.d);
  }
  return a.key > b.key || (!(b.key > a.key) && a.d < b.d);
}

__global__ __launch_bounds__(SEL_T) void detect_choose_kernel(const l2s_det_record* rec, const l2s_det_gt* gt, const int* count, int cap,
                                                              const int* gt_area, const float* expr, SelLambdas lam, int n_lambda, int per_token,
                                                              int n_tok, l2s_det_choice* out) {
#pragma clang fp contract(off)
  __shared__ SelCand best[SEL_T];
  const int t = threadIdx.x;
  int n = count[0];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  const int rules = 2 + (expr ? 1 + n_lambda : 0);
  const double div = per_token ? (double)n_tok : 1.0;
  for (int rule = 0; rule < rules; ++rule) {
    SelCand mine;
    mine.d = -1; mine.key = 0.0; mine.I = 0; mine.U = 1;
    for (int d = t; d < n; d += SEL_T) {            // every key is computed once; ascending, so a later index has to be strictly better
      SelCand c;
      c.d = d; c.key = 0.0; c.I = 0; c.U = 1;
      if (rule == 1) {
        if (gt[d].U) { c.I = gt[d].I; c.U = gt[d].U; }
      } else {
        c.key = sel_key(rule, d, rec, expr, lam, div);
      }
      if (sel_beats(rule, c, mine)) mine = c;
    }
    __syncthreads();                                // the last rule's reader
    best[t] = mine;
    __syncthreads();
    for (int o = SEL_T >> 1; o > 0; o >>= 1) {
      if (t < o && sel_beats(rule, best[t + o], best[t])) best[t] = best[t + o];
      __syncthreads();
    }
    if (t == 0) {
      const int d = best[0].d;
      l2s_det_choice c;
      c.det = d; c.reserved = 0;
      if (d < 0) {
        c.cls = -1; c.hit = 0; c.I = 0; c.U = gt_area[0]; c.key = 0.0;
      } else {
        c.cls = rec[d].cls; c.hit = gt[d].hit; c.I = gt[d].I; c.U = gt[d].U;
        c.key = rule == 1 ? (gt[d].U ? (double)gt[d].I / (double)gt[d].U : 0.0) : best[0].key;
      }
      out[rule] = c;
    }
  }
}

}  // namespace

extern "C" int l2s_detect_gt_iou(const uint8_t* canvases, const l2s_det_record* rec, const int* count, int cap, int ih, int iw, const uint8_t* gt,
                                 int Hs, int Ws, const float* gt_box, float im_scale, l2s_det_gt* out, int* gt_area, hipStream_t s) {
  if (!canvases || !rec || !count || !gt || !gt_box || !out || !gt_area || cap <= 0 || cap > 65535 || ih <= 0 || iw <= 0 || Hs <= 0 || Ws <= 0 ||
      (long)ih * iw >= (1L << 31) || cdiv(ih, SEL_ROWS) > 65535 || !(im_scale > 0.f))
    return L2S_EINVAL;
  L2S_LAUNCH(detect_gt_iou_kernel, dim3(cap + SEL_WHOLE, cdiv(ih, SEL_ROWS)), dim3(SEL_T), 0, s, canvases, rec, count, cap, ih, iw, gt, Hs, Ws,
             gt_box, im_scale, out, gt_area);
  return l2s_check_launch();
}

extern "C" int l2s_detect_choose(const l2s_det_record* rec, const l2s_det_gt* gt, const int* count, int cap, const int* gt_area, const float* expr,
                                 const float* lambdas, int n_lambda, int per_token, int n_tok, l2s_det_choice* out, hipStream_t s) {
  if (!rec || !gt || !count || !gt_area || !out || cap <= 0 || n_lambda < 0 || n_lambda > SEL_MAX_LAMBDA || (n_lambda > 0 && (!expr || !lambdas)) ||
      (per_token && n_tok <= 0))
    return L2S_EINVAL;
  SelLambdas lam;
  for (int k = 0; k < SEL_MAX_LAMBDA; ++k) lam.v[k] = k < n_lambda ? lambdas[k] : 0.f;
  L2S_LAUNCH(detect_choose_kernel, dim3(1), dim3(SEL_T), 0, s, rec, gt, count, cap, gt_area, expr, lam, n_lambda, per_token, n_tok, out);
  return l2s_check_launch();
}
