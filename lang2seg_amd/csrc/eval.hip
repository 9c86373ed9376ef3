// Evaluation on the device (model/eval_device.py): the per-sentence host post-processing of model/test.py eval_split as two launches.
//   l2s_eval_pick      best_detection + detect_from_outputs + computeIoU_box on the chosen row, the mask head's RoI
//                      (model/test.py:41-87, reference test.py:97-176,257-260)
//   l2s_eval_mask_iou  segment_from_mask_prob (recover_masks: bytescale, PIL BILINEAR resize, paste, > 122) + PIL NEAREST resize of
//                      the gt mask + computeIoU_seg (utils/mask_utils.py, model/test.py:90-95,138-141)
// Every expression is restated operation by operation in the host's precision (float32 where numpy works in float32, float64
// where Pillow does); products and sums round separately (fp contract off).  The one exception is exp() of the box deltas:
// numpy's float32 exp is not correctly rounded, the device takes float64 exp rounded to float32 (a few ulp apart at most).
#include "common.h"
#include "../../include/lang2seg_hip.h"
#include "pil_resize.h"
#include <climits>
#include <cmath>

namespace {

// ---------------------------------------------------------------- helpers (host + device: one text for kernels and checks)
struct EvalGeom {
  int x, y, w, h;
};
// mask_utils.recover_masks on one float32 box: clip_np_boxes, then h = int(y2 - y1 + 1), w = int(x2 - x1 + 1), x = int(x1), y = int(y1)
__host__ __device__ inline EvalGeom eval_box_geometry(const float* box, int ih, int iw) {
#pragma clang fp contract(off)
  const float xm = (float)(iw - 1), ym = (float)(ih - 1);
  const float x1 = fmaxf(fminf(box[0], xm), 0.f), y1 = fmaxf(fminf(box[1], ym), 0.f);
  const float x2 = fmaxf(fminf(box[2], xm), 0.f), y2 = fmaxf(fminf(box[3], ym), 0.f);
  EvalGeom g;
  const float fh = y2 - y1 + 1.f, fw = x2 - x1 + 1.f;
  const bool ok = fh == fh && fw == fw && fh > 0.f && fw > 0.f;        // a NaN box pastes nothing
  g.h = ok ? (int)fh : 0;
  g.w = ok ? (int)fw : 0;
  g.x = ok ? (int)x1 : 0;
  g.y = ok ? (int)y1 : 0;
  return g;
}
// mask *= 255. then scipy's bytescale in float32 (NumPy 2 keeps every step in float32): cscale = cmax - cmin (0 -> 1),
// scale = 255 / cscale, (x - cmin) * scale, clip to [0, 255], + 0.5, truncate to uint8
__host__ __device__ inline int eval_bytescale_one(float x255, float cmin, float scale) {
#pragma clang fp contract(off)
  float v = (x255 - cmin) * scale;
  v = fminf(fmaxf(v, 0.f), 255.f);
  v = v + 0.5f;
  return (int)v;
}
__host__ __device__ inline float eval_bytescale_factor(float cmin, float cmax) {
#pragma clang fp contract(off)
  const float cscale = cmax - cmin;
  return cscale == 0.f ? 255.f : 255.f / cscale;
}
// the horizontal pass of Pillow's two-pass resize for output column xx of a w-wide box: the uint8 intermediate of every source row
// (src [ms][ms], row-major); a pass whose size does not change is skipped (need_horizontal)
__host__ __device__ inline void eval_column(const uint8_t* src, int ms, int w, int xx, int* tmp) {
  if (w == ms) {
    for (int y = 0; y < ms; ++y) tmp[y] = src[y * ms + xx];
    return;
  }
  PilTaps th;
  pil_bilinear_taps(ms, w, xx, th);
  for (int y = 0; y < ms; ++y) {
    int ss = 1 << (L2S_PIL_PRECISION_BITS - 1);
    for (int x = 0; x < th.n; ++x) ss += src[y * ms + th.xmin + x] * th.k[x];
    tmp[y] = pil_clip8(ss);
  }
}
// the vertical pass for output row yy (taps tv of that row, unused when h == ms)
__host__ __device__ inline int eval_vertical(const int* tmp, int ms, int h, int yy, const PilTaps& tv) {
  if (h == ms) return tmp[yy];
  int ss = 1 << (L2S_PIL_PRECISION_BITS - 1);
  for (int y = 0; y < tv.n; ++y) ss += tmp[tv.xmin + y] * tv.k[y];
  return pil_clip8(ss);
}

// ---------------------------------------------------------------- l2s_eval_pick
__global__ __launch_bounds__(256) void eval_pick_kernel(const float* cls_prob, const float* bbox_pred, const float* rois, const int* nkeep,
                                                        int post, int C, float im_scale, int im_h, int im_w, const float* gt_box, int bbox_reg,
                                                        l2s_eval_record* rec, float* mask_roi, int* mask_label) {
#pragma clang fp contract(off)
  __shared__ float smax[256];
  __shared__ int sidx[256];
  const int t = threadIdx.x;
  int n = nkeep ? nkeep[0] : post;
  n = n < 0 ? 0 : (n > post ? post : n);
  const long tot = (long)n * C;
  // max(scores[:n, 1:])
  float m = -INFINITY;
  for (long i = t; i < tot; i += blockDim.x)
    if (i % C >= 1) m = fmaxf(m, cls_prob[i]);
  smax[t] = m;
  __syncthreads();
  for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
    if (t < o) smax[t] = fmaxf(smax[t], smax[t + o]);
    __syncthreads();
  }
  const float best = smax[0];
  // np.where(scores == best)[.][0]: the first (row, col) in row-major order over ALL columns (the background column can win a tie)
  int first = INT_MAX;
  for (long i = t; i < tot; i += blockDim.x)
    if (cls_prob[i] == best) { first = (int)i; break; }
  sidx[t] = first;
  __syncthreads();
  for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
    if (t < o) sidx[t] = min(sidx[t], sidx[t + o]);
    __syncthreads();
  }
  if (t != 0) return;
  l2s_eval_record r;
  r.I = 0; r.U = 0; r.reserved = 0;
  if (n == 0 || C < 2 || sidx[0] == INT_MAX) {             // nothing to pick (the host loop raises there): marked, no box, no mask
    r.roi = -1; r.cls = -1; r.hit = 0;
    for (int k = 0; k < 4; ++k) r.box[k] = 0.f;
    *rec = r;
    for (int k = 0; k < 5; ++k) mask_roi[k] = 0.f;
    *mask_label = 0;
    return;
  }
  const int row = sidx[0] / C, cls = sidx[0] % C;
  // detect_from_outputs on the chosen row: boxes = rois[:, 1:5] / scale, bbox_transform_inv_np, _clip_boxes (all float32)
  float b[4], o[4];
  for (int k = 0; k < 4; ++k) b[k] = rois[(long)row * 5 + 1 + k] / im_scale;
  if (bbox_reg) {
    const float* d = bbox_pred + (long)row * 4 * C + 4 * cls;
    const float widths = b[2] - b[0] + 1.f, heights = b[3] - b[1] + 1.f;
    const float ctr_x = b[0] + 0.5f * widths, ctr_y = b[1] + 0.5f * heights;
    const float pcx = d[0] * widths + ctr_x, pcy = d[1] * heights + ctr_y;
    const float pw = (float)exp((double)d[2]) * widths, ph = (float)exp((double)d[3]) * heights;
    o[0] = pcx - 0.5f * pw; o[1] = pcy - 0.5f * ph; o[2] = pcx + 0.5f * pw; o[3] = pcy + 0.5f * ph;
    o[0] = fmaxf(o[0], 0.f); o[1] = fmaxf(o[1], 0.f);
    o[2] = fminf(o[2], (float)(im_w - 1)); o[3] = fminf(o[3], (float)(im_h - 1));
  } else {
    for (int k = 0; k < 4; ++k) o[k] = b[k];
  }
  // computeIoU_box(pred_box, gt_box / im_scale) >= 0.5 in float32, the host's order of operations
  float g[4];
  for (int k = 0; k < 4; ++k) g[k] = gt_box[k] / im_scale;
  const float ix1 = fmaxf(o[0], g[0]), iy1 = fmaxf(o[1], g[1]), ix2 = fminf(o[2], g[2]), iy2 = fminf(o[3], g[3]);
  float inter = 0.f;
  if (ix1 < ix2 && iy1 < iy2) inter = (ix2 - ix1 + 1.f) * (iy2 - iy1 + 1.f);
  const float a1 = (o[2] - o[0] + 1.f) * (o[3] - o[1] + 1.f), a2 = (g[2] - g[0] + 1.f) * (g[3] - g[1] + 1.f);
  const float uni = a1 + a2 - inter;
  const float iou = inter / uni;
  r.roi = row; r.cls = cls; r.hit = iou >= 0.5f ? 1 : 0;
  for (int k = 0; k < 4; ++k) r.box[k] = o[k];
  *rec = r;
  // the mask head's RoI: np.array([pred_box]) * im_scale (float32) behind a zero batch index
  mask_roi[0] = 0.f;
  for (int k = 0; k < 4; ++k) mask_roi[1 + k] = o[k] * im_scale;
  *mask_label = cls;
}

// ---------------------------------------------------------------- l2s_eval_mask_iou
// One thread per canvas column, EVAL_ROWS canvas rows per workgroup; the canvas itself is never stored (unless dumped).
#define EVAL_ROWS 8
__global__ __launch_bounds__(256) void eval_mask_iou_kernel(const float* prob, int ms, l2s_eval_record* rec, const uint8_t* gt, int Hs, int Ws,
                                                            int ih, int iw, uint8_t* canvas) {
#pragma clang fp contract(off)
  __shared__ float smin[256], smax[256];
  __shared__ uint8_t src[L2S_PIL_MAX_TAPS * L2S_PIL_MAX_TAPS];
  __shared__ PilTaps tv[EVAL_ROWS];
  __shared__ int ty[EVAL_ROWS];
  __shared__ int red[2][4];
  const int t = threadIdx.x, r0 = blockIdx.y * EVAL_ROWS, c = blockIdx.x * blockDim.x + t;
  const int mm = ms * ms;
  float box[4];
  for (int k = 0; k < 4; ++k) box[k] = rec->box[k];
  const bool valid = rec->roi >= 0;
  const EvalGeom g = eval_box_geometry(box, ih, iw);
  // bytescale of the 14 x 14 probabilities * 255 over their own [min, max]
  const float x255 = t < mm ? prob[t] * 255.f : 0.f;
  smin[t] = t < mm ? x255 : INFINITY;
  smax[t] = t < mm ? x255 : -INFINITY;
  __syncthreads();
  for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
    if (t < o) { smin[t] = fminf(smin[t], smin[t + o]); smax[t] = fmaxf(smax[t], smax[t + o]); }
    __syncthreads();
  }
  const float cmin = smin[0], scale = eval_bytescale_factor(cmin, smax[0]);
  if (t < mm) src[t] = (uint8_t)eval_bytescale_one(x255, cmin, scale);
  if (t < EVAL_ROWS) {
    const int r = r0 + t;
    ty[t] = r < ih ? pil_nearest_src(r, Hs, ih) : 0;
    tv[t].n = 0; tv[t].xmin = 0;
    if (valid && r < ih && r >= g.y && r < g.y + g.h && g.h != ms) pil_bilinear_taps(ms, g.h, r - g.y, tv[t]);
  }
  __syncthreads();
  int cI = 0, cU = 0;
  if (c < iw) {
    const int tx = pil_nearest_src(c, Ws, iw);
    const bool in_x = valid && c >= g.x && c < g.x + g.w;
    int tmp[L2S_PIL_MAX_TAPS];
    if (in_x) eval_column(src, ms, g.w, c - g.x, tmp);
    for (int i = 0; i < EVAL_ROWS; ++i) {
      const int r = r0 + i;
      if (r >= ih) break;
      int pred = 0;
      if (in_x && r >= g.y && r < g.y + g.h) pred = eval_vertical(tmp, ms, g.h, r - g.y, tv[i]) > 122;
      const int gv = gt[(long)ty[i] * Ws + tx] != 0;
      cI += pred & gv;
      cU += pred | gv;
      if (canvas) canvas[(long)r * iw + c] = (uint8_t)pred;
    }
  }
  // integer sums: exact, independent of order
  for (int o = 32; o > 0; o >>= 1) {
    cI += __shfl_down(cI, o);
    cU += __shfl_down(cU, o);
  }
  if ((t & 63) == 0) { red[0][t >> 6] = cI; red[1][t >> 6] = cU; }
  __syncthreads();
  if (t == 0) {
    long long sI = 0, sU = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { sI += red[0][w]; sU += red[1][w]; }
    if (sI) atomicAdd((unsigned long long*)&rec->I, (unsigned long long)sI);
    if (sU) atomicAdd((unsigned long long*)&rec->U, (unsigned long long)sU);
  }
}

}  // namespace

extern "C" int l2s_eval_pick(const float* cls_prob, const float* bbox_pred, const float* rois, const int* nkeep, int post, int ncls,
                             float im_scale, int im_h, int im_w, const float* gt_box, int bbox_reg, l2s_eval_record* rec, float* mask_roi,
                             int* mask_label, hipStream_t s) {
  if (post <= 0 || ncls <= 0 || !cls_prob || !rois || !gt_box || !rec || !mask_roi || !mask_label || (bbox_reg && !bbox_pred) ||
      !(im_scale > 0.f) || (long)post * ncls >= INT_MAX)
    return L2S_EINVAL;
  L2S_LAUNCH(eval_pick_kernel, dim3(1), dim3(256), 0, s, cls_prob, bbox_pred, rois, nkeep, post, ncls, im_scale, im_h, im_w, gt_box, bbox_reg,
             rec, mask_roi, mask_label);
  return l2s_check_launch();
}

extern "C" int l2s_eval_mask_iou(const float* mask_prob, int ms, l2s_eval_record* rec, const uint8_t* gt, int Hs, int Ws, int ih, int iw,
                                 uint8_t* canvas, hipStream_t s) {
  if (ms <= 0 || ms > L2S_PIL_MAX_TAPS || !mask_prob || !rec || !gt || Hs <= 0 || Ws <= 0 || ih <= 0 || iw <= 0) return L2S_EINVAL;
  L2S_LAUNCH(eval_mask_iou_kernel, dim3(cdiv(iw, 256), cdiv(ih, EVAL_ROWS)), dim3(256), 0, s, mask_prob, ms, rec, gt, Hs, Ws, ih, iw, canvas);
  return l2s_check_launch();
}
