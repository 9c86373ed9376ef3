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
#include "eval_helpers.h"
#include <climits>
#include <cmath>

namespace {

// (the helpers shared with detect.hip - box geometry, bytescale, the two resize passes, the box decode - are in eval_helpers.h)
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
  float o[4];
  eval_decode_box(rois + (long)row * 5, bbox_pred ? bbox_pred + (long)row * 4 * C + 4 * cls : rois, im_scale, im_h, im_w, bbox_reg, o);
  // computeIoU_box(pred_box, gt_box / im_scale) >= 0.5 in float32, the host's order of operations (eval_helpers.h)
  r.roi = row; r.cls = cls; r.hit = eval_box_hit(o, gt_box, im_scale);
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
  eval_bytescale_block(prob, mm, smin, smax, src);
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
