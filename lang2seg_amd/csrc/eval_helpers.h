// Per-pixel and per-box helpers of the evaluation kernels (eval.hip) and the detection kernels (detect.hip): one text for both, and for
// host checks.  Every expression is float32 with separate roundings (fp contract off), see eval.hip.
#pragma once
#include "pil_resize.h"
#include <cmath>
#include <stdint.h>

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

// model/test.py detect_from_outputs on one (row, class): boxes = rois[:, 1:5] / scale, bbox_transform_inv_np, _clip_boxes to (im_h, im_w),
// all float32; exp() is float64 rounded to float32.  bbox_reg off: the box is repeated.  roi: the row's [5], d: its class's 4 deltas.
__host__ __device__ inline void eval_decode_box(const float* roi, const float* d, float im_scale, int im_h, int im_w, int bbox_reg, float* o) {
#pragma clang fp contract(off)
  float b[4];
  for (int k = 0; k < 4; ++k) b[k] = roi[1 + k] / im_scale;
  if (bbox_reg) {
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
}

// computeIoU_box(pred_box, gt_box / im_scale) >= 0.5 in float32, the host's order of operations (o: the box in the original image,
// gt_box: x1 y1 x2 y2 in the scaled image): one text for l2s_eval_pick and l2s_detect_gt_iou
__host__ __device__ inline int eval_box_hit(const float* o, const float* gt_box, float im_scale) {
#pragma clang fp contract(off)
  float g[4];
  for (int k = 0; k < 4; ++k) g[k] = gt_box[k] / im_scale;
  const float ix1 = fmaxf(o[0], g[0]), iy1 = fmaxf(o[1], g[1]), ix2 = fminf(o[2], g[2]), iy2 = fminf(o[3], g[3]);
  float inter = 0.f;
  if (ix1 < ix2 && iy1 < iy2) inter = (ix2 - ix1 + 1.f) * (iy2 - iy1 + 1.f);
  const float a1 = (o[2] - o[0] + 1.f) * (o[3] - o[1] + 1.f), a2 = (g[2] - g[0] + 1.f) * (g[3] - g[1] + 1.f);
  const float uni = a1 + a2 - inter;
  const float iou = inter / uni;
  return iou >= 0.5f ? 1 : 0;
}

#ifdef __HIPCC__
// the first step of a paste, by a workgroup of 256 threads: bytescale of the ms x ms probabilities * 255 over their own [min, max] -> src
__device__ inline void eval_bytescale_block(const float* prob, int mm, float* smin, float* smax, uint8_t* src) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
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
}
#endif
