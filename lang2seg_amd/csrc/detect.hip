// Every instance per sentence (model/detect_device.py): the full Mask R-CNN test path of the reference's
// pyutils/mask-faster-rcnn/lib/model/test.py next to its one-box pick, on the heads' outputs of one sentence.
//   l2s_detect_nms     :268-283  per class j >= 1: rows with cls_prob > thresh, ordered by score (ties: lower row), greedy NMS as
//                                cpu_nms (lib/nms/src/nms.c:35-63: +1 areas, ovr >= thresh suppresses); one workgroup per class
//   l2s_detect_select  :285-297  max_per_image over all classes (image_thresh = the max_per_image-th largest surviving score, ties
//                                stay), the detections in class order, the mask head's RoIs and labels
//   l2s_detect_paste   :310-344  recover_masks + > 122 of every kept detection's own-class mask probabilities into one canvas each
// All float arithmetic is float32 with separate roundings (fp contract off); the box decode is eval_helpers.h's, the one l2s_eval_pick
// uses.  Nothing here depends on scheduling: every output word has one writer, the sums are integer atomics.
#include "common.h"
#include "../../include/lang2seg_hip.h"
#include "eval_helpers.h"
#include <climits>

#define DET_T 1024                      // threads of an NMS / select workgroup
#define DET_Q 5                         // sorted candidates a thread owns: DET_T * DET_Q rows at most
#define DET_MAX_POST (DET_T * DET_Q)    // 5120 >= cfg.TEST.RPN_TOP_N (5000)
#define DET_SORT_N 8192                 // next power of two
#define DET_LDS_BOXES (DET_MAX_POST / 4)  // the score array's bytes hold this many boxes once the order is known
#define DET_MAX_CLS 1024
#define DET_ROWS 8                      // canvas rows per paste workgroup (eval.hip EVAL_ROWS)

namespace {

// workspace: per class the number of kept rows, then [C][post] kept rows, scores, boxes and the sorted candidates' boxes
struct DetWs {
  int* cnt; int* row; float* score; float4* box; float4* sbox;
  __host__ __device__ DetWs(void* ws, int post, int C) {
    const long n = (long)post * C;
    sbox = (float4*)ws; box = sbox + n;
    row = (int*)(box + n); score = (float*)(row + n); cnt = (int*)(score + n);
  }
};

// a total order on floats as unsigned integers (-0 counts as +0); NaN never gets here
__device__ __forceinline__ uint32_t det_key(float v) {
  const uint32_t b = v == 0.f ? 0u : __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float det_unkey(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// ---------------------------------------------------------------- l2s_detect_nms
__global__ __launch_bounds__(DET_T) void detect_nms_kernel(const float* cls_prob, const float* bbox_pred, const float* rois, const int* nkeep,
                                                            int post, int C, float im_scale, int im_h, int im_w, int bbox_reg, float thresh,
                                                            float nms_thresh, void* ws, float* boxes_dump) {
#pragma clang fp contract(off)
  __shared__ float4 sc_box[DET_LDS_BOXES];          // first the scores of the class's column (float [DET_MAX_POST]), then the sorted boxes
  __shared__ int idx[DET_SORT_N];                   // the order: rows, then (behind the candidates) INT_MAX
  __shared__ uint8_t sup[DET_MAX_POST];
  __shared__ int s_m;
  float* sc = (float*)sc_box;
  const int t = threadIdx.x, j = blockIdx.x;
  DetWs W(ws, post, C);
  int n = nkeep ? nkeep[0] : post;
  n = n < 0 ? 0 : (n > post ? post : n);
  if (boxes_dump)
    for (int r = t; r < post; r += DET_T) {
      float o[4];
      eval_decode_box(rois + (long)r * 5, bbox_pred ? bbox_pred + (long)r * 4 * C + 4 * j : rois, im_scale, im_h, im_w, bbox_reg, o);
      for (int k = 0; k < 4; ++k) boxes_dump[((long)r * C + j) * 4 + k] = o[k];
    }
  if (j == 0) {                                     // the background class has no detections
    if (t == 0) W.cnt[0] = 0;
    return;
  }
  // candidates: score > thresh (false for NaN)
  int P = 1;
  while (P < n) P <<= 1;
  if (t == 0) s_m = 0;
  __syncthreads();
  int mine = 0;
  for (int r = t; r < P; r += DET_T) {
    const float v = r < n ? cls_prob[(long)r * C + j] : 0.f;
    const bool cand = r < n && v > thresh;
    if (r < n) sc[r] = v;
    idx[r] = cand ? r : INT_MAX;
    mine += cand;
  }
  if (mine) atomicAdd(&s_m, mine);
  __syncthreads();
  const int m = s_m;
  // bitonic sort of the rows: score descending, ties by lower row, non-candidates last
  for (int k = 2; k <= P; k <<= 1)
    for (int s = k >> 1; s > 0; s >>= 1) {
      for (int i = t; i < P; i += DET_T) {
        const int l = i ^ s;
        if (l > i) {
          const int a = idx[i], b = idx[l];
          bool a_first;                             // a sorts before b
          if (a == INT_MAX || b == INT_MAX) a_first = b == INT_MAX;
          else {
            const float sa = sc[a], sb = sc[b];
            a_first = sa > sb || (sa == sb && a < b);
          }
          const bool up = (i & k) == 0;
          if (a_first != up) { idx[i] = b; idx[l] = a; }
        }
      }
      __syncthreads();
    }
  // the sorted candidates this thread owns (k = t + q * DET_T): row, score, box, area
  int row[DET_Q];
  float score[DET_Q], area[DET_Q];
  float4 bx[DET_Q];
#pragma unroll
  for (int q = 0; q < DET_Q; ++q) {
    const int k = t + q * DET_T;
    row[q] = k < m ? idx[k] : -1;
    score[q] = k < m ? sc[row[q]] : 0.f;
  }
  __syncthreads();                                  // the scores' bytes become the boxes'
  const bool in_lds = m <= DET_LDS_BOXES;
  float4* sbox = W.sbox + (long)j * post;
#pragma unroll
  for (int q = 0; q < DET_Q; ++q) {
    const int k = t + q * DET_T;
    bx[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    area[q] = 0.f;
    if (k < m) {
      float o[4];
      eval_decode_box(rois + (long)row[q] * 5, bbox_pred ? bbox_pred + (long)row[q] * 4 * C + 4 * j : rois, im_scale, im_h, im_w, bbox_reg, o);
      bx[q] = make_float4(o[0], o[1], o[2], o[3]);
      area[q] = (o[2] - o[0] + 1.f) * (o[3] - o[1] + 1.f);
      if (in_lds) sc_box[k] = bx[q]; else sbox[k] = bx[q];
      sup[k] = 0;
    }
  }
  __syncthreads();
  // greedy NMS: every thread walks the same list; a kept box suppresses the ones behind it in one parallel pass
  int nk = 0;
  for (int i = 0; i < m; ++i) {
    if (sup[i]) continue;                           // uniform: written before the last barrier
    const float4 p = in_lds ? sc_box[i] : sbox[i];
    const float parea = (p.z - p.x + 1.f) * (p.w - p.y + 1.f);
    if ((i & (DET_T - 1)) == t) {                   // its owner files it
      const int q = i / DET_T;
      const long o = (long)j * post + nk;
#pragma unroll
      for (int qq = 0; qq < DET_Q; ++qq)
        if (qq == q) { W.row[o] = row[qq]; W.score[o] = score[qq]; W.box[o] = bx[qq]; }
    }
    ++nk;
    if (i + 1 >= m) break;
#pragma unroll
    for (int q = 0; q < DET_Q; ++q) {
      const int k = t + q * DET_T;
      if (k > i && k < m) {
        const float xx1 = fmaxf(p.x, bx[q].x), yy1 = fmaxf(p.y, bx[q].y), xx2 = fminf(p.z, bx[q].z), yy2 = fminf(p.w, bx[q].w);
        const float w = fmaxf(0.f, xx2 - xx1 + 1.f), h = fmaxf(0.f, yy2 - yy1 + 1.f);
        const float inter = w * h;
        const float ovr = inter / (parea + area[q] - inter);
        if (ovr >= nms_thresh) sup[k] = 1;
      }
    }
    __syncthreads();
  }
  if (t == 0) W.cnt[j] = nk;
}

// ---------------------------------------------------------------- l2s_detect_select
__global__ __launch_bounds__(DET_T) void detect_select_kernel(const void* ws, int post, int C, int max_per_image, float im_scale,
                                                               l2s_det_record* rec, float* mask_rois, int* mask_labels, int cap, int* count) {
#pragma clang fp contract(off)
  __shared__ int cnt[DET_MAX_CLS], off[DET_MAX_CLS + 1];
  __shared__ int hist[256];
  __shared__ uint32_t s_prefix;
  __shared__ int s_rank;
  const int t = threadIdx.x;
  const DetWs W((void*)ws, post, C);
  for (int j = t; j < C; j += DET_T) cnt[j] = W.cnt[j];
  __syncthreads();
  if (t == 0) {
    int s = 0;
    for (int j = 0; j < C; ++j) { off[j] = s; s += cnt[j]; }
    off[C] = s;
  }
  __syncthreads();
  const long grid = (long)C * post;
  float image_thresh = -INFINITY;
  if (max_per_image > 0 && off[C] > max_per_image) {
    // radix select, most significant byte first: the max_per_image-th largest key among the survivors
    if (t == 0) { s_prefix = 0u; s_rank = max_per_image; }
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (t < 256) hist[t] = 0;
      __syncthreads();
      const uint32_t prefix = s_prefix, himask = shift == 24 ? 0u : ~0u << (shift + 8);
      for (long e = t; e < grid; e += DET_T) {
        const int j = (int)(e / post), k = (int)(e % post);
        if (k < cnt[j]) {
          const uint32_t u = det_key(W.score[e]);
          if ((u & himask) == prefix) atomicAdd(&hist[(u >> shift) & 255], 1);
        }
      }
      __syncthreads();
      if (t == 0) {
        int r = s_rank, b = 255;
        for (; b > 0; --b) {
          if (hist[b] >= r) break;
          r -= hist[b];
        }
        s_rank = r;
        s_prefix = prefix | ((uint32_t)b << shift);
      }
      __syncthreads();
    }
    image_thresh = det_unkey(s_prefix);
    // a class's scores descend: what stays is a prefix of its list
    __syncthreads();
    for (int j = t; j < C; j += DET_T) cnt[j] = 0;
    __syncthreads();
    for (long e = t; e < grid; e += DET_T) {
      const int j = (int)(e / post), k = (int)(e % post);
      if (k < W.cnt[j] && W.score[e] >= image_thresh) atomicAdd(&cnt[j], 1);
    }
    __syncthreads();
    if (t == 0) {
      int s = 0;
      for (int j = 0; j < C; ++j) { off[j] = s; s += cnt[j]; }
      off[C] = s;
    }
    __syncthreads();
  }
  const int total = off[C], written = total < cap ? total : cap;
  for (long e = t; e < grid; e += DET_T) {
    const int j = (int)(e / post), k = (int)(e % post);
    if (k >= cnt[j]) continue;
    const int d = off[j] + k;
    if (d >= cap) continue;
    const float4 b = W.box[e];
    l2s_det_record r;
    r.roi = W.row[e]; r.cls = j; r.box[0] = b.x; r.box[1] = b.y; r.box[2] = b.z; r.box[3] = b.w; r.score = W.score[e]; r.area = 0;
    rec[d] = r;
    float* mr = mask_rois + (long)d * 5;
    mr[0] = 0.f; mr[1] = b.x * im_scale; mr[2] = b.y * im_scale; mr[3] = b.z * im_scale; mr[4] = b.w * im_scale;
    mask_labels[d] = j;
  }
  for (int d = written + t; d < cap; d += DET_T) {
    l2s_det_record r;
    r.roi = 0; r.cls = 0; r.box[0] = r.box[1] = r.box[2] = r.box[3] = 0.f; r.score = 0.f; r.area = 0;
    rec[d] = r;
    for (int k = 0; k < 5; ++k) mask_rois[(long)d * 5 + k] = 0.f;
    mask_labels[d] = 0;
  }
  if (t == 0) { count[0] = written; count[1] = total; }
}

// ---------------------------------------------------------------- l2s_detect_paste
// eval.hip's eval_mask_iou_kernel without a ground truth and with the detection in the grid: one thread per canvas column,
// DET_ROWS canvas rows per workgroup
__global__ __launch_bounds__(256) void detect_paste_kernel(const float* mask_prob, int ms, l2s_det_record* rec, const int* count, int ih, int iw,
                                                           uint8_t* canvases) {
#pragma clang fp contract(off)
  __shared__ float smin[256], smax[256];
  __shared__ uint8_t src[L2S_PIL_MAX_TAPS * L2S_PIL_MAX_TAPS];
  __shared__ PilTaps tv[DET_ROWS];
  __shared__ int red[4];
  const int d = blockIdx.z;
  if (d >= count[0]) return;                        // uniform
  const int t = threadIdx.x, r0 = blockIdx.y * DET_ROWS, c = blockIdx.x * blockDim.x + t;
  const int mm = ms * ms;
  float box[4];
  for (int k = 0; k < 4; ++k) box[k] = rec[d].box[k];
  const EvalGeom g = eval_box_geometry(box, ih, iw);
  eval_bytescale_block(mask_prob + (long)d * mm, mm, smin, smax, src);
  if (t < DET_ROWS) {
    const int r = r0 + t;
    tv[t].n = 0; tv[t].xmin = 0;
    if (r < ih && r >= g.y && r < g.y + g.h && g.h != ms) pil_bilinear_taps(ms, g.h, r - g.y, tv[t]);
  }
  __syncthreads();
  int area = 0;
  if (c < iw) {
    uint8_t* canvas = canvases + (long)d * ih * iw;
    const bool in_x = c >= g.x && c < g.x + g.w;
    int tmp[L2S_PIL_MAX_TAPS];
    if (in_x) eval_column(src, ms, g.w, c - g.x, tmp);
    for (int i = 0; i < DET_ROWS; ++i) {
      const int r = r0 + i;
      if (r >= ih) break;
      int pred = 0;
      if (in_x && r >= g.y && r < g.y + g.h) pred = eval_vertical(tmp, ms, g.h, r - g.y, tv[i]) > 122;
      area += pred;
      canvas[(long)r * iw + c] = (uint8_t)pred;
    }
  }
  for (int o = 32; o > 0; o >>= 1) area += __shfl_down(area, o);
  if ((t & 63) == 0) red[t >> 6] = area;
  __syncthreads();
  if (t == 0) {
    const int s = red[0] + red[1] + red[2] + red[3];
    if (s) atomicAdd(&rec[d].area, s);
  }
}

}  // namespace

extern "C" size_t l2s_detect_ws_bytes(int post, int ncls) {
  if (post <= 0 || ncls <= 0) return 0;
  return (size_t)post * ncls * (2 * sizeof(float4) + sizeof(int) + sizeof(float)) + (size_t)ncls * sizeof(int);
}

extern "C" int l2s_detect_nms(const float* cls_prob, const float* bbox_pred, const float* rois, const int* nkeep, int post, int ncls,
                              float im_scale, int im_h, int im_w, int bbox_reg, float thresh, float nms_thresh, void* ws, float* boxes_dump,
                              hipStream_t s) {
  if (post <= 0 || post > DET_MAX_POST || ncls < 2 || ncls > DET_MAX_CLS || !cls_prob || !rois || !ws || (bbox_reg && !bbox_pred) ||
      !(im_scale > 0.f) || im_h <= 0 || im_w <= 0 || thresh != thresh || nms_thresh != nms_thresh)
    return L2S_EINVAL;
  L2S_LAUNCH(detect_nms_kernel, dim3(ncls), dim3(DET_T), 0, s, cls_prob, bbox_pred, rois, nkeep, post, ncls, im_scale, im_h, im_w, bbox_reg,
             thresh, nms_thresh, ws, boxes_dump);
  return l2s_check_launch();
}

extern "C" int l2s_detect_select(const void* ws, int post, int ncls, int max_per_image, float im_scale, l2s_det_record* rec, float* mask_rois,
                                 int* mask_labels, int cap, int* count, hipStream_t s) {
  if (post <= 0 || post > DET_MAX_POST || ncls < 2 || ncls > DET_MAX_CLS || !ws || !rec || !mask_rois || !mask_labels || !count || cap <= 0 ||
      !(im_scale > 0.f))
    return L2S_EINVAL;
  L2S_LAUNCH(detect_select_kernel, dim3(1), dim3(DET_T), 0, s, ws, post, ncls, max_per_image, im_scale, rec, mask_rois, mask_labels, cap, count);
  return l2s_check_launch();
}

extern "C" int l2s_detect_paste(const float* mask_prob, int ms, l2s_det_record* rec, const int* count, int cap, int ih, int iw, uint8_t* canvases,
                                hipStream_t s) {
  if (ms <= 0 || ms > L2S_PIL_MAX_TAPS || !mask_prob || !rec || !count || !canvases || cap <= 0 || cap > 65535 || ih <= 0 || iw <= 0 ||
      (long)ih * iw >= (1L << 31))
    return L2S_EINVAL;
  L2S_LAUNCH(detect_paste_kernel, dim3(cdiv(iw, 256), cdiv(ih, DET_ROWS), cap), dim3(256), 0, s, mask_prob, ms, rec, (const int*)count, ih, iw,
             canvases);
  return l2s_check_launch();
}
