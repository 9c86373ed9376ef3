// Output side of evaluation and prediction (model/eval_device.py, model/predict_device.py): the predicted canvas leaves the device as
// COCO run lengths instead of pixels.
//   l2s_rle_from_mask   device   pyutils/refer/external/maskApi.c:32-41 (rleEncode), the counterpart of l2s_rle_to_mask (data.hip)
//   l2s_rle_from_masks  device   the same for n masks of one size in the same three launches (model/detect_device.py)
//   l2s_rle_to_string   host     maskApi.c:203-215 (rleToString), the counterpart of l2s_rle_from_string
//
// rleEncode walks the mask in column-major order k = x * h + y and emits a count whenever p[k] != p[k - 1], with p[-1] = 0.  That test
// is local, so the sequence is cut into chunks of RLE_SEG rows of one column (chunk c = x * nseg + seg, in sequence order) and
//   1. rle_count_kernel  one lane per chunk, lanes on adjacent columns (every row read is one coalesced line of the row-major canvas):
//                        the chunk's RLE_SEG pixels as a 64-bit word, its transitions t = bits ^ (bits << 1 | predecessor), their
//                        number popcount(t) and the position of the last one;
//   2. rle_scan_kernel   ONE workgroup: exclusive sum of the chunk counts (where each chunk's counts start) and exclusive maximum of
//                        the last positions (the transition before each chunk's first); then the pool decision on the device: the
//                        span, the bump of the cursor and the closing count h * w - last;
//   3. rle_write_kernel  one lane per chunk again: the j-th set bit of t is a transition at k, its count is k - (previous transition).
// Phases are separate launches; nothing waits on another workgroup.  Every output word has exactly one writer and the cursor is
// read and bumped by one thread, so the bytes do not depend on scheduling.
#include "common.h"
#include "../../include/lang2seg_hip.h"
#include <climits>

#define RLE_SEG 64          // rows per chunk: one bit per row in a 64-bit word
#define RLE_SCAN_T 1024

namespace {

// ws: [0] 1 if the counts fit the pool, [1] their first pool word; then per chunk (sequence order) four arrays of nchunks words
struct RleWs {
  uint32_t* hdr; uint32_t* tlo; uint32_t* thi; uint32_t* cnt; int* last;
  __host__ __device__ RleWs(uint32_t* ws, long nch) : hdr(ws), tlo(ws + 8), thi(ws + 8 + nch), cnt(ws + 8 + 2 * nch), last((int*)(ws + 8 + 3 * nch)) {}
};

// (count and write take the mask index in the grid's z: mask b is mask + b * h * w with its own ws_stride words of workspace; masks at
// b >= *n_valid are skipped.  l2s_rle_from_mask is the grid of one mask with n_valid NULL.)
__global__ __launch_bounds__(256) void rle_count_kernel(const uint8_t* mask, int h, int w, int nseg, uint32_t* ws, long ws_stride, const int* n_valid) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, seg = blockIdx.y;
  if (x >= w) return;
  if (n_valid && (int)blockIdx.z >= *n_valid) return;
  mask += (long)blockIdx.z * h * w;
  ws += (long)blockIdx.z * ws_stride;
  const int r0 = seg * RLE_SEG, nr = min(RLE_SEG, h - r0);
  // the pixel before the chunk in column-major order: the row above, else the last row of the column to the left, else p[-1] = 0
  uint64_t prev = 0;
  if (r0 > 0) prev = mask[(long)(r0 - 1) * w + x] != 0;
  else if (x > 0) prev = mask[(long)(h - 1) * w + x - 1] != 0;
  const uint8_t* p = mask + (long)r0 * w + x;
  uint64_t bits = 0;
#pragma unroll 8
  for (int i = 0; i < nr; ++i) bits |= (uint64_t)(p[(long)i * w] != 0) << i;
  uint64_t t = bits ^ ((bits << 1) | prev);
  if (nr < 64) t &= (1ull << nr) - 1;
  const long nch = (long)w * nseg, c = (long)x * nseg + seg;
  RleWs W(ws, nch);
  W.tlo[c] = (uint32_t)t; W.thi[c] = (uint32_t)(t >> 32);
  W.cnt[c] = (uint32_t)__popcll(t);
  W.last[c] = t ? x * h + r0 + 63 - __clzll((long long)t) : -1;
}

// inclusive scans inside a wave (sum, max), the fixed order of a Hillis-Steele ladder
__device__ __forceinline__ void wave_scan(uint32_t& s, int& m) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t vs = __shfl_up(s, o);
    const int vm = __shfl_up(m, o);
    if (lane >= o) { s += vs; m = max(m, vm); }
  }
}

// the scan and the pool decision of one mask by one workgroup (wsum, wmax: its shared scratch, free again behind the scan's last barrier)
__device__ __forceinline__ void rle_scan_one(long nch, int hw, uint32_t* ws, uint32_t* pool, int pool_words, int* cursor, l2s_rle_span* span,
                                             uint32_t* wsum, int* wmax) {
  RleWs W(ws, nch);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  uint32_t carry_s = 0; int carry_m = -1;                 // the same in every thread
  for (long base = 0; base < nch; base += RLE_SCAN_T) {
    const long c = base + t;
    const uint32_t s0 = c < nch ? W.cnt[c] : 0u;
    const int m0 = c < nch ? W.last[c] : -1;
    uint32_t s = s0; int m = m0;
    wave_scan(s, m);
    if (lane == 63) { wsum[wv] = s; wmax[wv] = m; }
    __syncthreads();
    uint32_t ps = carry_s, ts = carry_s; int pm = carry_m, tm = carry_m;
    for (int i = 0; i < RLE_SCAN_T / 64; ++i) {
      if (i == wv) { ps = ts; pm = tm; }
      ts += wsum[i]; tm = max(tm, wmax[i]);
    }
    // exclusive: everything before this element
    const uint32_t es = ps + s - s0;
    int em = __shfl_up(m, 1);
    em = lane == 0 ? pm : max(pm, em);
    if (c < nch) { W.cnt[c] = es; W.last[c] = em; }
    carry_s = ts; carry_m = tm;
    __syncthreads();
  }
  if (t != 0) return;                                     // (no barrier follows in this function)
  const long n = (long)carry_s + 1;                       // transitions + the closing run
  const long off = *cursor;
  const bool fits = off >= 0 && off + n <= (long)pool_words;
  W.hdr[0] = fits ? 1u : 0u;
  W.hdr[1] = fits ? (uint32_t)off : 0u;
  span->off = fits ? (int)off : -1;
  span->n = (int)(n > INT_MAX ? INT_MAX : n);
  if (fits) {
    pool[off + n - 1] = (uint32_t)(hw - (carry_m < 0 ? 0 : carry_m));
    *cursor = (int)(off + n);
  }
}

__global__ __launch_bounds__(RLE_SCAN_T) void rle_scan_kernel(long nch, int hw, uint32_t* ws, uint32_t* pool, int pool_words, int* cursor,
                                                              l2s_rle_span* span) {
  __shared__ uint32_t wsum[RLE_SCAN_T / 64];
  __shared__ int wmax[RLE_SCAN_T / 64];
  rle_scan_one(nch, hw, ws, pool, pool_words, cursor, span, wsum, wmax);
}

// the masks in order: the pool decision is sequential (a mask either fits behind its predecessors or leaves the cursor alone).  Thread 0
// alone reads and bumps the cursor, so it sees its own earlier writes.
__global__ __launch_bounds__(RLE_SCAN_T) void rle_scan_batch_kernel(int n, const int* n_valid, long nch, int hw, uint32_t* ws, long ws_stride,
                                                                    uint32_t* pool, int pool_words, int* cursor, l2s_rle_span* spans) {
  __shared__ uint32_t wsum[RLE_SCAN_T / 64];
  __shared__ int wmax[RLE_SCAN_T / 64];
  int nv = *n_valid;
  nv = nv < 0 ? 0 : (nv > n ? n : nv);
  for (int b = 0; b < nv; ++b) rle_scan_one(nch, hw, ws + (long)b * ws_stride, pool, pool_words, cursor, spans + b, wsum, wmax);
  for (int b = nv + threadIdx.x; b < n; b += RLE_SCAN_T) { spans[b].off = 0; spans[b].n = 0; }
}

__global__ __launch_bounds__(256) void rle_write_kernel(int h, int w, int nseg, const uint32_t* ws, long ws_stride, const int* n_valid, uint32_t* pool) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, seg = blockIdx.y;
  if (x >= w) return;
  if (n_valid && (int)blockIdx.z >= *n_valid) return;
  ws += (long)blockIdx.z * ws_stride;
  const long nch = (long)w * nseg, c = (long)x * nseg + seg;
  const RleWs W((uint32_t*)ws, nch);
  if (!W.hdr[0]) return;                                  // the pool is too small: nothing is written
  uint64_t t = (uint64_t)W.tlo[c] | ((uint64_t)W.thi[c] << 32);
  if (!t) return;
  uint32_t* out = pool + W.hdr[1] + W.cnt[c];
  int prev = W.last[c] < 0 ? 0 : W.last[c];
  const int k0 = x * h + seg * RLE_SEG;
  while (t) {
    const int k = k0 + __ffsll((long long)t) - 1;
    *out++ = (uint32_t)(k - prev);
    prev = k;
    t &= t - 1;
  }
}

}  // namespace

extern "C" int l2s_rle_encode_chunk_rows(void) { return RLE_SEG; }

extern "C" long l2s_rle_encode_ws_words(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  return 8 + 4 * (long)w * cdiv(h, RLE_SEG);
}

extern "C" int l2s_rle_from_mask(const uint8_t* mask, int h, int w, uint32_t* pool, int pool_words, int* cursor, l2s_rle_span* span,
                                 uint32_t* ws, hipStream_t s) {
  if (!mask || !pool || !cursor || !span || !ws || h <= 0 || w <= 0 || pool_words < 0 || (long)h * w >= (1L << 31)) return L2S_EINVAL;
  const int nseg = cdiv(h, RLE_SEG);
  const long nch = (long)w * nseg;
  const dim3 grid(cdiv(w, 256), nseg);
  L2S_LAUNCH(rle_count_kernel, grid, dim3(256), 0, s, mask, h, w, nseg, ws, 0L, (const int*)nullptr);
  L2S_LAUNCH(rle_scan_kernel, dim3(1), dim3(RLE_SCAN_T), 0, s, nch, h * w, ws, pool, pool_words, cursor, span);
  L2S_LAUNCH(rle_write_kernel, grid, dim3(256), 0, s, h, w, nseg, (const uint32_t*)ws, 0L, (const int*)nullptr, pool);
  return l2s_check_launch();
}

extern "C" int l2s_rle_from_masks(const uint8_t* masks, int n, const int* n_valid, int h, int w, uint32_t* pool, int pool_words, int* cursor,
                                  l2s_rle_span* spans, uint32_t* ws, hipStream_t s) {
  if (!masks || !n_valid || !pool || !cursor || !spans || !ws || n <= 0 || n > 65535 || h <= 0 || w <= 0 || pool_words < 0 ||
      (long)h * w >= (1L << 31))
    return L2S_EINVAL;
  const int nseg = cdiv(h, RLE_SEG);
  const long nch = (long)w * nseg, stride = l2s_rle_encode_ws_words(h, w);
  const dim3 grid(cdiv(w, 256), nseg, n);
  L2S_LAUNCH(rle_count_kernel, grid, dim3(256), 0, s, masks, h, w, nseg, ws, stride, n_valid);
  L2S_LAUNCH(rle_scan_batch_kernel, dim3(1), dim3(RLE_SCAN_T), 0, s, n, n_valid, nch, h * w, ws, stride, pool, pool_words, cursor, spans);
  L2S_LAUNCH(rle_write_kernel, grid, dim3(256), 0, s, h, w, nseg, (const uint32_t*)ws, stride, n_valid, pool);
  return l2s_check_launch();
}

extern "C" int l2s_rle_to_string(const uint32_t* cnts, int n, char* out, int max_chars) {
  if (!cnts || !out || n < 0) return -1;
  int p = 0;
  for (int i = 0; i < n; ++i) {
    long x = (long)cnts[i];
    if (i > 2) x -= (long)cnts[i - 2];
    int more = 1;
    while (more) {
      char c = (char)(x & 0x1f);
      x >>= 5;
      more = (c & 0x10) ? x != -1 : x != 0;
      if (more) c |= 0x20;
      if (p >= max_chars) return -1;
      out[p++] = (char)(c + 48);
    }
  }
  if (p >= max_chars) return -1;                          // room for the terminator
  out[p] = 0;
  return p;
}
