// Caption decoding decisions on the device (nets/decode.py): what AttModel.sample / CaptionModel.beam_search decide on the host between two
// steps of the captioner.  One workgroup per launch, like l2s_detect_select: a decision is a few thousand values, and what matters is that
// the next step's launches never wait for the host.
//   l2s_decode_pick            AttModel.py:172-201    argmax or inverse-CDF draw of one row, the finished flag, the next input token
//   l2s_decode_pick_rows       that argmax for every row of a batch of detections (one workgroup per row; the same two device functions, so
//                              a row decides what l2s_decode_pick decides on it), or the log-probability of a forced token
//   l2s_decode_force_rows      teacher forcing with a token row and a length per row: AttModel.forward + LanguageModelCriterion's gather
//                              and mask for a batch of different sentences, one step per launch
//   l2s_decode_beam_step       CaptionModel.py:27-121 beam_step + the completion loop for one t
//   l2s_decode_beam_step_rows  that step for every detection of a sentence (one workgroup per detection, the same device function)
//   l2s_decode_beam_finish_rows  CaptionModel.py:123 the final ordering of every detection's completed beams, on the device
//   l2s_mask_resize_nearest    a predicted canvas at the blob's size, by the rule of the loader's ground-truth masks
#include "common.h"
#include "../../include/lang2seg_hip.h"
#include "pil_resize.h"
#include "rows.h"
#include <climits>
#include <cmath>

namespace {

constexpr int DEC_T = 256;
constexpr int RS_ROWS = 8;

__device__ __forceinline__ uint64_t dec_mix64(uint64_t z) {  // splitmix64 finaliser (the dropout masks' and sampling keys' hash)
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// (value, index) with "greater value, then lower index" first; INT_MAX = nothing yet; a NaN is never a candidate
__device__ __forceinline__ bool dec_better(float ov, int ok, float bv, int bk) {
  return ok != INT_MAX && ov == ov && (bk == INT_MAX || ov > bv || (ov == bv && ok < bk));
}
__device__ __forceinline__ void wave_best(float& bv, int& bk) {
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int ok = __shfl_xor(bk, o);
    if (dec_better(ov, ok, bv, bk)) { bv = ov; bk = ok; }
  }
}

// ---------------------------------------------------------------- l2s_decode_pick, l2s_decode_pick_rows
// the log-softmax of one row x[V1] by a workgroup of DEC_T threads is (x[k] - m) - ls: the maximum and the log of the sum (red: 4 floats)
__device__ __forceinline__ void row_max_logsum(const float* x, int V1, float* red, float& m, float& ls) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  m = -INFINITY;
  for (int k = tid; k < V1; k += DEC_T) m = fmaxf(m, x[k]);
  m = block_max(m, red);
  float s = 0.f;
  for (int k = tid; k < V1; k += DEC_T) s += expf(x[k] - m);
  s = block_sum(s, red);
  ls = logf(s);
}
// a teacher-forced token as an index of that row (a token outside the table: clamped, never an address) and its log-probability: what
// l2s_decode_pick_rows' forced branch and l2s_decode_force_rows both write, so equal logits and tokens give equal bits
__device__ __forceinline__ int forced_index(int64_t f, int V1) { return f < 0 ? 0 : (f >= V1 ? V1 - 1 : (int)f); }
__device__ __forceinline__ float row_logprob(const float* x, int k, float m, float ls) {
#pragma clang fp contract(off)
  return (x[k] - m) - ls;
}
// the greedy pick of that workgroup: the best word of each thread, of each wave, then of the four waves in order (wv, wk: 4 each).  The
// result is the same in every thread; all NaN: no candidate, word 0
__device__ __forceinline__ int block_argmax(const float* x, int V1, float m, float ls, float* wv, int* wk) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  float bv = 0.f;
  int bk = INT_MAX;
  for (int k = tid; k < V1; k += DEC_T) {
    const float lp = (x[k] - m) - ls;
    if (dec_better(lp, k, bv, bk)) { bv = lp; bk = k; }
  }
  wave_best(bv, bk);
  if ((tid & 63) == 0) { wv[tid >> 6] = bv; wk[tid >> 6] = bk; }
  __syncthreads();
  for (int w = 0; w < DEC_T / 64; ++w)
    if (w == 0 || dec_better(wv[w], wk[w], bv, bk)) { bv = wv[w]; bk = wk[w]; }
  return bk == INT_MAX ? 0 : bk;
}

__global__ __launch_bounds__(DEC_T) void decode_pick_kernel(const float* logits, int V1, int t, int sample_max, float inv_temp, const float* u_in,
                                                            const uint64_t* seed_dev, uint64_t salt, int* finished, int64_t* seq,
                                                            float* seq_logprobs, int64_t* next_token) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  __shared__ float part[DEC_T];
  __shared__ float wv[4];
  __shared__ int wk[4];
  __shared__ int s_first, s_last;
  const int tid = threadIdx.x;
  float m, ls;
  row_max_logsum(logits, V1, red, m, ls);
  int pick = 0;
  if (sample_max) {
    pick = block_argmax(logits, V1, m, ls, wv, wk);
  } else {
    // every thread owns a run of consecutive words: cdf(k) = [sum of the runs before, left to right] + [running sum inside the run], the
    // same roundings wherever it is evaluated, so the cdf is monotone and its last value is `total`
    const int chunk = (V1 + DEC_T - 1) / DEC_T, k0 = tid * chunk, k1 = k0 + chunk < V1 ? k0 + chunk : V1;
    float loc = 0.f;
    for (int k = k0; k < k1; ++k) loc += expf(((logits[k] - m) - ls) * inv_temp);
    part[tid] = loc;
    if (tid == 0) { s_first = INT_MAX; s_last = 0; }
    __syncthreads();
    float before = 0.f, total = 0.f;
    for (int j = 0; j < DEC_T; ++j) {
      if (j == tid) before = total;
      total += part[j];
    }
    float u;
    if (u_in) {
      u = u_in[t];
    } else {
      const uint64_t seed = dec_mix64(*seed_dev * 0x9E3779B97F4A7C15ull + salt);
      u = (float)(uint32_t)(dec_mix64(seed * 0x100000001B3ull + (uint64_t)t) >> 40) * (1.f / 16777216.f);   // 24 bits: [0, 1 - 2^-24]
    }
    const float target = u * total;
    loc = 0.f;
    int first = INT_MAX, last = -1;
    for (int k = k0; k < k1; ++k) {
      const float p = expf(((logits[k] - m) - ls) * inv_temp);
      loc += p;
      if (p > 0.f) last = k;
      if (first == INT_MAX && before + loc > target) first = k;
    }
    if (first != INT_MAX) atomicMin(&s_first, first);
    if (last >= 0) atomicMax(&s_last, last);
    __syncthreads();
    pick = s_first != INT_MAX ? s_first : s_last;       // (u * total rounded up to total: the last word that has any mass)
  }
  if (tid == 0) {
    const int fin = t == 0 ? 0 : *finished;
    const int tok = fin ? 0 : pick;
    seq[t] = tok;
    seq_logprobs[t] = fin ? 0.f : (logits[pick] - m) - ls;
    *next_token = tok;
    *finished = fin | (tok == 0);
  }
}
// one workgroup per live row (rows.h): that greedy decision, or a forced token and its log-probability
__global__ __launch_bounds__(DEC_T) void decode_pick_rows_kernel(const float* logits, int ld, int V1, int row0, const int* __restrict__ count, int t, int T,
                                                                 const int64_t* forced, int* finished, int64_t* seq, float* logprobs,
                                                                 int64_t* next_token, float* sum) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  __shared__ float wv[4];
  __shared__ int wk[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (!row_live(r, row0, count)) return;
  const float* x = logits + (long)r * ld;
  float m, ls;
  row_max_logsum(x, V1, red, m, ls);
  int pick = 0;
  if (forced) {
    pick = forced_index(*forced, V1);
  } else {
    pick = block_argmax(x, V1, m, ls, wv, wk);
  }
  if (tid == 0) {
    // teacher forcing has no finished rows: the expression is scored to its end (AttModel.forward with the criterion's mask all ones)
    const int fin = (forced || t == 0) ? 0 : finished[r];
    const int tok = fin ? 0 : pick;
    seq[(long)r * T + t] = tok;
    const float lp = fin ? 0.f : row_logprob(x, pick, m, ls);
    logprobs[(long)r * T + t] = lp;
    if (sum) sum[r] = t == 0 ? lp : sum[r] + lp;           // the row's joint log-probability, added up left to right
    next_token[r] = tok;
    finished[r] = fin | (tok == 0);
  }
}
// one workgroup per live row: teacher forcing with the row's own token and length.  Step t of a row with t < lengths[r] scores
// targets[r][t]; behind its length a row writes nothing but a valid next input
__global__ __launch_bounds__(DEC_T) void decode_force_rows_kernel(const float* logits, int ld, int V1, int row0, const int* __restrict__ count, int t, int T,
                                                                  const int64_t* __restrict__ targets, const int* __restrict__ lengths, float* logprobs,
                                                                  int64_t* next_token, float* sum) {
#pragma clang fp contract(off)
  __shared__ float red[4];
  const int r = blockIdx.x, tid = threadIdx.x;
  if (!row_live(r, row0, count)) return;
  if (t >= lengths[r]) {                                   // (the same in every thread of the workgroup)
    if (tid == 0) next_token[r] = 0;
    return;
  }
  const float* x = logits + (long)r * ld;
  float m, ls;
  row_max_logsum(x, V1, red, m, ls);
  if (tid == 0) {
    const int pick = forced_index(targets[(long)r * T + t], V1);
    const float lp = row_logprob(x, pick, m, ls);
    logprobs[(long)r * T + t] = lp;
    if (sum) sum[r] = t == 0 ? lp : sum[r] + lp;           // the row's joint log-probability, added up left to right
    next_token[r] = pick;
  }
}

// ---------------------------------------------------------------- l2s_decode_beam_step, l2s_decode_beam_step_rows
// one caption's step by a workgroup of DEC_T threads on that caption's slices: the body of both kernels, so a detection of the rows entry
// decides what the single entry decides on the same logits and tables
__device__ __forceinline__ void decode_beam_step_body(const l2s_beam_step_args& a) {
#pragma clang fp contract(off)
  __shared__ float ys[L2S_BEAM_MAX][L2S_BEAM_MAX];
  __shared__ int ix[L2S_BEAM_MAX][L2S_BEAM_MAX];
  __shared__ float cp[L2S_BEAM_MAX * L2S_BEAM_MAX];
  __shared__ int win[L2S_BEAM_MAX], slot_of[L2S_BEAM_MAX];
  __shared__ float psum[L2S_BEAM_MAX];
  __shared__ int pseq[L2S_BEAM_MAX_T * L2S_BEAM_MAX];
  __shared__ float plog[L2S_BEAM_MAX_T * L2S_BEAM_MAX];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int B = a.B, V1 = a.V1, t = a.t, T = a.T;
  const int rows = t == 0 ? 1 : B, cols = B < V1 ? B : V1;
  // the previous tables (CaptionModel.py:56-59)
  for (int e = tid; e < t * B; e += DEC_T) { pseq[e] = a.beam_seq[e]; plog[e] = a.beam_seq_logprobs[e]; }
  if (tid < L2S_BEAM_MAX) {
    psum[tid] = (t > 0 && tid < B) ? a.beam_logprobs_sum[tid] : 0.f;
    win[tid] = 0;
  }
  // a wave per row: log-softmax, then the `cols` best words one after the other, each the best of what comes after the one before it
  for (int q = w; q < rows; q += DEC_T / 64) {
    const float* x = a.logits + (long)q * a.ld_logits;
    float m = -INFINITY;
    for (int k = lane; k < V1; k += 64) m = fmaxf(m, x[k]);
    m = wave_max(m);
    float s = 0.f;
    for (int k = lane; k < V1; k += 64) s += expf(x[k] - m);
    s = wave_sum(s);
    const float ls = logf(s);
    float pv = 0.f;
    int pk = -1;                                          // -1: nothing picked yet, everything comes "after" it
    for (int c = 0; c < cols; ++c) {
      float bv = 0.f;
      int bk = INT_MAX;
      if (pk != INT_MAX) {
        for (int k = lane; k < V1; k += 64) {
          float v = (x[k] - m) - ls;
          if (k == V1 - 1) v = v - 1000.f;                  // :93
          const bool after = pk < 0 ? (v == v) : (v < pv || (v == pv && k > pk));
          if (after && dec_better(v, k, bv, bk)) { bv = v; bk = k; }
        }
        wave_best(bv, bk);
      }
      pv = bv; pk = bk;
      if (lane == 0) {
        ys[q][c] = bk == INT_MAX ? -INFINITY : bv;          // (NaN logits: fewer than `cols` candidates)
        ix[q][c] = bk == INT_MAX ? 0 : bk;
      }
    }
  }
  __syncthreads();
  // candidates, column-major then row (:46-51); rank = the position in the stable descending order by p (:52)
  const int n = cols * rows;
  float p = 0.f;
  if (tid < n) {
    const int c = tid / rows, q = tid % rows;
    p = psum[q] + ys[q][c];
    if (!(p == p)) p = -INFINITY;                           // a NaN sum ranks last: every p is ordered, so the ranks are a permutation
    cp[tid] = p;
  }
  __syncthreads();
  if (tid < n) {
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float pj = cp[j];
      rank += (pj > p || (pj == p && j < tid)) ? 1 : 0;
    }
    if (rank < B) win[rank] = tid;
  }
  __syncthreads();
  if (tid == 0) {
    int cnt = t == 0 ? 0 : *a.done_count;
    for (int v = 0; v < B; ++v) {
      const int i = win[v], tok = ix[i % rows][i / rows];
      slot_of[v] = (tok == 0 || t == T - 1) ? cnt++ : -1;   // :109
    }
    *a.done_count = cnt;
  }
  __syncthreads();
  // fork the histories (:60-73)
  for (int e = tid; e < t * B; e += DEC_T) {
    const int srow = e / B, v = e % B, q = win[v] % rows;
    a.beam_seq[e] = pseq[srow * B + q];
    a.beam_seq_logprobs[e] = plog[srow * B + q];
  }
  if (tid < B) {
    const int i = win[tid], c = i / rows, q = i % rows;
    a.beam_seq[t * B + tid] = ix[q][c];
    a.beam_seq_logprobs[t * B + tid] = ys[q][c];
    a.beam_logprobs_sum[tid] = slot_of[tid] >= 0 ? -1000.f : cp[i];     // :73, :117
    a.next_tokens[tid] = ix[q][c];
    a.parents[tid] = q;
  }
  // completed beams (:110-115): the whole column, zeros behind t
  const int RW = L2S_BEAM_RECORD_WORDS(T);
  for (int e = tid; e < B * T; e += DEC_T) {
    const int v = e / T, srow = e % T, slot = slot_of[v];
    if (slot < 0 || slot >= B * T) continue;
    const int i = win[v], c = i / rows, q = i % rows;
    int* rec = a.done + (long)slot * RW;
    rec[srow] = srow < t ? pseq[srow * B + q] : (srow == t ? ix[q][c] : 0);
    rec[T + srow] = __float_as_int(srow < t ? plog[srow * B + q] : (srow == t ? ys[q][c] : 0.f));
    if (srow == 0) { rec[2 * T] = __float_as_int(cp[i]); rec[2 * T + 1] = slot; }
  }
  // the recurrent state rows by parent (:67-69)
  for (int j = 0; j < a.n_state; ++j) {
    const float* src = a.state_in[j];
    float* dst = a.state_out[j];
    const int li = a.ld_in[j], lo = a.ld_out[j];
    for (int e = tid; e < B * a.R; e += DEC_T) {
      const int v = e / a.R, r = e % a.R;
      dst[(long)v * lo + r] = src[(long)(win[v] % rows) * li + r];
    }
  }
}
__global__ __launch_bounds__(DEC_T) void decode_beam_step_kernel(l2s_beam_step_args a) { decode_beam_step_body(a); }
// one workgroup per detection (rows.h): detection d owns B consecutive rows of the logits and of every state array, and its own tables
__global__ __launch_bounds__(DEC_T) void decode_beam_step_rows_kernel(l2s_beam_step_args a, int row0, const int* __restrict__ count) {
  const int d = blockIdx.x;
  if (!row_live(d, row0, count)) return;
  const long B = a.B, T = a.T;
  a.logits += d * B * a.ld_logits;
  a.beam_seq += d * T * B;
  a.beam_seq_logprobs += d * T * B;
  a.beam_logprobs_sum += d * B;
  a.next_tokens += d * B;
  a.parents += d * B;
  a.done += d * B * T * L2S_BEAM_RECORD_WORDS(T);
  a.done_count += d;
  for (int j = 0; j < 4; ++j) {
    if (j >= a.n_state) break;
    a.state_in[j] += d * B * a.ld_in[j];
    a.state_out[j] += d * B * a.ld_out[j];
  }
  decode_beam_step_body(a);
}

// ---------------------------------------------------------------- l2s_decode_beam_finish_rows
// one workgroup per detection: its completed records ordered by p descending, equal p in completion order (CaptionModel.py:123; the rank by
// counting of the step kernel), the first B written out and the best one once more in the layout of l2s_decode_pick_rows' tables
__global__ __launch_bounds__(DEC_T) void decode_beam_finish_rows_kernel(const int* __restrict__ done, const int* __restrict__ done_count, int B, int T,
                                                                        int row0, const int* __restrict__ count, int64_t* beam_seq, float* beam_logps,
                                                                        float* beam_p, int* beam_n, int64_t* seq, float* logprobs) {
  __shared__ float ps[L2S_BEAM_MAX * L2S_BEAM_MAX_T];
  __shared__ int win[L2S_BEAM_MAX];
  __shared__ int s_first0;
  const int d = blockIdx.x, tid = threadIdx.x;
  if (!row_live(d, row0, count)) return;
  const int RW = L2S_BEAM_RECORD_WORDS(T);
  const int* recs = done + (long)d * B * T * RW;
  int n = done_count[d];
  n = n < 0 ? 0 : (n > B * T ? B * T : n);
  const int nb = n < B ? n : B;
  for (int i = tid; i < n; i += DEC_T) ps[i] = __int_as_float(recs[(long)i * RW + 2 * T]);
  __syncthreads();
  for (int i = tid; i < n; i += DEC_T) {
    const float p = ps[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float pj = ps[j];
      rank += (pj > p || (pj == p && j < i)) ? 1 : 0;
    }
    if (rank < B) win[rank] = i;
  }
  __syncthreads();
  if (tid == 0) {
    int f = T;
    if (nb > 0) {
      const int* rec = recs + (long)win[0] * RW;
      for (int s = T - 1; s >= 0; --s) f = rec[s] == 0 ? s : f;
    } else {
      f = 0;
    }
    s_first0 = f;
    beam_n[d] = nb;
  }
  __syncthreads();
  for (int e = tid; e < B * T; e += DEC_T) {
    const int v = e / T, s = e % T;
    const int* rec = v < nb ? recs + (long)win[v] * RW : nullptr;
    beam_seq[((long)d * B + v) * T + s] = rec ? rec[s] : 0;
    beam_logps[((long)d * B + v) * T + s] = rec ? __int_as_float(rec[T + s]) : 0.f;
    if (s == 0) beam_p[(long)d * B + v] = rec ? __int_as_float(rec[2 * T]) : 0.f;
  }
  for (int s = tid; s < T; s += DEC_T) {
    const int* rec = nb > 0 ? recs + (long)win[0] * RW : nullptr;
    seq[(long)d * T + s] = (rec && s < s_first0) ? rec[s] : 0;
    logprobs[(long)d * T + s] = (rec && s <= s_first0) ? __int_as_float(rec[T + s]) : 0.f;
  }
}

// ---------------------------------------------------------------- l2s_mask_resize_nearest
__global__ __launch_bounds__(256) void mask_resize_nearest_kernel(const uint8_t* src, int ih, int iw, uint8_t* dst, int H, int W) {
  __shared__ int ty[RS_ROWS];
  const int t = threadIdx.x, x = blockIdx.x * 256 + t, y0 = blockIdx.y * RS_ROWS;
  if (t < RS_ROWS) ty[t] = y0 + t < H ? pil_nearest_src(y0 + t, ih, H) : 0;
  __syncthreads();
  if (x >= W) return;
  const int tx = pil_nearest_src(x, iw, W);
  for (int i = 0; i < RS_ROWS && y0 + i < H; ++i) dst[(long)(y0 + i) * W + x] = src[(long)ty[i] * iw + tx];
}

}  // namespace

extern "C" int l2s_decode_pick(const float* logits, int V1, int t, int sample_max, float temperature, const float* u_in, const uint64_t* seed_dev,
                               uint64_t salt, int* finished, int64_t* seq, float* seq_logprobs, int64_t* next_token, hipStream_t s) {
  if (!logits || V1 < 1 || t < 0 || !finished || !seq || !seq_logprobs || !next_token || (!sample_max && !(temperature > 0.f)) ||
      (!sample_max && !u_in && !seed_dev))
    return L2S_EINVAL;
  L2S_LAUNCH(decode_pick_kernel, dim3(1), dim3(DEC_T), 0, s, logits, V1, t, sample_max, sample_max ? 1.f : 1.f / temperature, u_in, seed_dev, salt,
             finished, seq, seq_logprobs, next_token);
  return l2s_check_launch();
}
extern "C" int l2s_decode_pick_rows(const float* logits, int ld_logits, int V1, int rows, int row0, const int* count, int t, int T,
                                    const int64_t* forced, int* finished, int64_t* seq, float* logprobs, int64_t* next_token, float* sum,
                                    hipStream_t s) {
  if (!logits || V1 < 1 || ld_logits < V1 || rows < 1 || row0 < 0 || t < 0 || t >= T || !finished || !seq || !logprobs || !next_token) return L2S_EINVAL;
  L2S_LAUNCH(decode_pick_rows_kernel, dim3(rows), dim3(DEC_T), 0, s, logits, ld_logits, V1, row0, count, t, T, forced, finished, seq, logprobs,
             next_token, sum);
  return l2s_check_launch();
}
extern "C" int l2s_decode_force_rows(const float* logits, int ld_logits, int V1, int rows, int row0, const int* count, int t, int T,
                                     const int64_t* targets, const int* lengths, float* logprobs, int64_t* next_token, float* sum, hipStream_t s) {
  if (!logits || V1 < 1 || ld_logits < V1 || rows < 1 || row0 < 0 || t < 0 || t >= T || !targets || !lengths || !logprobs || !next_token) return L2S_EINVAL;
  L2S_LAUNCH(decode_force_rows_kernel, dim3(rows), dim3(DEC_T), 0, s, logits, ld_logits, V1, row0, count, t, T, targets, lengths, logprobs, next_token,
             sum);
  return l2s_check_launch();
}

static bool beam_args_ok(const l2s_beam_step_args* a) {
  if (!a || !a->logits || a->B < 1 || a->B > L2S_BEAM_MAX || a->V1 < a->B || a->ld_logits < a->V1 || a->T < 1 || a->T > L2S_BEAM_MAX_T || a->t < 0 ||
      a->t >= a->T || a->n_state < 0 || a->n_state > 4 || (a->n_state && a->R < 1) || !a->beam_seq || !a->beam_seq_logprobs ||
      !a->beam_logprobs_sum || !a->next_tokens || !a->parents || !a->done || !a->done_count)
    return false;
  for (int j = 0; j < a->n_state; ++j)
    if (!a->state_in[j] || !a->state_out[j] || a->ld_in[j] < a->R || a->ld_out[j] < a->R) return false;
  return true;
}
extern "C" int l2s_decode_beam_step(const l2s_beam_step_args* a, hipStream_t s) {
  if (!beam_args_ok(a)) return L2S_EINVAL;
  const l2s_beam_step_args args = *a;
  L2S_LAUNCH(decode_beam_step_kernel, dim3(1), dim3(DEC_T), 0, s, args);
  return l2s_check_launch();
}
extern "C" int l2s_decode_beam_step_rows(const l2s_beam_step_args* a, int rows, int row0, const int* count, hipStream_t s) {
  if (!beam_args_ok(a) || rows < 1 || row0 < 0) return L2S_EINVAL;
  const l2s_beam_step_args args = *a;
  L2S_LAUNCH(decode_beam_step_rows_kernel, dim3(rows), dim3(DEC_T), 0, s, args, row0, count);
  return l2s_check_launch();
}
extern "C" int l2s_decode_beam_finish_rows(const int* done, const int* done_count, int B, int T, int rows, int row0, const int* count,
                                           int64_t* beam_seq, float* beam_logps, float* beam_p, int* beam_n, int64_t* seq, float* logprobs,
                                           hipStream_t s) {
  if (!done || !done_count || B < 1 || B > L2S_BEAM_MAX || T < 1 || T > L2S_BEAM_MAX_T || rows < 1 || row0 < 0 || !beam_seq || !beam_logps ||
      !beam_p || !beam_n || !seq || !logprobs)
    return L2S_EINVAL;
  L2S_LAUNCH(decode_beam_finish_rows_kernel, dim3(rows), dim3(DEC_T), 0, s, done, done_count, B, T, row0, count, beam_seq, beam_logps, beam_p,
             beam_n, seq, logprobs);
  return l2s_check_launch();
}

extern "C" int l2s_mask_resize_nearest(const uint8_t* src, int ih, int iw, uint8_t* dst, int H, int W, hipStream_t s) {
  if (!src || !dst || ih < 1 || iw < 1 || H < 1 || W < 1) return L2S_EINVAL;
  L2S_LAUNCH(mask_resize_nearest_kernel, dim3(cdiv(W, 256), cdiv(H, RS_ROWS)), dim3(256), 0, s, src, ih, iw, dst, H, W);
  return l2s_check_launch();
}
