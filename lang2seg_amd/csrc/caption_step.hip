// Per-token kernels of the two captioners, forward + backward, fp32, wave64, gfx950:
//   att2in2 (lib/caption_models/AttModel.py:406-423 attention, 446-466 core): the attention halves, the gate block alone and fused with
//     the a2c GEMV / with the projected attention, the GEMVs of the recurrence, the attention backward per token and summed over tokens;
//   top-down (AttModel.py:370-395: an attention nn.LSTMCell feeding a language nn.LSTMCell): the two cell steps, the centred attention
//     backward and a row packer.  The softmax + weighted sum (cap_att_apply_kernel) and the attention dots serve both.
// The recurrences are GEMV-shaped (M = 1): weights are streamed once per launch, one wave per output row or hidden unit, wave-level DPP
// reductions in a fixed order, no atomics; latency-bound links of the caption branch's dependent chain, the train step's critical path.
// The gate block, the LSTM cell and the softmax pieces are recur.h's; cap_recur.hip runs the att2in2 recurrence as one resident launch.
// The attention dots, the softmax + weighted sum and the softmax + gates also run on rows, one row per detection (l2s_cap_att_dots_rows,
// l2s_cap_att_apply_rows, l2s_cap_apply_gates_rows for --describe / --expr_score): the same body instantiated with a row index, so a row
// has the bits the single-row kernel gives it.  The *_groups entries (beam search on rows, nets/caption_rows.py) are the rows bodies with a
// divisor: state row r belongs to detection r / group, reads that detection's patt / P / att and is live iff the detection is.
#include "common.h"
#include "../../include/lang2seg_hip.h"
#include "recur.h"
#include "rows.h"

namespace {

// ---------------------------------------------------------------- att2in2 attention (L <= 256)
// forward: (A) one wave per location: dots[l] = alpha . tanh(patt[l] + att_h) ; (B) D/64 workgroups: softmax over L (recomputed per
// workgroup, 196 values) and att_res[d] = sum_l w[l] att[l][d] with 4 l-groups per 64 channels.  (B)'s feature width D is independent of
// att_hid_size: it is the top-down captioner's second attention half too (l2s_cap_att_apply_fwd).
//
// Each forward body is written once, for ROWS (nets/caption_rows.py: row r = blockIdx.y of patt [rows][L][D], att_h [rows][ld_att_h], dots
// [rows][256], att [rows][L][D], att_res [rows][ld_res]; dead rows return, rows.h) and for the single row of training and decoding, where
// r is the constant 0 and the liveness test and the row strides fold away.  TRAIN is what only that single row has: the wave priority of
// a link of the train step's critical path, and the stores that backward reads (tanh_ws, weight, save).
template <bool ROWS, bool TRAIN>
__device__ __forceinline__ void cap_att_dots(const float* patt, const float* att_h, int ld_att_h, const float* aw,
                                             const float* ab, int row0, const int* count, int group, int L, int D, float* tanh_ws,
                                             float* dots) {
  if (TRAIN) __builtin_amdgcn_s_setprio(3);   // a link of the caption branch's dependent chain (the step's critical path): issue ahead of co-resident GEMM waves
  const int r = ROWS ? blockIdx.y : 0, l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int dr = ROWS ? r / group : 0;
  if (l >= L || (ROWS && !row_live(dr, row0, count))) return;
  patt += (long)dr * L * D;
  att_h += (long)r * ld_att_h;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) {
    const float t = tanhf(patt[(long)l * D + d] + att_h[d]);
    if (TRAIN) tanh_ws[(long)l * D + d] = t;
    s = fmaf(t, aw[d], s);
  }
  s = wave_sum(s);
  if (lane == 0) dots[(long)r * 256 + l] = s + ab[0];
}
template <bool ROWS, bool TRAIN>
__device__ __forceinline__ void cap_att_apply(const float* att, const float* dots, int row0, const int* count, int group, int L,
                                              int D, float* weight, float* att_res, int ld_res) {
  if (TRAIN) __builtin_amdgcn_s_setprio(3);
  __shared__ float w[256];
  __shared__ float red[4];
  __shared__ float part[4][64];
  const int r = ROWS ? blockIdx.y : 0, tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const int dr = ROWS ? r / group : 0;
  if (ROWS && !row_live(dr, row0, count)) return;
  const float wt = block_softmax(dots + (long)r * 256, L, red);
  if (tid < L) { w[tid] = wt; if (TRAIN && blockIdx.x == 0) weight[tid] = wt; }
  __syncthreads();
  const int d = blockIdx.x * 64 + lane;
  att += (long)dr * L * D;
  float s = 0.f;
  if (d < D) for (int l = g; l < L; l += 4) s = fmaf(w[l], att[(long)l * D + d], s);
  part[g][lane] = s;
  __syncthreads();
  if (g == 0 && d < D) att_res[(long)r * ld_res + d] = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
}
__global__ __launch_bounds__(256) void cap_att_dots_kernel(const float* __restrict__ patt, const float* __restrict__ att_h, const float* __restrict__ aw,
                                                          const float* __restrict__ ab, int L, int D, float* tanh_ws, float* dots) {
  cap_att_dots<false, true>(patt, att_h, 0, aw, ab, 0, nullptr, 1, L, D, tanh_ws, dots);
}
__global__ __launch_bounds__(256) void cap_att_dots_rows_kernel(const float* __restrict__ patt, const float* __restrict__ att_h, int ld_att_h,
                                                               const float* __restrict__ aw, const float* __restrict__ ab, int row0,
                                                               const int* __restrict__ count, int L, int D, float* dots) {
  cap_att_dots<true, false>(patt, att_h, ld_att_h, aw, ab, row0, count, 1, L, D, nullptr, dots);
}
__global__ __launch_bounds__(256) void cap_att_dots_groups_kernel(const float* __restrict__ patt, const float* __restrict__ att_h, int ld_att_h,
                                                                 const float* __restrict__ aw, const float* __restrict__ ab, int row0,
                                                                 const int* __restrict__ count, int group, int L, int D, float* dots) {
  cap_att_dots<true, false>(patt, att_h, ld_att_h, aw, ab, row0, count, group, L, D, nullptr, dots);
}
__global__ __launch_bounds__(256) void cap_att_apply_kernel(const float* __restrict__ att, const float* __restrict__ dots, int L, int D, float* weight, float* att_res) {
  cap_att_apply<false, true>(att, dots, 0, nullptr, 1, L, D, weight, att_res, 0);
}
__global__ __launch_bounds__(256) void cap_att_apply_rows_kernel(const float* __restrict__ att, const float* __restrict__ dots, float* att_res, int ld_res,
                                                                int row0, const int* __restrict__ count, int L, int D) {
  cap_att_apply<true, false>(att, dots, row0, count, 1, L, D, nullptr, att_res, ld_res);
}
__global__ __launch_bounds__(256) void cap_att_apply_groups_kernel(const float* __restrict__ att, const float* __restrict__ dots, float* att_res, int ld_res,
                                                                  int row0, const int* __restrict__ count, int group, int L, int D) {
  cap_att_apply<true, false>(att, dots, row0, count, group, L, D, nullptr, att_res, ld_res);
}
// backward: (A) dweight[l] = dres . att[l] (one wave per l); (B) D/64 workgroups: softmax backward over L (recomputed), then the
// per-channel accumulations with 4 l-groups per 64 channels.
__global__ __launch_bounds__(256) void cap_att_bwd_dw_kernel(const float* __restrict__ dres, const float* __restrict__ att, int L, int D, float* dweight) {
  const int l = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (l >= L) return;
  float s = 0.f;
  for (int d = lane; d < D; d += 64) s = fmaf(dres[d], att[(long)l * D + d], s);
  s = wave_sum(s);
  if (lane == 0) dweight[l] = s;
}
__global__ __launch_bounds__(256) void cap_att_bwd_kernel(const float* __restrict__ dres, const float* __restrict__ dweight, const float* __restrict__ tanh_ws,
                                                         const float* __restrict__ weight, const float* __restrict__ aw, int L, int D,
                                                         float* dpatt, float* datt, float* datt_h, float* daw, float* dab) {
  __shared__ float ddot[256];
  __shared__ float wsh[256];
  __shared__ float red[4];
  __shared__ float p1[4][64], p2[4][64];
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const float wl = tid < L ? weight[tid] : 0.f;
  const float dwl = tid < L ? dweight[tid] : 0.f;
  const float dot = block_sum(wl * dwl, red);
  const float dd = wl * (dwl - dot);                      // softmax backward
  if (tid < 256) { ddot[tid] = tid < L ? dd : 0.f; wsh[tid] = wl; }
  const float sdd = block_sum(tid < L ? dd : 0.f, red);
  if (blockIdx.x == 0 && tid == 0) dab[0] += sdd;
  __syncthreads();
  const int d = blockIdx.x * 64 + lane;
  float sah = 0.f, saw = 0.f;
  if (d < D) {
    const float a = aw[d], dr = dres[d];
    for (int l = g; l < L; l += 4) {
      const float t = tanh_ws[(long)l * D + d];
      const float dt_ = ddot[l] * a * (1.f - t * t);
      dpatt[(long)l * D + d] += dt_;
      datt[(long)l * D + d] += wsh[l] * dr;
      sah += dt_;
      saw = fmaf(ddot[l], t, saw);
    }
  }
  p1[g][lane] = sah; p2[g][lane] = saw;
  __syncthreads();
  if (g == 0 && d < D) {
    datt_h[d] = p1[0][lane] + p1[1][lane] + p1[2][lane] + p1[3][lane];
    daw[d] += p2[0][lane] + p2[1][lane] + p2[2][lane] + p2[3][lane];
  }
}

__global__ void cap_gates_fwd_kernel(const float* s, const float* a2c, const float* c_prev, float* c, float* h, float* save, int R) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= R) return;
  float sj[5], sv[6];
  ld_rows<5>(sj, s, R, j);
  att2in_gates_fwd(sj, a2c[j], a2c[R + j], c_prev[j], c[j], h[j], sv);
  st_rows<6>(save, R, j, sv);
}
__global__ void cap_gates_bwd_kernel(const float* dh_a, const float* dh_b, const float* dc_in, const float* save, const float* c_prev, float* ds, float* da2c,
                                     float* dc_prev, int R) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= R) return;
  float sv[6], dsj[3], d0, d1;
  ld_rows<6>(sv, save, R, j);
  att2in_gates_bwd(sv, dh_a[j] + (dh_b ? dh_b[j] : 0.f), dc_in ? dc_in[j] : 0.f, c_prev[j], dsj, d0, d1, dc_prev[j]);
  st_rows<3>(ds, R, j, dsj);
  ds[3 * R + j] = d0; ds[4 * R + j] = d1;
  da2c[j] = d0; da2c[R + j] = d1;
}

// ---- fused per-step kernels of the att2in2 recurrence (one launch each; the recurrence is a chain of dependent launches,
// so every launch removed is a few microseconds off the caption branch's critical path) ----

// two GEMVs over the same input: y1 = w1 x + b1 (blocks [0, nb1)),  y2 (+)= w2 x + b2 (the rest).  One wave per output.
__global__ __launch_bounds__(256) void linear2_fwd_kernel(const float* __restrict__ x, int K, const float* __restrict__ w1, const float* __restrict__ b1,
                                                         float* y1, int N1, int acc1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                         float* y2, int N2, int acc2, int nb1) {
  __builtin_amdgcn_s_setprio(3);   // a link of the caption branch's dependent chain (the step's critical path): issue ahead of co-resident GEMM waves
  const bool second = (int)blockIdx.x >= nb1;
  const int n = ((int)blockIdx.x - (second ? nb1 : 0)) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int N = second ? N2 : N1;
  if (n >= N) return;
  const float* wr = (second ? w2 : w1) + (long)n * K;
  float acc = 0.f;
  for (int k = lane * 4; k < K; k += 256) {
    const float4 wv = *(const float4*)(wr + k), xv = *(const float4*)(x + k);
    acc = dot4(wv, xv, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    const float* b = second ? b2 : b1;
    float* o = (second ? y2 : y1) + n;
    float v = acc + (b ? b[n] : 0.f);
    if (second ? acc2 : acc1) v += *o;
    *o = v;
  }
}
// y[n] (+)= w1[n] . x1 + w2[n] . x2   (two inputs, one output vector; one wave per n)
__global__ __launch_bounds__(256) void linear_sum2_kernel(const float* __restrict__ x1, const float* __restrict__ w1, int K1, const float* __restrict__ x2,
                                                         const float* __restrict__ w2, int K2, float* y, int N, int accumulate) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  float a1 = 0.f, a2 = 0.f;
  const float* r1 = w1 + (long)n * K1; const float* r2 = w2 + (long)n * K2;
  for (int k = lane * 4; k < K1; k += 256) {
    const float4 wv = *(const float4*)(r1 + k), xv = *(const float4*)(x1 + k);
    a1 = dot4(wv, xv, a1);
  }
  for (int k = lane * 4; k < K2; k += 256) {
    const float4 wv = *(const float4*)(r2 + k), xv = *(const float4*)(x2 + k);
    a2 = dot4(wv, xv, a2);
  }
  a1 = wave_sum(a1); a2 = wave_sum(a2);
  if (lane == 0) { float v = a1 + a2; if (accumulate) v += y[n]; y[n] = v; }
}
// the same with the four waves of a workgroup splitting the K range of ONE output (four times the workgroups, a quarter of the
// dependent loads per wave): the launch sits on the caption branch's backward chain once per token
__global__ __launch_bounds__(256) void linear_sum2_split_kernel(const float* __restrict__ x1, const float* __restrict__ w1, int K1, const float* __restrict__ x2,
                                                               const float* __restrict__ w2, int K2, float* y, int N, int accumulate) {
  __builtin_amdgcn_s_setprio(3);   // a link of the caption branch's dependent chain (the step's critical path): issue ahead of co-resident GEMM waves
  __shared__ float part[4];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* r1 = w1 + (long)n * K1; const float* r2 = w2 + (long)n * K2;
  const int q1 = ((K1 / 4 + 3) / 4) * 4, q2 = ((K2 / 4 + 3) / 4) * 4;       // per-wave K ranges, multiples of 4
  float a = 0.f;
  for (int k = wv * q1 + lane * 4; k < min(K1, (wv + 1) * q1); k += 256) {
    const float4 wv4 = *(const float4*)(r1 + k), xv = *(const float4*)(x1 + k);
    a = dot4(wv4, xv, a);
  }
  for (int k = wv * q2 + lane * 4; k < min(K2, (wv + 1) * q2); k += 256) {
    const float4 wv4 = *(const float4*)(r2 + k), xv = *(const float4*)(x2 + k);
    a = dot4(wv4, xv, a);
  }
  a = wave_sum(a);
  if (lane == 0) part[wv] = a;
  __syncthreads();
  if (threadIdx.x == 0) { float v = ((part[0] + part[1]) + part[2]) + part[3]; if (accumulate) v += y[n]; y[n] = v; }
}
// a2c Linear (rows j and R + j) fused with the gate nonlinearity of unit j (ATT:449-462): one wave per unit
__global__ __launch_bounds__(256) void cap_a2c_gates_kernel(const float* __restrict__ ares, const float* __restrict__ w, const float* __restrict__ b, int K,
                                                           const float* __restrict__ s, const float* __restrict__ c_prev, float* c, float* h,
                                                           float* save, int R) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= R) return;
  const float* r0 = w + (long)j * K; const float* r1 = w + (long)(R + j) * K;
  float a0 = 0.f, a1 = 0.f;
  for (int k = lane * 4; k < K; k += 256) {
    const float4 xv = *(const float4*)(ares + k), w0 = *(const float4*)(r0 + k), w1 = *(const float4*)(r1 + k);
    a0 = dot4(w0, xv, a0);
    a1 = dot4(w1, xv, a1);
  }
  a0 = wave_sum(a0); a1 = wave_sum(a1);
  if (lane == 0) {
    a0 += b[j]; a1 += b[R + j];
    float sj[5], sv[6];
    ld_rows<5>(sj, s, R, j);
    att2in_gates_fwd(sj, a0, a1, c_prev[j], c[j], h[j], sv);
    st_rows<6>(save, R, j, sv);
  }
}
// datt_h[d] = sum_l ddot[l] aw[d] (1 - tanh^2[l][d]) for the 16 channels of a 1024-thread workgroup: 16 channels x 64 location groups, the
// groups added in order through part (the tail of the two att2in2 attention-backward step kernels; ddot: LDS, 0 beyond L)
__device__ __forceinline__ void att_h_grad(const float* ddot, const float* __restrict__ tanh_ws, const float* __restrict__ aw, int L, int D,
                                           float (*part)[17], float* datt_h) {
  const int dl = threadIdx.x & 15, lg = threadIdx.x >> 4;
  const int d = blockIdx.x * 16 + dl;
  float sah = 0.f;
  if (d < D) {
    const float a = aw[d];
    for (int l = lg; l < L; l += 64) {
      const float t = tanh_ws[(long)l * D + d];
      sah = fmaf(ddot[l] * a, 1.f - t * t, sah);
    }
  }
  part[lg][dl] = sah;
  __syncthreads();
  if (lg == 0 && d < D) {
    float v = 0.f;
    for (int g = 0; g < 64; ++g) v += part[g][dl];
    datt_h[d] = v;
  }
}
// attention backward, the part the recurrence needs at step t: ddot[l] (softmax backward of dweight[l] = dres . att[l],
// recomputed by every workgroup) and datt_h[d] = sum_l ddot[l] aw[d] (1 - tanh^2).  Workgroup = 16 channels x 16 l-groups.
__global__ __launch_bounds__(1024) void cap_att_bwd_step_kernel(const float* __restrict__ dres, const float* __restrict__ att, const float* __restrict__ tanh_ws,
                                                               const float* __restrict__ weight, const float* __restrict__ aw, int L, int D,
                                                               float* ddot_out, float* datt_h) {
  __shared__ float dwl[256];
  __shared__ float ddot[256];
  __shared__ float red[16];
  __shared__ float part[64][17];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // dweight[l] = dres . att[l]: 16 waves x (L / 16) rows, ONE row per trip.  (Round 2: the two-rows-per-trip form -- two interleaved
  // shuffle reductions whose results lane 0 stored with two LDS writes -- sporadically produced a wrong SECOND sum when other kernels
  // shared the CU: the compiler consumes the last ds_bpermute of the second chain after `s_waitcnt lgkmcnt(1)` with the first
  // ds_write already issued, i.e. it relies on a DS permute and a younger DS write retiring in order.  Found by the bit-reproducibility
  // test; tools/scan_lgkm_order.py looks for the pattern in the generated ISA.)
  for (int l = wv; l < L; l += 16) {
    float s0 = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
      const float4 r = *(const float4*)(dres + d);
      const float4 a = *(const float4*)(att + (long)l * D + d);
      s0 = dot4(a, r, s0);
    }
    s0 = wave_sum(s0);
    if (lane == 0) dwl[l] = s0;
  }
  __syncthreads();
  block_softmax_bwd(tid < L ? weight[tid] : 0.f, tid < L ? dwl[tid] : 0.f, L, ddot, red, ddot_out);
  att_h_grad(ddot, tanh_ws, aw, L, D, part, datt_h);
}
// ---------------------------------------------------------------------------------------------------------------------------------
// Projected-attention form of the att2in2 step (round 2).  a2c(att_res) = W (sum_l w_l att_l) + b = sum_l w_l (W att_l) + b because the
// softmax weights sum to one: with P = att . W_a2c^T computed once per sentence ([L][2R], one MFMA GEMM), the per-token chain
//     h2h/h2att GEMVs -> attention dots -> softmax + weighted sum of att -> a2c GEMV + gates          (4 launches, 2 MB of W_a2c per token)
// becomes
//     h2h/h2att GEMVs -> attention dots -> softmax + weighted sum of P's columns + gates               (3 launches),
// and backward  gates -> W_a2c^T GEMV -> attention step -> W_h2h^T / W_h2att^T GEMVs  becomes
//     gates + d(weight)_l = P_l . d(a2c)  ->  attention step  ->  GEMVs                                 (3 launches).
// The step-summed d(P) = sum_t w_t (x) d(a2c)_t is one small GEMM after the loop; d(att) and d(W_a2c) follow from it as two more.
// The caption branch is the train step's critical path, and each dependent launch on it costs ~10 us.
//
// forward: workgroup = 16 units x 16 location groups; softmax over the L dots recomputed per workgroup (L <= 256).  ROWS / TRAIN as above:
// row r of P [rows][L][2R], s [rows][ld_s], c_prev / c / h [rows][R]
template <bool ROWS, bool TRAIN>
__device__ __forceinline__ void cap_apply_gates(const float* P, const float* dots, const float* b,
                                                const float* s, int ld_s, const float* c_prev, float* c, float* h,
                                                float* save, float* weight, int row0, const int* count, int group, int L, int R) {
  if (TRAIN) __builtin_amdgcn_s_setprio(3);
  __shared__ float w[256];
  __shared__ float red[4];
  __shared__ float p0[16][17], p1[16][17];
  const int r = ROWS ? blockIdx.y : 0, tid = threadIdx.x, dl = tid & 15, lg = tid >> 4;
  const int dr = ROWS ? r / group : 0;
  if (ROWS && !row_live(dr, row0, count)) return;
  const float wt = block_softmax(dots + (long)r * 256, L, red);
  w[tid] = tid < L ? wt : 0.f;
  if (TRAIN && blockIdx.x == 0 && tid < L) weight[tid] = wt;
  __syncthreads();
  const int j = blockIdx.x * 16 + dl;
  float a0 = 0.f, a1 = 0.f;
  if (j < R) {
    const float* q = P + (long)dr * L * 2 * R + j;
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
    const long o = (long)r * R + j;
    att2in_gates_fwd(sj, a0, a1, c_prev[o], c[o], h[o], sv);
    if (TRAIN) st_rows<6>(save, R, j, sv);
  }
}
__global__ __launch_bounds__(256) void cap_apply_gates_kernel(const float* __restrict__ P, const float* __restrict__ dots, const float* __restrict__ b,
                                                             const float* __restrict__ s, const float* __restrict__ c_prev, float* c, float* h,
                                                             float* save, float* weight, int L, int R) {
  cap_apply_gates<false, true>(P, dots, b, s, 0, c_prev, c, h, save, weight, 0, nullptr, 1, L, R);
}
__global__ __launch_bounds__(256) void cap_apply_gates_rows_kernel(const float* __restrict__ P, const float* __restrict__ dots, const float* __restrict__ b,
                                                                  const float* __restrict__ s, int ld_s, const float* __restrict__ c_prev, float* c,
                                                                  float* h, int row0, const int* __restrict__ count, int L, int R) {
  cap_apply_gates<true, false>(P, dots, b, s, ld_s, c_prev, c, h, nullptr, nullptr, row0, count, 1, L, R);
}
__global__ __launch_bounds__(256) void cap_apply_gates_groups_kernel(const float* __restrict__ P, const float* __restrict__ dots, const float* __restrict__ b,
                                                                    const float* __restrict__ s, int ld_s, const float* __restrict__ c_prev, float* c,
                                                                    float* h, int row0, const int* __restrict__ count, int group, int L, int R) {
  cap_apply_gates<true, false>(P, dots, b, s, ld_s, c_prev, c, h, nullptr, nullptr, row0, count, group, L, R);
}
// backward (1): the gate backward of cap_gates_bwd_kernel recomputed by every workgroup into LDS (2R values; workgroup 0 also stores
// dsums / da2c / dc_prev), then one wave per location: dweight[l] = P[l] . da2c.   R <= 1024.
__global__ __launch_bounds__(256) void cap_gates_bwd_dw_kernel(const float* __restrict__ dh_a, const float* __restrict__ dh_b, const float* __restrict__ dc_in,
                                                              const float* __restrict__ save, const float* __restrict__ c_prev, const float* __restrict__ P,
                                                              float* ds, float* da2c, float* dc_prev, float* dweight, int L, int R) {
  __builtin_amdgcn_s_setprio(3);   // a link of the caption branch's dependent chain (the step's critical path): issue ahead of co-resident GEMM waves
  __shared__ __attribute__((aligned(16))) float g[2048];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool out = blockIdx.x == 0;
  for (int j = tid; j < R; j += 256) {
    float sv[6], dsj[3], d0, d1, dcp;
    ld_rows<6>(sv, save, R, j);
    att2in_gates_bwd(sv, dh_a[j] + (dh_b ? dh_b[j] : 0.f), dc_in ? dc_in[j] : 0.f, c_prev[j], dsj, d0, d1, dcp);
    g[j] = d0; g[R + j] = d1;
    if (out) {
      st_rows<3>(ds, R, j, dsj);
      ds[3 * R + j] = d0; ds[4 * R + j] = d1;
      da2c[j] = d0; da2c[R + j] = d1;
      dc_prev[j] = dcp;
    }
  }
  __syncthreads();
  const int l = blockIdx.x * 4 + wv;
  if (l >= L) return;
  const float* q = P + (long)l * 2 * R;
  float a = 0.f;
  for (int n = lane * 4; n < 2 * R; n += 256) {
    const float4 pv = *(const float4*)(q + n), gv = *(const float4*)(g + n);
    a = dot4(pv, gv, a);
  }
  a = wave_sum(a);
  if (lane == 0) dweight[l] = a;
}
// backward (2): softmax backward of the L location weights (recomputed by every workgroup from dweight) and
// datt_h[d] = sum_l ddot[l] aw[d] (1 - tanh^2).  Workgroup = 16 channels x 64 location groups.
__global__ __launch_bounds__(1024) void cap_att_bwd_step2_kernel(const float* __restrict__ dweight, const float* __restrict__ tanh_ws, const float* __restrict__ weight,
                                                                const float* __restrict__ aw, int L, int D, float* ddot_out, float* datt_h) {
  __builtin_amdgcn_s_setprio(3);   // a link of the caption branch's dependent chain (the step's critical path): issue ahead of co-resident GEMM waves
  __shared__ float ddot[256];
  __shared__ float red[16];
  __shared__ float part[64][17];
  const int tid = threadIdx.x;
  block_softmax_bwd(tid < L ? weight[tid] : 0.f, tid < L ? dweight[tid] : 0.f, L, ddot, red, ddot_out);
  att_h_grad(ddot, tanh_ws, aw, L, D, part, datt_h);
}
// after the loop: everything the per-step kernel left out, summed over the S steps in one launch.  A workgroup owns 16 channels d
// (64 location lanes x 16 channels; round 3: 1024 threads instead of 256 - the launch sits on the caption branch's critical chain and each
// thread's (location, step) loop is a chain of dependent loads: 65-89 -> ~25 us): dpatt / datt rows are written per (l, d), the alpha_net
// weight gradient daw[d] is summed over all locations inside the workgroup in a fixed order (no atomics); workgroup 0 also takes the bias
// gradient.
__global__ __launch_bounds__(1024) void cap_att_bwd_batched_kernel(const float* __restrict__ ddot, const float* __restrict__ weight, const float* __restrict__ dres,
                                                                  int ldr, const float* __restrict__ tanh_ws, const float* __restrict__ aw, int S, int L, int D,
                                                                  float* dpatt, float* datt, float* daw, float* dab) {
  __shared__ float part[64][16];
  __shared__ float red[16];
  const int tid = threadIdx.x, dl = tid & 15, ll = tid >> 4;
  const int d = blockIdx.x * 16 + dl;
  float dwsum = 0.f;
  if (d < D) {
    const float a = aw[d];
    for (int l = ll; l < L; l += 64) {
      float dp = 0.f, da = 0.f, dw = 0.f;
      for (int t = 0; t < S; ++t) {
        const float dd = ddot[(long)t * L + l], w = weight[(long)t * L + l];
        const float th = tanh_ws[((long)t * L + l) * D + d];
        dp = fmaf(dd * a, 1.f - th * th, dp);
        if (dres) da = fmaf(w, dres[(long)t * ldr + d], da);
        dw = fmaf(dd, th, dw);
      }
      dpatt[(long)l * D + d] += dp;
      if (dres) datt[(long)l * D + d] += da;
      dwsum += dw;
    }
  }
  part[ll][dl] = dwsum;
  __syncthreads();
  if (ll == 0 && d < D) {
    float v = 0.f;
    for (int g = 0; g < 64; ++g) v += part[g][dl];
    daw[d] += v;
  }
  if (blockIdx.x == 0) {
    float sb = 0.f;
    for (int e = tid; e < S * L; e += 1024) sb += ddot[e];
    sb = block_sum(sb, red);
    if (tid == 0) dab[0] += sb;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Per-token steps of the top-down attention captioner.  The decomposition is rnn_step.hip's: grid ceil(R / 4), 256 threads = 4 waves, ONE
// WAVE PER HIDDEN UNIT; a lane loads float4s of the unit's weight rows and of the input vectors, the wave adds up (wave_sum) and lane 0
// finishes the cell.  One launch per cell and token; no atomics, nothing waits for another workgroup.
//   forward : gates[4R] = pre + add0 + add1 + sum over up to two segments W_k x_k, where W_k is a COLUMN SLICE [4R][n_k] (leading dimension
//             ld_k) of a wider matrix: the attention cell reads h_lang(i-1) and h_att(i-1), the language cell [att_res; h_att(i)] and h_lang(i-1).
//   backward: dh[R] = add0 + add1 + sum over up to three segments T_k v_k with T_k a [R][n_k] block (leading dimension ld_k) of a transposed
//             copy; then the cell's own backward: the four gate gradients and dc_prev.
// Segments whose length, leading dimension or address is not a multiple of 4 floats take the scalar loop (one launch-wide switch).
struct Seg { const float* x; const float* w; int ld; int n; };
struct CellF { const float* pre; const float* add0; const float* add1; Seg s0, s1; const float* c_prev; float* c; float* h; float* act; };

template <bool VEC>
__global__ __launch_bounds__(256) void topdown_cell_fwd_kernel(CellF a, int R) {
  __builtin_amdgcn_s_setprio(3);   // a link of the caption branch's dependent chain (the step's critical path): issue ahead of co-resident GEMM waves
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= R) return;
  float g[4] = {0.f, 0.f, 0.f, 0.f};
  if (a.s0.n > 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = row_dot<VEC>(a.s0.w + (long)(q * R + j) * a.s0.ld, a.s0.x, a.s0.n, lane, g[q]);
  }
  if (a.s1.n > 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = row_dot<VEC>(a.s1.w + (long)(q * R + j) * a.s1.ld, a.s1.x, a.s1.n, lane, g[q]);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) g[q] = wave_sum(g[q]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (a.pre) g[q] += a.pre[q * R + j];
      if (a.add0) g[q] += a.add0[q * R + j];
      if (a.add1) g[q] += a.add1[q * R + j];
    }
    float act[4];
    lstm_cell_fwd(g, a.c_prev[j], a.c[j], a.h[j], act);
    st_rows<4>(a.act, R, j, act);
  }
}

struct CellB { Seg s0, s1, s2; const float* add0; const float* add1; const float* dc_in; const float* act; const float* c_prev; const float* c;
               float* dg; float* dc_prev; };

template <bool VEC>
__global__ __launch_bounds__(256) void topdown_cell_bwd_kernel(CellB a, int R) {
  __builtin_amdgcn_s_setprio(3);
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= R) return;
  float dh = 0.f;
  if (a.s0.n > 0) dh = row_dot<VEC>(a.s0.w + (long)j * a.s0.ld, a.s0.x, a.s0.n, lane, dh);
  if (a.s1.n > 0) dh = row_dot<VEC>(a.s1.w + (long)j * a.s1.ld, a.s1.x, a.s1.n, lane, dh);
  if (a.s2.n > 0) dh = row_dot<VEC>(a.s2.w + (long)j * a.s2.ld, a.s2.x, a.s2.n, lane, dh);
  dh = wave_sum(dh);
  if (lane == 0) {
    if (a.add0) dh += a.add0[j];
    if (a.add1) dh += a.add1[j];
    float act[4], dg[4];
    ld_rows<4>(act, a.act, R, j);
    lstm_cell_bwd(dh, a.dc_in ? a.dc_in[j] : 0.f, act, a.c_prev[j], a.c[j], dg, a.dc_prev[j]);
    st_rows<4>(a.dg, R, j, dg);
  }
}

// dst[r][c] = src[r][c] for a rows x cols block with leading dimensions ldd / lds (lds = 0: one source row for every destination row)
__global__ __launch_bounds__(256) void topdown_pack_rows_kernel(float* dst, int ldd, const float* __restrict__ src, int lds, int rows, int cols) {
  const long n = (long)rows * cols;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    const long r = i / cols; const int c = (int)(i - r * cols);
    dst[r * ldd + c] = src[r * lds + c];
  }
}

// attention backward at one token (the part the recurrence needs): softmax backward ddot[l] = w[l] (dweight[l] - sum_l w dweight), recomputed by
// every workgroup, and datt_h[d] = aw[d] sum_l ddot[l] (1 - tanh^2[l][d]).  sum_l ddot[l] is 0 exactly (the softmax ignores a common shift), but
// in float32 it is the rounding error of the inner sum times sum_l w[l]: where tanh^2 hardly varies over the locations that error IS the result.
// So the sum is taken in the form that does not see it: datt_h[d] = -aw[d] sum_l ddot[l] (tanh^2[l][d] - m[d]) with m[d] = sum_l w[l] tanh^2[l][d],
// the weighted mean - an error e w[l] in ddot[l] then adds e (m - m) = 0.  Workgroup = 16 channels x 64 location groups; fixed summation order.
// (That is why this kernel shares the softmax backward with the two att2in2 step kernels but not their att_h_grad tail.)
__global__ __launch_bounds__(1024) void topdown_att_bwd_step_kernel(const float* __restrict__ dweight, const float* __restrict__ tanh_ws,
                                                                   const float* __restrict__ weight, const float* __restrict__ aw, int L, int D,
                                                                   float* ddot_out, float* datt_h) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ float ddot[256];
  __shared__ float wsh[256];
  __shared__ float red[16];
  __shared__ float part[64][17];
  __shared__ float mean[16];
  const int tid = threadIdx.x;
  const float wl = tid < L ? weight[tid] : 0.f;
  if (tid < 256) wsh[tid] = wl;
  block_softmax_bwd(wl, tid < L ? dweight[tid] : 0.f, L, ddot, red, ddot_out);
  const int dl = tid & 15, lg = tid >> 4;
  const int d = blockIdx.x * 16 + dl;
  float sm = 0.f;
  if (d < D) for (int l = lg; l < L; l += 64) { const float t = tanh_ws[(long)l * D + d]; sm = fmaf(wsh[l], t * t, sm); }
  part[lg][dl] = sm;
  __syncthreads();
  if (lg == 0) { float v = 0.f; for (int gi = 0; gi < 64; ++gi) v += part[gi][dl]; mean[dl] = v; }
  __syncthreads();
  const float m = mean[dl];
  float sah = 0.f;
  if (d < D) for (int l = lg; l < L; l += 64) { const float t = tanh_ws[(long)l * D + d]; sah = fmaf(ddot[l], t * t - m, sah); }
  __syncthreads();
  part[lg][dl] = sah;
  __syncthreads();
  if (lg == 0 && d < D) {
    float v = 0.f;
    for (int gi = 0; gi < 64; ++gi) v += part[gi][dl];
    datt_h[d] = -aw[d] * v;
  }
}

bool seg_ok(const l2s_topdown_seg& q) { return q.n == 0 || (q.n > 0 && q.x && q.w && q.ld >= q.n); }
bool seg_vec(const l2s_topdown_seg& q) { return q.n == 0 || !((q.n & 3) || (q.ld & 3) || ((uintptr_t)q.x & 15) || ((uintptr_t)q.w & 15)); }
Seg seg_of(const l2s_topdown_seg& q) { return Seg{q.x, q.w, q.ld, q.n > 0 ? q.n : 0}; }

}  // namespace

extern "C" int l2s_cap_attention_fwd(const float* patt, const float* att, const float* att_h, const float* aw, const float* ab, int L, int D,
                                     float* tanh_ws, float* weight, float* att_res, hipStream_t s) {
  if (L > 256) return L2S_EINVAL;
  // the softmax weights buffer doubles as the raw-dot scratch between the two launches
  L2S_LAUNCH(cap_att_dots_kernel, dim3(cdiv(L, 4)), dim3(256), 0, s, patt, att_h, aw, ab, L, D, tanh_ws, att_res + D);
  L2S_LAUNCH(cap_att_apply_kernel, dim3(cdiv(D, 64)), dim3(256), 0, s, att, att_res + D, L, D, weight, att_res);
  return l2s_check_launch();
}
extern "C" int l2s_cap_att_dots_fwd(const float* patt, const float* att_h, const float* aw, const float* ab, int L, int D, float* tanh_ws, float* dots,
                                    hipStream_t s) {
  if (L > 256) return L2S_EINVAL;
  L2S_LAUNCH(cap_att_dots_kernel, dim3(cdiv(L, 4)), dim3(256), 0, s, patt, att_h, aw, ab, L, D, tanh_ws, dots);
  return l2s_check_launch();
}
extern "C" int l2s_cap_att_dots_rows(const float* patt, const float* att_h, int ld_att_h, const float* aw, const float* ab, int rows, int row0,
                                     const int* count, int L, int D, float* dots, hipStream_t s) {
  if (!patt || !att_h || !aw || !ab || !dots || rows < 1 || rows > 65535 || row0 < 0 || L < 1 || L > 256 || D < 1 || ld_att_h < D) return L2S_EINVAL;
  L2S_LAUNCH(cap_att_dots_rows_kernel, dim3(cdiv(L, 4), rows), dim3(256), 0, s, patt, att_h, ld_att_h, aw, ab, row0, count, L, D, dots);
  return l2s_check_launch();
}
extern "C" int l2s_cap_att_dots_groups(const float* patt, const float* att_h, int ld_att_h, const float* aw, const float* ab, int rows, int group,
                                       int row0, const int* count, int L, int D, float* dots, hipStream_t s) {
  if (!patt || !att_h || !aw || !ab || !dots || rows < 1 || rows > 65535 || group < 1 || rows % group || row0 < 0 || L < 1 || L > 256 || D < 1 ||
      ld_att_h < D)
    return L2S_EINVAL;
  L2S_LAUNCH(cap_att_dots_groups_kernel, dim3(cdiv(L, 4), rows), dim3(256), 0, s, patt, att_h, ld_att_h, aw, ab, row0, count, group, L, D, dots);
  return l2s_check_launch();
}
extern "C" int l2s_cap_apply_gates_fwd(const float* P, const float* dots, const float* b_a2c, const float* sums, const float* c_prev, float* c, float* h,
                                       float* save, float* weight, int L, int R, hipStream_t s) {
  if (L > 256) return L2S_EINVAL;
  L2S_LAUNCH(cap_apply_gates_kernel, dim3(cdiv(R, 16)), dim3(256), 0, s, P, dots, b_a2c, sums, c_prev, c, h, save, weight, L, R);
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
extern "C" int l2s_cap_apply_gates_groups(const float* P, const float* dots, const float* b_a2c, const float* sums, int ld_sums, const float* c_prev,
                                          float* c, float* h, int rows, int group, int row0, const int* count, int L, int R, hipStream_t s) {
  if (!P || !dots || !b_a2c || !sums || !c_prev || !c || !h || rows < 1 || rows > 65535 || group < 1 || rows % group || row0 < 0 || L < 1 ||
      L > 256 || R < 1 || R > 1024 || ld_sums < 5 * R)
    return L2S_EINVAL;
  L2S_LAUNCH(cap_apply_gates_groups_kernel, dim3(cdiv(R, 16), rows), dim3(256), 0, s, P, dots, b_a2c, sums, ld_sums, c_prev, c, h, row0, count, group,
             L, R);
  return l2s_check_launch();
}
extern "C" int l2s_cap_gates_bwd_dw(const float* dh, const float* dh2, const float* dc_in, const float* save, const float* c_prev, const float* P,
                                    float* dsums, float* da2c, float* dc_prev, float* dweight, int L, int R, hipStream_t s) {
  if (R > 1024 || (R & 3) || ((uintptr_t)P & 15)) return L2S_EINVAL;
  L2S_LAUNCH(cap_gates_bwd_dw_kernel, dim3(cdiv(L, 4)), dim3(256), 0, s, dh, dh2, dc_in, save, c_prev, P, dsums, da2c, dc_prev, dweight, L, R);
  return l2s_check_launch();
}
extern "C" int l2s_cap_attention_bwd_step2(const float* dweight, const float* tanh_ws, const float* weight, const float* aw, int L, int D, float* ddot,
                                           float* datt_h, hipStream_t s) {
  if (L > 256) return L2S_EINVAL;
  L2S_LAUNCH(cap_att_bwd_step2_kernel, dim3(cdiv(D, 16)), dim3(1024), 0, s, dweight, tanh_ws, weight, aw, L, D, ddot, datt_h);
  return l2s_check_launch();
}
extern "C" int l2s_cap_attention_bwd(const float* datt_res, const float* att, const float* tanh_ws, const float* weight, const float* aw, int L, int D,
                                     float* dpatt, float* datt, float* datt_h, float* daw, float* dab, hipStream_t s) {
  if (L > 256) return L2S_EINVAL;
  L2S_LAUNCH(cap_att_bwd_dw_kernel, dim3(cdiv(L, 4)), dim3(256), 0, s, datt_res, att, L, D, datt_h + D);
  L2S_LAUNCH(cap_att_bwd_kernel, dim3(cdiv(D, 64)), dim3(256), 0, s, datt_res, datt_h + D, tanh_ws, weight, aw, L, D, dpatt, datt, datt_h, daw, dab);
  return l2s_check_launch();
}
extern "C" int l2s_linear2_fwd(const float* x, int K, const float* w1, const float* b1, float* y1, int N1, int acc1, const float* w2,
                               const float* b2, float* y2, int N2, int acc2, hipStream_t s) {
  if ((K & 3) || ((uintptr_t)x & 15) || ((uintptr_t)w1 & 15) || ((uintptr_t)w2 & 15)) return L2S_EINVAL;
  const int nb1 = cdiv(N1, 4);
  L2S_LAUNCH(linear2_fwd_kernel, dim3(nb1 + cdiv(N2, 4)), dim3(256), 0, s, x, K, w1, b1, y1, N1, acc1, w2, b2, y2, N2, acc2, nb1);
  return l2s_check_launch();
}
extern "C" int l2s_linear_sum2_fwd(const float* x1, const float* w1, int K1, const float* x2, const float* w2, int K2, float* y, int N,
                                   int accumulate, hipStream_t s) {
  if ((K1 & 3) || (K2 & 3) || ((uintptr_t)x1 & 15) || ((uintptr_t)x2 & 15) || ((uintptr_t)w1 & 15) || ((uintptr_t)w2 & 15)) return L2S_EINVAL;
  if (N <= 4096) L2S_LAUNCH(linear_sum2_split_kernel, dim3(N), dim3(256), 0, s, x1, w1, K1, x2, w2, K2, y, N, accumulate);
  else L2S_LAUNCH(linear_sum2_kernel, dim3(cdiv(N, 4)), dim3(256), 0, s, x1, w1, K1, x2, w2, K2, y, N, accumulate);
  return l2s_check_launch();
}
extern "C" int l2s_cap_a2c_gates_fwd(const float* att_res, const float* w_a2c, const float* b_a2c, int K, const float* sums, const float* c_prev,
                                     float* c, float* h, float* save, int R, hipStream_t s) {
  if ((K & 3) || ((uintptr_t)att_res & 15) || ((uintptr_t)w_a2c & 15)) return L2S_EINVAL;
  L2S_LAUNCH(cap_a2c_gates_kernel, dim3(cdiv(R, 4)), dim3(256), 0, s, att_res, w_a2c, b_a2c, K, sums, c_prev, c, h, save, R);
  return l2s_check_launch();
}
extern "C" int l2s_cap_attention_bwd_step(const float* datt_res, const float* att, const float* tanh_ws, const float* weight, const float* aw, int L,
                                          int D, float* ddot, float* datt_h, hipStream_t s) {
  if (L > 256 || (D & 3) || ((uintptr_t)datt_res & 15) || ((uintptr_t)att & 15)) return L2S_EINVAL;
  L2S_LAUNCH(cap_att_bwd_step_kernel, dim3(cdiv(D, 16)), dim3(1024), 0, s, datt_res, att, tanh_ws, weight, aw, L, D, ddot, datt_h);
  return l2s_check_launch();
}
extern "C" int l2s_cap_attention_bwd_batched(const float* ddot, const float* weight, const float* datt_res, int ldr, const float* tanh_ws,
                                             const float* aw, int S, int L, int D, float* dpatt, float* datt, float* daw, float* dab, hipStream_t s) {
  L2S_LAUNCH(cap_att_bwd_batched_kernel, dim3(cdiv(D, 16)), dim3(1024), 0, s, ddot, weight, datt_res, ldr, tanh_ws, aw, S, L, D, dpatt, datt, daw, dab);
  return l2s_check_launch();
}
extern "C" int l2s_cap_gates_fwd(const float* sums, const float* a2c, const float* c_prev, float* c, float* h, float* save, int R, hipStream_t s) {
  L2S_LAUNCH(cap_gates_fwd_kernel, dim3(cdiv(R, 256)), dim3(256), 0, s, sums, a2c, c_prev, c, h, save, R);
  return l2s_check_launch();
}
extern "C" int l2s_cap_gates_bwd(const float* dh, const float* dh2, const float* dc_in, const float* save, const float* c_prev, float* dsums, float* da2c,
                                 float* dc_prev, int R, hipStream_t s) {
  L2S_LAUNCH(cap_gates_bwd_kernel, dim3(cdiv(R, 256)), dim3(256), 0, s, dh, dh2, dc_in, save, c_prev, dsums, da2c, dc_prev, R);
  return l2s_check_launch();
}
extern "C" int l2s_topdown_cell_fwd(const l2s_topdown_fwd* a, int R, hipStream_t s) {
  if (!a || R < 4 || (R & 3) || !a->c_prev || !a->c || !a->h || !a->act || !seg_ok(a->seg[0]) || !seg_ok(a->seg[1])) return L2S_EINVAL;
  const CellF k{a->pre, a->add0, a->add1, seg_of(a->seg[0]), seg_of(a->seg[1]), a->c_prev, a->c, a->h, a->act};
  if (seg_vec(a->seg[0]) && seg_vec(a->seg[1])) L2S_LAUNCH(topdown_cell_fwd_kernel<true>, dim3(cdiv(R, 4)), dim3(256), 0, s, k, R);
  else L2S_LAUNCH(topdown_cell_fwd_kernel<false>, dim3(cdiv(R, 4)), dim3(256), 0, s, k, R);
  return l2s_check_launch();
}
extern "C" int l2s_topdown_cell_bwd(const l2s_topdown_bwd* a, int R, hipStream_t s) {
  if (!a || R < 4 || (R & 3) || !a->act || !a->c_prev || !a->c || !a->dgates || !a->dc_prev) return L2S_EINVAL;
  for (int i = 0; i < 3; ++i) if (!seg_ok(a->seg[i])) return L2S_EINVAL;
  const CellB k{seg_of(a->seg[0]), seg_of(a->seg[1]), seg_of(a->seg[2]), a->add0, a->add1, a->dc_in, a->act, a->c_prev, a->c, a->dgates, a->dc_prev};
  if (seg_vec(a->seg[0]) && seg_vec(a->seg[1]) && seg_vec(a->seg[2])) L2S_LAUNCH(topdown_cell_bwd_kernel<true>, dim3(cdiv(R, 4)), dim3(256), 0, s, k, R);
  else L2S_LAUNCH(topdown_cell_bwd_kernel<false>, dim3(cdiv(R, 4)), dim3(256), 0, s, k, R);
  return l2s_check_launch();
}
extern "C" int l2s_cap_att_apply_fwd(const float* att, const float* dots, int L, int R, float* weight, float* att_res, hipStream_t s) {
  if (!att || !dots || !weight || !att_res || L < 1 || L > 256 || R < 1) return L2S_EINVAL;
  L2S_LAUNCH(cap_att_apply_kernel, dim3(cdiv(R, 64)), dim3(256), 0, s, att, dots, L, R, weight, att_res);
  return l2s_check_launch();
}
extern "C" int l2s_cap_att_apply_rows(const float* att, const float* dots, float* att_res, int ld_res, int rows, int row0, const int* count, int L,
                                      int R, hipStream_t s) {
  if (!att || !dots || !att_res || rows < 1 || rows > 65535 || row0 < 0 || L < 1 || L > 256 || R < 1 || ld_res < R) return L2S_EINVAL;
  L2S_LAUNCH(cap_att_apply_rows_kernel, dim3(cdiv(R, 64), rows), dim3(256), 0, s, att, dots, att_res, ld_res, row0, count, L, R);
  return l2s_check_launch();
}
extern "C" int l2s_cap_att_apply_groups(const float* att, const float* dots, float* att_res, int ld_res, int rows, int group, int row0,
                                        const int* count, int L, int R, hipStream_t s) {
  if (!att || !dots || !att_res || rows < 1 || rows > 65535 || group < 1 || rows % group || row0 < 0 || L < 1 || L > 256 || R < 1 || ld_res < R)
    return L2S_EINVAL;
  L2S_LAUNCH(cap_att_apply_groups_kernel, dim3(cdiv(R, 64), rows), dim3(256), 0, s, att, dots, att_res, ld_res, row0, count, group, L, R);
  return l2s_check_launch();
}
extern "C" int l2s_pack_rows(float* dst, int ldd, const float* src, int lds, int rows, int cols, hipStream_t s) {
  if (!dst || !src || rows < 1 || cols < 1 || ldd < cols || (lds != 0 && lds < cols)) return L2S_EINVAL;
  const long n = (long)rows * cols;
  L2S_LAUNCH(topdown_pack_rows_kernel, dim3(cdiv(n, 256) < 1024 ? cdiv(n, 256) : 1024), dim3(256), 0, s, dst, ldd, src, lds, rows, cols);
  return l2s_check_launch();
}
extern "C" int l2s_cap_att_bwd_step_centered(const float* dweight, const float* tanh_ws, const float* weight, const float* aw, int L, int D, float* ddot,
                                             float* datt_h, hipStream_t s) {
  if (!dweight || !tanh_ws || !weight || !aw || !ddot || !datt_h || L < 1 || L > 256 || D < 1) return L2S_EINVAL;
  L2S_LAUNCH(topdown_att_bwd_step_kernel, dim3(cdiv(D, 16)), dim3(1024), 0, s, dweight, tanh_ws, weight, aw, L, D, ddot, datt_h);
  return l2s_check_launch();
}
