// Per-token steps of the top-down attention captioner (lib/caption_models/AttModel.py:370-395: an attention nn.LSTMCell feeding a language
// nn.LSTMCell, gate rows i, f, g, o, two biases each).  fp32, wave64, gfx950.
// The decomposition is rnn_step.hip's: grid ceil(R / 4), 256 threads = 4 waves, ONE WAVE PER HIDDEN UNIT; a lane loads float4s of the unit's
// weight rows and of the input vectors, the wave adds up on the DPP path (wave_sum, fixed order) and lane 0 finishes the cell.  One launch per
// cell and token; no atomics, nothing waits for another workgroup.
//   forward : gates[4R] = pre + add0 + add1 + sum over up to two segments W_k x_k, where W_k is a COLUMN SLICE [4R][n_k] (leading dimension
//             ld_k) of a wider matrix: the attention cell reads h_lang(i-1) and h_att(i-1), the language cell [att_res; h_att(i)] and h_lang(i-1).
//   backward: dh[R] = add0 + add1 + sum over up to three segments T_k v_k with T_k a [R][n_k] block (leading dimension ld_k) of a transposed
//             copy; then the cell's own backward: the four gate gradients and dc_prev.
// Segments whose length, leading dimension or address is not a multiple of 4 floats take the scalar loop (one launch-wide switch).
// Beside the two cell steps: the two attention halves this captioner needs with a feature width of its own (softmax + weighted sum forward; the
// softmax backward with the sum over the locations in its well-conditioned form) and a row packer.
#include "common.h"
#include "../../include/lang2seg_hip.h"

namespace {

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float dot4(const float4 a, const float4 b, float acc) {
  return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, fmaf(a.w, b.w, acc))));
}
// one wave's partial dot product of row `w` with `x` over n elements (the caller reduces)
template <bool VEC>
__device__ __forceinline__ float row_dot(const float* __restrict__ w, const float* __restrict__ x, int n, int lane, float acc) {
  if (VEC) {
    for (int k = lane * 4; k < n; k += 256) acc = dot4(*(const float4*)(w + k), *(const float4*)(x + k), acc);
  } else {
    for (int k = lane; k < n; k += 64) acc = fmaf(w[k], x[k], acc);
  }
  return acc;
}

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
    const float ig = sigm(g[0]), fg = sigm(g[1]), gg = tanhf(g[2]), og = sigm(g[3]);
    const float cn = fg * a.c_prev[j] + ig * gg;
    a.c[j] = cn; a.h[j] = og * tanhf(cn);
    a.act[j] = ig; a.act[R + j] = fg; a.act[2 * R + j] = gg; a.act[3 * R + j] = og;
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
    const float ig = a.act[j], fg = a.act[R + j], gg = a.act[2 * R + j], og = a.act[3 * R + j];
    const float tc = tanhf(a.c[j]);
    const float dcn = (a.dc_in ? a.dc_in[j] : 0.f) + dh * og * (1.f - tc * tc);
    a.dg[j] = dcn * gg * ig * (1.f - ig);
    a.dg[R + j] = dcn * a.c_prev[j] * fg * (1.f - fg);
    a.dg[2 * R + j] = dcn * ig * (1.f - gg * gg);
    a.dg[3 * R + j] = dh * tc * og * (1.f - og);
    a.dc_prev[j] = dcn * fg;
  }
}

// softmax over the L <= 256 attention scores (recomputed by every workgroup) and att_res[d] = sum_l weight[l] att[l][d] for 64 channels per
// workgroup, 4 l-groups: the second half of ATT:419-421 with the feature width R independent of att_hid_size
__global__ __launch_bounds__(256) void topdown_att_apply_kernel(const float* __restrict__ att, const float* __restrict__ dots, int L, int R, float* weight,
                                                           float* att_res) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ float w[256];
  __shared__ float red[4];
  __shared__ float part[4][64];
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const float v = tid < L ? dots[tid] : -INFINITY;
  const float mx = block_max(v, red);
  const float e = tid < L ? expf(v - mx) : 0.f;
  const float sum = block_sum(e, red);
  if (tid < L) { w[tid] = e / sum; if (blockIdx.x == 0) weight[tid] = e / sum; }
  __syncthreads();
  const int d = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (d < R) for (int l = g; l < L; l += 4) s = fmaf(w[l], att[(long)l * R + d], s);
  part[g][lane] = s;
  __syncthreads();
  if (g == 0 && d < R) att_res[d] = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
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
  const float dw = tid < L ? dweight[tid] : 0.f;
  const float dot = block_sum(wl * dw, red);
  const float dd = wl * (dw - dot);
  if (tid < 256) { ddot[tid] = tid < L ? dd : 0.f; wsh[tid] = wl; }
  if (blockIdx.x == 0 && tid < L) ddot_out[tid] = dd;
  __syncthreads();
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
  L2S_LAUNCH(topdown_att_apply_kernel, dim3(cdiv(R, 64)), dim3(256), 0, s, att, dots, L, R, weight, att_res);
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
