// Language side of the lang2seg train step on gfx950 outside the recurrences: the row-batch linear layers (forward, data and weight
// gradients), the embedding, the spatial dynamic-filter correlation and the captioner's log-softmax + NLL, forward + backward, fp32.
// Reference: lib/layers/lang_encoder.py:27-82, lib/caption_models/AttModel.py:60-101, lib/misc/utils.py:43-53,
// pyutils/mask-faster-rcnn/lib/nets/network_cycle_res5_2.py:504-562.
// Single rows (M = 1) are GEMVs: weights streamed once per call, one wave per output row, wave-level reductions; row batches (M = 21
// tokens, 196 attention locations) run on the exact-fp32 MFMA (linear_nt_mfma_kernel / linear_nn_mfma_kernel / linear_tn_mfma_kernel).
// The encoder's recurrent steps are in rnn_step.hip, the captioners' per-token kernels in caption_step.hip and cap_recur.hip.
#include "common.h"
#include "../../include/lang2seg_hip.h"
#include "recur.h"   // sigm

namespace {

constexpr int MAXM = 24;   // rows handled per wave pass in the skinny kernels
typedef float floatx4 __attribute__((ext_vector_type(4)));


__device__ __forceinline__ float act_apply(float v, int act) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 2) return tanhf(v);
  return v;
}

// y[m][n] = act(sum_k x[m][k] w[n][k] + b[n] (+ y[m][n]));  a wave owns NW consecutive outputs n and M <= MT rows per pass: every x
// vector it loads is used for NW weight rows (the one-output-per-wave form re-read the whole x block per output: 144 MB of L1 traffic
// for the 21 x 3350 x 512 logit layer, 40 us).  VW = floats per load: 4 (rows 16-byte aligned), 2 (8-byte aligned: K = 3350) or 1.
template <int MT, int VW, int NW>
__global__ __launch_bounds__(256) void linear_fwd_kernel(const float* __restrict__ x, int ldx_, const float* __restrict__ w, int ldw,
                                                        const float* __restrict__ b, float* y, int ldy, int m0, int M, int N, int K,
                                                        int act, int accumulate) {
  const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * NW, lane = threadIdx.x & 63;
  if (n0 >= N) return;
  m0 += blockIdx.y * MT;                       // row chunks of one launch
  float acc[MT][NW];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < NW; ++j) acc[m][j] = 0.f;
  for (int k = lane * VW; k < K; k += 64 * VW) {
    float wv[NW][VW];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const float* wr = w + (long)min(n0 + j, N - 1) * ldw + k;
      if (VW == 4) { const float4 t = *(const float4*)wr; wv[j][0] = t.x; wv[j][1] = t.y; wv[j][VW > 2 ? 2 : 0] = t.z; wv[j][VW > 3 ? 3 : 0] = t.w; }
      else if (VW == 2) { const float2 t = *(const float2*)wr; wv[j][0] = t.x; wv[j][VW > 1 ? 1 : 0] = t.y; }
      else wv[j][0] = *wr;
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      if (m0 + m < M) {
        const float* xr = x + (long)(m0 + m) * ldx_ + k;
        float xv[VW];
        if (VW == 4) { const float4 t = *(const float4*)xr; xv[0] = t.x; xv[1] = t.y; xv[VW > 2 ? 2 : 0] = t.z; xv[VW > 3 ? 3 : 0] = t.w; }
        else if (VW == 2) { const float2 t = *(const float2*)xr; xv[0] = t.x; xv[VW > 1 ? 1 : 0] = t.y; }
        else xv[0] = *xr;
#pragma unroll
        for (int j = 0; j < NW; ++j)
#pragma unroll
          for (int e = 0; e < VW; ++e) acc[m][j] = fmaf(wv[j][e], xv[e], acc[m][j]);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < NW; ++j) acc[m][j] = wave_sum(acc[m][j]);
  if (lane == 0) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
      if (m0 + m < M) {
#pragma unroll
        for (int j = 0; j < NW; ++j)
          if (n0 + j < N) {
            float v = acc[m][j] + (b ? b[n0 + j] : 0.f);
            float* o = y + (long)(m0 + m) * ldy + n0 + j;
            if (accumulate) v += *o;
            *o = act_apply(v, act);
          }
      }
  }
}

// dx[m][k] (+)= (sum_n dy[m][n] w[n][k]) (* mul[m][k])  (transposed GEMV): block = 64 k-columns (one per lane) x 16 n-groups
// (one per wave); every wave streams whole 256-byte rows of w; cross-wave reduction through LDS; no atomics.
template <int MT>
__global__ __launch_bounds__(1024) void gemvT_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ w, float* dx,
                                                    int lddx, int m0, int M, int N, int K, int accumulate, const float* __restrict__ mul) {
  __shared__ float sh[MT][16][64];
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int k = blockIdx.x * 64 + lane;
  float acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = 0.f;
  if (k < K) {
    for (int n = g; n < N; n += 16) {
      const float wv = w[(long)n * K + k];
#pragma unroll
      for (int m = 0; m < MT; ++m)
        if (m0 + m < M) acc[m] = fmaf(dy[(long)(m0 + m) * lddy + n], wv, acc[m]);
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m) sh[m][g][lane] = acc[m];
  __syncthreads();
  // 1024 threads reduce MT*64 outputs: thread -> (m = tid / 64, lane)
  for (int o = threadIdx.x; o < MT * 64; o += 1024) {
    const int m = o >> 6, l = o & 63, kk = blockIdx.x * 64 + l;
    if (m0 + m < M && kk < K) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 16; ++j) s += sh[m][j][l];
      if (mul) s *= mul[(long)(m0 + m) * lddx + kk];     // the product alone, as in the MFMA kernels: what dx held is added after it
      float* out = dx + (long)(m0 + m) * lddx + kk;
      *out = accumulate ? (*out + s) : s;
    }
  }
}

// dw[n][k] += sum_m dy[m][n] x[m][k]; db[n] += sum_m dy[m][n].  A block owns 256 columns k and NB rows n (dy[m][n] is uniform: scalar
// loads); single owner per output, no atomics.
__global__ __launch_bounds__(256) void linear_bwd_w_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx_,
                                                          float* dw, float* db, int M, int N, int K) {
  constexpr int NB = 1;                    // (8 rows per block was measured slower inside the step: 378 vs 319 us for the 12 launches)
  const int n0 = blockIdx.y * NB;
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < K) {
    float acc[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[j] = 0.f;
    for (int m = 0; m < M; ++m) {
      const float xv = x[(long)m * ldx_ + k];
#pragma unroll
      for (int j = 0; j < NB; ++j) acc[j] = fmaf(dy[(long)m * lddy + min(n0 + j, N - 1)], xv, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) if (n0 + j < N) dw[(long)(n0 + j) * K + k] += acc[j];
  }
  if (db && blockIdx.x == 0 && threadIdx.x < NB && n0 + threadIdx.x < N) {
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += dy[(long)m * lddy + n0 + threadIdx.x];
    db[n0 + threadIdx.x] += s;
  }
}

__global__ void act_bwd_kernel(float* dy, const float* y, long n, int act) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = y[i];
    if (act == 1) { if (!(v > 0.f)) dy[i] = 0.f; }
    else if (act == 2) dy[i] *= (1.f - v * v);
  }
}

// x *= mul (optional); x = 0 where !(relu_ref > 0); out = x in the activation dtype: dropout mask, ReLU backward and the cast in front of a
// convolution's data gradient in ONE launch (the tail of the captioner's backward pass, on the caption branch's critical chain)
template <typename T>
__global__ void mask_relu_cast_kernel(float* x, const float* __restrict__ mul, const float* __restrict__ relu_ref, T* out, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = x[i];
    if (mul) v *= mul[i];
    if (!(relu_ref[i] > 0.f)) v = 0.f;
    x[i] = v;
    Elem<T>::st(out + i, v);
  }
}

__global__ void embed_fwd_kernel(const float* table, const int64_t* ids, const float* mask, float* out, int T, int D, int relu) {
  const int t = blockIdx.x;
  const float* row = table + ids[t] * (long)D;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float v = row[d];
    if (relu) v = fmaxf(v, 0.f);
    if (mask) v *= mask[(long)t * D + d];
    out[(long)t * D + d] = v;
  }
}
// The same token may occur more than once in an expression: the block of its FIRST occurrence adds all of them into the table row, in
// position order (single owner per row: no atomics, bit-reproducible).
__global__ void embed_bwd_kernel(const float* dout, const float* out, const int64_t* ids, const float* mask, float* dtable, int T, int D, int relu) {
  const int t = blockIdx.x;
  const int64_t id = ids[t];
  for (int u = 0; u < t; ++u) if (ids[u] == id) return;          // (uniform) an earlier position owns this row
  float* row = dtable + id * (long)D;
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float acc = row[d];
    for (int u = t; u < T; ++u) {
      if (ids[u] != id) continue;
      float g = dout[(long)u * D + d];
      if (mask) g *= mask[(long)u * D + d];
      if (relu && out[(long)u * D + d] == 0.f) g = 0.f;   // relu killed it (or the mask did, then g is 0 already)
      acc += g;
    }
    row[d] = acc;
  }
}

// ---------------------------------------------------------------- dynamic filter correlation
__device__ __forceinline__ void spatial_mask7(int y, int x, int H, int W, float m[7]) {
  // NET:530-557 (python-2 true division then int())
  m[0] = 1.f;
  m[1] = (y < (int)(H / 2.0)) ? 1.f : 0.f;
  m[2] = (y >= (int)(H / 2.0)) ? 1.f : 0.f;
  m[3] = (x < (int)(W / 2.0)) ? 1.f : 0.f;
  m[4] = (x >= (int)(W / 2.0)) ? 1.f : 0.f;
  m[5] = (y >= (int)(H / 4.0) && y < (int)(H * 3 / 4.0)) ? 1.f : 0.f;
  m[6] = (x >= (int)(W / 4.0) && x < (int)(W * 3 / 4.0)) ? 1.f : 0.f;
}
// one wave per pixel: 7 masked channel dot products, 7->1 mix, modulate
// gate 0: y = x * response (NET:562); gate 1: y = x * sigmoid(response) (network_cycle_response.py:568-570).  resp keeps the raw response.
__global__ __launch_bounds__(256) void dynfilter_fwd_kernel(const void* x, const float* __restrict__ filt, const float* __restrict__ r, void* y,
                                                           float* resp, float* respk, int H, int W, int C, int dt, int gate) {
  const int pix = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pix >= H * W) return;
  float d[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int c = lane; c < C; c += 64) {
    const float v = ldx(x, (long)pix * C + c, dt);
#pragma unroll
    for (int k = 0; k < 7; ++k) d[k] = fmaf(v, filt[k * C + c], d[k]);
  }
  float m[7]; spatial_mask7(pix / W, pix % W, H, W, m);
  float rs = 0.f;
#pragma unroll
  for (int k = 0; k < 7; ++k) { d[k] = wave_sum(d[k]) * m[k]; rs = fmaf(r[k], d[k], rs); }
  if (lane < 7) respk[(long)pix * 7 + lane] = d[lane];
  if (lane == 0) resp[pix] = rs;
  const float mult = gate ? sigm(rs) : rs;
  for (int c = lane; c < C; c += 64) stx(y, (long)pix * C + c, dt, ldx(x, (long)pix * C + c, dt) * mult);
}
// bf16, C % 8 == 0, C <= 2048: 8 channels (16 bytes) per lane and trip, the pixel's values stay in registers for the modulation
__global__ __launch_bounds__(256) void dynfilter_fwd_bf16_kernel(const bf16_t* __restrict__ x, const float* __restrict__ filt, const float* __restrict__ r, bf16_t* y,
                                                                float* resp, float* respk, int H, int W, int C, int gate) {
  const int pix = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pix >= H * W) return;
  float d[7] = {0, 0, 0, 0, 0, 0, 0};
  float xv[4][8];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = (lane + 64 * t) * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) xv[t][e] = 0.f;
    if (c < C) {
      const uint4 q = *(const uint4*)(x + (long)pix * C + c);
      const uint32_t qw[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) { xv[t][2 * e] = __uint_as_float(qw[e] << 16); xv[t][2 * e + 1] = __uint_as_float(qw[e] & 0xFFFF0000u); }
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const float4 f0 = *(const float4*)(filt + k * C + c), f1 = *(const float4*)(filt + k * C + c + 4);
        d[k] = fmaf(xv[t][0], f0.x, d[k]); d[k] = fmaf(xv[t][1], f0.y, d[k]); d[k] = fmaf(xv[t][2], f0.z, d[k]); d[k] = fmaf(xv[t][3], f0.w, d[k]);
        d[k] = fmaf(xv[t][4], f1.x, d[k]); d[k] = fmaf(xv[t][5], f1.y, d[k]); d[k] = fmaf(xv[t][6], f1.z, d[k]); d[k] = fmaf(xv[t][7], f1.w, d[k]);
      }
    }
  }
  float m[7]; spatial_mask7(pix / W, pix % W, H, W, m);
  float rs = 0.f;
#pragma unroll
  for (int k = 0; k < 7; ++k) { d[k] = wave_sum(d[k]) * m[k]; rs = fmaf(r[k], d[k], rs); }
  if (lane < 7) {
    float dv = d[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) if (lane == k) dv = d[k];
    respk[(long)pix * 7 + lane] = dv;
  }
  if (lane == 0) resp[pix] = rs;
  const float mult = gate ? sigm(rs) : rs;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int c = (lane + 64 * t) * 8;
    if (c < C) {
      uint4 o;
      o.x = (uint32_t)f2bf(xv[t][0] * mult) | ((uint32_t)f2bf(xv[t][1] * mult) << 16); o.y = (uint32_t)f2bf(xv[t][2] * mult) | ((uint32_t)f2bf(xv[t][3] * mult) << 16);
      o.z = (uint32_t)f2bf(xv[t][4] * mult) | ((uint32_t)f2bf(xv[t][5] * mult) << 16); o.w = (uint32_t)f2bf(xv[t][6] * mult) | ((uint32_t)f2bf(xv[t][7] * mult) << 16);
      *(uint4*)(y + (long)pix * C + c) = o;
    }
  }
}
// pass 1: dresp[p] = sum_c dy[p][c] x[p][c]   (dr[k] += sum_p dresp[p]*respk[p][k] is taken by pass 3, in a fixed order)
// (sigmoid gate: times sigma'(response); dresp_extra = gradient of the response BCE loss w.r.t. the raw response)
__global__ __launch_bounds__(256) void dynfilter_bwd1_kernel(const void* dy, const void* x, const float* respk, float* dresp, float* dr, int HW, int C, int dt,
                                                            int gate, const float* resp, const float* dresp_extra) {
  const int pix = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pix >= HW) return;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s = fmaf(ldx(dy, (long)pix * C + c, dt), ldx(x, (long)pix * C + c, dt), s);
  s = wave_sum(s);
  if (gate) { const float sg = sigm(resp[pix]); s *= sg * (1.f - sg); }
  if (dresp_extra) s += dresp_extra[pix];
  if (lane == 0) dresp[pix] = s;
}
// pass 2: dx[p][c] = dy*resp + dresp[p]*sum_k r_k m_k[p] f_k[c] (ReLU-masked by relu_ref); part[chunk][k][c] = sum_{p in chunk} dresp r_k m_k x[p][c]
// block = 64 channels x 4 pixel lanes, grid.y over pixel chunks; pass 3 adds the chunks' partial sums to dfilt in chunk order (no atomics)
__global__ __launch_bounds__(256) void dynfilter_bwd2_kernel(const void* dy, const void* x, const float* __restrict__ filt, const float* __restrict__ r,
                                                            const float* __restrict__ resp, const float* __restrict__ dresp, void* dx, const void* ref,
                                                            float* dfilt, int H, int W, int C, int dt, int pchunk, int gate) {
  __shared__ float red[4][7][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), pl = threadIdx.x >> 6;
  const int p0 = blockIdx.y * pchunk, p1 = min(H * W, p0 + pchunk);
  float fk[7], acc[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) { fk[k] = (c < C) ? filt[k * C + c] * r[k] : 0.f; acc[k] = 0.f; }
  for (int p = p0 + pl; p < p1; p += 4) {
    if (c >= C) break;
    float m[7]; spatial_mask7(p / W, p % W, H, W, m);
    const float dr_ = dresp[p];
    const float xv = ldx(x, (long)p * C + c, dt);
    float g = ldx(dy, (long)p * C + c, dt) * (gate ? sigm(resp[p]) : resp[p]);
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 7; ++k) { t = fmaf(m[k], fk[k], t); acc[k] = fmaf(dr_ * m[k], xv, acc[k]); }
    g = fmaf(dr_, t, g);
    if (ref && !(ldx(ref, (long)p * C + c, dt) > 0.f)) g = 0.f;
    stx(dx, (long)p * C + c, dt, g);
  }
#pragma unroll
  for (int k = 0; k < 7; ++k) red[pl][k][threadIdx.x & 63] = acc[k];
  __syncthreads();
  if (pl == 0 && c < C) {
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const int l = threadIdx.x;
      dfilt[((long)blockIdx.y * 7 + k) * C + c] = (red[0][k][l] + red[1][k][l] + red[2][k][l] + red[3][k][l]) * r[k];
    }
  }
}

// bf16 fast paths of passes 1 and 2 (C % 8 == 0 / C % 4 == 0, 16- and 8-byte accesses instead of one bf16 per lane).
__global__ __launch_bounds__(256) void dynfilter_bwd1_bf16_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, float* dresp, int HW, int C,
                                                                 int gate, const float* __restrict__ resp, const float* __restrict__ dresp_extra) {
  const int pix = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (pix >= HW) return;
  float s = 0.f;
  for (int c = lane * 8; c < C; c += 512) {
    const uint4 a = *(const uint4*)(dy + (long)pix * C + c), b = *(const uint4*)(x + (long)pix * C + c);
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s = fmaf(__uint_as_float(aw[k] << 16), __uint_as_float(bw[k] << 16), s);
      s = fmaf(__uint_as_float(aw[k] & 0xFFFF0000u), __uint_as_float(bw[k] & 0xFFFF0000u), s);
    }
  }
  s = wave_sum(s);
  if (gate) { const float sg = sigm(resp[pix]); s *= sg * (1.f - sg); }
  if (dresp_extra) s += dresp_extra[pix];
  if (lane == 0) dresp[pix] = s;
}
// block = 256 channels (64 lanes x 4) x 4 pixel lanes
__global__ __launch_bounds__(256) void dynfilter_bwd2_bf16_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x, const float* __restrict__ filt,
                                                                 const float* __restrict__ r, const float* __restrict__ resp, const float* __restrict__ dresp,
                                                                 bf16_t* dx, const bf16_t* __restrict__ ref, float* dfilt, int H, int W, int C, int pchunk, int gate) {
  __shared__ float red[4][7][256];
  const int lane = threadIdx.x & 63, pl = threadIdx.x >> 6;
  const int c = blockIdx.x * 256 + lane * 4;
  const int p0 = blockIdx.y * pchunk, p1 = min(H * W, p0 + pchunk);
  float fk[7][4], acc[7][4];
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) { fk[k][e] = (c < C) ? filt[k * C + c + e] * r[k] : 0.f; acc[k][e] = 0.f; }
  if (c < C) {
    for (int p = p0 + pl; p < p1; p += 4) {
      float m[7]; spatial_mask7(p / W, p % W, H, W, m);
      const float dr_ = dresp[p], mult = gate ? sigm(resp[p]) : resp[p];
      const uint2 xr = *(const uint2*)(x + (long)p * C + c), gr = *(const uint2*)(dy + (long)p * C + c);
      uint2 rr = make_uint2(0x3f803f80u, 0x3f803f80u);
      if (ref) rr = *(const uint2*)(ref + (long)p * C + c);
      const float xv[4] = {__uint_as_float(xr.x << 16), __uint_as_float(xr.x & 0xFFFF0000u), __uint_as_float(xr.y << 16), __uint_as_float(xr.y & 0xFFFF0000u)};
      const float gv[4] = {__uint_as_float(gr.x << 16), __uint_as_float(gr.x & 0xFFFF0000u), __uint_as_float(gr.y << 16), __uint_as_float(gr.y & 0xFFFF0000u)};
      const float rv[4] = {__uint_as_float(rr.x << 16), __uint_as_float(rr.x & 0xFFFF0000u), __uint_as_float(rr.y << 16), __uint_as_float(rr.y & 0xFFFF0000u)};
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float g = gv[e] * mult;
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 7; ++k) { t = fmaf(m[k], fk[k][e], t); acc[k][e] = fmaf(dr_ * m[k], xv[e], acc[k][e]); }
        g = fmaf(dr_, t, g);
        if (!(rv[e] > 0.f)) g = 0.f;
        o[e] = g;
      }
      *(uint2*)(dx + (long)p * C + c) = make_uint2((uint32_t)f2bf(o[0]) | ((uint32_t)f2bf(o[1]) << 16), (uint32_t)f2bf(o[2]) | ((uint32_t)f2bf(o[3]) << 16));
    }
  }
#pragma unroll
  for (int k = 0; k < 7; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) red[pl][k][lane * 4 + e] = acc[k][e];
  __syncthreads();
  // 256 threads: thread t finishes channel blockIdx.x * 256 + t for the seven taps
  const int cc = blockIdx.x * 256 + threadIdx.x;
  if (cc < C) {
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const int l = threadIdx.x;
      dfilt[((long)blockIdx.y * 7 + k) * C + cc] = (red[0][k][l] + red[1][k][l] + red[2][k][l] + red[3][k][l]) * r[k];
    }
  }
}
// pass 3: dfilt[k][c] += sum_chunk part[chunk][k][c] (chunk order); block 0 also dr[k] += sum_p dresp[p] respk[p][k] (fixed tree)
__global__ __launch_bounds__(256) void dynfilter_bwd3_kernel(const float* __restrict__ part, int nchunk, const float* __restrict__ dresp,
                                                            const float* __restrict__ respk, float* dfilt, float* dr, int HW, int C) {
  __shared__ float red[4];
  const int e = blockIdx.x * 256 + threadIdx.x;              // (k, c) flattened
  if (e < 7 * C) {
    float s = 0.f;
    for (int q = 0; q < nchunk; ++q) s += part[(long)q * 7 * C + e];
    dfilt[e] += s;
  }
  if (blockIdx.x == 0) {
    for (int k = 0; k < 7; ++k) {
      float s = 0.f;
      for (int p = threadIdx.x; p < HW; p += 256) s = fmaf(dresp[p], respk[(long)p * 7 + k], s);
      s = block_sum(s, red);
      if (threadIdx.x == 0) dr[k] += s;
    }
  }
}

// log_softmax + masked NLL over S rows (one workgroup per row)
__global__ __launch_bounds__(1024) void lsm_nll_kernel(const float* logits, const int64_t* target, const float* mask, int S, int V1, float gscale,
                                                      float* loss_slot, float* dlogits, float* logprobs) {
  __shared__ float red[16];
  const int srow = blockIdx.x, tid = threadIdx.x;
  const float* lr = logits + (long)srow * V1;
  float mx = -INFINITY;
  for (int v = tid; v < V1; v += blockDim.x) mx = fmaxf(mx, lr[v]);
  mx = block_max(mx, red);
  float se = 0.f;
  for (int v = tid; v < V1; v += blockDim.x) se += expf(lr[v] - mx);
  se = block_sum(se, red);
  const float lse = mx + logf(se);
  float msum = 0.f;
  for (int i = 0; i < S; ++i) msum += mask[i];
  const float mk = mask[srow];
  const int tg = (int)target[srow];
  for (int v = tid; v < V1; v += blockDim.x) {
    const float lp = lr[v] - lse;
    if (logprobs) logprobs[(long)srow * V1 + v] = lp;
    if (dlogits) dlogits[(long)srow * V1 + v] = gscale * mk / msum * (expf(lp) - (v == tg ? 1.f : 0.f));
  }
  if (tid == 0) atomicAdd(loss_slot, -(lr[tg] - lse) * mk / msum);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Row-batch linears on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32: a lane holds A[l%16][l/16] and B[l/16][l%16], D rows 4(l/16)+r).
// The wave-per-output kernels above re-read the x block per output and leave the 21 x 3350 x 512 logit layer at 40-200 us; these
// stream every weight exactly once with 16-byte loads, 4 k (or n) per lane per load: the MFMA's k index is a permutation of memory
// order, the same permutation on both operands.
//
// NT: y[m][n] = act(sum_k x[m][k] w[n][k] + b[n] (+ y)).  Workgroup = one 16-column tile x MT 16-row tiles; its 4 waves split K.
template <int MT>
__global__ __launch_bounds__(256) void linear_nt_mfma_kernel(const float* __restrict__ x, int ldx_, const float* __restrict__ w, int ldw,
                                                            const float* __restrict__ b, float* y, int ldy, int M, int N, int K,
                                                            int act, int accumulate) {
  __shared__ float red[4][MT][4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.x * 16, m0 = blockIdx.y * (16 * MT);
  const float* wr = w + (long)min(n0 + j, N - 1) * ldw;
  const float* xr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) xr[t] = x + (long)min(m0 + 16 * t + j, M - 1) * ldx_;
  floatx4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = floatx4{0.f, 0.f, 0.f, 0.f};
  const int kper = ((K + 63) / 64) * 16;                  // K range of one wave, a multiple of 16
  const int kb = wv * kper, ke = min(K, kb + kper);
#pragma unroll 4
  for (int k = kb; k < ke; k += 16) {
    const int kk = k + 4 * kq;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f), av[MT];
    const bool in = kk < ke;                              // K % 4 == 0: a lane's four k are all inside or all outside
    if (in) bv = *(const float4*)(wr + kk);
#pragma unroll
    for (int t = 0; t < MT; ++t) av[t] = in ? *(const float4*)(xr[t] + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t].x, bv.x, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t].y, bv.y, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t].z, bv.z, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t].w, bv.w, acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wv][t][r][lane] = acc[t][r];
  __syncthreads();
  // wave wv finishes register r = wv of every tile: row 4 (lane/16) + r, column lane % 16
  const int n = n0 + j;
  if (n < N) {
    const float bias = b ? b[n] : 0.f;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = m0 + 16 * t + 4 * kq + wv;
      if (m < M) {
        float v = ((red[0][t][wv][lane] + red[1][t][wv][lane]) + red[2][t][wv][lane]) + red[3][t][wv][lane] + bias;
        float* o = y + (long)m * ldy + n;
        if (accumulate) v += *o;
        *o = act_apply(v, act);
      }
    }
  }
}

// NN: dx[m][k] (+)= (sum_n dy[m][n] w[n][k]) (* mul[m][k]) from the weight as stored (no transposed copy).  A wave owns 64 output columns
// as four interleaved 16-column tiles (column k0 + 4 (lane%16) + q belongs to tile q: one 16-byte load of a weight row feeds four
// MFMAs), MT 16-row tiles, and a share of the contraction range; workgroup = 4 waves (LDS sum), grid.y = further split of n whose
// partial sums go to `ws` and are added in order by linear_nn_reduce_kernel (no atomics).
template <int MT>
__global__ __launch_bounds__(256) void linear_nn_mfma_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ w, float* dx,
                                                            int lddx, int M, int N, int K, int accumulate, const float* __restrict__ mul,
                                                            float* ws, int nper) {
  __shared__ float red[4][MT * 4][4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 15, kq = lane >> 4;
  const int k0 = blockIdx.x * 64, m0 = blockIdx.z * (16 * MT);
  const int nb0 = blockIdx.y * nper, ne0 = min(N, nb0 + nper);
  const int wper = ((ne0 - nb0 + 63) / 64) * 16;          // n range of one wave, a multiple of 16
  const int nb = nb0 + wv * wper, ne = min(ne0, nb + wper);
  const int kc = min(k0 + 4 * j, K - 4);                  // K % 4 == 0; columns past K are computed on a clamped address and not stored
  const float* dyr[MT]; bool rv[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) { const int m = m0 + 16 * t + j; rv[t] = m < M; dyr[t] = dy + (long)min(m, M - 1) * lddy; }
  floatx4 acc[MT][4];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[t][q] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int n = nb; n < ne; n += 16) {
    float4 bv[4]; float av[MT][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int nn = n + 4 * kq + e;
      bv[e] = *(const float4*)(w + (long)min(nn, N - 1) * K + kc);
#pragma unroll
      for (int t = 0; t < MT; ++t) av[t][e] = (nn < ne && rv[t]) ? dyr[t][nn] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][e], bv[e].x, acc[t][0], 0, 0, 0);
        acc[t][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][e], bv[e].y, acc[t][1], 0, 0, 0);
        acc[t][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][e], bv[e].z, acc[t][2], 0, 0, 0);
        acc[t][3] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t][e], bv[e].w, acc[t][3], 0, 0, 0);
      }
  }
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wv][t * 4 + q][r][lane] = acc[t][q][r];
  __syncthreads();
  // wave wv finishes the (tile, column set) pairs p = wv, wv + 4, ...: row 4 (lane/16) + r, column k0 + 4 (lane%16) + q
  const int Mpad = gridDim.z * 16 * MT;
  for (int p = wv; p < MT * 4; p += 4) {
    const int t = p >> 2, q = p & 3;
    const int kcol = k0 + 4 * j + q;
    if (kcol >= K) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + 16 * t + 4 * kq + r;
      if (m >= M) continue;
      float v = ((red[0][p][r][lane] + red[1][p][r][lane]) + red[2][p][r][lane]) + red[3][p][r][lane];
      if (gridDim.y > 1) { ws[((long)blockIdx.y * Mpad + m) * K + kcol] = v; continue; }
      if (mul) v *= mul[(long)m * lddx + kcol];
      float* o = dx + (long)m * lddx + kcol;
      *o = accumulate ? *o + v : v;
    }
  }
}
__global__ void linear_nn_reduce_kernel(const float* __restrict__ ws, int nsplit, int Mpad, float* dx, int lddx, int M, int K, int accumulate,
                                        const float* __restrict__ mul) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= (long)M * K) return;
  const int m = (int)(i / K), k = (int)(i - (long)m * K);
  float v = 0.f;
  for (int sp = 0; sp < nsplit; ++sp) v += ws[((long)sp * Mpad + m) * K + k];
  if (mul) v *= mul[(long)m * lddx + k];
  float* o = dx + (long)m * lddx + k;
  *o = accumulate ? *o + v : v;
}
// TN: dw[n][k] += sum_m dy[m][n] x[m][k] (weight gradient of a row batch), db[n] += sum_m dy[m][n].  The contraction index m is the slow
// index of both operands, so a 16-byte load along n (dy) / along k (x) feeds four interleaved 16-wide tiles: a wave owns a 64 (n) x 64 (k)
// block of dw as 4 x 4 tiles and walks m in steps of 4 (two loads, 16 MFMAs).  Single owner per output: no atomics.  The
// one-thread-per-column kernel above spent 55 us per call on average (13 calls, 0.7 ms of a 6.4 ms step) on these shapes.
template <bool VEC_DY>
__global__ __launch_bounds__(256) void linear_tn_mfma_kernel(const float* __restrict__ dy, int lddy, const float* __restrict__ x, int ldx_, float* dw, float* db,
                                                            int M, int N, int K) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, j = lane & 15, kq = lane >> 4;
  const int n0 = (blockIdx.y * 4 + wv) * 64, k0 = blockIdx.x * 64;
  if (n0 >= N) return;
  const int nc = n0 + 4 * j, kc = min(k0 + 4 * j, K - 4);         // K % 4 == 0; clamped columns are computed and not stored
  floatx4 acc[4][4];
  float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (int m0 = 0; m0 < M; m0 += 4) {
    const int m = m0 + kq;
    const bool mv = m < M;
    const float* dr = dy + (long)min(m, M - 1) * lddy;
    float av[4];
    if (VEC_DY) {
      const float4 t = (mv && nc + 3 < N) ? *(const float4*)(dr + nc) : make_float4(0.f, 0.f, 0.f, 0.f);
      av[0] = t.x; av[1] = t.y; av[2] = t.z; av[3] = t.w;
      if (mv && nc < N && nc + 3 >= N) {
#pragma unroll
        for (int q = 0; q < 4; ++q) av[q] = nc + q < N ? dr[nc + q] : 0.f;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) av[q] = (mv && nc + q < N) ? dr[nc + q] : 0.f;
    }
    const float4 bv = *(const float4*)(x + (long)min(m, M - 1) * ldx_ + kc);   // rows past M meet av == 0
    const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int a = 0; a < 4; ++a) cs[a] += av[a];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bb[b], acc[a][b], 0, 0, 0);
  }
  // tile (a, b): D row i <-> n = n0 + 4 i + a (i = 4 (lane / 16) + r), D column lane % 16 <-> k = k0 + 4 (lane % 16) + b: the four b make one float4
  const int kcol = k0 + 4 * j;
  if (kcol < K) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + 4 * (4 * kq + r) + a;
        if (n < N) {
          float4* o = (float4*)(dw + (long)n * K + kcol);
          float4 v = *o;
          v.x += acc[a][0][r]; v.y += acc[a][1][r]; v.z += acc[a][2][r]; v.w += acc[a][3][r];
          *o = v;
        }
      }
  }
  if (db && blockIdx.x == 0) {
    // column sums of dy from the values the lanes already hold: lane (j, kq) summed rows kq, kq + 4, ... of columns nc .. nc + 3
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = cs[q];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (kq == 0 && nc + q < N) db[nc + q] += v;
    }
  }
}
}  // namespace

extern "C" int l2s_linear_fwd(const float* x, int ldx_, const float* w, int ldw, const float* b, float* y, int ldy, int M, int N, int K, int act,
                              int accumulate, hipStream_t s) {
  if (M <= 0 || N <= 0) return L2S_OK;
  const bool v4 = !((K & 3) || (ldx_ & 3) || (ldw & 3) || ((uintptr_t)x & 15) || ((uintptr_t)w & 15));
  const bool v2 = !((K & 1) || (ldx_ & 1) || (ldw & 1) || ((uintptr_t)x & 7) || ((uintptr_t)w & 7));
  if (v4 && M >= 2) {
    // row batches: exact-fp32 MFMA tiles, every weight read once
    if (M <= 16) L2S_LAUNCH((linear_nt_mfma_kernel<1>), dim3(cdiv(N, 16), 1), dim3(256), 0, s, x, ldx_, w, ldw, b, y, ldy, M, N, K, act, accumulate);
    else L2S_LAUNCH((linear_nt_mfma_kernel<2>), dim3(cdiv(N, 16), cdiv(M, 32)), dim3(256), 0, s, x, ldx_, w, ldw, b, y, ldy, M, N, K, act, accumulate);
    return l2s_check_launch();
  }
  {
    const int m0 = 0;
    // one output per wave for a single row (GEMV: nothing to reuse), four outputs per wave for row batches
#define LF(MT, NW) do { dim3 grid(cdiv(N, 4 * NW), cdiv(M, MT)); \
                    if (v4) L2S_LAUNCH((linear_fwd_kernel<MT, 4, NW>), grid, dim3(256), 0, s, x, ldx_, w, ldw, b, y, ldy, m0, M, N, K, act, accumulate); \
                    else if (v2) L2S_LAUNCH((linear_fwd_kernel<MT, 2, NW>), grid, dim3(256), 0, s, x, ldx_, w, ldw, b, y, ldy, m0, M, N, K, act, accumulate); \
                    else L2S_LAUNCH((linear_fwd_kernel<MT, 1, NW>), grid, dim3(256), 0, s, x, ldx_, w, ldw, b, y, ldy, m0, M, N, K, act, accumulate); } while (0)
    // NW = 4 (x reused for four outputs) was measured slower inside the step (635 vs 441 us for the 11 row-batch launches: four times
    // fewer waves to hide the load latency on 512..3350 outputs), so every wave keeps one output
    static_assert(MAXM == 24, "the last form below is written as a number so that l2s_last_kernel names the instantiation");
    if (M <= 1) LF(1, 1); else if (M <= 8) LF(8, 1); else if (M <= 16) LF(16, 1); else LF(24, 1);
#undef LF
  }
  return l2s_check_launch();
}
// n-splits of the NN kernel for (M, N, K): enough workgroups to reach ~128, at least 64 n per workgroup
static int nn_split(int M, int N, int K) {
  const int tiles = cdiv(K, 64) * cdiv(M, 32);
  int sp = 128 / (tiles > 0 ? tiles : 1);
  const int maxsp = N / 64;
  if (sp > maxsp) sp = maxsp;
  if (sp > 32) sp = 32;
  return sp < 1 ? 1 : sp;
}
extern "C" long l2s_linear_bwd_x_ws_floats(int M, int N, int K) {
  const int sp = nn_split(M, N, K);
  return sp > 1 ? (long)sp * cdiv(M, 32) * 32 * K : 0;
}
extern "C" int l2s_linear_bwd_x(const float* dy, int lddy, const float* w, float* dx, int lddx, int M, int N, int K, int accumulate,
                                const float* mul, float* ws, long ws_floats, hipStream_t s) {
  if (M <= 0) return L2S_OK;
  // (a single row takes this path too when the matrix is large: it streams the weight once over ~128 workgroups instead of K / 64)
  if ((M >= 2 || (long)N * K >= (1L << 20)) && !(K & 3) && !((uintptr_t)w & 15) && K >= 4) {
    int sp = nn_split(M, N, K);
    const int mch = cdiv(M, 32), Mpad = mch * 32;
    if (!ws || ws_floats < (long)sp * Mpad * K) sp = 1;
    const int nper = cdiv(cdiv(N, sp), 16) * 16;
    sp = cdiv(N, nper);
    if (M <= 16 && sp == 1) L2S_LAUNCH((linear_nn_mfma_kernel<1>), dim3(cdiv(K, 64), 1, cdiv(M, 16)), dim3(256), 0, s, dy, lddy, w, dx, lddx, M, N, K, accumulate, mul, ws, nper);
    else L2S_LAUNCH((linear_nn_mfma_kernel<2>), dim3(cdiv(K, 64), sp, mch), dim3(256), 0, s, dy, lddy, w, dx, lddx, M, N, K, accumulate, mul, ws, nper);
    if (sp > 1) L2S_LAUNCH(linear_nn_reduce_kernel, dim3(cdiv((long)M * K, 256)), dim3(256), 0, s, (const float*)ws, sp, Mpad, dx, lddx, M, K, accumulate, mul);
    return l2s_check_launch();
  }
  dim3 grid(cdiv(K, 64));
  if (M == 1) L2S_LAUNCH(gemvT_kernel<1>, grid, dim3(1024), 0, s, dy, lddy, w, dx, lddx, 0, M, N, K, accumulate, mul);
  else for (int m0 = 0; m0 < M; m0 += 8) L2S_LAUNCH(gemvT_kernel<8>, grid, dim3(1024), 0, s, dy, lddy, w, dx, lddx, m0, M, N, K, accumulate, mul);
  return l2s_check_launch();
}
extern "C" int l2s_linear_bwd_w(const float* dy, int lddy, const float* x, int ldx_, float* dw, float* db, int M, int N, int K, hipStream_t s) {
  if (M <= 0) return L2S_OK;
  if (M >= 2 && K >= 4 && !(K & 3) && !(ldx_ & 3) && !((uintptr_t)x & 15) && !((uintptr_t)dw & 15)) {
    const dim3 grid(cdiv(K, 64), cdiv(N, 256));
    if (!(lddy & 3) && !((uintptr_t)dy & 15)) L2S_LAUNCH((linear_tn_mfma_kernel<true>), grid, dim3(256), 0, s, dy, lddy, x, ldx_, dw, db, M, N, K);
    else L2S_LAUNCH((linear_tn_mfma_kernel<false>), grid, dim3(256), 0, s, dy, lddy, x, ldx_, dw, db, M, N, K);
    return l2s_check_launch();
  }
  L2S_LAUNCH(linear_bwd_w_kernel, dim3(cdiv(K, 256), N), dim3(256), 0, s, dy, lddy, x, ldx_, dw, db, M, N, K);
  return l2s_check_launch();
}
extern "C" int l2s_act_bwd(float* dy, const float* y, long n, int act, hipStream_t s) {
  L2S_LAUNCH(act_bwd_kernel, dim3(cdiv(n, 256) > 1024 ? 1024 : cdiv(n, 256)), dim3(256), 0, s, dy, y, n, act);
  return l2s_check_launch();
}
extern "C" int l2s_mask_relu_cast(float* x, const float* mul, const float* relu_ref, void* out, int out_dtype, long n, hipStream_t s) {
  if (!x || !relu_ref || !out || (out_dtype != L2S_BF16 && out_dtype != L2S_F32)) return L2S_EINVAL;
  const int g = cdiv(n, 256) > 1024 ? 1024 : (int)cdiv(n, 256);
  if (out_dtype == L2S_BF16) { L2S_LAUNCH(mask_relu_cast_kernel<bf16_t>, dim3(g), dim3(256), 0, s, x, mul, relu_ref, (bf16_t*)out, n); }
  else { L2S_LAUNCH(mask_relu_cast_kernel<float>, dim3(g), dim3(256), 0, s, x, mul, relu_ref, (float*)out, n); }
  return l2s_check_launch();
}
extern "C" int l2s_embed_fwd(const float* table, const int64_t* ids, const float* mask, float* out, int T, int D, int relu, hipStream_t s) {
  L2S_LAUNCH(embed_fwd_kernel, dim3(T), dim3(256), 0, s, table, ids, mask, out, T, D, relu);
  return l2s_check_launch();
}
extern "C" int l2s_embed_bwd(const float* dout, const float* out, const int64_t* ids, const float* mask, float* dtable, int T, int D, int relu, hipStream_t s) {
  L2S_LAUNCH(embed_bwd_kernel, dim3(T), dim3(256), 0, s, dout, out, ids, mask, dtable, T, D, relu);
  return l2s_check_launch();
}
extern "C" int l2s_dynfilter_fwd(const void* x, const float* filt, const float* r, void* y, float* resp, float* respk, int H, int W, int C,
                                 int dtype, int gate, hipStream_t s) {
  if (dtype == L2S_BF16 && !(C & 7) && C <= 2048 && !((uintptr_t)x & 15) && !((uintptr_t)y & 15) && !((uintptr_t)filt & 15)) {
    L2S_LAUNCH(dynfilter_fwd_bf16_kernel, dim3(cdiv(H * W, 4)), dim3(256), 0, s, (const bf16_t*)x, filt, r, (bf16_t*)y, resp, respk, H, W, C, gate);
    return l2s_check_launch();
  }
  L2S_LAUNCH(dynfilter_fwd_kernel, dim3(cdiv(H * W, 4)), dim3(256), 0, s, x, filt, r, y, resp, respk, H, W, C, dtype, gate);
  return l2s_check_launch();
}
constexpr int DYN_PCHUNK = 32;   // pixels per partial-sum chunk of pass 2
extern "C" long l2s_dynfilter_ws_floats(int H, int W, int C) { return (long)H * W + (long)cdiv(H * W, DYN_PCHUNK) * 7 * C; }
extern "C" int l2s_dynfilter_bwd_finish(const float* ws, const float* respk, float* dfilt, float* dr, int H, int W, int C, hipStream_t s) {
  const float* dresp_ws = ws; const float* part = ws + (long)H * W;
  L2S_LAUNCH(dynfilter_bwd3_kernel, dim3(cdiv(7 * C, 256)), dim3(256), 0, s, part, cdiv(H * W, DYN_PCHUNK), dresp_ws, respk, dfilt, dr, H * W, C);
  return l2s_check_launch();
}
extern "C" int l2s_dynfilter_bwd(const void* dy, const void* x, const float* filt, const float* r, const float* resp, const float* respk,
                                 void* dx, const void* relu_ref, float* dfilt, float* dr, float* ws, int H, int W, int C, int dtype,
                                 int gate, const float* dresp_extra, hipStream_t s) {
  // ws: [H*W] d(response) followed by [chunks][7][C] partial filter gradients (l2s_dynfilter_ws_floats)
  // dfilt == NULL: only passes 1 and 2 (dx); the caller runs l2s_dynfilter_bwd_finish on whichever stream needs dfilt / dr
  float* dresp_ws = ws; float* part = ws + (long)H * W;
  const int pchunk = DYN_PCHUNK, nchunk = cdiv(H * W, pchunk);
  const bool fast = dtype == L2S_BF16 && !(C & 7) && !((uintptr_t)dy & 15) && !((uintptr_t)x & 15) && !((uintptr_t)dx & 15) && !((uintptr_t)relu_ref & 15);
  if (fast) {
    L2S_LAUNCH(dynfilter_bwd1_bf16_kernel, dim3(cdiv(H * W, 4)), dim3(256), 0, s, (const bf16_t*)dy, (const bf16_t*)x, dresp_ws, H * W, C, gate, resp, dresp_extra);
    L2S_LAUNCH(dynfilter_bwd2_bf16_kernel, dim3(cdiv(C, 256), nchunk), dim3(256), 0, s, (const bf16_t*)dy, (const bf16_t*)x, filt, r, resp, (const float*)dresp_ws,
               (bf16_t*)dx, (const bf16_t*)relu_ref, part, H, W, C, pchunk, gate);
  } else {
    L2S_LAUNCH(dynfilter_bwd1_kernel, dim3(cdiv(H * W, 4)), dim3(256), 0, s, dy, x, respk, dresp_ws, dr, H * W, C, dtype, gate, resp, dresp_extra);
    L2S_LAUNCH(dynfilter_bwd2_kernel, dim3(cdiv(C, 64), nchunk), dim3(256), 0, s, dy, x, filt, r, resp, (const float*)dresp_ws, dx, relu_ref,
                       part, H, W, C, dtype, pchunk, gate);
  }
  if (!dfilt) return l2s_check_launch();
  L2S_LAUNCH(dynfilter_bwd3_kernel, dim3(cdiv(7 * C, 256)), dim3(256), 0, s, (const float*)part, nchunk, (const float*)dresp_ws, respk, dfilt, dr, H * W, C);
  return l2s_check_launch();
}
extern "C" int l2s_logsoftmax_nll(const float* logits, const int64_t* target, const float* mask, int S, int V1, float gscale, float* loss_slot,
                                  float* dlogits, float* logprobs_opt, hipStream_t s) {
  L2S_LAUNCH(lsm_nll_kernel, dim3(S), dim3(1024), 0, s, logits, target, mask, S, V1, gscale, loss_slot, dlogits, logprobs_opt);
  return l2s_check_launch();
}
