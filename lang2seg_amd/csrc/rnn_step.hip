// Recurrent steps of the language encoder (lang_encoder.py:21-24 builds getattr(nn, rnn_type.upper())): nn.LSTM (gate rows i, f, g, o),
// nn.GRU (gate rows r, z, n) and nn.RNN with tanh, plus the two copies that stack layers.  fp32, wave64, gfx950.
// One decomposition for every cell: grid (ceil(H / 4), ndir), 256 threads = 4 waves, ONE WAVE PER HIDDEN UNIT; a lane loads float4s of the
// unit's weight rows and of the previous state, the wave adds up on the DPP path (wave_sum, fixed order) and lane 0 finishes the cell.  Both
// directions of a layer in one launch (blockIdx.y); no atomics, nothing waits for another workgroup.  The LSTM cell itself is recur.h's (the
// top-down captioner's cells in caption_step.hip are the same cell); the unfused l2s_lstm_cell_* entries take ready-made pre-activations.
#include "common.h"
#include "../../include/lang2seg_hip.h"
#include "recur.h"

namespace {

__global__ void lstm_cell_fwd_kernel(const float* g, const float* c_prev, float* c, float* h, float* act, int Hh) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= Hh) return;
  // (the arithmetic of recur.h's lstm_cell_fwd stays written out here: through the function the compiler fuses the other product of the
  // cell update into the FMA in this kernel, and the low bits of c change)
  const float i = sigm(g[j]), f = sigm(g[Hh + j]), gg = tanhf(g[2 * Hh + j]), o = sigm(g[3 * Hh + j]);
  const float cn = f * c_prev[j] + i * gg;
  c[j] = cn; h[j] = o * tanhf(cn);
  act[j] = i; act[Hh + j] = f; act[2 * Hh + j] = gg; act[3 * Hh + j] = o;
}
__global__ void lstm_cell_bwd_kernel(const float* dh, const float* dc_in, const float* act, const float* c_prev, const float* c,
                                     float* dg, float* dc_prev, int Hh) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= Hh) return;
  float a[4], d[4];
  ld_rows<4>(a, act, Hh, j);
  lstm_cell_bwd(dh[j], dc_in ? dc_in[j] : 0.f, a, c_prev[j], c[j], d, dc_prev[j]);
  st_rows<4>(dg, Hh, j, d);
}

// ---- fused bi-LSTM steps (ENC:62, nn.LSTM gate order i,f,g,o).  One launch per time step for BOTH directions (grid.y = direction):
// forward : gates = g_in (x W_ih + b_ih, precomputed for all steps) + W_hh h_prev + b_hh, then the cell update; one wave per unit.
// backward: dh = W_hh^T dg_next (through the [Hh][4Hh] transposed copy; skipped at the first step, where dh is the gradient of the
//           final hidden state) and then the cell backward of this step for the same unit -- both are per-unit once dg_next is known.
struct LstmDir { const float* w; const float* b; const float* g_in; const float* h_prev; const float* c_prev; float* c; float* h; float* act; float* g_out; };
__global__ __launch_bounds__(256) void lstm_step_fwd_kernel(LstmDir d0, LstmDir d1, int Hh) {
  const LstmDir d = blockIdx.y ? d1 : d0;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= Hh) return;
  float a[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = lane * 4; k < Hh; k += 256) {
    const float4 hv = *(const float4*)(d.h_prev + k);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 wv = *(const float4*)(d.w + (long)(q * Hh + j) * Hh + k);
      a[q] = dot4(wv, hv, a[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) a[q] = wave_sum(a[q]);
  if (lane == 0) {
    float g[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { g[q] = d.g_in[q * Hh + j] + a[q] + d.b[q * Hh + j]; d.g_out[q * Hh + j] = g[q]; }
    float act[4];
    lstm_cell_fwd(g, d.c_prev[j], d.c[j], d.h[j], act);
    st_rows<4>(d.act, Hh, j, act);
  }
}
struct LstmBDir { const float* wT; const float* dg_next; const float* dh_ext; const float* dc_in; const float* act; const float* c_prev; const float* c; float* dg; float* dc_prev; };
__global__ __launch_bounds__(256) void lstm_step_bwd_kernel(LstmBDir d0, LstmBDir d1, int Hh) {
  const LstmBDir d = blockIdx.y ? d1 : d0;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= Hh) return;
  float dh = 0.f;
  if (d.dg_next) {
    const float* wr = d.wT + (long)j * 4 * Hh;
    for (int k = lane * 4; k < 4 * Hh; k += 256) {
      const float4 wv = *(const float4*)(wr + k), gv = *(const float4*)(d.dg_next + k);
      dh = dot4(wv, gv, dh);
    }
    dh = wave_sum(dh);
  }
  if (lane == 0) {
    if (d.dh_ext) dh += d.dh_ext[j];
    float act[4], dg[4];
    ld_rows<4>(act, d.act, Hh, j);
    lstm_cell_bwd(dh, d.dc_in ? d.dc_in[j] : 0.f, act, d.c_prev[j], d.c[j], dg, d.dc_prev[j]);
    st_rows<4>(d.dg, Hh, j, dg);
  }
}

// ---- nn.GRU: a = W_hh h_prev + b_hh; r = s(gi_r + a_r), z = s(gi_z + a_z), n = tanh(gi_n + r a_n), h = (1 - z) n + z h_prev
struct GruDir { const float* w; const float* b; const float* g_in; const float* h_prev; float* h; float* act; };
__global__ __launch_bounds__(256) void gru_step_fwd_kernel(GruDir d0, GruDir d1, int Hh) {
  const GruDir d = blockIdx.y ? d1 : d0;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= Hh) return;
  float a[3] = {0.f, 0.f, 0.f};
  for (int k = lane * 4; k < Hh; k += 256) {
    const float4 hv = *(const float4*)(d.h_prev + k);
#pragma unroll
    for (int q = 0; q < 3; ++q) a[q] = dot4(*(const float4*)(d.w + (long)(q * Hh + j) * Hh + k), hv, a[q]);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) a[q] = wave_sum(a[q]);
  if (lane == 0) {
    const float an = a[2] + d.b[2 * Hh + j];
    const float r = sigm(d.g_in[j] + a[0] + d.b[j]);
    const float z = sigm(d.g_in[Hh + j] + a[1] + d.b[Hh + j]);
    const float n = tanhf(d.g_in[2 * Hh + j] + r * an);
    d.h[j] = (1.f - z) * n + z * d.h_prev[j];
    d.act[j] = r; d.act[Hh + j] = z; d.act[2 * Hh + j] = n; d.act[3 * Hh + j] = an;
  }
}
// dh = W_hh^T dgh_next (through the [H][3H] transposed copy) + dh_ext + dh_carry_in; the carry is the direct path h_prev -> h (dh z)
struct GruBDir { const float* wT; const float* dgh_next; const float* dh_ext; const float* carry_in; const float* act; const float* h_prev;
                 float* dgi; float* dgh; float* carry_out; };
__global__ __launch_bounds__(256) void gru_step_bwd_kernel(GruBDir d0, GruBDir d1, int Hh) {
  const GruBDir d = blockIdx.y ? d1 : d0;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= Hh) return;
  float dh = 0.f;
  if (d.dgh_next) {
    const float* wr = d.wT + (long)j * 3 * Hh;
    for (int k = lane * 4; k < 3 * Hh; k += 256) dh = dot4(*(const float4*)(wr + k), *(const float4*)(d.dgh_next + k), dh);
    dh = wave_sum(dh);
  }
  if (lane == 0) {
    if (d.dh_ext) dh += d.dh_ext[j];
    if (d.carry_in) dh += d.carry_in[j];
    const float r = d.act[j], z = d.act[Hh + j], n = d.act[2 * Hh + j], an = d.act[3 * Hh + j];
    const float dn = dh * (1.f - z), dz = dh * (d.h_prev[j] - n);
    const float dan = dn * (1.f - n * n), daz = dz * z * (1.f - z), dar = dan * an * r * (1.f - r);
    d.dgi[j] = dar; d.dgi[Hh + j] = daz; d.dgi[2 * Hh + j] = dan;
    d.dgh[j] = dar; d.dgh[Hh + j] = daz; d.dgh[2 * Hh + j] = dan * r;
    d.carry_out[j] = dh * z;
  }
}

// ---- nn.RNN (tanh): h = tanh(gi + W_hh h_prev + b_hh); h is its own saved activation
struct RnnDir { const float* w; const float* b; const float* g_in; const float* h_prev; float* h; };
__global__ __launch_bounds__(256) void rnn_step_fwd_kernel(RnnDir d0, RnnDir d1, int Hh) {
  const RnnDir d = blockIdx.y ? d1 : d0;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= Hh) return;
  float a = 0.f;
  const float* wr = d.w + (long)j * Hh;
  for (int k = lane * 4; k < Hh; k += 256) a = dot4(*(const float4*)(wr + k), *(const float4*)(d.h_prev + k), a);
  a = wave_sum(a);
  if (lane == 0) d.h[j] = tanhf(d.g_in[j] + a + d.b[j]);
}
struct RnnBDir { const float* wT; const float* dg_next; const float* dh_ext; const float* h; float* dg; };
__global__ __launch_bounds__(256) void rnn_step_bwd_kernel(RnnBDir d0, RnnBDir d1, int Hh) {
  const RnnBDir d = blockIdx.y ? d1 : d0;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= Hh) return;
  float dh = 0.f;
  if (d.dg_next) {
    const float* wr = d.wT + (long)j * Hh;
    for (int k = lane * 4; k < Hh; k += 256) dh = dot4(*(const float4*)(wr + k), *(const float4*)(d.dg_next + k), dh);
    dh = wave_sum(dh);
  }
  if (lane == 0) {
    if (d.dh_ext) dh += d.dh_ext[j];
    const float h = d.h[j];
    d.dg[j] = dh * (1.f - h * h);
  }
}

// ---- stacking: the next layer's input row t is [h_fwd(t) | h_rev(t)] (* the inter-layer dropout mask); backward splits it again and adds
// the gradient of `hidden` at the row each direction processed last (forward: T - 1, reverse: 0)
__global__ __launch_bounds__(256) void rnn_concat_fwd_kernel(const float* h0, const float* h1, const float* mask, float* out, int T, int Hh, int ndir) {
  const long n = (long)T * ndir * Hh, W = (long)ndir * Hh;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    const long t = i / W; const int c = (int)(i - t * W);
    const float v = c < Hh ? h0[t * Hh + c] : h1[t * Hh + c - Hh];
    out[i] = mask ? v * mask[i] : v;
  }
}
__global__ __launch_bounds__(256) void rnn_concat_bwd_kernel(const float* dx, const float* mask, const float* add0, const float* add1, float* d0, float* d1,
                                                             int T, int Hh, int ndir) {
  const long n = (long)T * ndir * Hh, W = (long)ndir * Hh;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
    const long t = i / W; const int c = (int)(i - t * W);
    float v = mask ? dx[i] * mask[i] : dx[i];
    if (c < Hh) {
      if (add0 && t == T - 1) v += add0[c];
      d0[t * Hh + c] = v;
    } else {
      if (add1 && t == 0) v += add1[c - Hh];
      d1[t * Hh + c - Hh] = v;
    }
  }
}

}  // namespace

extern "C" int l2s_lstm_cell_fwd(const float* gates, const float* c_prev, float* c, float* h, float* act, int Hh, hipStream_t s) {
  L2S_LAUNCH(lstm_cell_fwd_kernel, dim3(cdiv(Hh, 256)), dim3(256), 0, s, gates, c_prev, c, h, act, Hh);
  return l2s_check_launch();
}
extern "C" int l2s_lstm_cell_bwd(const float* dh, const float* dc_in, const float* act, const float* c_prev, const float* c,
                                 float* dgates, float* dc_prev, int Hh, hipStream_t s) {
  L2S_LAUNCH(lstm_cell_bwd_kernel, dim3(cdiv(Hh, 256)), dim3(256), 0, s, dh, dc_in, act, c_prev, c, dgates, dc_prev, Hh);
  return l2s_check_launch();
}
#ifndef L2S_LSTM_STEP_FWD_EXTERNAL   // tools/lstm_pk_probe.sh links tools/lstm_pk_probe.hip's entry (and kernel variants) in place of this one
extern "C" int l2s_lstm_step_fwd(const l2s_lstm_fwd_dir* dirs, int ndir, int Hh, hipStream_t s) {
  if (!dirs || ndir < 1 || ndir > 2 || Hh < 4 || (Hh & 3)) return L2S_EINVAL;
  LstmDir a[2];
  for (int i = 0; i < 2; ++i) { const l2s_lstm_fwd_dir& q = dirs[i < ndir ? i : 0]; a[i] = LstmDir{q.w_hh, q.b_hh, q.gates_in, q.h_prev, q.c_prev, q.c, q.h, q.act, q.gates_out}; }
  L2S_LAUNCH(lstm_step_fwd_kernel, dim3(cdiv(Hh, 4), ndir), dim3(256), 0, s, a[0], a[1], Hh);
  return l2s_check_launch();
}
#endif
extern "C" int l2s_lstm_step_bwd(const l2s_lstm_bwd_dir* dirs, int ndir, int Hh, hipStream_t s) {
  if (!dirs || ndir < 1 || ndir > 2 || Hh < 4 || (Hh & 3)) return L2S_EINVAL;
  LstmBDir a[2];
  for (int i = 0; i < 2; ++i) { const l2s_lstm_bwd_dir& q = dirs[i < ndir ? i : 0]; a[i] = LstmBDir{q.w_hh_T, q.dgates_next, q.dh_ext, q.dc_in, q.act, q.c_prev, q.c, q.dgates, q.dc_prev}; }
  L2S_LAUNCH(lstm_step_bwd_kernel, dim3(cdiv(Hh, 4), ndir), dim3(256), 0, s, a[0], a[1], Hh);
  return l2s_check_launch();
}
extern "C" int l2s_gru_step_fwd(const l2s_gru_fwd_dir* dirs, int ndir, int Hh, hipStream_t s) {
  if (!dirs || ndir < 1 || ndir > 2 || Hh < 4 || (Hh & 3)) return L2S_EINVAL;
  GruDir a[2];
  for (int i = 0; i < 2; ++i) { const l2s_gru_fwd_dir& q = dirs[i < ndir ? i : 0]; a[i] = GruDir{q.w_hh, q.b_hh, q.gates_in, q.h_prev, q.h, q.act}; }
  L2S_LAUNCH(gru_step_fwd_kernel, dim3(cdiv(Hh, 4), ndir), dim3(256), 0, s, a[0], a[1], Hh);
  return l2s_check_launch();
}
extern "C" int l2s_gru_step_bwd(const l2s_gru_bwd_dir* dirs, int ndir, int Hh, hipStream_t s) {
  if (!dirs || ndir < 1 || ndir > 2 || Hh < 4 || (Hh & 3)) return L2S_EINVAL;
  GruBDir a[2];
  for (int i = 0; i < 2; ++i) {
    const l2s_gru_bwd_dir& q = dirs[i < ndir ? i : 0];
    a[i] = GruBDir{q.w_hh_T, q.dgh_next, q.dh_ext, q.dh_carry_in, q.act, q.h_prev, q.dgi, q.dgh, q.dh_carry_out};
  }
  L2S_LAUNCH(gru_step_bwd_kernel, dim3(cdiv(Hh, 4), ndir), dim3(256), 0, s, a[0], a[1], Hh);
  return l2s_check_launch();
}
extern "C" int l2s_rnn_step_fwd(const l2s_rnn_fwd_dir* dirs, int ndir, int Hh, hipStream_t s) {
  if (!dirs || ndir < 1 || ndir > 2 || Hh < 4 || (Hh & 3)) return L2S_EINVAL;
  RnnDir a[2];
  for (int i = 0; i < 2; ++i) { const l2s_rnn_fwd_dir& q = dirs[i < ndir ? i : 0]; a[i] = RnnDir{q.w_hh, q.b_hh, q.gates_in, q.h_prev, q.h}; }
  L2S_LAUNCH(rnn_step_fwd_kernel, dim3(cdiv(Hh, 4), ndir), dim3(256), 0, s, a[0], a[1], Hh);
  return l2s_check_launch();
}
extern "C" int l2s_rnn_step_bwd(const l2s_rnn_bwd_dir* dirs, int ndir, int Hh, hipStream_t s) {
  if (!dirs || ndir < 1 || ndir > 2 || Hh < 4 || (Hh & 3)) return L2S_EINVAL;
  RnnBDir a[2];
  for (int i = 0; i < 2; ++i) { const l2s_rnn_bwd_dir& q = dirs[i < ndir ? i : 0]; a[i] = RnnBDir{q.w_hh_T, q.dg_next, q.dh_ext, q.h, q.dg}; }
  L2S_LAUNCH(rnn_step_bwd_kernel, dim3(cdiv(Hh, 4), ndir), dim3(256), 0, s, a[0], a[1], Hh);
  return l2s_check_launch();
}
extern "C" int l2s_rnn_concat_fwd(const float* h0, const float* h1, const float* mask, float* out, int T, int Hh, int ndir, hipStream_t s) {
  if (!h0 || !out || T < 1 || Hh < 1 || ndir < 1 || ndir > 2 || (ndir == 2 && !h1)) return L2S_EINVAL;
  const long n = (long)T * ndir * Hh;
  L2S_LAUNCH(rnn_concat_fwd_kernel, dim3(cdiv(n, 256) < 1024 ? cdiv(n, 256) : 1024), dim3(256), 0, s, h0, h1, mask, out, T, Hh, ndir);
  return l2s_check_launch();
}
extern "C" int l2s_rnn_concat_bwd(const float* dx, const float* mask, const float* add0, const float* add1, float* d0, float* d1, int T, int Hh,
                                  int ndir, hipStream_t s) {
  if (!dx || !d0 || T < 1 || Hh < 1 || ndir < 1 || ndir > 2 || (ndir == 2 && !d1)) return L2S_EINVAL;
  const long n = (long)T * ndir * Hh;
  L2S_LAUNCH(rnn_concat_bwd_kernel, dim3(cdiv(n, 256) < 1024 ? cdiv(n, 256) : 1024), dim3(256), 0, s, dx, mask, add0, add1, d0, d1, T, Hh, ndir);
  return l2s_check_launch();
}
