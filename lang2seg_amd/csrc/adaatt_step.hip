// Kernels of the adaptive-attention captioners (--caption_model adaatt | adaattmo; lib/caption_models/AttModel.py:211-368), fp32, wave64, gfx950.
//   cell (ATT:241-297): an LSTM with row blocks in, forget, out, transform (adaattmo: two transform rows and their max) and a sentinel gate
//     fake = sigmoid(n5) tanh(c).  One launch per token each way: grid ceil(R / 4) x 256 threads, ONE WAVE PER HIDDEN UNIT, the G + 1 row dots
//     of the unit with h(i-1) (backward: the unit's rows of the transposed copies with d(sums | n5) of token i + 1), wave_sum, lane 0 finishes.
//   attention (ATT:325-357): additive attention over L + 1 slots, slot 0 the sentinel.  It reads the cell's outputs and feeds only the token's
//     logits - NOT the recurrence - so every launch here takes all S tokens at once (blockIdx.y = token): scores, softmax + weighted sum, and
//     backward the softmax backward + what flows on to the cell, then one launch for everything summed over tokens.
// No atomics, fixed summation order, nothing waits on another workgroup.  The cell's arithmetic is recur.h's.
#include "common.h"
#include "../../include/lang2seg_hip.h"
#include "recur.h"

namespace {

struct CellF { const float* pre; const float* fcrow; const float* w_hh; const float* b_hh; const float* w_r; const float* b_r; int ld_hh, ld_r;
               const float* h_prev; const float* c_prev; float* c; float* h; float* fake; float* save; };

template <int G, bool VEC>
__global__ __launch_bounds__(256) void adaatt_cell_fwd_kernel(CellF a, int R) {
  __builtin_amdgcn_s_setprio(3);   // a link of the caption branch's dependent chain: issue ahead of co-resident GEMM waves
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= R) return;
  float g[G + 1];
#pragma unroll
  for (int q = 0; q < G; ++q) g[q] = row_dot<VEC>(a.w_hh + (long)(q * R + j) * a.ld_hh, a.h_prev, R, lane, 0.f);
  g[G] = row_dot<VEC>(a.w_r + (long)j * a.ld_r, a.h_prev, R, lane, 0.f);
#pragma unroll
  for (int q = 0; q <= G; ++q) g[q] = wave_sum(g[q]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < G; ++q) g[q] = (a.pre[q * R + j] + a.fcrow[q * R + j]) + (g[q] + a.b_hh[q * R + j]);
    g[G] = (a.pre[G * R + j] + a.fcrow[G * R + j]) + (g[G] + a.b_r[j]);
    float sv[7];
    adaatt_cell_fwd<G == 5>(g, g[G], a.c_prev[j], a.c[j], a.h[j], a.fake[j], sv);
    st_rows<7>(a.save, R, j, sv);
  }
}

struct CellB { const float* dsn; const float* t_hh; const float* t_r; int ld_thh, ld_tr; const float* dh_ext; const float* dfake; const float* dc_in;
               const float* save; const float* c_prev; float* ds; float* dc_prev; };

template <int G, bool VEC>
__global__ __launch_bounds__(256) void adaatt_cell_bwd_kernel(CellB a, int R) {
  __builtin_amdgcn_s_setprio(3);
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= R) return;
  float dh = 0.f;
  if (a.dsn) {
    dh = row_dot<VEC>(a.t_hh + (long)j * a.ld_thh, a.dsn, G * R, lane, dh);
    dh = row_dot<VEC>(a.t_r + (long)j * a.ld_tr, a.dsn + G * R, R, lane, dh);
  }
  dh = wave_sum(dh);
  if (lane == 0) {
    if (a.dh_ext) dh += a.dh_ext[j];
    float sv[7], ds[5], dn5;
    ld_rows<7>(sv, a.save, R, j);
    adaatt_cell_bwd<G == 5>(sv, dh, a.dfake ? a.dfake[j] : 0.f, a.dc_in ? a.dc_in[j] : 0.f, a.c_prev[j], ds, dn5, a.dc_prev[j]);
    st_rows<G>(a.ds, R, j, ds);
    a.ds[G * R + j] = dn5;
  }
}

// scores: one wave per (token, slot).  Slot 0 embeds the sentinel (fre), slot l >= 1 location l - 1 (patt); hoe is added alike in every slot.
// tanh_ws keeps the tanh BEFORE the hA dropout mask; dots[s][256].
__global__ __launch_bounds__(256) void adaatt_scores_kernel(const float* __restrict__ patt, const float* __restrict__ fre, const float* __restrict__ hoe,
                                                           const float* __restrict__ aw, const float* __restrict__ ab, const float* __restrict__ mask,
                                                           int L1, int R, float* tanh_ws, float* dots) {
  __builtin_amdgcn_s_setprio(3);
  const int s = blockIdx.y, slot = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (slot >= L1) return;
  const float* e = slot == 0 ? fre + (long)s * R : patt + (long)(slot - 1) * R;
  const float* ho = hoe + (long)s * R;
  const long o = ((long)s * L1 + slot) * R;
  float acc = 0.f;
  for (int d = lane; d < R; d += 64) {
    const float t = tanhf(e[d] + ho[d]);
    tanh_ws[o + d] = t;
    acc = fmaf(mask ? t * mask[o + d] : t, aw[d], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) dots[s * 256 + slot] = acc + ab[0];
}
// PI = softmax over the L + 1 scores (recomputed per workgroup); atten[d] = PI[0] frl[d] + sum_l PI[l] att[l-1][d] + hol[d]; 64 channels per workgroup
__global__ __launch_bounds__(256) void adaatt_apply_kernel(const float* __restrict__ att, const float* __restrict__ frl, const float* __restrict__ hol,
                                                          const float* __restrict__ dots, int L1, int R, float* PI, float* atten) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ float w[256];
  __shared__ float red[4];
  __shared__ float part[4][64];
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const float wt = block_softmax(dots + s * 256, L1, red);
  w[tid] = tid < L1 ? wt : 0.f;
  if (tid < L1 && blockIdx.x == 0) PI[(long)s * L1 + tid] = wt;
  __syncthreads();
  const int d = blockIdx.x * 64 + lane;
  float acc = 0.f;
  if (d < R) for (int l = g; l < L1; l += 4) acc = fmaf(w[l], l == 0 ? frl[(long)s * R + d] : att[(long)(l - 1) * R + d], acc);
  part[g][lane] = acc;
  __syncthreads();
  if (g == 0 && d < R) atten[(long)s * R + d] = ((part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane])) + hol[(long)s * R + d];
}

// backward at every token, the part that flows on to the cell: dPI[l] = datten . slot_l, softmax backward ddot (recomputed per workgroup), and per
// channel d with u[l][d] = mask[l][d] (1 - tanh^2[l][d]):
//   d(hoe)[d] = aw[d] sum_l ddot[l] u[l][d]      d(fre)[d] = aw[d] ddot[0] u[0][d]      d(frl)[d] = PI[0] datten[d]      d(hol)[d] = datten[d]
// sum_l ddot[l] is 0 exactly and in float32 the rounding error e of the softmax backward's inner sum times sum_l PI[l]; where u hardly varies over
// the slots that error IS the plain sum.  As in l2s_cap_att_bwd_step_centered the sum is taken about the weighted mean m[d] = sum_l PI[l] u[l][d]:
// an error e PI[l] in ddot[l] then adds e (m - m) = 0.  (With the dropout mask inside, u replaces 1 - tanh^2; the argument does not change.)
// dctx = d(hoe) - d(fre): the sum over the LOCATIONS, which is ctx2att.bias's gradient.  Workgroup = 16 channels x 64 slot groups.
__global__ __launch_bounds__(1024) void adaatt_att_bwd_step_kernel(const float* __restrict__ datten, const float* __restrict__ att, const float* __restrict__ frl,
                                                                  const float* __restrict__ tanh_ws, const float* __restrict__ mask,
                                                                  const float* __restrict__ PI, const float* __restrict__ aw, int L1, int R,
                                                                  float* ddot_out, float* dhoe, float* dfre, float* dctx, float* dfrl, float* dhol) {
  __builtin_amdgcn_s_setprio(3);
  __shared__ float dwl[256];
  __shared__ float ddot[256];
  __shared__ float wsh[256];
  __shared__ float red[16];
  __shared__ float part[64][17];
  __shared__ float mean[16];
  const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* dres = datten + (long)s * R;
  // one row per trip (see cap_att_bwd_step_kernel in caption_step.hip)
  for (int l = wv; l < L1; l += 16) {
    const float* row = l == 0 ? frl + (long)s * R : att + (long)(l - 1) * R;
    float s0 = row_dot<true>(row, dres, R, lane, 0.f);
    s0 = wave_sum(s0);
    if (lane == 0) dwl[l] = s0;
  }
  __syncthreads();
  const float wl = tid < L1 ? PI[(long)s * L1 + tid] : 0.f;
  if (tid < 256) wsh[tid] = wl;
  block_softmax_bwd(wl, tid < L1 ? dwl[tid] : 0.f, L1, ddot, red, ddot_out + (long)s * L1);
  const int dl = tid & 15, lg = tid >> 4;
  const int d = blockIdx.x * 16 + dl;
  const long o = (long)s * L1 * R + d;
  float sm = 0.f;
  if (d < R) for (int l = lg; l < L1; l += 64) {
    const float t = tanh_ws[o + (long)l * R];
    const float u = mask ? mask[o + (long)l * R] * (1.f - t * t) : 1.f - t * t;
    sm = fmaf(wsh[l], u, sm);
  }
  part[lg][dl] = sm;
  __syncthreads();
  if (lg == 0) { float v = 0.f; for (int gi = 0; gi < 64; ++gi) v += part[gi][dl]; mean[dl] = v; }
  __syncthreads();
  const float m = mean[dl];
  float sah = 0.f, u0 = 0.f;
  if (d < R) for (int l = lg; l < L1; l += 64) {
    const float t = tanh_ws[o + (long)l * R];
    const float u = mask ? mask[o + (long)l * R] * (1.f - t * t) : 1.f - t * t;
    if (l == 0) u0 = u;
    sah = fmaf(ddot[l], u - m, sah);
  }
  __syncthreads();
  part[lg][dl] = sah;
  __syncthreads();
  if (lg == 0 && d < R) {
    float v = 0.f;
    for (int gi = 0; gi < 64; ++gi) v += part[gi][dl];
    const float ho = aw[d] * v, fr = aw[d] * ddot[0] * u0;
    const long q = (long)s * R + d;
    dhoe[q] = ho; dfre[q] = fr; dctx[q] = ho - fr;
    dfrl[q] = wsh[0] * dres[d]; dhol[q] = dres[d];
  }
}

// after that: everything summed over the S tokens in one launch (cap_att_bwd_batched_kernel's decomposition: 16 channels x 64 slot groups, a
// thread walks the tokens of its slots): d(p_att)[l] and d(att)[l] per location, d(alpha_net.weight)[d] over all slots and tokens in a fixed order
__global__ __launch_bounds__(1024) void adaatt_att_bwd_batched_kernel(const float* __restrict__ ddot, const float* __restrict__ PI, const float* __restrict__ datten,
                                                                     const float* __restrict__ tanh_ws, const float* __restrict__ mask,
                                                                     const float* __restrict__ aw, int S, int L1, int R, float* dpatt, float* datt, float* daw) {
  __shared__ float part[64][16];
  const int tid = threadIdx.x, dl = tid & 15, ll = tid >> 4;
  const int d = blockIdx.x * 16 + dl;
  float dwsum = 0.f;
  if (d < R) {
    const float a = aw[d];
    for (int l = ll; l < L1; l += 64) {
      float dp = 0.f, da = 0.f, dw = 0.f;
      for (int t = 0; t < S; ++t) {
        const long e = (long)t * L1 + l;
        const float th = tanh_ws[e * R + d];
        const float dd = mask ? ddot[e] * mask[e * R + d] : ddot[e];
        dp = fmaf(dd * a, 1.f - th * th, dp);
        da = fmaf(PI[e], datten[(long)t * R + d], da);
        dw = fmaf(dd, th, dw);
      }
      if (l > 0) { dpatt[(long)(l - 1) * R + d] += dp; datt[(long)(l - 1) * R + d] += da; }
      dwsum += dw;
    }
  }
  part[ll][dl] = dwsum;
  __syncthreads();
  if (ll == 0 && d < R) {
    float v = 0.f;
    for (int g = 0; g < 64; ++g) v += part[g][dl];
    daw[d] += v;
  }
}

bool al16(const void* p) { return !((uintptr_t)p & 15); }

}  // namespace

extern "C" int l2s_adaatt_cell_fwd(const l2s_adaatt_fwd* a, int R, int G, hipStream_t s) {
  if (!a || R < 4 || (R & 3) || (G != 4 && G != 5) || !a->pre || !a->fcrow || !a->w_hh || !a->b_hh || !a->w_r || !a->b_r || !a->h_prev || !a->c_prev ||
      !a->c || !a->h || !a->fake || !a->save || a->ld_hh < R || a->ld_r < R) return L2S_EINVAL;
  const CellF k{a->pre, a->fcrow, a->w_hh, a->b_hh, a->w_r, a->b_r, a->ld_hh, a->ld_r, a->h_prev, a->c_prev, a->c, a->h, a->fake, a->save};
  const bool vec = al16(a->w_hh) && al16(a->w_r) && al16(a->h_prev) && !(a->ld_hh & 3) && !(a->ld_r & 3);
  const dim3 grid(cdiv(R, 4)), blk(256);
  if (G == 4) { if (vec) L2S_LAUNCH((adaatt_cell_fwd_kernel<4, true>), grid, blk, 0, s, k, R); else L2S_LAUNCH((adaatt_cell_fwd_kernel<4, false>), grid, blk, 0, s, k, R); }
  else { if (vec) L2S_LAUNCH((adaatt_cell_fwd_kernel<5, true>), grid, blk, 0, s, k, R); else L2S_LAUNCH((adaatt_cell_fwd_kernel<5, false>), grid, blk, 0, s, k, R); }
  return l2s_check_launch();
}
extern "C" int l2s_adaatt_cell_bwd(const l2s_adaatt_bwd* a, int R, int G, hipStream_t s) {
  if (!a || R < 4 || (R & 3) || (G != 4 && G != 5) || !a->save || !a->c_prev || !a->ds || !a->dc_prev) return L2S_EINVAL;
  if (a->dsn && (!a->t_hh || !a->t_r || a->ld_thh < G * R || a->ld_tr < R)) return L2S_EINVAL;
  const CellB k{a->dsn, a->t_hh, a->t_r, a->ld_thh, a->ld_tr, a->dh_ext, a->dfake, a->dc_in, a->save, a->c_prev, a->ds, a->dc_prev};
  const bool vec = !a->dsn || (al16(a->dsn) && al16(a->t_hh) && al16(a->t_r) && !(a->ld_thh & 3) && !(a->ld_tr & 3));
  const dim3 grid(cdiv(R, 4)), blk(256);
  if (G == 4) { if (vec) L2S_LAUNCH((adaatt_cell_bwd_kernel<4, true>), grid, blk, 0, s, k, R); else L2S_LAUNCH((adaatt_cell_bwd_kernel<4, false>), grid, blk, 0, s, k, R); }
  else { if (vec) L2S_LAUNCH((adaatt_cell_bwd_kernel<5, true>), grid, blk, 0, s, k, R); else L2S_LAUNCH((adaatt_cell_bwd_kernel<5, false>), grid, blk, 0, s, k, R); }
  return l2s_check_launch();
}
extern "C" int l2s_adaatt_att_fwd(const float* att, const float* patt, const float* frl, const float* fre, const float* hoe, const float* hol,
                                  const float* aw, const float* ab, const float* mask, int S, int L, int R, float* tanh_ws, float* dots, float* PI,
                                  float* atten, hipStream_t s) {
  if (!att || !patt || !frl || !fre || !hoe || !hol || !aw || !ab || !tanh_ws || !dots || !PI || !atten || S < 1 || S > 65535 || L < 1 || L + 1 > 256 ||
      R < 1) return L2S_EINVAL;
  L2S_LAUNCH(adaatt_scores_kernel, dim3(cdiv(L + 1, 4), S), dim3(256), 0, s, patt, fre, hoe, aw, ab, mask, L + 1, R, tanh_ws, dots);
  L2S_LAUNCH(adaatt_apply_kernel, dim3(cdiv(R, 64), S), dim3(256), 0, s, att, frl, hol, dots, L + 1, R, PI, atten);
  return l2s_check_launch();
}
extern "C" int l2s_adaatt_att_bwd_step(const float* datten, const float* att, const float* frl, const float* tanh_ws, const float* mask, const float* PI,
                                       const float* aw, int S, int L, int R, float* ddot, float* dhoe, float* dfre, float* dctx, float* dfrl,
                                       float* dhol, hipStream_t s) {
  if (!datten || !att || !frl || !tanh_ws || !PI || !aw || !ddot || !dhoe || !dfre || !dctx || !dfrl || !dhol || S < 1 || S > 65535 || L < 1 ||
      L + 1 > 256 || R < 4 || (R & 3) || !al16(datten) || !al16(att) || !al16(frl)) return L2S_EINVAL;
  L2S_LAUNCH(adaatt_att_bwd_step_kernel, dim3(cdiv(R, 16), S), dim3(1024), 0, s, datten, att, frl, tanh_ws, mask, PI, aw, L + 1, R, ddot, dhoe, dfre, dctx,
             dfrl, dhol);
  return l2s_check_launch();
}
extern "C" int l2s_adaatt_att_bwd_batched(const float* ddot, const float* PI, const float* datten, const float* tanh_ws, const float* mask,
                                          const float* aw, int S, int L, int R, float* dpatt, float* datt, float* daw, hipStream_t s) {
  if (!ddot || !PI || !datten || !tanh_ws || !aw || !dpatt || !datt || !daw || S < 1 || L < 1 || L + 1 > 256 || R < 1) return L2S_EINVAL;
  L2S_LAUNCH(adaatt_att_bwd_batched_kernel, dim3(cdiv(R, 16)), dim3(1024), 0, s, ddot, PI, datten, tanh_ws, mask, aw, S, L + 1, R, dpatt, datt, daw);
  return l2s_check_launch();
}
