// What the weight-gradient files share: conv_wgrad.hip (the register-staged tiles, the dispatch and the C ABI), conv_wgrad_dma.hip (the LDS-DMA
// filter-row tile, variant 5) and conv_wgrad_dma1.hip (the LDS-DMA 256x256 tile of the 1x1 problems, variant 6).  Host-side declarations
// between the files first, then small device helpers; every kernel stays in its own file.
#pragma once
#include "common.h"
#include "../../include/lang2seg_hip.h"
#include <stddef.h>

typedef l2s_wgrad_prob wgp;

namespace l2s {
// stream-K plan of one launch: problem i owns the (tile, slice) units [unit0[i], unit0[i + 1]), S[i] slices per tile; U units in all
// mode 1 (XCD-lockstep, see conv_wgrad_dma.hip): T tiles per (problem, filter row) group, Ng groups, k1 workgroups per tile and XCD
struct wgrad_sk_plan { int n; long U; long unit0[L2S_WGRAD_MAX_GROUP + 1]; int S[L2S_WGRAD_MAX_GROUP]; int mode, T, Ng, k1, Q, r, m; };
bool wgrad_row3_dma_ok(const l2s_wgrad_prob& q);
long wgrad_row3_dma_tiles(int Cin, int Cout);
size_t wgrad_row3_dma_ws_bytes(int G);
int wgrad_row3_dma_launch(const l2s_wgrad_prob* tab_dev, const l2s_wgrad_prob* tab_host, int nprob, float* ws, size_t ws_bytes, int G, hipStream_t st);
// the LDS-DMA 256x256 tile of the large 1x1 problems (conv_wgrad_dma1.hip): one workgroup per tile
bool wgrad_1x1_dma_ok(const l2s_wgrad_prob& q);
long wgrad_1x1_dma_tiles(int Cin, int Cout);
int wgrad_1x1_dma_launch(const l2s_wgrad_prob* tab_dev, const l2s_wgrad_prob* tab_host, int nprob, hipStream_t st);

// tile list of a launch over a problem table: problem i owns tiles [tile0[i], tile0[i + 1]); tile0[n] = all of them
struct wgrad_tile_prefix { int n; int tile0[L2S_WGRAD_MAX_GROUP + 1]; };
}  // namespace l2s

namespace l2s_wgrad {

// fills pre from the host table, tiles(q) tiles for problem q; returns the total (the caller bounds it)
template <class F> long fill_tile_prefix(l2s::wgrad_tile_prefix& pre, const wgp* tab_host, int nprob, F tiles) {
  pre.n = nprob;
  long t = 0;
  for (int i = 0; i < nprob; ++i) { pre.tile0[i] = (int)t; t += tiles(tab_host[i]); }
  for (int i = nprob; i <= L2S_WGRAD_MAX_GROUP; ++i) pre.tile0[i] = (int)t;
  return t;
}

// One launch: the kernel's dynamic-LDS limit is raised to lds once (the static is the enclosing launcher instantiation's), then L2S_LAUNCH.
// A macro, not a function template that receives the kernel: l2s::last_kernel is the kernel argument of L2S_LAUNCH as it is spelled.
#define WGRAD_LAUNCH(kern, grid, block, lds, st, ...)                                                                                     \
  do {                                                                                                                                    \
    static bool attr_done = false;                                                                                                        \
    if (!attr_done) { (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds)); attr_done = true; } \
    L2S_LAUNCH(kern, grid, block, lds, st, __VA_ARGS__);                                                                                  \
  } while (0)

// ---- buffer resources and LDS-DMA ----
typedef int i32x4s __attribute__((ext_vector_type(4)));
constexpr unsigned OOR = 0x80000000u;   // an offset past every resource's range: the buffer's range check returns (or writes to LDS) zeros

// raw buffer resource over [base, base + bytes) (default: the whole 31-bit range), as the four dwords the DMA's inline asm takes
__device__ __forceinline__ i32x4s rsrc(const void* base, long bytes = 0x7FFFFFFF) {
  i32x4s r; r.x = (int)(uintptr_t)base; r.y = (int)((uintptr_t)base >> 32); r.z = (int)bytes; r.w = 0x00020000; return r;
}

// one request = 1 KiB = FOUR 256-byte pixel rows (16 lanes x 16 B each): the vector memory pipe of a CU takes ~16 cycles per wave
// instruction whatever its width - with one row per `buffer_load_dword ... lds` the 136 requests of a slice cost 0.87 us, more than
// its MFMAs (knock-outs: requests alone 128 us of the launch, MFMAs alone 101 us, and the two did not overlap).
// (Measured on the filter-row tile; in conv_wgrad_dma1.hip the same 1 KiB is two 512-byte rows, 32 lanes each.)
__device__ __forceinline__ void dma_1kib(const i32x4s& r, unsigned voff, unsigned lds_) {
  const unsigned lds = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_);   // (uniform; makes the "s" operand a scalar register even where hipcc kept the value in a VGPR)
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(r), "s"(lds) : "memory");
}

// the DMA is inline asm: hipcc's waitcnt pass neither sees nor drains it.  A wave's requests complete in order, PER of them per slice: wait
// until at most min(younger, KMAX) slices' requests of this wave are outstanding (the immediates are compile-time constants)
template <int PER, int KMAX = 3> __device__ __forceinline__ void wait_vm_keep(int younger) {
  if (KMAX >= 3 && younger >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * PER) : "memory");
  else if (KMAX >= 2 && younger >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * PER) : "memory");
  else if (KMAX >= 1 && younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void wg_barrier() { asm volatile("s_barrier" ::: "memory"); }
__device__ __forceinline__ void lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// one bf16 MFMA operand fragment out of LDS: two ds_read_b64_tr_b16 (a 4-pixel x 16-channel block per 16 lanes, transposed by the hardware),
// pixel rows q and q + 16 rows of `rowbytes`
__device__ __forceinline__ uint4 lds_frag(const char* q, int rowbytes) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(q));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(q + 16 * rowbytes));
  return __builtin_bit_cast(uint4, (s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
}

// ---- workgroup -> (problem, tile) ----
// XCD-aware order: workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8), each with its own L2; XCD x takes the x-th
// CONTIGUOUS eighth of the tile list, whose neighbours share an operand tile, instead of every XCD fetching every operand tile (operands
// far larger than one XCD's 4 MiB L2 are otherwise served at the fabric's ~33 GB/s per CU).  L: the workgroup's place in launch order;
// returns the problem, t = its tile there.
__device__ __forceinline__ int tile_of(const l2s::wgrad_tile_prefix& pre, int L, int& t) {
  const int G = pre.tile0[pre.n], x = L & 7, slot = L >> 3, q = G >> 3, r = G & 7;
  const int bid = x * q + min(x, r) + slot;
  int lo = 0, hi = pre.n;                                  // tile0[lo] <= bid < tile0[hi]
  while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (pre.tile0[mid] <= bid) lo = mid; else hi = mid; }
  t = bid - pre.tile0[lo];
  return lo;
}

// ---- the virtual pixel layout (image rows of width Wv, ohwv = OH * Wv pixels per image) ----
// virtual pixel (>= 0) -> (image, row, column)
__device__ __forceinline__ void pixel_split(int pix, int ohwv, int Wv, int& n, int& y, int& x) {
  n = pix / ohwv; const int rem = pix - n * ohwv; y = rem / Wv; x = rem - y * Wv;
}
// ... of an X row: a filter-row tile's X image starts one pixel early, and pixel -1 is a zero column
__device__ __forceinline__ void pixel_place(int pix, int ohwv, int Wv, int& n, int& y, int& x) {
  if (pix < 0) { n = 0; y = 0; x = -1; }
  else pixel_split(pix, ohwv, Wv, n, y, x);
}
// a slice of bkp pixels as a step in that layout: bkp = a * ohwv + b * Wv + c
__device__ __forceinline__ void slice_step(int bkp, int ohwv, int Wv, int& a, int& b, int& c) {
  a = bkp / ohwv; b = (bkp - a * ohwv) / Wv; c = bkp - a * ohwv - b * Wv;
}

// ---- dW (+)= tile ----
__device__ __forceinline__ float4 add4(float4 a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; return a; }
__device__ __forceinline__ float4 f4(const f32x4& a) { return make_float4(a[0], a[1], a[2], a[3]); }
__device__ __forceinline__ void dw_store(float4* q, float4 v, bool accumulate) {
  if (accumulate) v = add4(v, *q);
  *q = v;
}

}  // namespace l2s_wgrad
