/* lang2seg_hip.h — C ABI of liblang2seg_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the hot path of wenz116/lang2seg: every arithmetic op of
 * Network.train_step (pyutils/mask-faster-rcnn/lib/nets/network_cycle_res5_2.py:702-719) that the
 * reference delegates to cuDNN / THC / its own torch.utils.ffi extensions is one entry point here.
 * Conventions (mirroring the reference FFI in lib/nms/src/nms_cuda.c:17 and
 * lib/layer_utils/roi_pooling/src/roi_pooling_cuda.c:7,49, but re-entrant and stream-explicit):
 *   - plain pointers (DEVICE memory unless stated) + explicit sizes, no torch types;
 *   - caller-owned outputs and workspaces, no hidden allocation, no host sync, graph-capturable;
 *   - every call enqueues on `stream` and returns 0 (L2S_OK) or a nonzero error code, never aborts;
 *   - `dtype` selects the activation storage type: L2S_F32 (verification mode, exact-f32 MFMA) or
 *     L2S_BF16 (bf16 storage, fp32 accumulate).  Parameters, gradients, losses, box math: fp32.
 *   - activations are NHWC ([pixel][channel]); conv weights are [Cout][KH][KW][Cin].
 */
#ifndef LANG2SEG_HIP_H
#define LANG2SEG_HIP_H
#include <stdint.h>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
typedef struct ihipStream_t* hipStream_t;
#endif
#ifdef __cplusplus
extern "C" {
#endif

#define L2S_F32 0
#define L2S_BF16 1

int l2s_version(void);

/* ---------------------------------------------------------------- convolution / GEMM ------- */
/* replaces nn.Conv2d / F.conv2d / nn.Linear / nn.ConvTranspose2d(k2,s2) forward and data-gradient:
 * resnet_v1_cycle_res5_2.py:83-88,121,147,324-335; network_cycle_res5_2.py:236-251,279-301. */
#define L2S_CONV_RELU 1        /* y = max(y, 0) after bias/add */
#define L2S_CONV_OUT_F32 4     /* y is float regardless of dtype */
#define L2S_CONV_DECONV2X2 8   /* Cout = 4*Cq, n = (dy*2+dx)*Cq + co; pixel-shuffled 2x upsampled output */
#define L2S_CONV_SCATTER 16    /* output pixel (n, oy*out_stride, ox*out_stride) in an out_h x out_w grid */
#define L2S_ALGO_AUTO 0
#define L2S_ALGO_STAGED 1      /* register-staged tiles (ring / wave-specialised / software-pipelined kernels) */
#define L2S_ALGO_DMA 2         /* 256x128 tile, LDS-DMA fill (buffer_load ... lds), two wave groups alternating load / multiply */
#define L2S_ALGO_DMA_STAMPED 4 /* the same kernel with in-kernel clock stamps written to `ws` (tools/dma_stamps.py) */
#define L2S_ALGO_KSPLIT 5      /* 64x64 tile, LDS-DMA fill by four requester waves, four multiplier waves splitting each slice's K */
#define L2S_ALGO_KSPLIT_D3 6   /* the same with a ring of three LDS stages instead of four */
#define L2S_ALGO_PATCH 3       /* 3x3 / stride 1 / pad 1 on one map: 128 pixels x 32 or 64 channels per workgroup, input patch staged once for the nine taps */
#define L2S_ALGO_PDMA 7           /* the LDS-DMA tile as ONE persistent workgroup per CU walking its tiles, requests running ahead across tile boundaries (plain GEMMs) */
#define L2S_ALGO_DMA196 10         /* igemm_dma196_kernel: the 256 x 128 LDS-DMA pipeline on tiles of 196 rows (on request: 2-4 % faster alone, 1 % slower inside the step) */
#define L2S_ALGO_DMA256 9          /* igemm_dma256_kernel: 256x256 LDS-DMA tile for wide plain GEMMs (chosen automatically for them) */
#define L2S_ALGO_WS64_STAMPED 8  /* the 64x64 wave-specialised tile with clock stamps per workgroup in ws (tools/ws64_stamps.py) */
typedef struct {
  const void* x;      /* [n_img, IH, IW, ldx] activations (dtype) */
  const void* w;      /* [Cout][KH*KW*Cin] (dtype) */
  void* y;            /* [rows][ldy] (dtype, or float with OUT_F32) */
  const float* bias;  /* [Cout] or NULL (indexed by co for DECONV2X2) */
  const void* add;    /* [rows][ldadd] (dtype) added before relu/mask, or NULL */
  const void* ref;    /* [rows][ldref] (dtype): y = ref > 0 ? y : 0 (ReLU backward), or NULL */
  int n_img, IH, IW, Cin, OH, OW, Cout, KH, KW, stride, pad;
  int ldx, ldy, ldadd, ldref;
  int flags;
  int out_h, out_w, out_stride; /* SCATTER */
  int tile;                     /* 0 = auto, 64, 128, 224 or 256 (rows of the workgroup tile) */
  int split_k;                  /* K split over workgroups, partial tiles added in a fixed order by a second launch: 0 / 1 = off, n = force (needs ws) */
  int xcd_mode;                 /* tile order over the 8 XCDs: -1 = auto, 0 = M-chunks, 1 = N-chunks (speed only) */
  int algo;                     /* kernel family: 0 = auto; L2S_ALGO_* forces one (benchmarks / tests; same arithmetic, speed only) */
  float* ws;                    /* optional float workspace for split-K partial sums: split x rows x Cout floats (any contents; one per stream) */
  size_t ws_floats;             /* its size; the split is reduced until the slabs fit */
  int prio;                     /* 1: the kernel's waves raise their issue priority (s_setprio 3): launches of a latency-bound dependent chain that shares
                                   CUs with throughput-bound background work (the backbone's convolutions beside the weight-gradient stream) */
} l2s_conv_desc;
int l2s_conv_igemm(const l2s_conv_desc* d, int dtype, hipStream_t stream);
/* name of the kernel l2s_conv_igemm launches for this problem (reporting: bench.py's roofline object); static storage */
const char* l2s_conv_plan_name(const l2s_conv_desc* d, int dtype);
/* for tests and reports only: the kernel of the calling thread's latest launch, as the launch site names it (template arguments
 * included); static storage, NULL before the thread's first launch.  Nothing reads it to decide anything. */
const char* l2s_last_kernel(void);

/* weight gradient: dw[Cout][KH*KW*Cin] (float) += sum_pixels dy[p][co] * x(p,tap)[ci]
 * (cuDNN backward-filter behind autograd in the reference: resnet_v1_cycle_res5_2.py:83-88,324-335, network_cycle_res5_2.py:236-251,279-301).
 * No floating-point atomics: with split-K every workgroup stores its partial tile into its own slab of `ws` and a second launch on the
 * same stream adds the slabs to dw in a fixed order, so the result is bit-identical from run to run.  Without a workspace (or when it is
 * too small for two slabs) the pixels are not split.  The caller must not run two launches that accumulate into the SAME dw, or that
 * share a workspace, concurrently on different streams.  l2s_wgrad_ws_bytes: workspace the automatic split of this problem would use. */
typedef struct {
  const void* dy;  /* [n_img*OH*OW][lddy] (dtype) */
  const void* x;   /* [n_img, IH, IW, ldx] (dtype) */
  float* dw;
  int n_img, IH, IW, Cin, OH, OW, Cout, KH, KW, stride, pad;
  int lddy, ldx;
  int split_k;     /* 0 = auto */
  int tile;        /* 0 = auto, 64 or 128 (output-channel tile) */
  float* ws;       /* split-K slabs (device), may be NULL */
  size_t ws_bytes;
} l2s_wgrad_desc;
size_t l2s_wgrad_ws_bytes(const l2s_wgrad_desc* d, int dtype);

/* Deferred, grouped weight gradients: every weight gradient of a backward stage in ONE launch (nothing needs them before the optimiser
 * / the gradient all-reduce of that stage).  Each workgroup owns a whole output tile over all pixels: no split-K, no atomics, no partial
 * sums, bit-reproducible, and a few thousand workgroups fill the chip where a single small layer has ~100 tiles.  A tensor that is used
 * twice in the step (resnet.layer4 on the RoIs and on the whole map, network_cycle_res5_2.py:415-435) is one problem with two pixel
 * segments.  All problems of a launch use the same tile variant (l2s_wgrad_variant: 0 = 64x64 tile per tap, 1 = 128x128 per tap,
 * 2 = 64x64 x three taps of a 3x3 filter row, 3 = 128x64 x filter row); `table_dev` is the device copy of `table_host` and must stay
 * valid until the launch has run.  dw += gradient.  Problems with few output tiles and many pixels (layer2: 9375 pixels, 128 channels)
 * may still split their pixels (`split`): slabs in `ws`, no atomics either. */
#define L2S_WGRAD_MAX_GROUP 64
#define L2S_WGRAD_MAX_SEG 2
typedef struct {
  const void* dy[L2S_WGRAD_MAX_SEG];   /* [n_img*OH*OW][lddy] (dtype) per segment */
  const void* x[L2S_WGRAD_MAX_SEG];    /* [n_img, IH, IW, ldx] (dtype) per segment */
  int n_img[L2S_WGRAD_MAX_SEG], IH[L2S_WGRAD_MAX_SEG], IW[L2S_WGRAD_MAX_SEG], OH[L2S_WGRAD_MAX_SEG], OW[L2S_WGRAD_MAX_SEG];
  int lddy[L2S_WGRAD_MAX_SEG], ldx[L2S_WGRAD_MAX_SEG];
  float* dw;                           /* [Cout][KH*KW*Cin] */
  int nseg, Cin, Cout, KH, KW, stride, pad;
  int split;                           /* <= 1: whole tiles; n: the pixels of every segment are cut into n ranges whose partial tiles go to */
  long ws_off;                         /*       n slabs at float offset ws_off of the launch's workspace, summed in order by a second launch */
  int flags;                           /* 1: dw = gradient (the tensor's first contribution of the step: nothing is read, nothing had to be cleared); */
  int reserved;                        /*    0: dw += gradient */
} l2s_wgrad_prob;
int l2s_wgrad_variant(int Cin, int Cout, int KH, int KW, int stride, int pad, int same_hw, long M, int tile);
long l2s_wgrad_tiles(int variant, int Cin, int Cout, int KH, int KW);
/* variant 5 (bf16, 3x3 / stride 1 / pad 1, >= 8192 pixels, channels multiples of 128): the LDS-DMA filter-row tile, balanced stream-K style
 * over 128 workgroups; its slabs need l2s_wgrad_grouped_ws_bytes(5) of workspace. */
size_t l2s_wgrad_grouped_ws_bytes(int variant);
int l2s_conv_wgrad_grouped(const l2s_wgrad_prob* table_dev, const l2s_wgrad_prob* table_host, int nprob, int variant, int dtype,
                           float* ws, size_t ws_bytes, hipStream_t stream);
int l2s_conv_wgrad(const l2s_wgrad_desc* d, int dtype, hipStream_t stream);

/* shadow weights: dst(dtype)[Cout][taps][Cin] = scale[co] * src[Cout][taps][Cin]  (scale may be NULL) */
int l2s_weight_cast(const float* src, const float* scale, void* dst, int Cout, int taps, int Cin, int dtype, hipStream_t s);
/* data-gradient layout: dst(dtype)[Cin][taps][Cout], tap order reversed (180-degree flip), * scale[co] */
int l2s_weight_transpose(const float* src, const float* scale, void* dst, int Cout, int taps, int Cin, int dtype, hipStream_t s);
/* all data-gradient copies of one step in one launch: table (DEVICE memory) of n descriptors; total_tiles = sum over the descriptors of
 * ceil(Cin / 64) * ceil(Cout / 64) * taps (the launch walks one flat tile index) */
typedef struct { const float* src; const float* scale; void* dst; int Cout, taps, Cin;
                 int force_f32; /* bit 0: dst is f32 whatever the launch's dtype; bit 1: src points at bf16 values (the shadow: scale = NULL) */ } l2s_transpose_desc;
int l2s_weight_transpose_batched(const l2s_transpose_desc* table_dev, int n, int total_tiles, int dtype, hipStream_t s);
/* column sums: out[c] += sum_r a[r][c] (bias gradients), no atomics; ws (nullable, 32*cols floats): partial sums of the row ranges a tall
 * matrix is cut into, added in order by a second launch */
int l2s_colsum(const void* a, int rows, int cols, int lda, float* out, float* ws, long ws_floats, int dtype, hipStream_t s);

/* stem: conv 7x7 s2 p3 (3->64) + frozen-BN affine + ReLU (RES:121-124), input float NHWC; then maxpool k3 s2 p1 (RES:126) */
int l2s_stem_conv(const float* img, const float* w /*[64][7][7][3]*/, const float* scale, const float* bias,
                  void* y, int H, int W, int OH, int OW, int dtype, hipStream_t s);
/* bf16 mode: the same stem AND the pooling behind it in one launch on the matrix cores (stem_mfma.hip): image as two bf16 terms (16
 * significant bits), weights rounded to bf16 in the fragment order l2s_stem_pack() writes (l2s_stem_pack_bytes() bytes; repack whenever
 * conv1's weights change), f32 accumulation / affine / ReLU, one rounding to bf16, pooled output y [PH*PW][64] bf16. */
size_t l2s_stem_pack_bytes(void);
int l2s_stem_pack(const float* w /*[64][7][7][3]*/, void* pack, hipStream_t s);
int l2s_stem_pool_bf16(const float* img, const void* pack, const float* scale, const float* bias, void* y, int H, int W,
                       int OH, int OW, int PH, int PW, hipStream_t s);
/* VGG16 variant (nets/vgg16.py:43-54, network_vgg.py:139-143): conv1_1 (3 -> 64, 3x3, pad 1, bias, ReLU) on the fp32 NHWC image with
 * weights [64][3][3][3]; 2x2 / stride-2 max pooling (floor mode) forward / backward over n_img NHWC maps [IH][IW][C] (also the
 * 14x14 -> 7x7 pool behind the crop-pool).  relu_out != 0: x is a ReLU output, dx is the gradient of its pre-activation. */
/* out = x * mask (fp32 scaled dropout mask), zero where relu_ref <= 0 (nullable): dropout forward / backward of fc6 and fc7 */
int l2s_scale_mask(const void* x, const float* mask, const void* relu_ref, void* out, long n, int dtype, hipStream_t s);
int l2s_conv3x3_c3(const float* img, const float* w, const float* bias, void* y, int H, int W, int dtype, hipStream_t s);
int l2s_maxpool2x2_fwd(const void* x, void* y, int n_img, int IH, int IW, int C, int dtype, hipStream_t s);
int l2s_maxpool2x2_bwd(const void* dy, const void* x, void* dx, int n_img, int IH, int IW, int C, int relu_out, int dtype, hipStream_t s);
int l2s_maxpool3x3s2(const void* x, void* y, int IH, int IW, int C, int OH, int OW, int dtype, hipStream_t s);

/* ---------------------------------------------------------------- pooling / elementwise ---- */
int l2s_fill_f32(float* p, float v, long n, hipStream_t s);
int l2s_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, hipStream_t s);
int l2s_mul_f32(const float* a, const float* b, float* out, long n, hipStream_t s);
int l2s_add_f32(const float* a, const float* b, float* out, long n, hipStream_t s);   /* out = a + b (out may alias a or b) */
/* dst(dtype) = a(dtype) + b(dtype) + c(float)   (any of b, c may be NULL) */
int l2s_add3(const void* a, const void* b, const float* c, void* dst, long n, int dtype, hipStream_t s);
/* spatial mean over hw pixels per image: y[n][c] = mean_p x[n][p][c]  (NET:278) and its backward */
int l2s_avgpool_fwd(const void* x, void* y, int n_img, int hw, int C, int dtype, hipStream_t s);
int l2s_avgpool_bwd(const void* dy, void* dx, const void* addend, const void* relu_ref, int n_img, int hw, int C, int dtype, hipStream_t s);
/* adaptive_avg_pool2d (H,W)->(OH,OW), bins [floor(i*H/OH), ceil((i+1)*H/OH)) (NET:419,432); optional {0,1} pixel mask */
int l2s_adaptive_pool_fwd(const void* x, const float* pixmask, void* y, int H, int W, int C, int OH, int OW, int ldy, int dtype, hipStream_t s);
/* dx[p][c] (+)= sum over bins containing p of dy_all[bin][c]/cnt + pixmask[p]*dy_mask[bin][c]/cnt ; then ReLU-masked by relu_ref */
int l2s_adaptive_pool_bwd(const void* dy, int lddy, int off_all, int off_mask, const float* pixmask, void* dx,
                          const void* relu_ref, int H, int W, int C, int OH, int OW, int dtype, hipStream_t s);
/* gt mask (uint8 HxW) -> adaptive avg pool to (h,w) -> >= 0.5 (NET:424-428) */
int l2s_mask_downsample(const uint8_t* mask, float* out, int H, int W, int h, int w, hipStream_t s);
/* counter-based hash RNG: the step counter lives in DEVICE memory (so a captured hipGraph replays with fresh randomness);
 * l2s_counter_inc bumps it once per step; `salt` separates the call sites */
int l2s_counter_inc(uint64_t* counter_dev, hipStream_t s);
/* diagnostics (tools/step_timeline.py): one-thread launch that stores the device's constant 100 MHz clock when the stream reaches it */
int l2s_stamp(uint64_t* slot_dev, hipStream_t s);
/* dropout mask, entries 0 or 1/(1-p) */
int l2s_dropout_mask(float* mask, long n, float p, const uint64_t* seed_dev, uint64_t salt, hipStream_t s);

/* ---------------------------------------------------------------- RoI path ------------------ */
/* RPN pair-softmax + box decode + clip (NET:242-246, proposal_layer.py:42-46, bbox_transform.py:36-80).
 * heads: float [HW][ldh] with columns [0,2A) = cls scores (bg A, fg A), [2A,6A) = bbox deltas.
 * outputs: prob [HW][2A] float, boxes [HW*A][4] float, scores [HW*A] float (fg prob) */
int l2s_rpn_decode(const float* heads, int ldh, const float* base_anchors /*[A][4]*/, int H, int W, int A, int feat_stride,
                   float im_h, float im_w, float* prob, float* boxes, float* scores, hipStream_t s);
/* descending stable sort (ties: lower index first), emits the top-k boxes/scores in order.
 * ws: int32 workspace of l2s_sort_ws_ints(n); sorted_boxes [k][4], sorted_scores [k], sorted_idx [k] (int32) */
long l2s_sort_ws_ints(int n);
int l2s_sort_topk(const float* scores, const float* boxes, int n, int k, int* ws, float* sorted_boxes,
                  float* sorted_scores, int* sorted_idx, hipStream_t s);
/* greedy NMS over score-sorted boxes (replaces gpu_nms / cpu_nms, nms_cuda.c:17, nms.c:4).
 * cmp_mode 0: suppress when IoU >= thresh (cpu_nms, nms.c:59); 1: IoU > thresh (nms_kernel.cu:63).
 * mask_ws: l2s_nms_workspace_bytes(n) bytes (8-byte aligned; the bit mask of ONE 4096-box stage - the boxes are scanned in stages, a
 * stage's mask is that of its own boxes and what earlier stages kept enters as one OR word per 64 boxes - plus those words: 2 MB at
 * n = 12000, where the reference's mask is 18 MB).  max_keep >= 1.  keep_out[max_keep] int32 (indices into the sorted list),
 * num_out[1] int32 — both DEVICE memory (the 18 MB D2H + host loop of nms_cuda.c:47-58 is gone); the stages after the first return
 * at once when keep_out is already full.  num_out[0] = -1: a wave of the scan gave up a bounded wait (not reachable while the scan's
 * workgroup runs as a whole); the remaining stages return at once and l2s_gather_rois emits an empty list. */
size_t l2s_nms_workspace_bytes(int n);
int l2s_nms(const float* sorted_boxes, int n, float thresh, int cmp_mode, int max_keep, uint64_t* mask_ws,
            int* keep_out, int* num_out, hipStream_t s);
/* gather kept proposals: rois[max_keep][5] = [0, box], roi_scores[max_keep]; rows >= *num_out are zero */
int l2s_gather_rois(const float* sorted_boxes, const float* sorted_scores, const int* keep, const int* num, int max_keep,
                    float* rois, float* roi_scores, hipStream_t s);
/* uint32 sampling priority keys from the same counter hash */
int l2s_random_keys(uint32_t* keys, long n, const uint64_t* seed_dev, uint64_t salt, hipStream_t s);

/* anchor_target_layer.py:19-153 on device.  gt float [n_gt][5]; keys uint32 [HWA] (smallest keys are disabled first).
 * outputs: labels int32 [A*H*W] in the (a,h,w) order of ATL:133-134 (-1,0,1), targets/inside/outside float [HW][4A].
 * ws: int32/float scratch of l2s_anchor_target_ws_ints(HWA) ints. */
long l2s_anchor_target_ws_ints(int hwa);
int l2s_anchor_target(const float* gt, int n_gt, const float* base_anchors, int H, int W, int A, int feat_stride,
                      float im_h, float im_w, const uint32_t* fg_keys, const uint32_t* bg_keys,
                      float neg_ov, float pos_ov, int batch, float fg_frac,
                      int* labels, float* targets, float* inside_w, float* outside_w, int* ws, hipStream_t s);

/* proposal_target_layer.py:22-204 on device (torch-0.3 ByteTensor semantics at :146).
 * rois [n_max][5], n_rois device int; gt [n_gt][5]; gt_masks uint8 [n_gt][im_h][im_w].
 * outputs: out_rois [R][5], labels int32 [R], bbox_targets/inside/outside [R][4*ncls], mask_targets float
 * [mask_slots][ms*ms], counts int32[4] = {num_fg (capped at mask_slots), n_fg_cand, n_bg_cand, appended_gt}.  ws: int32 [4*(n_max+n_gt)+16].
 * fg_max = round(FG_FRACTION * R) caps the sampled foreground when background candidates exist; without any (PTL:155-158) all R sampled
 * RoIs are foreground, and the mask targets cover the first mask_slots (fg_max <= mask_slots <= R) of them. */
int l2s_proposal_target(const float* rois, const float* roi_scores, const int* n_rois, int n_max, const float* gt, int n_gt,
                        const uint8_t* gt_masks, int im_h, int im_w, const uint32_t* fg_keys, const uint32_t* bg_keys,
                        const uint32_t* bg_rand, int R, int fg_max, int mask_slots, float fg_thresh, float bg_hi, float bg_lo,
                        const float* means4, const float* stds4, const float* inw4, int ncls, int ms,
                        float* out_rois, int* labels, float* bbox_targets, float* bbox_inside, float* bbox_outside,
                        float* mask_targets, int* counts, int* ws, hipStream_t s);

/* RoIAlign fused into the first bottleneck of the RoI head (bf16 activations): crop-and-resize (network_cycle_res5_2.py:107-149) feeding
 * resnet.layer4[0].conv1 (+ frozen-BN shift + ReLU) and resnet.layer4[0].downsample (+ shift), resnet_v1_cycle_res5_2.py:271-273, in ONE
 * launch, one workgroup per RoI.  `pooled` receives the P x P x C crop exactly as l2s_roialign_fwd writes it (the weight gradients and the
 * backward pass read it; the forward pass does not).  Requirements: P*P <= 64, C % 128 == 0, P*P*C*2 + 4 KiB <= 160 KiB of LDS,
 * N1 % 128 == 0, N2 % 128 == 0; L2S_EINVAL otherwise (callers fall back to l2s_roialign_fwd + two l2s_conv_igemm). */
typedef struct {
  const void* feat;        /* [H*W][C] bf16 */
  const float* rois;       /* [R][5] (batch index, x1, y1, x2, y2) in image pixels */
  const void* w1;          /* [N1][C] bf16 (BN scale folded) */
  const float* b1;         /* [N1] or NULL */
  const void* w2;          /* [N2][C] bf16 */
  const float* b2;         /* [N2] or NULL */
  void* pooled;            /* [R*P*P][C] bf16 */
  void* y1;                /* [R*P*P][N1] bf16 = relu(pooled . w1^T + b1) */
  void* y2;                /* [R*P*P][N2] bf16 = pooled . w2^T + b2 */
  int H, W, C, R, P, N1, N2;
  float spatial_scale;
  int debug;               /* 0; tools/roi_block0_bench.py: 1 = no products, 2 = no weight loads behind the prologue, 4 = no stores */
} l2s_roi_block0_desc;
int l2s_roialign_block0_fwd(const l2s_roi_block0_desc* d, hipStream_t stream);
/* crop-and-resize RoIAlign = affine_grid + grid_sample, align_corners=True, zero padding (NET:107-149) */
int l2s_roialign_fwd(const void* feat, int H, int W, int C, const float* rois, int R, int P, float spatial_scale,
                     void* out, int dtype, hipStream_t s);
/* d(feat) float [H*W][C] of dout [R*P*P][C].  dfeat is WRITTEN (round 5: it need not arrive cleared): a gather per map pixel in a fixed
 * summation order, no atomics, when C % 4 == 0 and P <= 32; otherwise cleared here and scattered into with atomics */
int l2s_roialign_bwd(const void* dout, int H, int W, int C, const float* rois, int R, int P, float spatial_scale,
                     float* dfeat, int dtype, hipStream_t s);

/* _crop_pool_layer_align (NET:151-182, selected by cfg.POOLING_ALIGN at NET:569-570,610-611): the same sampler with the affine
 * grid computed from the RoI in image pixels over the image size (im_info) instead of roi/16 over the map size */
int l2s_cropalign_fwd(const void* feat, int H, int W, int C, const float* rois, int R, int P, float im_h, float im_w,
                      void* out, int dtype, hipStream_t s);
/* d(feat) is WRITTEN, like l2s_roialign_bwd's: a caller that accumulates into an existing gradient adds the result itself */
int l2s_cropalign_bwd(const void* dout, int H, int W, int C, const float* rois, int R, int P, float im_h, float im_w,
                      float* dfeat, int dtype, hipStream_t s);

/* ---------------------------------------------------------------- losses -------------------- */
/* loss slots in the float loss[8] buffer */
#define L2S_LOSS_RPN_CLS 0
#define L2S_LOSS_RPN_BOX 1
#define L2S_LOSS_CLS 2
#define L2S_LOSS_BOX 3
#define L2S_LOSS_MASK 4
#define L2S_LOSS_CAP 5
#define L2S_LOSS_TOTAL 6
#define L2S_LOSS_RESPONSE 7   /* network_7f_response.py:411-419 / network_cycle_response.py:415-423; 0 in the other variants */
/* RPN CE over anchors with label != -1 (NET:377-382) + smooth-L1 sigma=3 (NET:385-390).
 * heads as in l2s_rpn_decode; labels in (a,h,w) order.  dheads(dtype) [HW][ldd] receives d(loss)/d(heads)*gscale. */
/* RoI max pooling, POOLING_MODE == 'pool' (layer_utils/roi_pooling/roi_pool.py:19-50 -> src/cuda/roi_pooling_kernel.cu:15-70,104-180;
 * the reference's second native FFI besides NMS).  feat NHWC [H*W][C]; out [R*P*P][C]; argmax [R*P*P][C] int32 = h*W + w of the
 * maximum (-1: empty bin); backward adds dout into dfeat [H*W][C] f32 through the recorded argmax (dfeat is not cleared). */
int l2s_roipool_fwd(const void* feat, int H, int W, int C, const float* rois, int R, int P, float spatial_scale, void* out, int* argmax,
                    int dtype, hipStream_t s);
int l2s_roipool_bwd(const void* dout, const int* argmax, int R, int P, int C, float* dfeat, int dtype, hipStream_t s);
int l2s_rpn_loss(const float* heads, int ldh, const int* labels, const float* targets, const float* inside_w,
                 const float* outside_w, int H, int W, int A, float sigma, float gscale, float* loss /* += */, void* dheads, int ldd,
                 int dtype, const int* count_dev /* #labels != -1 (l2s_anchor_target_count) or NULL */, int* count_ws /* 1 int, used when count_dev is NULL */,
                 hipStream_t s);
/* device pointer to the number of sampled anchors inside an l2s_anchor_target workspace */
const int* l2s_anchor_target_count(const int* ws);
/* RCNN CE mean over R (NET:393-395) + smooth-L1 sigma=1 (NET:398-402). heads float [R][ldh]: [0,ncls) cls, [ncls,5ncls) bbox */
int l2s_rcnn_loss(const float* heads, int ldh, const int* labels, const float* bbox_targets, const float* inside_w,
                  const float* outside_w, int R, int ncls, float gscale, float* loss, void* dheads, int ldd, int dtype, hipStream_t s);
/* mask BCE-with-logits on the class channel of the first num_fg rois (NET:405-413). score float [fg_max*ms2][ldsc] */
int l2s_mask_loss(const float* score, int ldsc, const int* labels, const float* mask_targets, const int* num_fg, int fg_max,
                  int ms2, float gscale, float* loss, float* dscore /*[fg_max*ms2]*/, hipStream_t s);
/* total = cls + box + rpn_cls + rpn_box + mask + w*cap (NET:448) */
/* response BCE loss of the *_response variants: target = GT mask [mask_h][mask_w] u8 {0,1} resized PIL-NEAREST to [H][W];
 * loss[L2S_LOSS_RESPONSE] += mean BCE; dresp[HW] = gscale * d loss / d response */
int l2s_response_loss(const float* resp, const uint8_t* gt_mask, int mask_h, int mask_w, int H, int W, float gscale, float* loss,
                      float* dresp, hipStream_t s);
/* TEST mode (NET:277-307, 650-658; test_image NET:684-699): heads [R][ldh] = (cls scores | box deltas) ->
 * cls_prob [R][ncls] (softmax), bbox_pred [R][4 ncls] de-normalised with TRAIN.BBOX_NORMALIZE_STDS / MEANS (4 floats each) */
int l2s_rcnn_predict(const float* heads, int ldh, int R, int ncls, const float* stds4, const float* means4, float* cls_prob,
                     float* bbox_pred, hipStream_t s);
/* mask probabilities: score [n_elem][ldsc] (n_elem = n_roi * ms2 mask pixels); labels == NULL -> out [n_elem][ncls] = sigmoid(score)
 * (NET:292-307); labels [n_roi] -> out [n_elem] = sigmoid of the labelled class only (NET:620-624) */
int l2s_mask_prob(const float* score, int ldsc, int ncls, const int* labels, int ms2, long n_elem, float* out, hipStream_t s);
int l2s_total_loss(float* loss, float cap_w, hipStream_t s);
/* mask_pred_net backward (only the label channel carries gradient): dx(dtype)[fg_max*ms2][C] = dscore[p]*W[label][:],
 * dW[label][:] += sum dscore[p]*x[p][:], db[label] += sum dscore[p]; ws: l2s_maskpred_ws_floats(fg_max, C) floats of per-(RoI, pixel chunk) partial sums
 * (added in order by a second launch: no atomics) */
long l2s_maskpred_ws_floats(int fg_max, int C);
int l2s_maskpred_bwd(const float* dscore, const int* labels, const int* num_fg, int fg_max, int ms2, int C,
                     const float* w /*[ncls][C]*/, const void* x, const void* relu_ref, void* dx, float* dw, float* db, float* ws, int dtype,
                     hipStream_t s);
/* its two launches separately: l2s_maskpred_bwd_dx = dx and the partial sums into ws; l2s_maskpred_bwd_reduce = dW / db from ws (may run on another
 * stream behind it: nothing of the data-gradient chain reads dW) */
int l2s_maskpred_bwd_dx(const float* dscore, const int* labels, const int* num_fg, int fg_max, int ms2, int C, const float* w,
                        const void* x, const void* relu_ref, void* dx, float* ws, int dtype, hipStream_t s);
int l2s_maskpred_bwd_reduce(const float* ws, const int* labels, const int* num_fg, int fg_max, int C, float* dw, float* db, hipStream_t s);

/* ---------------------------------------------------------------- language side ------------- */
/* small-M linear layers, fp32: y[m][n] = act(sum_k x[m][k] w[n][k] + b[n] (+ y_in)) ; act 0 none, 1 relu, 2 tanh */
int l2s_linear_fwd(const float* x, int ldx, const float* w, int ldw, const float* b, float* y, int ldy, int M, int N, int K, int act,
                   int accumulate, hipStream_t s);
/* dx[m][k] (+)= (sum_n dy[m][n] w[n][k]) (* mul[m][k], same leading dimension as dx; may be NULL) from the weight as stored.
 * Row batches split the contraction over workgroups when `ws` (>= l2s_linear_bwd_x_ws_floats floats) is given: partial sums in ws,
 * added in a fixed order by a second launch (no atomics); without ws one workgroup per 64 output columns walks all of n. */
long l2s_linear_bwd_x_ws_floats(int M, int N, int K);
int l2s_linear_bwd_x(const float* dy, int lddy, const float* w, float* dx, int lddx, int M, int N, int K, int accumulate,
                     const float* mul, float* ws, long ws_floats, hipStream_t s);
/* dw[n][k] += sum_m dy[m][n] x[m][k]; db[n] += sum_m dy[m][n] */
int l2s_linear_bwd_w(const float* dy, int lddy, const float* x, int ldx, float* dw, float* db, int M, int N, int K, hipStream_t s);
/* activation backward in place: dy *= act'(y)  (act 1 relu, 2 tanh) */
int l2s_act_bwd(float* dy, const float* y, long n, int act, hipStream_t s);
/* x *= mul (mul may be NULL); x = 0 where !(relu_ref > 0); out = x cast to out_dtype: dropout mask + ReLU backward + cast in one launch */
int l2s_mask_relu_cast(float* x, const float* mul, const float* relu_ref, void* out, int out_dtype, long n, hipStream_t s);
/* embedding gather out[t][:] = table[ids[t]][:] * (mask ? mask[t][:] : 1), optional relu; and scatter-add backward */
int l2s_embed_fwd(const float* table, const int64_t* ids, const float* mask, float* out, int T, int D, int relu, hipStream_t s);
int l2s_embed_bwd(const float* dout, const float* out, const int64_t* ids, const float* mask, float* dtable, int T, int D, int relu, hipStream_t s);
/* nn.LSTM cell (gate order i,f,g,o; lang_encoder.py:21-24): gates[4H] pre-activations (already x-proj + h-proj + biases) */
/* Fused bi-LSTM time step (lang_encoder.py:62; nn.LSTM gate order i,f,g,o), one launch for up to two directions.
 * forward : gates_out[4H] = gates_in[4H] (x W_ih^T + b_ih, precomputed) + W_hh h_prev + b_hh; cell update -> c, h, act[4H] (gate activations)
 * backward: dh = w_hh_T[H][4H] . dgates_next (NULL at the first step) + dh_ext (NULL or the gradient of the final hidden state);
 *           then the cell backward of this step: dgates[4H], dc_prev[H] */
typedef struct { const float* w_hh; const float* b_hh; const float* gates_in; const float* h_prev; const float* c_prev;
                 float* c; float* h; float* act; float* gates_out; } l2s_lstm_fwd_dir;
typedef struct { const float* w_hh_T; const float* dgates_next; const float* dh_ext; const float* dc_in; const float* act;
                 const float* c_prev; const float* c; float* dgates; float* dc_prev; } l2s_lstm_bwd_dir;
int l2s_lstm_step_fwd(const l2s_lstm_fwd_dir* dirs, int ndir, int Hh, hipStream_t s);
int l2s_lstm_step_bwd(const l2s_lstm_bwd_dir* dirs, int ndir, int Hh, hipStream_t s);
int l2s_lstm_cell_fwd(const float* gates, const float* c_prev, float* c, float* h, float* act /*[4H] saved*/, int Hh, hipStream_t s);
int l2s_lstm_cell_bwd(const float* dh, const float* dc_in, const float* act, const float* c_prev, const float* c,
                      float* dgates, float* dc_prev, int Hh, hipStream_t s);
/* Fused GRU time step (nn.GRU, gate rows r,z,n; lang_encoder.py:21-24 with rnn_type 'gru'), one launch for up to two directions.
 * forward : a = W_hh h_prev + b_hh; r = sigmoid(gi_r + a_r), z = sigmoid(gi_z + a_z), n = tanh(gi_n + r a_n), h = (1 - z) n + z h_prev
 *           with gates_in[3H] = x W_ih^T + b_ih (precomputed); stores h and act[4H] = r, z, n, a_n
 * backward: dh = w_hh_T[H][3H] . dgh_next (NULL at the first processed step) + dh_ext (NULL or [H], any step) + dh_carry_in (NULL or [H]);
 *           dgi[3H] = (da_r, da_z, da_n) is the gradient of gates_in (feeds W_ih, b_ih, dx), dgh[3H] = (da_r, da_z, da_n r) the gradient
 *           of a (feeds W_hh, b_hh and the next step's product), dh_carry_out[H] = dh z the direct path into h_prev (ping-ponged by the host)
 * H % 4 != 0 or ndir outside {1, 2}: error code, nothing launched (the same for the l2s_rnn_step_* pair). */
typedef struct { const float* w_hh; const float* b_hh; const float* gates_in; const float* h_prev; float* h; float* act; } l2s_gru_fwd_dir;
typedef struct { const float* w_hh_T; const float* dgh_next; const float* dh_ext; const float* dh_carry_in; const float* act;
                 const float* h_prev; float* dgi; float* dgh; float* dh_carry_out; } l2s_gru_bwd_dir;
int l2s_gru_step_fwd(const l2s_gru_fwd_dir* dirs, int ndir, int Hh, hipStream_t s);
int l2s_gru_step_bwd(const l2s_gru_bwd_dir* dirs, int ndir, int Hh, hipStream_t s);
/* Fused Elman time step (nn.RNN, tanh; rnn_type 'rnn').
 * forward : h = tanh(gates_in[H] + W_hh h_prev + b_hh); h is its own saved activation
 * backward: dh = w_hh_T[H][H] . dg_next (NULL at the first processed step) + dh_ext (NULL or [H]); dg[H] = dh (1 - h h) */
typedef struct { const float* w_hh; const float* b_hh; const float* gates_in; const float* h_prev; float* h; } l2s_rnn_fwd_dir;
typedef struct { const float* w_hh_T; const float* dg_next; const float* dh_ext; const float* h; float* dg; } l2s_rnn_bwd_dir;
int l2s_rnn_step_fwd(const l2s_rnn_fwd_dir* dirs, int ndir, int Hh, hipStream_t s);
int l2s_rnn_step_bwd(const l2s_rnn_bwd_dir* dirs, int ndir, int Hh, hipStream_t s);
/* Stacked layers (any cell).  forward: out[T][ndir H], row t = [h0[t][:] | h1[t][:]] (* mask[T][ndir H], NULL: none) - the next layer's input;
 * h0 / h1 are [T][H] (h1 unused when ndir == 1).  backward: d0[t][:] / d1[t][:] = the halves of dx[t][:] (* mask) - the per-step dh_ext of
 * the layer below; add0 / add1 (NULL or [H]) are added to the row each direction processes last (d0: T - 1, d1: 0): the layer's part of
 * the gradient of `hidden`. */
int l2s_rnn_concat_fwd(const float* h0, const float* h1, const float* mask, float* out, int T, int Hh, int ndir, hipStream_t s);
int l2s_rnn_concat_bwd(const float* dx, const float* mask, const float* add0, const float* add1, float* d0, float* d1, int T, int Hh,
                       int ndir, hipStream_t s);
/* Per-token steps of the top-down attention captioner (AttModel.py:370-395; csrc/caption_step.hip): nn.LSTMCell arithmetic, gate rows
 * i, f, g, o, one launch per cell and token, one wave per hidden unit.
 * A segment is (vector x[n], matrix block w with leading dimension ld); n = 0: unused.
 * forward : gates[4R] = pre + add0 + add1 (each NULL or [4R]) + sum_k W_k x_k with W_k = rows [4R] x columns [n_k] of a wider matrix
 *           (seg[k].w points at the block's first column); i, f, o = sigmoid, g = tanh; c = f c_prev + i g; h = o tanh(c);
 *           stores h[R], c[R] and act[4R] = i, f, g, o.
 * backward: dh[R] = add0 + add1 (each NULL or [R]) + sum_k T_k v_k with T_k = rows [R] x columns [n_k] of a TRANSPOSED copy;
 *           dgates[4R] (gradient of the pre-activations) and dc_prev[R] from dc_in (NULL or [R]), act, c_prev, c.
 * R % 4 != 0, R < 4 or ld < n: error code, nothing launched.  Segments that are not 16-byte aligned take a scalar loop. */
typedef struct { const float* x; const float* w; int ld; int n; } l2s_topdown_seg;
typedef struct { const float* pre; const float* add0; const float* add1; l2s_topdown_seg seg[2]; const float* c_prev; float* c; float* h;
                 float* act; } l2s_topdown_fwd;
typedef struct { l2s_topdown_seg seg[3]; const float* add0; const float* add1; const float* dc_in; const float* act; const float* c_prev;
                 const float* c; float* dgates; float* dc_prev; } l2s_topdown_bwd;
int l2s_topdown_cell_fwd(const l2s_topdown_fwd* a, int R, hipStream_t s);
int l2s_topdown_cell_bwd(const l2s_topdown_bwd* a, int R, hipStream_t s);
/* second half of the attention (AttModel.py:419-421) for a feature width R that need not equal att_hid_size: weight[L] = softmax(dots[L]),
 * att_res[R] = sum_l weight[l] att[l][:]; L <= 256.  (l2s_cap_att_dots_fwd is the first half.) */
int l2s_cap_att_apply_fwd(const float* att /*[L][R]*/, const float* dots, int L, int R, float* weight, float* att_res, hipStream_t s);
/* l2s_cap_attention_bwd_step2 with the sum over the locations in its well-conditioned form: datt_h[d] = -aw[d] sum_l ddot[l] (tanh^2[l][d] - m[d]),
 * m[d] = sum_l weight[l] tanh^2[l][d]; equal to aw[d] sum_l ddot[l] (1 - tanh^2) because sum_l ddot[l] = 0, without that sum's rounding error */
int l2s_cap_att_bwd_step_centered(const float* dweight, const float* tanh_ws, const float* weight, const float* aw, int L, int D, float* ddot,
                                  float* datt_h, hipStream_t s);
/* dst[r][0..cols) = src[r][0..cols) with leading dimensions ldd / lds; lds = 0 repeats one source row */
int l2s_pack_rows(float* dst, int ldd, const float* src, int lds, int rows, int cols, hipStream_t s);
/* Adaptive-attention captioners (csrc/adaatt_step.hip; AttModel.py:211-368).  G = 4 (adaatt) or 5 (adaattmo: two transform rows, their max).
 * Cell, one token: sums[q R + j] = pre + fcrow + w_hh[q R + j] . h_prev + b_hh (q < G; row blocks in, forget, out, transform) and
 * n5[j] = pre[G R + j] + fcrow[G R + j] + w_r[j] . h_prev + b_r[j]; pre / fcrow are [(G+1) R].  Writes c, h, fake = sigmoid(n5) tanh(c) and
 * save[7 R] (in, forget, out, transform, selector, tanh(c), sigmoid(n5)).
 * backward: dh = dh_ext + t_hh[j] . dsn[0 .. G R) + t_r[j] . dsn[G R ..) with t_hh [R][ld_thh] / t_r [R][ld_tr] transposed copies and dsn the
 * ds of token i + 1 (NULL at the last token); writes ds[(G+1) R] = d(sums | n5) and dc_prev.  dfake / dc_in / dh_ext may be NULL.
 * R % 4 != 0, R < 4, G not 4 or 5, a leading dimension shorter than its rows: error code, nothing launched. */
typedef struct { const float* pre; const float* fcrow; const float* w_hh; const float* b_hh; const float* w_r; const float* b_r; int ld_hh; int ld_r;
                 const float* h_prev; const float* c_prev; float* c; float* h; float* fake; float* save; } l2s_adaatt_fwd;
typedef struct { const float* dsn; const float* t_hh; const float* t_r; int ld_thh; int ld_tr; const float* dh_ext; const float* dfake;
                 const float* dc_in; const float* save; const float* c_prev; float* ds; float* dc_prev; } l2s_adaatt_bwd;
int l2s_adaatt_cell_fwd(const l2s_adaatt_fwd* a, int R, int G, hipStream_t s);
int l2s_adaatt_cell_bwd(const l2s_adaatt_bwd* a, int R, int G, hipStream_t s);
/* Attention over L + 1 slots for S tokens at once (it does not feed the recurrence): slot 0 is the token's sentinel (frl[s], embedded fre[s]),
 * slots 1..L the locations (att [L][R], patt [L][R]).  tanh_ws[S][L+1][R] = tanh(embed_slot + hoe[s]) (before `mask`, the hA dropout mask
 * [S][L+1][R] or NULL), dots [S][256], PI[S][L+1] = softmax, atten[S][R] = PI[0] frl + sum_l PI[l] att[l-1] + hol.  L + 1 <= 256. */
int l2s_adaatt_att_fwd(const float* att, const float* patt, const float* frl, const float* fre, const float* hoe, const float* hol, const float* aw,
                       const float* ab, const float* mask, int S, int L, int R, float* tanh_ws, float* dots, float* PI, float* atten, hipStream_t s);
/* its backward per token, what flows on to the cell: ddot[S][L+1] (softmax backward), dhoe / dfre [S][R] (the sum over the slots taken about
 * its PI-weighted mean), dctx = dhoe - dfre, dfrl = PI[0] datten, dhol = datten.  R % 4 == 0, 16-byte aligned datten / att / frl. */
int l2s_adaatt_att_bwd_step(const float* datten, const float* att, const float* frl, const float* tanh_ws, const float* mask, const float* PI,
                            const float* aw, int S, int L, int R, float* ddot, float* dhoe, float* dfre, float* dctx, float* dfrl, float* dhol,
                            hipStream_t s);
/* and what is summed over the tokens: dpatt[L][R] +=, datt[L][R] += sum_s PI[s][l] datten[s], daw[R] += (all slots) */
int l2s_adaatt_att_bwd_batched(const float* ddot, const float* PI, const float* datten, const float* tanh_ws, const float* mask, const float* aw,
                               int S, int L, int R, float* dpatt, float* datt, float* daw, hipStream_t s);
/* dynamic-filter correlation (NET:504-562): filt float [7][C] (tanh'ed), r float [7].
 * y(dtype)[HW][C] = x * resp, resp float [HW], respk float [HW][7] (masked per-filter responses) */
int l2s_dynfilter_fwd(const void* x, const float* filt, const float* r, void* y, float* resp, float* respk, int H, int W, int C,
                      int dtype, int gate /*0: y = x*response, 1: y = x*sigmoid(response) (the *_response variants)*/, hipStream_t s);
/* dy(dtype) -> dx(dtype), dfilt float [7][C] (+=), dr float [7] (+=); ws: l2s_dynfilter_ws_floats(H, W, C) floats (d(response) per pixel
 * + per-pixel-chunk partial filter gradients, summed in chunk order by a third launch: no atomics) */
long l2s_dynfilter_ws_floats(int H, int W, int C);
int l2s_dynfilter_bwd(const void* dy, const void* x, const float* filt, const float* r, const float* resp, const float* respk,
                      void* dx, const void* relu_ref, float* dfilt, float* dr, float* ws, int H, int W, int C, int dtype,
                      int gate, const float* dresp_extra /*nullable [HW]: d(response loss)/d(response)*/, hipStream_t s);
/* dfilt == NULL in l2s_dynfilter_bwd: only dx is produced (the main queue needs nothing else); l2s_dynfilter_bwd_finish then turns the
 * workspace into dfilt += / dr += on whichever stream the language-side backward runs on. */
int l2s_dynfilter_bwd_finish(const float* ws, const float* respk, float* dfilt, float* dr, int H, int W, int C, hipStream_t s);
/* att2in2 attention (AttModel.py:406-423): patt [L][D], att [L][D] float; att_h [D]; alpha w[D], b.
 * out: weight [L] (softmax), att_res [D + 256] (the tail is scratch for the raw dots) */
int l2s_cap_attention_fwd(const float* patt, const float* att, const float* att_h, const float* aw, const float* ab, int L, int D,
                          float* tanh_ws /*[L][D]*/, float* weight, float* att_res, hipStream_t s);
int l2s_cap_attention_bwd(const float* datt_res, const float* att, const float* tanh_ws, const float* weight, const float* aw, int L, int D,
                          float* dpatt /*[L][D] +=*/, float* datt /*[L][D] +=*/, float* datt_h /*[D + 256] = (tail: scratch)*/, float* daw /*[D] +=*/, float* dab /*+=*/, hipStream_t s);
/* att2in2 core gates (AttModel.py:446-466): s[5R] = i2h+h2h, a2c[2R]; maxout candidate, no tanh */
/* Fused per-step launches of the att2in2 recurrence (AttModel.py:406-466): the recurrence is a chain of dependent launches on
 * the caption stream, so the per-step work is packed into as few launches as the data dependencies allow.
 *   l2s_linear2_fwd        : h2att(h) and h2h(h) (+= into the i2h sums) from one read of h            (ATT:425,453)
 *   l2s_cap_a2c_gates_fwd  : a2c Linear + sigmoid / maxout / cell update of l2s_cap_gates_fwd          (ATT:449-462)
 *   l2s_linear_sum2_fwd    : dh = W_h2h^T dsums + W_h2att^T datt_h (transposed copies, one launch)
 *   l2s_cap_attention_bwd_step / _batched : the attention backward split into what the recurrence needs at step t
 *       (ddot[L], datt_h[D]) and the step-summed parameter / feature gradients computed once after the loop. */
int l2s_linear2_fwd(const float* x, int K, const float* w1, const float* b1, float* y1, int N1, int acc1, const float* w2, const float* b2,
                    float* y2, int N2, int acc2, hipStream_t s);
int l2s_linear_sum2_fwd(const float* x1, const float* w1 /*[N][K1]*/, int K1, const float* x2, const float* w2 /*[N][K2]*/, int K2, float* y, int N,
                        int accumulate, hipStream_t s);
int l2s_cap_a2c_gates_fwd(const float* att_res, const float* w_a2c /*[2R][K]*/, const float* b_a2c, int K, const float* sums /*[5R]*/,
                          const float* c_prev, float* c, float* h, float* save /*[6R]*/, int R, hipStream_t s);
/* Projected-attention form of the same step (csrc/caption_step.hip): P = att . W_a2c^T [L][2R] once per sentence, then per token
 *   l2s_cap_att_dots_fwd      : dots[l] = alpha . tanh(patt[l] + att_h) + b                                  (ATT:411-418)
 *   l2s_cap_apply_gates_fwd   : softmax(dots) -> weight[L]; a2c = sum_l weight[l] P[l] + b_a2c; gates / cell update  (ATT:419-423,449-462)
 *   l2s_cap_gates_bwd_dw      : gate backward (as l2s_cap_gates_bwd) + dweight[l] = P[l] . da2c
 *   l2s_cap_attention_bwd_step2 : softmax backward from dweight -> ddot[L], datt_h[D]
 * l2s_cap_attention_bwd_batched accepts datt_res == NULL (no d(att) term: it then comes from d(P)). */
int l2s_cap_att_dots_fwd(const float* patt, const float* att_h, const float* aw, const float* ab, int L, int D, float* tanh_ws, float* dots, hipStream_t s);
int l2s_cap_apply_gates_fwd(const float* P, const float* dots, const float* b_a2c, const float* sums, const float* c_prev, float* c, float* h,
                            float* save, float* weight, int L, int R, hipStream_t s);
int l2s_cap_gates_bwd_dw(const float* dh, const float* dh2, const float* dc_in, const float* save, const float* c_prev, const float* P,
                         float* dsums, float* da2c, float* dc_prev, float* dweight, int L, int R, hipStream_t s);
int l2s_cap_attention_bwd_step2(const float* dweight, const float* tanh_ws, const float* weight, const float* aw, int L, int D, float* ddot,
                                float* datt_h, hipStream_t s);
int l2s_cap_attention_bwd_step(const float* datt_res, const float* att, const float* tanh_ws, const float* weight, const float* aw, int L, int D,
                               float* ddot /*[L]*/, float* datt_h /*[D]*/, hipStream_t s);
int l2s_cap_attention_bwd_batched(const float* ddot /*[S][L]*/, const float* weight /*[S][L]*/, const float* datt_res /*[S][ldr]*/, int ldr,
                                  const float* tanh_ws /*[S][L][D]*/, const float* aw, int S, int L, int D, float* dpatt /*+=*/, float* datt /*+=*/,
                                  float* daw /*+=*/, float* dab /*+=*/, hipStream_t s);
/* A frozen 64-plane bottleneck behind its first 1x1 convolution as ONE launch (csrc/bottleneck_fused.hip; RES:78-114, the frozen layer1 of
 * RES:291-299), bf16, forward only: b = relu(conv3x3(a) + b2); y = relu(conv1x1(b) + b3 + shortcut), shortcut = x (Cx = 256) or conv1x1(x; wd) + bd
 * (Cx = 64); optionally a_next = relu(conv1x1(y; w1n) + b1n) = the next block's first convolution.  Weights BN-folded bf16 [Cout][KH][KW][Cin],
 * biases f32; every pointer 16-byte aligned; any H, W. */
typedef struct {
  const void* a;                    /* [H*W][64]  */
  const void* x;                    /* [H*W][Cx]  */
  const void *w2, *w3, *wd, *w1n;   /* [64][3][3][64], [256][64], [256][64] (Cx = 64) or NULL, [64][256] or NULL */
  const float *b2, *b3, *bd, *b1n;
  void* y;                          /* [H*W][256] */
  void* a_next;                     /* [H*W][64] or NULL */
  int H, W, Cx;
} l2s_bottleneck64_desc;
int l2s_bottleneck64_fwd(const l2s_bottleneck64_desc* d, hipStream_t s);

/* The whole recurrence as ONE resident launch per direction (csrc/cap_recur.hip; ATT:406-423,446-466): L2S_CAP_RECUR_WGS workgroups own 16 hidden units each
 * (weights in registers, fp32), three granule exchanges per token.  Supported for rnn_size = att_hid_size = 512 and L <= 224 locations
 * (l2s_cap_recur_supported); callers fall back to the three launches per token above otherwise.  `state`: a caller-owned buffer of
 * l2s_cap_recur_state_bytes(backward) bytes, 16-byte aligned, ZEROED ONCE when it is allocated and then left to the kernels (word 0: launch
 * count = the exchange epoch; word 1: set to 1 when a bounded spin gave up - results are then invalid); one per direction. */
#define L2S_CAP_RECUR_WGS 32
typedef struct {
  const float *w_h2h, *b_h2h;      /* [5R][R], [5R] */
  const float *w_h2att, *b_h2att;  /* [AH][R], [AH] */
  const float *patt;               /* [L][AH]  ctx2att(att) */
  const float *aw, *ab;            /* alpha_net weight [AH], bias [1] */
  const float *P, *b_a2c;          /* [L][2R] = att . W_a2c^T, [2R] */
  const float *sums;               /* [S][5R]  i2h(x_t) + b_i2h (read only) */
  float *hs, *cs;                  /* [(S+1)][R], row 0 = the initial state */
  float *save;                     /* [S][6R] as l2s_cap_gates_fwd */
  float *tanh_ws;                  /* [S][L][AH] */
  float *wgt;                      /* [S][L] attention weights */
  unsigned* state;
  int S, R, AH, L;
} l2s_cap_recur_fwd_args;
typedef struct {
  const float *w_h2h, *w_h2att, *P, *aw;
  const float *save, *cs, *wgt, *tanh_ws;   /* as written by the forward launch */
  const float *dho;                /* [S][R] gradient of the loss w.r.t. h_t through the logit layer */
  float *dsums, *da2c;             /* [S][5R], [S][2R] */
  float *ddot, *datt_h;            /* [S][ld_ddot] (L used), [S][ld_datt_h] (AH used) */
  unsigned* state;
  int S, R, AH, L, ld_ddot, ld_datt_h;
} l2s_cap_recur_bwd_args;
int l2s_cap_recur_supported(int S, int R, int AH, int L);
size_t l2s_cap_recur_state_bytes(int backward);
int l2s_cap_recur_fwd(const l2s_cap_recur_fwd_args* a, hipStream_t s);
int l2s_cap_recur_bwd(const l2s_cap_recur_bwd_args* a, hipStream_t s);
int l2s_cap_gates_fwd(const float* sums, const float* a2c, const float* c_prev, float* c, float* h, float* save /*[6R]: sig(3R), sel(R), cand(R), tanh(c)(R)*/, int R, hipStream_t s);
int l2s_cap_gates_bwd(const float* dh, const float* dh2 /*nullable: dh = dh + dh2*/, const float* dc_in, const float* save, const float* c_prev, float* dsums /*[5R]*/, float* da2c /*[2R]*/, float* dc_prev, int R, hipStream_t s);
/* log_softmax + masked NLL (AttModel.py:98, misc/utils.py:43-53): logits [S][V1]; dlogits = gscale*(softmax - onehot)*mask/sum(mask) */
int l2s_logsoftmax_nll(const float* logits, const int64_t* target, const float* mask, int S, int V1, float gscale, float* loss_slot,
                       float* dlogits, float* logprobs_opt, hipStream_t s);

/* ---------------------------------------------------------------- input side ----- */
/* Host. COCO compressed run-length string -> run lengths; replaces rleFrString, pyutils/refer/external/maskApi.c:217-231
 * (reached through external/mask.py decode <- lib/loaders/cycle_loader.py:199).  Returns the number of runs written to
 * cnts[0..max_counts), or -1 for a truncated string / too small a buffer. */
int l2s_rle_from_string(const char* s, uint32_t* cnts, int max_counts);
/* Host. prep_im_for_blob's scale (pyutils/mask-faster-rcnn/lib/utils/blob.py:35-43: target_size / short side, capped so that
 * round(scale * long side) <= max_size) and cv2.resize's output size (round-half-even of h * scale, w * scale). */
int l2s_prep_geometry(int h, int w, int target_size, int max_size, double* scale, int* oh, int* ow);
/* Device. blob.py:32-47 on one image: uint8 BGR [h][w][3] -> float32 [oh][ow][3] = cv2.resize(float32(img) - means, fx = fy =
 * scale, INTER_LINEAR); the result is the `data` blob of cycle_loader.py:119-138 for a batch of one image. */
int l2s_prep_image(const uint8_t* img_bgr, int h, int w, double mean_b, double mean_g, double mean_r, double scale,
                   int oh, int ow, float* out, hipStream_t s);
/* Device. The gt mask of one referred object (cycle_loader.py:198-210): rleDecode (maskApi.c:43-47) of its n run-length objects
 * (column-major runs, concatenated in cnts, object r = cnts[offs[r]..offs[r+1])), union over the objects (sum > 0), PIL-nearest
 * resize from [h][w] to [oh][ow] (scipy.misc.imresize 'nearest'); out uint8 {0,1} row-major.  ws: l2s_rle_ws_words() uint32. */
long l2s_rle_ws_words(int total_counts, int oh, int ow);
int l2s_rle_to_mask(const uint32_t* cnts, const int* offs, int n, int total_counts, int h, int w, int oh, int ow,
                    uint32_t* ws, uint8_t* out, hipStream_t s);

/* ---------------------------------------------------------------- evaluation (model/eval_device.py) ----- */
/* One sentence's result, in a caller-owned device array (48 bytes): the picked (roi, class), its box in the original image,
 * box hit (IoU >= 0.5), and the mask's intersection / union pixel counts. */
typedef struct { int roi; int cls; float box[4]; int hit; int reserved; long long I; long long U; } l2s_eval_record;
/* Device, one workgroup.  model/test.py best_detection over cls_prob [post][ncls] rows < *nkeep (nkeep NULL: all `post` rows; rows
 * behind it are padding and ignored) + detect_from_outputs / bbox_transform_inv_np / _clip_boxes on the chosen row (im_h, im_w: the
 * original image size round(im_info / scale); bbox_reg = cfg.TEST.BBOX_REG) + computeIoU_box against gt_box (x1 y1 x2 y2, scaled
 * image) / im_scale.  Writes *rec with I = U = 0, the mask head's RoI [5] (batch index 0, pred_box * im_scale) and its class label. */
int l2s_eval_pick(const float* cls_prob, const float* bbox_pred, const float* rois, const int* nkeep, int post, int ncls, float im_scale,
                  int im_h, int im_w, const float* gt_box, int bbox_reg, l2s_eval_record* rec, float* mask_roi, int* mask_label, hipStream_t s);
/* Device.  segment_from_mask_prob of the chosen class's [ms][ms] probabilities (ms <= 16) on rec->box into an ih x iw canvas (bytescale,
 * Pillow 8-bit BILINEAR, paste, > 122) against the gt mask [Hs][Ws] uint8 PIL-NEAREST resized to ih x iw: adds the intersection and
 * union pixel counts to rec->I, rec->U (integer atomics).  canvas: optional uint8 [ih][iw] dump of the predicted mask (checks). */
int l2s_eval_mask_iou(const float* mask_prob, int ms, l2s_eval_record* rec, const uint8_t* gt, int Hs, int Ws, int ih, int iw,
                      uint8_t* canvas, hipStream_t s);

/* Device.  rleEncode (pyutils/refer/external/maskApi.c:32-41) of one row-major uint8 [h][w] mask (nonzero = 1), the counterpart of
 * l2s_rle_to_mask: runs over the column-major order, starting with a run of zeros (a leading 0 if the first pixel is set; an all-zero
 * mask is the single count h * w).  The n counts go to pool[off .. off + n) with off = *cursor at entry, *cursor advances by n and
 * *span = {off, n}: calls on one stream pack their outputs back to back without the host.  If off + n > pool_words nothing is written
 * to pool, *cursor stays and *span = {-1, n}.  pool, cursor, span, ws are device memory; ws: l2s_rle_encode_ws_words(h, w) uint32.
 * h * w < 2^31.  l2s_rle_encode_chunk_rows(): the rows of one column that one lane encodes (the decomposition's chunk, for tests). */
typedef struct { int off; int n; } l2s_rle_span;
long l2s_rle_encode_ws_words(int h, int w);
int l2s_rle_encode_chunk_rows(void);
int l2s_rle_from_mask(const uint8_t* mask, int h, int w, uint32_t* pool, int pool_words, int* cursor, l2s_rle_span* span, uint32_t* ws,
                      hipStream_t s);
/* Device.  l2s_rle_from_mask for n row-major masks of one size (masks [n][h][w]) in the same three launches: the masks are taken in
 * order, each with the pool / cursor / span contract above and its own spans[b]; masks at b >= *n_valid (device int) are skipped
 * with spans[b] = {0, 0}.  The bytes left in pool, the spans and the cursor are those of *n_valid consecutive l2s_rle_from_mask
 * calls.  ws: n * l2s_rle_encode_ws_words(h, w) uint32.  n <= 65535. */
int l2s_rle_from_masks(const uint8_t* masks, int n, const int* n_valid, int h, int w, uint32_t* pool, int pool_words, int* cursor,
                       l2s_rle_span* spans, uint32_t* ws, hipStream_t s);
/* Host.  Run lengths -> COCO compressed run-length string (rleToString, maskApi.c:203-215), the inverse of l2s_rle_from_string.
 * Returns the length of the zero-terminated string written to out[0..max_chars), or -1 if it does not fit. */
int l2s_rle_to_string(const uint32_t* cnts, int n, char* out, int max_chars);

/* ---------------------------------------------------------------- every instance per sentence (model/detect_device.py) ----- */
/* One detection, in a caller-owned device array (32 bytes): the RoI row and class, the box in the original image, cls_prob[roi][cls]
 * and the number of set pixels of its mask (0 until l2s_detect_paste). */
typedef struct { int roi; int cls; float box[4]; float score; int area; } l2s_det_record;
/* Device, one workgroup per class.  The reference's test.py:268-283 on the inputs of l2s_eval_pick (same decode, bit for bit): for every
 * class j >= 1 the rows < *nkeep with cls_prob[r][j] > thresh (a NaN score is no candidate), ordered by score descending with ties by
 * lower row, through greedy NMS as cpu_nms (lib/nms/src/nms.c:35-63: areas with + 1, ovr >= nms_thresh suppresses; float32, separate
 * roundings).  The kept (row, score, box) lists go to ws (l2s_detect_ws_bytes(post, ncls) bytes) for l2s_detect_select.  boxes_dump:
 * optional float [post][ncls][4], every decoded box (checks).  post <= 5120, 2 <= ncls <= 1024; L2S_EINVAL otherwise. */
size_t l2s_detect_ws_bytes(int post, int ncls);
int l2s_detect_nms(const float* cls_prob, const float* bbox_pred, const float* rois, const int* nkeep, int post, int ncls, float im_scale,
                   int im_h, int im_w, int bbox_reg, float thresh, float nms_thresh, void* ws, float* boxes_dump, hipStream_t s);
/* Device, one workgroup.  test.py:285-297 on the lists l2s_detect_nms left in ws: with max_per_image > 0 and more survivors than that,
 * image_thresh = the max_per_image-th largest surviving score (exact: a radix select over the scores' bits) and a detection stays iff
 * score >= image_thresh (ties all stay); max_per_image <= 0: no limit.  The detections in class order (inside a class: score
 * descending, ties by lower row) go to rec[0 .. written), the mask head's RoIs (batch index 0, box * im_scale) and labels to
 * mask_rois [cap][5], mask_labels [cap]; count = {written = min(total, cap), total}.  Rows in [written, cap) are zeroed; nothing
 * behind cap is written. */
int l2s_detect_select(const void* ws, int post, int ncls, int max_per_image, float im_scale, l2s_det_record* rec, float* mask_rois,
                      int* mask_labels, int cap, int* count, hipStream_t s);
/* Device.  l2s_eval_mask_iou's paste (recover_masks: bytescale, Pillow 8-bit BILINEAR, paste, > 122) for every detection d < count[0]:
 * mask_prob [cap][ms][ms] on rec[d].box into canvases [cap][ih][iw] (uint8 {0, 1}), the set pixels added to rec[d].area (integer
 * atomics).  Detections d >= count[0] are skipped, their canvases untouched.  cap <= 65535. */
int l2s_detect_paste(const float* mask_prob, int ms, l2s_det_record* rec, const int* count, int cap, int ih, int iw, uint8_t* canvases,
                     hipStream_t s);

/* ---------------------------------------------------------------- judging the detections (model/detect_device.py, csrc/select.hip) ----- */
/* One detection against the sentence's ground truth (16 bytes): the intersection and union pixel counts of its mask with the gt
 * mask, and whether its box hits the gt box (IoU >= 0.5). */
typedef struct { int I; int U; int hit; int reserved; } l2s_det_gt;
/* One rule's choice among a sentence's detections (40 bytes): its index in the list (-1: the list is empty; then cls = -1, hit = 0,
 * I = 0, U = the gt's pixels), its class, hit, I, U and the key it won with. */
typedef struct { int det; int cls; int hit; int reserved; long long I; long long U; double key; } l2s_det_choice;
/* Device.  For every detection d < count[0] (clamped to cap) of canvases [cap][ih][iw] (uint8 {0, 1}, as l2s_detect_paste left them:
 * zero outside eval_box_geometry of rec[d].box, rec[d].area set pixels): I = |canvas & gt|, U = |canvas | gt| with the gt mask [Hs][Ws]
 * PIL-NEAREST resized to ih x iw as l2s_eval_mask_iou reads it, and hit = computeIoU_box(rec[d].box, gt_box / im_scale) >= 0.5 by
 * l2s_eval_pick's float32 expressions; gt_area[0] = the set pixels of the resized gt.  Only the box of a detection is read:
 * U = rec[d].area + gt_area - I, in integers.  out [cap] and gt_area [1] are accumulated into with integer atomics and must be zero on
 * entry; rows d >= count[0] are written as zeros.  cap <= 65535, ih * iw < 2^31; L2S_EINVAL otherwise. */
int l2s_detect_gt_iou(const uint8_t* canvases, const l2s_det_record* rec, const int* count, int cap, int ih, int iw, const uint8_t* gt, int Hs,
                      int Ws, const float* gt_box, float im_scale, l2s_det_gt* out, int* gt_area, hipStream_t s);
/* Device, one workgroup.  Among the detections d < count[0] (clamped to cap), ties to the lowest d, out[0] = `detector`: max rec[d].score;
 * out[1] = `oracle`: max I / U, compared exactly (a beats b iff I_a * U_b > I_b * U_a in 64 bits; U = 0 counts as 0 / 1), key = I / U in
 * double; and with expr (device float [cap], the expression's log-likelihood under every detection's mask) out[2] = `speaker`: max
 * expr[d]; out[3 + k] = `rerank@lambdas[k]`: max key = log((double)score) + (double)lambdas[k] * (double)expr[d] / (per_token ? n_tok : 1),
 * every operation rounded on its own.  lambdas: host float [n_lambda], n_lambda <= 8; n_lambda > 0 without expr is L2S_EINVAL.
 * Scores and expr are taken to be no NaN. */
int l2s_detect_choose(const l2s_det_record* rec, const l2s_det_gt* gt, const int* count, int cap, const int* gt_area, const float* expr,
                      const float* lambdas, int n_lambda, int per_token, int n_tok, l2s_det_choice* out, hipStream_t s);

/* ---------------------------------------------------------------- caption decoding (nets/decode.py, csrc/decode.hip) ----- */
/* Device, one workgroup.  One decision of AttModel.sample (AttModel.py:172-201) on logits[V1]: log-softmax in f32, then
 *   sample_max != 0: the argmax (lowest index on equal values);
 *   sample_max == 0: k drawn from p_k ~ exp(logprob_k / temperature) by inverse CDF in index order: the first k whose cumulative sum
 *                    exceeds u * total.  u = u_in[t] when u_in is given, else 24 bits of the counter hash of (*seed_dev, salt, t).
 * The reported log-probability is the untempered logprob[k].  *finished (device int, reset at t == 0): once a 0 was drawn every later
 * token is 0 with log-probability 0.  Writes seq[t], seq_logprobs[t] and *next_token (what the next step's l2s_embed_fwd reads). */
int l2s_decode_pick(const float* logits, int V1, int t, int sample_max, float temperature, const float* u_in, const uint64_t* seed_dev,
                    uint64_t salt, int* finished, int64_t* seq, float* seq_logprobs, int64_t* next_token, hipStream_t s);
#define L2S_BEAM_MAX 16           /* beam_size */
#define L2S_BEAM_MAX_T 64         /* seq_length: the previous tables of a step are copied to the LDS */
/* One completed beam, in a caller-owned device array of L2S_BEAM_RECORD_WORDS(T) 32-bit words each: seq[T] (int), logps[T] (float),
 * p (float: the joint log-probability), index (int: the order of completion). */
#define L2S_BEAM_RECORD_WORDS(T) (2 * (T) + 2)
typedef struct {
  const float* logits; int ld_logits;                    /* [B][V1] */
  int V1, B, t, T, R, n_state;
  int* beam_seq; float* beam_seq_logprobs; float* beam_logprobs_sum;     /* [T][B], [T][B], [B] */
  const float* state_in[4]; float* state_out[4]; int ld_in[4], ld_out[4]; /* n_state arrays of B rows of R; in and out never overlap */
  int64_t* next_tokens; int* parents;                    /* [B], [B] */
  int* done; int* done_count;                            /* B * T records; device counter (reset at t == 0) */
} l2s_beam_step_args;
/* Device, one workgroup.  beam_step plus the completion loop of CaptionModel.py:27-121 for one t: per row the log-softmax with -1000 on
 * the last column (:93; one row at t == 0) and its min(B, V1) best words, descending (equal values: lower index first); the candidates
 * in column-major order with p = sum[q] + r (one f32 add), ordered by p descending, stable; the first B win.  Their histories are forked
 * from a copy of the previous tables, the state rows gathered by parent, the B tokens written to next_tokens.  A beam whose token is 0,
 * or any beam at t == T - 1, is appended to `done` and its sum becomes -1000.  1 <= B <= min(16, V1), T <= 64, 0 <= t < T.
 * A NaN logit is no candidate and a NaN sum ranks last (as -inf): the outputs stay well defined and in range. */
int l2s_decode_beam_step(const l2s_beam_step_args* a, hipStream_t s);
/* Device, one workgroup per detection: l2s_decode_beam_step for every live detection of a sentence (detection d is live iff
 * row0 + d < *count, see the rows section below; a dead one is neither read nor written, the grid is `rows`).  `a` describes detection 0;
 * detection d uses logits rows [d B, d B + B) of [rows * B][ld_logits], beam_seq / beam_seq_logprobs [rows][T][B], beam_logprobs_sum
 * [rows][B], next_tokens [rows * B], parents [rows][B], done [rows][B * T] records, done_count [rows] and rows [d B, d B + B) of every
 * state array (gathered by parent inside the group).  The same device function: a detection gets the bits l2s_decode_beam_step gives it. */
int l2s_decode_beam_step_rows(const l2s_beam_step_args* a, int rows, int row0, const int* count, hipStream_t s);
/* Device, one workgroup per detection: the final ordering of CaptionModel.py:123.  The done_count[d] (clamped to B * T) records of
 * detection d ordered by p descending, equal p in completion order; the first beam_n[d] = min(B, done_count[d]) go to beam_seq int64
 * [rows][B][T], beam_logps f32 [rows][B][T] and beam_p f32 [rows][B] (zeros behind beam_n[d]), and the best one to seq int64 [rows][T]
 * (zero from its first 0 on) and logprobs f32 [rows][T] (kept up to and with that 0, zero behind it): l2s_decode_pick_rows' layout.
 * B <= 16, T <= 64.  Dead detections are not written. */
int l2s_decode_beam_finish_rows(const int* done, const int* done_count, int B, int T, int rows, int row0, const int* count,
                                int64_t* beam_seq, float* beam_logps, float* beam_p, int* beam_n, int64_t* seq, float* logprobs, hipStream_t s);
/* Device.  dst [H][W] = src [ih][iw] (uint8) resized by PIL NEAREST (csrc/pil_resize.h pil_nearest_src, the rule of the loader's masks). */
int l2s_mask_resize_nearest(const uint8_t* src, int ih, int iw, uint8_t* dst, int H, int W, hipStream_t s);

/* ---------------------------------------------------------------- the caption branch on rows (nets/caption_rows.py, csrc/caption_rows.hip) ----- */
/* One row per detection of a sentence.  Every entry takes the `rows` of its buffers, `row0` and `count` (device int32[1], null = all):
 * row r is live iff row0 + r < *count; a dead row is neither read nor written and no grid depends on *count, so the number of detections
 * never comes back to the host.  Each row is computed by the arithmetic, in the order, of the single-mask entry named. */
#define L2S_ROWS_MAX_W 8192       /* blob width of l2s_masks_to_map: its source-column table lives in the LDS */
/* out f32 {0,1} [rows][Hc * Wc] from masks uint8 [rows][mh][mw]: l2s_mask_resize_nearest to H x W (skipped when (mh, mw) == (H, W)), then
 * l2s_mask_downsample to Hc x Wc, as one launch; the H x W mask is never stored.  Integer counts: equal to the two launches bit for bit. */
int l2s_masks_to_map(const uint8_t* masks, int rows, int row0, const int* count, int mh, int mw, int H, int W, int Hc, int Wc, float* out,
                     hipStream_t s);
/* y [rows][OH * OW][ldy] (C channels each) = l2s_adaptive_pool_fwd of x [H * W][C] under pm [rows][H * W]; pm null: the unmasked pooling,
 * summed once and stored to every live row.  dtype of x and y: 0 = f32, 1 = bf16. */
int l2s_adaptive_pool_rows(const void* x, const float* pm, void* y, int rows, int row0, const int* count, int H, int W, int C, int OH, int OW,
                           int ldy, int dtype, hipStream_t s);
/* The att2in2 step in the projected form, per row on the row's own operands (L <= 256, R <= 1024); nothing is kept for backward.
 * dots [rows][256] = l2s_cap_att_dots_fwd of patt [rows][L][D] and att_h [rows][ld_att_h];
 * (c, h) [rows][R] = l2s_cap_apply_gates_fwd of P [rows][L][2R], dots, sums [rows][ld_sums] and c_prev [rows][R]. */
int l2s_cap_att_dots_rows(const float* patt, const float* att_h, int ld_att_h, const float* aw, const float* ab, int rows, int row0,
                          const int* count, int L, int D, float* dots, hipStream_t s);
int l2s_cap_apply_gates_rows(const float* P, const float* dots, const float* b_a2c, const float* sums, int ld_sums, const float* c_prev,
                             float* c, float* h, int rows, int row0, const int* count, int L, int R, hipStream_t s);
/* One workgroup per row: the log-softmax of logits [rows][ld_logits] over V1, then the argmax (lowest index on equal values) as
 * l2s_decode_pick takes it with finished int32 [rows] (reset at t == 0: after a 0 every token of the row is 0 with log-probability 0),
 * or, with `forced` (device int64[1], one token for all rows: teacher forcing, no finished rows), that token and its log-probability.
 * Writes seq [rows][T] and logprobs [rows][T] at column t, next_token [rows] and, where `sum` f32 [rows] is given, the sum of the row's
 * log-probabilities so far (set at t == 0, then added to in the order of t). */
int l2s_decode_pick_rows(const float* logits, int ld_logits, int V1, int rows, int row0, const int* count, int t, int T, const int64_t* forced,
                         int* finished, int64_t* seq, float* logprobs, int64_t* next_token, float* sum, hipStream_t s);
/* One workgroup per row: teacher forcing with a token row per row (AttModel.forward + LanguageModelCriterion for a batch of different
 * sentences), step t of T.  targets int64 [rows][T]: row r holds w_1 .. w_n, 0, then padding; lengths int32 [rows]: the scored positions
 * n_r + 1 of row r, 1 <= lengths[r] <= T.  A live row with t < lengths[r] gets logprobs[r][t] = logits[r][targets[r][t]] - logsumexp of
 * its V1 logits (l2s_decode_pick_rows' forced arithmetic: the same bits for the same logits and token; a token outside the table is
 * clamped), that value added to `sum` f32 [rows] where given (set at t == 0), and next_token[r] = targets[r][t].  With t >= lengths[r]
 * logprobs and sum are not written (the caller's zeros stay) and next_token[r] = 0.  Dead rows are neither read nor written. */
int l2s_decode_force_rows(const float* logits, int ld_logits, int V1, int rows, int row0, const int* count, int t, int T, const int64_t* targets,
                          const int* lengths, float* logprobs, int64_t* next_token, float* sum, hipStream_t s);
/* The top-down step on rows.  l2s_lstm_cell_rows: one nn.LSTMCell step (gate order i, f, g, o; l2s_topdown_cell_fwd's arithmetic) for every
 * live row in one launch:
 *   gates[r][4R] = pre[r * ld_pre] + pre2[r * ld_pre2] + add0 + add1 + sum over up to two segments w_k[4R][:n_k] . x_k[r * ldx_k][:n_k]
 * pre / pre2: NULL or [4R] per row with a row stride (0: one row for all rows); add0 / add1: NULL or [4R]; w_k: a column block (leading
 * dimension ld_k) of a wider matrix; a segment with n = 0 is skipped.  c_prev, c and h have their own row strides (h may be the second
 * half of a [rows][2R] array).  c and h must not alias c_prev or a segment's x.  The products run on the exact-fp32 MFMA: a workgroup owns
 * the four gate rows of 4 hidden units for a tile of 16 (rows <= 16) or 32 rows, so a weight element is fetched once per tile of rows.
 * Segments whose length, strides or addresses are not multiples of 4 floats take scalar loads.  R >= 1, any rows >= 1. */
typedef struct { const float* x; int ldx; const float* w; int ld; int n; } l2s_rows_seg;
typedef struct { const float* pre; int ld_pre; const float* pre2; int ld_pre2; const float* add0; const float* add1; l2s_rows_seg seg[2];
                 const float* c_prev; int ld_c_prev; float* c; int ld_c; float* h; int ld_h; } l2s_lstm_rows;
int l2s_lstm_cell_rows(const l2s_lstm_rows* a, int R, int rows, int row0, const int* count, hipStream_t s);
/* att_res[r * ld_res][:R] = l2s_cap_att_apply_fwd of att [rows][L][R] and dots [rows][256] per live row (no `weight` output), in that
 * kernel's summation order: the same bits as the single-row launch.  L <= 256, ld_res >= R. */
int l2s_cap_att_apply_rows(const float* att, const float* dots, float* att_res, int ld_res, int rows, int row0, const int* count, int L, int R,
                           hipStream_t s);
/* The step on GROUPS (beam search on rows): `rows` state rows, `group` consecutive ones per detection (rows % group == 0).  Row r reads
 * its own att_h / dots / sums / states and detection r / group's patt, P, att and (the cell) pre2, and is live iff
 * row0 + r / group < *count.  The bodies of the *_rows entries, which are the group == 1 case: the same bits as those entries on operands
 * replicated `group` times.  patt, P and att have rows / group rows of [L][.]; the cell's pre2 has rows / group rows of ld_pre2 floats
 * (ld_pre2 = 0: one row for all), read at row r / group, while pre, the segments' x, c_prev, c and h keep one row per state row. */
int l2s_cap_att_dots_groups(const float* patt, const float* att_h, int ld_att_h, const float* aw, const float* ab, int rows, int group,
                            int row0, const int* count, int L, int D, float* dots, hipStream_t s);
int l2s_cap_apply_gates_groups(const float* P, const float* dots, const float* b_a2c, const float* sums, int ld_sums, const float* c_prev,
                               float* c, float* h, int rows, int group, int row0, const int* count, int L, int R, hipStream_t s);
int l2s_cap_att_apply_groups(const float* att, const float* dots, float* att_res, int ld_res, int rows, int group, int row0,
                             const int* count, int L, int R, hipStream_t s);
int l2s_lstm_cell_groups(const l2s_lstm_rows* a, int R, int rows, int group, int row0, const int* count, hipStream_t s);

/* ---------------------------------------------------------------- launch tape / streams ----- */
/* `to` waits (device side) for everything enqueued so far on `from`; fork or join of the step's branches */
int l2s_stream_fork(hipStream_t from, hipStream_t to);
/* the two halves of a fork under a process-wide name (slot in [0,16)): l2s_event_record marks "everything enqueued so far on s",
 * l2s_event_wait makes s wait for the most recent mark of that slot (no-op if never marked).  Both are tape ops.  Used where the
 * mark and the wait belong to different steps: the first half of the optimiser update (train_val_cycle.py:194-220) is awaited
 * before the next step's first trainable layer while the deferred weight gradients run on behind it. */
int l2s_event_record(int slot, hipStream_t s);
int l2s_event_wait(int slot, hipStream_t s);
int l2s_memset_async(void* p, int value, size_t bytes, hipStream_t s);
int l2s_memcpy_d2d_async(void* dst, const void* src, size_t bytes, hipStream_t s);
/* record every launch / fork / memset issued through this ABI on the registered streams (they still execute), then replay
 * the whole multi-stream step from one call.  Valid while the recorded pointers, shapes and scalars stay the same. */
void* l2s_tape_begin(const hipStream_t* streams, int n);
int l2s_tape_end(void* tape);
long l2s_tape_size(void* tape);
int l2s_tape_run(void* tape, const hipStream_t* streams, int n);
/* segments: l2s_tape_mark() (while recording) cuts the tape where the host must act between launches (RCCL all-reduce of a finished
 * gradient bucket); l2s_tape_run_segment replays segment `seg` in [0, l2s_tape_segments) */
int l2s_tape_pause(int on);   /* 1: launches execute but are not recorded until l2s_tape_pause(0) (host work between two segments) */
int l2s_tape_mark(void);
/* measurement: "record a timing event here" as a tape op (id >= 0 while recording, -1 otherwise); elapsed HIP-event time between two such
   points of the last replayed step (bench.py brackets the dominant launch inside the pipelined replay with these) */
int l2s_tape_time_event(hipStream_t s);
int l2s_time_event_elapsed(int a, int b, float* ms);
int l2s_tape_segments(void* tape);
int l2s_tape_run_segment(void* tape, const hipStream_t* streams, int n, int seg);
int l2s_tape_destroy(void* tape);

/* ---------------------------------------------------------------- optimizer ---------------- */
/* torch.optim.SGD with momentum as configured at train_val_cycle.py:194-220, fused over a flat parameter buffer.
 * seg table (device): per segment {offset, count, rows, wd_flag}; rowscale (optional, per segment offset into a float array,
 * -1 = none) multiplies the gradient per output row (folded frozen-BN scale). */
typedef struct { long offset; long count; int row_len; int weight_decay; long rowscale_off; float lr_mult;
                 int chunk0; /* running count of ceil(count / l2s_sgd_chunk()) over the table's earlier segments (any common origin) */
                 int flags;  /* 1: the gradient is overwritten whole by its producer every step (l2s_wgrad_prob.flags): the update leaves it alone */
                 int reserved; } l2s_sgd_seg;
/* the same update restricted to the elements [lo, hi) of the flat buffer: a rank's shard of a gradient bucket (data parallel, reduce-scatter
 * -> sharded update -> all-gather of the weights).  [chunk_lo, chunk_hi): the work chunks of the table that can hold such elements, numbered from the
 * table's first chunk (chunk_hi < 0: to the end).  flags: 1 = zero the gradients consumed, 2 = only rewrite the shadow from the parameters. */
int l2s_sgd_momentum_range(float* param, float* grad, float* mom, const l2s_sgd_seg* segs, int nseg, const float* rowscale,
                           float lr, float momentum, float wd, float grad_scale, void* shadow, int shadow_dtype, int flags,
                           long lo, long hi, int chunk_lo, int chunk_hi, hipStream_t s);
/* the ranged update with the gradients read from a bf16 buffer instead: element o of the flat buffer takes grad_bf16[o - grad_lo] (grad_lo a
 * multiple of 4, grad_bf16 8-byte aligned, every updated element at or behind grad_lo).  Data parallel: the reduce-scattered bf16 shard of a
 * bucket feeds the update as it is - no cast pass back into the f32 gradient buffer, which this call neither reads nor clears. */
int l2s_sgd_momentum_range_g16(float* param, const void* grad_bf16, long grad_lo, float* mom, const l2s_sgd_seg* segs, int nseg, const float* rowscale,
                               float lr, float momentum, float wd, float grad_scale, void* shadow, int shadow_dtype,
                               long lo, long hi, int chunk_lo, int chunk_hi, hipStream_t s);
int l2s_sgd_chunk(void);          /* elements of one work chunk of the update kernel */
int l2s_sgd_momentum(float* param, float* grad, float* mom, const l2s_sgd_seg* segs, int nseg, const float* rowscale,
                     float lr, float momentum, float wd, float grad_scale, void* shadow /*optional: dtype copy of rowscale*param at the same offsets*/,
                     int shadow_dtype, int clear_grad /*1: the gradient is zeroed as it is read (optimizer.zero_grad() of train_val_cycle.py:383 folded in)*/,
                     hipStream_t s);

#ifdef __cplusplus
}
#endif
#endif
