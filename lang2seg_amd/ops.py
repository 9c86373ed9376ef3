"""Thin tensor-level wrappers over the C ABI (include/lang2seg_hip.h).

PyTorch is used for device memory and streams only: every wrapper passes raw
`data_ptr()`s + sizes + the current HIP stream to liblang2seg_hip.so.  Outputs are
caller- or wrapper-allocated torch tensors; no arithmetic happens in torch here."""
import ctypes as C
import torch
from . import _lib
from ._lib import ptr, call, F32, BF16, ConvDesc, WgradDesc

TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16}


def stream():
    return torch.cuda.current_stream().cuda_stream


def dt_of(t):
    return BF16 if t.dtype == torch.bfloat16 else F32


def empty(shape, dt, device='cuda'):
    return torch.empty(shape, dtype=TORCH_DT[dt], device=device)


# ------------------------------------------------------------------ streams / tape
def stream_fork(from_stream, to_stream):
    """`to_stream` waits for everything enqueued so far on `from_stream` (torch.cuda.Stream objects)."""
    call('l2s_stream_fork', from_stream.cuda_stream, to_stream.cuda_stream)


def event_record(slot, s):
    """mark 'everything enqueued so far on stream s' under the process-wide slot number (csrc/tape.hip)"""
    call('l2s_event_record', int(slot), s.cuda_stream)


def event_wait(slot, s):
    """stream s waits for the most recent mark of the slot"""
    call('l2s_event_wait', int(slot), s.cuda_stream)


def memset_zero(t):
    call('l2s_memset_async', ptr(t), 0, t.numel() * t.element_size(), stream())


def memcpy(dst, src):
    call('l2s_memcpy_d2d_async', ptr(dst), ptr(src), src.numel() * src.element_size(), stream())


def tape_begin(streams):
    arr = (C.c_void_p * len(streams))(*[s.cuda_stream for s in streams])
    h = _lib.load().l2s_tape_begin(arr, len(streams))
    if not h:
        raise _lib.L2SError('l2s_tape_begin failed')
    return h


def tape_end(h):
    call('l2s_tape_end', h)


def tape_run(h, streams):
    arr = (C.c_void_p * len(streams))(*[s.cuda_stream for s in streams])
    call('l2s_tape_run', h, arr, len(streams))


def tape_mark():
    call('l2s_tape_mark')


def tape_pause(on):
    call('l2s_tape_pause', 1 if on else 0)


def tape_time_event():
    """(measurement) 'record a timing event here' on the current stream's tape order; id >= 0 while a tape is recording, else -1"""
    return int(_lib.load().l2s_tape_time_event(stream()))


def time_event_elapsed(a, b):
    ms = C.c_float(0.0)
    call('l2s_time_event_elapsed', a, b, C.byref(ms))
    return float(ms.value)


def tape_run_segment(h, streams, seg):
    arr = (C.c_void_p * len(streams))(*[s.cuda_stream for s in streams])
    call('l2s_tape_run_segment', h, arr, len(streams), seg)


def tape_destroy(h):
    torch.cuda.synchronize()                     # nothing of the tape may still be in flight
    call('l2s_tape_destroy', h)


def tape_size(h):
    return int(_lib.load().l2s_tape_size(h))


def last_kernel():
    """tests and reports only: the kernel of this thread's latest launch as its launch site names it, without blanks or the macro's
    parentheses ('linear_fwd_kernel<8,2,1>'); None before the first launch"""
    n = _lib.load().l2s_last_kernel()
    return None if n is None else n.decode().replace(' ', '').strip('()')


# ------------------------------------------------------------------ conv / gemm
# kernel family of every convolution that does not name one (l2s_conv_desc.algo: 0 = auto); set by the benchmark tools only
# (bench.py --conv-algo, tools/*bench*.py): same arithmetic, speed only
CONV_ALGO = 0
LAST_PLAN = None        # name of the kernel the dispatcher picked for the last conv_igemm call (bench.py's launch timer reads it)
TRACK_PLAN = False      # set by bench.py's LaunchTimer: the extra ctypes call per launch is measurement only


def conv_igemm(x, w, y, n_img, IH, IW, Cin, OH, OW, Cout, KH=1, KW=1, stride=1, pad=0, bias=None, add=None,
               ref=None, relu=False, out_f32=False, deconv=False, scatter=None, ldx=None, ldy=None, ldadd=None,
               ldref=None, tile=0, dt=None, ws=None, split_k=0, xcd_mode=-1, algo=None, prio=0):
    d = ConvDesc()
    d.x, d.w, d.y = ptr(x), ptr(w), ptr(y)
    d.bias, d.add, d.ref = ptr(bias), ptr(add), ptr(ref)
    d.n_img, d.IH, d.IW, d.Cin, d.OH, d.OW, d.Cout = n_img, IH, IW, Cin, OH, OW, Cout
    d.KH, d.KW, d.stride, d.pad = KH, KW, stride, pad
    d.ldx = Cin if ldx is None else ldx
    ocols = (Cout // 4) if deconv else Cout
    d.ldy = ocols if ldy is None else ldy
    d.ldadd = (ocols if ldadd is None else ldadd)
    d.ldref = (ocols if ldref is None else ldref)
    fl = 0
    if relu:
        fl |= _lib.CONV_RELU
    if out_f32:
        fl |= _lib.CONV_OUT_F32
    if deconv:
        fl |= _lib.CONV_DECONV2X2
    if scatter is not None:
        fl |= _lib.CONV_SCATTER
        d.out_h, d.out_w, d.out_stride = scatter
    d.flags = fl
    d.tile = tile
    d.split_k = split_k
    d.xcd_mode = xcd_mode
    d.algo = CONV_ALGO if algo is None else algo
    d.ws = ptr(ws)
    d.ws_floats = 0 if ws is None else ws.numel()
    d.prio = prio
    global LAST_PLAN
    dtv = dt_of(x) if dt is None else dt
    if TRACK_PLAN:
        LAST_PLAN = _lib.load().l2s_conv_plan_name(C.byref(d), dtv).decode()
    call('l2s_conv_igemm', C.byref(d), dtv, stream())
    return y


def roialign_block0_fwd(feat, H, W, C_, rois, R, P, spatial_scale, w1, b1, N1, w2, b2, N2, pooled, y1, y2, debug=0):
    """RoIAlign fused into layer4[0].conv1 (+ shift + ReLU) and layer4[0].downsample (+ shift): one launch, one workgroup per RoI (bf16)"""
    d = _lib.RoiBlock0Desc()
    d.feat, d.rois, d.w1, d.b1, d.w2, d.b2 = ptr(feat), ptr(rois), ptr(w1), ptr(b1), ptr(w2), ptr(b2)
    d.pooled, d.y1, d.y2 = ptr(pooled), ptr(y1), ptr(y2)
    d.H, d.W, d.C, d.R, d.P, d.N1, d.N2, d.spatial_scale = H, W, C_, R, P, N1, N2, float(spatial_scale)
    d.debug = debug
    call('l2s_roialign_block0_fwd', C.byref(d), stream())


def roialign_block0_ok(C_, P, N1, N2):
    """the fused kernel's shape requirements (include/lang2seg_hip.h)"""
    return P * P <= 64 and C_ % 128 == 0 and N1 % 128 == 0 and N2 % 128 == 0 and P * P * C_ * 2 + 4096 <= 160 * 1024


def _wgrad_desc(dy, x, dw, n_img, IH, IW, Cin, OH, OW, Cout, KH, KW, stride, pad, lddy, ldx, split_k, tile, ws):
    d = WgradDesc()
    d.dy, d.x, d.dw = ptr(dy), ptr(x), ptr(dw)
    d.n_img, d.IH, d.IW, d.Cin, d.OH, d.OW, d.Cout = n_img, IH, IW, Cin, OH, OW, Cout
    d.KH, d.KW, d.stride, d.pad = KH, KW, stride, pad
    d.lddy = Cout if lddy is None else lddy
    d.ldx = Cin if ldx is None else ldx
    d.split_k, d.tile = split_k, tile
    d.ws = ptr(ws)
    d.ws_bytes = 0 if ws is None else ws.numel() * ws.element_size()
    return d


def conv_wgrad(dy, x, dw, n_img, IH, IW, Cin, OH, OW, Cout, KH=1, KW=1, stride=1, pad=0, lddy=None, ldx=None,
               split_k=0, tile=0, ws=None):
    """dw += weight gradient.  `ws`: float workspace for the split-K slabs (summed in a fixed order by a second launch on the same
    stream: no float atomics); None = pixels are not split.  One workspace per stream that runs these launches."""
    d = _wgrad_desc(dy, x, dw, n_img, IH, IW, Cin, OH, OW, Cout, KH, KW, stride, pad, lddy, ldx, split_k, tile, ws)
    call('l2s_conv_wgrad', C.byref(d), dt_of(x), stream())
    return dw


def wgrad_ws_bytes(n_img, IH, IW, Cin, OH, OW, Cout, KH=1, KW=1, stride=1, pad=0, dt=BF16, split_k=0, tile=0):
    d = _wgrad_desc(None, None, None, n_img, IH, IW, Cin, OH, OW, Cout, KH, KW, stride, pad, None, None, split_k, tile, None)
    return int(_lib.load().l2s_wgrad_ws_bytes(C.byref(d), dt))


def weight_cast(src, scale, dst, Cout, taps, Cin):
    call('l2s_weight_cast', ptr(src), ptr(scale), ptr(dst), Cout, taps, Cin, dt_of(dst), stream())


def weight_transpose(src, scale, dst, Cout, taps, Cin):
    call('l2s_weight_transpose', ptr(src), ptr(scale), ptr(dst), Cout, taps, Cin, dt_of(dst), stream())


def weight_transpose_batched(table_dev, n, total_tiles, dt):
    call('l2s_weight_transpose_batched', ptr(table_dev), n, total_tiles, dt, stream())


def colsum(a, rows, cols, lda, out, ws=None):
    """out[c] += sum_r a[r][c].  ws (32 * cols floats, one per concurrent call site): tall matrices are summed in row ranges."""
    call('l2s_colsum', ptr(a), rows, cols, lda, ptr(out), ptr(ws), 0 if ws is None else ws.numel(), dt_of(a), stream())


def stem_pack(w, pack=None):
    """conv1's weights [64][7][7][3] f32 -> the bf16 fragment order of l2s_stem_pool_bf16 (into `pack` when given: recorded tapes hold its address)"""
    if pack is None:
        pack = torch.empty(int(_lib.load().l2s_stem_pack_bytes()), dtype=torch.uint8, device=w.device)
    call('l2s_stem_pack', ptr(w), ptr(pack), stream())
    return pack


def stem_pool_bf16(img, pack, scale, bias, y, H, W, OH, OW, PH, PW):
    call('l2s_stem_pool_bf16', ptr(img), ptr(pack), ptr(scale), ptr(bias), ptr(y), H, W, OH, OW, PH, PW, stream())


def stem_conv(img, w, scale, bias, y, H, W, OH, OW):
    call('l2s_stem_conv', ptr(img), ptr(w), ptr(scale), ptr(bias), ptr(y), H, W, OH, OW, dt_of(y), stream())


def scale_mask(x, mask, relu_ref, out):
    call('l2s_scale_mask', ptr(x), ptr(mask), ptr(relu_ref), ptr(out), x.numel(), dt_of(x), stream())


def conv3x3_c3(img, w, bias, y, H, W):
    call('l2s_conv3x3_c3', ptr(img), ptr(w), ptr(bias), ptr(y), H, W, dt_of(y), stream())


def maxpool2x2_fwd(x, y, n_img, IH, IW, Cc):
    call('l2s_maxpool2x2_fwd', ptr(x), ptr(y), n_img, IH, IW, Cc, dt_of(x), stream())


def maxpool2x2_bwd(dy, x, dx, n_img, IH, IW, Cc, relu_out):
    call('l2s_maxpool2x2_bwd', ptr(dy), ptr(x), ptr(dx), n_img, IH, IW, Cc, int(relu_out), dt_of(x), stream())


def maxpool(x, y, IH, IW, Cc, OH, OW):
    call('l2s_maxpool3x3s2', ptr(x), ptr(y), IH, IW, Cc, OH, OW, dt_of(x), stream())


# ------------------------------------------------------------------ elementwise / pooling
def fill(t, v):
    call('l2s_fill_f32', ptr(t), float(v), t.numel(), stream())


def cast(src, dst):
    call('l2s_cast', ptr(src), dt_of(src), ptr(dst), dt_of(dst), src.numel(), stream())


def add3(a, b, c, dst):
    call('l2s_add3', ptr(a), ptr(b), ptr(c), ptr(dst), a.numel(), dt_of(a), stream())


def avgpool_fwd(x, y, n_img, hw, Cc):
    call('l2s_avgpool_fwd', ptr(x), ptr(y), n_img, hw, Cc, dt_of(x), stream())


def avgpool_bwd(dy, dx, addend, ref, n_img, hw, Cc):
    call('l2s_avgpool_bwd', ptr(dy), ptr(dx), ptr(addend), ptr(ref), n_img, hw, Cc, dt_of(dy), stream())


def adaptive_pool_fwd(x, pixmask, y, H, W, Cc, OH, OW, ldy):
    call('l2s_adaptive_pool_fwd', ptr(x), ptr(pixmask), ptr(y), H, W, Cc, OH, OW, ldy, dt_of(x), stream())


def adaptive_pool_bwd(dy, lddy, off_all, off_mask, pixmask, dx, ref, H, W, Cc, OH, OW):
    call('l2s_adaptive_pool_bwd', ptr(dy), lddy, off_all, off_mask, ptr(pixmask), ptr(dx), ptr(ref), H, W, Cc, OH, OW,
         dt_of(dx), stream())


def mask_downsample(mask_u8, out, H, W, h, w):
    call('l2s_mask_downsample', ptr(mask_u8), ptr(out), H, W, h, w, stream())


def counter_inc(counter):
    call('l2s_counter_inc', ptr(counter), stream())


def stamp(buf, slot):
    """diagnostics: element `slot` of the int64 tensor `buf` receives the device clock (100 MHz) when the current stream gets here"""
    call('l2s_stamp', buf.data_ptr() + 8 * int(slot), stream())


def dropout_mask(mask, p, seed_dev, salt):
    call('l2s_dropout_mask', ptr(mask), mask.numel(), float(p), ptr(seed_dev), int(salt), stream())


def random_keys(keys, seed_dev, salt):
    call('l2s_random_keys', ptr(keys), keys.numel(), ptr(seed_dev), int(salt), stream())


# ------------------------------------------------------------------ RoI path
def rpn_decode(heads, ldh, base_anchors, H, W, A, fs, im_h, im_w, prob, boxes, scores):
    call('l2s_rpn_decode', ptr(heads), ldh, ptr(base_anchors), H, W, A, fs, float(im_h), float(im_w), ptr(prob), ptr(boxes),
         ptr(scores), stream())


def sort_ws_ints(n):
    return int(_lib.load().l2s_sort_ws_ints(n))


def sort_topk(scores, boxes, n, k, ws, sboxes, sscores, sidx):
    call('l2s_sort_topk', ptr(scores), ptr(boxes), n, k, ptr(ws), ptr(sboxes), ptr(sscores), ptr(sidx), stream())


def nms_workspace_bytes(n):
    return int(_lib.load().l2s_nms_workspace_bytes(n))


def nms(sboxes, n, thresh, cmp_mode, max_keep, mask_ws, keep, num):
    call('l2s_nms', ptr(sboxes), n, float(thresh), cmp_mode, max_keep, ptr(mask_ws), ptr(keep), ptr(num), stream())


def gather_rois(sboxes, sscores, keep, num, max_keep, rois, roi_scores):
    call('l2s_gather_rois', ptr(sboxes), ptr(sscores), ptr(keep), ptr(num), max_keep, ptr(rois), ptr(roi_scores), stream())


def anchor_target_ws_ints(hwa):
    return int(_lib.load().l2s_anchor_target_ws_ints(hwa))


def anchor_target(gt, n_gt, base_anchors, H, W, A, fs, im_h, im_w, fg_keys, bg_keys, neg_ov, pos_ov, batch, fg_frac,
                  labels, targets, inw, outw, ws):
    call('l2s_anchor_target', ptr(gt), n_gt, ptr(base_anchors), H, W, A, fs, float(im_h), float(im_w), ptr(fg_keys),
         ptr(bg_keys), float(neg_ov), float(pos_ov), batch, float(fg_frac), ptr(labels), ptr(targets), ptr(inw),
         ptr(outw), ptr(ws), stream())


def proposal_target(rois, roi_scores, n_rois, n_max, gt, n_gt, gt_masks, im_h, im_w, fg_keys, bg_keys, bg_rand, R, fg_max, mask_slots,
                    fg_thresh, bg_hi, bg_lo, means4, stds4, inw4, ncls, ms, out_rois, labels, bt, bi, bo, mt, counts, ws):
    call('l2s_proposal_target', ptr(rois), ptr(roi_scores), ptr(n_rois), n_max, ptr(gt), n_gt, ptr(gt_masks), im_h, im_w,
         ptr(fg_keys), ptr(bg_keys), ptr(bg_rand), R, fg_max, mask_slots, float(fg_thresh), float(bg_hi), float(bg_lo), ptr(means4),
         ptr(stds4), ptr(inw4), ncls, ms, ptr(out_rois), ptr(labels), ptr(bt), ptr(bi), ptr(bo), ptr(mt), ptr(counts),
         ptr(ws), stream())


def roialign_fwd(feat, H, W, Cc, rois, R, P, sscale, out):
    call('l2s_roialign_fwd', ptr(feat), H, W, Cc, ptr(rois), R, P, float(sscale), ptr(out), dt_of(feat), stream())


def roialign_bwd(dout, H, W, Cc, rois, R, P, sscale, dfeat):
    call('l2s_roialign_bwd', ptr(dout), H, W, Cc, ptr(rois), R, P, float(sscale), ptr(dfeat), dt_of(dout), stream())


# ------------------------------------------------------------------ losses
def rpn_loss(heads, ldh, labels, targets, inw, outw, H, W, A, sigma, gscale, loss, dheads, ldd, atl_ws=None):
    """atl_ws: the anchor-target workspace (its sampled-anchor count is reused); otherwise the labels are counted."""
    if atl_ws is not None:
        cnt, cws = ptr(atl_ws) + 8, None
    else:
        cws = torch.zeros(1, dtype=torch.int32, device=heads.device)
        cnt, cws = None, ptr(cws)
    call('l2s_rpn_loss', ptr(heads), ldh, ptr(labels), ptr(targets), ptr(inw), ptr(outw), H, W, A, float(sigma), float(gscale),
         ptr(loss), ptr(dheads), ldd, dt_of(dheads), cnt, cws, stream())


def rcnn_loss(heads, ldh, labels, bt, bi, bo, R, ncls, gscale, loss, dheads, ldd):
    call('l2s_rcnn_loss', ptr(heads), ldh, ptr(labels), ptr(bt), ptr(bi), ptr(bo), R, ncls, float(gscale), ptr(loss),
         ptr(dheads), ldd, dt_of(dheads), stream())


def mask_loss(score, ldsc, labels, mt, num_fg, fg_max, ms2, gscale, loss, dscore):
    call('l2s_mask_loss', ptr(score), ldsc, ptr(labels), ptr(mt), ptr(num_fg), fg_max, ms2, float(gscale), ptr(loss),
         ptr(dscore), stream())


def total_loss(loss, cap_w):
    call('l2s_total_loss', ptr(loss), float(cap_w), stream())


def maskpred_bwd(dscore, labels, num_fg, fg_max, ms2, Cc, w, x, ref, dx, dw, db, ws=None):
    if ws is None:                                   # per-(RoI, pixel chunk) partial sums
        ws = torch.empty(int(_lib.load().l2s_maskpred_ws_floats(fg_max, Cc)), dtype=torch.float32, device=dx.device)
    call('l2s_maskpred_bwd', ptr(dscore), ptr(labels), ptr(num_fg), fg_max, ms2, Cc, ptr(w), ptr(x), ptr(ref), ptr(dx),
         ptr(dw), ptr(db), ptr(ws), dt_of(x), stream())


def maskpred_bwd_dx(dscore, labels, num_fg, fg_max, ms2, Cc, w, x, ref, dx, ws):
    """the first launch of maskpred_bwd: dx and the per-(RoI, pixel chunk) partial sums into ws"""
    call('l2s_maskpred_bwd_dx', ptr(dscore), ptr(labels), ptr(num_fg), fg_max, ms2, Cc, ptr(w), ptr(x), ptr(ref), ptr(dx), ptr(ws), dt_of(x), stream())


def maskpred_bwd_reduce(ws, labels, num_fg, fg_max, Cc, dw, db):
    """the second: dW / db from ws, per label in RoI order (on the current stream: the caller puts it on a weight-gradient stream)"""
    call('l2s_maskpred_bwd_reduce', ptr(ws), ptr(labels), ptr(num_fg), fg_max, Cc, ptr(dw), ptr(db), stream())


# ------------------------------------------------------------------ language side (fp32)
def linear_fwd(x, w, b, y, M, N, K, act=0, accumulate=False, ldx=None, ldy=None, ldw=None):
    call('l2s_linear_fwd', ptr(x), K if ldx is None else ldx, ptr(w), K if ldw is None else ldw, ptr(b), ptr(y),
         N if ldy is None else ldy, M, N, K, act, 1 if accumulate else 0, stream())


def linear_bwd_x(dy, w, dx, M, N, K, accumulate=False, lddy=None, lddx=None, mul=None, ws=None):
    """dx[M][K] (+)= (dy[M][N] . w[N][K]) (* mul); ws: float tensor of linear_bwd_x_ws_floats(M, N, K) for the split contraction"""
    call('l2s_linear_bwd_x', ptr(dy), N if lddy is None else lddy, ptr(w), ptr(dx), K if lddx is None else lddx, M, N, K,
         1 if accumulate else 0, ptr(mul), ptr(ws), 0 if ws is None else ws.numel(), stream())


def linear_bwd_x_ws_floats(M, N, K):
    return int(_lib.load().l2s_linear_bwd_x_ws_floats(M, N, K))


def linear_bwd_w(dy, x, dw, db, M, N, K, lddy=None, ldx=None):
    call('l2s_linear_bwd_w', ptr(dy), N if lddy is None else lddy, ptr(x), K if ldx is None else ldx, ptr(dw), ptr(db), M, N,
         K, stream())


def mask_relu_cast(x, mul, relu_ref, out):
    """x *= mul (optional); x = 0 where relu_ref <= 0; out = x in out's dtype (one launch)"""
    call('l2s_mask_relu_cast', ptr(x), ptr(mul), ptr(relu_ref), ptr(out), dt_of(out), x.numel(), stream())


def act_bwd(dy, y, act):
    call('l2s_act_bwd', ptr(dy), ptr(y), dy.numel(), act, stream())


def embed_fwd(table, ids, mask, out, T, D, relu):
    call('l2s_embed_fwd', ptr(table), ptr(ids), ptr(mask), ptr(out), T, D, 1 if relu else 0, stream())


def embed_bwd(dout, out, ids, mask, dtable, T, D, relu):
    call('l2s_embed_bwd', ptr(dout), ptr(out), ptr(ids), ptr(mask), ptr(dtable), T, D, 1 if relu else 0, stream())


def lstm_cell_fwd(gates, c_prev, c, h, act, Hh):
    call('l2s_lstm_cell_fwd', ptr(gates), ptr(c_prev), ptr(c), ptr(h), ptr(act), Hh, stream())


def lstm_cell_bwd(dh, dc_in, act, c_prev, c, dgates, dc_prev, Hh):
    call('l2s_lstm_cell_bwd', ptr(dh), ptr(dc_in), ptr(act), ptr(c_prev), ptr(c), ptr(dgates), ptr(dc_prev), Hh, stream())


def lstm_step_fwd(dirs, Hh):
    """dirs: list (1 or 2) of dicts with the l2s_lstm_fwd_dir fields (tensors)."""
    arr = (_lib.LstmFwdDir * len(dirs))()
    for i, d in enumerate(dirs):
        for k, _ in _lib.LstmFwdDir._fields_:
            setattr(arr[i], k, ptr(d[k]))
    call('l2s_lstm_step_fwd', arr, len(dirs), Hh, stream())


def lstm_step_bwd(dirs, Hh):
    arr = (_lib.LstmBwdDir * len(dirs))()
    for i, d in enumerate(dirs):
        for k, _ in _lib.LstmBwdDir._fields_:
            setattr(arr[i], k, ptr(d.get(k)))
    call('l2s_lstm_step_bwd', arr, len(dirs), Hh, stream())


def _step(entry, struct, dirs, Hh):
    arr = (struct * len(dirs))()
    for i, d in enumerate(dirs):
        for k, _ in struct._fields_:
            setattr(arr[i], k, ptr(d.get(k)))
    call(entry, arr, len(dirs), Hh, stream())


def gru_step_fwd(dirs, Hh):
    """dirs: list (1 or 2) of dicts with the l2s_gru_fwd_dir fields (tensors)"""
    _step('l2s_gru_step_fwd', _lib.GruFwdDir, dirs, Hh)


def gru_step_bwd(dirs, Hh):
    """l2s_gru_bwd_dir fields; dgh_next / dh_ext / dh_carry_in may be missing or None"""
    _step('l2s_gru_step_bwd', _lib.GruBwdDir, dirs, Hh)


def rnn_step_fwd(dirs, Hh):
    _step('l2s_rnn_step_fwd', _lib.RnnFwdDir, dirs, Hh)


def rnn_step_bwd(dirs, Hh):
    _step('l2s_rnn_step_bwd', _lib.RnnBwdDir, dirs, Hh)


def _topdown_segs(arr, segs):
    for q, sg in zip(arr, segs):
        if sg is not None:
            x, w, ld, n = sg
            q.x, q.w, q.ld, q.n = ptr(x), ptr(w), int(ld), int(n)


def topdown_cell_fwd(pre, add0, add1, segs, c_prev, c, h, act, R):
    """one nn.LSTMCell step (csrc/caption_step.hip): gates = pre + add0 + add1 + sum over segs (x[n], w, ld, n) of w[4R][:n] . x, with w a
    column block (leading dimension ld) of a wider matrix; writes h, c and act[4R] = i, f, g, o.  Up to two segments; None entries are skipped."""
    a = _lib.TopdownFwd()
    a.pre, a.add0, a.add1, a.c_prev, a.c, a.h, a.act = ptr(pre), ptr(add0), ptr(add1), ptr(c_prev), ptr(c), ptr(h), ptr(act)
    assert len(segs) <= 2
    _topdown_segs(a.seg, segs)
    call('l2s_topdown_cell_fwd', C.byref(a), int(R), stream())


def topdown_cell_bwd(segs, add0, add1, dc_in, act, c_prev, c, dgates, dc_prev, R):
    """the matching backward step: dh = add0 + add1 + sum over segs (v[n], wT, ld, n) of wT[R][:n] . v (blocks of transposed copies), then
    dgates[4R] and dc_prev[R].  Up to three segments."""
    a = _lib.TopdownBwd()
    a.add0, a.add1, a.dc_in, a.act, a.c_prev, a.c, a.dgates, a.dc_prev = (ptr(add0), ptr(add1), ptr(dc_in), ptr(act), ptr(c_prev), ptr(c),
                                                                           ptr(dgates), ptr(dc_prev))
    assert len(segs) <= 3
    _topdown_segs(a.seg, segs)
    call('l2s_topdown_cell_bwd', C.byref(a), int(R), stream())


def cap_att_apply_fwd(att, dots, L, R, weight, att_res):
    """weight[L] = softmax(dots), att_res[R] = weight . att[L][R]"""
    call('l2s_cap_att_apply_fwd', ptr(att), ptr(dots), L, R, ptr(weight), ptr(att_res), stream())


def cap_att_bwd_step_centered(dweight, tanh_ws, weight, aw, L, D, ddot, datt_h):
    """cap_attention_bwd_step2 with the sum over the locations centred on its weighted mean (csrc/caption_step.hip)"""
    call('l2s_cap_att_bwd_step_centered', ptr(dweight), ptr(tanh_ws), ptr(weight), ptr(aw), L, D, ptr(ddot), ptr(datt_h), stream())


def pack_rows(dst, ldd, src, lds, rows, cols):
    """dst[r][:cols] = src[r][:cols] (leading dimensions ldd / lds; lds = 0 repeats one source row)"""
    call('l2s_pack_rows', ptr(dst), int(ldd), ptr(src), int(lds), int(rows), int(cols), stream())


def adaatt_cell_fwd(pre, fcrow, w_hh, b_hh, w_r, b_r, h_prev, c_prev, c, h, fake, save, R, G, ld_hh=None, ld_r=None):
    """one token of the adaptive-attention cell (csrc/adaatt_step.hip): sums = pre + fcrow + w_hh h_prev + b_hh (G row blocks: in, forget, out,
    transform; G = 5: the max of two transforms), n5 = the row after them + w_r h_prev + b_r; writes c, h, fake = sigmoid(n5) tanh(c), save[7R]"""
    a = _lib.AdaattFwd()
    a.pre, a.fcrow, a.w_hh, a.b_hh, a.w_r, a.b_r = ptr(pre), ptr(fcrow), ptr(w_hh), ptr(b_hh), ptr(w_r), ptr(b_r)
    a.ld_hh, a.ld_r = int(R if ld_hh is None else ld_hh), int(R if ld_r is None else ld_r)
    a.h_prev, a.c_prev, a.c, a.h, a.fake, a.save = ptr(h_prev), ptr(c_prev), ptr(c), ptr(h), ptr(fake), ptr(save)
    call('l2s_adaatt_cell_fwd', C.byref(a), int(R), int(G), stream())


def adaatt_cell_bwd(dsn, t_hh, t_r, dh_ext, dfake, dc_in, save, c_prev, ds, dc_prev, R, G, ld_thh=None, ld_tr=None):
    """its backward: dh = dh_ext + the unit's rows of the transposed copies t_hh [R][G R] / t_r [R][R] with dsn = d(sums | n5) of the next token
    (None at the last); writes ds[(G+1) R] = d(sums | n5) and dc_prev"""
    a = _lib.AdaattBwd()
    a.dsn, a.t_hh, a.t_r, a.ld_thh, a.ld_tr = ptr(dsn), ptr(t_hh), ptr(t_r), int(G * R if ld_thh is None else ld_thh), int(R if ld_tr is None else ld_tr)
    a.dh_ext, a.dfake, a.dc_in, a.save, a.c_prev, a.ds, a.dc_prev = ptr(dh_ext), ptr(dfake), ptr(dc_in), ptr(save), ptr(c_prev), ptr(ds), ptr(dc_prev)
    call('l2s_adaatt_cell_bwd', C.byref(a), int(R), int(G), stream())


def adaatt_att_fwd(att, patt, frl, fre, hoe, hol, aw, ab, mask, S, L, R, tanh_ws, dots, PI, atten):
    """the attention over L + 1 slots (slot 0 = sentinel) for S tokens: tanh_ws[S][L+1][R], dots[S][256], PI[S][L+1], atten[S][R]"""
    call('l2s_adaatt_att_fwd', ptr(att), ptr(patt), ptr(frl), ptr(fre), ptr(hoe), ptr(hol), ptr(aw), ptr(ab), ptr(mask), int(S), int(L), int(R),
         ptr(tanh_ws), ptr(dots), ptr(PI), ptr(atten), stream())


def adaatt_att_bwd_step(datten, att, frl, tanh_ws, mask, PI, aw, S, L, R, ddot, dhoe, dfre, dctx, dfrl, dhol):
    """what flows from d(atten)[S][R] on to the cell: ddot[S][L+1], d(hoe), d(fre), dctx = d(hoe) - d(fre), d(frl) = PI[0] datten, d(hol) = datten"""
    call('l2s_adaatt_att_bwd_step', ptr(datten), ptr(att), ptr(frl), ptr(tanh_ws), ptr(mask), ptr(PI), ptr(aw), int(S), int(L), int(R),
         ptr(ddot), ptr(dhoe), ptr(dfre), ptr(dctx), ptr(dfrl), ptr(dhol), stream())


def adaatt_att_bwd_batched(ddot, PI, datten, tanh_ws, mask, aw, S, L, R, dpatt, datt, daw):
    """the sums over the tokens: dpatt[L][R] +=, datt[L][R] +=, daw[R] +="""
    call('l2s_adaatt_att_bwd_batched', ptr(ddot), ptr(PI), ptr(datten), ptr(tanh_ws), ptr(mask), ptr(aw), int(S), int(L), int(R),
         ptr(dpatt), ptr(datt), ptr(daw), stream())


def rnn_concat_fwd(hs, mask, out, T, Hh):
    """out[T][len(hs) Hh] = the directions' [T][Hh] states side by side (* mask)"""
    call('l2s_rnn_concat_fwd', ptr(hs[0]), ptr(hs[1]) if len(hs) > 1 else None, ptr(mask), ptr(out), T, Hh, len(hs), stream())


def rnn_concat_bwd(dx, mask, adds, ds, T, Hh):
    """ds[dir][T][Hh] = the halves of dx[T][len(ds) Hh] (* mask), adds[dir] ([Hh] or None) added at the direction's last processed row"""
    call('l2s_rnn_concat_bwd', ptr(dx), ptr(mask), ptr(adds[0]), ptr(adds[1]) if len(ds) > 1 else None, ptr(ds[0]),
         ptr(ds[1]) if len(ds) > 1 else None, T, Hh, len(ds), stream())


def dynfilter_fwd(x, filt, r, y, resp, respk, H, W, Cc, gate=0):
    call('l2s_dynfilter_fwd', ptr(x), ptr(filt), ptr(r), ptr(y), ptr(resp), ptr(respk), H, W, Cc, dt_of(x), int(gate), stream())


def dynfilter_ws_floats(H, W, Cc):
    return int(_lib.load().l2s_dynfilter_ws_floats(H, W, Cc))


def dynfilter_bwd(dy, x, filt, r, resp, respk, dx, ref, dfilt, dr, dresp_ws, H, W, Cc, gate=0, dresp_extra=None):
    assert dresp_ws.numel() >= dynfilter_ws_floats(H, W, Cc)
    call('l2s_dynfilter_bwd', ptr(dy), ptr(x), ptr(filt), ptr(r), ptr(resp), ptr(respk), ptr(dx), ptr(ref), ptr(dfilt),
         ptr(dr), ptr(dresp_ws), H, W, Cc, dt_of(x), int(gate), ptr(dresp_extra), stream())


def dynfilter_bwd_finish(dresp_ws, respk, dfilt, dr, H, W, Cc):
    """the part of dynfilter_bwd that only the language-side backward needs (dfilt +=, dr +=); dynfilter_bwd was called with dfilt=None"""
    call('l2s_dynfilter_bwd_finish', ptr(dresp_ws), ptr(respk), ptr(dfilt), ptr(dr), H, W, Cc, stream())


def roipool_fwd(feat, H, W, Cc, rois, R, P, scale, out, argmax):
    call('l2s_roipool_fwd', ptr(feat), H, W, Cc, ptr(rois), R, P, float(scale), ptr(out), ptr(argmax), dt_of(feat), stream())


def cropalign_fwd(feat, H, W, Cc, rois, R, P, im_h, im_w, out):
    call('l2s_cropalign_fwd', ptr(feat), H, W, Cc, ptr(rois), R, P, float(im_h), float(im_w), ptr(out), dt_of(feat), stream())


def cropalign_bwd(dout, H, W, Cc, rois, R, P, im_h, im_w, dfeat):
    call('l2s_cropalign_bwd', ptr(dout), H, W, Cc, ptr(rois), R, P, float(im_h), float(im_w), ptr(dfeat), dt_of(dout), stream())


def roipool_bwd(dout, argmax, R, P, Cc, dfeat):
    call('l2s_roipool_bwd', ptr(dout), ptr(argmax), R, P, Cc, ptr(dfeat), dt_of(dout), stream())


# ------------------------------------------------------------------ input side (loaders)
def rle_from_string(s):
    """COCO compressed RLE string -> uint32 run lengths (host; maskApi.c:217-231)."""
    import numpy as np
    b = s.encode('ascii') if isinstance(s, str) else bytes(s)
    buf = np.empty(max(len(b), 1), np.uint32)
    m = _lib.load().l2s_rle_from_string(b, buf.ctypes.data, buf.size)
    if m < 0:
        raise ValueError('malformed run-length string')
    return buf[:m].copy()


def prep_geometry(h, w, target_size, max_size):
    """(im_scale, out_h, out_w) of prep_im_for_blob (host; blob.py:35-45)."""
    sc, oh, ow = C.c_double(), C.c_int(), C.c_int()
    call('l2s_prep_geometry', int(h), int(w), int(target_size), int(max_size), C.byref(sc), C.byref(oh), C.byref(ow))
    return sc.value, oh.value, ow.value


def prep_image(img_u8, means, scale, out):
    """img_u8 uint8 [h][w][3] BGR (device) -> out float32 [oh][ow][3]."""
    h, w = img_u8.shape[0], img_u8.shape[1]
    call('l2s_prep_image', ptr(img_u8), h, w, float(means[0]), float(means[1]), float(means[2]), float(scale),
         out.shape[0], out.shape[1], ptr(out), stream())


def rle_ws_words(total_counts, oh, ow):
    return int(_lib.load().l2s_rle_ws_words(total_counts, oh, ow))


def rle_to_mask(cnts, offs, n, total, h, w, ws, out):
    """cnts uint32 / offs int32 (device) -> out uint8 [oh][ow]."""
    call('l2s_rle_to_mask', ptr(cnts), ptr(offs), n, total, h, w, out.shape[0], out.shape[1], ptr(ws), ptr(out), stream())


def rle_encode_ws_words(h, w):
    return int(_lib.load().l2s_rle_encode_ws_words(int(h), int(w)))


def rle_encode_chunk_rows():
    return int(_lib.load().l2s_rle_encode_chunk_rows())


def rle_from_mask(mask, pool, cursor, span, ws):
    """mask uint8 [h][w] (device, nonzero = 1) -> its run lengths appended to `pool` (uint32) at *cursor (int32 [1]); span (int32 [2]) takes
    (offset, n), or (-1, n needed) with pool and cursor untouched when they do not fit.  ws: rle_encode_ws_words(h, w) uint32.  No host sync."""
    h, w = mask.shape[-2], mask.shape[-1]
    if ws.numel() < rle_encode_ws_words(h, w):
        raise ValueError('rle_from_mask: workspace of %d words, %d needed' % (ws.numel(), rle_encode_ws_words(h, w)))
    call('l2s_rle_from_mask', ptr(mask), h, w, ptr(pool), pool.numel(), ptr(cursor), ptr(span), ptr(ws), stream())


def rle_to_string(cnts):
    """uint32 run lengths -> COCO compressed RLE string (host; maskApi.c:203-215)."""
    import numpy as np
    c = np.ascontiguousarray(cnts, dtype=np.uint32)
    buf = C.create_string_buffer(7 * c.size + 1)               # a 32-bit difference takes at most 7 characters of 5 bits
    m = _lib.load().l2s_rle_to_string(c.ctypes.data, c.size, buf, len(buf))
    if m < 0:
        raise ValueError('rle_to_string: buffer too small')
    return buf.raw[:m].decode('ascii')


def mask_to_rle(mask_dev):
    """uint8 [h][w] device mask -> {'size': [h, w], 'counts': str}, the COCO form of the reference's mask.encode (one read-back)"""
    h, w = int(mask_dev.shape[-2]), int(mask_dev.shape[-1])
    dev = mask_dev.device
    pool = torch.empty((h * w + 1,), dtype=torch.int32, device=dev)
    cs = torch.zeros((3,), dtype=torch.int32, device=dev)      # cursor, span
    ws = torch.empty((rle_encode_ws_words(h, w),), dtype=torch.int32, device=dev)
    rle_from_mask(mask_dev.contiguous(), pool, cs[0:1], cs[1:3], ws)
    off, n = (int(v) for v in cs[1:3].cpu())
    assert off == 0, (off, n)
    return dict(size=[h, w], counts=rle_to_string(pool[:n].cpu().numpy().view('<u4')))


EVAL_RECORD_BYTES = 48     # l2s_eval_record: roi, cls (int32), box[4] (f32), hit, reserved (int32), I, U (int64)


def eval_records(n, device='cuda'):
    """a zeroed device array of n l2s_eval_record (int64 [n][6]; eval_record_fields() reads it on the host)"""
    return torch.zeros((n, EVAL_RECORD_BYTES // 8), dtype=torch.int64, device=device)


def eval_record_fields(rec):
    """host int64 [n][6] records -> (roi, cls, box [n][4] f32, hit, I, U) numpy arrays"""
    a = rec.numpy() if isinstance(rec, torch.Tensor) else rec
    i32 = a.view('<i4').reshape(a.shape[0], -1)
    return i32[:, 0], i32[:, 1], i32[:, 2:6].view('<f4'), i32[:, 6], a[:, 4], a[:, 5]


def eval_pick(cls_prob, bbox_pred, rois, nkeep, post, ncls, im_scale, im_h, im_w, gt_box, bbox_reg, rec, i, mask_roi, mask_label):
    """model/test.py best_detection + detect_from_outputs + computeIoU_box on the device -> record i of `rec`, the mask head's RoI / label"""
    call('l2s_eval_pick', ptr(cls_prob), ptr(bbox_pred), ptr(rois), ptr(nkeep), post, ncls, float(im_scale), im_h, im_w, ptr(gt_box),
         1 if bbox_reg else 0, ptr(rec) + i * EVAL_RECORD_BYTES, ptr(mask_roi), ptr(mask_label), stream())


def eval_mask_iou(mask_prob, rec, i, gt, ih, iw, canvas=None):
    """segment_from_mask_prob + nearest gt resize + computeIoU_seg on the device: adds I, U to record i (gt: uint8 [Hs][Ws])"""
    ms = mask_prob.shape[-1]
    call('l2s_eval_mask_iou', ptr(mask_prob), ms, ptr(rec) + i * EVAL_RECORD_BYTES, ptr(gt), gt.shape[-2], gt.shape[-1], ih, iw,
         ptr(canvas), stream())


def rle_from_masks(masks, n_valid, pool, cursor, spans, ws):
    """rle_from_mask for masks uint8 [n][h][w] in three launches: the first *n_valid (device int32 [1]) masks in order, spans int32 [n][2]
    (skipped masks: (0, 0)); ws: n * rle_encode_ws_words(h, w) uint32.  No host sync."""
    n, h, w = masks.shape
    if ws.numel() < n * rle_encode_ws_words(h, w) or spans.numel() < 2 * n:
        raise ValueError('rle_from_masks: workspace of %d words, %d needed (spans %d of %d)' % (ws.numel(), n * rle_encode_ws_words(h, w), spans.numel(), 2 * n))
    call('l2s_rle_from_masks', ptr(masks), n, ptr(n_valid), h, w, ptr(pool), pool.numel(), ptr(cursor), ptr(spans), ptr(ws), stream())


DET_RECORD_BYTES = 32      # l2s_det_record: roi, cls (int32), box[4], score (f32), area (int32)


def det_record_fields(rec):
    """host int32 [n][8] detection records -> (roi, cls, box [n][4] f32, score f32, area) numpy arrays"""
    a = rec.numpy() if isinstance(rec, torch.Tensor) else rec
    a = a.reshape(-1, DET_RECORD_BYTES // 4)
    return a[:, 0], a[:, 1], a[:, 2:6].view('<f4'), a[:, 6].view('<f4'), a[:, 7]


def detect_ws_bytes(post, ncls):
    return int(_lib.load().l2s_detect_ws_bytes(int(post), int(ncls)))


def detect_nms(cls_prob, bbox_pred, rois, nkeep, post, ncls, im_scale, im_h, im_w, bbox_reg, thresh, nms_thresh, ws, boxes_dump=None):
    """class-wise NMS of one sentence's head outputs (one workgroup per class) -> the kept lists in ws (detect_ws_bytes(post, ncls) bytes);
    boxes_dump: optional float32 [post][ncls][4], every decoded box"""
    if ws.numel() * ws.element_size() < detect_ws_bytes(post, ncls):
        raise ValueError('detect_nms: workspace of %d bytes, %d needed' % (ws.numel() * ws.element_size(), detect_ws_bytes(post, ncls)))
    if boxes_dump is not None and boxes_dump.numel() < post * ncls * 4:
        raise ValueError('detect_nms: boxes_dump of %d floats, %d needed' % (boxes_dump.numel(), post * ncls * 4))
    call('l2s_detect_nms', ptr(cls_prob), ptr(bbox_pred), ptr(rois), ptr(nkeep), post, ncls, float(im_scale), im_h, im_w, 1 if bbox_reg else 0,
         float(thresh), float(nms_thresh), ptr(ws), ptr(boxes_dump), stream())


def detect_select(ws, post, ncls, max_per_image, im_scale, rec, mask_rois, mask_labels, cap, count):
    """the top-N rule over all classes and the compaction in class order: rec int32 [cap][8], mask_rois f32 [cap][5], mask_labels int32 [cap],
    count int32 [2] = (written, total)"""
    if rec.numel() * rec.element_size() < cap * DET_RECORD_BYTES or mask_rois.numel() < 5 * cap or mask_labels.numel() < cap or count.numel() < 2:
        raise ValueError('detect_select: an output is smaller than cap = %d rows' % cap)
    call('l2s_detect_select', ptr(ws), post, ncls, int(max_per_image), float(im_scale), ptr(rec), ptr(mask_rois), ptr(mask_labels), cap, ptr(count),
         stream())


def detect_paste(mask_prob, rec, count, ih, iw, canvases):
    """recover_masks + > 122 of mask_prob f32 [cap][ms][ms] on the records' boxes -> canvases uint8 [cap][ih][iw], areas added to the records;
    only the first count[0] detections"""
    cap, ms = mask_prob.shape[0], mask_prob.shape[-1]
    if canvases.numel() < cap * ih * iw or rec.numel() * rec.element_size() < cap * DET_RECORD_BYTES:
        raise ValueError('detect_paste: canvases or records smaller than cap = %d' % cap)
    call('l2s_detect_paste', ptr(mask_prob), ms, ptr(rec), ptr(count), cap, ih, iw, ptr(canvases), stream())


# ------------------------------------------------------------------ judging the detections (csrc/select.hip)
DET_GT_BYTES = 16          # l2s_det_gt: I, U, hit, reserved (int32)
DET_CHOICE_BYTES = 40      # l2s_det_choice: det, cls, hit, reserved (int32), I, U (int64), key (float64)
DET_MAX_LAMBDA = 8
_DET_GT = [('I', '<i4'), ('U', '<i4'), ('hit', '<i4'), ('reserved', '<i4')]
_DET_CHOICE = [('det', '<i4'), ('cls', '<i4'), ('hit', '<i4'), ('reserved', '<i4'), ('I', '<i8'), ('U', '<i8'), ('key', '<f8')]


def _records(rec, fields, nbytes):
    import numpy as np
    a = rec.numpy() if isinstance(rec, torch.Tensor) else np.asarray(rec)
    a = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    if a.size % nbytes:
        raise ValueError('%d bytes are no whole number of %d-byte records' % (a.size, nbytes))
    return a.view(np.dtype(fields))


def det_gt_fields(rec):
    """host l2s_det_gt rows (any integer array of n * 16 bytes) -> (I, U, hit) numpy int32 arrays"""
    a = _records(rec, _DET_GT, DET_GT_BYTES)
    return a['I'], a['U'], a['hit']


def det_choice_fields(rec):
    """host l2s_det_choice rows (any integer array of n * 40 bytes) -> (det, cls, hit, I, U, key): int32 x 3, int64 x 2, float64"""
    a = _records(rec, _DET_CHOICE, DET_CHOICE_BYTES)
    return a['det'], a['cls'], a['hit'], a['I'], a['U'], a['key']


def detect_gt_iou(canvases, rec, count, gt, gt_box, im_scale, out, gt_area, clear=True):
    """every detection d < count[0] of canvases uint8 [cap][ih][iw] against the gt mask uint8 [Hs][Ws] (PIL NEAREST resized to the canvas)
    and the gt box f32 [4] (scaled image): out int32 [cap][4] (l2s_det_gt: I, U, hit), gt_area int32 [1].  The kernel accumulates:
    clear=False only for outputs that are zero already"""
    cap, ih, iw = canvases.shape
    if rec.numel() * rec.element_size() < cap * DET_RECORD_BYTES or out.numel() * out.element_size() < cap * DET_GT_BYTES or gt_area.numel() < 1:
        raise ValueError('detect_gt_iou: records or outputs smaller than cap = %d' % cap)
    if gt.dim() != 2 or gt.dtype != torch.uint8 or not gt.is_contiguous() or gt_box.numel() < 4:
        raise ValueError('detect_gt_iou: gt is a contiguous uint8 [Hs][Ws] mask and gt_box 4 floats, got %s %s' % (tuple(gt.shape), gt.dtype))
    if clear:
        memset_zero(out)
        memset_zero(gt_area)
    call('l2s_detect_gt_iou', ptr(canvases), ptr(rec), ptr(count), cap, ih, iw, ptr(gt), gt.shape[0], gt.shape[1], ptr(gt_box), float(im_scale),
         ptr(out), ptr(gt_area), stream())


def detect_choose(rec, gt_rows, count, cap, gt_area, out, expr=None, lambdas=(), per_token=False, n_tok=1):
    """one detection per rule: out (2 + (1 + len(lambdas) if expr is given) l2s_det_choice records of 40 bytes, 8-byte aligned) =
    detector, oracle[, speaker, rerank@lambda ...]; expr: device f32 [cap] (caption_score_rows' score)"""
    lam = [float(v) for v in lambdas]
    n_rules = 2 + (1 + len(lam) if expr is not None else 0)
    if out.numel() * out.element_size() < n_rules * DET_CHOICE_BYTES or out.data_ptr() % 8:
        raise ValueError('detect_choose: %d choice records need %d bytes, 8-byte aligned' % (n_rules, n_rules * DET_CHOICE_BYTES))
    if expr is not None and (expr.dtype != torch.float32 or expr.numel() < cap):
        raise ValueError('detect_choose: expr is float32 [cap = %d]' % cap)
    arr = (C.c_float * max(len(lam), 1))(*lam)
    call('l2s_detect_choose', ptr(rec), ptr(gt_rows), ptr(count), cap, ptr(gt_area), ptr(expr), arr, len(lam), 1 if per_token else 0, int(n_tok),
         ptr(out), stream())


# ------------------------------------------------------------------ caption decoding (csrc/decode.hip)
BEAM_MAX, BEAM_MAX_T = 16, 64


def decode_pick(logits, V1, t, sample_max, temperature, u, seed_dev, salt, finished, seq, seq_logprobs, next_token):
    """one decision of AttModel.sample on logits f32 [V1]: argmax (sample_max) or an inverse-CDF draw with u[t] (u f32 [T], injected) or the
    counter hash of (seed_dev, salt, t); finished int32 [1], seq int64 [T], seq_logprobs f32 [T], next_token int64 [1]"""
    if logits.numel() < V1 or seq.numel() <= t or seq_logprobs.numel() <= t or (u is not None and u.numel() <= t):
        raise ValueError('decode_pick: a buffer is smaller than V1 = %d / t = %d asks' % (V1, t))
    call('l2s_decode_pick', ptr(logits), int(V1), int(t), 1 if sample_max else 0, float(temperature), ptr(u), ptr(seed_dev), int(salt),
         ptr(finished), ptr(seq), ptr(seq_logprobs), ptr(next_token), stream())


def beam_record_words(T):
    return 2 * T + 2


def decode_beam_step(logits, V1, B, t, T, beam_seq, beam_seq_logprobs, beam_logprobs_sum, states, R, next_tokens, parents, done, done_count,
                     ld_logits=None):
    """beam_step + the completion loop of CaptionModel.beam_search for one t.  logits f32 [B][V1]; beam_seq int32 [T][B], beam_seq_logprobs
    f32 [T][B], beam_logprobs_sum f32 [B]; states: up to four (in, out, ld_in, ld_out) of B rows of R floats, gathered by parent; next_tokens
    int64 [B], parents int32 [B]; done int32 [B * T][2 T + 2] (seq | logps | p | completion index), done_count int32 [1]"""
    a = _beam_args('decode_beam_step', 1, logits, V1, B, t, T, beam_seq, beam_seq_logprobs, beam_logprobs_sum, states, R, next_tokens, parents, done,
                   done_count, ld_logits)
    call('l2s_decode_beam_step', C.byref(a), stream())


def _beam_args(name, rows, logits, V1, B, t, T, beam_seq, beam_seq_logprobs, beam_logprobs_sum, states, R, next_tokens, parents, done, done_count,
               ld_logits):
    """the checked argument block of the beam step for `rows` captions (the single entry: 1)"""
    if not 1 <= B <= BEAM_MAX:
        raise ValueError('--beam_size %r: 1 .. %d' % (B, BEAM_MAX))
    ld = V1 if ld_logits is None else ld_logits
    n = rows * B
    if (logits.numel() < (n - 1) * ld + V1 or beam_seq.numel() < T * n or beam_seq_logprobs.numel() < T * n or beam_logprobs_sum.numel() < n or
            next_tokens.numel() < n or parents.numel() < n or done.numel() < n * T * beam_record_words(T) or done_count.numel() < rows):
        raise ValueError('%s: a buffer is smaller than B = %d, T = %d, V1 = %d ask' % (name, B, T, V1))
    a = _lib.BeamStepArgs()
    a.logits, a.ld_logits, a.V1, a.B, a.t, a.T, a.R, a.n_state = ptr(logits), int(ld), int(V1), int(B), int(t), int(T), int(R), len(states)
    a.beam_seq, a.beam_seq_logprobs, a.beam_logprobs_sum = ptr(beam_seq), ptr(beam_seq_logprobs), ptr(beam_logprobs_sum)
    assert len(states) <= 4
    for j, (si, so, li, lo) in enumerate(states):
        if si.numel() < n * R or so.numel() < n * R or li < R or lo < R:     # (a strided [n][R] view counts its own elements only)
            raise ValueError('%s: state %d is smaller than B = %d rows of R = %d' % (name, j, B, R))
        a.state_in[j], a.state_out[j], a.ld_in[j], a.ld_out[j] = ptr(si), ptr(so), int(li), int(lo)
    a.next_tokens, a.parents, a.done, a.done_count = ptr(next_tokens), ptr(parents), ptr(done), ptr(done_count)
    return a


def mask_resize_nearest(src, ih, iw, dst, H, W):
    """dst uint8 [H][W] = src uint8 [ih][iw] resized by PIL NEAREST, the rule of the loader's ground-truth masks"""
    if src.numel() < ih * iw or dst.numel() < H * W:
        raise ValueError('mask_resize_nearest: a mask is smaller than its shape')
    call('l2s_mask_resize_nearest', ptr(src), int(ih), int(iw), ptr(dst), int(H), int(W), stream())


# ------------------------------------------------------------------ the caption branch on rows (csrc/caption_rows.hip)
# rows: the rows of the buffers; row r is live iff row0 + r < count[0] (count: device int32 [1], None = all)
def _rows_count(name, rows, row0, count):
    if rows < 1 or row0 < 0:
        raise ValueError('%s: rows = %r, row0 = %r' % (name, rows, row0))
    if count is not None and (count.dtype != torch.int32 or count.numel() < 1):
        raise ValueError('%s: count is a device int32 [1]' % name)


def masks_to_map(masks, rows, mh, mw, H, W, Hc, Wc, out, count=None, row0=0):
    """out f32 {0,1} [rows][Hc * Wc] = mask_resize_nearest to H x W (skipped when the masks have that size) + mask_downsample of masks
    uint8 [rows][mh][mw], one launch"""
    _rows_count('masks_to_map', rows, row0, count)
    if masks.dtype != torch.uint8 or masks.numel() < rows * mh * mw or out.dtype != torch.float32 or out.numel() < rows * Hc * Wc:
        raise ValueError('masks_to_map: a buffer is smaller than its shape, or not uint8 -> float32')
    call('l2s_masks_to_map', ptr(masks), int(rows), int(row0), ptr(count), int(mh), int(mw), int(H), int(W), int(Hc), int(Wc), ptr(out), stream())


def adaptive_pool_rows(x, pixmasks, y, rows, H, W, Cc, OH, OW, ldy, count=None, row0=0):
    """y [rows][OH * OW][ldy] = adaptive_pool_fwd of x [H * W][Cc] under pixmasks f32 [rows][H * W] (None: unmasked, every row alike)"""
    _rows_count('adaptive_pool_rows', rows, row0, count)
    if x.numel() < H * W * Cc or x.dtype != y.dtype or ldy < Cc or (pixmasks is not None and (pixmasks.dtype != torch.float32 or pixmasks.numel() < rows * H * W)):
        raise ValueError('adaptive_pool_rows: a buffer is smaller than its shape, or the dtypes differ')
    call('l2s_adaptive_pool_rows', ptr(x), ptr(pixmasks), ptr(y), int(rows), int(row0), ptr(count), H, W, Cc, OH, OW, ldy, dt_of(x), stream())


def cap_att_dots_rows(patt, att_h, aw, ab, rows, L, D, dots, count=None, row0=0, ld_att_h=None):
    """dots f32 [rows][256] = cap_att_dots_fwd per row of patt [rows][L][D] and att_h [rows][D]"""
    _rows_count('cap_att_dots_rows', rows, row0, count)
    if patt.numel() < rows * L * D or dots.numel() < rows * 256 or L > 256:
        raise ValueError('cap_att_dots_rows: a buffer is smaller than rows = %d asks, or L = %d > 256' % (rows, L))
    call('l2s_cap_att_dots_rows', ptr(patt), ptr(att_h), D if ld_att_h is None else ld_att_h, ptr(aw), ptr(ab), int(rows), int(row0), ptr(count), L, D,
         ptr(dots), stream())


def cap_apply_gates_rows(P, dots, b_a2c, sums, c_prev, c, h, rows, L, R, count=None, row0=0, ld_sums=None):
    """(c, h) [rows][R] = cap_apply_gates_fwd per row of P [rows][L][2R], dots [rows][256], sums [rows][5R], c_prev [rows][R]"""
    _rows_count('cap_apply_gates_rows', rows, row0, count)
    if P.numel() < rows * L * 2 * R or dots.numel() < rows * 256 or min(c_prev.numel(), c.numel(), h.numel()) < rows * R or L > 256 or R > 1024:
        raise ValueError('cap_apply_gates_rows: a buffer is smaller than rows = %d asks, or L = %d > 256, or R = %d > 1024' % (rows, L, R))
    call('l2s_cap_apply_gates_rows', ptr(P), ptr(dots), ptr(b_a2c), ptr(sums), 5 * R if ld_sums is None else ld_sums, ptr(c_prev), ptr(c), ptr(h),
         int(rows), int(row0), ptr(count), L, R, stream())


def lstm_cell_rows(pre, add0, add1, segs, c_prev, c, h, rows, R, count=None, row0=0, ld_pre=None, pre2=None, ld_pre2=None, ld_c_prev=None,
                   ld_c=None, ld_h=None):
    """one nn.LSTMCell step on rows (csrc/caption_rows.hip): gates[r] = pre[r * ld_pre] + pre2[r * ld_pre2] + add0 + add1 + sum over segs
    (x, ldx, w, ld, n) of w[4R][:n] . x[r * ldx][:n], with w a column block (leading dimension ld) of a wider matrix; writes c[r * ld_c]
    and h[r * ld_h].  ld_pre = 0: one row of pre for all rows.  Up to two segments; None entries are skipped.  Every tensor is the flat
    view that starts at its first element (h inside a wider row: array.view(-1)[offset:])."""
    _rows_count('lstm_cell_rows', rows, row0, count)
    a = _lstm_rows_args('lstm_cell_rows', pre, add0, add1, segs, c_prev, c, h, rows, R, ld_pre, pre2, ld_pre2, ld_c_prev, ld_c, ld_h, rows)
    call('l2s_lstm_cell_rows', C.byref(a), int(R), int(rows), int(row0), ptr(count), stream())


def _lstm_rows_args(name, pre, add0, add1, segs, c_prev, c, h, rows, R, ld_pre, pre2, ld_pre2, ld_c_prev, ld_c, ld_h, rows_pre2):
    """the checked argument block of the cell on rows; rows_pre2: the rows of pre2 (a detection's row under lstm_cell_groups)"""
    G = 4 * R
    ld_pre, ld_pre2 = (G if v is None else int(v) for v in (ld_pre, ld_pre2))
    ld_c_prev, ld_c, ld_h = (R if v is None else int(v) for v in (ld_c_prev, ld_c, ld_h))
    span = lambda ld, w: (rows - 1) * ld + w
    segs = [sg for sg in segs if sg is not None]
    if len(segs) > 2 or R < 1 or min(ld_c_prev, ld_c, ld_h) < R or \
            any(p is not None and (0 < ld < G or ld < 0 or p.numel() < (n - 1) * ld + G) for p, ld, n in ((pre, ld_pre, rows), (pre2, ld_pre2, rows_pre2))) or \
            any(v is not None and v.numel() < G for v in (add0, add1)) or \
            c_prev.numel() < span(ld_c_prev, R) or c.numel() < span(ld_c, R) or h.numel() < span(ld_h, R) or \
            any(n < 1 or ld < n or ldx < n or x.numel() < span(ldx, n) or w.numel() < (G - 1) * ld + n for x, ldx, w, ld, n in segs):
        raise ValueError('%s: a buffer is smaller than rows = %d, R = %d and its leading dimension ask, or more than two segments' % (name, rows, R))
    a = _lib.LstmRows()
    a.pre, a.ld_pre, a.pre2, a.ld_pre2, a.add0, a.add1 = ptr(pre), ld_pre, ptr(pre2), ld_pre2, ptr(add0), ptr(add1)
    a.c_prev, a.ld_c_prev, a.c, a.ld_c, a.h, a.ld_h = ptr(c_prev), ld_c_prev, ptr(c), ld_c, ptr(h), ld_h
    for q, (x, ldx, w, ld, n) in zip(a.seg, segs):
        q.x, q.ldx, q.w, q.ld, q.n = ptr(x), int(ldx), ptr(w), int(ld), int(n)
    return a


def cap_att_apply_rows(att, dots, att_res, rows, L, R, count=None, row0=0, ld_res=None):
    """att_res[r * ld_res][:R] = cap_att_apply_fwd per row of att [rows][L][R] and dots [rows][256], without the weights"""
    _rows_count('cap_att_apply_rows', rows, row0, count)
    ld = R if ld_res is None else int(ld_res)
    if att.numel() < rows * L * R or dots.numel() < rows * 256 or L > 256 or ld < R or att_res.numel() < (rows - 1) * ld + R:
        raise ValueError('cap_att_apply_rows: a buffer is smaller than rows = %d asks, or L = %d > 256' % (rows, L))
    call('l2s_cap_att_apply_rows', ptr(att), ptr(dots), ptr(att_res), ld, int(rows), int(row0), ptr(count), L, R, stream())


def decode_pick_rows(logits, V1, rows, t, T, finished, seq, logprobs, next_token, forced=None, count=None, row0=0, ld_logits=None, score=None):
    """per row of logits f32 [rows][V1]: the greedy decision of decode_pick, or with forced (device int64 [1]) that token and its
    log-probability; finished int32 [rows], seq int64 [rows][T], logprobs f32 [rows][T] (column t), next_token int64 [rows], score f32 [rows]
    (optional): the sum of the row's log-probabilities up to t"""
    _rows_count('decode_pick_rows', rows, row0, count)
    ld = V1 if ld_logits is None else ld_logits
    if logits.numel() < (rows - 1) * ld + V1 or not 0 <= t < T or min(seq.numel(), logprobs.numel()) < rows * T or \
            min(finished.numel(), next_token.numel()) < rows or seq.dtype != torch.int64 or next_token.dtype != torch.int64 or \
            (forced is not None and forced.dtype != torch.int64) or (score is not None and score.numel() < rows):
        raise ValueError('decode_pick_rows: a buffer is smaller than rows = %d / V1 = %d / t = %d of T = %d ask, or has the wrong dtype' % (rows, V1, t, T))
    call('l2s_decode_pick_rows', ptr(logits), int(ld), int(V1), int(rows), int(row0), ptr(count), int(t), int(T), ptr(forced), ptr(finished), ptr(seq),
         ptr(logprobs), ptr(next_token), ptr(score), stream())


def decode_force_rows(logits, V1, rows, t, T, targets, lengths, logprobs, next_token, count=None, row0=0, ld_logits=None, score=None):
    """teacher forcing with a token row per row, step t of T: targets int64 [rows][T] (w_1 .. w_n, 0, padding), lengths int32 [rows]
    (n + 1).  A row with t < lengths[r]: logprobs f32 [rows][T] column t = log_softmax(logits[r])[targets[r][t]] (decode_pick_rows' forced
    arithmetic), added to score f32 [rows] (optional), next_token int64 [rows] = targets[r][t]; behind its length a row only gets
    next_token = 0"""
    _rows_count('decode_force_rows', rows, row0, count)
    ld = V1 if ld_logits is None else ld_logits
    if logits.dtype != torch.float32 or V1 < 1 or ld < V1 or logits.numel() < (rows - 1) * ld + V1 or not 0 <= t < T or \
            min(targets.numel(), logprobs.numel()) < rows * T or min(lengths.numel(), next_token.numel()) < rows or \
            targets.dtype != torch.int64 or lengths.dtype != torch.int32 or logprobs.dtype != torch.float32 or next_token.dtype != torch.int64 or \
            (score is not None and (score.numel() < rows or score.dtype != torch.float32)):
        raise ValueError('decode_force_rows: a buffer is smaller than rows = %d / V1 = %d / t = %d of T = %d ask, or has the wrong dtype' % (rows, V1, t, T))
    call('l2s_decode_force_rows', ptr(logits), int(ld), int(V1), int(rows), int(row0), ptr(count), int(t), int(T), ptr(targets), ptr(lengths),
         ptr(logprobs), ptr(next_token), ptr(score), stream())


# ---- beam search on rows: `rows` detections with B beam rows each (group = B consecutive state rows per detection)
def decode_beam_step_rows(logits, V1, B, t, T, rows, beam_seq, beam_seq_logprobs, beam_logprobs_sum, states, R, next_tokens, parents, done,
                          done_count, count=None, row0=0, ld_logits=None):
    """decode_beam_step for every live detection in one launch: logits f32 [rows * B][V1]; beam_seq int32 [rows][T][B], beam_seq_logprobs f32
    [rows][T][B], beam_logprobs_sum f32 [rows][B]; states: up to four (in, out, ld_in, ld_out) of rows * B rows of R floats, gathered by
    parent inside each detection's B rows; next_tokens int64 [rows * B], parents int32 [rows][B]; done int32 [rows][B * T][2 T + 2],
    done_count int32 [rows]"""
    _rows_count('decode_beam_step_rows', rows, row0, count)
    a = _beam_args('decode_beam_step_rows', int(rows), logits, V1, B, t, T, beam_seq, beam_seq_logprobs, beam_logprobs_sum, states, R, next_tokens,
                   parents, done, done_count, ld_logits)
    if next_tokens.dtype != torch.int64:
        raise ValueError('decode_beam_step_rows: next_tokens is int64')
    call('l2s_decode_beam_step_rows', C.byref(a), int(rows), int(row0), ptr(count), stream())


def decode_beam_finish_rows(done, done_count, B, T, rows, beam_seq, beam_logps, beam_p, beam_n, seq, logprobs, count=None, row0=0):
    """the final ordering of every live detection's completed beams (p descending, completion order among equals): beam_seq int64
    [rows][B][T], beam_logps f32 [rows][B][T], beam_p f32 [rows][B], beam_n int32 [rows], and the best beam as seq int64 [rows][T] /
    logprobs f32 [rows][T] in decode_pick_rows' layout"""
    _rows_count('decode_beam_finish_rows', rows, row0, count)
    if not 1 <= B <= BEAM_MAX or not 1 <= T <= BEAM_MAX_T:
        raise ValueError('--beam_size %r: 1 .. %d, with at most %d tokens (got %r)' % (B, BEAM_MAX, BEAM_MAX_T, T))
    n = rows * B
    if (done.numel() < n * T * beam_record_words(T) or done_count.numel() < rows or min(beam_seq.numel(), beam_logps.numel()) < n * T or
            beam_p.numel() < n or beam_n.numel() < rows or min(seq.numel(), logprobs.numel()) < rows * T or beam_seq.dtype != torch.int64 or
            seq.dtype != torch.int64 or beam_n.dtype != torch.int32 or done.dtype != torch.int32 or done_count.dtype != torch.int32):
        raise ValueError('decode_beam_finish_rows: a buffer is smaller than rows = %d, B = %d, T = %d ask, or has the wrong dtype' % (rows, B, T))
    call('l2s_decode_beam_finish_rows', ptr(done), ptr(done_count), int(B), int(T), int(rows), int(row0), ptr(count), ptr(beam_seq), ptr(beam_logps),
         ptr(beam_p), ptr(beam_n), ptr(seq), ptr(logprobs), stream())


def _groups(name, rows, group, row0, count):
    _rows_count(name, rows, row0, count)
    if isinstance(group, bool) or group < 1 or rows % group:
        raise ValueError('%s: rows = %r is no multiple of group = %r' % (name, rows, group))
    return rows // group


def cap_att_dots_groups(patt, att_h, aw, ab, rows, group, L, D, dots, count=None, row0=0, ld_att_h=None):
    """cap_att_dots_rows on `rows` state rows of which `group` consecutive ones share a detection's patt [rows / group][L][D]"""
    dets = _groups('cap_att_dots_groups', rows, group, row0, count)
    ld = D if ld_att_h is None else int(ld_att_h)
    if patt.numel() < dets * L * D or dots.numel() < rows * 256 or L > 256 or ld < D or att_h.numel() < (rows - 1) * ld + D:
        raise ValueError('cap_att_dots_groups: a buffer is smaller than rows = %d in groups of %d ask, or L = %d > 256' % (rows, group, L))
    call('l2s_cap_att_dots_groups', ptr(patt), ptr(att_h), ld, ptr(aw), ptr(ab), int(rows), int(group), int(row0), ptr(count), L, D, ptr(dots),
         stream())


def cap_apply_gates_groups(P, dots, b_a2c, sums, c_prev, c, h, rows, group, L, R, count=None, row0=0, ld_sums=None):
    """cap_apply_gates_rows on `rows` state rows of which `group` consecutive ones share a detection's P [rows / group][L][2R]"""
    dets = _groups('cap_apply_gates_groups', rows, group, row0, count)
    ld = 5 * R if ld_sums is None else int(ld_sums)
    if P.numel() < dets * L * 2 * R or dots.numel() < rows * 256 or min(c_prev.numel(), c.numel(), h.numel()) < rows * R or L > 256 or R > 1024 or \
            ld < 5 * R or sums.numel() < (rows - 1) * ld + 5 * R:
        raise ValueError('cap_apply_gates_groups: a buffer is smaller than rows = %d in groups of %d ask, or L = %d > 256, or R = %d > 1024'
                         % (rows, group, L, R))
    call('l2s_cap_apply_gates_groups', ptr(P), ptr(dots), ptr(b_a2c), ptr(sums), ld, ptr(c_prev), ptr(c), ptr(h), int(rows), int(group), int(row0),
         ptr(count), L, R, stream())


def cap_att_apply_groups(att, dots, att_res, rows, group, L, R, count=None, row0=0, ld_res=None):
    """cap_att_apply_rows on `rows` state rows of which `group` consecutive ones share a detection's att [rows / group][L][R]"""
    dets = _groups('cap_att_apply_groups', rows, group, row0, count)
    ld = R if ld_res is None else int(ld_res)
    if att.numel() < dets * L * R or dots.numel() < rows * 256 or L > 256 or ld < R or att_res.numel() < (rows - 1) * ld + R:
        raise ValueError('cap_att_apply_groups: a buffer is smaller than rows = %d in groups of %d ask, or L = %d > 256' % (rows, group, L))
    call('l2s_cap_att_apply_groups', ptr(att), ptr(dots), ptr(att_res), ld, int(rows), int(group), int(row0), ptr(count), L, R, stream())


def lstm_cell_groups(pre, add0, add1, segs, c_prev, c, h, rows, group, R, count=None, row0=0, ld_pre=None, pre2=None, ld_pre2=None, ld_c_prev=None,
                     ld_c=None, ld_h=None):
    """lstm_cell_rows on `rows` state rows of which `group` consecutive ones belong to one detection: pre2 [rows / group][ld_pre2] is the
    per-detection term, read at row r // group; everything else is per state row"""
    dets = _groups('lstm_cell_groups', rows, group, row0, count)
    a = _lstm_rows_args('lstm_cell_groups', pre, add0, add1, segs, c_prev, c, h, rows, R, ld_pre, pre2, ld_pre2, ld_c_prev, ld_c, ld_h, dets)
    call('l2s_lstm_cell_groups', C.byref(a), int(R), int(rows), int(group), int(row0), ptr(count), stream())


def rcnn_predict(heads, ldh, R, ncls, stds4, means4, cls_prob, bbox_pred):
    call('l2s_rcnn_predict', ptr(heads), ldh, R, ncls, ptr(stds4), ptr(means4), ptr(cls_prob), ptr(bbox_pred), stream())


def mask_prob(score, ldsc, ncls, labels, ms2, n_elem, out):
    call('l2s_mask_prob', ptr(score), ldsc, ncls, ptr(labels), ms2, n_elem, ptr(out), stream())


def response_loss(resp, gt_mask_u8, mask_h, mask_w, H, W, gscale, loss, dresp):
    call('l2s_response_loss', ptr(resp), ptr(gt_mask_u8), mask_h, mask_w, H, W, float(gscale), ptr(loss), ptr(dresp), stream())


def cap_attention_fwd(patt, att, att_h, aw, ab, L, D, tanh_ws, weight, att_res):
    call('l2s_cap_attention_fwd', ptr(patt), ptr(att), ptr(att_h), ptr(aw), ptr(ab), L, D, ptr(tanh_ws), ptr(weight),
         ptr(att_res), stream())


def cap_attention_bwd(datt_res, att, tanh_ws, weight, aw, L, D, dpatt, datt, datt_h, daw, dab):
    call('l2s_cap_attention_bwd', ptr(datt_res), ptr(att), ptr(tanh_ws), ptr(weight), ptr(aw), L, D, ptr(dpatt), ptr(datt),
         ptr(datt_h), ptr(daw), ptr(dab), stream())


def cap_gates_fwd(sums, a2c, c_prev, c, h, save, R):
    call('l2s_cap_gates_fwd', ptr(sums), ptr(a2c), ptr(c_prev), ptr(c), ptr(h), ptr(save), R, stream())


def cap_gates_bwd(dh, dc_in, save, c_prev, dsums, da2c, dc_prev, R, dh2=None):
    call('l2s_cap_gates_bwd', ptr(dh), ptr(dh2), ptr(dc_in), ptr(save), ptr(c_prev), ptr(dsums), ptr(da2c), ptr(dc_prev), R, stream())


def linear2_fwd(x, K, w1, b1, y1, N1, acc1, w2, b2, y2, N2, acc2):
    call('l2s_linear2_fwd', ptr(x), K, ptr(w1), ptr(b1), ptr(y1), N1, int(acc1), ptr(w2), ptr(b2), ptr(y2), N2, int(acc2), stream())


def linear_sum2_fwd(x1, w1, K1, x2, w2, K2, y, N, accumulate=False):
    call('l2s_linear_sum2_fwd', ptr(x1), ptr(w1), K1, ptr(x2), ptr(w2), K2, ptr(y), N, int(accumulate), stream())


def cap_a2c_gates_fwd(att_res, w_a2c, b_a2c, K, sums, c_prev, c, h, save, R):
    call('l2s_cap_a2c_gates_fwd', ptr(att_res), ptr(w_a2c), ptr(b_a2c), K, ptr(sums), ptr(c_prev), ptr(c), ptr(h), ptr(save), R, stream())


def cap_att_dots_fwd(patt, att_h, aw, ab, L, D, tanh_ws, dots):
    call('l2s_cap_att_dots_fwd', ptr(patt), ptr(att_h), ptr(aw), ptr(ab), L, D, ptr(tanh_ws), ptr(dots), stream())


def cap_apply_gates_fwd(P, dots, b_a2c, sums, c_prev, c, h, save, weight, L, R):
    call('l2s_cap_apply_gates_fwd', ptr(P), ptr(dots), ptr(b_a2c), ptr(sums), ptr(c_prev), ptr(c), ptr(h), ptr(save), ptr(weight), L, R, stream())


def bottleneck64_fwd(a, x, w2, b2, w3, b3, y, H, W, wd=None, bd=None, w1n=None, b1n=None, a_next=None):
    """csrc/bottleneck_fused.hip: a frozen 64-plane bottleneck behind its conv1 (+ the next block's conv1) in one launch, bf16"""
    d = _lib.Bottleneck64Desc(ptr(a), ptr(x), ptr(w2), ptr(w3), ptr(wd), ptr(w1n), ptr(b2), ptr(b3), ptr(bd), ptr(b1n), ptr(y), ptr(a_next), H, W, x.shape[-1])
    call('l2s_bottleneck64_fwd', C.byref(d), stream())


def cap_recur_supported(S, R, AH, L):
    return bool(_lib.load().l2s_cap_recur_supported(int(S), int(R), int(AH), int(L)))


def cap_recur_state(backward, device='cuda'):
    """the exchange state of one direction of the resident recurrence: zeroed ONCE here, then owned by the kernels (launch count, give-up flag, granules)"""
    n = int(_lib.load().l2s_cap_recur_state_bytes(int(backward)))
    return torch.zeros((n + 3) // 4, dtype=torch.int32, device=device)


def cap_recur_fwd(w_h2h, b_h2h, w_h2att, b_h2att, patt, aw, ab, P, b_a2c, sums, hs, cs, save, tanh_ws, wgt, state, S, R, AH, L):
    a = _lib.CapRecurFwdArgs(ptr(w_h2h), ptr(b_h2h), ptr(w_h2att), ptr(b_h2att), ptr(patt), ptr(aw), ptr(ab), ptr(P), ptr(b_a2c), ptr(sums), ptr(hs), ptr(cs),
                             ptr(save), ptr(tanh_ws), ptr(wgt), ptr(state), S, R, AH, L)
    call('l2s_cap_recur_fwd', C.byref(a), stream())


def cap_recur_bwd(w_h2h, w_h2att, P, aw, save, cs, wgt, tanh_ws, dho, dsums, da2c, ddot, datt_h, state, S, R, AH, L):
    a = _lib.CapRecurBwdArgs(ptr(w_h2h), ptr(w_h2att), ptr(P), ptr(aw), ptr(save), ptr(cs), ptr(wgt), ptr(tanh_ws), ptr(dho), ptr(dsums), ptr(da2c), ptr(ddot),
                             ptr(datt_h), ptr(state), S, R, AH, L, ddot.stride(0), datt_h.stride(0))
    call('l2s_cap_recur_bwd', C.byref(a), stream())


def cap_gates_bwd_dw(dh, dc_in, save, c_prev, P, dsums, da2c, dc_prev, dweight, L, R, dh2=None):
    call('l2s_cap_gates_bwd_dw', ptr(dh), ptr(dh2), ptr(dc_in), ptr(save), ptr(c_prev), ptr(P), ptr(dsums), ptr(da2c), ptr(dc_prev), ptr(dweight),
         L, R, stream())


def cap_attention_bwd_step2(dweight, tanh_ws, weight, aw, L, D, ddot, datt_h):
    call('l2s_cap_attention_bwd_step2', ptr(dweight), ptr(tanh_ws), ptr(weight), ptr(aw), L, D, ptr(ddot), ptr(datt_h), stream())


def cap_attention_bwd_step(datt_res, att, tanh_ws, weight, aw, L, D, ddot, datt_h):
    call('l2s_cap_attention_bwd_step', ptr(datt_res), ptr(att), ptr(tanh_ws), ptr(weight), ptr(aw), L, D, ptr(ddot), ptr(datt_h), stream())


def cap_attention_bwd_batched(ddot, weight, datt_res, ldr, tanh_ws, aw, S, L, D, dpatt, datt, daw, dab):
    call('l2s_cap_attention_bwd_batched', ptr(ddot), ptr(weight), ptr(datt_res), ldr, ptr(tanh_ws), ptr(aw), S, L, D, ptr(dpatt), ptr(datt),
         ptr(daw), ptr(dab), stream())


def logsoftmax_nll(logits, target, mask, S, V1, gscale, loss_slot, dlogits, logprobs=None):
    call('l2s_logsoftmax_nll', ptr(logits), ptr(target), ptr(mask), S, V1, float(gscale), ptr(loss_slot), ptr(dlogits),
         ptr(logprobs), stream())


def sgd_momentum(param, grad, mom, segs_dev, nseg, rowscale, lr, momentum, wd, gscale=1.0, shadow=None, clear_grad=False):
    call('l2s_sgd_momentum', ptr(param), ptr(grad), ptr(mom), ptr(segs_dev), nseg, ptr(rowscale), float(lr), float(momentum),
         float(wd), float(gscale), ptr(shadow), dt_of(shadow) if shadow is not None else 0, 1 if clear_grad else 0, stream())


def sgd_momentum_range(param, grad, mom, segs_dev, nseg, rowscale, lr, momentum, wd, gscale, shadow, flags, lo, hi, chunk_lo, chunk_hi):
    """the update on the elements [lo, hi) only (flags: 1 = clear the gradients consumed, 2 = shadow rewrite only)"""
    call('l2s_sgd_momentum_range', ptr(param), ptr(grad), ptr(mom), ptr(segs_dev), nseg, ptr(rowscale), float(lr), float(momentum),
         float(wd), float(gscale), ptr(shadow), dt_of(shadow) if shadow is not None else 0, int(flags), int(lo), int(hi), int(chunk_lo), int(chunk_hi), stream())


def sgd_momentum_range_g16(param, grad_bf16, grad_lo, mom, segs_dev, nseg, rowscale, lr, momentum, wd, gscale, shadow, lo, hi, chunk_lo, chunk_hi):
    """the ranged update with the gradients of [lo, hi) read from `grad_bf16[o - grad_lo]` (a reduce-scattered bf16 shard)"""
    call('l2s_sgd_momentum_range_g16', ptr(param), ptr(grad_bf16), int(grad_lo), ptr(mom), ptr(segs_dev), nseg, ptr(rowscale), float(lr), float(momentum),
         float(wd), float(gscale), ptr(shadow), dt_of(shadow) if shadow is not None else 0, int(lo), int(hi), int(chunk_lo), int(chunk_hi), stream())


def sgd_chunk():
    return int(_lib.load().l2s_sgd_chunk())


def add_f32(a, b, out):
    call('l2s_add_f32', ptr(a), ptr(b), ptr(out), a.numel(), stream())


def mul(a, b, out):
    call('l2s_mul_f32', ptr(a), ptr(b), ptr(out), a.numel(), stream())
