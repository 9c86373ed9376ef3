"""Every instance per sentence: the reference's full Mask R-CNN test path (pyutils/mask-faster-rcnn/lib/model/test.py:268-297,310-344)
on the device, next to the one-box pick of model/eval_device.py.  Per sentence, behind Network.forward_test_sentence:
    l2s_detect_nms      per class: score > thresh, order, greedy NMS with cfg.TEST.NMS (one workgroup per class)
    l2s_detect_select   max_per_image over all classes, the detections in class order, the mask head's RoIs and labels
    the n-row mask head on `cap` rows, each with its own class (networks with a mask branch)
    l2s_detect_paste    recover_masks + > 122 of every kept detection into its canvas, the areas
    l2s_rle_from_masks  the canvases as COCO run lengths in the image's pool (three launches)
No host synchronisation per sentence; one read-back per image (the records, counts and spans, then the used part of the pool).  Nothing
is dropped: a sentence with more detections than `cap`, or whose run lengths overflowed the pool, runs again with buffers sized from the
counts its first run reported (the backbone map of forward_test_image is still there).

Optionally (detect_image describe= / expr_score=, cycle network) the caption branch on rows runs behind each sentence's detections, on the
sentence's canvases with the detector's device count (nets/caption_rows.py): what the captioner says about every detection, and the
teacher-forced log-likelihood of the sentence's own expression under every detection's mask.  Its results stay on the device per sentence
and come back as one more read-back per image.

Optionally (detect_image gt_masks= / eval_split_device judge=, rerank=) every detection is judged against the sentence's ground truth on
the device (csrc/select.hip: l2s_detect_gt_iou, l2s_detect_choose, behind the rows stage, whose score it reads): I, U and hit per
detection, and per rule (detector, oracle, speaker, rerank@lambda) the detection it picks.  One more read-back per image."""
import math

import numpy as np
import torch

from .. import ops as O
from . import eval_device as ED
from .config import cfg

_REC = O.DET_RECORD_BYTES // 4                                 # int32 words of one record


def default_cap(max_per_image):
    """rows of the detection buffers: max_per_image rounded up to a multiple of 64, 512 without a limit (a guess, not a bound)"""
    return (int(max_per_image) + 63) // 64 * 64 if max_per_image > 0 else 512


def _pool_budget(cap, iw):
    """run-length words for `cap` masks: eval_device._Export's per-mask budget"""
    return cap * (iw * (int(cfg.MASK_SIZE) + 2) + 2)


def detect_sentence(net, s, scale, ih, iw, max_per_image, thresh, cap, rec=None, count=None, spans=None, pool=None, cursor=None,
                    boxes_dump=None):
    """s: the dict of Network.forward_test_sentence.  -> dict of device buffers: rec int32 [cap][8] (l2s_det_record), count int32 [2]
    (written, total), and with a mask branch mask_prob f32 [cap][MS][MS] (the net's buffer: valid until its next mask head pass),
    canvases uint8 [cap][ih][iw], spans int32 [cap][2], pool, cursor.  rec, count, spans, pool, cursor: the caller's (an image's pool
    shared by its sentences), allocated here when None.  The mask head reuses the heads' buffers: read s's outputs before this call.
    No host synchronisation."""
    dev = torch.device(net.device)
    C, post = net._num_classes, s['post']
    with_masks = getattr(net, 'variant', None) != 'vgg'
    i32 = torch.int32
    rec = torch.empty((cap, _REC), dtype=i32, device=dev) if rec is None else rec
    count = torch.empty((2,), dtype=i32, device=dev) if count is None else count
    ws = net.buf('det.ws', ((O.detect_ws_bytes(post, C) + 3) // 4,), i32)
    roi = net.buf('det.mask_rois', (cap, 5), torch.float32)
    lab = net.buf('det.mask_labels', (cap,), i32)
    O.detect_nms(s['cls_prob'], s['bbox_pred'], s['rois'], s['nkeep'], post, C, scale, ih, iw, cfg.TEST.BBOX_REG, thresh, float(cfg.TEST.NMS),
                 ws, boxes_dump)
    O.detect_select(ws, post, C, max_per_image, scale, rec, roi, lab, cap, count)
    out = dict(rec=rec, count=count)
    if not with_masks:
        return out
    MS = int(cfg.MASK_SIZE)
    Hc, Wc = s['net_conv_hw']
    mprob = net._roi_heads_test(s['net_conv'], Hc, Wc, roi, cap, labels=lab)[3].view(cap, MS, MS)
    canvases = net.buf('det.canvases', (cap, ih, iw), torch.uint8)
    O.detect_paste(mprob, rec, count, ih, iw, canvases)
    spans = torch.empty((cap, 2), dtype=i32, device=dev) if spans is None else spans
    if pool is None:
        pool = torch.empty((_pool_budget(cap, iw),), dtype=i32, device=dev)
        cursor = torch.zeros((1,), dtype=i32, device=dev)
    rws = net.buf('det.rle_ws', (cap * O.rle_encode_ws_words(ih, iw),), i32)
    O.rle_from_masks(canvases, count[0:1], pool, cursor, spans, rws)
    out.update(mask_prob=mprob, canvases=canvases, spans=spans, pool=pool, cursor=cursor)
    return out


class _RowsStage(object):
    """the caption branch on rows behind a sentence's detections.  tokens: per sentence the expression's ids (its nonzero labels)"""

    def __init__(self, net, tokens, describe, expr_score, ix_to_word=None, beam_size=1):
        from ..nets import caption_rows, decode
        caption_rows.check_features(net)                          # ValueErrors that name the variant, before any launch
        decode.check_args(net, 1, beam_size if describe else 1, 1.0)
        self.net, self.tokens, self.describe, self.expr_score, self.ix_to_word = net, tokens, bool(describe), bool(expr_score), ix_to_word
        self.beam_size = int(beam_size) if describe else 1         # > 1: beam search on rows; 1: the greedy launches

    def one(self, i):
        """the stage of sentence i alone (its re-run)"""
        return _RowsStage(self.net, [self.tokens[i]], self.describe, self.expr_score, self.ix_to_word, self.beam_size)

    def run(self, i, canvases, cap, ih, iw, written):
        """-> the sentence's results as device copies (the network's row buffers are the next sentence's too)"""
        net = self.net
        att, fc = net.caption_features_rows(canvases, cap, (ih, iw), count=written)
        out = {}
        if self.describe and self.beam_size > 1:
            r = net.caption_beam_rows(att, fc, rows=cap, count=written, beam_size=self.beam_size)
            out.update(seq=r['seq'].clone(), lp=r['logprobs'].clone(), bseq=r['beam_seq'].clone(), blp=r['beam_logprobs'].clone(),
                       bp=r['beam_p'].clone(), bn=r['beam_n'].clone())
        elif self.describe:
            r = net.caption_decode_rows(att, fc, rows=cap, count=written)
            out['seq'], out['lp'] = r['seq'].clone(), r['logprobs'].clone()
        if self.expr_score:
            r = net.caption_score_rows(att, fc, self.tokens[i], rows=cap, count=written)
            out['elp'], out['score'] = r['logprobs'].clone(), r['score'].clone()
            self.net_score = r['score']                            # the network's buffer: the judge stage reads it in stream order
        return out

    KEYS = (('seq', np.int64), ('lp', np.float32), ('bseq', np.int64), ('blp', np.float32), ('bp', np.float32), ('bn', np.int32),
            ('elp', np.float32), ('score', np.float32))

    def read_back(self, outs):
        """one copy for all sentences -> per sentence {key: array}"""
        parts = [(i, k, dt, o[k]) for i, o in enumerate(outs) for k, dt in self.KEYS if k in o]
        host = torch.cat([t.reshape(-1).view(torch.uint8) for _, _, _, t in parts]).cpu().numpy()
        res, off = [dict() for _ in outs], 0
        for i, k, dt, t in parts:
            nb = t.numel() * t.element_size()
            res[i][k] = host[off:off + nb].view(dt).reshape(tuple(t.shape))
            off += nb
        return res

    def fields(self, h, k):
        """the fields of detection k of a sentence from its host arrays h"""
        p = {}
        if self.describe:
            s = h['seq'][k]
            n = int(np.argmax(s == 0)) if (s == 0).any() else s.size
            p['caption_tokens'] = [int(v) for v in s[:n]]
            p['caption_logprobs'] = [float(v) for v in h['lp'][k, :n]]
            if 'bn' in h:                                          # beam search: every beam, best first, as caption_image writes them
                p['caption_beams'] = [dict(seq=[int(v) for v in h['bseq'][k, j]], logps=[float(v) for v in h['blp'][k, j]], p=float(h['bp'][k, j]))
                                      for j in range(int(h['bn'][k]))]
            if self.ix_to_word is not None:
                from .caption_device import decode_sequence
                p['caption'] = decode_sequence(self.ix_to_word, p['caption_tokens'])
        if self.expr_score:
            p['expr_logprob'] = float(h['score'][k])
            p['expr_logprobs'] = [float(v) for v in h['elp'][k]]
        return p


def check_rerank(rerank):
    """the lambdas of the re-ranking rules as a list of floats.  ValueError (naming rerank / --rerank) on an entry that is no finite
    float, on more than ops.DET_MAX_LAMBDA entries and on an entry given twice (the rules are named by their lambda)"""
    out = []
    for v in (rerank or ()):
        try:
            f = float(v)
        except (TypeError, ValueError):
            f = float('nan')
        if not math.isfinite(f) or not math.isfinite(float(np.float32(f))):
            raise ValueError('rerank (--rerank): every entry is a finite float, got %r' % (v,))
        out.append(f)                                              # (the kernel takes them rounded to float32)
    if len(out) > O.DET_MAX_LAMBDA:
        raise ValueError('rerank (--rerank): at most %d entries, got %d' % (O.DET_MAX_LAMBDA, len(out)))
    if len(set(out)) != len(out):
        raise ValueError('rerank (--rerank): an entry is given twice in %r' % (list(rerank),))
    return out


def rule_names(lambdas, with_expr):
    """the rules of l2s_detect_choose in the order of its records"""
    return ['detector', 'oracle'] + (['speaker'] + ['rerank@%s' % l for l in lambdas] if with_expr else [])


class _JudgeStage(object):
    """every detection of a sentence against its ground truth, and one detection per rule (csrc/select.hip), behind the rows stage.
    gt_masks: per sentence a device uint8 [Hs][Ws] mask; gt_boxes: device f32 [S][4] (scaled image); n_tok: per sentence the
    expression's tokens + 1.  with_expr: the rows stage scores the expression (rules speaker and rerank@lambda)"""

    def __init__(self, net, gt_masks, gt_boxes, scale, n_tok, rerank=None, per_token=False, with_expr=False):
        if getattr(net, 'variant', None) == 'vgg':
            raise ValueError('judging detections (judge / --judge_detections, rerank / --rerank) compares masks: variant vgg has no mask branch')
        self.lambdas = check_rerank(rerank)
        if self.lambdas and not with_expr:
            raise ValueError('rerank (--rerank) weighs the expression\'s log-likelihood: it needs expr_score (--expr_score 1)')
        if per_token and not self.lambdas:
            raise ValueError('per_token (--rerank_per_token) divides the re-ranking term: it needs rerank (--rerank)')
        self.net, self.gt_masks, self.gt_boxes, self.scale, self.n_tok = net, gt_masks, gt_boxes, scale, [int(v) for v in n_tok]
        self.per_token, self.with_expr = bool(per_token), bool(with_expr)
        self.names = rule_names(self.lambdas, self.with_expr)

    def one(self, i):
        """the stage of sentence i alone (its re-run)"""
        return _JudgeStage(self.net, [self.gt_masks[i]], self.gt_boxes[i:i + 1], self.scale, [self.n_tok[i]], self.lambdas, self.per_token,
                           self.with_expr)

    def stride(self, cap):
        """int32 words of one sentence: the choice records (8-byte aligned: the stride is even), cap l2s_det_gt rows, gt_area, a pad"""
        return len(self.names) * (O.DET_CHOICE_BYTES // 4) + cap * (O.DET_GT_BYTES // 4) + 2

    def alloc(self, S, cap):
        """the image's device array, zeroed once (the kernel accumulates; every sentence's part is used once)"""
        return torch.zeros((S * self.stride(cap),), dtype=torch.int32, device=torch.device(self.net.device))

    def _views(self, arr, i, cap):
        b, nc = i * self.stride(cap), len(self.names) * (O.DET_CHOICE_BYTES // 4)
        ng = cap * (O.DET_GT_BYTES // 4)
        return arr[b:b + nc], arr[b + nc:b + nc + ng], arr[b + nc + ng:b + nc + ng + 1]

    def run(self, i, arr, canvases, rec, count, cap, expr):
        """two launches on sentence i's canvases and records; expr: the rows stage's score buffer, or None"""
        choice, rows, area = self._views(arr, i, cap)
        O.detect_gt_iou(canvases, rec, count, self.gt_masks[i], self.gt_boxes[i], self.scale, rows, area, clear=False)
        O.detect_choose(rec, rows, count, cap, area, choice, expr if self.with_expr else None, self.lambdas if self.with_expr else (),
                        self.per_token, self.n_tok[i])

    def host(self, arr, i, cap):
        """sentence i of the read-back -> ((I, U, hit) per row, gt_area, {rule: dict})"""
        choice, rows, area = self._views(arr, i, cap)
        det, cls, hit, I, U, key = O.det_choice_fields(choice)
        rules = {name: dict(det=int(det[k]), category_id=int(cls[k]), hit=int(hit[k]), I=int(I[k]), U=int(U[k]), key=float(key[k]))
                 for k, name in enumerate(self.names)}
        return O.det_gt_fields(rows), int(area[0]), rules


class _Detector(object):
    """the device side of one image's detections: per sentence `cap` records, the count and the spans in one int32 array (one read-back),
    the image's run-length pool"""

    def __init__(self, net, S, scale, ih, iw, max_per_image, thresh, cap=None, pool_words=None, capture=None, stage=None, judge=None):
        self.net, self.S, self.scale, self.ih, self.iw = net, S, scale, ih, iw
        self.stage, self.stage_out = stage, [None] * S
        self.judge = judge
        self.max_per_image, self.thresh = int(max_per_image), float(thresh)
        self.cap = cap = default_cap(max_per_image) if cap is None else int(cap)
        self.with_masks = getattr(net, 'variant', None) != 'vgg'
        self.capture = capture
        dev = torch.device(net.device)
        # meta: the pool cursor; per sentence (written, total), cap records, cap spans
        self.stride = 2 + cap * (_REC + 2)
        self.meta = torch.zeros((1 + S * self.stride,), dtype=torch.int32, device=dev)
        if self.with_masks:
            words = S * _pool_budget(cap, iw) if pool_words is None else int(pool_words)
            self.pool = torch.empty((max(words, 1),), dtype=torch.int32, device=dev)
        if judge is not None:
            self.jmeta = judge.alloc(S, cap)

    def _views(self, meta, i):
        b = 1 + i * self.stride
        cap = self.cap
        return meta[b:b + 2], meta[b + 2:b + 2 + cap * _REC].reshape(cap, _REC), meta[b + 2 + cap * _REC:b + self.stride].reshape(cap, 2)

    def run(self, i, s):
        """sentence i of the image on the outputs `s` of its forward_test_sentence"""
        count, rec, spans = self._views(self.meta, i)
        cap_in = None
        if self.capture is not None:                              # checks: the heads' outputs before the mask head reuses their buffers
            cap_in = dict(cls_prob=s['cls_prob'].clone(), bbox_pred=s['bbox_pred'].clone(), rois=s['rois'].clone(),
                          nkeep=None if s['nkeep'] is None else s['nkeep'].clone(), post=s['post'])
        out = detect_sentence(self.net, s, self.scale, self.ih, self.iw, self.max_per_image, self.thresh, self.cap, rec=rec, count=count,
                              spans=spans, pool=self.pool if self.with_masks else None, cursor=self.meta[0:1])
        if self.stage is not None:                                # on this sentence's canvases, before the next sentence overwrites them
            self.stage_out[i] = self.stage.run(i, out['canvases'], self.cap, self.ih, self.iw, count[0:1])
        if self.judge is not None:                                # behind the rows stage: it reads that stage's score
            self.judge.run(i, self.jmeta, out['canvases'], rec, count[0:1], self.cap,
                           self.stage.net_score if self.judge.with_expr else None)
        if cap_in is not None:
            if self.with_masks:
                cap_in['mask_prob'] = out['mask_prob'].clone()
            self.capture.append(cap_in)

    def collect(self, file_name, resentence, extra=None, selection=None):
        """the read-back -> one list of dicts per sentence.  resentence(i): forward_test_sentence of sentence i again (a sentence that did
        not fit its buffers runs again with the sizes its counts ask for).  selection: with a judge stage, a list that receives per
        sentence {file_name, sent_index, gt_area, rules: {rule: {det, category_id, hit, I, U, key}}}."""
        meta = self.meta.cpu().numpy()
        pool = self.pool[:int(meta[0])].cpu().numpy().view('<u4') if self.with_masks else None
        rows = None if self.stage is None else self.stage.read_back(self.stage_out)
        jm = None if self.judge is None else self.jmeta.cpu().numpy()

        def judged(det, arr, k, i):
            if arr is None:
                return None
            gt_rows, gt_area, rules = det.judge.host(arr, k, det.cap)
            if selection is not None:
                selection.append(dict(file_name=file_name, sent_index=i, gt_area=gt_area, rules=rules))
            return gt_rows
        out = []
        for i in range(self.S):
            count, rec, spans = self._views(meta, i)
            written, total = int(count[0]), int(count[1])
            fits = total <= self.cap and not (self.with_masks and (spans[:written, 0] < 0).any())
            if fits:
                out.append(self._dicts(rec[:written], spans[:written], pool, file_name, i, extra, None if rows is None else rows[i],
                                       gt_rows=judged(self, jm, i, i)))
                continue
            if self.capture is not None:
                self.capture.append(dict(rerun=i))
            cap = max(total, 1)
            words = int(spans[:written, 1].astype(np.int64).sum()) if total <= self.cap else _pool_budget(cap, self.iw)
            while True:                                            # sizes grow with every round: the counts of `total` masks are a finite sum
                one = _Detector(self.net, 1, self.scale, self.ih, self.iw, self.max_per_image, self.thresh, cap=cap, pool_words=words,
                                stage=None if self.stage is None else self.stage.one(i),
                                judge=None if self.judge is None else self.judge.one(i))
                one.run(0, resentence(i))
                m1 = one.meta.cpu().numpy()
                c1, r1, s1 = one._views(m1, 0)
                if int(c1[1]) > cap:
                    raise RuntimeError('detection: %d detections in the second run of a sentence, %d in its first' % (int(c1[1]), cap))
                if self.with_masks and (s1[:int(c1[0]), 0] < 0).any():
                    words = int(s1[:int(c1[0]), 1].astype(np.int64).sum())
                    continue
                p1 = one.pool[:int(m1[0])].cpu().numpy().view('<u4') if self.with_masks else None
                out.append(self._dicts(r1[:int(c1[0])], s1[:int(c1[0])], p1, file_name, i, extra,
                                       None if one.stage is None else one.stage.read_back(one.stage_out)[0], one.stage,
                                       gt_rows=judged(one, None if one.judge is None else one.jmeta.cpu().numpy(), 0, i)))
                break
        return out

    def _dicts(self, rec, spans, pool, file_name, i, extra, rows=None, stage=None, gt_rows=None):
        roi, cls, box, score, area = O.det_record_fields(np.ascontiguousarray(rec))
        res = []
        for k in range(rec.shape[0]):
            p = dict(file_name=file_name, sent_index=i, roi=int(roi[k]), category_id=int(cls[k]), box=[float(v) for v in box[k]],
                     score=float(score[k]))
            if extra:
                p.update(extra)
            if self.with_masks:
                off, n = int(spans[k, 0]), int(spans[k, 1])
                p['area'] = int(area[k])
                p['segmentation'] = dict(size=[self.ih, self.iw], counts=O.rle_to_string(pool[off:off + n]))
            if rows is not None:
                p.update((stage or self.stage).fields(rows, k))
            if gt_rows is not None:
                p.update(I=int(gt_rows[0][k]), U=int(gt_rows[1][k]), hit=int(gt_rows[2][k]))
            res.append(p)
        return res


def rows_stage(net, labels, describe, expr_score, ix_to_word=None, beam_size=1):
    """the stage detect_image / eval_split_device run behind every sentence, or None without the options.  ValueError on a network whose
    caption branch pools no mask (the variant is named)"""
    if not describe and not expr_score:
        return None
    return _RowsStage(net, [[int(w) for w in row if w != 0] for row in np.asarray(labels)], describe, expr_score, ix_to_word, beam_size)


def judge_stage(net, labels, gt_masks, gt_boxes, scale, judge, rerank, per_token, expr_score):
    """the stage that judges every detection against the ground truth, or None without the options (rerank implies judging).
    gt_masks / gt_boxes: eval_device._upload_image's device views.  ValueErrors name the options involved"""
    if not judge and not rerank:
        if per_token:
            raise ValueError('per_token (--rerank_per_token) divides the re-ranking term: it needs rerank (--rerank)')
        return None
    n_tok = [int((np.asarray(row) != 0).sum()) + 1 for row in np.asarray(labels)]
    return _JudgeStage(net, gt_masks, gt_boxes, scale, n_tok, rerank, per_token, bool(expr_score))


def detect_image(net, data, labels, max_per_image=100, thresh=0.0, _cap=None, _pool_words=None, _capture=None, describe=False, expr_score=False,
                 ix_to_word=None, gt_masks=None, gt_boxes=None, rerank=None, per_token=False, selection=None, beam_size=1):
    """data: {'data': float32 (1, H, W, 3) blob, 'im_info': [H, W, scale]} (+ 'file_name'); labels: int [S][T] token ids, zero padded.
    -> one list per sentence of dicts, class ascending and inside a class score descending: file_name, sent_index, roi (the proposal's
    row), category_id, box [x1, y1, x2, y2] (original image), score and (networks with a mask branch) area and segmentation
    {'size': [ih, iw], 'counts': COCO RLE string}.  max_per_image <= 0: no limit; ties at the limit all stay.
    describe (network 'cycle'): also what the captioner says about each detection's mask, greedy: caption_tokens, caption_logprobs and, with
    ix_to_word ({str(id): word}), caption.  beam_size > 1 (with describe): beam search on rows instead (Network.caption_beam_rows): the three
    fields are the best beam's, and caption_beams lists every beam, best first, as [{seq, logps, p}].  expr_score: also how well each detection's mask explains the sentence: expr_logprobs, the
    teacher-forced log-probabilities of the sentence's n tokens and the end token under that mask (n + 1 values), and expr_logprob, their
    sum.  Both run on the device behind each sentence (nets/caption_rows.py) and cost one more read-back per image.
    gt_masks (uint8 [S][Hs][Ws]) with gt_boxes ([S][4], x1 y1 x2 y2 in the scaled image): every detection is judged against its sentence's
    ground truth on the device (csrc/select.hip) and gains I, U (its mask's intersection and union with the gt mask, resized to the
    canvas as the evaluation resizes it) and hit (its box's IoU with the gt box >= 0.5); `selection` (a list) receives per sentence
    {file_name, sent_index, gt_area, rules}, where rules maps 'detector' (best score), 'oracle' (best mask IoU) and, with expr_score,
    'speaker' (best expr_logprob) and 'rerank@<lambda>' for every lambda of `rerank` (best log(score) + lambda * expr_logprob, divided by
    n + 1 with per_token) to {det (index in the sentence's list, -1 when it is empty), category_id, hit, I, U, key}.  One more read-back.
    (_cap, _pool_words: the buffers' first sizes instead of the defaults; _capture: a list that receives each sentence's head outputs and
    mask probabilities as device copies - checks.)"""
    labels = np.asarray(labels)
    if labels.ndim != 2 or labels.shape[0] < 1:
        raise ValueError('labels: an int array [S][T] with S >= 1, got shape %s' % (labels.shape,))
    if ((labels != 0).sum(1) == 0).any():
        raise ValueError('labels: every sentence needs at least one token')
    S = int(labels.shape[0])
    stage = rows_stage(net, labels, describe, expr_score, ix_to_word, beam_size)
    if (gt_masks is None) != (gt_boxes is None):
        raise ValueError('gt_masks and gt_boxes come together')
    if gt_masks is None and (rerank or per_token or selection is not None):
        raise ValueError('rerank / per_token / selection judge the detections against a ground truth: they need gt_masks and gt_boxes')
    d = dict(data=data['data'], im_info=data['im_info'], labels=labels.astype(np.int64),
             gt_boxes=np.zeros((S, 5), np.float32), gt_masks=np.zeros((S, 1, 1), np.uint8))
    if gt_masks is not None:
        gm, gb = np.asarray(gt_masks), np.asarray(gt_boxes, dtype=np.float32)
        if gm.ndim != 3 or gm.shape[0] != S or gb.ndim != 2 or gb.shape[0] != S or gb.shape[1] < 4:
            raise ValueError('gt_masks is uint8 [S][Hs][Ws] and gt_boxes [S][4] with S = %d, got %s and %s' % (S, gm.shape, gb.shape))
        d.update(gt_masks=gm, gt_boxes=gb)
    net.eval()
    img, lab_d, lens, box_d, gm_d = ED._upload_image(net, d, S)
    im_info = np.asarray(data['im_info'], dtype=np.float32).reshape(-1)[:3]
    scale, ih, iw = ED._geometry(im_info)
    judge = None if gt_masks is None else judge_stage(net, labels, gm_d, box_d, scale, True, rerank, per_token, expr_score)
    dd = dict(data=img, im_info=im_info, S=1)
    net.forward_test_image(dd)
    det = _Detector(net, S, scale, ih, iw, max_per_image, thresh, _cap, _pool_words, _capture, stage, judge)

    def sentence(i):
        dd['labels'] = lab_d[i, :lens[i]]
        dd['T'] = lens[i]
        return net.forward_test_sentence(dd)
    for i in range(S):
        det.run(i, sentence(i))
    return det.collect(data.get('file_name'), sentence, selection=selection)
