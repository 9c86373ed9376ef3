"""Evaluation on the device: model/test.py eval_split (and test_vgg.eval_split) with one backbone pass per image and no host
synchronisation per sentence.  Per image: one H2D of every sentence's inputs (labels padded to the image's longest, gt boxes, gt
masks unless the loader keeps them in HBM), Network.forward_test_image once, then per sentence Network.forward_test_sentence, the
pick kernel (csrc/eval.hip l2s_eval_pick: best_detection + detect_from_outputs + computeIoU_box), the n = 1 mask head on the picked
box and the mask / IoU kernel (l2s_eval_mask_iou: segment_from_mask_prob + nearest gt resize + computeIoU_seg).  Each sentence
leaves one fixed-size record in a device array; the host reads the records once and reduces them with eval_split's own
expressions, so the metrics are the host loop's by construction.  With world > 1, rank r takes the images at positions
p = r (mod world) of the split and the integer totals are summed with one all_reduce.

Predictions (opt-in, `predictions=[]`): the mask / IoU kernel also stores each sentence's canvas, l2s_rle_from_mask (csrc/rle_encode.hip)
turns it into COCO run lengths in a per-image pool on the device, and one read-back per image brings the records, the spans and the
used part of the pool to the host, where the counts become the `counts` string of the reference's mask.encode."""
import numpy as np
import torch

from .. import ops as O
from .config import cfg

EVAL_SEG_IOU_LIST = [.5, .6, .7, .8, .9]


def _geometry(im_info):
    """(im_scale, ih, iw): model/test.py detect_from_outputs / segment_from_mask_prob in float32, round half to even"""
    im_info = np.asarray(im_info, dtype=np.float32).reshape(-1, 3)
    scale = im_info[0][2]
    return scale, int(round(im_info[0][0] / scale)), int(round(im_info[0][1] / scale))


def _sentence_labels(labels, i):
    """the labels eval_split hands to upload_blob for sentence i: the first count-of-nonzero tokens, then the same cut again"""
    lab = labels[i, :int((labels[i] != 0).sum())]
    return lab[:int((lab != 0).sum())]


def _align(n, a=256):
    return (n + a - 1) // a * a


def _upload_image(net, data, n_sent):
    """one H2D for every sentence of the image -> (image blob, labels int64 [S][Tm], lengths, gt boxes f32 [S][4] view, gt masks [S] views)"""
    dev = dict.get(data, '_device', None) or {}
    device = torch.device(net.device)
    if 'data' in dev:
        img = dev['data']
    else:
        img = torch.from_numpy(np.ascontiguousarray(data['data'], dtype=np.float32)).to(device)
    labels = np.asarray(data['labels'])
    labs = [_sentence_labels(labels, i) for i in range(n_sent)]
    lens = [int(l.shape[0]) for l in labs]
    Tm = max(max(lens), 1)
    lab = np.zeros((n_sent, Tm), np.int64)
    for i, l in enumerate(labs):
        lab[i, :l.shape[0]] = l
    box = np.ascontiguousarray(np.asarray(data['gt_boxes'])[:n_sent, :4], dtype=np.float32)
    on_device = '_gt_masks_ref' in dev                        # loaders/cycle_loader.py: one device mask per referred object
    masks = None if on_device else np.ascontiguousarray(np.asarray(data['gt_masks'])[:n_sent], dtype=np.uint8)
    o_box = _align(lab.nbytes); o_mask = _align(o_box + box.nbytes)
    buf = np.zeros(o_mask + (0 if masks is None else masks.nbytes), np.uint8)
    buf[:lab.nbytes] = lab.view(np.uint8).reshape(-1)
    buf[o_box:o_box + box.nbytes] = box.view(np.uint8).reshape(-1)
    if masks is not None:
        buf[o_mask:] = masks.reshape(-1)
    src = torch.from_numpy(buf)
    if device.type == 'cuda':
        g = src.pin_memory().to(device, non_blocking=True)
    else:
        g = src.to(device)
    lab_d = g[:lab.nbytes].view(torch.int64).view(n_sent, Tm)
    box_d = g[o_box:o_box + box.nbytes].view(torch.float32).view(n_sent, 4)
    if on_device:
        ref = dev['_sent_ref_host']
        gm = [dev['_gt_masks_ref'][ref[i]] for i in range(n_sent)]
    else:
        Hs, Ws = masks.shape[1], masks.shape[2]
        gm = [g[o_mask + i * Hs * Ws:o_mask + (i + 1) * Hs * Ws].view(Hs, Ws) for i in range(n_sent)]
    return img, lab_d, lens, box_d, gm             # (freeing g behind the launches is safe: the allocator reuses it in stream order)


def rle_encode_host(mask):
    """maskApi.c:32-41 rleEncode on a host [h][w] mask -> uint32 counts (the fallback of a sentence whose counts overflowed the pool)"""
    t = np.asarray(mask).T.reshape(-1) != 0
    pos = np.flatnonzero(t != np.concatenate([[False], t[:-1]]))
    return np.diff(np.concatenate([[0], pos, [t.size]])).astype(np.uint32)


class _Export(object):
    """the device side of one image's predictions: S canvases, the run-length pool with its cursor and spans, the picked scores"""

    def __init__(self, device, S, ih, iw, with_masks, pool_words=None):
        self.S, self.ih, self.iw, self.with_masks = S, ih, iw, with_masks
        # meta: the pool cursor, S spans (off, n), S float32 scores
        self.meta = torch.zeros((1 + 3 * S,), dtype=torch.int32, device=device)
        self.scores = self.meta[1 + 2 * S:].view(torch.float32)
        if with_masks:
            # a budget, not a bound: Pillow's BILINEAR upscale of MASK_SIZE rows crosses the threshold at most ~MASK_SIZE times per
            # column (8651 counts for a 14 x 14 checkerboard over 640 x 640); a sentence beyond it is encoded on the host
            words = S * (iw * (int(cfg.MASK_SIZE) + 2) + 2) if pool_words is None else int(pool_words)
            self.canvas = torch.empty((S, ih, iw), dtype=torch.uint8, device=device)
            self.pool = torch.empty((max(words, 1),), dtype=torch.int32, device=device)
            self.ws = torch.empty((O.rle_encode_ws_words(ih, iw),), dtype=torch.int32, device=device)

    def score(self, rec, k, i, cls_prob, C):
        """cls_prob at the pick of record k, gathered behind the pick kernel (index 0 when nothing was picked)"""
        r = rec.view(torch.int32).view(-1, O.EVAL_RECORD_BYTES // 4)[k]
        idx = (r[0:1].to(torch.int64) * C + r[1:2]).clamp_(min=0)
        self.scores[i:i + 1].copy_(cls_prob.reshape(-1).index_select(0, idx))

    def encode(self, i):
        O.rle_from_mask(self.canvas[i], self.pool, self.meta[0:1], self.meta[1 + 2 * i:3 + 2 * i], self.ws)

    def collect(self, rec_h, file_name, gt=True):
        """the read-back (meta, then the used prefix of the pool) -> one dict per sentence"""
        S = self.S
        meta = self.meta.cpu().numpy()
        roi, cls, box, hit, Is, Us = O.eval_record_fields(rec_h)
        scores = meta[1 + 2 * S:].view('<f4')
        if self.with_masks:
            pool = self.pool[:int(meta[0])].cpu().numpy().view('<u4')
        out = []
        for i in range(S):
            p = dict(file_name=file_name, sent_index=i, category_id=int(cls[i]), box=[float(v) for v in box[i]], score=float(scores[i]))
            if gt:
                p.update(hit=int(hit[i]), I=int(Is[i]), U=int(Us[i]))
            else:
                p['area'] = int(Us[i])
            if self.with_masks:
                off, n = int(meta[1 + 2 * i]), int(meta[2 + 2 * i])
                cnts = pool[off:off + n] if off >= 0 else rle_encode_host(self.canvas[i].cpu().numpy())
                p['segmentation'] = dict(size=[self.ih, self.iw], counts=O.rle_to_string(cnts))
            out.append(p)
        return out


def _eval_image(net, data, n_sent, rec, base, with_masks, pool_words=-1, detect=None, caption=None, speaker=None):
    """every sentence of one image through the device path; record base + i for sentence i.  No host synchronisation.
    pool_words >= 0 or None: also keep the predictions on the device (None: the default pool budget) -> the image's _Export.
    detect: None, or a dict (max_per_image, thresh) that asks for every detection of each sentence too (model/detect_device.py) and
    receives 'detector' (the image's _Detector) and 'sentence' (forward_test_sentence of sentence i again, for its re-runs)
    caption: None, or a callable (i, the sentence's outputs, the image's _Export) run behind sentence i's mask, while the sentence's
    buffers are still its own (model/caption_device.py)
    speaker: None, or the image's model/caption_eval.py ImageStage: it receives the ground-truth masks on the device and runs behind
    sentence i's mask as `caption` does"""
    img, lab_d, lens, box_d, gm = _upload_image(net, data, n_sent)
    if speaker is not None:
        speaker.gm = gm
    im_info = np.asarray(data['im_info'], dtype=np.float32).reshape(-1)[:3]
    scale, ih, iw = _geometry(im_info)
    d = dict(data=img, im_info=im_info, S=1)
    net.forward_test_image(d)
    MS = int(cfg.MASK_SIZE)
    roi = net.buf('eval.mask_roi', (1, 5), torch.float32)
    lab = net.buf('eval.mask_label', (1,), torch.int32)
    ex = None if pool_words == -1 else _Export(torch.device(net.device), n_sent, ih, iw, with_masks, pool_words)

    def sentence(i):
        d['labels'] = lab_d[i, :lens[i]]
        d['T'] = lens[i]
        return net.forward_test_sentence(d)
    det = None
    if detect is not None:
        from .detect_device import _Detector
        from .detect_device import rows_stage
        stage = rows_stage(net, np.asarray(data['labels'])[:n_sent], detect.get('describe'), detect.get('expr_score'), detect.get('ix_to_word'),
                           detect.get('beam_size', 1))
        judge = None
        if detect.get('judge') or detect.get('rerank') or detect.get('per_token'):
            from .detect_device import judge_stage
            judge = judge_stage(net, np.asarray(data['labels'])[:n_sent], gm, box_d, scale, detect.get('judge'), detect.get('rerank'),
                                detect.get('per_token'), detect.get('expr_score'))
        det = detect['detector'] = _Detector(net, n_sent, scale, ih, iw, detect.get('max_per_image', 100), detect.get('thresh', 0.0), stage=stage,
                                             judge=judge)
        detect['sentence'] = sentence
    for i in range(n_sent):
        s = sentence(i)
        O.eval_pick(s['cls_prob'], s['bbox_pred'], s['rois'], s['nkeep'], s['post'], net._num_classes, scale, ih, iw, box_d[i],
                    cfg.TEST.BBOX_REG, rec, base + i, roi, lab)
        if ex is not None:
            ex.score(rec, base + i, i, s['cls_prob'], net._num_classes)
        if with_masks:
            Hc, Wc = s['net_conv_hw']
            mprob = net.predict_mask_device(s['net_conv'], Hc, Wc, roi, lab).view(MS, MS)
            O.eval_mask_iou(mprob, rec, base + i, gm[i], ih, iw, canvas=None if ex is None else ex.canvas[i])
            if ex is not None:
                ex.encode(i)
        if caption is not None:
            caption(i, s, ex)
        if speaker is not None:
            speaker.caption(i, s, ex)
        if det is not None:                                   # last: its mask head pass reuses the heads' buffers
            det.run(i, s)
    return ex


class _Totals(object):
    """eval_split's running sums, fed from host records with eval_split's own expressions"""

    def __init__(self):
        self.acc, self.loss_evals, self.num_sent, self.seg_total = 0, 0, 0, 0
        self.cum_I, self.cum_U = 0, 0
        self.seg_correct = np.zeros(len(EVAL_SEG_IOU_LIST), dtype=np.int32)

    def add(self, recs, details=None, with_masks=True):
        roi, cls, box, hit, Is, Us = O.eval_record_fields(recs)
        for j in range(recs.shape[0]):
            if roi[j] < 0:
                raise ValueError('evaluation: no proposal to pick from (empty score matrix), as np.max would raise in best_detection')
            if hit[j]:
                self.acc += 1
            self.loss_evals += 1
            if with_masks:
                I, U = Is[j], Us[j]                            # np.int64, as computeIoU_seg returns them
                self.cum_I += I; self.cum_U += U
                with np.errstate(divide='ignore', invalid='ignore'):
                    for k, t in enumerate(EVAL_SEG_IOU_LIST):
                        self.seg_correct[k] += (I * 1.0 / U >= t)
                self.seg_total += 1
            self.num_sent += 1
            if details is not None:
                details.append((int(roi[j]), int(cls[j]), box[j].copy(), int(hit[j]), int(Is[j]), int(Us[j])))


class _RuleTotals(object):
    """_Totals' sums for one rule of the judge stage, fed from its choice records with _Totals.add's own expressions"""

    def __init__(self):
        self.acc, self.num_sent, self.cum_I, self.cum_U = 0, 0, 0, 0
        self.seg_correct = np.zeros(len(EVAL_SEG_IOU_LIST), dtype=np.int32)

    def add(self, choice):
        if choice['hit']:
            self.acc += 1
        I, U = np.int64(choice['I']), np.int64(choice['U'])
        self.cum_I += I; self.cum_U += U
        with np.errstate(divide='ignore', invalid='ignore'):
            for k, t in enumerate(EVAL_SEG_IOU_LIST):
                self.seg_correct[k] += (I * 1.0 / U >= t)
        self.num_sent += 1

    def ints(self):
        return [self.num_sent, self.acc, int(self.cum_I), int(self.cum_U)] + [int(c) for c in self.seg_correct]

    def set_ints(self, v):
        self.num_sent, self.acc, self.cum_I, self.cum_U = int(v[0]), int(v[1]), np.int64(v[2]), np.int64(v[3])
        self.seg_correct = np.asarray(v[4:4 + len(EVAL_SEG_IOU_LIST)]).astype(np.int32)

    def as_dict(self):
        return dict(acc=self.acc, num_sent=self.num_sent, seg_correct=[int(c) for c in self.seg_correct], cum_I=int(self.cum_I),
                    cum_U=int(self.cum_U))


def check_judge_options(detections, judge, rerank, per_token, expr_score, variant=None):
    """the ValueErrors of the judging options, each naming the options (and tool flags) involved, before anything runs -> the lambdas"""
    from .detect_device import check_rerank
    lambdas = check_rerank(rerank)
    on = [n for n, v in (('judge (--judge_detections)', judge), ('rerank (--rerank)', lambdas), ('per_token (--rerank_per_token)', per_token)) if v]
    if on and not detections:
        raise ValueError('%s judge the detections: they need detections (--dump_detections)' % ', '.join(on))
    if lambdas and not expr_score:
        raise ValueError('rerank (--rerank) weighs the expression\'s log-likelihood: it needs expr_score (--expr_score 1)')
    if per_token and not lambdas:
        raise ValueError('per_token (--rerank_per_token) divides the re-ranking term: it needs rerank (--rerank)')
    if on and variant == 'vgg':
        raise ValueError('%s compare masks: --variant vgg has no mask branch' % ', '.join(on))
    return lambdas


def _run(loader, model, split, opt, rank, world, details, with_masks, progress, predictions=None, pool_words=None, detections=None,
         describe=False, expr_score=False, judge=False, rerank=None, per_token=False, selection=None, selection_totals=None, beam_size=1,
         caption_eval=False, caption_describe=False, caption_totals=None):
    if (caption_describe or caption_totals is not None) and not caption_eval:
        raise ValueError('caption_describe / caption_totals (--caption_eval_describe) belong to the speaker\'s evaluation: they need '
                         'caption_eval (--caption_eval 1)')
    ctot = None
    if caption_eval:
        from .caption_eval import CaptionTotals, ImageStage, check_variant
        check_variant(model)                                    # names the variant, before anything runs
        ctot = CaptionTotals()
    if (describe or expr_score) and detections is None:
        raise ValueError('describe / expr_score (--describe, --expr_score) add fields to the detections: they need detections (--dump_detections)')
    lambdas = check_judge_options(detections is not None, judge, rerank, per_token, expr_score, None if with_masks else 'vgg')
    judging = bool(judge or lambdas)
    if (selection is not None or selection_totals is not None) and not judging:
        raise ValueError('selection / selection_totals (--dump_selection) receive the judge stage\'s choices: they need judge (--judge_detections) '
                         'or rerank (--rerank)')
    rule_tot = {}
    if judging:
        from .detect_device import rule_names
        rule_tot = {name: _RuleTotals() for name in rule_names(lambdas, expr_score)}      # (a dict keeps the rules' order)
    sel = [] if judging and selection is None else selection
    num_sents = opt.get('num_sents', -1)
    verbose = opt.get('verbose', True)
    if world > 1 and num_sents > 0:
        raise ValueError('num_sents > 0 cuts the split at a sentence count, which does not shard over ranks: evaluate it on one rank')
    if not 0 <= rank < world:
        raise ValueError('rank %d of world %d' % (rank, world))
    model.eval()
    tot = _Totals()
    device = torch.device(model.device)
    chunks = []                                                # the records of each image not read back yet
    n_img = len(loader.split_ix[split])
    if world > 1:
        loader.iterators[split] = rank                         # this rank's first image; getTestBatch(stride=world) from there
    issued = 0
    if rank < n_img:
        while True:
            data = loader.getTestBatch(split, stride=world) if world > 1 else loader.getTestBatch(split)
            n = int(np.asarray(data['labels']).shape[0])
            if num_sents > 0:
                n = min(n, num_sents - issued)
            rec = O.eval_records(n, device)
            dopt = None if detections is None else dict(max_per_image=opt.get('max_per_image', 100), thresh=opt.get('det_thresh', 0.0),
                                                        describe=describe, expr_score=expr_score, ix_to_word=getattr(loader, 'ix_to_word', None),
                                                        beam_size=beam_size)
            if judging:
                dopt.update(judge=True, rerank=lambdas, per_token=per_token)
            if caption_eval:
                speaker = ImageStage(model, np.asarray(data['labels'])[:n], None, caption_describe, beam_size,
                                     opt.get('ix_to_word') or getattr(loader, 'ix_to_word', None))
                ex = _eval_image(model, data, n, rec, 0, with_masks, -1 if predictions is None else pool_words, detect=dopt, speaker=speaker)
            elif dopt is None:
                ex = _eval_image(model, data, n, rec, 0, with_masks, -1 if predictions is None else pool_words)
            else:
                ex = _eval_image(model, data, n, rec, 0, with_masks, -1 if predictions is None else pool_words, detect=dopt)
            chunks.append(rec)
            issued += n
            if ex is not None:                                 # one read-back per image: records, spans and cursor, then the pool's used part
                rec_h = rec.cpu()
                predictions.extend(ex.collect(rec_h, data.get('file_name')))
                chunks[-1] = rec_h
            if caption_eval:                                   # one more read-back per image: every sentence's log-probabilities at once
                cf = speaker.fields()
                speaker.add_to(ctot, cf)
                if predictions is not None:
                    for p, q in zip(predictions[len(predictions) - n:], cf):
                        p.update(q)
            if dopt is not None:                               # one read-back per image; a sentence that did not fit its buffers runs again
                extra = dict(image_id=data['image_id']) if 'image_id' in data else None
                n_sel = len(sel) if judging else 0
                for lst in dopt['detector'].collect(data.get('file_name'), dopt['sentence'], extra, selection=sel if judging else None):
                    detections.extend(lst)
                if judging:
                    for entry in sel[n_sel:]:
                        for name, choice in entry['rules'].items():
                            rule_tot[name].add(choice)
            if verbose:                                        # one host synchronisation per image, for the progress line
                for r in chunks:
                    tot.add(r.cpu(), details, with_masks)
                chunks = []
                progress(data, tot)
            if (num_sents > 0 and issued >= num_sents) or data['bounds']['wrapped']:
                break
    if chunks:
        tot.add(torch.cat(chunks).cpu(), details, with_masks)  # the single read-back of the records
    if world > 1:
        import torch.distributed as dist
        base = [tot.loss_evals, tot.acc, int(tot.cum_I), int(tot.cum_U)] + [int(c) for c in tot.seg_correct]
        per_rule = [x for t in rule_tot.values() for x in t.ints()]                      # empty unless judging: the same one all_reduce
        v = torch.tensor(base + per_rule, dtype=torch.int64)
        if dist.get_backend() != 'gloo':
            v = v.to(device)
        dist.all_reduce(v, op=dist.ReduceOp.SUM)
        v = v.cpu().numpy()
        tot.loss_evals = tot.num_sent = int(v[0]); tot.acc = int(v[1])
        tot.cum_I, tot.cum_U = np.int64(v[2]), np.int64(v[3])
        tot.seg_correct = v[4:len(base)].astype(np.int32)
        tot.seg_total = tot.loss_evals if with_masks else 0
        w = 4 + len(EVAL_SEG_IOU_LIST)
        for k, t in enumerate(rule_tot.values()):
            t.set_ints(v[len(base) + k * w:len(base) + (k + 1) * w])
        if caption_eval:                                       # the speaker's float64 sums: one all_reduce of their own
            cv = torch.from_numpy(ctot.vector())
            if dist.get_backend() != 'gloo':
                cv = cv.to(device)
            dist.all_reduce(cv, op=dist.ReduceOp.SUM)
            ctot.set_vector(cv.cpu().numpy())
    if caption_totals is not None:
        caption_totals.update(ctot.as_dict())
    if selection_totals is not None:
        selection_totals.update((name, t.as_dict()) for name, t in rule_tot.items())
    return tot


def eval_split_device(loader, model, crit, split, opt, rank=0, world=1, details=None, predictions=None, _pool_words=None, detections=None,
                      describe=False, expr_score=False, judge=False, rerank=None, per_token=False, selection=None, selection_totals=None,
                      beam_size=1, caption_eval=False, caption_describe=False, caption_totals=None):
    """model/test.py eval_split on the device.  Returns its 7-tuple (acc, eval_seg_iou_list, seg_correct, seg_total, cum_I, cum_U,
    num_sent).  details: a list that receives (pred_roi, pred_class, pred_box, hit, I, U) per sentence of this rank.
    predictions: a list that receives one dict per sentence of this rank: file_name, sent_index (position in the image's test batch),
    category_id, box [x1, y1, x2, y2] (original image), score, hit, I, U and segmentation {'size': [ih, iw], 'counts': COCO RLE string}.
    detections: a list that receives every detection of every sentence of this rank (model/detect_device.py detect_image's dicts, flat;
    opt['max_per_image'] (100) and opt['det_thresh'] (0.0) are its limits).  Metrics and predictions do not depend on it.
    describe / expr_score: detect_image's options for those detections (the captioner on every detection; the expression's log-likelihood
    under every detection's mask); they need `detections` and the cycle network.  beam_size > 1 with describe: beam search on rows, the
    detections gain caption_beams.
    judge / rerank (a list of lambdas; implies judge) / per_token: detect_image's judging of every detection against the sentence's ground
    truth (I, U, hit per detection) and its rules; they need `detections`, rerank needs expr_score.  selection: a list that receives
    per sentence of this rank {file_name, sent_index, gt_area, rules: {rule: {det, category_id, hit, I, U, key}}}; selection_totals: a dict
    that receives per rule {acc, num_sent, seg_correct (at EVAL_SEG_IOU_LIST), cum_I, cum_U}, summed over the ranks.  Without them the
    launches and every returned bit are what they are without these options.
    caption_eval: the speaker's evaluation (model/caption_eval.py; cycle and cycle_response): every sentence's own expression, cut to
    seq_length tokens, scored teacher-forced under its ground-truth mask.  The predictions gain gt_expr_logprob and gt_expr_logprobs
    (n + 1 values); with caption_describe also gt_caption_tokens, gt_caption_logprobs, gt_caption_exact (greedy, or the best of beam_size
    beams) and gt_caption, the words, where opt['ix_to_word'] or the loader's ix_to_word names them.  caption_totals: a dict that receives num_sent, num_tok, loss (minus the sum of all log-probabilities over
    num_tok), perplexity, loss_per_image (the mean over images of LanguageModelCriterion on the image's sentences) and exact_match,
    summed over the ranks in float64.  Without caption_eval the launches are what they are without it.
    (_pool_words: the run-length pool of an image in words instead of its default budget; checks of the host fallback.)"""
    def progress(data, t):
        b = data['bounds']
        print('evaluating [%s] ... image[%d/%d]\'s sents, det acc=%.2f%%, seg acc=%.2f%%, seg IoU=%.2f%%' % (
            split, b['it_pos_now'], b['it_max'], t.acc * 100.0 / max(t.loss_evals, 1), t.seg_correct[0] * 100.0 / max(t.seg_total, 1),
            t.cum_I * 100.0 / max(t.cum_U, 1)))
    t = _run(loader, model, split, opt, rank, world, details, True, progress, predictions, _pool_words, detections, describe, expr_score,
             judge, rerank, per_token, selection, selection_totals, beam_size, caption_eval, caption_describe, caption_totals)
    return t.acc / t.loss_evals, EVAL_SEG_IOU_LIST, t.seg_correct, t.seg_total, t.cum_I, t.cum_U, t.num_sent


def eval_split_vgg_device(loader, model, crit, split, opt, rank=0, world=1, details=None, predictions=None, detections=None):
    """model/test_vgg.py eval_split on the device (boxes only: the VGG16 network has no mask branch) -> (acc, num_sent).
    predictions: as in eval_split_device, without I, U's mask meaning and without `segmentation`; detections: as there, boxes only"""
    def progress(data, t):
        print('evaluating [%s] ... sent %d, det acc=%.2f%%' % (split, t.loss_evals, t.acc * 100.0 / max(t.loss_evals, 1)))
    t = _run(loader, model, split, opt, rank, world, details, False, progress, predictions, detections=detections)
    return t.acc * 1.0 / max(t.loss_evals, 1), t.loss_evals
