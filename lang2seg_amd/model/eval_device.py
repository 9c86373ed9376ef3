"""Evaluation on the device: model/test.py eval_split (and test_vgg.eval_split) with one backbone pass per image and no host
synchronisation per sentence.  Per image: one H2D of every sentence's inputs (labels padded to the image's longest, gt boxes, gt
masks unless the loader keeps them in HBM), Network.forward_test_image once, then per sentence Network.forward_test_sentence, the
pick kernel (csrc/eval.hip l2s_eval_pick: best_detection + detect_from_outputs + computeIoU_box), the n = 1 mask head on the picked
box and the mask / IoU kernel (l2s_eval_mask_iou: segment_from_mask_prob + nearest gt resize + computeIoU_seg).  Each sentence
leaves one fixed-size record in a device array; the host reads the records once and reduces them with eval_split's own
expressions, so the metrics are the host loop's by construction.  With world > 1, rank r takes the images at positions
p = r (mod world) of the split and the integer totals are summed with one all_reduce."""
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


def _eval_image(net, data, n_sent, rec, base, with_masks):
    """every sentence of one image through the device path; record base + i for sentence i.  No host synchronisation."""
    img, lab_d, lens, box_d, gm = _upload_image(net, data, n_sent)
    im_info = np.asarray(data['im_info'], dtype=np.float32).reshape(-1)[:3]
    scale, ih, iw = _geometry(im_info)
    d = dict(data=img, im_info=im_info, S=1)
    net.forward_test_image(d)
    MS = int(cfg.MASK_SIZE)
    roi = net.buf('eval.mask_roi', (1, 5), torch.float32)
    lab = net.buf('eval.mask_label', (1,), torch.int32)
    for i in range(n_sent):
        d['labels'] = lab_d[i, :lens[i]]
        d['T'] = lens[i]
        s = net.forward_test_sentence(d)
        O.eval_pick(s['cls_prob'], s['bbox_pred'], s['rois'], s['nkeep'], s['post'], net._num_classes, scale, ih, iw, box_d[i],
                    cfg.TEST.BBOX_REG, rec, base + i, roi, lab)
        if with_masks:
            Hc, Wc = s['net_conv_hw']
            mprob = net.predict_mask_device(s['net_conv'], Hc, Wc, roi, lab).view(MS, MS)
            O.eval_mask_iou(mprob, rec, base + i, gm[i], ih, iw)


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


def _run(loader, model, split, opt, rank, world, details, with_masks, progress):
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
            _eval_image(model, data, n, rec, 0, with_masks)
            chunks.append(rec)
            issued += n
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
        v = torch.tensor([tot.loss_evals, tot.acc, int(tot.cum_I), int(tot.cum_U)] + [int(c) for c in tot.seg_correct], dtype=torch.int64)
        if dist.get_backend() != 'gloo':
            v = v.to(device)
        dist.all_reduce(v, op=dist.ReduceOp.SUM)
        v = v.cpu().numpy()
        tot.loss_evals = tot.num_sent = int(v[0]); tot.acc = int(v[1])
        tot.cum_I, tot.cum_U = np.int64(v[2]), np.int64(v[3])
        tot.seg_correct = v[4:].astype(np.int32)
        tot.seg_total = tot.loss_evals if with_masks else 0
    return tot


def eval_split_device(loader, model, crit, split, opt, rank=0, world=1, details=None):
    """model/test.py eval_split on the device.  Returns its 7-tuple (acc, eval_seg_iou_list, seg_correct, seg_total, cum_I, cum_U,
    num_sent).  details: a list that receives (pred_roi, pred_class, pred_box, hit, I, U) per sentence of this rank."""
    def progress(data, t):
        b = data['bounds']
        print('evaluating [%s] ... image[%d/%d]\'s sents, det acc=%.2f%%, seg acc=%.2f%%, seg IoU=%.2f%%' % (
            split, b['it_pos_now'], b['it_max'], t.acc * 100.0 / max(t.loss_evals, 1), t.seg_correct[0] * 100.0 / max(t.seg_total, 1),
            t.cum_I * 100.0 / max(t.cum_U, 1)))
    t = _run(loader, model, split, opt, rank, world, details, True, progress)
    return t.acc / t.loss_evals, EVAL_SEG_IOU_LIST, t.seg_correct, t.seg_total, t.cum_I, t.cum_U, t.num_sent


def eval_split_vgg_device(loader, model, crit, split, opt, rank=0, world=1, details=None):
    """model/test_vgg.py eval_split on the device (boxes only: the VGG16 network has no mask branch) -> (acc, num_sent)"""
    def progress(data, t):
        print('evaluating [%s] ... sent %d, det acc=%.2f%%' % (split, t.loss_evals, t.acc * 100.0 / max(t.loss_evals, 1)))
    t = _run(loader, model, split, opt, rank, world, details, False, progress)
    return t.acc * 1.0 / max(t.loss_evals, 1), t.loss_evals
