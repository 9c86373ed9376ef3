#!/usr/bin/env python
"""Device time per sentence of the detection stage (model/detect_device.py detect_sentence: class-wise NMS, select, the n-row mask head,
the batched paste and the batched run-length encoder) on the heads' outputs of one sentence of the full-size ResNet-101 'cycle' network
(initial weights, bf16, a 600 x 1000 SyntheticLoader image: post = 300, C = 81, canvas 375 x 625), by HIP events, stage by stage; next to
the host restatement of NMS + select on the same outputs (tests/detect_util.py: numpy, including the D2H of the three matrices; it has
no mask stage, so it is a lower bound of a host path).  --judge 1: also the judge stage behind it (l2s_detect_gt_iou, l2s_detect_choose)
and the bytes per second l2s_detect_gt_iou achieves on the detections' boxes.  Prints one JSON line."""
import argparse
import json
import os.path as osp
import sys
import time

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, osp.join(ROOT, 'tools'))
sys.path.insert(0, osp.join(ROOT, 'tests'))

import numpy as np
import torch

from eval_bench import _event_us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='bf16'); ap.add_argument('--max_per_image', type=int, default=100)
    ap.add_argument('--thresh', type=float, default=0.0); ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    ap.add_argument('--judge', type=int, default=0, help='1: also time the judge stage (l2s_detect_gt_iou, l2s_detect_choose) behind the sentence')
    a = ap.parse_args()
    import detect_util as DU
    from lang2seg_amd import ops as O
    from lang2seg_amd.model.config import cfg, cfg_from_file
    from lang2seg_amd.model import detect_device as DD, eval_device as ED
    from lang2seg_amd.model.test import detect_from_outputs
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    from opt import parse_opt
    torch.cuda.set_device(0)
    T, V = 10, 1999
    b = SyntheticLoader(num_images=1, sents_per_image=1, H=600, W=1000, T=T, vocab_size=V, seed=1234)._image(0)
    opt = parse_opt([])
    opt.update(vocab_size=V, C4_feat_dim=1024, seq_length=T)
    if osp.exists(osp.join(ROOT, 'experiments/cfgs/res101.yml')):
        cfg_from_file(osp.join(ROOT, 'experiments/cfgs/res101.yml'))
    cfg.COMPUTE_DTYPE = a.dtype
    net = resnetv1(opt, batch_size=1, num_layers=101, variant='cycle')
    net.create_architecture(81, tag='default', anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    net.eval()
    img, lab_d, lens, box_d, gm = ED._upload_image(net, b, 1)
    im_info = np.asarray(b['im_info'], dtype=np.float32).reshape(-1)[:3]
    scale, ih, iw = ED._geometry(im_info)
    d = dict(data=img, im_info=im_info, S=1, labels=lab_d[0, :lens[0]], T=lens[0])
    net.forward_test_image(d)
    s = net.forward_test_sentence(d)
    C, post, cap = net._num_classes, s['post'], DD.default_cap(a.max_per_image)
    heads = dict(cls_prob=s['cls_prob'].clone(), bbox_pred=s['bbox_pred'].clone(), rois=s['rois'].clone())
    sent = dict(s); sent.update(heads)                          # (copies: the mask head pass may reuse the heads' buffers)
    out = DD.detect_sentence(net, sent, scale, ih, iw, a.max_per_image, a.thresh, cap)
    torch.cuda.synchronize()
    written, total = (int(v) for v in out['count'].cpu())
    res = dict(metric='detect_stage_us_per_sentence', dtype=a.dtype, post=post, classes=C, max_per_image=a.max_per_image, thresh=a.thresh,
               cap=cap, canvas=[ih, iw], nkeep=post if s['nkeep'] is None else int(s['nkeep'].cpu()[0]), detections=total, written=written,
               iters=a.iters)

    def stage():
        out['cursor'].zero_()
        DD.detect_sentence(net, sent, scale, ih, iw, a.max_per_image, a.thresh, cap, rec=out['rec'], count=out['count'], spans=out['spans'],
                           pool=out['pool'], cursor=out['cursor'])
    t_zero = _event_us(lambda: out['cursor'].zero_(), a.iters)
    res['device_stage_us'] = _event_us(stage, a.iters) - t_zero
    # stage by stage, on the buffers the full call left
    ws = net.buf('det.ws', ((O.detect_ws_bytes(post, C) + 3) // 4,), torch.int32)
    roi = net.buf('det.mask_rois', (cap, 5), torch.float32); lab = net.buf('det.mask_labels', (cap,), torch.int32)
    Hc, Wc = s['net_conv_hw']
    rws = net.buf('det.rle_ws', (cap * O.rle_encode_ws_words(ih, iw),), torch.int32)
    res['nms_us'] = _event_us(lambda: O.detect_nms(sent['cls_prob'], sent['bbox_pred'], sent['rois'], s['nkeep'], post, C, scale, ih, iw,
                                                   cfg.TEST.BBOX_REG, a.thresh, float(cfg.TEST.NMS), ws), a.iters)
    res['select_us'] = _event_us(lambda: O.detect_select(ws, post, C, a.max_per_image, scale, out['rec'], roi, lab, cap, out['count']), a.iters)
    res['mask_head_us'] = _event_us(lambda: net._roi_heads_test(s['net_conv'], Hc, Wc, roi, cap, labels=lab), a.iters)
    res['paste_us'] = _event_us(lambda: O.detect_paste(out['mask_prob'], out['rec'], out['count'], ih, iw, out['canvases']), a.iters)

    def enc():
        out['cursor'].zero_()
        O.rle_from_masks(out['canvases'], out['count'][0:1], out['pool'], out['cursor'], out['spans'], rws)
    res['encode_us'] = _event_us(enc, a.iters) - t_zero
    # the host restatement of NMS + select on the same outputs, D2H of the matrices included
    host = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cp, bp, rr = heads['cls_prob'].cpu().numpy(), heads['bbox_pred'].cpu().numpy(), heads['rois'].cpu().numpy()
        t1 = time.perf_counter()
        n = res['nkeep']
        scores, boxes = detect_from_outputs(cp[:n], bp[:n], rr[:n], im_info.reshape(1, 3))
        y = DU.detect_yardstick(scores, boxes, a.thresh, float(cfg.TEST.NMS), a.max_per_image)
        host.append((time.perf_counter() - t0, t1 - t0))
    host.sort()
    res['host_nms_select_us'] = host[len(host) // 2][0] * 1e6
    res['host_d2h_us'] = host[len(host) // 2][1] * 1e6
    res['host_detections'] = int(y[0].size)
    if a.judge:
        # the judge stage behind the same sentence (model/detect_device.py _JudgeStage): its two launches on the canvases and records the
        # detection stage left, with a synthetic expression score (the captioner is the rows stage's time, not this one's)
        stage = DD._JudgeStage(net, gm[:1], box_d[:1], scale, [lens[0] + 1], rerank=[0.0, 0.5, 4.0], with_expr=True)
        arr = stage.alloc(1, cap)
        choice, rows, area = stage._views(arr, 0, cap)
        expr = torch.from_numpy(-np.random.RandomState(0).rand(cap).astype(np.float32) * 30).cuda()
        cnt = out['count'][0:1]

        def judge():
            O.memset_zero(arr)
            stage.run(0, arr, out['canvases'], out['rec'], cnt, cap, expr)
        t_zero = _event_us(lambda: O.memset_zero(arr), a.iters)
        res['judge_stage_us'] = _event_us(judge, a.iters) - t_zero
        res['judge_zero_us'] = t_zero                               # (in the product the image's array is zeroed once, at its allocation)

        def gt_iou():
            O.memset_zero(arr)
            O.detect_gt_iou(out['canvases'], out['rec'], cnt, gm[0], box_d[0], scale, rows, area, clear=False)
        res['gt_iou_us'] = _event_us(gt_iou, a.iters) - t_zero
        res['choose_us'] = _event_us(lambda: O.detect_choose(out['rec'], rows, cnt, cap, area, choice, expr, stage.lambdas, False, lens[0] + 1), a.iters)
        # what l2s_detect_gt_iou streams: every detection's box of its canvas, and the resized gt once (its gathers under set pixels hit
        # the cache); the canvases as a whole are written * ih * iw bytes
        _, _, box, _, _ = O.det_record_fields(out['rec'].cpu())
        f = np.float32
        bx = np.clip(box[:written], 0, [f(iw - 1), f(ih - 1), f(iw - 1), f(ih - 1)]).astype(f)
        bw, bh = (bx[:, 2] - bx[:, 0] + f(1)).astype(np.int64), (bx[:, 3] - bx[:, 1] + f(1)).astype(np.int64)
        res['gt_iou_box_bytes'] = int((bw * bh).sum())
        res['gt_iou_gt_bytes'] = int(ih * iw)
        res['gt_iou_whole_canvas_bytes'] = int(written * ih * iw)
        res['gt_iou_GBps'] = (res['gt_iou_box_bytes'] + res['gt_iou_gt_bytes']) / (res['gt_iou_us'] * 1e-6) / 1e9
        res['judge_rules'] = stage.names
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
