#!/usr/bin/env python
"""Sentences per second of the evaluation loop: the host loop model/test.py eval_split vs the device path model/eval_device.py vs the
device path exporting its predictions (run-length masks, `predictions=[]`), on the same SyntheticLoader-style split shaped like RefCOCO
(8 images at 600 x {800, 900, 1000}, 7 sentences each, T = 10, V = 1999), the full-size ResNet-101 'cycle' network with its initial
weights, bf16.  One warm-up pass per leg, then `--rounds` timed rounds with the three legs alternating inside each round (the median
round is reported); then the encoder alone (`encoder`: device-event times in microseconds).
Device path timers: `issue_s` is the host time of the loop up to its last launch, `total_s` includes the final read-back.
Prints one JSON line."""
import argparse
import json
import os.path as osp
import sys
import time

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, osp.join(ROOT, 'tools'))

import numpy as np
import torch


class _Split(object):
    def __init__(self, blobs):
        self.blobs = blobs
        self.split_ix = {'val': list(range(len(blobs)))}
        self.iterators = {'val': 0}

    def getTestBatch(self, split, stride=1):
        i = self.iterators[split]
        nxt = i + stride
        wrapped = nxt >= len(self.blobs)
        self.iterators[split] = 0 if wrapped else nxt
        b = dict(self.blobs[i])
        b['bounds'] = dict(it_pos_now=i + 1, it_max=len(self.blobs), wrapped=wrapped)
        return b


def _event_us(fn, iters=200):
    """device time of one call of fn (HIP events around `iters` calls behind a warm-up), microseconds"""
    for _ in range(10):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def encoder_times(pred):
    """l2s_rle_from_mask alone (its three launches, back to back): a 480 x 640 mask of density 0.5 and the mask of one exported prediction,
    next to l2s_eval_mask_iou writing a canvas of that prediction's size"""
    from lang2seg_amd import ops as O
    rs = np.random.RandomState(0)
    h, w = pred['segmentation']['size']
    cnts = O.rle_from_string(pred['segmentation']['counts'])
    typical = np.zeros(h * w, np.uint8)
    pos = np.cumsum(cnts.astype(np.int64))
    for j in range(1, len(cnts), 2):
        typical[pos[j - 1]:pos[j]] = 1
    typical = np.ascontiguousarray(typical.reshape(w, h).T)
    out = {}
    for name, m in (('dense_480x640', (rs.uniform(0, 1, (480, 640)) < 0.5).astype(np.uint8)), ('typical', typical)):
        md = torch.from_numpy(m).cuda()
        pool = torch.empty((m.size + 1,), dtype=torch.int32, device='cuda')
        cs = torch.zeros((3,), dtype=torch.int32, device='cuda')
        ws = torch.empty((O.rle_encode_ws_words(*m.shape),), dtype=torch.int32, device='cuda')

        def enc():
            cs.zero_()
            O.rle_from_mask(md, pool, cs[0:1], cs[1:3], ws)
        t_enc = _event_us(enc)
        t_zero = _event_us(lambda: cs.zero_())
        out[name] = dict(h=int(m.shape[0]), w=int(m.shape[1]), counts=int(cs[2].item()), encode_us=t_enc - t_zero)
    prob = torch.from_numpy(rs.uniform(0, 1, (14, 14)).astype(np.float32)).cuda()
    rec = O.eval_records(1)
    rec.view(torch.int32)[0, 2:6].view(torch.float32).copy_(torch.tensor(pred['box'], dtype=torch.float32))
    gt = torch.from_numpy(typical).cuda()
    canvas = torch.empty((h, w), dtype=torch.uint8, device='cuda')
    out['typical']['eval_mask_iou_us'] = _event_us(lambda: O.eval_mask_iou(prob, rec, 0, gt, h, w))
    out['typical']['eval_mask_iou_canvas_us'] = _event_us(lambda: O.eval_mask_iou(prob, rec, 0, gt, h, w, canvas=canvas))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8); ap.add_argument('--sents', type=int, default=7)
    ap.add_argument('--dtype', default='bf16'); ap.add_argument('--variant', default='cycle')
    ap.add_argument('--rounds', type=int, default=3, help='timed rounds; the three legs alternate inside each round')
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    from lang2seg_amd.model.config import cfg, cfg_from_file
    from lang2seg_amd.model.test import eval_split
    from lang2seg_amd.model import eval_device as ED
    from lang2seg_amd import ops as O
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    from opt import parse_opt
    torch.cuda.set_device(0)
    T, V = 10, 1999
    blobs = []
    for j in range(a.images):
        W = (800, 900, 1000)[j % 3]
        b = SyntheticLoader(num_images=1, sents_per_image=a.sents, H=600, W=W, T=T, vocab_size=V, seed=1234 + 31 * j)._image(0)
        blobs.append({k: v for k, v in b.items() if k in ('data', 'im_info', 'gt_boxes', 'gt_masks', 'labels', 'file_name')})
    opt = parse_opt([])
    opt.update(vocab_size=V, C4_feat_dim=1024, seq_length=T)
    if osp.exists(osp.join(ROOT, 'experiments/cfgs/res101.yml')):
        cfg_from_file(osp.join(ROOT, 'experiments/cfgs/res101.yml'))
    cfg.COMPUTE_DTYPE = a.dtype
    net = resnetv1(opt, batch_size=1, num_layers=101, variant=a.variant)
    net.create_architecture(81, tag='default', anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    n = a.images * a.sents
    out = dict(metric='eval_sentences_per_s', images=a.images, sents_per_image=a.sents, dtype=a.dtype, variant=a.variant, rounds=a.rounds)
    res, times, preds = {}, {}, []

    def run(path):
        """one pass of one leg -> (result, total seconds, issue seconds)"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if path == 'host':
            r = eval_split(_Split(blobs), net, None, 'val', dict(verbose=False))
            t_issue = time.perf_counter()
        else:
            tot = [None]
            orig = ED._Totals.add

            def add(self, recs, details=None, with_masks=True, _o=orig):
                tot[0] = time.perf_counter() if tot[0] is None else tot[0]
                return _o(self, recs, details, with_masks)
            # the issue time: up to the read-back of the records (the first host wait of the path; the export leg reads back per image)
            ED._Totals.add = add
            del preds[:]
            try:
                r = ED.eval_split_device(_Split(blobs), net, None, 'val', dict(verbose=False), predictions=preds if path == 'export' else None)
            finally:
                ED._Totals.add = orig
            t_issue = tot[0]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return r, t1 - t0, t_issue - t0
    legs = ('host', 'device', 'export')
    for path in legs:                                          # warm-up
        run(path)
    for rep in range(a.rounds):                                # timed rounds, the legs interleaved
        for path in legs:
            r, total, issue = run(path)
            res[path] = r
            times.setdefault(path, []).append((total, issue))
    for path in legs:
        total, issue = sorted(times[path])[len(times[path]) // 2]          # the median round
        out[path + '_sents_per_s'] = n / total
        out[path + '_total_s'] = total
        out[path + '_issue_s'] = issue
        out[path + '_rounds_sents_per_s'] = [n / t for t, _ in times[path]]
    out['speedup'] = out['device_sents_per_s'] / out['host_sents_per_s']
    out['export_speedup'] = out['export_sents_per_s'] / out['host_sents_per_s']
    out['export_above_host'] = bool(out['export_sents_per_s'] > out['host_sents_per_s'])
    out['same_metrics'] = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(res['host'], res['device']))
    out['export_same_metrics'] = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(res['device'], res['export']))
    out['export_predictions'] = len(preds)
    out['export_counts_per_mask'] = float(np.mean([len(O.rle_from_string(p['segmentation']['counts'])) for p in preds]))
    out['host_result'] = [float(res['host'][0]), [int(v) for v in res['host'][2]], int(res['host'][4]), int(res['host'][5])]
    out['device_result'] = [float(res['device'][0]), [int(v) for v in res['device'][2]], int(res['device'][4]), int(res['device'][5])]
    out['encoder'] = encoder_times(preds[0])
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
