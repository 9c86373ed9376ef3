#!/usr/bin/env python
"""Sentences per second of the evaluation loop: the host loop model/test.py eval_split vs the device path model/eval_device.py, on the
same SyntheticLoader-style split shaped like RefCOCO (8 images at 600 x {800, 900, 1000}, 7 sentences each, T = 10, V = 1999), the
full-size ResNet-101 'cycle' network with its initial weights, bf16.  One warm-up pass per path, then one timed pass each.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=8); ap.add_argument('--sents', type=int, default=7)
    ap.add_argument('--dtype', default='bf16'); ap.add_argument('--variant', default='cycle')
    a = ap.parse_args()
    from lang2seg_amd.model.config import cfg, cfg_from_file
    from lang2seg_amd.model.test import eval_split
    from lang2seg_amd.model import eval_device as ED
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
    out = dict(metric='eval_sentences_per_s', images=a.images, sents_per_image=a.sents, dtype=a.dtype, variant=a.variant)
    res = {}
    for path in ('host', 'device'):
        for rep in range(2):                                   # warm-up, timed
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
                # the issue time: up to the read-back of the records (the first host wait of the path)
                ED._Totals.add = add
                try:
                    r = ED.eval_split_device(_Split(blobs), net, None, 'val', dict(verbose=False))
                finally:
                    ED._Totals.add = orig
                t_issue = tot[0]
            torch.cuda.synchronize()
            t1 = time.perf_counter()
        res[path] = r
        out[path + '_sents_per_s'] = n / (t1 - t0)
        out[path + '_total_s'] = t1 - t0
        out[path + '_issue_s'] = t_issue - t0
    out['speedup'] = out['device_sents_per_s'] / out['host_sents_per_s']
    out['same_metrics'] = all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(res['host'], res['device']))
    out['host_result'] = [float(res['host'][0]), [int(v) for v in res['host'][2]], int(res['host'][4]), int(res['host'][5])]
    out['device_result'] = [float(res['device'][0]), [int(v) for v in res['device'][2]], int(res['device'][4]), int(res['device'][5])]
    print(json.dumps(out))


if __name__ == '__main__':
    main()
