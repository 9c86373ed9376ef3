#!/usr/bin/env python
"""What the speaker's evaluation costs, on the full-size ResNet-101 'cycle' network of tools/describe_bench.py (initial weights, bf16, a
600 x 1000 SyntheticLoader image, canvases 375 x 625, --caption_model att2in2 and topdown at the production widths).

`pairs`: Network.caption_score_pairs on rows = 1, 8 and 64 sentences of 10 tokens (T = 11 scored positions), each row its own expression
under its own mask, against the same sentences scored one Network.caption_score_rows call at a time (one row per call: the only way to
score different sentences before caption_score_pairs).  The features (caption_features_rows, once) are outside both timings.  Device
time by HIP events; the two paths alternate inside one process, `--reps` rounds, the median reported.

`eval`: sentences per second of eval_split_device on tools/eval_bench.py's synthetic split (8 images at 600 x {800, 900, 1000}, 7
sentences each) with caption_eval off, on, and on with descriptions; the legs alternate, `--rounds` rounds, the median round reported.
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

from describe_bench import _once_us
from eval_bench import _Split

T_TOK, V = 10, 1999


def _network(model, dtype, variant='cycle'):
    from lang2seg_amd.model.config import cfg, cfg_from_file
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    from opt import parse_opt
    opt = parse_opt([])
    opt.update(vocab_size=V, C4_feat_dim=1024, seq_length=T_TOK, caption_model=model)
    if osp.exists(osp.join(ROOT, 'experiments/cfgs/res101.yml')):
        cfg_from_file(osp.join(ROOT, 'experiments/cfgs/res101.yml'))
    cfg.COMPUTE_DTYPE = dtype
    net = resnetv1(opt, batch_size=1, num_layers=101, variant=variant)
    net.create_architecture(81, tag='default', anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    net.eval()
    return net


def pairs_us(net, reps, rows_list):
    """{'rows<n>': {'pairs_us', 'per_call_us', 'speedup'}} on one image's map and 64 masks"""
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    from lang2seg_amd.model import eval_device as ED
    b = SyntheticLoader(num_images=1, sents_per_image=1, H=600, W=1000, T=T_TOK, vocab_size=V, seed=1234)._image(0)
    img, lab_d, lens, _, _ = ED._upload_image(net, b, 1)
    im_info = np.asarray(b['im_info'], dtype=np.float32).reshape(-1)[:3]
    _, ih, iw = ED._geometry(im_info)
    d = dict(data=img, im_info=im_info, S=1, labels=lab_d[0, :lens[0]], T=lens[0])
    net.forward_test_image(d)
    net.forward_test_sentence(d)
    rs = np.random.RandomState(0)
    cap = max(rows_list)
    masks = np.zeros((cap, ih, iw), np.uint8)
    for k in range(cap):
        y0, x0 = rs.randint(0, ih - 40), rs.randint(0, iw - 40)
        masks[k, y0:y0 + rs.randint(30, ih - y0), x0:x0 + rs.randint(30, iw - x0)] = 1
    att, fc = net.caption_features_rows(torch.from_numpy(masks).cuda(), cap, (ih, iw))
    att, fc = att.clone(), None if fc is None else fc.clone()
    tok = rs.randint(1, V + 1, (cap, T_TOK)).astype(np.int64)
    out = {}
    for rows in rows_list:
        a, f, t = att[:rows], None if fc is None else fc[:rows], tok[:rows]

        def pairs():
            net.caption_score_pairs(a, f, t)

        def per_call():
            for r in range(rows):
                net.caption_score_rows(a[r:r + 1], None if f is None else f[r:r + 1], t[r], rows=1)
        paths = {'pairs': pairs, 'per_call': per_call}
        times = {k: [] for k in paths}
        for fn in paths.values():
            fn()                                                    # warm-up: the buffers of this shape
        for _ in range(reps):
            for k, fn in paths.items():                             # in turn: a drift of the clocks meets both alike
                times[k].append(_once_us(fn))
        m = {k + '_us': float(np.median(v)) for k, v in times.items()}
        m['speedup'] = m['per_call_us'] / m['pairs_us']
        out['rows%d' % rows] = m
    return out


def eval_sents_per_s(net, rounds, images, sents):
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    from lang2seg_amd.model import eval_device as ED
    blobs = []
    for j in range(images):
        W = (800, 900, 1000)[j % 3]
        b = SyntheticLoader(num_images=1, sents_per_image=sents, H=600, W=W, T=T_TOK, vocab_size=V, seed=1234 + 31 * j)._image(0)
        blobs.append({k: v for k, v in b.items() if k in ('data', 'im_info', 'gt_boxes', 'gt_masks', 'labels', 'file_name')})
    legs = {'off': {}, 'caption_eval': dict(caption_eval=True), 'caption_eval_describe': dict(caption_eval=True, caption_describe=True)}
    totals, times, res = {}, {k: [] for k in legs}, {}

    def run(k):
        kw = dict(legs[k])
        if kw:
            kw['caption_totals'] = totals[k] = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res[k] = ED.eval_split_device(_Split(blobs), net, None, 'val', dict(verbose=False), **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    for k in legs:
        run(k)
    for _ in range(rounds):
        for k in legs:
            times[k].append(run(k))
    n = images * sents
    out = dict(images=images, sents_per_image=sents, rounds=rounds)
    for k in legs:
        out[k + '_sents_per_s'] = n / float(np.median(times[k]))
        out[k + '_rounds_sents_per_s'] = [n / t for t in times[k]]
    out['same_metrics'] = all(np.array_equal(np.asarray(x), np.asarray(y)) for k in legs for x, y in zip(res['off'], res[k]))
    out['totals'] = totals['caption_eval_describe']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='bf16'); ap.add_argument('--reps', type=int, default=5); ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--rows', default='1,8,64'); ap.add_argument('--models', default='att2in2,topdown')
    ap.add_argument('--images', type=int, default=8); ap.add_argument('--sents', type=int, default=7)
    ap.add_argument('--eval', type=int, default=1, help='0: the pairs timings only')
    ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = dict(metric='caption_eval', dtype=a.dtype, tokens=T_TOK, scored_positions=T_TOK + 1, reps=a.reps, pairs={}, eval={})
    for model in a.models.split(','):
        net = _network(model, a.dtype)
        res['pairs'][model] = pairs_us(net, a.reps, [int(r) for r in a.rows.split(',')])
        if a.eval:
            res['eval'][model] = eval_sents_per_s(net, a.rounds, a.images, a.sents)
        del net
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
