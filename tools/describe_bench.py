#!/usr/bin/env python
"""Device time of describing and of scoring every detection of one sentence (nets/caption_rows.py) on the full-size ResNet-101 'cycle'
network (initial weights, bf16, a 600 x 1000 SyntheticLoader image, canvases 375 x 625, --caption_model att2in2 or topdown at the
production widths), for count = 1, 8 and 64 live rows of cap = 64 (and count = 1 of cap = 128: what the head GEMMs on unused rows cost),
by HIP events.  Three paths, timed in turn inside one process, `reps` rounds, the median reported:
    batched   caption_features_rows + caption_decode_rows / caption_score_rows, the batched route where the captioner has one, else the
              loop (count stays on the device on the batched route)
    loop      the same entry points with net.rows_batched = False: the single-mask launches row by row
    per_mask  what the tree offered before: per mask l2s_mask_resize_nearest + caption_features(mask) + caption_decode (one read-back each);
              it has no score, so it is the yardstick of both
Each timing includes the features.  --beam_size B > 1 times beam search instead (and no scoring): `beam_batched` and `beam_loop` are
caption_features_rows + caption_beam_rows by the two routes, `per_mask_beam` is what the tree offered before for the same job,
caption_decode(beam_size=B) mask by mask on the same masks (one read-back each).  --cells 1 adds `cells`: one nn.LSTMCell step of the top-down attention cell at
rnn_size = input_encoding_size = 512 on 1, 8 and 64 rows, as l2s_lstm_cell_rows, as the existing launches it stands for on rows (two
l2s_linear_fwd + l2s_lstm_cell_fwd per row) and as l2s_topdown_cell_fwd per row; per path the time of CELL_CALLS steps issued back to
back between two events, over CELL_CALLS (where a kernel is shorter than the host takes to issue it, that is the issue rate).
Prints one JSON line."""
import argparse
import json
import os.path as osp
import sys

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, osp.join(ROOT, 'tools'))

import numpy as np
import torch


def _once_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0


CELL_CALLS = 20


def cells_us(O, reps):
    """{'rows<n>': {path + '_us': the median time of one step}}"""
    R = IE = 512
    Ka, G = IE + 2 * R, 4 * R
    g = torch.Generator(device='cuda').manual_seed(5)
    rn = lambda *shp: torch.randn(*shp, generator=g, device='cuda')
    un = lambda *shp: (torch.rand(*shp, generator=g, device='cuda') * 2 - 1) / float(np.sqrt(R))      # (as nn.LSTMCell draws its weights)
    w_ih, w_hh = un(G, Ka), un(G, R)
    out = {}
    for rows in (1, 8, 64):
        pre, fcrow, hl, lin0, ca = rn(rows, G), rn(rows, G), rn(rows, R) * 0.5, rn(rows, 2 * R) * 0.5, rn(rows, R)
        ca1, lin1, h1, gates, act = (torch.empty(s, device='cuda') for s in ((rows, R), (rows, 2 * R), (rows, R), (rows, G), (G,)))
        ha0 = lin0.view(-1)[R:]

        def fused():
            O.lstm_cell_rows(pre, None, None, [(hl, R, w_ih, Ka, R), (ha0, 2 * R, w_hh, R, R)], ca, ca1, lin1.view(-1)[R:], rows, R, pre2=fcrow,
                             ld_h=2 * R)

        def composed():
            O.linear_fwd(hl, w_ih, None, gates, rows, G, R, ldw=Ka)
            O.linear_fwd(ha0, w_hh, None, gates, rows, G, R, accumulate=True, ldx=2 * R)
            for r in range(rows):
                O.lstm_cell_fwd(gates[r], ca[r], ca1[r], h1[r], act, R)

        def per_row():
            for r in range(rows):
                O.topdown_cell_fwd(pre[r], fcrow[r], None, [(hl[r], w_ih, Ka, R), (lin0[r][R:], w_hh, R, R)], ca[r], ca1[r], h1[r], act, R)

        paths = {'lstm_cell_rows': fused, 'linear2_plus_cell_per_row': composed, 'topdown_cell_fwd_per_row': per_row}
        times = {k: [] for k in paths}
        for fn in paths.values():
            fn()
        for _ in range(reps):
            for k, fn in paths.items():
                times[k].append(_once_us(lambda: [fn() for _ in range(CELL_CALLS)]) / CELL_CALLS)
        out['rows%d' % rows] = {k + '_us': float(np.median(v)) for k, v in times.items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='bf16'); ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--counts', default='1,8,64'); ap.add_argument('--out', default=None, help='also write the JSON result to this file')
    ap.add_argument('--caption_model', default='att2in2', choices=['att2in2', 'topdown'])
    ap.add_argument('--beam_size', type=int, default=1, help='> 1: time beam search on rows against caption_decode(beam_size=) mask by mask')
    ap.add_argument('--cells', type=int, default=0, help='1: also time one LSTMCell step on rows three ways (see above)')
    a = ap.parse_args()
    from lang2seg_amd import ops as O
    from lang2seg_amd.model.config import cfg, cfg_from_file
    from lang2seg_amd.model import eval_device as ED
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    from opt import parse_opt
    torch.cuda.set_device(0)
    T, V = 10, 1999
    b = SyntheticLoader(num_images=1, sents_per_image=1, H=600, W=1000, T=T, vocab_size=V, seed=1234)._image(0)
    opt = parse_opt([])
    opt.update(vocab_size=V, C4_feat_dim=1024, seq_length=T, caption_model=a.caption_model)
    if osp.exists(osp.join(ROOT, 'experiments/cfgs/res101.yml')):
        cfg_from_file(osp.join(ROOT, 'experiments/cfgs/res101.yml'))
    cfg.COMPUTE_DTYPE = a.dtype
    net = resnetv1(opt, batch_size=1, num_layers=101, variant='cycle')
    net.create_architecture(81, tag='default', anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    net.eval()
    img, lab_d, lens, _, _ = ED._upload_image(net, b, 1)
    im_info = np.asarray(b['im_info'], dtype=np.float32).reshape(-1)[:3]
    scale, ih, iw = ED._geometry(im_info)
    d = dict(data=img, im_info=im_info, S=1, labels=lab_d[0, :lens[0]], T=lens[0])
    net.forward_test_image(d)
    s = net.forward_test_sentence(d)
    H, W = (int(v) for v in img.shape[1:3])
    expr = [int(w) for w in np.asarray(b['labels'])[0] if w]
    # 128 canvases: boxes of different sizes and places, as pasted detections are
    rs = np.random.RandomState(0)
    masks = np.zeros((128, ih, iw), np.uint8)
    for k in range(128):
        y0, x0 = rs.randint(0, ih - 40), rs.randint(0, iw - 40)
        masks[k, y0:y0 + rs.randint(30, ih - y0), x0:x0 + rs.randint(30, iw - x0)] = 1
    masks = torch.from_numpy(masks).cuda()
    big = torch.empty((H, W), dtype=torch.uint8, device='cuda')
    res = dict(metric='describe_us_per_sentence', dtype=a.dtype, caption_model=net.cap_model, seq_length=T, expression_tokens=len(expr),
               canvas=[ih, iw], blob=[H, W], map=list(s['net_conv_hw']), reps=a.reps, rows={})
    if a.beam_size > 1:
        res['beam_size'] = a.beam_size

    def rows_path(cap, cnt, batched, score):
        net.rows_batched = batched
        att, fc = net.caption_features_rows(masks[:cap], cap, (ih, iw), count=cnt)
        if a.beam_size > 1:
            net.caption_beam_rows(att, fc, rows=cap, count=cnt, beam_size=a.beam_size)
        elif score:
            net.caption_score_rows(att, fc, expr, rows=cap, count=cnt)
        else:
            net.caption_decode_rows(att, fc, rows=cap, count=cnt)
        net.rows_batched = True

    def per_mask(n):
        for k in range(n):
            O.mask_resize_nearest(masks[k], ih, iw, big, H, W)
            att, fc = net.caption_features(big)
            net.caption_decode(att, fc, beam_size=a.beam_size)

    cases = [(64, int(c)) for c in a.counts.split(',')] + [(128, 1)]
    for cap, n in cases:
        cnt = torch.tensor([n], dtype=torch.int32, device='cuda')
        paths = {'describe_batched': lambda: rows_path(cap, cnt, True, False), 'describe_loop': lambda: rows_path(cap, cnt, False, False),
                 'score_batched': lambda: rows_path(cap, cnt, True, True), 'score_loop': lambda: rows_path(cap, cnt, False, True),
                 'per_mask': lambda: per_mask(n)}
        if a.beam_size > 1:
            paths = {'beam_batched': paths['describe_batched'], 'beam_loop': paths['describe_loop'], 'per_mask_beam': paths['per_mask']}
        if cap == 128:
            paths = {k: v for k, v in paths.items() if k.endswith('batched')}
        times = {k: [] for k in paths}
        for k, fn in paths.items():
            fn()                                                    # warm-up: the buffers of this shape
        for _ in range(a.reps):
            for k, fn in paths.items():                             # in turn: a drift of the clocks meets every path alike
                times[k].append(_once_us(fn))
        res['rows']['cap%d_count%d' % (cap, n)] = {k + '_us': float(np.median(v)) for k, v in times.items()}
    if a.cells:
        res['cells'] = dict(rnn_size=512, input_encoding_size=512, calls_per_timing=CELL_CALLS, rows=cells_us(O, a.reps))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
