#!/usr/bin/env python
"""Predict the referred object of free sentences on one image, no ground truth needed (model/predict_device.py):
    python tools/predict.py --image FILE --sent "the man on the left" --sent "red umbrella" [--png DIR]
    python tools/predict.py --synthetic 1 --allow_init_weights 1                       (a SyntheticLoader image and its token ids)
Prints one JSON list: per sentence the class, the box, the score, the mask's area and its COCO run-length form.  --png DIR also writes
each mask as DIR/<image>_<sent_index>.png, decoded on the device from the run lengths (l2s_rle_to_mask): the round trip.
    --all_detections 1 [--max_per_image N] [--det_thresh T]: every instance the network finds for each sentence instead of its first
pick (model/detect_device.py: class-wise NMS with cfg.TEST.NMS, the best N over all classes); prints one list per sentence, --png writes
DIR/<image>_<sent_index>_<k>.png.  With it, --describe 1 adds what the captioner says about EVERY detection (caption_tokens,
caption_logprobs, caption; greedy, or with --beam_size B > 1 by beam search on all detections at once, which also lists every beam as
caption_beams, best first) and --expr_score 1 how well every detection's mask explains the sentence (expr_logprob: the
teacher-forced log-likelihood of the sentence under that mask, expr_logprobs: per token and the end token); both need --variant cycle
(nets/caption_rows.py) and either without --all_detections 1 is an error.
    --caption 1 [--beam_size B] [--sample_max 0|1] [--temperature t]: also what the captioner says about each predicted mask
(model/caption_device.py: the caption branch's features under the mask, decoded on the device: greedy by default, sampled with
--sample_max 0, beam search with --beam_size > 1); adds caption_tokens, caption_logprobs and caption to every sentence's dict.  The
captioner is the snapshot's: --caption_model (with --adaatt 1 for adaatt / adaattmo) and the size flags as the train tools take them.  With
--synthetic 1 the words print as w<id>.  --beam_size > 1 is beam search whatever --sample_max says, as in the reference; --caption 1 together
with --all_detections 1 is an error."""
import argparse
import json
import os
import os.path as osp
import sys

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, osp.join(ROOT, 'tools'))

import numpy as np
import torch


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--image', default=None); p.add_argument('--sent', action='append', default=[])
    p.add_argument('--synthetic', type=int, default=0); p.add_argument('--png', default=None)
    p.add_argument('--variant', default='cycle'); p.add_argument('--dataset', default='refcoco'); p.add_argument('--splitBy', default='unc')
    p.add_argument('--output_postfix', default='cycle'); p.add_argument('--model_iter', type=int, default=0)
    p.add_argument('--cfg', dest='cfg_file', default='experiments/cfgs/res101.yml'); p.add_argument('--dtype', default='bf16')
    p.add_argument('--allow_init_weights', type=int, default=0)
    p.add_argument('--all_detections', type=int, default=0); p.add_argument('--max_per_image', type=int, default=100)
    p.add_argument('--det_thresh', type=float, default=0.0)
    p.add_argument('--describe', type=int, default=0); p.add_argument('--expr_score', type=int, default=0)
    # the expression encoder the snapshot was trained with (tools/opt.py; a snapshot of another encoder is an error that names the flag)
    # (default None: tools/opt.py's own defaults apply)
    p.add_argument('--rnn_type', default=None, help='lstm, gru or rnn'); p.add_argument('--rnn_num_layers', type=int, default=None)
    p.add_argument('--bidirectional', type=int, default=None)
    # mask -> sentence; the captioner flags of tools/opt.py (default None: its own defaults)
    p.add_argument('--caption', type=int, default=0); p.add_argument('--beam_size', type=int, default=1)
    p.add_argument('--sample_max', type=int, default=1); p.add_argument('--temperature', type=float, default=1.0)
    p.add_argument('--caption_model', default=None); p.add_argument('--adaatt', type=int, default=None)
    for k in ('rnn_size', 'input_encoding_size', 'att_hid_size', 'fc_feat_size', 'att_feat_size'):
        p.add_argument('--' + k, type=int, default=None)
    return vars(p.parse_args(argv))


def write_png(pred, path):
    """the mask of one prediction, decoded from its run lengths on the device, as a black / white PNG"""
    from PIL import Image
    from lang2seg_amd import ops as O
    h, w = pred['segmentation']['size']
    cnts = O.rle_from_string(pred['segmentation']['counts'])
    c = torch.from_numpy(cnts.view(np.int32)).cuda()
    offs = torch.tensor([0, cnts.size], dtype=torch.int32, device='cuda')
    ws = torch.empty((O.rle_ws_words(cnts.size, h, w),), dtype=torch.int32, device='cuda')
    out = torch.empty((h, w), dtype=torch.uint8, device='cuda')
    O.rle_to_mask(c, offs, 1, cnts.size, h, w, ws, out)
    Image.fromarray(out.cpu().numpy() * 255).save(path)


def main(args):
    if args.get('all_detections') and args.get('caption'):
        raise ValueError('--caption 1 with --all_detections 1: a caption describes the one mask picked for a sentence, not each detection; give one of the two')
    for k in ('describe', 'expr_score'):
        if args.get(k) and not args.get('all_detections'):
            raise ValueError('--%s 1 without --all_detections 1: it adds fields to every detection; give --all_detections 1 with --%s 1' % (k, k))
    from lang2seg_amd import ops as O
    from lang2seg_amd.model.config import cfg, cfg_from_file
    from lang2seg_amd.model.predict_device import predict_image
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    from opt import parse_opt
    torch.cuda.set_device(0)
    if args['cfg_file'] and osp.exists(osp.join(ROOT, args['cfg_file'])):
        cfg_from_file(osp.join(ROOT, args['cfg_file']))
    cfg.COMPUTE_DTYPE = args['dtype']
    name = args['dataset'] + '_' + args['splitBy']
    if args['synthetic']:
        from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
        loader = SyntheticLoader(num_images=1, sents_per_image=3, T=10, vocab_size=1999)
        b = loader._image(0)
        data, labels = dict(data=b['data'], im_info=b['im_info'], file_name=b['file_name']), b['labels']
    else:
        if not args['image'] or not args['sent']:
            raise SystemExit('--image FILE and at least one --sent "..." (or --synthetic 1)')
        from lang2seg_amd.loaders.loader import Loader
        from lang2seg_amd.loaders.cycle_loader import imread_bgr
        loader = Loader(osp.join(ROOT, 'cache/prepro', name, 'data.json'), verbose=False)        # the vocabulary
        labels = loader.encode_labels(args['sent'])
        img = imread_bgr(args['image'])
        sc, oh, ow = O.prep_geometry(img.shape[0], img.shape[1], cfg.TRAIN.SCALES[0], cfg.TRAIN.MAX_SIZE)    # the blob of the test loaders
        blob = torch.empty((1, oh, ow, 3), dtype=torch.float32, device='cuda')
        O.prep_image(torch.from_numpy(img).cuda(), cfg.PIXEL_MEANS.reshape(-1), sc, blob[0])
        data = dict(data=blob.cpu().numpy(), im_info=np.array([[oh, ow, sc]], np.float32), file_name=osp.basename(args['image']))
    opt = parse_opt([])
    opt.update(vocab_size=loader.vocab_size, C4_feat_dim=1024, seq_length=loader.label_length, dataset_splitBy=name)
    opt.update({k: args[k] for k in ('rnn_type', 'rnn_num_layers', 'bidirectional', 'caption_model', 'adaatt', 'rnn_size', 'input_encoding_size',
                                     'att_hid_size', 'fc_feat_size', 'att_feat_size') if args.get(k) is not None})
    if args['variant'] == 'vgg':
        from lang2seg_amd.nets.vgg16 import vgg16
        opt['C4_feat_dim'] = 512
        net = vgg16(opt, batch_size=1)
    else:
        net = resnetv1(opt, batch_size=1, num_layers=101, variant=args['variant'])
    net.create_architecture(81, tag='default', anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    ckpt = osp.join(ROOT, name, 'output_{}'.format(args['output_postfix']), cfg.TRAIN.SNAPSHOT_PREFIX + '_iter_{:d}.pth'.format(args['model_iter']))
    if osp.exists(ckpt):
        net.load_state_dict(torch.load(ckpt, map_location='cpu'))
    elif not args['allow_init_weights']:
        raise FileNotFoundError('no snapshot at %s (--allow_init_weights 1 predicts with the initialisers)' % ckpt)
    if args.get('all_detections'):
        from lang2seg_amd.model.detect_device import detect_image
        words = None
        if args.get('describe'):
            words = {str(i): 'w%d' % i for i in range(1, loader.vocab_size + 1)} if args['synthetic'] else loader.ix_to_word
        dets = detect_image(net, data, labels, max_per_image=args['max_per_image'], thresh=args['det_thresh'], describe=bool(args.get('describe')),
                            expr_score=bool(args.get('expr_score')), ix_to_word=words, beam_size=args['beam_size'] if args.get('describe') else 1)
        if args['png']:
            os.makedirs(args['png'], exist_ok=True)
            for lst in dets:
                for k, p in enumerate(lst):
                    if 'segmentation' in p:
                        write_png(p, osp.join(args['png'], '%s_%d_%d.png' % (osp.splitext(p['file_name'])[0], p['sent_index'], k)))
        print(json.dumps(dets))
        return dets
    if args.get('caption'):
        from lang2seg_amd.model.caption_device import caption_image
        if args['synthetic']:
            words = {str(i): 'w%d' % i for i in range(1, loader.vocab_size + 1)}
        else:
            words = loader.ix_to_word
        preds = caption_image(net, data, labels, sample_max=args['sample_max'], beam_size=args['beam_size'], temperature=args['temperature'],
                              ix_to_word=words)
    else:
        preds = predict_image(net, data, labels)
    if args['png']:
        os.makedirs(args['png'], exist_ok=True)
        for p in preds:
            if 'segmentation' in p:
                write_png(p, osp.join(args['png'], '%s_%d.png' % (osp.splitext(p['file_name'])[0], p['sent_index'])))
    print(json.dumps(preds))
    return preds


if __name__ == '__main__':
    main(parse_args())
