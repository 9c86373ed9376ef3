"""Shared body of the evaluation entry points tools/eval*.py (reference: tools/eval.py:40-127, eval_spatial.py, eval_response.py):
load the snapshot `<dataset_splitBy>/output_<postfix>/<prefix>_iter_<model_iter>.pth` into the variant's resnetv1 and run
model.test.eval_split on a split.  Without dataset files in this repository the SyntheticLoader stands in for the loader."""
import argparse
import os
import os.path as osp
import sys

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--dataset', default='refcoco'); p.add_argument('--splitBy', default='unc')
    p.add_argument('--split', default='val'); p.add_argument('--id', default='mrcn_cmr_with_st')
    p.add_argument('--output_postfix', default='cycle'); p.add_argument('--model_iter', type=int, default=0)
    p.add_argument('--num_sents', type=int, default=-1); p.add_argument('--verbose', type=int, default=1)
    p.add_argument('--cfg', dest='cfg_file', default='experiments/cfgs/res101.yml')
    p.add_argument('--set', dest='set_cfgs', default=None, nargs=argparse.REMAINDER)
    p.add_argument('--synthetic_images', type=int, default=8); p.add_argument('--dtype', default='bf16')
    p.add_argument('--results_dir', default=None, help='where det_results.txt / mask_results.txt are appended (default: experiments/)')
    p.add_argument('--synthetic', type=int, default=0, help='1: evaluate on the SyntheticLoader when the dataset files are absent')
    p.add_argument('--allow_init_weights', type=int, default=0, help='1: evaluate the initial weights when the snapshot is missing (otherwise an error)')
    p.add_argument('--device_eval', type=int, default=0, help='1: model/eval_device.py (one backbone pass per image, metrics on the GPU, '
                   'sharded over RANK / WORLD_SIZE); 0: the host loop model/test.py')
    p.add_argument('--dump_predictions', default=None, help='with --device_eval 1: write every sentence\'s prediction (class, box, score, hit, '
                   'I, U, COCO RLE mask) as one JSON list to this path (rank r of WORLD_SIZE > 1 writes PATH.rank<r>)')
    p.add_argument('--dump_detections', default=None, help='with --device_eval 1: write every detection of every sentence (class-wise NMS with '
                   'cfg.TEST.NMS, --max_per_image, --det_thresh; box, score, area, COCO RLE mask) as one JSON list to this path (rank suffix as above)')
    p.add_argument('--max_per_image', type=int, default=100, help='--dump_detections: detections kept per sentence over all classes (<= 0: all)')
    p.add_argument('--det_thresh', type=float, default=0.0, help='--dump_detections: a detection needs a score above this')
    p.add_argument('--describe', type=int, default=0, help='--dump_detections on the cycle network: also what the captioner says about every '
                   'detection (caption_tokens, caption_logprobs, caption; greedy)')
    p.add_argument('--beam_size', type=int, default=1, help='--describe 1: beam search with this many beams instead of greedy decoding; every '
                   'detection also gets caption_beams, best first')
    p.add_argument('--expr_score', type=int, default=0, help='--dump_detections on the cycle network: also the log-likelihood of the sentence '
                   'under every detection\'s mask (expr_logprob, expr_logprobs)')
    p.add_argument('--judge_detections', type=int, default=0, help='--dump_detections on a network with masks: also judge every detection against '
                   'the sentence\'s ground truth on the device (I, U, hit per detection) and print what the rules detector / oracle would score')
    p.add_argument('--rerank', default=None, help='--dump_detections --expr_score 1: lambdas L1,L2,... (at most 8); per lambda the rule that picks '
                   'the detection with the best log(score) + lambda * expr_logprob, and the rule speaker (best expr_logprob); implies '
                   '--judge_detections 1')
    p.add_argument('--rerank_per_token', type=int, default=0, help='--rerank: divide expr_logprob by the expression\'s tokens + 1')
    p.add_argument('--dump_selection', default=None, help='with judging: write every sentence\'s choice per rule as one JSON list to this path '
                   '(rank suffix as above)')
    p.add_argument('--caption_eval', type=int, default=0, help='with --device_eval 1 on cycle / cycle_response: evaluate the captioner too - every '
                   'sentence\'s own expression (cut to seq_length tokens) scored teacher-forced under its ground-truth mask; prints loss, '
                   'perplexity and loss_per_image, and --dump_predictions gains gt_expr_logprob / gt_expr_logprobs')
    p.add_argument('--caption_eval_describe', type=int, default=0, help='--caption_eval 1: also the captioner\'s own sentence for every ground-truth '
                   'mask (greedy, or the best of --beam_size beams) and the exact-match rate against the expression')
    p.add_argument('--start_from', default=None, help='warm-start the captioner from <dataset_splitBy>/<start_from>/model-best.pth, as training '
                   'does; --caption_eval prints its infos-best.pkl best_val_score beside the loss')
    # the expression encoder the snapshot was trained with (tools/opt.py; a snapshot of another encoder is an error that names the flag)
    # (default None: tools/opt.py's own defaults apply)
    p.add_argument('--rnn_type', default=None, help='lstm, gru or rnn'); p.add_argument('--rnn_num_layers', type=int, default=None)
    p.add_argument('--bidirectional', type=int, default=None)
    return vars(p.parse_args(argv))


def dump_predictions(args, preds, rank, world, key='dump_predictions', what='predictions'):
    """--dump_predictions / --dump_detections: this rank's list as one JSON list"""
    if preds is None:
        return
    import json
    path = args[key] + ('.rank%d' % rank if world > 1 else '')
    with open(path, 'w') as f:
        json.dump(preds, f)
    print('wrote %d %s to %s' % (len(preds), what, path))


def parse_rerank(text):
    """--rerank L1,L2,... -> the list of floats (None without the flag).  ValueError naming --rerank on an entry that is no finite float
    and on more than 8 entries"""
    if text is None or text == '':
        return None
    out = []
    for part in str(text).split(','):
        try:
            out.append(float(part))
        except ValueError:
            raise ValueError('--rerank: every entry of L1,L2,... is a finite float, got %r' % part)
    from lang2seg_amd.model.detect_device import check_rerank
    return check_rerank(out)


def selection_options(args, variant):
    """the judging flags -> (judge, the lambdas or None, per_token).  ValueErrors name the flags involved"""
    lambdas = parse_rerank(args.get('rerank'))
    judge = bool(args.get('judge_detections')) or bool(lambdas)
    flags = [f for f, v in (('--judge_detections', args.get('judge_detections')), ('--rerank', lambdas),
                            ('--rerank_per_token', args.get('rerank_per_token')), ('--dump_selection', args.get('dump_selection'))) if v]
    if flags and not args.get('dump_detections'):
        raise ValueError('%s judge the detections: they need --dump_detections PATH' % ', '.join(flags))
    if lambdas and not args.get('expr_score'):
        raise ValueError('--rerank weighs the expression\'s log-likelihood under every detection\'s mask: it needs --expr_score 1')
    if args.get('rerank_per_token') and not lambdas:
        raise ValueError('--rerank_per_token divides the re-ranking term: it needs --rerank L1,L2,...')
    if args.get('dump_selection') and not judge:
        raise ValueError('--dump_selection writes the judged choices: it needs --judge_detections 1 or --rerank L1,L2,...')
    if flags and variant == 'vgg':
        raise ValueError('%s compare masks: --variant vgg has no mask branch' % ', '.join(flags))
    return judge, lambdas, bool(args.get('rerank_per_token'))


def caption_eval_options(args, variant):
    """the speaker's flags -> (caption_eval, describe, the beams of its descriptions).  ValueErrors name the flags involved"""
    on, desc = bool(args.get('caption_eval')), bool(args.get('caption_eval_describe'))
    if desc and not on:
        raise ValueError('--caption_eval_describe 1 describes the ground-truth masks of the captioner\'s evaluation: it needs --caption_eval 1')
    if on and not args.get('device_eval'):
        raise ValueError('--caption_eval 1 runs inside the device evaluation: it needs --device_eval 1')
    if on and variant not in ('cycle', 'cycle_response'):
        raise ValueError('--caption_eval 1: --variant %s has no caption branch to evaluate (cycle and cycle_response have one)' % variant)
    return on, desc, (args.get('beam_size', 1) if desc else 1)


def print_caption_eval(t, infos=None):
    """the speaker's line behind the usual summary; infos: the warm-start checkpoint's infos-best.pkl (context, not a check)"""
    if not t or t.get('loss') is None:
        print('Captioner: no sentence scored')
        return
    line = 'Captioner on the ground-truth masks (%d sents, %d tokens): loss %.4f, perplexity %.2f, loss_per_image %.4f' % (
        t['num_sent'], t['num_tok'], t['loss'], t['perplexity'], t['loss_per_image'])
    if t.get('exact_match') is not None:
        line += ', exact match %.2f%%' % (t['exact_match'] * 100.0)
    print(line)
    if infos is not None and infos.get('best_val_score') is not None:
        print('  -loss %.4f here; the checkpoint\'s own best_val_score %.4f (--start_from: its own features and its own validation split)' % (
            -t['loss'], float(infos['best_val_score'])))


def print_selection(totals):
    """one line per rule: det acc, seg acc at 0.5 and overall IoU of the detection that rule picks"""
    for name, t in totals.items():
        n = max(t['num_sent'], 1)
        print('rule %-14s det acc %.2f%%, seg acc@0.5 %.2f%%, overall IoU %.2f%% (%d sents)' % (
            name, t['acc'] * 100.0 / n, t['seg_correct'][0] * 100.0 / n, t['cum_I'] * 100.0 / max(t['cum_U'], 1), t['num_sent']))


def main(args, variant):
    from lang2seg_amd.model.config import cfg, cfg_from_file, cfg_from_list
    from lang2seg_amd.model.test import eval_split, summarize
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    sys.path.insert(0, osp.join(ROOT, 'tools'))
    from opt import parse_opt
    rank = int(os.environ.get('RANK', 0)); world = int(os.environ.get('WORLD_SIZE', 1)); local = int(os.environ.get('LOCAL_RANK', 0))
    if world > 1 and not args['device_eval']:
        raise ValueError('WORLD_SIZE > 1 evaluates through --device_eval 1 only')
    if args.get('dump_predictions') and not args['device_eval']:
        raise ValueError('--dump_predictions needs --device_eval 1 (the host loop keeps no predictions)')
    if args.get('dump_detections') and not args['device_eval']:
        raise ValueError('--dump_detections needs --device_eval 1 (the host loop keeps one box per sentence)')
    for k in ('describe', 'expr_score'):
        if args.get(k) and not args.get('dump_detections'):
            raise ValueError('--%s 1 needs --dump_detections PATH: it adds fields to every detection (--%s, --dump_detections)' % (k, k))
    cap_eval, cap_desc, cap_beams = caption_eval_options(args, variant)
    if args.get('beam_size', 1) > 1 and not args.get('describe') and not cap_desc:
        raise ValueError('--beam_size %d without --describe 1: the beams are those of the captions of every detection (--beam_size, --describe)'
                         % args['beam_size'])
    if (args.get('describe') or args.get('expr_score')) and variant == 'vgg':
        raise ValueError('--describe / --expr_score: --variant vgg has no caption branch (the cycle network has one)')
    judge, lambdas, per_token = selection_options(args, variant)
    preds = [] if args.get('dump_predictions') else None
    dets = [] if args.get('dump_detections') else None
    torch.cuda.set_device(local % max(torch.cuda.device_count(), 1))
    T = 20 if args['dataset'] == 'refcocog' else 10
    V = 3349 if args['dataset'] == 'refcocog' else 1999
    data_json = osp.join(ROOT, 'cache/prepro', args['dataset'] + '_' + args['splitBy'], 'data.json')       # eval_cycle.py:45-48
    data_h5 = osp.join(ROOT, 'cache/prepro', args['dataset'] + '_' + args['splitBy'], 'data.h5')
    if osp.exists(data_json):
        from lang2seg_amd.loaders.cycle_loader import GtMRCNLoader
        loader = GtMRCNLoader(data_json, data_h5, image_root=osp.join(ROOT, 'pyutils/mask-faster-rcnn/data/coco/images/train2014'))
    elif args['synthetic']:
        loader = SyntheticLoader(num_images=args['synthetic_images'], sents_per_image=3, T=T, vocab_size=V)
    else:
        raise FileNotFoundError('%s not found (pass --synthetic 1 to run on the synthetic stand-in)' % data_json)
    opt = parse_opt([])
    opt.update(vocab_size=loader.vocab_size, C4_feat_dim=1024, seq_length=loader.label_length,
               dataset_splitBy=args['dataset'] + '_' + args['splitBy'])
    opt.update({k: args[k] for k in ('rnn_type', 'rnn_num_layers', 'bidirectional', 'start_from') if args.get(k) is not None})
    if args['cfg_file'] and osp.exists(osp.join(ROOT, args['cfg_file'])):
        cfg_from_file(osp.join(ROOT, args['cfg_file']))
    if args['set_cfgs']:
        cfg_from_list(args['set_cfgs'])
    cfg.COMPUTE_DTYPE = args['dtype']
    if world > 1:
        torch.distributed.init_process_group(cfg.TRAIN.DP_BACKEND)
    if variant == 'vgg':
        from lang2seg_amd.nets.vgg16 import vgg16
        opt['C4_feat_dim'] = 512
        net = vgg16(opt, batch_size=1)
    else:
        net = resnetv1(opt, batch_size=1, num_layers=101, variant=variant)
    net.create_architecture(81, tag='default', anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
    ckpt = osp.join(ROOT, opt['dataset_splitBy'], 'output_{}'.format(args['output_postfix']),
                    cfg.TRAIN.SNAPSHOT_PREFIX + '_iter_{:d}.pth'.format(args['model_iter']))
    if osp.exists(ckpt):
        net.load_state_dict(torch.load(ckpt, map_location='cpu'))
        print('loaded', ckpt)
    elif args['allow_init_weights']:
        print('no snapshot at %s: evaluating the initial weights (--allow_init_weights 1)' % ckpt)
    else:
        raise FileNotFoundError('no snapshot at %s (eval.py:66 torch.load would fail; --allow_init_weights 1 evaluates the initialisers)' % ckpt)
    split = args['split'] if args['split'] in loader.split_ix else 'val'
    if variant == 'vgg':                                     # tools/eval_vgg.py: boxes only (model/test_vgg.py)
        from lang2seg_amd.model.test_vgg import eval_split as eval_split_vgg
        eopt = dict(num_sents=args['num_sents'], verbose=bool(args['verbose']), max_per_image=args.get('max_per_image', 100),
                    det_thresh=args.get('det_thresh', 0.0))
        if args['device_eval']:
            from lang2seg_amd.model.eval_device import eval_split_vgg_device
            acc, n = eval_split_vgg_device(loader, net, None, split, eopt, rank=rank, world=world, predictions=preds, detections=dets)
            dump_predictions(args, preds, rank, world)
            dump_predictions(args, dets, rank, world, 'dump_detections', 'detections')
        else:
            acc, n = eval_split_vgg(loader, net, None, split, eopt)
        if rank != 0:
            return acc, None, None
        print('Comprehension on %s\'s %s (%s sents): box acc %.2f%%' % (opt['dataset_splitBy'], args['split'], n, acc * 100))
        return acc, None, None
    opt['split'], opt['id'] = args['split'], args['id']
    eopt = dict(num_sents=args['num_sents'], verbose=bool(args['verbose']), max_per_image=args.get('max_per_image', 100),
                det_thresh=args.get('det_thresh', 0.0))
    if args['device_eval']:
        from lang2seg_amd.model.eval_device import eval_split_device
        sel, sel_tot = ([], {}) if judge else (None, None)
        kw = dict(judge=True, rerank=lambdas, per_token=per_token, selection=sel, selection_totals=sel_tot) if judge else {}
        cap_tot = {} if cap_eval else None
        if cap_eval:
            kw.update(caption_eval=True, caption_describe=cap_desc, caption_totals=cap_tot)
            if cap_desc and not hasattr(loader, 'ix_to_word'):       # the synthetic stand-in has no words: w<id>, as tools/predict.py names them
                eopt['ix_to_word'] = {str(i): 'w%d' % i for i in range(1, loader.vocab_size + 1)}
        res = eval_split_device(loader, net, None, split, eopt, rank=rank, world=world, predictions=preds, detections=dets,
                                describe=bool(args.get('describe')), expr_score=bool(args.get('expr_score')),
                                beam_size=args.get('beam_size', 1) if (args.get('describe') or cap_desc) else 1, **kw)
        dump_predictions(args, preds, rank, world)
        dump_predictions(args, dets, rank, world, 'dump_detections', 'detections')
        if args.get('dump_selection'):
            dump_predictions(args, sel, rank, world, 'dump_selection', 'selections')
    else:
        res = eval_split(loader, net, None, split, eopt)
    acc, eval_seg_iou_list, seg_correct, seg_total, cum_I, cum_U, num_sent = res
    if rank != 0:                                            # the totals are the same on every rank; rank 0 prints and writes the logs
        return acc, None, None
    print('Comprehension on %s\'s %s (%s sents) is %.2f%%' % (opt['dataset_splitBy'], split, num_sent, acc * 100.))
    results_str, prec, iou = summarize(eval_seg_iou_list, seg_correct, seg_total, cum_I, cum_U)
    print('Segmentation results on [%s][%s]' % (opt['dataset_splitBy'], split))
    print(results_str)
    if args['device_eval'] and judge:
        print_selection(sel_tot)
    if args['device_eval'] and cap_eval:
        infos = None
        if opt.get('start_from') is not None:
            from lang2seg_amd.utils.caption_ckpt import read_infos, start_dir
            f = osp.join(start_dir(opt, opt.get('checkpoint_root', '.')), 'infos-best.pkl')
            infos = read_infos(f) if osp.isfile(f) else None
        print_caption_eval(cap_tot, infos)
    # tools/eval_spatial.py:95-98,121-124: the two running result logs
    res_dir = args.get('results_dir') or osp.join(ROOT, 'experiments')
    os.makedirs(res_dir, exist_ok=True)
    with open(osp.join(res_dir, 'det_results.txt'), 'a') as f:
        f.write('[%s][%s], id[%s]\'s acc is %.2f%%\n' % (opt['dataset_splitBy'], opt['split'], opt['id'], acc * 100.0))
    with open(osp.join(res_dir, 'mask_results.txt'), 'a') as f:
        f.write('[%s][%s]\'s iou is:\n%s' % (opt['dataset_splitBy'], split, results_str))
    return acc, iou, prec
