#!/usr/bin/env python
"""The caption branch of the full-size cycle network under --caption_model att2in2 (per-token launches, resident launch), topdown,
adaatt and adaattmo.

Three measurements on one device, every one with device events and the paths alternating inside each round:
  1. the captioner alone, forward and backward (+ its deferred parameter gradients), on the main stream, S = 12 tokens, on the pooled
     features of a real step;
  2. the whole replayed train step of every captioner (eight pipelined steps per sample);
  3. from the device-clock stamps of the replayed step: when the main queue reaches the caption join and when the caption stream is done.

    python tools/caption_model_bench.py [--rounds 20] [--out profiles/<name>.txt] [--json profiles/<name>.json]

--decode measures caption decoding instead (Network.caption_decode, nets/decode.py): time per caption by device events at rnn_size 512,
vocab_size 1999, seq_length 10 for every captioner, greedy and beam 3, interleaved rounds after a warm-up, medians; and the launches per
caption, counted by recording one call on a launch tape.

    python tools/caption_model_bench.py --decode [--rounds 20] [--json profiles/r09_decode_bench.json]
"""
import sys, os, argparse, collections, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--tokens', type=int, default=11, help='words per caption: S = tokens + 1 captioner steps')
    ap.add_argument('--out', default='')
    ap.add_argument('--json', default='', help='the same numbers as one JSON object')
    ap.add_argument('--models', default='att2in2,topdown,adaatt,adaattmo')
    ap.add_argument('--decode', action='store_true', help='time caption decoding (greedy and beam 3) instead of the training branch')
    args = ap.parse_args()
    if args.decode:
        return decode_bench(args)
    from lang2seg_amd.model.config import cfg
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    from lang2seg_amd.optim import SGD
    from lang2seg_amd import ops as O
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    T, V = args.tokens, 3349
    cfg.COMPUTE_DTYPE = 'bf16'
    lines, res = [], {'tokens': None, 'rounds': args.rounds, 'captioner_alone_ms': {}, 'step_ms': {}, 'join_us': {}}

    def say(s):
        print(s, flush=True); lines.append(s)

    def make(model):
        opt = dict(vocab_size=V, word_embedding_size=512, word_vec_size=512, rnn_hidden_size=512, bidirectional=1, word_drop_out=0.5,
                   rnn_drop_out=0.2, rnn_num_layers=1, rnn_type='lstm', variable_lengths=1, C4_feat_dim=1024, cap_loss_weight=1.0,
                   caption_model=model, input_encoding_size=512, rnn_size=512, num_layers=1, drop_prob_lm=0.5, seq_length=T,
                   fc_feat_size=4096, att_feat_size=4096, att_hid_size=512, adaatt=1)
        np.random.seed(cfg.RNG_SEED)
        net = resnetv1(opt, batch_size=1, num_layers=101)
        net.create_architecture(81, tag='default', anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
        net.train()
        return net, SGD(net, cfg.TRAIN.LEARNING_RATE, cfg.TRAIN.MOMENTUM, cfg.TRAIN.WEIGHT_DECAY)
    blob = SyntheticLoader(num_images=1, sents_per_image=1, H=600, W=1000, T=T, vocab_size=V).getBatch('train')
    models = [m for m in args.models.split(',') if m]
    nets = collections.OrderedDict((m, make(m)) for m in models)
    # ---- 1. the captioner alone ----
    paths = [('att2in2 per-token', 'att2in2', False), ('att2in2 resident', 'att2in2', True), ('topdown', 'topdown', None),
             ('adaatt', 'adaatt', None), ('adaattmo', 'adaattmo', None)]
    paths = [p for p in paths if p[1] in nets]
    state = {}
    for m, (net, optim) in nets.items():
        for _ in range(2):
            net.train_step(blob, 0, optim)                      # a real step: pooled features, buffers, transposes
        torch.cuda.synchronize()
        dev = net.upload_blob(blob, 0)
        state[m] = (dev, net.t['att_feats'].clone(), net.t['fc_feats'].clone() if 'fc_feats' in net.t else None, torch.zeros(8, device='cuda'))
    S = res['tokens'] = int(state[models[0]][0]['S'])
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def run(name, m, resident):
        net = nets[m][0]
        dev, att, fc, loss = state[m]
        if resident is not None:
            net.cap_persistent = resident
        net._cap_pre = None
        net.t = {'fc_feats': fc}
        O.memset_zero(net.P.grad)
        e = [ev() for _ in range(4)]
        e[0].record(); net._caption_fwd(dev, att, loss); e[1].record()
        e[2].record(); net._caption_bwd(dev, att)
        for f in net._cap_deferred:
            f()
        net._cap_deferred = []
        net.join_wgrad()
        e[3].record()
        torch.cuda.synchronize()
        return e[0].elapsed_time(e[1]), e[2].elapsed_time(e[3])
    say('captioner alone, S = %d steps, bf16 network (the captioner itself is fp32), %d rounds, paths alternating; ms, median [min .. max]' % (S, args.rounds))
    for p in paths:
        run(*p); run(*p)                                        # warm every path's buffers
    tm = {p[0]: [] for p in paths}
    for _ in range(args.rounds):
        for p in paths:
            tm[p[0]].append(run(*p))
    per_token = {'att2in2 per-token': '3 + 3', 'att2in2 resident': 'one launch per direction for all tokens', 'topdown': '5 + 5',
                 'adaatt': '1 + 1 (the attention runs once for all tokens)', 'adaattmo': '1 + 1 (the attention runs once for all tokens)'}
    for p in paths:
        a = np.array(tm[p[0]])
        say('  %-18s forward %.3f [%.3f .. %.3f]  backward + parameter gradients %.3f [%.3f .. %.3f]   launches per token (forward + backward): %s' % (
            p[0], np.median(a[:, 0]), a[:, 0].min(), a[:, 0].max(), np.median(a[:, 1]), a[:, 1].min(), a[:, 1].max(), per_token[p[0]]))
        res['captioner_alone_ms'][p[0]] = dict(forward=float(np.median(a[:, 0])), backward=float(np.median(a[:, 1])), launches_per_token=per_token[p[0]])
    for net, _ in nets.values():
        O.memset_zero(net.P.grad)                               # the direct calls left gradients behind; the steps below start from zero
        net._cap_pre = None
    torch.cuda.synchronize()
    if 'att2in2' in nets:
        nets['att2in2'][0].cap_persistent = True
    # ---- 2. the whole replayed step ----
    for m, (net, optim) in nets.items():
        net.use_tape = True
        net.stamp_buf = torch.zeros(96, dtype=torch.int64, device='cuda'); net.stamp_names = []
        for _ in range(3):
            net.train_step(blob, 0, optim)
        torch.cuda.synchronize()
    st = {m: [] for m in nets}; stamps = {m: [] for m in nets}
    for _ in range(args.rounds):
        for m, (net, optim) in nets.items():
            a, b = ev(), ev()
            a.record()
            for _ in range(8):
                net.train_step_async(blob, 0, optim)
            b.record(); torch.cuda.synchronize()
            st[m].append(a.elapsed_time(b) / 8)
            stamps[m].append(net.stamp_buf[:len(net.stamp_names)].cpu().numpy().astype(np.int64))
    say('whole replayed step (launch tape, eight pipelined steps per sample, ~30 one-thread clock stamps on the tape), ms per step')
    for m in nets:
        a = np.array(st[m])
        say('  %-10s %.3f [%.3f .. %.3f]' % (m, np.median(a), a.min(), a.max()))
        res['step_ms'][m] = float(np.median(a))
    # ---- 3. the caption join ----
    say('caption join of the replayed step (device clock, us since the step\'s first launch, medians)')
    for m, (net, _) in nets.items():
        names = net.stamp_names
        a = np.stack(stamps[m])
        rel = np.median((a - a[:, names.index('step start'):names.index('step start') + 1]) * 0.01, 0)
        at = lambda n: rel[names.index(n)]
        cap_done = at('cap: pool bwd + layer4 on map dgrad')
        say('  %-10s captioner fwd done %.1f  captioner bwd done %.1f  caption stream done %.1f  main reaches the join %.1f  -> main waits %.1f' % (
            m, at('cap: captioner fwd'), at('cap: captioner bwd'), cap_done, at('main reaches the caption join'),
            max(0.0, cap_done - at('main reaches the caption join'))))
        res['join_us'][m] = dict(captioner_fwd_done=float(at('cap: captioner fwd')), captioner_bwd_done=float(at('cap: captioner bwd')),
                                 caption_stream_done=float(cap_done), main_reaches_join=float(at('main reaches the caption join')))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)


def decode_bench(args):
    from lang2seg_amd.model.config import cfg
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    from lang2seg_amd import ops as O
    T, V, R = 10, 1999, 512
    cfg.COMPUTE_DTYPE = 'bf16'
    models = [m for m in args.models.split(',') if m]
    modes = [('greedy', dict(beam_size=1)), ('beam 3', dict(beam_size=3))]
    nets = {}
    for m in models:
        opt = dict(vocab_size=V, word_embedding_size=512, word_vec_size=512, rnn_hidden_size=512, bidirectional=1, word_drop_out=0.5,
                   rnn_drop_out=0.2, rnn_num_layers=1, rnn_type='lstm', variable_lengths=1, C4_feat_dim=1024, cap_loss_weight=1.0,
                   caption_model=m, input_encoding_size=R, rnn_size=R, num_layers=1, drop_prob_lm=0.5, seq_length=T,
                   fc_feat_size=4096, att_feat_size=4096, att_hid_size=R, adaatt=1)
        np.random.seed(cfg.RNG_SEED)
        net = resnetv1(opt, batch_size=1, num_layers=101)
        net.create_architecture(81, tag='default', anchor_scales=cfg.ANCHOR_SCALES, anchor_ratios=cfg.ANCHOR_RATIOS)
        net.eval()
        nets[m] = net
    g = torch.Generator().manual_seed(1)
    att = torch.randn(196, 4096, generator=g).abs().to(torch.bfloat16).cuda()         # pooled ReLU outputs: non-negative
    fc = torch.randn(4096, generator=g).abs().to(torch.bfloat16).cuda()
    ev = lambda: torch.cuda.Event(enable_timing=True)
    res = dict(rnn_size=R, vocab_size=V, seq_length=T, rounds=args.rounds, dtype='bf16 network, fp32 captioner', ms_per_caption={}, launches_per_caption={},
               words={})
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    for m, net in nets.items():
        for name, kw in modes:
            for _ in range(3):                                     # warm-up: buffers, code objects
                r = net.caption_decode(att, fc, **kw)
            torch.cuda.synchronize()
            h = O.tape_begin([torch.cuda.current_stream()] + list(net.streams().values()))     # (the joins in front of the head touch the side streams)
            try:
                net.caption_decode(att, fc, **kw)
            finally:
                O.tape_end(h)
            res['launches_per_caption']['%s %s' % (m, name)] = O.tape_size(h)
            res['words']['%s %s' % (m, name)] = len(r['seq'])
            O.tape_destroy(h)
    tm = {'%s %s' % (m, name): [] for m in nets for name, _ in modes}
    for _ in range(args.rounds):
        for m, net in nets.items():
            for name, kw in modes:
                a, b = ev(), ev()
                a.record(); net.caption_decode(att, fc, **kw); b.record()
                torch.cuda.synchronize()
                tm['%s %s' % (m, name)].append(a.elapsed_time(b))
    say('caption decoding, rnn_size %d, vocab_size %d, seq_length %d, %d interleaved rounds; ms per caption (device events around the call, its one '
        'read-back included), median [min .. max]; launches per caption (tape ops: kernels, clears, the counter)' % (R, V, T, args.rounds))
    for k, v in tm.items():
        a = np.array(v)
        say('  %-18s %.3f [%.3f .. %.3f]   %d launches' % (k, np.median(a), a.min(), a.max(), res['launches_per_caption'][k]))
        res['ms_per_caption'][k] = float(np.median(a))
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    main()
