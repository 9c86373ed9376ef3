"""Caption decoding (AttModel.sample / sample_beam, CaptionModel.beam_search) as one queue of launches: Network.caption_decode.

The captioner's head once, then T = seq_length tokens, each [word embedding of the device token slot -> one recurrent step of the selected
captioner, by the token function its training forward calls (nets/captioners.py) -> the logit Linear -> the decision kernel
(csrc/decode.hip)].  All T tokens are enqueued unconditionally: the decision kernels keep a finished flag (greedy / sampled) or the -1000
sums and the list of completed beams (beam search) on the device, and the host reads the result back once per call.

Beam rows go through the per-token entries row by row and through the row-batch Linears with M = beam_size.  The state of every captioner
lives in two sets of [beam_size][rnn_size] arrays: a step reads `cur` and writes `new`, the beam kernel gathers `new` back into `cur` by
parent.  Greedy and sampled decoding are the same loop with one row whose two sets swap roles every token.

One deliberate deviation from the reference as it runs under a current torch, see DESIGN.md 4.4f: completed beams are ordered by their joint
log-probability (the rule the reference was written for), not by completion order."""
import numpy as np
import torch

from .. import ops as O

f32 = torch.float32
L = 196
SAMPLE_SALT = 1000003 * sum(map(ord, 'sample'))


def check_args(net, sample_max, beam_size, temperature):
    """ValueErrors that name the flag (tools/predict.py passes its flags straight through)"""
    if getattr(net, 'var', None) is None or net.var.get('cap') is None or getattr(net, 'cap_model', None) is None:
        raise ValueError('--variant %s has no caption branch: nothing to decode (cycle and cycle_response have one)' % getattr(net, 'variant', '?'))
    if isinstance(beam_size, bool) or not isinstance(beam_size, (int, np.integer)) or not 1 <= beam_size <= O.BEAM_MAX:
        raise ValueError('--beam_size %r: an integer, 1 .. %d' % (beam_size, O.BEAM_MAX))
    if beam_size > net.opt['vocab_size'] + 1:
        raise ValueError('--beam_size %r: more beams than the %d words' % (beam_size, net.opt['vocab_size'] + 1))
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float, np.integer, np.floating)) or not float(temperature) > 0.0:
        raise ValueError('--temperature %r: a positive number' % (temperature,))
    if sample_max not in (0, 1, False, True):
        raise ValueError('--sample_max %r: 0 or 1' % (sample_max,))
    if beam_size > 1 and net.opt['seq_length'] > O.BEAM_MAX_T:
        raise ValueError('--beam_size %r with seq_length %d: beam search keeps at most %d tokens' % (beam_size, net.opt['seq_length'], O.BEAM_MAX_T))


def _fc_checked(net, fc_feats):
    """fc_feats as the flat vector fc_embed reads"""
    FC = net.opt['fc_feat_size']
    if fc_feats is None:
        raise ValueError('caption_decode: --caption_model %s reads fc_feats' % net.cap_model)
    fc = fc_feats.reshape(-1)
    if fc.numel() != FC:
        raise ValueError('caption_decode: fc_feats has %d values, fc_feat_size is %d' % (fc.numel(), FC))
    return fc if fc.dtype != f32 else fc.contiguous()


def step(net, H, cur, new, tokens, B):
    """one recurrent step of the network's captioner on B rows: the word embedding of tokens int64 [B] (device) -> the captioner's token
    function on the state rows cur[name][b] -> new[name][b] (nets/captioners.py decode_step) -> the logits f32 [B][V1]"""
    cap = net.captioner
    R, IE, V1 = net.opt['rnn_size'], net.opt['input_encoding_size'], net.opt['vocab_size'] + 1
    xt, x = net.buf('dec.xt', (B, IE), f32), net.buf('dec.' + cap.x_name, (B, cap.in_width()), f32)
    O.embed_fwd(cap.pv('embed.0.weight'), tokens, None, xt, B, IE, True)
    cap.token_inputs(xt, x, B)
    out = cap.decode_step(H, cur, new, x, B)
    logits = net.buf('dec.logits', (B, V1), f32)
    O.linear_fwd(out, cap.pv('logit.weight'), cap.pv('logit.bias'), logits, B, V1, R)
    return logits


def _head(net, att_feats):
    """att_embed (Linear + ReLU) + ctx2att, Captioner.head without the dropout, into buffers of decoding's own ('dec.'): a caption decoded
    between a training forward and its backward leaves what that backward reads (net.t, cap.*) alone"""
    AF = net.opt['att_feat_size']
    if att_feats.numel() != L * AF:
        raise ValueError('caption_decode: att_feats has %d values, expected 196 x att_feat_size = %d' % (att_feats.numel(), L * AF))
    want = O.TORCH_DT[net.dt]
    if att_feats.dtype != want:
        raise ValueError('caption_decode: att_feats is %s, the network computes in %s' % (att_feats.dtype, want))
    return net.captioner.head(att_feats.contiguous(), net.captioner.db)[1:]


def caption_decode(net, att_feats, fc_feats=None, sample_max=1, beam_size=1, temperature=1.0):
    """-> {'seq': [ints], 'logprobs': [floats]} (+ 'beams': [{'seq', 'logps', 'p', 'index'}] for beam_size > 1, best first).
    att_feats [196][att_feat_size] in the network's activation dtype, fc_feats [fc_feat_size] for the captioners that read it.
    beam_size > 1 is beam search whatever sample_max says (AttModel.sample :155-156); sample_max and temperature matter for beam_size 1.
    Every buffer is decoding's own ('dec.*'); the call reads the parameters and leaves a train step's activations untouched."""
    check_args(net, sample_max, beam_size, temperature)
    if net.training:
        raise RuntimeError('caption_decode runs in eval mode (net.eval()): the dropouts are off')
    net.join_update()
    net.join_transposes()
    T, V1, B = int(net.opt['seq_length']), net.opt['vocab_size'] + 1, int(beam_size)
    ad, patt = _head(net, att_feats)
    cap = net.captioner
    H = cap.decode_start(ad, patt, _fc_checked(net, fc_feats) if cap.reads_fc else None)
    ib = lambda n, shp, dt: net.buf('dec.' + n, shp, dt)
    tokens = ib('tokens', (B,), torch.int64)
    O.memset_zero(tokens)                                       # <bos>
    cur, new = cap.new_states('a', B), cap.new_states('b', B)
    if B == 1:
        out, fin = ib('out', (12 * T,), torch.uint8), ib('finished', (1,), torch.int32)    # seq | log-probabilities: one buffer, one copy back
        seq, lps = out[:8 * T].view(torch.int64), out[8 * T:].view(f32)
        u = None
        if not sample_max:
            u = (net.parity or {}).get('sample')                 # injected draws (parity runs); None: the device RNG
            if u is None:
                O.counter_inc(net.seed_counter())               # a fresh draw for every call
            elif u.numel() < T or u.dtype != f32:
                raise ValueError("parity['sample'] must hold seq_length = %d float32 values" % T)
        for t in range(T):
            logits = step(net, H, cur, new, tokens, B)
            O.decode_pick(logits, V1, t, bool(sample_max), temperature, u, net.seed_counter(), SAMPLE_SALT + getattr(net, 'rank_seed', 0),
                          fin, seq, lps, tokens)
            cur, new = new, cur
        host = out.cpu()                                        # the one read-back
        s, lp = host[:8 * T].view(torch.int64).numpy(), host[8 * T:].view(f32).numpy()
        n = int(np.argmax(s == 0)) if (s == 0).any() else T
        return {'seq': [int(v) for v in s[:n]], 'logprobs': [float(v) for v in lp[:n]]}
    RW = O.beam_record_words(T)
    bseq, blp, bsum = ib('beam_seq', (T, B), torch.int32), ib('beam_seq_logprobs', (T, B), f32), ib('beam_logprobs_sum', (B,), f32)
    parents, rec_dev = ib('parents', (B,), torch.int32), ib('done', (1 + B * T * RW,), torch.int32)          # counter | records: one copy back
    cnt, done = rec_dev[:1], rec_dev[1:]
    names = cap.states
    for t in range(T):
        logits = step(net, H, cur, new, tokens, B)
        O.decode_beam_step(logits, V1, B, t, T, bseq, blp, bsum, [(new[k][0], cur[k][0], new[k][1], cur[k][1]) for k in names], net.opt['rnn_size'],
                           tokens, parents, done, cnt)
    rec = rec_dev.cpu().numpy()                                 # the one read-back
    rec = rec[1:].reshape(B * T, RW)[:int(rec[0])]
    beams = [{'seq': [int(v) for v in r[:T]], 'logps': [float(v) for v in r[T:2 * T].view(np.float32)], 'p': float(r[2 * T:2 * T + 1].view(np.float32)[0]),
              'index': int(r[2 * T + 1])} for r in rec]
    beams = sorted(beams, key=lambda b: -b['p'])[:B]            # stable: completion order among equals (CaptionModel.py:123)
    best = beams[0]
    n = best['seq'].index(0) if 0 in best['seq'] else T
    return {'seq': best['seq'][:n], 'logprobs': best['logps'][:n], 'beams': beams}
