"""Caption decoding (AttModel.sample / sample_beam, CaptionModel.beam_search) as one queue of launches: Network.caption_decode.

The captioner's head once, then T = seq_length tokens, each [word embedding of the device token slot -> one recurrent step of the selected
captioner through the entry points its training forward uses -> the logit Linear -> the decision kernel (csrc/decode.hip)].  All T tokens
are enqueued unconditionally: the decision kernels keep a finished flag (greedy / sampled) or the -1000 sums and the list of completed beams
(beam search) on the device, and the host reads the result back once per call.

Beam rows go through the per-token entries row by row and through the row-batch Linears with M = beam_size.  The state of every captioner
lives in two sets of [beam_size][rnn_size] arrays: a step reads `cur` and writes `new`, the beam kernel gathers `new` back into `cur` by
parent.  Greedy and sampled decoding are the same loop with one row whose two sets swap roles every token.

One deliberate deviation from the reference as it runs under a current torch, see DESIGN.md 4.4f: completed beams are ordered by their joint
log-probability (the rule the reference was written for), not by completion order."""
import numpy as np
import torch

from .. import ops as O
from .params import ADAATT_GATES, FC_CAPTIONERS
from . import adaatt as AA

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


class _Stepper(object):
    """one recurrent step of the selected captioner on B rows: the head's per-sentence projections once, then step(cur, new, tokens), which
    reads the state rows cur[name][b], writes new[name][b] and returns the logits [B][V1]"""

    def __init__(self, net, B, ad, patt, fc_feats):
        self.net, self.B, self.ad, self.patt = net, B, ad, patt
        opt = net.opt
        self.R, self.IE, self.AH, self.V1 = opt['rnn_size'], opt['input_encoding_size'], opt['att_hid_size'], opt['vocab_size'] + 1
        self.pv = lambda k: net.P.view('caption_model.' + k)
        self.b = lambda n, shp, **kw: net.buf('dec.' + n, shp, f32, **kw)
        self.model = net.cap_model
        self.xt = self.b('xt', (B, self.IE))
        getattr(self, '_head_' + self._kind())(fc_feats)

    def _kind(self):
        return 'topdown' if self.model == 'topdown' else 'adaatt' if self.model in ADAATT_GATES else 'att2in2'

    def state_names(self):
        return {'att2in2': ('h', 'c'), 'topdown': ('hl', 'cl', 'ca', 'ha'), 'adaatt': ('h', 'c')}[self._kind()]

    def new_states(self, tag):
        """one set of state arrays (zeroed: the start state); (array, leading dimension) per name"""
        B, R = self.B, self.R
        if self._kind() == 'topdown':
            # h_att lives behind att_res in the language cell's input row [att_res | h_att], as in training
            lin = self.b('lin.' + tag, (B, 2 * R), zero=True)
            s = {k: (self.b('%s.%s' % (k, tag), (B, R), zero=True), R) for k in ('hl', 'cl', 'ca')}
            s['ha'] = (lin[:, R:], 2 * R)
            s['_lin'] = lin
            return s
        return {k: (self.b('%s.%s' % (k, tag), (B, R), zero=True), R) for k in ('h', 'c')}

    def _fc_embed(self, fc_feats):
        net, R, FC = self.net, self.R, self.net.opt['fc_feat_size']
        if fc_feats is None:
            raise ValueError('caption_decode: --caption_model %s reads fc_feats' % self.model)
        fc = fc_feats.reshape(-1)
        if fc.numel() != FC:
            raise ValueError('caption_decode: fc_feats has %d values, fc_feat_size is %d' % (fc.numel(), FC))
        if fc.dtype != f32:
            fc32 = self.b('fc32', (FC,)); O.cast(fc, fc32)
        else:
            fc32 = fc.contiguous()
        fce = self.b('fce', (R,))
        O.linear_fwd(fc32, self.pv('fc_embed.0.weight'), self.pv('fc_embed.0.bias'), fce, 1, R, FC, act=1)
        return fce

    # -------------------------------------------------------------- att2in2: the per-token path of _caption_fwd
    def _head_att2in2(self, fc_feats):
        net, R = self.net, self.R
        self.proj = net.cap_projected and R <= 1024
        if self.proj:
            self.Pm = self.b('P', (L, 2 * R))
            O.linear_fwd(self.ad, self.pv('core.a2c.weight'), None, self.Pm, L, 2 * R, R)

    def _step_att2in2(self, cur, new):
        B, R, AH, pv = self.B, self.R, self.AH, self.pv
        sums = self.b('sums', (B, 5 * R))
        O.linear_fwd(self.xt, pv('core.i2h.weight'), pv('core.i2h.bias'), sums, B, 5 * R, self.IE)
        att_h, tanh_ws, wgt, save = self.b('att_h', (B, AH)), self.b('tanh', (L, AH)), self.b('wgt', (L,)), self.b('save', (6 * R,))
        (h0, _), (c0, _), (h1, _), (c1, _) = cur['h'], cur['c'], new['h'], new['c']
        for r in range(B):
            O.linear2_fwd(h0[r], R, pv('core.attention.h2att.weight'), pv('core.attention.h2att.bias'), att_h[r], AH, False,
                          pv('core.h2h.weight'), pv('core.h2h.bias'), sums[r], 5 * R, True)
            if self.proj:
                dots = self.b('dots', (256,))
                O.cap_att_dots_fwd(self.patt, att_h[r], pv('core.attention.alpha_net.weight'), pv('core.attention.alpha_net.bias'), L, AH, tanh_ws, dots)
                O.cap_apply_gates_fwd(self.Pm, dots, pv('core.a2c.bias'), sums[r], c0[r], c1[r], h1[r], save, wgt, L, R)
            else:
                ares = self.b('ares', (R + 256,))
                O.cap_attention_fwd(self.patt, self.ad, att_h[r], pv('core.attention.alpha_net.weight'), pv('core.attention.alpha_net.bias'), L, AH,
                                    tanh_ws, wgt, ares)
                O.cap_a2c_gates_fwd(ares, pv('core.a2c.weight'), pv('core.a2c.bias'), R, sums[r], c0[r], c1[r], h1[r], save, R)
        return new['h'][0]

    # -------------------------------------------------------------- top-down: two cells and the attention per token
    def _head_topdown(self, fc_feats):
        R, pv = self.R, self.pv
        fce = self._fc_embed(fc_feats)
        self.Ka = self.IE + 2 * R
        self.fcrow = self.b('fcrow', (4 * R,))
        O.linear_fwd(fce, pv('core.att_lstm.weight_ih')[R:], pv('core.att_lstm.bias_hh'), self.fcrow, 1, 4 * R, R, ldw=self.Ka)

    def _step_topdown(self, cur, new):
        B, R, AH, Ka, pv = self.B, self.R, self.AH, self.Ka, self.pv
        xpre = self.b('xpre', (B, 4 * R))
        O.linear_fwd(self.xt, pv('core.att_lstm.weight_ih')[2 * R:], pv('core.att_lstm.bias_ih'), xpre, B, 4 * R, self.IE, ldw=Ka)
        wa_ih, wa_hh, wl_ih, wl_hh = pv('core.att_lstm.weight_ih'), pv('core.att_lstm.weight_hh'), pv('core.lang_lstm.weight_ih'), pv('core.lang_lstm.weight_hh')
        att_h, tanh_ws, wgt, dots = self.b('att_h', (B, AH)), self.b('tanh', (L, AH)), self.b('wgt', (L,)), self.b('dots', (256,))
        act = self.b('act', (4 * R,))
        lin0, lin1 = cur['_lin'], new['_lin']
        hl0, cl0, ca0, hl1, cl1, ca1 = cur['hl'][0], cur['cl'][0], cur['ca'][0], new['hl'][0], new['cl'][0], new['ca'][0]
        for r in range(B):
            h_att = lin1[r][R:]
            O.topdown_cell_fwd(xpre[r], self.fcrow, None, [(hl0[r], wa_ih, Ka, R), (lin0[r][R:], wa_hh, R, R)], ca0[r], ca1[r], h_att, act, R)
            O.linear_fwd(h_att, pv('core.attention.h2att.weight'), pv('core.attention.h2att.bias'), att_h[r], 1, AH, R)
            O.cap_att_dots_fwd(self.patt, att_h[r], pv('core.attention.alpha_net.weight'), pv('core.attention.alpha_net.bias'), L, AH, tanh_ws, dots)
            O.cap_att_apply_fwd(self.ad, dots, L, R, wgt, lin1[r])
            O.topdown_cell_fwd(None, pv('core.lang_lstm.bias_ih'), pv('core.lang_lstm.bias_hh'), [(lin1[r], wl_ih, 2 * R, 2 * R), (hl0[r], wl_hh, R, R)],
                               cl0[r], cl1[r], hl1[r], act, R)
        return hl1

    # -------------------------------------------------------------- adaptive attention: the cell per row, the attention on all rows at once
    def _head_adaatt(self, fc_feats):
        R, pv, G = self.R, self.pv, ADAATT_GATES[self.model]
        fce = self._fc_embed(fc_feats)
        self.G, self.W = G, (G + 1) * R
        self.fcrow = self.b('fcrow', (self.W,))
        O.linear_fwd(fce, pv('core.lstm.v2h.weight'), pv('core.lstm.v2h.bias'), self.fcrow, 1, G * R, R)
        O.linear_fwd(fce, pv('core.lstm.r_v2h.weight'), pv('core.lstm.r_v2h.bias'), self.fcrow[G * R:], 1, R, R)

    def _step_adaatt(self, cur, new):
        B, R, G, W, pv = self.B, self.R, self.G, self.W, self.pv
        xpre = self.b('xpre', (B, W))
        O.linear_fwd(self.xt, pv('core.lstm.w2h.weight'), pv('core.lstm.w2h.bias'), xpre, B, G * R, self.IE, ldy=W)
        O.linear_fwd(self.xt, pv('core.lstm.r_w2h.weight'), pv('core.lstm.r_w2h.bias'), xpre[:, G * R:], B, R, self.IE, ldy=W)
        Bf = {k: self.b('ada.' + k, shp) for k, shp in AA.fwd_shapes(B, L, R).items() if k not in ('hs', 'cs')}
        h0, c0, h1, c1 = cur['h'][0], cur['c'][0], new['h'][0], new['c'][0]
        cpv = lambda k: pv('core.' + k)
        for r in range(B):
            O.adaatt_cell_fwd(xpre[r], self.fcrow, cpv('lstm.h2h.0.weight'), cpv('lstm.h2h.0.bias'), cpv('lstm.r_h2h.weight'), cpv('lstm.r_h2h.bias'),
                              h0[r], c0[r], c1[r], h1[r], Bf['fake'][r], Bf['save'][r], R, G)
        AA.att_fwd(O, cpv, Bf, h1, self.ad, self.patt, {}, B, L, R)
        return Bf['outs']

    def step(self, cur, new, tokens):
        """tokens int64 [B] on the device -> logits f32 [B][V1]"""
        B, R, V1, pv = self.B, self.R, self.V1, self.pv
        O.embed_fwd(pv('embed.0.weight'), tokens, None, self.xt, B, self.IE, True)
        out = getattr(self, '_step_' + self._kind())(cur, new)
        logits = self.b('logits', (B, V1))
        O.linear_fwd(out, pv('logit.weight'), pv('logit.bias'), logits, B, V1, R)
        return logits


def _head(net, att_feats):
    """att_embed (Linear + ReLU) + ctx2att, the launches of _cap_head_fwd without its dropout, into buffers of decoding's own ('dec.'): a
    caption decoded between a training forward and its backward leaves what that backward reads (net.t, cap.*) alone"""
    R, AH = net.opt['rnn_size'], net.opt['att_hid_size']
    AF = net.opt['att_feat_size']
    if att_feats.numel() != L * AF:
        raise ValueError('caption_decode: att_feats has %d values, expected 196 x att_feat_size = %d' % (att_feats.numel(), L * AF))
    want = O.TORCH_DT[net.dt]
    if att_feats.dtype != want:
        raise ValueError('caption_decode: att_feats is %s, the network computes in %s' % (att_feats.dtype, want))
    ad = net.buf('dec.a', (L, R), f32)
    net.att_embed.fwd(att_feats.contiguous(), L, 1, 1, ad, relu=True, out_f32=True)
    patt = net.buf('dec.patt', (L, AH), f32)
    O.linear_fwd(ad, net.P.view('caption_model.ctx2att.weight'), net.P.view('caption_model.ctx2att.bias'), patt, L, AH, R)
    return ad, patt


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
    st = _Stepper(net, B, ad, patt, fc_feats if net.cap_model in FC_CAPTIONERS else None)
    ib = lambda n, shp, dt: net.buf('dec.' + n, shp, dt)
    tokens = ib('tokens', (B,), torch.int64)
    O.memset_zero(tokens)                                       # <bos>
    cur, new = st.new_states('a'), st.new_states('b')
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
            logits = st.step(cur, new, tokens)
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
    names = st.state_names()
    for t in range(T):
        logits = st.step(cur, new, tokens)
        O.decode_beam_step(logits, V1, B, t, T, bseq, blp, bsum, [(new[k][0], cur[k][0], new[k][1], cur[k][1]) for k in names], st.R,
                           tokens, parents, done, cnt)
    rec = rec_dev.cpu().numpy()                                 # the one read-back
    rec = rec[1:].reshape(B * T, RW)[:int(rec[0])]
    beams = [{'seq': [int(v) for v in r[:T]], 'logps': [float(v) for v in r[T:2 * T].view(np.float32)], 'p': float(r[2 * T:2 * T + 1].view(np.float32)[0]),
              'index': int(r[2 * T + 1])} for r in rec]
    beams = sorted(beams, key=lambda b: -b['p'])[:B]            # stable: completion order among equals (CaptionModel.py:123)
    best = beams[0]
    n = best['seq'].index(0) if 0 in best['seq'] else T
    return {'seq': best['seq'][:n], 'logprobs': best['logps'][:n], 'beams': beams}
