"""The captioners of the caption-cycle branch (--caption_model; lib/caption_models/AttModel.py = ATT, lib/misc/utils.py = CRIT): one class
each, CAPTIONERS[name], created by the network beside `cap_model` and holding a reference to it.  A captioner uses the network's buffers
(`buf`), parameters (`P`), transposed copies (`wT`, `bwd_x`), dropout streams (`_drop`), `att_embed`, step dictionary `t` and options, and
reads `cap_projected` / `cap_persistent` from it at call time (tools and tests set them after construction).

Training (nets/resnet_v1.py: _caption_pre / _caption_fwd / _caption_bwd) and decoding (nets/decode.py) run the SAME per-token launches:
each captioner has one `token` function (AdaAtt: adaatt.cell_fwd, the loop body of adaatt.core_fwd), which training calls with rows
i / i + 1 of its (S + 1)-row state arrays (row 0 stays zero) and decoding with row r of its `cur` / `new` sets, and one function per
per-sentence product (`projected`, `fcrow`, `token_inputs`) that takes the caller's buffer.  Training keeps its buffers under `cap.*` /
`td.*` / `ada.*`, decoding under `dec.*`: a caption decoded between a forward and its backward leaves what that backward reads alone."""
import functools
import math

import torch

from .. import ops as O
from . import adaatt as AA
from .params import ADAATT_GATES

f32 = torch.float32
L = 196                     # attention locations: the 14 x 14 pooling of layer4 on the map
SC = 256                    # per-row scratch tail of the attention kernels


class Captioner(object):
    """head (att_embed, ctx2att), tail (logits, loss) and fc_embed of every captioner (ATT:60-101; CRIT:43-53)"""
    reads_fc = False        # the captioner reads fc_feats (Att2in2Model deletes fc_embed)
    tag = 'cap'             # prefix of the training buffers and step-dictionary keys that are the captioner's own
    x_name, x_blocks = 'xpre', 4        # `token_inputs`: its buffer below the tag (training) or 'dec.' (decoding), its width in rnn_size
    w_keys = ()             # below 'caption_model.core.': the parameters `token` reads, in the order it unpacks them
    states = ('h', 'c')     # decoding: the state arrays a step reads and writes

    def __init__(self, net):
        self.net = net
        self.pv = lambda k: net.P.view('caption_model.' + k)                    # a parameter, its gradient, its transposed copy
        self.gv = lambda k: net.P.view('caption_model.' + k, net.P.grad)
        self.wT = lambda k: net.wT['caption_model.' + k][0]
        own = self.tag + '.'
        self.b = lambda n, shp, zero=False: net.buf(own + n, shp, f32, zero)    # float buffers: training's, decoding's
        self.db = lambda n, shp, zero=False: net.buf('dec.' + n, shp, f32, zero)

    def dims(self):
        o = self.net.opt
        return o['rnn_size'], o['input_encoding_size'], o['att_hid_size']

    def in_width(self):
        return self.x_blocks * self.net.opt['rnn_size']

    def masked(self, x, m, b, *buf):
        """x under the dropout mask m in the buffer b(*buf); x itself where there is none"""
        if m is None:
            return x
        out = b(*buf); O.mul(x, m, out)
        return out

    def sentence(self, ad, patt, **products):
        """what `token` reads of one sentence: the head's outputs, the per-sentence products and the parameter views"""
        return dict(ad=ad, patt=patt, w=tuple(self.pv('core.' + k) for k in self.w_keys), **products)

    # ------------------------------------------------------------------ training: pre -> fwd -> bwd (+ the deferred gradients)
    def pre(self, d):
        """token-only part of fwd / bwd, issued early on the language stream: dropout masks (att, fc if read, xt, out, then the captioner's
        own), word embedding, `token_inputs` for all S tokens, the zeroed backward buffer"""
        net, S = self.net, d['S']
        R, IE, AH = self.dims()
        shapes = [('att', (L, R))] + ([('fc', (R,))] if self.reads_fc else []) + [('xt', (S, IE)), ('out', (S, R))] + self.more_masks(S)
        pre = {'drop_' + k: net._drop(k, shp, net.opt['drop_prob_lm']) for k, shp in shapes}
        xt, x = net.buf('cap.xt', (S, IE), f32), self.b(self.x_name, (S, self.in_width()))
        O.embed_fwd(self.pv('embed.0.weight'), d['cap_in'], pre['drop_xt'], xt, S, IE, True)
        self.token_inputs(xt, x, S)
        self.zeroed(True, views=False)
        pre.update(xt=xt, x=x, zeroed=True)
        return pre

    def more_masks(self, S):
        return []

    def zeroed(self, clear, views=True):
        """the gradients that backward adds to, side by side in one buffer that one launch clears (`zero_layout`: names and shapes): `pre`
        clears it (or `bwd`, where no `pre` ran), `bwd` takes its named views"""
        lay = self.zero_layout()
        n = [math.prod(shp) for _, shp in lay]
        zb = self.b('bwd_zero', (sum(n),), zero=clear)
        return {k: v.view(shp) for (k, shp), v in zip(lay, zb.split(n))} if views else None

    def head(self, att_feats, b, mask=None):
        """att_embed (Linear + ReLU on the 196 attention features) -> attention dropout (training passes its mask) -> ctx2att, in the
        caller's float buffers b(name, shape): (a, ad [196][rnn_size], patt [196][att_hid_size])"""
        R, IE, AH = self.dims()
        a, patt = b('a', (L, R)), b('patt', (L, AH))
        self.net.att_embed.fwd(att_feats, L, 1, 1, a, relu=True, out_f32=True)
        ad = self.masked(a, mask, b, 'ad', (L, R))
        O.linear_fwd(ad, self.pv('ctx2att.weight'), self.pv('ctx2att.bias'), patt, L, AH, R)
        return a, ad, patt

    def fwd(self, d, att_feats, loss):
        """head -> the captioner's recurrence (recur_fwd: its outputs h [S][rnn_size]) -> output dropout -> logits -> log-softmax + masked
        NLL into loss[5] (ATT:60-101; CRIT:43-53)"""
        net, t, S = self.net, self.net.t, d['S']
        R, V1 = net.opt['rnn_size'], net.opt['vocab_size'] + 1
        pre = getattr(net, '_cap_pre', None) or self.pre(d)
        a, ad, patt = self.head(att_feats, lambda n, shp: net.buf('cap.' + n, shp, f32), pre['drop_att'])
        ho = self.masked(self.recur_fwd(S, pre, ad, patt), pre['drop_out'], net.buf, 'cap.ho', (S, R), f32)
        logits, dlogits = net.buf('cap.logits', (S, V1), f32), net.buf('cap.dlogits', (S, V1), f32)
        O.linear_fwd(ho, self.pv('logit.weight'), self.pv('logit.bias'), logits, S, V1, R)
        lp = net.buf('cap.logp', (S, V1), f32) if net.keep_logprobs else None
        O.logsoftmax_nll(logits, d['cap_tgt'], d['cap_mask'], S, V1, net._cap_loss_weight, loss[5:6], dlogits, lp)
        t.update({'cap.a_pre': a, 'cap.drop_att': pre['drop_att'], 'cap.drop_out': pre['drop_out'], 'cap.ad': ad, 'cap.patt': patt, 'cap.xt': pre['xt'],
                  'cap.drop_xt': pre['drop_xt'], 'cap.ho': ho, 'cap.dlogits': dlogits, 'cap.logp': lp, self.tag + '.zeroed': pre.get('zeroed')})

    def bwd(self, d, att_feats):
        """returns d(att_feats) in the activation dtype [196][att_feat_size], also left in net.t['cap.datt']; a captioner that reads fc_feats
        leaves d(fc_feats) float [fc_feat_size] in net.t['cap.dfc'].  Only d(att_feats) is on the step's critical path (the main queue waits
        for it at the caption join): the parameter gradients that nothing downstream reads are collected in `later` = net._cap_deferred and
        issued after the branch has produced its result (caption_branch: on the language stream, behind the join point); the logit layer's
        is the first."""
        net, t, S = self.net, self.net.t, d['S']
        R, V1 = net.opt['rnn_size'], net.opt['vocab_size'] + 1
        dlogits = t['cap.dlogits']
        later = net._cap_deferred = []
        later.append(lambda: O.linear_bwd_w(dlogits, t['cap.ho'], self.gv('logit.weight'), self.gv('logit.bias'), S, V1, R))
        dho = net.buf('cap.dho', (S, R), f32)                # d(outputs of the recurrence)
        net.bwd_x(dlogits, 'caption_model.logit.weight', dho, S, mul=t['cap.drop_out'])
        dad = self.recur_bwd(d, dho, later)                  # d(ad) [196][rnn_size], complete
        dadT = net.buf('cap.dadT', (L, R))
        # dropout mask (it multiplies the accumulated sum, not only this term), ReLU backward and the cast to the activation dtype: one launch
        O.mask_relu_cast(dad, t['cap.drop_att'], t['cap.a_pre'], dadT)
        net.att_embed.wgrad(dadT, att_feats, L, 1, 1)
        datt = t['cap.datt'] = net.buf('cap.datt_feats', (L, net.opt['att_feat_size']))
        net.att_embed.dgrad(dadT, L, 1, 1, datt)
        return datt

    def shared_grads(self, d, dxt, dpatt, ad, bias_rows=None):
        """the end of every captioner's deferred gradients: d(xt) [S][input_encoding_size] -> the word embedding; ctx2att's weight, and its
        bias as the column sums of dpatt or, where the captioner has them in a better-conditioned form, of bias_rows [S][att_hid_size]"""
        t, S = self.net.t, d['S']
        R, IE, AH = self.dims()
        AH = int(dpatt.shape[1])
        O.embed_bwd(dxt, t['cap.xt'], d['cap_in'], t['cap.drop_xt'], self.gv('embed.0.weight'), S, IE, True)
        O.linear_bwd_w(dpatt, ad, self.gv('ctx2att.weight'), self.gv('ctx2att.bias') if bias_rows is None else None, L, AH, R)
        if bias_rows is not None:
            O.colsum(bias_rows, S, AH, AH, self.gv('ctx2att.bias'))

    # ------------------------------------------------------------------ fc_embed (the captioners that read fc_feats)
    def fc_embed(self, fc, b, mask=None):
        """Linear + ReLU (+ dropout: training passes its mask) on the pooled vector fc [fc_feat_size] -> (fc in float, fc_embed, fc_embed
        after the dropout); b(name, shape): the caller's float buffers"""
        R, FC = self.net.opt['rnn_size'], self.net.opt['fc_feat_size']
        if fc.dtype != f32:
            fc32 = b('fc32', (FC,)); O.cast(fc, fc32)
        else:
            fc32 = fc
        fce = b('fce', (R,))
        O.linear_fwd(fc32, self.pv('fc_embed.0.weight'), self.pv('fc_embed.0.bias'), fce, 1, R, FC, act=1)
        return fc32, fce, self.masked(fce, mask, b, 'fcd', (R,))

    def fc_fwd(self, pre):
        """training: fc_embed of t['fc_feats'] and its per-sentence product `fcrow`, kept for backward"""
        t = self.net.t
        fc32, fce, fcd = self.fc_embed(t['fc_feats'], self.b, pre['drop_fc'])
        fcrow = self.b('fcrow', (self.in_width(),))
        self.fcrow(fcd, fcrow)
        t.update({self.tag + '.fc32': fc32, self.tag + '.fce': fce, self.tag + '.fcd': fcd, self.tag + '.drop_fc': pre['drop_fc']})
        return fcrow

    def fc_bwd(self, dfcd):
        """training: d(fc_embed after the dropout) [rnn_size], overwritten -> d(fc_feats) float [fc_feat_size] in t['cap.dfc']"""
        net, t = self.net, self.net.t
        if t[self.tag + '.drop_fc'] is not None:
            O.mul(dfcd, t[self.tag + '.drop_fc'], dfcd)
        O.act_bwd(dfcd, t[self.tag + '.fce'], 1)
        dfc = t['cap.dfc'] = self.b('dfc', (net.opt['fc_feat_size'],))
        net.bwd_x(dfcd, 'caption_model.fc_embed.0.weight', dfc, 1)

    # ------------------------------------------------------------------ decoding: states as (array [B][...], leading dimension) per name
    def new_states(self, tag, B):
        """one set of state arrays (zeroed: the start state)"""
        R = self.net.opt['rnn_size']
        return {k: (self.db('%s.%s' % (k, tag), (B, R), zero=True), R) for k in self.states}

    def decode_start(self, ad, patt, fc):
        """the per-sentence products into decoding's buffers -> what `token` reads of the sentence"""
        fcrow = self.db('fcrow', (self.in_width(),))
        self.fcrow(self.fc_embed(fc, self.db)[2], fcrow)
        return self.sentence(ad, patt, fcrow=fcrow)

    # ------------------------------------------------------------------ the caption branch on rows (nets/caption_rows.py: the batched route)
    # b(name, shape, zero=False): the route's float buffers ('rows.*'), sized for nb rows; n <= nb rows of the chunk are in use.  A captioner
    # that serves the route has rows_forced (teacher forcing: the token-only work of the T inputs, once per call -> what rows_step takes as
    # pre_t, per t), rows_head (per chunk), rows_states (two zeroed sets), rows_step (one token: cur -> new, returns the outputs
    # [nb][rnn_size]) and rows_gather (beam search: the state arrays of set `src` as (in, out, ld_in, ld_out) into set `dst`); the number
    # of entries each issues depends neither on n nor on count[0].  Beam search calls rows_step with group = beam_size: n and nb then count
    # STATE rows, `group` consecutive ones per row of the head, and the row entries are their *_groups forms (on_rows).
    @staticmethod
    def on_rows(name, group, head, n, *tail, **kw):
        """ops.<name>_rows(*head, n, *tail), or with group > 1 ops.<name>_groups(*head, n, group, *tail): one call site for both"""
        if group == 1:
            return getattr(O, name + '_rows')(*head, n, *tail, **kw)
        return getattr(O, name + '_groups')(*head, n, group, *tail, **kw)

    def rows_ok(self):
        """the batched route serves this captioner at the network's shapes (otherwise: the loop)"""
        return False


class Att2in2(Captioner):
    """ATT:406-466.  The recurrence as one resident launch (csrc/cap_recur.hip) where the shapes allow, else 3 launches per token in the
    projected-attention form (P = att . W_a2c^T once per sentence; csrc/caption_step.hip) or 3 in the unprojected one"""

    x_name, x_blocks = 'sums', 5
    w_keys = ('attention.h2att.weight', 'attention.h2att.bias', 'h2h.weight', 'h2h.bias', 'attention.alpha_net.weight', 'attention.alpha_net.bias',
              'a2c.weight', 'a2c.bias')

    def proj(self):
        return self.net.cap_projected and self.net.opt['rnn_size'] <= 1024

    def transposed_keys(self):
        # (the projected-attention recurrence never multiplies by a2c^T row by row)
        return ['core.h2h.weight', 'core.attention.h2att.weight'] + ([] if self.proj() else ['core.a2c.weight'])

    def token_inputs(self, xt, out, M):
        """i2h of M embedded tokens -> out [M][5 rnn_size] (`token` adds h2h(h) to its row)"""
        R, IE, AH = self.dims()
        O.linear_fwd(xt, self.pv('core.i2h.weight'), self.pv('core.i2h.bias'), out, M, 5 * R, IE)

    def projected(self, ad, b):
        """P = att . W_a2c^T [196][2 rnn_size] in the caller's buffer b('P', shape), once per sentence; None in the unprojected form"""
        R = self.net.opt['rnn_size']
        if not self.proj():
            return None
        Pm = b('P', (L, 2 * R)); O.linear_fwd(ad, self.pv('core.a2c.weight'), None, Pm, L, 2 * R, R)
        return Pm

    def token(self, H, sums, h0, c0, h1, c1, att_h, tanh_ws, wgt, save, scr):
        """h2att(h) and h2h(h) (+= i2h sums) in one launch; attention; a2c Linear fused with the gates.  scr: the dots row [256]
        (projected: H['Pm'] is set) or the attention result's row [rnn_size + 256]"""
        R, IE, AH = self.dims()
        h2w, h2b, hw, hb, aw, ab, a2w, a2b = H['w']
        O.linear2_fwd(h0, R, h2w, h2b, att_h, AH, False, hw, hb, sums, 5 * R, True)
        if H['Pm'] is not None:
            O.cap_att_dots_fwd(H['patt'], att_h, aw, ab, L, AH, tanh_ws, scr)
            O.cap_apply_gates_fwd(H['Pm'], scr, a2b, sums, c0, c1, h1, save, wgt, L, R)
        else:
            O.cap_attention_fwd(H['patt'], H['ad'], att_h, aw, ab, L, AH, tanh_ws, wgt, scr)
            O.cap_a2c_gates_fwd(scr, a2w, a2b, R, sums, c0, c1, h1, save, R)

    def zero_layout(self):
        R, IE, AH = self.dims()
        return [('dpatt', (L, AH)), ('dad', (L, R)), ('dh', (2, R)), ('dc', (2, R))] + ([('dP', (L, 2 * R))] if self.proj() else [])

    def bufs(self, S):
        R, IE, AH = self.dims()
        return dict(hs=self.b('hfull', (S + 1, R)), cs=self.b('cfull', (S + 1, R)), save=self.b('save', (S, 6 * R)), tanh=self.b('tanh', (S, L, AH)),
                    wgt=self.b('wgt', (S, L)), ares=self.b('ares', (S, R + SC)))

    def recur_fwd(self, S, pre, ad, patt):
        net, t, sums = self.net, self.net.t, pre['x']
        R, IE, AH = self.dims()
        B = self.bufs(S)
        hs, cs, att_h = B['hs'], B['cs'], self.b('att_h', (S, AH))
        Pm = t['cap.P'] = self.projected(ad, self.b)
        scr = B['ares'] if Pm is None else self.b('dots', (S, 256))
        H = self.sentence(ad, patt, Pm=Pm)
        t['cap.resident'] = resident = Pm is not None and net.cap_persistent and O.cap_recur_supported(S, R, AH, L)
        if resident:
            # the whole recurrence as one resident launch: 32 workgroups own 16 units each, three granule exchanges per token
            if getattr(net, '_cap_state', None) is None:
                net._cap_state = (O.cap_recur_state(False), O.cap_recur_state(True))
            h2w, h2b, hw, hb, aw, ab, a2w, a2b = H['w']
            O.cap_recur_fwd(hw, hb, h2w, h2b, patt, aw, ab, Pm, a2b, sums, hs, cs, B['save'], B['tanh'], B['wgt'], net._cap_state[0], S, R, AH, L)
        for i in range(0 if resident else S):
            self.token(H, sums[i], hs[i], cs[i], hs[i + 1], cs[i + 1], att_h[i], B['tanh'][i], B['wgt'][i], B['save'][i], scr[i])
        return hs[1:]

    def recur_bwd(self, d, dho, later):
        net, t, S = self.net, self.net.t, d['S']
        R, IE, AH = self.dims()
        pv, gv = self.pv, self.gv
        B = self.bufs(S)
        hs, cs, save, tanh_ws, wgt, ares = B['hs'], B['cs'], B['save'], B['tanh'], B['wgt'], B['ares']
        ad = t['cap.ad']
        dsums, da2c = self.b('dsums', (S, 5 * R)), self.b('da2c', (S, 2 * R))
        datt_h, dares, ddot = self.b('datt_h', (S, AH + SC)), self.b('dares', (S, R)), self.b('ddot', (S, L))
        Z = self.zeroed(not t.get('cap.zeroed'))
        dpatt, dad, dh, dc, dP = Z['dpatt'], Z['dad'], Z['dh'], Z['dc'], Z.get('dP')
        proj = dP is not None
        wT_h2h, wT_h2att = self.wT('core.h2h.weight'), self.wT('core.attention.h2att.weight')
        aw = pv('core.attention.alpha_net.weight')
        k = 0
        if proj:
            Pm, dwl = t['cap.P'], self.b('dwl', (S, 256))
        if t.get('cap.resident'):
            O.cap_recur_bwd(pv('core.h2h.weight'), pv('core.attention.h2att.weight'), Pm, aw, save, cs, wgt, tanh_ws, dho,
                            dsums, da2c, ddot, datt_h, net._cap_state[1], S, R, AH, L)
        for i in range(-1 if t.get('cap.resident') else S - 1, -1, -1):
            if proj:
                # 3 launches per step: gates + d(weight) = P . d(a2c); softmax backward + datt_h; dh(i-1)
                O.cap_gates_bwd_dw(dh[k], dc[k], save[i], cs[i], Pm, dsums[i], da2c[i], dc[1 - k], dwl[i], L, R, dh2=dho[i])
                O.cap_attention_bwd_step2(dwl[i], tanh_ws[i], wgt[i], aw, L, AH, ddot[i], datt_h[i])
            else:
                # 4 launches per step: gates (dh = recurrent part + this step's output gradient), a2c^T, the attention pieces the
                # recurrence needs, and dh(i-1) = W_h2h^T dsums + W_h2att^T datt_h
                O.cap_gates_bwd(dh[k], dc[k], save[i], cs[i], dsums[i], da2c[i], dc[1 - k], R, dh2=dho[i])
                net.bwd_x(da2c[i], 'caption_model.core.a2c.weight', dares[i], 1)
                O.cap_attention_bwd_step(dares[i], ad, tanh_ws[i], wgt[i], aw, L, AH, ddot[i], datt_h[i])
            O.linear_sum2_fwd(dsums[i], wT_h2h, 5 * R, datt_h[i], wT_h2att, AH, dh[1 - k], R)
            k = 1 - k
        O.cap_attention_bwd_batched(ddot, wgt, None if proj else dares, R, tanh_ws, aw, S, L, AH, dpatt, dad,
                                    gv('core.attention.alpha_net.weight'), gv('core.attention.alpha_net.bias'))
        if proj:
            # d(P) = sum_t weight_t (x) d(a2c)_t  [L][2R];  d(att) += d(P) . W_a2c
            O.linear_bwd_w(wgt, da2c, dP, None, S, L, 2 * R)
            net.bwd_x(dP, 'caption_model.core.a2c.weight', dad, L, accumulate=True)
        hprev = hs[0:S]

        def recurrence_grads():
            if proj:
                O.linear_bwd_w(dP, ad, gv('core.a2c.weight'), gv('core.a2c.bias'), L, 2 * R, R)
            else:
                O.linear_bwd_w(da2c, ares, gv('core.a2c.weight'), gv('core.a2c.bias'), S, 2 * R, R, ldx=R + SC)
            O.linear_bwd_w(dsums, hprev, gv('core.h2h.weight'), gv('core.h2h.bias'), S, 5 * R, R)
            O.linear_bwd_w(datt_h, hprev, gv('core.attention.h2att.weight'), gv('core.attention.h2att.bias'), S, AH, R, lddy=AH + SC)
            O.linear_bwd_w(dsums, t['cap.xt'], gv('core.i2h.weight'), gv('core.i2h.bias'), S, 5 * R, IE)
            dxt = self.b('dxt', (S, IE))
            net.bwd_x(dsums, 'caption_model.core.i2h.weight', dxt, S)
            self.shared_grads(d, dxt, dpatt, ad)
        later.append(recurrence_grads)
        net.bwd_x(dpatt, 'caption_model.ctx2att.weight', dad, L, accumulate=True)
        return dad

    def decode_start(self, ad, patt, fc):
        return self.sentence(ad, patt, Pm=self.projected(ad, self.db))

    def decode_step(self, H, cur, new, sums, B):
        """one step on B rows: x [B][in_width()] = token_inputs of the B tokens -> the outputs [B][rnn_size]"""
        R, IE, AH = self.dims()
        b = self.db
        att_h, tanh_ws, wgt, save = b('att_h', (B, AH)), b('tanh', (L, AH)), b('wgt', (L,)), b('save', (6 * R,))
        scr = b('dots', (256,)) if H['Pm'] is not None else b('ares', (R + 256,))
        (h0, _), (c0, _), (h1, _), (c1, _) = cur['h'], cur['c'], new['h'], new['c']
        for r in range(B):
            self.token(H, sums[r], h0[r], c0[r], h1[r], c1[r], att_h[r], tanh_ws, wgt, save, scr)
        return h1

    # ---- on rows: the projected form.  8 launches a token with the logits and the decision (6 when scoring)
    def rows_ok(self):
        return bool(self.proj()) and self.net.opt['rnn_size'] <= 1024

    def rows_forced(self, b, inputs, T):
        """the embedding and i2h of the T inputs; h2h's bias joins each row"""
        R, IE, AH = self.dims()
        xs, bias = b('xt_all', (T, IE)), b('bias_all', (T, 5 * R))
        O.embed_fwd(self.pv('embed.0.weight'), inputs, None, xs, T, IE, True)
        self.token_inputs(xs, bias, T)
        for t in range(T):
            O.add_f32(bias[t], self.pv('core.h2h.bias'), bias[t])
        return bias

    def rows_head(self, b, att, fc, n, nb):
        """att_embed (Linear + ReLU), ctx2att and P = att . W_a2c^T as GEMMs on n * 196 rows"""
        R, IE, AH = self.dims()
        a, patt, Pm = b('a', (nb * L, R)), b('patt', (nb * L, AH)), b('P', (nb * L, 2 * R))
        self.net.att_embed.fwd(att, n * L, 1, 1, a, relu=True, out_f32=True)
        O.linear_fwd(a, self.pv('ctx2att.weight'), self.pv('ctx2att.bias'), patt, n * L, AH, R)
        O.linear_fwd(a, self.pv('core.a2c.weight'), None, Pm, n * L, 2 * R, R)
        return dict(patt=patt, Pm=Pm)

    def rows_states(self, b, nb):
        R = self.net.opt['rnn_size']
        return [(b('h.' + k, (nb, R), True), b('c.' + k, (nb, R), True)) for k in 'ab']

    def rows_gather(self, src, dst):
        R = self.net.opt['rnn_size']
        return [(src[0], dst[0], R, R), (src[1], dst[1], R, R)]

    def rows_step(self, b, H, cur, new, n, nb, tokens, pre_t, count, row0, group=1):
        R, IE, AH = self.dims()
        pv = self.pv
        sums, att_h, dots = b('sums', (nb, 5 * R)), b('att_h', (nb, AH)), b('dots', (nb, 256))
        (h0, cp), (h1, c1) = cur, new
        if pre_t is not None:
            O.linear_fwd(h0, pv('core.h2h.weight'), pre_t, sums, n, 5 * R, R)
        else:
            xt = b('xt', (nb, IE))
            O.embed_fwd(pv('embed.0.weight'), tokens, None, xt, n, IE, True)
            self.token_inputs(xt, sums, n)
            O.linear_fwd(h0, pv('core.h2h.weight'), pv('core.h2h.bias'), sums, n, 5 * R, R, accumulate=True)
        O.linear_fwd(h0, pv('core.attention.h2att.weight'), pv('core.attention.h2att.bias'), att_h, n, AH, R)
        self.on_rows('cap_att_dots', group, (H['patt'], att_h, pv('core.attention.alpha_net.weight'), pv('core.attention.alpha_net.bias')), n, L, AH,
                     dots, count, row0)
        self.on_rows('cap_apply_gates', group, (H['Pm'], dots, pv('core.a2c.bias'), sums, cp, c1, h1), n, L, R, count, row0)
        return h1


class TopDown(Captioner):
    """ATT:60-101,370-395,486-490.  Two nn.LSTMCell per token: att_lstm([h_lang(i-1); fc; xt_i]) -> attention(h_att(i)) ->
    lang_lstm([att_res; h_att(i)]); the output is h_lang(i).  Per-token launches only (csrc/caption_step.hip), 5 forward and 5 backward.
    Training's (S+1)-row arrays: hl / cl / ca row i+1 = step i; `lin` row i+1 = [att_res(i) | h_att(i)], the language cell's input AND the
    attention cell's state."""
    reads_fc = True
    tag = 'td'
    states = ('hl', 'cl', 'ca', 'ha')
    w_keys = ('att_lstm.weight_ih', 'att_lstm.weight_hh', 'lang_lstm.weight_ih', 'lang_lstm.weight_hh', 'lang_lstm.bias_ih', 'lang_lstm.bias_hh',
              'attention.h2att.weight', 'attention.h2att.bias', 'attention.alpha_net.weight', 'attention.alpha_net.bias')

    def transposed_keys(self):
        # both cells' matrices (att_lstm.weight_ih: its h_lang and fc column blocks, rows of the transposed copy) and h2att
        return ['core.' + k for k in ('att_lstm.weight_ih', 'att_lstm.weight_hh', 'lang_lstm.weight_ih', 'lang_lstm.weight_hh', 'attention.h2att.weight')]

    def token_inputs(self, xt, out, M):
        """the xt columns of att_lstm.weight_ih (+ bias_ih) for M embedded tokens -> out [M][4 rnn_size]"""
        R, IE, AH = self.dims()
        O.linear_fwd(xt, self.pv('core.att_lstm.weight_ih')[2 * R:], self.pv('core.att_lstm.bias_ih'), out, M, 4 * R, IE, ldw=IE + 2 * R)

    def fcrow(self, fcd, out):
        """the fc columns of att_lstm.weight_ih (+ bias_hh) on fc_embed's output: once per sentence -> out [4 rnn_size]"""
        R, IE, AH = self.dims()
        O.linear_fwd(fcd, self.pv('core.att_lstm.weight_ih')[R:], self.pv('core.att_lstm.bias_hh'), out, 1, 4 * R, R, ldw=IE + 2 * R)

    def token(self, H, xpre, hl0, cl0, ca0, ha0, hl1, cl1, ca1, lin1, att_h, tanh_ws, wgt, dots, act_a, act_l):
        """the five launches of one token.  lin1 [2 rnn_size] = [att_res | h_att]: the new attention state is its second half"""
        R, IE, AH = self.dims()
        Ka = IE + 2 * R
        wa_ih, wa_hh, wl_ih, wl_hh, bl_ih, bl_hh, h2w, h2b, aw, ab = H['w']
        h_att = lin1[R:]
        O.topdown_cell_fwd(xpre, H['fcrow'], None, [(hl0, wa_ih, Ka, R), (ha0, wa_hh, R, R)], ca0, ca1, h_att, act_a, R)
        O.linear_fwd(h_att, h2w, h2b, att_h, 1, AH, R)
        O.cap_att_dots_fwd(H['patt'], att_h, aw, ab, L, AH, tanh_ws, dots)
        O.cap_att_apply_fwd(H['ad'], dots, L, R, wgt, lin1)
        O.topdown_cell_fwd(None, bl_ih, bl_hh, [(lin1, wl_ih, 2 * R, 2 * R), (hl0, wl_hh, R, R)], cl0, cl1, hl1, act_l, R)

    def zero_layout(self):
        R, IE, AH = self.dims()
        return [('dpatt', (L, AH)), ('dad', (L, R)), ('dgsum', (4 * R,))]         # dgsum: the sum over tokens of d(att gates)

    def bufs(self, S):
        R, IE, AH = self.dims()
        b = self.b
        return dict(hl=b('hl', (S + 1, R)), cl=b('cl', (S + 1, R)), ca=b('ca', (S + 1, R)), lin=b('lin', (S + 1, 2 * R)), act_a=b('act_a', (S, 4 * R)),
                    act_l=b('act_l', (S, 4 * R)), att_h=b('att_h', (S, AH)), tanh=b('tanh', (S, L, AH)), wgt=b('wgt', (S, L)), dots=b('dots', (S, 256)))

    def recur_fwd(self, S, pre, ad, patt):
        R = self.net.opt['rnn_size']
        H = self.sentence(ad, patt, fcrow=self.fc_fwd(pre))
        B = self.bufs(S)
        hl, cl, ca, lin, xpre = B['hl'], B['cl'], B['ca'], B['lin'], pre['x']
        for i in range(S):
            self.token(H, xpre[i], hl[i], cl[i], ca[i], lin[i][R:], hl[i + 1], cl[i + 1], ca[i + 1], lin[i + 1],
                       B['att_h'][i], B['tanh'][i], B['wgt'][i], B['dots'][i], B['act_a'][i], B['act_l'][i])
        return hl[1:]

    def recur_bwd(self, d, dho, later):
        net, t, S = self.net, self.net.t, d['S']
        R, IE, AH = self.dims()
        Ka = IE + 2 * R
        pv, gv, wT, b = self.pv, self.gv, self.wT, self.b
        B = self.bufs(S)
        hl, cl, ca, lin = B['hl'], B['cl'], B['ca'], B['lin']
        ad = t['cap.ad']
        Z = self.zeroed(not t.get('td.zeroed'))
        dpatt, dad, dgsum = Z['dpatt'], Z['dad'], Z['dgsum']
        dga, dgl, dares, dwl = b('dga', (S, 4 * R)), b('dgl', (S, 4 * R)), b('dares', (S, R)), b('dwl', (S, 256))
        ddot, datt_h, dca, dcl = b('ddot', (S, L)), b('datt_h', (S, AH)), b('dca', (2, R)), b('dcl', (2, R))
        ta_ih, ta_hh, tl_ih, tl_hh, th2 = wT('core.att_lstm.weight_ih'), wT('core.att_lstm.weight_hh'), wT('core.lang_lstm.weight_ih'), \
            wT('core.lang_lstm.weight_hh'), wT('core.attention.h2att.weight')
        aw = pv('core.attention.alpha_net.weight')
        G = 4 * R
        k = 0
        for i in range(S - 1, -1, -1):
            last = i == S - 1
            # language cell: dh = this token's output gradient + what the NEXT token's two cells read of h_lang(i)
            O.topdown_cell_bwd([] if last else [(dga[i + 1], ta_ih, G, G), (dgl[i + 1], tl_hh, G, G)], dho[i], None, None if last else dcl[k],
                               B['act_l'][i], cl[i], cl[i + 1], dgl[i], dcl[1 - k], R)
            # attention: d(att_res) through the first R rows of lang_lstm.weight_ih^T, d(weight) = att . d(att_res), softmax backward + d(att_h)
            O.linear_fwd(dgl[i], tl_ih, None, dares[i], 1, R, G)
            O.linear_fwd(dares[i], ad, None, dwl[i], 1, L, R)
            O.cap_att_bwd_step_centered(dwl[i], B['tanh'][i], B['wgt'][i], aw, L, AH, ddot[i], datt_h[i])
            # attention cell: dh = the language cell's input + h2att + its own recurrence
            O.topdown_cell_bwd([(dgl[i], tl_ih[R * G:], G, G), (datt_h[i], th2, AH, AH)] + ([] if last else [(dga[i + 1], ta_hh, G, G)]), None, None,
                               None if last else dca[k], B['act_a'][i], ca[i], ca[i + 1], dga[i], dca[1 - k], R)
            k = 1 - k
        # everything the per-token launches left out of the attention, summed over the S tokens
        # (alpha_net.bias shifts every score alike and the softmax does not see it: its gradient is 0, and what the launch adds up for it -
        # sum ddot, pure rounding error - goes to a scratch word instead of the gradient buffer)
        O.cap_attention_bwd_batched(ddot, B['wgt'], None, R, B['tanh'], aw, S, L, AH, dpatt, dad, gv('core.attention.alpha_net.weight'),
                                    b('dab_unused', (1,)))
        O.linear_bwd_w(B['wgt'], dares, dad, None, S, L, R)                     # d(att) += sum_t weight_t (x) d(att_res)_t
        net.bwd_x(dpatt, 'caption_model.ctx2att.weight', dad, L, accumulate=True)
        # d(fc_feats): the fc columns see every token's gate gradient, so their sum goes through the transposed block once
        O.colsum(dga, S, G, G, dgsum)
        dfcd = b('dfcd', (R,))
        O.linear_fwd(dgsum, ta_ih[R * G:], None, dfcd, 1, R, G)
        self.fc_bwd(dfcd)

        def recurrence_grads():
            # the attention cell's input rows [h_lang(i-1) | fc | xt_i], packed once: its weight gradient is ONE product
            X = b('xatt', (S, Ka), zero=True)
            if S > 1:
                O.pack_rows(X[1:], Ka, hl[1:], R, S - 1, R)
            O.pack_rows(X[:, R:], Ka, t['td.fcd'], 0, S, R)
            O.pack_rows(X[:, 2 * R:], Ka, t['cap.xt'], IE, S, IE)
            O.linear_bwd_w(dga, X, gv('core.att_lstm.weight_ih'), gv('core.att_lstm.bias_ih'), S, G, Ka)
            O.linear_bwd_w(dga, lin[:, R:], gv('core.att_lstm.weight_hh'), gv('core.att_lstm.bias_hh'), S, G, R, ldx=2 * R)
            O.linear_bwd_w(dgl, lin[1:], gv('core.lang_lstm.weight_ih'), gv('core.lang_lstm.bias_ih'), S, G, 2 * R)
            O.linear_bwd_w(dgl, hl, gv('core.lang_lstm.weight_hh'), gv('core.lang_lstm.bias_hh'), S, G, R)
            O.linear_bwd_w(datt_h, lin[1:, R:], gv('core.attention.h2att.weight'), gv('core.attention.h2att.bias'), S, AH, R, ldx=2 * R)
            O.linear_bwd_w(dfcd, t[self.tag + '.fc32'], gv('fc_embed.0.weight'), gv('fc_embed.0.bias'), 1, R, net.opt['fc_feat_size'])
            dxt = net.buf('cap.dxt', (S, IE), f32)
            dX = b('dxatt', (S, Ka))
            net.bwd_x(dga, 'caption_model.core.att_lstm.weight_ih', dX, S)
            O.pack_rows(dxt, IE, dX[:, 2 * R:], Ka, S, IE)
            # ctx2att.bias enters the tanh like h2att's output: its gradient is sum_t datt_h[t], whose sum over the locations was taken in the
            # well-conditioned form; the column sums of dpatt would add that sum's rounding error back
            self.shared_grads(d, dxt, dpatt, ad, bias_rows=datt_h)
        later.append(recurrence_grads)
        return dad

    def new_states(self, tag, B):
        # h_att lives behind att_res in the language cell's input row [att_res | h_att], as in training
        R = self.net.opt['rnn_size']
        b = lambda k, w: self.db('%s.%s' % (k, tag), (B, w), zero=True)
        lin = b('lin', 2 * R)
        s = {k: (b(k, R), R) for k in ('hl', 'cl', 'ca')}
        s['ha'] = (lin[:, R:], 2 * R)
        s['_lin'] = lin
        return s

    def decode_step(self, H, cur, new, xpre, B):
        R, IE, AH = self.dims()
        b = self.db
        att_h, tanh_ws, wgt, dots, act = b('att_h', (B, AH)), b('tanh', (L, AH)), b('wgt', (L,)), b('dots', (256,)), b('act', (4 * R,))
        lin0, lin1 = cur['_lin'], new['_lin']
        hl0, cl0, ca0, hl1, cl1, ca1 = cur['hl'][0], cur['cl'][0], cur['ca'][0], new['hl'][0], new['cl'][0], new['ca'][0]
        for r in range(B):
            self.token(H, xpre[r], hl0[r], cl0[r], ca0[r], lin0[r][R:], hl1[r], cl1[r], ca1[r], lin1[r], att_h[r], tanh_ws, wgt, dots, act, act)
        return hl1

    # ---- on rows: `token`'s five launches with the two cells as l2s_lstm_cell_rows (a weight element fetched once per tile of rows, not
    # once per row) and the attention row-strided.  9 launches a token with the logits and the decision (7 when scoring)
    def rows_ok(self):
        return self.net.opt['rnn_size'] <= 1024

    def rows_forced(self, b, inputs, T):
        """the embedding and the xt columns of att_lstm.weight_ih (+ bias_ih) of the T inputs: step t takes row t for every row"""
        R, IE, AH = self.dims()
        xs, pre = b('xt_all', (T, IE)), b('xpre_all', (T, 4 * R))
        O.embed_fwd(self.pv('embed.0.weight'), inputs, None, xs, T, IE, True)
        self.token_inputs(xs, pre, T)
        return pre

    def rows_head(self, b, att, fc, n, nb):
        """att_embed (Linear + ReLU) and ctx2att as GEMMs on n * 196 rows; fc_embed (Linear + ReLU) and the fc product (`fcrow` per row:
        the fc columns of att_lstm.weight_ih + bias_hh) on n rows.  No projected attention: the top-down attention reads `a` itself"""
        R, IE, AH = self.dims()
        FC = self.net.opt['fc_feat_size']
        a, patt, fce, fcrow = b('a', (nb * L, R)), b('patt', (nb * L, AH)), b('fce', (nb, R)), b('fcrow', (nb, 4 * R))
        self.net.att_embed.fwd(att, n * L, 1, 1, a, relu=True, out_f32=True)
        O.linear_fwd(a, self.pv('ctx2att.weight'), self.pv('ctx2att.bias'), patt, n * L, AH, R)
        if fc.dtype != f32:
            fc32 = b('fc32', (nb, FC)); O.cast(fc, fc32)
        else:
            fc32 = fc
        O.linear_fwd(fc32, self.pv('fc_embed.0.weight'), self.pv('fc_embed.0.bias'), fce, n, R, FC, act=1)
        O.linear_fwd(fce, self.pv('core.att_lstm.weight_ih')[R:], self.pv('core.att_lstm.bias_hh'), fcrow, n, 4 * R, R, ldw=IE + 2 * R)
        return dict(a=a, patt=patt, fcrow=fcrow)

    def rows_states(self, b, nb):
        """two sets of hl | cl | ca [nb][R] and lin [nb][2R] = [att_res | h_att] side by side: one launch clears both"""
        R = self.net.opt['rnn_size']
        st = b('td_state', (2, 5 * nb * R), True)
        return [dict(zip(('hl', 'cl', 'ca', 'lin'), s.split([nb * R, nb * R, nb * R, 2 * nb * R]))) for s in st]

    def rows_gather(self, src, dst):
        R = self.net.opt['rnn_size']
        return [(src[k], dst[k], R, R) for k in ('hl', 'cl', 'ca')] + [(src['lin'][R:], dst['lin'][R:], 2 * R, 2 * R)]

    def rows_step(self, b, H, cur, new, n, nb, tokens, pre_t, count, row0, group=1):
        R, IE, AH = self.dims()
        Ka = IE + 2 * R
        pv = self.pv
        wa_ih, wa_hh, wl_ih, wl_hh, bl_ih, bl_hh, h2w, h2b, aw, ab = (pv('core.' + k) for k in self.w_keys)
        att_h, dots = b('att_h', (nb, AH)), b('dots', (nb, 256))
        if pre_t is not None:
            xpre, ld_pre = pre_t, 0
        else:
            xt, xpre, ld_pre = b('xt', (nb, IE)), b('xpre', (nb, 4 * R)), 4 * R
            O.embed_fwd(pv('embed.0.weight'), tokens, None, xt, n, IE, True)
            self.token_inputs(xt, xpre, n)
        lin0, lin1 = cur['lin'], new['lin']
        h_att = lin1[R:]
        self.on_rows('lstm_cell', group, (xpre, None, None, [(cur['hl'], R, wa_ih, Ka, R), (lin0[R:], 2 * R, wa_hh, R, R)], cur['ca'], new['ca'], h_att),
                     n, R, count, row0, ld_pre=ld_pre, pre2=H['fcrow'], ld_h=2 * R)
        O.linear_fwd(h_att, h2w, h2b, att_h, n, AH, R, ldx=2 * R)
        self.on_rows('cap_att_dots', group, (H['patt'], att_h, aw, ab), n, L, AH, dots, count, row0)
        self.on_rows('cap_att_apply', group, (H['a'], dots, lin1), n, L, R, count, row0, ld_res=2 * R)
        self.on_rows('lstm_cell', group, (None, bl_ih, bl_hh, [(lin1, 2 * R, wl_ih, 2 * R, 2 * R), (cur['hl'], R, wl_hh, R, R)], cur['cl'], new['cl'],
                                         new['hl']), n, R, count, row0)
        return new['hl']


class AdaAtt(Captioner):
    """ATT:211-368,468-477 (adaatt; adaattmo: five gate blocks, the transform is the max of two).  An LSTM with a sentinel gate, then an
    additive attention over the 196 locations + the sentinel.  Only the cell is recurrent: one launch per token each way; the attention runs
    once for all tokens (nets/adaatt.py has the sequence, csrc/adaatt_step.hip the kernels)."""
    reads_fc = True
    tag = 'ada'
    w_keys = AA.CELL_KEYS

    def __init__(self, net, G):
        Captioner.__init__(self, net)
        self.G, self.x_blocks = G, G + 1        # row blocks of w2h / v2h / h2h.0: in, forget, out, transform (adaattmo: two, their max)
        self.cpv = lambda k: self.pv('core.' + k)

    def transposed_keys(self):
        return ['core.lstm.h2h.0.weight', 'core.lstm.r_h2h.weight']     # what token i + 1 reads of h(i)

    def token_inputs(self, xt, out, M):
        """w2h(xt) | r_w2h(xt) for M embedded tokens -> out [M][(G + 1) rnn_size]"""
        R, IE, AH = self.dims()
        G, W = self.G, self.in_width()
        O.linear_fwd(xt, self.pv('core.lstm.w2h.weight'), self.pv('core.lstm.w2h.bias'), out, M, G * R, IE, ldy=W)
        O.linear_fwd(xt, self.pv('core.lstm.r_w2h.weight'), self.pv('core.lstm.r_w2h.bias'), out[:, G * R:], M, R, IE, ldy=W)

    def fcrow(self, fcd, out):
        """v2h | r_v2h of fc_embed's output: once per sentence -> out [(G + 1) rnn_size]"""
        R, G = self.net.opt['rnn_size'], self.G
        O.linear_fwd(fcd, self.pv('core.lstm.v2h.weight'), self.pv('core.lstm.v2h.bias'), out, 1, G * R, R)
        O.linear_fwd(fcd, self.pv('core.lstm.r_v2h.weight'), self.pv('core.lstm.r_v2h.bias'), out[G * R:], 1, R, R)

    def zero_layout(self):
        R = self.net.opt['rnn_size']
        return [('dpatt', (L, R)), ('dad', (L, R)), ('dgsum', (self.in_width(),))]      # dgsum: the sum over tokens of d(sums | n5)

    def more_masks(self, S):
        R = self.net.opt['rnn_size']
        return [('hA', (S, L + 1, R))] + [(k, (S, R)) for k in ('toph', 'fake', 'frl', 'hol')]

    def recur_fwd(self, S, pre, ad, patt):
        R = self.net.opt['rnn_size']
        B = {k: self.b(k, shp) for k, shp in AA.fwd_shapes(S, L, R).items()}
        masks = {k: pre['drop_' + k] for k in ('toph', 'fake', 'frl', 'hol', 'hA')}
        V = AA.core_fwd(O, self.cpv, B, pre['x'], self.fc_fwd(pre), ad, patt, masks, S, L, R, self.G)
        self.net.t.update({'ada.pre': pre, 'ada.B': B, 'ada.V': V, 'ada.masks': masks})
        return B['outs']

    def recur_bwd(self, d, dho, later):
        net, t, S = self.net, self.net.t, d['S']
        R, IE, AH = self.dims()
        G, W = self.G, self.in_width()
        gv = self.gv
        B, V, masks = t['ada.B'], t['ada.V'], t['ada.masks']
        ad = t['cap.ad']
        Z = self.zeroed(not t.get('ada.zeroed'))
        dpatt, dad, dgsum = Z['dpatt'], Z['dad'], Z['dgsum']
        D = {k: self.b(k, shp) for k, shp in AA.bwd_shapes(S, L, R, G).items()}
        bwd_x = lambda dy, k, dx, M, **kw: net.bwd_x(dy, 'caption_model.core.' + k, dx, M, **kw)
        AA.core_bwd(O, self.cpv, (self.wT('core.lstm.h2h.0.weight'), self.wT('core.lstm.r_h2h.weight')), bwd_x, B, D, V, dho, ad, dpatt, dad,
                    gv('core.attention.alpha_net.weight'), masks, S, L, R, G)
        # d(fc_feats): v2h | r_v2h see every token's gradient, so their sum goes through the two matrices once
        O.colsum(D['dall'], S, W, W, dgsum)
        dfcd = self.b('dfcd', (R,))
        bwd_x(dgsum, 'lstm.v2h.weight', dfcd, 1)
        bwd_x(dgsum[G * R:], 'lstm.r_v2h.weight', dfcd, 1, accumulate=True)
        self.fc_bwd(dfcd)
        net.bwd_x(dpatt, 'caption_model.ctx2att.weight', dad, L, accumulate=True)

        def recurrence_grads():
            AA.core_wgrads(O, lambda k: gv('core.' + k), B, D, V, dho, t['cap.xt'], t['ada.fcd'], dgsum, S, R, IE, G)
            O.linear_bwd_w(dfcd, t[self.tag + '.fc32'], gv('fc_embed.0.weight'), gv('fc_embed.0.bias'), 1, R, net.opt['fc_feat_size'])
            dxt = net.buf('cap.dxt', (S, IE), f32)
            bwd_x(D['dall'], 'lstm.w2h.weight', dxt, S, lddy=W)
            bwd_x(D['dall'][:, G * R:], 'lstm.r_w2h.weight', dxt, S, accumulate=True, lddy=W)
            # ctx2att.bias: the sum over the LOCATIONS of what enters the tanh, taken in the well-conditioned form by the step kernel (dctx);
            # the column sums of dpatt would add that sum's rounding error back (as for the top-down captioner)
            self.shared_grads(d, dxt, dpatt, ad, bias_rows=D['dctx'])
        later.append(recurrence_grads)
        return dad

    def decode_step(self, H, cur, new, xpre, B):
        """the cell per row, the attention on all B rows at once"""
        R = self.net.opt['rnn_size']
        Bf = {k: self.db('ada.' + k, shp) for k, shp in AA.fwd_shapes(B, L, R).items() if k not in ('hs', 'cs')}
        h0, c0, h1, c1 = cur['h'][0], cur['c'][0], new['h'][0], new['c'][0]
        for r in range(B):
            AA.cell_fwd(O, H['w'], xpre[r], H['fcrow'], h0[r], c0[r], h1[r], c1[r], Bf['fake'][r], Bf['save'][r], R, self.G)
        AA.att_fwd(O, self.cpv, Bf, h1, H['ad'], H['patt'], {}, B, L, R)
        return Bf['outs']


CAPTIONERS = {'att2in2': Att2in2, 'topdown': TopDown}
CAPTIONERS.update({name: functools.partial(AdaAtt, G=G) for name, G in ADAATT_GATES.items()})
