"""Shared by tests/test_topdown_{cpu,gpu}.py: the oracle of the top-down attention captioner (--caption_model topdown).

`TopDownRef` restates the captioner with torch modules whose state_dict() keys are the checkpoint's own: two nn.LSTMCell (attention and
language), the additive attention and the embeddings, written from the recurrence
    att_lstm([h_lang(i-1); fc; xt_i]) -> att_res = Attention(h_att(i)) -> lang_lstm([att_res; h_att(i)]) -> dropout(h_lang(i)) -> logit.
tests/golden/ref_topdown.npz pins it to the reference's own model.  `TopDownOracleNet` is oracle.net.OracleNet with that captioner and the
`fc_feats` input the att2in2 oracle never builds."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import net as ON
from oracle import weights as OW

CAP = 'caption_model.'
# the step-entry shapes (R, IE, AH, S) and the number of attention locations each runs with
STEP_SHAPES = [(8, 12, 8, 1), (8, 12, 8, 3), (260, 128, 64, 3), (512, 512, 512, 5)]


def rel_err(a, b):
    """tests/test_kernels_gpu.py's: max |a - b| over the reference's max magnitude"""
    a = torch.as_tensor(a).detach().double().cpu(); b = torch.as_tensor(b).detach().double().cpu()
    return float((a.reshape(-1) - b.reshape(-1)).abs().max() / (b.abs().max() + 1e-12))


ZERO_GRAD = 'attention.alpha_net.bias'


def grad_errs(got, ref):
    """{key: rel_err} of two gradient dicts.  alpha_net.bias shifts every attention score alike and the softmax does not see it: its exact
    gradient is 0 and both sides hold rounding noise (1e-9), so it is measured against the magnitude of its sibling, alpha_net.weight's
    gradient, instead of against its own."""
    out = {}
    for k, r in ref.items():
        if k.endswith(ZERO_GRAD):
            w = k[:-len('bias')] + 'weight'
            r_ = torch.as_tensor(r).detach().double().cpu(); g_ = torch.as_tensor(got[k]).detach().double().cpu()
            out[k] = float((g_.reshape(-1) - r_.reshape(-1)).abs().max() / (torch.as_tensor(ref[w]).detach().double().abs().max() + 1e-12))
        else:
            out[k] = rel_err(got[k], r)
    return out


def cosine(a, b):
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1); b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-30))


class _Attention(nn.Module):
    def __init__(self, R, AH):
        super().__init__()
        self.h2att = nn.Linear(R, AH)
        self.alpha_net = nn.Linear(AH, 1)

    def forward(self, h, att, p_att):
        """h (1,R), att (L,R), p_att (L,AH) -> (att_res (1,R), weight (1,L))"""
        dot = self.alpha_net(torch.tanh(p_att + self.h2att(h))).view(1, -1)
        w = F.softmax(dot, 1)
        return w @ att, w


class _Core(nn.Module):
    def __init__(self, IE, R, AH):
        super().__init__()
        self.att_lstm = nn.LSTMCell(IE + 2 * R, R)
        self.lang_lstm = nn.LSTMCell(2 * R, R)
        self.attention = _Attention(R, AH)

    def forward(self, xt, fc, att, p_att, state):
        (h_att, c_att), (h_lang, c_lang) = state
        h_att, c_att = self.att_lstm(torch.cat([h_lang, fc, xt], 1), (h_att, c_att))
        att_res, _ = self.attention(h_att, att, p_att)
        h_lang, c_lang = self.lang_lstm(torch.cat([att_res, h_att], 1), (h_lang, c_lang))
        return h_lang, ((h_att, c_att), (h_lang, c_lang))


class TopDownRef(nn.Module):
    """batch 1.  Dropout is never drawn here: a mask is applied where `drops` gives one ('att' (L,R), 'fc' (R,), 'xt' (S,IE), 'out' (S,R))."""

    def __init__(self, opt):
        super().__init__()
        V, IE, R, AH = opt['vocab_size'], opt['input_encoding_size'], opt['rnn_size'], opt['att_hid_size']
        p = opt.get('drop_prob_lm', 0.5)
        self.R = R
        self.embed = nn.Sequential(nn.Embedding(V + 1, IE), nn.ReLU(), nn.Dropout(p))
        self.fc_embed = nn.Sequential(nn.Linear(opt['fc_feat_size'], R), nn.ReLU(), nn.Dropout(p))
        self.att_embed = nn.Sequential(nn.Linear(opt['att_feat_size'], R), nn.ReLU(), nn.Dropout(p))
        self.logit = nn.Linear(R, V + 1)
        self.ctx2att = nn.Linear(R, AH)
        self.core = _Core(IE, R, AH)

    def forward(self, fc_feats, att_feats, seq, drops=None):
        """fc_feats (1,FC), att_feats (1,L,AF), seq (1,n) int64 starting with the 0 token -> log-probabilities (1, steps, V+1); the step
        count follows the tokens: it ends in front of the first 0 after the start token"""
        drops = drops or {}
        m = lambda x, k, i=None: x if drops.get(k) is None else x * (drops[k] if i is None else drops[k][i])
        R = self.R
        fc = m(F.relu(self.fc_embed[0](fc_feats.view(1, -1))), 'fc')
        att = m(F.relu(self.att_embed[0](att_feats.view(-1, att_feats.shape[-1]))), 'att')
        p_att = self.ctx2att(att)
        z = lambda: torch.zeros(1, R, dtype=fc.dtype)
        state = ((z(), z()), (z(), z()))
        outs = []
        self.trace = []
        for i in range(seq.shape[1] - 1):
            if i >= 1 and int(seq[0, i]) == 0:
                break
            xt = m(F.relu(self.embed[0](seq[:, i])), 'xt', i)
            h, state = self.core(xt, fc, att, p_att, state)
            self.trace.append(state)
            outs.append(F.log_softmax(self.logit(m(h, 'out', i)), 1))
        return torch.stack(outs, 1)


def nll(logp, seq, masks):
    """the masked mean of -log p(target) (LanguageModelCriterion): targets and masks are seq / masks shifted by one"""
    n = logp.shape[1]
    tgt, msk = seq[:, 1:1 + n], masks[:, 1:1 + n].to(logp.dtype)
    return (-logp.gather(2, tgt.unsqueeze(2)).squeeze(2) * msk).sum() / msk.sum()


def td_opt(**kw):
    opt = OW.default_opt(vocab_size=kw.pop('vocab_size', 60), seq_length=kw.pop('seq_length', 6))
    opt['caption_model'] = 'topdown'
    opt.update(kw)
    return opt


def cap_state(opt, seed=11):
    """{'caption_model.<torch key>': ndarray} of a seeded TopDownRef"""
    torch.manual_seed(seed)
    return {CAP + k: v.detach().numpy().copy() for k, v in TopDownRef(opt).state_dict().items()}


def make_sd(opt, seed=3, variant='cycle', head_gain=4.0, cap_seed=11):
    """oracle.weights.make_state_dict's dict with its att2in2 captioner entries replaced by a seeded TopDownRef's"""
    sd = OW.make_state_dict(opt, seed=seed, head_gain=head_gain, variant=variant)
    for k in [k for k in sd if k.startswith(CAP)]:
        del sd[k]
    sd.update(cap_state(opt, cap_seed))
    return sd


class TopDownOracleNet(ON.OracleNet):
    """oracle.net.OracleNet with the top-down captioner on the same leaf tensors.  forward_train hands `caption` the attention features only,
    so the blob and layer4's outputs on the map are stashed on the way: fc_feats = [mean | masked mean] of the map ('cycle') or [mean before
    the gating | mean after] ('cycle_response')."""

    def forward_train(self, blob, samp, drops=None):
        self._blob, self._h2t = blob, []
        return ON.OracleNet.forward_train(self, blob, samp, drops)

    def head_to_tail(self, x, drops=None):
        y = ON.OracleNet.head_to_tail(self, x, drops)
        if hasattr(self, '_h2t'):
            self._h2t.append(y)
        return y

    def fc_feats(self):
        mean = lambda f: f.mean(3).mean(2)
        if self.var['cap'] == 'mask':
            feats = self._h2t[-1]
            gm = torch.from_numpy(self._blob['gt_masks']).unsqueeze(1).float()
            gm = (F.adaptive_avg_pool2d(gm, [feats.shape[2], feats.shape[3]]) >= 0.5).float()
            return torch.cat((mean(feats), mean(feats * gm)), 1)
        feats, feats_b = self._h2t[-2], self._h2t[-1]
        return torch.cat((mean(feats_b), mean(feats)), 1)

    def caption(self, att_feats, seq, drops=None):
        """the captioner between the float32 features and the float32 log-probabilities is evaluated in float64 (the leaves stay the oracle's
        float32 tensors; the casts are differentiable).  The gradients of what enters the attention's tanh alike for every location
        (h2att.*, ctx2att.bias) are sums over the locations that cancel to 1e-7 of their terms when the features are nearly uniform - the
        softmax ignores a common shift - and a float32 autograd pass then carries an error of 3e-4 of its own in them (measured against
        float64 on the tiny cycle_response step), three times the bound it is the reference for."""
        from torch.func import functional_call
        fc = self.fc_feats()
        fc.retain_grad(); att_feats.retain_grad()
        self.t_fc, self.t_att = fc, att_feats
        mod = TopDownRef(self.opt).double()
        p = {k[len(CAP):]: v.double() for k, v in self.p.items() if k.startswith(CAP)}
        d64 = {k: v.double() for k, v in drops.items() if v is not None and k in ('att', 'fc', 'xt', 'out')} if drops else None
        return functional_call(mod, p, (fc.double(), att_feats.double(), seq, d64)).float()


# ------------------------------------------------------------------ the core alone (the step entries' reference)
def core_reference(R, IE, AH, S, L, seed, dtype=torch.float32):
    """a seeded core with random inputs and a random d(output) per step -> dict of inputs, per-step states and autograd gradients"""
    torch.manual_seed(seed)
    core = _Core(IE, R, AH).to(dtype)
    g = torch.Generator().manual_seed(seed + 1)
    rn = lambda *s: torch.randn(*s, generator=g).to(dtype)
    xt, fc, att, p_att, dout = rn(S, IE), rn(1, R), rn(L, R), rn(L, AH), rn(S, R)
    leaves = dict(xt=xt, fc=fc, att=att, p_att=p_att)
    for v in leaves.values():
        v.requires_grad_(True)
    z = lambda: torch.zeros(1, R, dtype=dtype)
    state = ((z(), z()), (z(), z()))
    tr, tot = [], 0.0
    for i in range(S):
        h, state = core(xt[i:i + 1], fc, att, p_att, state)
        tr.append(state)
        tot = tot + (h * dout[i]).sum()
    tot.backward()
    out = dict(core=core, dout=dout, **{k: v.detach() for k, v in leaves.items()})
    out['h_att'] = torch.cat([s[0][0] for s in tr]).detach(); out['c_att'] = torch.cat([s[0][1] for s in tr]).detach()
    out['h_lang'] = torch.cat([s[1][0] for s in tr]).detach(); out['c_lang'] = torch.cat([s[1][1] for s in tr]).detach()
    out['grads'] = {k: p.grad for k, p in core.named_parameters()}
    out['grads'].update({'d ' + k: v.grad for k, v in leaves.items()})
    return out


# ------------------------------------------------------------------ the entry points the captioner calls, restated in torch (CPU host-order test)
def _mat(t, rows, cols, ld=None):
    """rows x cols matrix starting at the first element of view `t` with leading dimension ld (what a raw pointer + ld means to a kernel)"""
    return torch.as_strided(t, (rows, cols), (cols if ld is None else ld, 1))


sig = torch.sigmoid


class TorchOps(object):
    """lang2seg_amd.ops entries used by nets/captioners.py TopDown (training and the decoding step), on CPU tensors: the host's order of launches,
    buffers, column blocks and keys runs without a device.  The kernels themselves are checked in tests/test_topdown_gpu.py."""
    @staticmethod
    def linear_fwd(x, w, b, y, M, N, K, act=0, accumulate=False, ldx=None, ldy=None, ldw=None):
        r = _mat(x, M, K, ldx) @ _mat(w, N, K, ldw).t() + (b.reshape(-1)[:N] if b is not None else 0)
        yv = _mat(y, M, N, ldy)
        if accumulate: r = r + yv
        yv.copy_(F.relu(r) if act == 1 else torch.tanh(r) if act == 2 else r)
    @staticmethod
    def linear_bwd_x(dy, w, dx, M, N, K, accumulate=False, lddy=None, lddx=None, mul=None, ws=None):
        r = _mat(dy, M, N, lddy) @ _mat(w, N, K)
        dv = _mat(dx, M, K, lddx)
        if accumulate: r = r + dv
        dv.copy_(r * _mat(mul, M, K, lddx) if mul is not None else r)
    @staticmethod
    def linear_bwd_x_ws_floats(M, N, K): return 0
    @staticmethod
    def linear_bwd_w(dy, x, dw, db, M, N, K, lddy=None, ldx=None):
        dyv, xv = _mat(dy, M, N, lddy), _mat(x, M, K, ldx)
        _mat(dw, N, K).add_(dyv.t() @ xv)
        if db is not None: db.view(-1)[:N].add_(dyv.sum(0))
    @staticmethod
    def act_bwd(dy, y, act):
        assert act == 1
        dy.mul_((y > 0).float())
    @staticmethod
    def embed_fwd(table, ids, mask, out, T, D, relu):
        r = table.view(-1, D)[ids]
        r = F.relu(r) if relu else r
        out.copy_(r * mask if mask is not None else r)
    @staticmethod
    def embed_bwd(dout, out, ids, mask, dtable, T, D, relu):
        g = dout * mask if mask is not None else dout.clone()
        if relu: g = g * (out != 0).float()              # the ReLU killed it (or the mask did: g is 0 already)
        dtable.view(-1, D).index_add_(0, ids, g)
    @staticmethod
    def mul(a, b, out): out.copy_(a.view(-1) .mul(b.reshape(-1)).view(out.shape))
    @staticmethod
    def cast(src, dst): dst.copy_(src)
    @staticmethod
    def memset_zero(t): t.zero_()
    @staticmethod
    def colsum(a, rows, cols, lda, out, ws=None): out.view(-1)[:cols].add_(_mat(a, rows, cols, lda).sum(0))
    @staticmethod
    def pack_rows(dst, ldd, src, lds, rows, cols):
        _mat(dst, rows, cols, ldd).copy_(_mat(src, rows, cols, lds))
    @staticmethod
    def topdown_cell_fwd(pre, add0, add1, segs, c_prev, c, h, act, R):
        g = torch.zeros(4 * R)
        for x, w, ld, n in segs:
            g = g + _mat(w, 4 * R, n, ld) @ x.reshape(-1)[:n]
        for a in (pre, add0, add1):
            if a is not None: g = g + a.reshape(-1)[:4 * R]
        i, f, gg, o = sig(g[:R]), sig(g[R:2*R]), torch.tanh(g[2*R:3*R]), sig(g[3*R:])
        cn = f * c_prev + i * gg
        c.copy_(cn); h.copy_(o * torch.tanh(cn)); act.copy_(torch.cat([i, f, gg, o]))
    @staticmethod
    def topdown_cell_bwd(segs, add0, add1, dc_in, act, c_prev, c, dgates, dc_prev, R):
        dh = torch.zeros(R)
        for v, w, ld, n in segs:
            dh = dh + _mat(w, R, n, ld) @ v.reshape(-1)[:n]
        for a in (add0, add1):
            if a is not None: dh = dh + a
        i, f, gg, o = act[:R], act[R:2*R], act[2*R:3*R], act[3*R:]
        tc = torch.tanh(c)
        dcn = (dc_in if dc_in is not None else 0) + dh * o * (1 - tc * tc)
        dgates.copy_(torch.cat([dcn*gg*i*(1-i), dcn*c_prev*f*(1-f), dcn*i*(1-gg*gg), dh*tc*o*(1-o)])); dc_prev.copy_(dcn * f)
    @staticmethod
    def cap_att_dots_fwd(patt, att_h, aw, ab, L, D, tanh_ws, dots):
        th = torch.tanh(_mat(patt, L, D) + att_h.view(1, -1)[:, :D])
        _mat(tanh_ws, L, D).copy_(th); dots.view(-1)[:L].copy_(th @ aw.view(-1)[:D] + ab.view(-1)[0])
    @staticmethod
    def cap_att_apply_fwd(att, dots, L, R, weight, att_res):
        w = F.softmax(dots.view(-1)[:L], 0)
        weight.view(-1)[:L].copy_(w); att_res.view(-1)[:R].copy_(w @ _mat(att, L, R))
    @staticmethod
    def cap_att_bwd_step_centered(dweight, tanh_ws, weight, aw, L, D, ddot, datt_h):
        w, dw = weight.view(-1)[:L], dweight.view(-1)[:L]
        dd = w * (dw - (w * dw).sum())
        t2 = _mat(tanh_ws, L, D) ** 2
        ddot.view(-1)[:L].copy_(dd); datt_h.view(-1)[:D].copy_(-aw.view(-1)[:D] * (dd.view(-1, 1) * (t2 - (w.view(-1, 1) * t2).sum(0))).sum(0))
    @staticmethod
    def cap_attention_bwd_step2(dweight, tanh_ws, weight, aw, L, D, ddot, datt_h):
        w, dw = weight.view(-1)[:L], dweight.view(-1)[:L]
        dd = w * (dw - (w * dw).sum())
        th = _mat(tanh_ws, L, D)
        ddot.view(-1)[:L].copy_(dd); datt_h.view(-1)[:D].copy_(((dd.view(-1, 1) * aw.view(1, -1)[:, :D]) * (1 - th * th)).sum(0))
    @staticmethod
    def cap_attention_bwd_batched(ddot, weight, datt_res, ldr, tanh_ws, aw, S, L, D, dpatt, datt, daw, dab):
        assert datt_res is None
        dd, th = _mat(ddot, S, L), tanh_ws.reshape(-1)[:S * L * D].view(S, L, D)
        _mat(dpatt, L, D).add_(((dd.unsqueeze(2) * aw.view(1, 1, -1)[:, :, :D]) * (1 - th * th)).sum(0))
        daw.view(-1)[:D].add_((dd.unsqueeze(2) * th).sum((0, 1))); dab.view(-1)[:1].add_(dd.sum())
    @staticmethod
    def logsoftmax_nll(logits, target, mask, S, V1, gscale, loss_slot, dlogits, logprobs=None):
        lp = F.log_softmax(_mat(logits, S, V1), 1)
        oh = F.one_hot(target, V1).float()
        loss_slot.add_(-(lp * oh).sum(1).mul(mask).sum() / mask.sum())
        _mat(dlogits, S, V1).copy_(gscale * (mask / mask.sum()).view(-1, 1) * (lp.exp() - oh))
        if logprobs is not None: _mat(logprobs, S, V1).copy_(lp)
    @staticmethod
    def mask_relu_cast(x, mul, relu_ref, out):
        if mul is not None: x.mul_(mul)
        x.mul_((relu_ref > 0).float()); out.copy_(x)
    NAMES = ('linear_fwd', 'linear_bwd_x', 'linear_bwd_x_ws_floats', 'linear_bwd_w', 'act_bwd', 'embed_fwd', 'embed_bwd', 'mul', 'cast', 'memset_zero',
             'colsum', 'pack_rows', 'topdown_cell_fwd', 'topdown_cell_bwd', 'cap_att_dots_fwd', 'cap_att_apply_fwd', 'cap_attention_bwd_step2', 'cap_att_bwd_step_centered',
             'cap_attention_bwd_batched', 'logsoftmax_nll', 'mask_relu_cast')


class TorchLinearOp(object):
    """stands in for the att_embed ConvOp (a 1x1 convolution = a row-batch Linear) in the CPU host-order test"""

    def __init__(self, P, wkey, bkey):
        self.P, self.wkey, self.bkey = P, wkey, bkey

    def fwd(self, x, M, h, w, y, relu=False, out_f32=False):
        N, K = self.P.shapes[self.wkey]
        r = x.view(M, K) @ self.P.view(self.wkey).view(N, K).t() + self.P.view(self.bkey)
        y.copy_(F.relu(r) if relu else r)

    def wgrad(self, dy, x, M, h, w):
        N, K = self.P.shapes[self.wkey]
        self.P.view(self.wkey, self.P.grad).view(N, K).add_(dy.view(M, N).t() @ x.view(M, K))
        self.P.view(self.bkey, self.P.grad).add_(dy.view(M, N).sum(0))

    def dgrad(self, dy, M, h, w, dx):
        N, K = self.P.shapes[self.wkey]
        dx.copy_(dy.view(M, N) @ self.P.view(self.wkey).view(N, K))
