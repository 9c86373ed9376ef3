"""Shared by tests/test_adaatt_{cpu,gpu}.py: the oracle of the adaptive-attention captioners (--caption_model adaatt | adaattmo).

`AdaAttRef` restates the captioner with torch modules whose state_dict() keys are the checkpoint's own, written from the recurrence
    sums = w2h(xt) + v2h(fc) + h2h.0(h(i-1))   (row blocks in, forget, out, transform; adaattmo: the max of two transform blocks, no tanh)
    c = f c(i-1) + in transform, h = out tanh(c), fake = sigmoid(r_w2h(xt) + r_v2h(fc) + r_h2h(h(i-1))) tanh(c)
    attention over [sentinel | 196 locations] -> tanh(att2h(.)) -> logit.
tests/golden/ref_adaatt.npz / ref_adaattmo.npz pin it to the reference's own models.  `AdaAttOracleNet` is topdown_util.TopDownOracleNet
(its fc_feats) with this captioner, evaluated in float64."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import weights as OW
from topdown_util import CAP, TopDownOracleNet, TorchOps as _TopDownOps, _mat, rel_err, grad_errs, cosine, nll   # noqa: F401

GATES = {'adaatt': 4, 'adaattmo': 5}
MASK_NAMES = ('att', 'fc', 'xt', 'out', 'toph', 'fake', 'frl', 'hol', 'hA')
# the step-entry shapes (R, L, S)
STEP_SHAPES = [(8, 10, 1), (8, 10, 3), (260, 196, 3), (512, 196, 5)]


class _Lstm(nn.Module):
    def __init__(self, IE, R, G):
        super().__init__()
        self.R, self.G = R, G
        self.w2h, self.v2h = nn.Linear(IE, G * R), nn.Linear(R, G * R)
        self.i2h = nn.ModuleList([])
        self.h2h = nn.ModuleList([nn.Linear(R, G * R)])
        self.r_w2h, self.r_v2h, self.r_h2h = nn.Linear(IE, R), nn.Linear(R, R), nn.Linear(R, R)

    def forward(self, xt, fc, h, c):
        R = self.R
        s = self.w2h(xt) + self.v2h(fc) + self.h2h[0](h)
        ig, fg, og = torch.sigmoid(s[:, :R]), torch.sigmoid(s[:, R:2 * R]), torch.sigmoid(s[:, 2 * R:3 * R])
        it = torch.tanh(s[:, 3 * R:]) if self.G == 4 else torch.max(s[:, 3 * R:4 * R], s[:, 4 * R:])
        c = fg * c + ig * it
        tc = torch.tanh(c)
        fake = torch.sigmoid(self.r_w2h(xt) + self.r_v2h(fc) + self.r_h2h(h)) * tc
        return og * tc, c, fake


class _Attention(nn.Module):
    def __init__(self, IE, R, AH):
        super().__init__()
        self.fr_linear = nn.Sequential(nn.Linear(R, IE), nn.ReLU(), nn.Dropout(0.5))
        self.fr_embed = nn.Linear(IE, AH)
        self.ho_linear = nn.Sequential(nn.Linear(R, IE), nn.Tanh(), nn.Dropout(0.5))
        self.ho_embed = nn.Linear(IE, AH)
        self.alpha_net = nn.Linear(AH, 1)
        self.att2h = nn.Linear(R, R)

    def forward(self, top_h, fake, att, p_att, m):
        """top_h / fake (1,R) after their dropout, att / p_att (L,R); m(x, name): the mask hook -> tanh(att2h(atten)) (1,R)"""
        frl = m(F.relu(self.fr_linear[0](fake)), 'frl')
        hol = m(torch.tanh(self.ho_linear[0](top_h)), 'hol')
        img = torch.cat([frl, att], 0)
        emb = torch.cat([self.fr_embed(frl), p_att], 0)
        hA = m(torch.tanh(emb + self.ho_embed(hol)), 'hA')
        PI = F.softmax(self.alpha_net(hA).view(1, -1), 1)
        return torch.tanh(self.att2h(PI @ img + hol))


class _Core(nn.Module):
    def __init__(self, IE, R, AH, G):
        super().__init__()
        self.lstm = _Lstm(IE, R, G)
        self.attention = _Attention(IE, R, AH)

    def forward(self, xt, fc, att, p_att, h, c, m):
        h, c, fake = self.lstm(xt, fc, h, c)
        return self.attention(m(h, 'toph'), m(fake, 'fake'), att, p_att, m), h, c, fake


class AdaAttRef(nn.Module):
    """batch 1.  Dropout is never drawn here: a mask is applied where `drops` gives one ('att' (L,R), 'fc' (R,), 'xt' (S,IE), 'out' / 'toph' /
    'fake' / 'frl' / 'hol' (S,R), 'hA' (S,L+1,R))."""

    def __init__(self, opt):
        super().__init__()
        V, IE, R, AH = opt['vocab_size'], opt['input_encoding_size'], opt['rnn_size'], opt['att_hid_size']
        assert IE == R == AH
        p = opt.get('drop_prob_lm', 0.5)
        self.R = R
        self.embed = nn.Sequential(nn.Embedding(V + 1, IE), nn.ReLU(), nn.Dropout(p))
        self.fc_embed = nn.Sequential(nn.Linear(opt['fc_feat_size'], R), nn.ReLU(), nn.Dropout(p))
        self.att_embed = nn.Sequential(nn.Linear(opt['att_feat_size'], R), nn.ReLU(), nn.Dropout(p))
        self.logit = nn.Linear(R, V + 1)
        self.ctx2att = nn.Linear(R, AH)
        self.core = _Core(IE, R, AH, GATES[opt['caption_model']])

    def forward(self, fc_feats, att_feats, seq, drops=None):
        """fc_feats (1,FC), att_feats (1,L,AF), seq (1,n) int64 starting with the 0 token -> log-probabilities (1, steps, V+1); the step
        count follows the tokens: it ends in front of the first 0 after the start token"""
        drops = drops or {}
        R = self.R
        mm = lambda x, k, i=None: x if drops.get(k) is None else x * (drops[k] if i is None else drops[k][i])
        fc = mm(F.relu(self.fc_embed[0](fc_feats.view(1, -1))), 'fc')
        att = mm(F.relu(self.att_embed[0](att_feats.view(-1, att_feats.shape[-1]))), 'att')
        p_att = self.ctx2att(att)
        h, c = torch.zeros(1, R, dtype=fc.dtype), torch.zeros(1, R, dtype=fc.dtype)
        outs = []
        for i in range(seq.shape[1] - 1):
            if i >= 1 and int(seq[0, i]) == 0:
                break
            xt = mm(F.relu(self.embed[0](seq[:, i])), 'xt', i)
            o, h, c, _ = self.core(xt, fc, att, p_att, h, c, lambda x, k, i=i: mm(x, k, i))
            outs.append(F.log_softmax(self.logit(mm(o, 'out', i)), 1))
        return torch.stack(outs, 1)


def ada_opt(model='adaatt', **kw):
    opt = OW.default_opt(vocab_size=kw.pop('vocab_size', 60), seq_length=kw.pop('seq_length', 6))
    opt['caption_model'], opt['adaatt'] = model, 1                              # the pair is opt-in: --adaatt 1
    opt.update(kw)
    return opt


def cap_state(opt, seed=11):
    """{'caption_model.<torch key>': ndarray} of a seeded AdaAttRef"""
    torch.manual_seed(seed)
    return {CAP + k: v.detach().numpy().copy() for k, v in AdaAttRef(opt).state_dict().items()}


def make_sd(opt, seed=3, variant='cycle', head_gain=4.0, cap_seed=11):
    """oracle.weights.make_state_dict's dict with its att2in2 captioner entries replaced by a seeded AdaAttRef's"""
    sd = OW.make_state_dict(dict(opt, caption_model='att2in2'), seed=seed, head_gain=head_gain, variant=variant)
    for k in [k for k in sd if k.startswith(CAP)]:
        del sd[k]
    sd.update(cap_state(opt, cap_seed))
    return sd


def make_masks(opt, S, L=196, seed=41):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.rand(*s, generator=g) > 0.5).float() / 0.5
    R, IE = opt['rnn_size'], opt['input_encoding_size']
    return dict(att=mk(L, R), fc=mk(R), xt=mk(S, IE), out=mk(S, R), toph=mk(S, R), fake=mk(S, R), frl=mk(S, R), hol=mk(S, R), hA=mk(S, L + 1, R))


class AdaAttOracleNet(TopDownOracleNet):
    """the oracle network with an AdaAtt captioner on the same leaf tensors; fc_feats is TopDownOracleNet's.  The captioner between the float32
    features and the float32 log-probabilities is evaluated in float64 (see TopDownOracleNet.caption for why)."""

    def caption(self, att_feats, seq, drops=None):
        from torch.func import functional_call
        fc = self.fc_feats()
        fc.retain_grad(); att_feats.retain_grad()
        self.t_fc, self.t_att = fc, att_feats
        mod = AdaAttRef(self.opt).double()
        p = {k[len(CAP):]: v.double() for k, v in self.p.items() if k.startswith(CAP)}
        d64 = {k: v.double() for k, v in drops.items() if v is not None and k in MASK_NAMES} if drops else None
        return functional_call(mod, p, (fc.double(), att_feats.double(), seq, d64)).float()


# ------------------------------------------------------------------ the core alone (the step entries' reference)
def core_reference(model, R, L, S, seed, masks=False, dtype=torch.float64):
    """a seeded core with random inputs and a random d(output) per step -> dict of inputs, per-step states and autograd gradients.  float64:
    the reference of a 1e-4 bound should not carry float32's own error"""
    torch.manual_seed(seed)
    core = _Core(R, R, R, GATES[model]).to(dtype)
    g = torch.Generator().manual_seed(seed + 1)
    rn = lambda *s: torch.randn(*s, generator=g).to(dtype)
    xt, fc, att, p_att, dout = rn(S, R), rn(1, R), rn(L, R), rn(L, R), rn(S, R)
    mk = lambda *s: ((torch.rand(*s, generator=g) > 0.5).float() / 0.5).to(dtype)
    drops = dict(toph=mk(S, R), fake=mk(S, R), frl=mk(S, R), hol=mk(S, R), hA=mk(S, L + 1, R)) if masks else {}
    leaves = dict(xt=xt, fc=fc, att=att, p_att=p_att)
    for v in leaves.values():
        v.requires_grad_(True)
    h, c = torch.zeros(1, R, dtype=dtype), torch.zeros(1, R, dtype=dtype)
    hs, cs, fakes, outs, tot = [], [], [], [], 0.0
    for i in range(S):
        o, h, c, fake = core(xt[i:i + 1], fc, att, p_att, h, c, lambda x, k, i=i: x * drops[k][i] if k in drops else x)
        hs.append(h); cs.append(c); fakes.append(fake); outs.append(o)
        tot = tot + (o * dout[i]).sum()
    tot.backward()
    out = dict(core=core, dout=dout, drops=drops, **{k: v.detach() for k, v in leaves.items()})
    out.update(h=torch.cat(hs).detach(), c=torch.cat(cs).detach(), fake=torch.cat(fakes).detach(), out=torch.cat(outs).detach())
    out['grads'] = {k: p.grad for k, p in core.named_parameters()}
    out['grads'].update({'d ' + k: v.grad for k, v in leaves.items()})
    return out


# ------------------------------------------------------------------ the new entry points restated in torch (CPU host-order test)
sig = torch.sigmoid


class TorchOps(_TopDownOps):
    """topdown_util.TorchOps + the five entries of csrc/adaatt_step.hip on CPU tensors"""
    @staticmethod
    def act_bwd(dy, y, act):
        dy.mul_((y > 0).float() if act == 1 else 1 - y * y)
    @staticmethod
    def adaatt_cell_fwd(pre, fcrow, w_hh, b_hh, w_r, b_r, h_prev, c_prev, c, h, fake, save, R, G, ld_hh=None, ld_r=None):
        W = (G + 1) * R
        s = pre.reshape(-1)[:W] + fcrow.reshape(-1)[:W]
        s = s + torch.cat([_mat(w_hh, G * R, R, ld_hh) @ h_prev + b_hh.reshape(-1)[:G * R], _mat(w_r, R, R, ld_r) @ h_prev + b_r.reshape(-1)[:R]])
        ig, fg, og = sig(s[:R]), sig(s[R:2 * R]), sig(s[2 * R:3 * R])
        if G == 5:
            it, sel = torch.max(s[3 * R:4 * R], s[4 * R:5 * R]), (s[3 * R:4 * R] < s[4 * R:5 * R]).float()
        else:
            it, sel = torch.tanh(s[3 * R:4 * R]), torch.zeros(R)
        cn = fg * c_prev + ig * it
        tc, sg = torch.tanh(cn), sig(s[G * R:])
        c.copy_(cn); h.copy_(og * tc); fake.copy_(sg * tc); save.copy_(torch.cat([ig, fg, og, it, sel, tc, sg]))
    @staticmethod
    def adaatt_cell_bwd(dsn, t_hh, t_r, dh_ext, dfake, dc_in, save, c_prev, ds, dc_prev, R, G, ld_thh=None, ld_tr=None):
        dh = dh_ext.clone() if dh_ext is not None else torch.zeros(R)
        if dsn is not None:
            dh = dh + _mat(t_hh, R, G * R, ld_thh) @ dsn.reshape(-1)[:G * R] + _mat(t_r, R, R, ld_tr) @ dsn.reshape(-1)[G * R:(G + 1) * R]
        ig, fg, og, it, sel, tc, sg = save.view(7, R)
        df = dfake if dfake is not None else torch.zeros(R)
        dcn = (dc_in if dc_in is not None else 0) + (og * dh + sg * df) * (1 - tc * tc)
        dit = dcn * ig
        tr = [dit * (1 - sel), dit * sel] if G == 5 else [dit * (1 - it * it)]
        ds.copy_(torch.cat([dcn * it * ig * (1 - ig), dcn * c_prev * fg * (1 - fg), dh * tc * og * (1 - og)] + tr + [df * tc * sg * (1 - sg)]))
        dc_prev.copy_(dcn * fg)
    @staticmethod
    def adaatt_att_fwd(att, patt, frl, fre, hoe, hol, aw, ab, mask, S, L, R, tanh_ws, dots, PI, atten):
        for s in range(S):
            th = torch.tanh(torch.cat([fre[s:s + 1], _mat(patt, L, R)], 0) + hoe[s:s + 1])
            tanh_ws[s].copy_(th)
            sc = (th * mask[s] if mask is not None else th) @ aw.view(-1)[:R] + ab.view(-1)[0]
            dots[s, :L + 1].copy_(sc)
            w = F.softmax(sc, 0)
            PI[s].copy_(w); atten[s].copy_(w @ torch.cat([frl[s:s + 1], _mat(att, L, R)], 0) + hol[s])
    @staticmethod
    def adaatt_att_bwd_step(datten, att, frl, tanh_ws, mask, PI, aw, S, L, R, ddot, dhoe, dfre, dctx, dfrl, dhol):
        for s in range(S):
            w = PI[s]
            dw = torch.cat([frl[s:s + 1], _mat(att, L, R)], 0) @ datten[s]
            dd = w * (dw - (w * dw).sum())
            u = 1 - tanh_ws[s] ** 2
            if mask is not None: u = u * mask[s]
            g = dd.view(-1, 1) * aw.view(1, -1)[:, :R] * u
            ddot[s].copy_(dd); dhoe[s].copy_(g.sum(0)); dfre[s].copy_(g[0]); dctx[s].copy_(g[1:].sum(0))
            dfrl[s].copy_(w[0] * datten[s]); dhol[s].copy_(datten[s])
    @staticmethod
    def adaatt_att_bwd_batched(ddot, PI, datten, tanh_ws, mask, aw, S, L, R, dpatt, datt, daw):
        dd = ddot.unsqueeze(2) * (mask if mask is not None else 1)
        _mat(dpatt, L, R).add_((dd * aw.view(1, 1, -1)[:, :, :R] * (1 - tanh_ws ** 2)).sum(0)[1:])
        _mat(datt, L, R).add_(PI[:, 1:].t() @ datten)
        daw.view(-1)[:R].add_((dd * tanh_ws).sum((0, 1)))
    NAMES = _TopDownOps.NAMES + ('adaatt_cell_fwd', 'adaatt_cell_bwd', 'adaatt_att_fwd', 'adaatt_att_bwd_step', 'adaatt_att_bwd_batched')
