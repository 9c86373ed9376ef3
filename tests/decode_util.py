"""Shared by tests/test_decode_{cpu,gpu}.py and tests/golden/make_golden_decode.py: caption decoding restated in numpy.

`sample`, `beam_step` and `beam_search` restate AttModel.sample (AttModel.py:151-209) and CaptionModel.beam_search (CaptionModel.py:23-124)
for one image, driven by `next_logprobs(prefix)`: the float32 log-probabilities [V1] of the word that follows <bos> + prefix.  A beam's
recurrent state is a function of its prefix, so nothing is shuffled here: every beam asks for its own prefix.

`legacy_p_alias`: under a current torch `final_beam['p'] = beam_logprobs_sum[vix]` (:113) is a VIEW of the tensor whose element the next
line sets to -1000, so every completed beam carries p = -1000, the final sort (:123) keeps the completion order, and done_beams is the
first beam_size completions.  Under the torch the reference was written for (0.3) indexing a 1-D tensor gave a Python float and the sort
is by joint log-probability; that is the rule the product implements (legacy_p_alias=False).

`RefDriver` builds next_logprobs on the captioner restatements of the other suites (topdown_util.TopDownRef, adaatt_util.AdaAttRef, the
att2in2 captioner of oracle.net.OracleNet), unchanged: they stop at a 0 token, and a completed beam goes on with 0 as its input, so the
restatement runs on a vocabulary with one more word, a copy of word 0 (same embedding row; a logit of -1e30, which adds exactly 0 to the
softmax's sum), and interior zeros of a prefix are sent as that word."""
import os

import numpy as np
import torch

CAP = 'caption_model.'
f32 = np.float32


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def sample(next_logprobs, T, sample_max=1, temperature=1.0, u=None):
    """-> (seq, logprobs, per-step margins): tokens until the first 0 (not included), at most T.  Sampled: inverse CDF in index order with
    u[t], float64 accumulation (the kernel's rule up to rounding; the GPU test brackets the draw instead of comparing with this)."""
    seq, lps, margins = [], [], []
    for t in range(T):
        lp = np.asarray(next_logprobs(tuple(seq)), dtype=f32)
        if sample_max:
            k = int(np.argmax(lp))
            s = np.sort(lp)[::-1]
            margins.append(float(s[0] - s[1]))
        else:
            p = np.exp(lp.astype(np.float64) / temperature)
            cdf = np.cumsum(p)
            k = int(min(np.searchsorted(cdf, u[t] * cdf[-1], side='right'), lp.size - 1))
        if k == 0:
            break
        seq.append(k); lps.append(float(lp[k]))
    return seq, lps, margins


def beam_step(lp, B, t, beam_seq, beam_seq_logprobs, beam_logprobs_sum):
    """CaptionModel.py:27-75 on lp float32 [B][V1] (the -1000 of :93 already applied), tables updated in place -> (parents, candidates)"""
    lp = np.asarray(lp, dtype=f32)
    ix = np.argsort(-lp, axis=1, kind='stable')
    ys = np.take_along_axis(lp, ix, 1)
    cols, rows = min(B, lp.shape[1]), (1 if t == 0 else B)
    cand = []
    for c in range(cols):
        for q in range(rows):
            r = ys[q, c]
            cand.append(dict(c=int(ix[q, c]), q=q, p=f32(beam_logprobs_sum[q] + r), r=r))
    cand = sorted(cand, key=lambda x: -x['p'])
    prev_seq, prev_lp = beam_seq[:t].copy(), beam_seq_logprobs[:t].copy()
    parents = []
    for vix in range(B):
        v = cand[vix]
        if t >= 1:
            beam_seq[:t, vix] = prev_seq[:, v['q']]
            beam_seq_logprobs[:t, vix] = prev_lp[:, v['q']]
        beam_seq[t, vix] = v['c']
        beam_seq_logprobs[t, vix] = v['r']
        beam_logprobs_sum[vix] = v['p']
        parents.append(v['q'])
    return parents, cand


def completions(t, T, B, beam_seq, beam_seq_logprobs, beam_logprobs_sum, done, legacy_p_alias=False):
    """the completion loop, CaptionModel.py:107-117"""
    for vix in range(B):
        if beam_seq[t, vix] == 0 or t == T - 1:
            done.append(dict(seq=beam_seq[:, vix].copy(), logps=beam_seq_logprobs[:, vix].copy(),
                             p=f32(-1000.0) if legacy_p_alias else f32(beam_logprobs_sum[vix]), index=len(done)))
            beam_logprobs_sum[vix] = -1000.0


def beam_search(next_logprobs, T, B, legacy_p_alias=False):
    """-> (done_beams: the best B completions, all completions, per-step gaps between consecutive candidates among the best B + 1)"""
    beam_seq, beam_lp, beam_sum = np.zeros((T, B), np.int64), np.zeros((T, B), f32), np.zeros((B,), f32)
    done, gaps = [], []
    for t in range(T):
        lp = np.stack([np.asarray(next_logprobs(tuple(int(w) for w in beam_seq[:t, b])), dtype=f32) for b in range(B)]).copy()
        lp[:, -1] -= f32(1000.0)
        _, cand = beam_step(lp, B, t, beam_seq, beam_lp, beam_sum)
        ps = [float(c['p']) for c in cand[:B + 1]]
        gaps.append(min(a - b for a, b in zip(ps, ps[1:])) if len(ps) > 1 else float('inf'))
        completions(t, T, B, beam_seq, beam_lp, beam_sum, done, legacy_p_alias)
    return sorted(done, key=lambda x: -x['p'])[:B], done, gaps


# ------------------------------------------------------------------ next_logprobs on the suites' restatements
def _pad_vocab(w):
    """the captioner's weights on a vocabulary with one more word: a copy of word 0 that is never predicted"""
    w = {k: torch.as_tensor(np.asarray(v)).clone() for k, v in w.items()}
    w['embed.0.weight'] = torch.cat([w['embed.0.weight'], w['embed.0.weight'][:1]], 0)
    w['logit.weight'] = torch.cat([w['logit.weight'], torch.zeros_like(w['logit.weight'][:1])], 0)
    w['logit.bias'] = torch.cat([w['logit.bias'], torch.full((1,), -1e30)], 0)
    return w


class RefDriver(object):
    """next_logprobs(prefix) of one captioner: model in ('att2in2', 'topdown', 'adaatt', 'adaattmo'), opt: its sizes, weights: {torch key
    below caption_model.: array}, fc_feats [FC] (None for att2in2), att_feats [196][AF]"""

    def __init__(self, model, opt, weights, fc_feats, att_feats):
        self.V1 = opt['vocab_size'] + 1
        opt = dict(opt, vocab_size=opt['vocab_size'] + 1, caption_model=model)
        w = _pad_vocab(weights)
        self.att = torch.as_tensor(np.asarray(att_feats), dtype=torch.float32).view(1, 196, -1)
        self.fc = None if fc_feats is None else torch.as_tensor(np.asarray(fc_feats), dtype=torch.float32).view(1, -1)
        if model == 'att2in2':
            from oracle import net as ON
            o = object.__new__(ON.OracleNet)                    # its captioner reads only these two
            o.opt, o.p = opt, {CAP + k: v for k, v in w.items()}
            self.fwd = lambda seq: o.caption(self.att, seq)
        else:
            if model == 'topdown':
                from topdown_util import TopDownRef as Ref
            else:
                from adaatt_util import AdaAttRef as Ref
            mod = Ref(opt)
            mod.load_state_dict(w, strict=True)
            mod.eval()
            self.fwd = lambda seq: mod(self.fc, self.att, seq)
        self.cache = {}

    def __call__(self, prefix):
        prefix = tuple(int(v) for v in prefix)
        if prefix not in self.cache:
            seq = torch.tensor([[0] + [self.V1 if v == 0 else v for v in prefix] + [1]], dtype=torch.int64)
            with torch.no_grad():
                lp = self.fwd(seq)
            assert lp.shape[1] == len(prefix) + 1
            self.cache[prefix] = lp[0, -1, :self.V1].numpy().astype(f32)
        return self.cache[prefix]


# ------------------------------------------------------------------ the reference fixture
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'ref_decode.npz')
MODELS = ('att2in2', 'topdown', 'adaatt', 'adaattmo')
_Z = {}


def fixture(model):
    """-> (opt, weights, fc_feats or None, att_feats, the recorded results) of one captioner"""
    if 'z' not in _Z:
        _Z['z'] = np.load(GOLD)
    z = _Z['z']
    g = {k[len(model) + 1:]: z[k] for k in z.files if k.startswith(model + '/')}
    opt = {k[4:]: int(v) for k, v in g.items() if k.startswith('opt.')}
    w = {k[2:]: v for k, v in g.items() if k.startswith('w.')}
    return opt, w, (None if model == 'att2in2' else g['fc_feats'][0]), g['att_feats'][0], g


def driver(model):
    if ('drv', model) not in _Z:
        opt, w, fc, att, _ = fixture(model)
        _Z[('drv', model)] = RefDriver(model, opt, w, fc, att)
    return _Z[('drv', model)]
