"""The speaker's evaluation inside the device evaluation (model/eval_device.py): behind every sentence's mask, the caption branch's
features under the sentence's GROUND-TRUTH mask and Network.caption_score_pairs on the sentence's own expression, cut to seq_length tokens
as the training loader's cap_labels cuts it - the held-out, dropout-off value of the loss the caption branch trains on
(AttModel.forward + LanguageModelCriterion).  With `describe`, also the captioner's own sentence for that mask (greedy, or the best of
beam_size beams, by the rows functions on one row) and whether it equals the expression token for token.

Per sentence, not per image: on both networks the features depend on the sentence's own forward.  `cycle` pools layer4 of net_conv, and
net_conv is the backbone map times the response of the sentence's dynamic filters (Network._dynfilter_fwd, NET:562), so pooling all S
ground-truth masks behind the last sentence would pool S masks on ONE sentence's map; `cycle_response` pools the map before and after its
sentence's gating.  So every sentence takes one row: caption_features_rows on its gt mask (cycle) or caption_features (cycle_response),
then a one-row caption_score_pairs.  Nothing is read back per sentence: each sentence's results are copied into one device array of the
image, which comes back once per image."""
import math

import numpy as np
import torch

f32 = torch.float32


def check_variant(net):
    """ValueError naming the variant: the speaker is evaluated where a caption branch exists (cycle, cycle_response on a ResNet)"""
    variant = getattr(net, 'variant', '?')
    var = getattr(net, 'var', None) or {}
    if variant == 'vgg' or var.get('cap') is None or not hasattr(net, 'att_embed'):
        raise ValueError('caption_eval (--caption_eval): --variant %s has no caption branch to evaluate (cycle and cycle_response have one)' % variant)


def truncated_tokens(labels, seq_length):
    """per sentence the expression's ids (its non-zero labels) cut to seq_length, as cap_labels is cut"""
    out = []
    for row in np.asarray(labels):
        toks = [int(v) for v in row if v != 0][:int(seq_length)]
        out.append(toks)
    return out


class CaptionTotals(object):
    """the split's sums in float64, fed per image with the device's per-sentence float32 sums"""
    FIELDS = ('num_sent', 'num_tok', 'sum_logprob', 'num_img', 'sum_img_loss', 'num_described', 'num_exact')

    def __init__(self):
        self.v = np.zeros((len(self.FIELDS),), np.float64)

    def add_image(self, scores, ntoks, exact=None):
        """scores: the image's per-sentence sums of log-probabilities; ntoks: their n + 1; exact: per sentence 0 / 1 (describe) or None"""
        s, k = float(np.asarray(scores, np.float64).sum()), int(np.asarray(ntoks, np.int64).sum())
        self.v[0] += len(ntoks); self.v[1] += k; self.v[2] += s
        if k > 0:
            self.v[3] += 1; self.v[4] += -s / k                      # LanguageModelCriterion on the image's batch
        if exact is not None:
            self.v[5] += len(exact); self.v[6] += int(np.sum(exact))

    def vector(self):
        return self.v.copy()

    def merge(self, vector):
        """another rank's (or the all_reduce's) sums"""
        self.v = self.v + np.asarray(vector, np.float64)
        return self

    def set_vector(self, vector):
        self.v = np.asarray(vector, np.float64).copy()

    def as_dict(self):
        n_sent, n_tok, s, n_img, s_img, n_desc, n_exact = (float(x) for x in self.v)
        loss = -s / n_tok if n_tok > 0 else None
        try:
            ppl = None if loss is None else math.exp(loss)
        except OverflowError:
            ppl = float('inf')
        return dict(num_sent=int(n_sent), num_tok=int(n_tok), loss=loss, perplexity=ppl,
                    loss_per_image=s_img / n_img if n_img > 0 else None, exact_match=n_exact / n_desc if n_desc > 0 else None)


class ImageStage(object):
    """one image's sentences: `caption` is _eval_image's hook behind sentence i's mask, `fields` the per-sentence dicts after the image's
    one read-back"""

    def __init__(self, net, labels, gt_masks, describe=False, beam_size=1, ix_to_word=None):
        from ..nets import decode
        check_variant(net)
        decode.check_args(net, 1, beam_size if describe else 1, 1.0)
        self.net, self.gm, self.describe, self.beam_size, self.ix_to_word = net, gt_masks, bool(describe), int(beam_size) if describe else 1, ix_to_word
        self.T = T = int(net.opt['seq_length'])
        self.tokens = truncated_tokens(labels, T)
        if any(not t for t in self.tokens):
            raise ValueError('caption_eval (--caption_eval): every sentence needs at least one token')
        # per sentence: T + 1 log-probabilities | their sum | (describe) T tokens | T log-probabilities
        self.out = torch.zeros((len(self.tokens), 2 + 3 * T), dtype=f32, device=torch.device(net.device))

    def caption(self, i, s, ex):
        net, T, toks = self.net, self.T, self.tokens[i]
        if net.var['cap'] == 'mask':
            m = self.gm[i]
            shape = (int(m.shape[-2]), int(m.shape[-1]))
            att, fc = net.caption_features_rows(m.reshape(1, *shape), 1, shape)
        else:
            att, fc = net.caption_features(None)
            att, fc = att.view(1, att.shape[0], att.shape[1]), None if fc is None else fc.view(1, -1)
        r = net.caption_score_pairs(att, fc, np.asarray([toks], np.int64), rows=1)
        row = self.out[i]
        row[:len(toks) + 1].copy_(r['logprobs'][0])
        row[T + 1:T + 2].copy_(r['score'])
        if self.describe:
            if self.beam_size > 1:
                d = net.caption_beam_rows(att, fc, rows=1, beam_size=self.beam_size)
            else:
                d = net.caption_decode_rows(att, fc, rows=1)
            row[T + 2:2 * T + 2].copy_(d['seq'][0])                     # (a token id is exact in float32)
            row[2 * T + 2:].copy_(d['logprobs'][0])

    def fields(self):
        """the read-back -> one dict per sentence"""
        T, h = self.T, self.out.cpu().numpy()
        out = []
        for i, toks in enumerate(self.tokens):
            n = len(toks)
            p = dict(gt_expr_logprob=float(h[i, T + 1]), gt_expr_logprobs=[float(v) for v in h[i, :n + 1]])
            if self.describe:
                seq = h[i, T + 2:2 * T + 2].astype(np.int64)
                k = int(np.argmax(seq == 0)) if (seq == 0).any() else seq.size
                p['gt_caption_tokens'] = [int(v) for v in seq[:k]]
                p['gt_caption_logprobs'] = [float(v) for v in h[i, 2 * T + 2:2 * T + 2 + k]]
                if self.ix_to_word is not None:
                    from .caption_device import decode_sequence
                    p['gt_caption'] = decode_sequence(self.ix_to_word, p['gt_caption_tokens'])
                p['gt_caption_exact'] = int(p['gt_caption_tokens'] == toks)
            out.append(p)
        return out

    def add_to(self, totals, fields):
        totals.add_image([p['gt_expr_logprob'] for p in fields], [len(p['gt_expr_logprobs']) for p in fields],
                         [p['gt_caption_exact'] for p in fields] if self.describe else None)
