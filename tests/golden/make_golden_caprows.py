"""Generate tests/golden/ref_caprows.npz by running the REFERENCE's captioners on a BATCH of rows - AttModel.sample (greedy) and
AttModel.forward of Att2in2Model and TopDownModel, imported as they are the way make_golden_decode.py imports `caption_models` - in eval
mode at the sizes of ref_decode.npz, on 5 rows of att_feats [5][196][64] / fc_feats [5][64]: per captioner the weights, the features, the
batch's greedy sequences [5][6] with their log-probabilities, and forward(fc, att, [[0, 3, 7, 1, 12, 0]] * 5) as [5][5][21].

    python tests/golden/make_golden_caprows.py <path to the reference checkout>

`sample` calls .cuda() unconditionally; Tensor.cuda is the identity here.  The weights are the seeded initialisers times 3 with
logit.bias[0] raised by 1 (weights are data).  sample() zeroes a finished row's tokens but goes on recording the log-probability of the
argmax it would have fed, and leaves out the step at which the last rows end: the stored log-probabilities are the reference's in front of
every row's first 0 and 0 from there on.  Seeds are searched until the conditions asserted hold: (a) one row ends before seq_length and one runs to it, (b) at
least three different sentences, (c) every greedy decision of an unfinished row has a top-two gap > 1e-3; and the batch equals the rows
run one by one (by the reference and by the restatement of tests/decode_util.py).

Only needed to regenerate the fixture; the tests read the committed file."""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import decode_util as DU  # noqa: E402

BASE = dict(vocab_size=20, rnn_size=32, num_layers=1, drop_prob_lm=0.5, seq_length=6, fc_feat_size=64, att_feat_size=64, start_from=None,
            input_encoding_size=12, att_hid_size=16)
MODELS = ('att2in2', 'topdown')
L, N, MARGIN = 196, 5, 1e-3
FORCED = [0, 3, 7, 1, 12, 0]


def padded(seq, lps, T):
    """sample()'s outputs as [N][T]: zeros from the step at which every row had finished, log-probabilities cut at a row's first 0"""
    s, p = np.zeros((N, T), np.int64), np.zeros((N, T), np.float32)
    if not isinstance(seq, list):
        s[:, :seq.shape[1]] = seq.numpy()
        p[:, :lps.shape[1]] = lps.numpy()
    for r in range(N):
        z = np.nonzero(s[r] == 0)[0]
        if z.size:
            p[r, z[0]:] = 0.0
    return s, p


def run(caption_models, model, seed):
    opt = dict(BASE, caption_model=model)
    torch.manual_seed(seed)
    cap = caption_models.setup(dict(opt))
    cap.eval()
    with torch.no_grad():
        for p in cap.parameters():
            p.mul_(3.0)
        cap.logit.bias[0] += 1.0
    rs = np.random.RandomState(100 + seed)
    fc = torch.from_numpy(rs.normal(0, 1, (N, opt['fc_feat_size'])).astype(np.float32))
    att = torch.from_numpy(rs.normal(0, 1, (N, L, opt['att_feat_size'])).astype(np.float32))
    T = opt['seq_length']
    forced = torch.tensor([FORCED] * N, dtype=torch.int64)
    with torch.no_grad():
        seq, lps = padded(*cap.sample(fc, att, {'sample_max': 1, 'beam_size': 1}), T=T)
        fwd = cap(fc, att, forced).numpy()
        assert fwd.shape == (N, len(FORCED) - 1, opt['vocab_size'] + 1), fwd.shape
        margins, lens, same = [], [], True
        for r in range(N):
            # the batch equals the row alone, by the reference ...
            s1, p1 = padded(*cap.sample(fc[r:r + 1].repeat(N, 1), att[r:r + 1].repeat(N, 1, 1), {'sample_max': 1, 'beam_size': 1}), T=T)
            same = same and bool((s1[0] == seq[r]).all() and np.allclose(p1[0], lps[r], atol=1e-6))
            f1 = cap(fc[r:r + 1], att[r:r + 1], forced[:1]).numpy()
            same = same and bool(np.allclose(f1[0], fwd[r], atol=1e-6))
            # ... and by the restatement, whose margins the fixture records
            drv = DU.RefDriver(model, {k: v for k, v in opt.items() if isinstance(v, int)}, {k: v.detach().numpy() for k, v in cap.state_dict().items()},
                               None if model == 'att2in2' else fc[r].numpy(), att[r].numpy())
            rseq, rlp, gm = DU.sample(drv, T)
            n = len(rseq)
            same = same and rseq == [int(v) for v in seq[r, :n]] and (n == T or seq[r, n] == 0) and bool(np.allclose(rlp, lps[r, :n], atol=1e-6))
            margins.append(min(gm)); lens.append(n)
    out = {'opt.' + k: np.asarray(v) for k, v in opt.items() if isinstance(v, int)}
    out.update({'w.' + k: v.detach().numpy() for k, v in cap.state_dict().items()})
    out.update(fc_feats=fc.numpy(), att_feats=att.numpy(), greedy_seq=seq, greedy_logprobs=lps, greedy_margin=np.float32(min(margins)),
               forced=np.asarray(FORCED, np.int64), forward_logprobs=fwd.astype(np.float32), seed=np.asarray(seed))
    info = dict(lens=lens, margin=min(margins), same=same, sentences=len({tuple(int(v) for v in s) for s in seq}))
    return out, info


def main(ref):
    sys.path.insert(0, os.path.join(ref, 'lib'))
    torch.Tensor.cuda = lambda self, *a, **k: self              # sample calls .cuda() unconditionally
    import caption_models
    T = BASE['seq_length']
    out = {'torch_version': np.asarray(torch.__version__)}
    for model in MODELS:
        for seed in range(1, 400):
            o, info = run(caption_models, model, seed)
            if min(info['lens']) < T and max(info['lens']) == T and info['sentences'] >= 3 and info['margin'] > MARGIN:      # (a), (b), (c)
                break
        else:
            raise SystemExit('no seed for %s' % model)
        print('%-9s seed %3d: %s' % (model, seed, info))
        assert min(info['lens']) < T and max(info['lens']) == T and info['sentences'] >= 3 and info['margin'] > MARGIN
        assert info['same'], (model, seed)          # a decision above the margin is the same in the batch, alone and restated
        out.update({model + '/' + k: v for k, v in o.items()})
    np.savez_compressed(os.path.join(HERE, 'ref_caprows.npz'), **out)
    print('ref_caprows.npz written, torch', torch.__version__)


if __name__ == '__main__':
    main(sys.argv[1])
