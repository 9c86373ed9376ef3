"""Generate tests/golden/ref_decode.npz by running the REFERENCE's own decoding - AttModel.sample (greedy) and sample_beam / beam_search
(beam_size 3) of Att2in2Model, TopDownModel, AdaAttModel and AdaAttMOModel, imported as they are the way make_golden_topdown.py imports
`caption_models` - in eval mode at tiny sizes: per captioner the weights, both feature inputs, the greedy sequence with its
log-probabilities, done_beams (seq, logps, p) and the margins of every decision.

    python tests/golden/make_golden_decode.py <path to the reference checkout>

`sample` and `beam_search` call .cuda() unconditionally; Tensor.cuda is the identity here.  The weights are the seeded initialisers times 3
(weights are data): at the initialisers' scale every distribution is nearly flat and no captioner ever ends a sentence.  The top-down
captioner's are times 10 with logit.bias[0] raised by 2: only with peaked distributions does a longer sentence ever beat a shorter one that
completed before it, which is what (d) asks for.  Seeds are searched
until the conditions asserted at the end hold: (a) one greedy sentence ends early and one runs to seq_length, (b) every greedy decision has
a top-two gap > 1e-3, (c) every beam step's best beam_size + 1 candidates are > 1e-3 apart, (d) in one beam case the completion with the best
joint log-probability is not the first completed, so that the two ordering rules (tests/decode_util.py legacy_p_alias) differ.

Only needed to regenerate the fixture; the tests read the committed file."""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import decode_util as DU  # noqa: E402

BASE = dict(vocab_size=20, rnn_size=32, num_layers=1, drop_prob_lm=0.5, seq_length=6, fc_feat_size=64, att_feat_size=64, start_from=None)
SIZES = {'att2in2': dict(input_encoding_size=12, att_hid_size=16), 'topdown': dict(input_encoding_size=12, att_hid_size=16),
         'adaatt': dict(input_encoding_size=32, att_hid_size=32), 'adaattmo': dict(input_encoding_size=32, att_hid_size=32)}
L, B, MARGIN = 196, 3, 1e-3
SCALE, BIAS0 = {'topdown': 10.0}, {'topdown': 2.0}                # the others: 3.0 and 0.0


def run(caption_models, model, seed):
    opt = dict(BASE, caption_model=model, **SIZES[model])
    torch.manual_seed(seed)
    cap = caption_models.setup(dict(opt))
    cap.eval()
    with torch.no_grad():
        for p in cap.parameters():
            p.mul_(SCALE.get(model, 3.0))
        cap.logit.bias[0] += BIAS0.get(model, 0.0)                             # the end token more likely: beams that complete at different steps
    rs = np.random.RandomState(100 + seed)
    fc = torch.from_numpy(rs.normal(0, 1, (1, opt['fc_feat_size'])).astype(np.float32))
    att = torch.from_numpy(rs.normal(0, 1, (1, L, opt['att_feat_size'])).astype(np.float32))
    T = opt['seq_length']
    with torch.no_grad():
        seq, lps = cap.sample(fc, att, {'sample_max': 1, 'beam_size': 1})
        gseq = [] if isinstance(seq, list) else [int(v) for v in seq[0]]
        glp = [] if isinstance(seq, list) else [float(v) for v in lps[0]]
        cap.sample(fc, att, {'beam_size': B})
        done = cap.done_beams[0]

        def next_logprobs(prefix):
            """the reference's own get_logprobs_state from <bos> along the prefix"""
            f = cap.fc_embed(fc) if hasattr(cap, 'fc_embed') else fc
            a = cap.att_embed(att.view(-1, opt['att_feat_size'])).view(1, L, -1)
            pa = cap.ctx2att(a.view(-1, opt['rnn_size'])).view(1, L, -1)
            state = cap.init_hidden(1)
            for w in (0,) + tuple(prefix):
                lp, state = cap.get_logprobs_state(torch.tensor([w], dtype=torch.int64), f, a, pa, state)
            return lp[0].numpy()
        rseq, rlp, gm = DU.sample(next_logprobs, T)
        alias, _, gaps = DU.beam_search(next_logprobs, T, B, legacy_p_alias=True)
        intended, every, _ = DU.beam_search(next_logprobs, T, B, legacy_p_alias=False)
    # the restatement is the reference: the fixture's margins are computed by it
    assert rseq == gseq[:len(rseq)] and len(gseq) == len(rseq) and np.allclose(rlp, glp, atol=1e-6), (model, seed, rseq, gseq)
    assert len(done) == len(alias) == B
    for a, b in zip(done, alias):
        assert [int(v) for v in a['seq']] == [int(v) for v in b['seq']] and np.allclose(a['logps'].numpy(), b['logps'], atol=1e-6), (model, seed)
    out = {'opt.' + k: np.asarray(v) for k, v in opt.items() if isinstance(v, int)}
    out.update({'w.' + k: v.detach().numpy() for k, v in cap.state_dict().items()})
    out.update(fc_feats=fc.numpy(), att_feats=att.numpy(), greedy_seq=np.asarray(gseq, np.int64), greedy_logprobs=np.asarray(glp, np.float32),
               greedy_margin=np.float32(min(gm)), beam_margin=np.float32(min(gaps)), beam_size=np.asarray(B),
               beam_seq=np.stack([d['seq'].numpy() for d in done]), beam_logps=np.stack([d['logps'].numpy() for d in done]),
               beam_p=np.asarray([float(d['p']) for d in done], np.float32), seed=np.asarray(seed))
    best_first = max(range(len(every)), key=lambda i: float(every[i]['p'])) == 0
    info = dict(greedy_len=len(gseq), greedy_margin=min(gm), beam_margin=min(gaps), orders_differ=not best_first,
                same_sets=sorted(d['index'] for d in intended) == sorted(d['index'] for d in alias))
    return out, info


def main(ref):
    sys.path.insert(0, os.path.join(ref, 'lib'))
    torch.Tensor.cuda = lambda self, *a, **k: self              # sample / beam_search call .cuda() unconditionally
    import caption_models
    T = BASE['seq_length']
    out, infos = {'torch_version': np.asarray(torch.__version__)}, {}
    for model in SIZES:
        want_early = model == 'adaatt'                          # (a): this one ends early, att2in2 runs to seq_length
        for seed in range(1, 200):
            o, info = run(caption_models, model, seed)
            ok = info['greedy_margin'] > MARGIN and info['beam_margin'] > MARGIN
            if want_early:
                ok = ok and 1 <= info['greedy_len'] < T
            if model == 'att2in2':
                ok = ok and info['greedy_len'] == T
            if model == 'topdown':
                ok = ok and info['orders_differ'] and not info['same_sets']              # (d), and the kept sets differ too
            if ok:
                break
        else:
            raise SystemExit('no seed for %s' % model)
        print('%-9s seed %3d: %s' % (model, seed, info))
        infos[model] = info
        out.update({model + '/' + k: v for k, v in o.items()})
    assert any(1 <= i['greedy_len'] < T for i in infos.values()) and any(i['greedy_len'] == T for i in infos.values())        # (a)
    assert all(i['greedy_margin'] > MARGIN and i['beam_margin'] > MARGIN for i in infos.values())                              # (b), (c)
    assert any(i['orders_differ'] for i in infos.values())                                                                     # (d)
    np.savez_compressed(os.path.join(HERE, 'ref_decode.npz'), **out)
    print('ref_decode.npz written, torch', torch.__version__)


if __name__ == '__main__':
    main(sys.argv[1])
