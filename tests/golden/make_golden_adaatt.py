"""Generate tests/golden/ref_adaatt.npz and ref_adaattmo.npz by running the REFERENCE's own AdaAttModel / AdaAttMOModel
(lib/caption_models/AttModel.py, imported as it is, the way make_golden_topdown.py imports `caption_models`) in eval mode at tiny sizes:
weights, inputs, log-probabilities, the criterion's loss and the gradients of every parameter and of both feature inputs.

    python tests/golden/make_golden_adaatt.py <path to the reference checkout>

Only needed to regenerate the fixtures; the tests read the committed files."""
import os
import sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OPT = dict(vocab_size=20, input_encoding_size=32, rnn_size=32, num_layers=1, drop_prob_lm=0.5, seq_length=6, fc_feat_size=64, att_feat_size=64,
           att_hid_size=32, start_from=None)
L = 196


def main(ref):
    sys.path.insert(0, os.path.join(ref, 'lib'))
    import caption_models
    import misc.utils as mutils
    for model in ('adaatt', 'adaattmo'):
        torch.manual_seed(5)
        cap = caption_models.setup(dict(OPT, caption_model=model))
        cap.eval()
        rs = np.random.RandomState(17)
        fc = torch.from_numpy(rs.normal(0, 1, (1, OPT['fc_feat_size'])).astype(np.float32)).requires_grad_(True)
        att = torch.from_numpy(rs.normal(0, 1, (1, L, OPT['att_feat_size'])).astype(np.float32)).requires_grad_(True)
        seq = np.zeros((1, OPT['seq_length'] + 2), np.int64)
        seq[0, 1:6] = rs.randint(1, OPT['vocab_size'] + 1, 5)                   # five words: the loop ends at the first 0 behind them
        masks = np.zeros(seq.shape, np.float32); masks[0, :7] = 1.0
        lp = cap(fc, att, torch.from_numpy(seq))
        n = lp.shape[1]
        loss = mutils.LanguageModelCriterion()(lp, torch.from_numpy(seq)[:, 1:1 + n], torch.from_numpy(masks)[:, 1:1 + n])
        loss.backward()
        out = {'opt.' + k: np.asarray(v) for k, v in OPT.items() if isinstance(v, int)}
        out.update({'w.' + k: v.detach().numpy() for k, v in cap.state_dict().items()})
        out.update({'g.' + k: p.grad.numpy() for k, p in cap.named_parameters()})
        out.update(fc_feats=fc.detach().numpy(), att_feats=att.detach().numpy(), seq=seq, masks=masks, logprobs=lp.detach().numpy(),
                   loss=np.float32(loss.item()), g_fc_feats=fc.grad.numpy(), g_att_feats=att.grad.numpy())
        np.savez_compressed(os.path.join(HERE, 'ref_%s.npz' % model), **out)
        print('ref_%s.npz: %d steps, loss %.6f, %d parameters, alpha_net.bias grad %.1e' % (
            model, n, loss.item(), len(cap.state_dict()), float(cap.core.attention.alpha_net.bias.grad.abs().max())))


if __name__ == '__main__':
    main(sys.argv[1])
