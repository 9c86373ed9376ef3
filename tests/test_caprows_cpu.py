"""The numpy restatement of the caption branch on rows (tests/caprows_util.py) held against the reference: the batched greedy loop and the
teacher-forced score against the reference's own batch runs (tests/golden/ref_caprows.npz: AttModel.sample and AttModel.forward on 5
rows), the masks at the map's size and the pooled rows against torch's adaptive_avg_pool2d, the rule the reference pools by.

Tokens exact; log-probabilities within 1e-6 absolute, the bound make_golden_decode.py holds its own restatement to."""
import numpy as np
import pytest
import torch

import caprows_util as CU

TOL = 1e-6


@pytest.mark.parametrize('model', CU.MODELS)
def test_fixture_is_what_the_tests_need(model):
    """(a) one row ends before seq_length and one runs to it, (b) three different sentences, (c) the recorded margin"""
    opt, w, fc, att, g = CU.fixture(model)
    T = opt['seq_length']
    seq = g['greedy_seq']
    assert seq.shape == (5, T) and att.shape == (5, 196, opt['att_feat_size']) and fc.shape == (5, opt['fc_feat_size'])
    lens = [int(np.argmax(s == 0)) if (s == 0).any() else T for s in seq]
    assert min(lens) < T and max(lens) == T
    assert len({tuple(int(v) for v in s) for s in seq}) >= 3
    assert float(g['greedy_margin']) > 1e-3
    assert g['forward_logprobs'].shape == (5, 5, opt['vocab_size'] + 1) and [int(v) for v in g['forced']] == [0, 3, 7, 1, 12, 0]


@pytest.mark.parametrize('model', CU.MODELS)
def test_batched_greedy_loop_equals_the_references_batch(model):
    opt, w, fc, att, g = CU.fixture(model)
    T = opt['seq_length']
    seq, lps, gap = CU.greedy_rows(CU.drivers(model), T)
    assert np.array_equal(seq, g['greedy_seq'])
    assert gap > 1e-3
    worst = 0.0
    for r in range(5):
        n = int(np.argmax(seq[r] == 0)) if (seq[r] == 0).any() else T
        worst = max(worst, float(np.abs(lps[r, :n] - g['greedy_logprobs'][r, :n]).max(initial=0.0)))
        assert (lps[r, n + 1:] == 0).all() and (n == T or lps[r, n] < 0)          # the 0 carries its log-probability, nothing behind it
    print('%s batched greedy restated vs sample(): %.2e' % (model, worst))
    assert worst <= TOL


@pytest.mark.parametrize('model', CU.MODELS)
def test_teacher_forced_score_equals_the_references_forward(model):
    opt, w, fc, att, g = CU.fixture(model)
    forced = [int(v) for v in g['forced']]
    toks, tgt = forced[1:-1], forced[1:]
    lps, score = CU.score_rows(CU.drivers(model), toks)
    ref = g['forward_logprobs'][:, np.arange(len(tgt)), tgt]
    worst = float(np.abs(lps - ref).max())
    print('%s teacher-forced restated vs forward(): %.2e' % (model, worst))
    assert lps.shape == (5, len(toks) + 1) and worst <= TOL
    assert np.abs(score - ref.astype(np.float64).sum(1)).max() <= TOL * 10       # five float32 additions of values near 3


@pytest.mark.parametrize('shape', [(37, 53, 160, 224, 10, 14), (160, 224, 160, 224, 10, 14), (50, 70, 600, 1000, 38, 63)])
def test_masks_to_map_is_nearest_then_adaptive_average(shape):
    from oracle import boxes as OB
    mh, mw, H, W, Hc, Wc = shape
    rs = np.random.RandomState(mh)
    masks = (rs.rand(3, mh, mw) > 0.5).astype(np.uint8)
    masks[1, :mh // 2] = 1
    got = CU.masks_to_map(masks, H, W, Hc, Wc)
    big = np.stack([OB.imresize_nearest_u8(m, (H, W)) for m in masks])
    avg = torch.nn.functional.adaptive_avg_pool2d(torch.from_numpy(big.astype(np.float64))[:, None], (Hc, Wc))[:, 0].numpy()
    assert np.array_equal(got.reshape(3, Hc, Wc), (avg >= 0.5).astype(np.float32))
    assert 0 < got.sum() < got.size


@pytest.mark.parametrize('shape', [(10, 14, 14, 14), (38, 63, 14, 14), (10, 14, 1, 1)])
def test_pooled_rows_are_adaptive_average_pooling(shape):
    H, W, OH, OW = shape
    rs = np.random.RandomState(H)
    x = rs.normal(0, 1, (H * W, 7))
    pm = (rs.rand(3, H * W) > 0.4).astype(np.float32)
    for m in (None, pm):
        got = CU.adaptive_pool_rows(x, m, 3, H, W, OH, OW)
        for r in range(3):
            v = x if m is None else x * m[r][:, None]
            ref = torch.nn.functional.adaptive_avg_pool2d(torch.from_numpy(v.reshape(H, W, 7)).permute(2, 0, 1)[None], (OH, OW))[0]
            assert np.abs(got[r] - ref.permute(1, 2, 0).reshape(OH * OW, 7).numpy()).max() < 1e-12
