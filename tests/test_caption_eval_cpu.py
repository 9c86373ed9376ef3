"""The speaker's evaluation without a device: tests/caption_eval_util.py's float64 restatement of teacher forcing with a token row per row
against torch (log_softmax + gather + the reference's criterion formula), the split totals (model/caption_eval.py CaptionTotals), the
argument errors Network.caption_score_pairs raises before any launch, the flag errors of tools/eval*.py, and the mutation checks: a
restatement with one misplaced term does not pass the comparison the device tests use."""
import os
import sys

import numpy as np
import pytest
import torch

import caption_eval_util as EU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(T=9, V1=23, seed=5):
    """5 rows with 2, 3, 7, T and 2 scored positions (n + 1), logits per step"""
    rs = np.random.RandomState(seed)
    ntok = np.asarray([2, 3, 7, T, 2])
    tokens = np.zeros((5, T - 1), np.int64)
    for r, k in enumerate(ntok):
        tokens[r, :k - 1] = rs.randint(1, V1, k - 1)
    logits = rs.normal(0, 3, (T, 5, V1))
    return tokens, ntok, logits


# ------------------------------------------------------------------ 1. the restatement against torch
def test_restatement_equals_torch_log_softmax_gather_and_the_criterion():
    tokens, ntok, logits = _batch()
    tgt, n1 = EU.targets_of(tokens)
    assert np.array_equal(n1, ntok) and (tgt[np.arange(5), ntok - 1] == 0).all()
    lps, score, toks = EU.force_rows(logits, tgt, ntok)
    x = torch.from_numpy(logits).permute(1, 0, 2)                      # [rows][T][V1], AttModel.forward's layout
    lsm = torch.log_softmax(x, dim=2)
    g = lsm.gather(2, torch.from_numpy(tgt).unsqueeze(2)).squeeze(2)
    mask = (torch.arange(tgt.shape[1])[None, :] < torch.from_numpy(ntok)[:, None]).to(torch.float64)
    assert np.abs(lps - (g * mask).numpy()).max() <= 1e-12
    assert np.abs(score - (g * mask).sum(1).numpy()).max() <= 1e-12
    crit = float((-g * mask).sum() / mask.sum())                       # lib/misc/utils.py LanguageModelCriterion
    assert abs(EU.criterion(lps, ntok) - crit) <= 1e-12 and abs(-score.sum() / ntok.sum() - crit) <= 1e-12
    # the next input: the row's own target inside its length (0 at its end token), 0 behind it
    for t in range(tgt.shape[1]):
        for r in range(5):
            assert toks[t, r] == (tgt[r, t] if t < ntok[r] else 0)
    # rows at or beyond count: nothing
    l3, s3, t3 = EU.force_rows(logits, tgt, ntok, live=3)
    assert np.array_equal(l3[:3], lps[:3]) and (l3[3:] == 0).all() and (s3[3:] == 0).all() and (t3[:, 3:] == 0).all()


def test_lengths_given_explicitly_cut_the_rows():
    tokens, ntok, logits = _batch()
    tgt, n1 = EU.targets_of(tokens, lengths=[1, 1, 3, 8, 1])
    assert n1.tolist() == [2, 2, 4, 9, 2] and (tgt[1, 1:] == 0).all() and (tgt[2, 3:] == 0).all() and tgt[2, 2] == tokens[2, 2]


# ------------------------------------------------------------------ 2. the totals
def _records():
    """three images: (per-sentence sums, their n + 1)"""
    return [([-3.5, -1.25], [4, 2]), ([-7.0], [5]), ([-0.5, -2.0, -4.75], [2, 3, 6])]


def test_totals_from_hand_made_records():
    from lang2seg_amd.model.caption_eval import CaptionTotals
    t = CaptionTotals()
    for s, k in _records():
        t.add_image(np.asarray(s, np.float32), k)
    d = t.as_dict()
    assert d['num_sent'] == 6 and d['num_tok'] == 22
    assert abs(d['loss'] - 19.0 / 22) <= 1e-15 and abs(d['perplexity'] - np.exp(19.0 / 22)) <= 1e-12
    assert abs(d['loss_per_image'] - (4.75 / 6 + 7.0 / 5 + 7.25 / 11) / 3) <= 1e-15
    assert d['exact_match'] is None
    t.add_image([-1.0], [2], exact=[1]); t.add_image([-1.0, -2.0], [2, 2], exact=[0, 1])
    assert abs(t.as_dict()['exact_match'] - 2.0 / 3) <= 1e-15


def test_two_ranks_merge_to_the_one_rank_totals():
    from lang2seg_amd.model.caption_eval import CaptionTotals
    one, a, b = CaptionTotals(), CaptionTotals(), CaptionTotals()
    for i, (s, k) in enumerate(_records()):
        one.add_image(s, k, exact=[1] * len(k))
        (a if i % 2 == 0 else b).add_image(s, k, exact=[1] * len(k))
    summed = CaptionTotals()
    summed.set_vector(a.vector() + b.vector())                        # what the float64 all_reduce leaves on every rank
    assert summed.as_dict() == one.as_dict() == CaptionTotals().merge(a.vector()).merge(b.vector()).as_dict()


def test_no_sentence_gives_no_division():
    from lang2seg_amd.model.caption_eval import CaptionTotals
    d = CaptionTotals().as_dict()
    assert d == dict(num_sent=0, num_tok=0, loss=None, perplexity=None, loss_per_image=None, exact_match=None)


def test_truncation_is_cap_labels():
    from lang2seg_amd.model.caption_eval import truncated_tokens
    assert truncated_tokens(np.asarray([[3, 4, 5, 6, 0], [7, 0, 0, 0, 0]]), 3) == [[3, 4, 5], [7]]


# ------------------------------------------------------------------ 3. argument errors before any launch
def _net(variant='cycle', cap='mask', **opt):
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    net = object.__new__(resnetv1)                                   # the argument checks come before anything touches a device
    net.variant, net.var, net.cap_model, net.training = variant, {'cap': cap}, ('att2in2' if cap else None), False
    net.opt = dict(dict(vocab_size=20, seq_length=6), **opt)
    return net


@pytest.mark.parametrize('kw,word', [
    (dict(tokens=[[3, 21, 1]]), 'tokens.*vocab_size'),                                  # above the table
    (dict(tokens=[[3, -1, 1]]), 'tokens.*vocab_size'),
    (dict(tokens=[[3, 0, 1]]), 'tokens.*vocab_size'),                                   # a zero inside the default length
    (dict(tokens=[[3, 4], [0, 0]]), 'tokens.*empty'),
    (dict(tokens=[[3, 4], [5, 6]], lengths=[2, 0]), 'empty'),
    (dict(tokens=[[3, 4], [5, 6]], lengths=[2, 3]), 'lengths.*Tmax'),
    (dict(tokens=[[3, 4], [5, 6]], lengths=[2]), 'lengths'),
    (dict(tokens=[[3, 4], [5, 6]], lengths=[1.0, 2.0]), 'lengths'),
    (dict(tokens=[3, 4]), 'tokens.*rows'),                                             # one dimension
    (dict(tokens=[[3.0, 4.0]]), 'tokens'),                                             # floats
    (dict(tokens=[[3, 4]], rows=2), 'rows'),
])
def test_caption_score_pairs_argument_errors(kw, word):
    with pytest.raises(ValueError, match='caption_score_pairs.*' + word):
        _net().caption_score_pairs(None, None, **kw)


def test_a_token_behind_the_given_length_is_not_read():
    """lengths cut a row: what lies behind them may be anything.  The call gets as far as its next check (no device here)"""
    with pytest.raises(Exception) as e:
        _net().caption_score_pairs(None, None, [[3, 99], [5, 6]], lengths=[1, 2])
    assert 'vocab_size' not in str(e.value)


def test_decode_force_rows_checks_its_buffers():
    from lang2seg_amd import ops as O
    z = lambda n, dt: torch.zeros((n,), dtype=dt)
    good = dict(logits=z(2 * 7, torch.float32), V1=7, rows=2, t=0, T=3, targets=z(6, torch.int64), lengths=z(2, torch.int32),
                logprobs=z(6, torch.float32), next_token=z(2, torch.int64))
    for k, v in (('targets', z(6, torch.int32)), ('targets', z(5, torch.int64)), ('lengths', z(2, torch.int64)), ('lengths', z(1, torch.int32)),
                 ('logprobs', z(5, torch.float32)), ('next_token', z(2, torch.int32)), ('logits', z(13, torch.float32)), ('t', 3), ('rows', 0)):
        with pytest.raises(ValueError, match='decode_force_rows'):
            O.decode_force_rows(**dict(good, **{k: v}))
    with pytest.raises(ValueError, match='decode_force_rows.*count'):
        O.decode_force_rows(count=z(1, torch.int64), **good)
    with pytest.raises(ValueError, match='decode_force_rows'):
        O.decode_force_rows(score=z(1, torch.float32), **good)


# ------------------------------------------------------------------ 4. the tools' flags
def _eval_common():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import eval_common
    finally:
        sys.path.pop(0)
    return eval_common


def test_eval_tools_take_the_flags():
    EC = _eval_common()
    a = EC.parse_args(['--synthetic', '1', '--device_eval', '1', '--caption_eval', '1', '--caption_eval_describe', '1', '--beam_size', '3',
                       '--start_from', 'caption_log_res5_2'])
    assert (a['caption_eval'], a['caption_eval_describe'], a['beam_size'], a['start_from']) == (1, 1, 3, 'caption_log_res5_2')
    assert EC.caption_eval_options(a, 'cycle') == (True, True, 3) and EC.caption_eval_options(a, 'cycle_response') == (True, True, 3)
    d = EC.parse_args(['--synthetic', '1'])
    assert d['caption_eval'] == 0 and d['caption_eval_describe'] == 0 and d['start_from'] is None
    assert EC.caption_eval_options(d, 'baseline') == (False, False, 1)


@pytest.mark.parametrize('flags,variant,words', [
    (['--caption_eval', '1'], 'cycle', '--caption_eval.*--device_eval'),
    (['--device_eval', '1', '--caption_eval_describe', '1'], 'cycle', '--caption_eval_describe.*--caption_eval'),
    (['--device_eval', '1', '--caption_eval', '1'], 'baseline', '--caption_eval.*--variant baseline'),
    (['--device_eval', '1', '--caption_eval', '1'], 'spatial', '--caption_eval.*--variant spatial'),
    (['--device_eval', '1', '--caption_eval', '1'], 'response', '--caption_eval.*--variant response'),
    (['--device_eval', '1', '--caption_eval', '1'], 'vgg', '--caption_eval.*--variant vgg'),
    (['--device_eval', '1', '--caption_eval', '1', '--beam_size', '3'], 'cycle', '--beam_size.*--describe'),
])
def test_eval_tools_flag_errors(flags, variant, words):
    EC = _eval_common()
    with pytest.raises(ValueError, match=words):
        EC.main(EC.parse_args(['--synthetic', '1', '--allow_init_weights', '1'] + flags), variant)


def test_eval_split_device_option_errors():
    from lang2seg_amd.model.eval_device import eval_split_device
    with pytest.raises(ValueError, match='caption_describe.*--caption_eval'):
        eval_split_device(None, None, None, 'val', {}, caption_describe=True)
    with pytest.raises(ValueError, match='--caption_eval.*--variant baseline'):
        eval_split_device(None, _net('baseline', None), None, 'val', {}, caption_eval=True)


def test_print_caption_eval_names_the_checkpoint_figure(capsys):
    EC = _eval_common()
    EC.print_caption_eval(dict(num_sent=6, num_tok=22, loss=0.5, perplexity=float(np.exp(0.5)), loss_per_image=0.6, exact_match=0.25),
                          dict(best_val_score=-2.5))
    out = capsys.readouterr().out
    assert 'loss 0.5000' in out and 'perplexity 1.65' in out and 'loss_per_image 0.6000' in out and 'exact match 25.00%' in out
    assert '-loss -0.5000' in out and 'best_val_score -2.5000' in out and 'its own' in out
    EC.print_caption_eval(dict(num_sent=0, num_tok=0, loss=None, perplexity=None, loss_per_image=None, exact_match=None))
    assert 'no sentence' in capsys.readouterr().out


# ------------------------------------------------------------------ 5. mutation checks
@pytest.mark.parametrize('mut', [dict(mask_shift=1), dict(mask_shift=-1), dict(target_shift=1)])
def test_a_misplaced_term_in_the_kernel_restatement_is_caught(mut):
    """the mask one position early or late, the target taken at t + 1: the comparison of the device tests raises"""
    tokens, ntok, logits = _batch()
    tgt, _ = EU.targets_of(tokens)
    lps, score, _ = EU.force_rows(logits, tgt, ntok)
    assert EU.check_close(lps.astype(np.float32), lps) <= EU.FWD_TOL      # (float32 rounding alone passes)
    bad, bad_score, _ = EU.force_rows(logits, tgt, ntok, **mut)
    with pytest.raises(AssertionError):
        EU.check_close(bad, lps)
    with pytest.raises(AssertionError):
        EU.check_close(bad_score, score, 'score')


def test_a_sum_without_the_end_token_is_caught():
    """the whole pairs scoring on stand-in drivers (a fixed table per row, indexed by the prefix length)"""
    tokens, ntok, logits = _batch()
    lsm = EU.log_softmax64(logits)
    drv = [(lambda prefix, r=r: lsm[len(prefix), r]) for r in range(5)]
    lps, score, n1 = EU.score_pairs(drv, tokens)
    tgt, _ = EU.targets_of(tokens)
    ref, ref_score, _ = EU.force_rows(logits, tgt, ntok)
    assert np.array_equal(n1, ntok) and EU.check_close(lps, ref) == 0.0 and EU.check_close(score, ref_score, 'score') <= 1e-12
    _, short, _ = EU.score_pairs(drv, tokens, drop_end=True)
    with pytest.raises(AssertionError):
        EU.check_close(short, ref_score, 'score')
