"""Caption decoding without a device: the numpy restatement of AttModel.sample / CaptionModel.beam_search (tests/decode_util.py) against
tests/golden/ref_decode.npz - the reference's own greedy and beam-search runs of all four captioners - and the argument errors of
Network.caption_decode.  tests/test_decode_gpu.py then holds the device path to the restatement."""
import numpy as np
import pytest

import decode_util as DU

from decode_util import fixture, driver, MODELS

TOL = 1e-5


def test_fixture_conditions():
    """what the generator asserted: an early end and a full-length sentence among the greedy runs, every margin above 1e-3"""
    lens = []
    for m in MODELS:
        opt, _, _, _, g = fixture(m)
        lens.append((len(g['greedy_seq']), opt['seq_length']))
        assert float(g['greedy_margin']) > 1e-3 and float(g['beam_margin']) > 1e-3, m
        assert int(g['beam_size']) == 3 and g['beam_seq'].shape == (3, opt['seq_length'])
    assert any(1 <= n < T for n, T in lens) and any(n == T for n, T in lens), lens


@pytest.mark.parametrize('model', MODELS)
def test_greedy_restatement_equals_the_reference(model):
    opt, _, _, _, g = fixture(model)
    seq, lps, margins = DU.sample(driver(model), opt['seq_length'])
    assert seq == [int(v) for v in g['greedy_seq']]
    assert np.abs(np.asarray(lps, np.float64) - g['greedy_logprobs']).max(initial=0.0) < TOL
    assert abs(min(margins) - float(g['greedy_margin'])) < 1e-4


@pytest.mark.parametrize('model', MODELS)
def test_beam_restatement_with_the_alias_equals_the_reference(model):
    """legacy_p_alias=True is the reference as it runs under the torch that wrote the fixture: every p is -1000 and done_beams is the
    first beam_size completions, in completion order"""
    opt, _, _, _, g = fixture(model)
    beams, every, gaps = DU.beam_search(driver(model), opt['seq_length'], 3, legacy_p_alias=True)
    assert [b['index'] for b in beams] == [0, 1, 2]
    assert np.array_equal(np.stack([b['seq'] for b in beams]), g['beam_seq'])
    assert np.abs(np.stack([b['logps'] for b in beams]).astype(np.float64) - g['beam_logps']).max() < TOL
    assert np.all(g['beam_p'] == -1000.0) and all(float(b['p']) == -1000.0 for b in beams)
    assert abs(min(gaps) - float(g['beam_margin'])) < 1e-4


@pytest.mark.parametrize('model', MODELS)
def test_beam_restatement_without_the_alias_orders_by_joint_logprob(model):
    """the same completions (the alias changes no decision), kept by p descending, stable in completion order; p is the sum of the
    beam's log-probabilities up to its end"""
    opt, _, _, _, g = fixture(model)
    T = opt['seq_length']
    _, every_a, _ = DU.beam_search(driver(model), T, 3, legacy_p_alias=True)
    beams, every, _ = DU.beam_search(driver(model), T, 3, legacy_p_alias=False)
    assert len(every) == len(every_a) >= 3
    for a, b in zip(every_a, every):
        assert np.array_equal(a['seq'], b['seq']) and np.array_equal(a['logps'], b['logps']) and a['index'] == b['index']
    order = sorted(range(len(every)), key=lambda i: (-float(every[i]['p']), i))[:3]
    assert [b['index'] for b in beams] == order
    for b in beams:
        n = int(np.argmax(b['seq'] == 0)) + 1 if (b['seq'] == 0).any() else T
        if float(b['p']) > -900:                                 # (a beam that went on from a completed one carries its -1000)
            assert abs(float(b['p']) - float(b['logps'][:n].astype(np.float64).sum())) < 1e-4


def test_the_two_ordering_rules_differ_on_the_fixture():
    """topdown: the best completion by p is not the first completed, and the kept sets differ"""
    opt, _, _, _, _ = fixture('topdown')
    a, _, _ = DU.beam_search(driver('topdown'), opt['seq_length'], 3, legacy_p_alias=True)
    b, _, _ = DU.beam_search(driver('topdown'), opt['seq_length'], 3, legacy_p_alias=False)
    assert b[0]['index'] != 0
    assert sorted(x['index'] for x in a) != sorted(x['index'] for x in b)


def test_decode_sequence():
    """the product's lib/misc/utils.py decode_sequence: words up to the first 0, with the str keys of the captioner's infos file and with the
    int keys of Loader.ix_to_word (what tools/predict.py passes for real data)"""
    from lang2seg_amd.model.caption_device import decode_sequence
    for words in ({str(i): 'w%d' % i for i in range(1, 8)}, {i: 'w%d' % i for i in range(1, 8)}):
        assert decode_sequence(words, [3, 1, 7, 0, 5]) == 'w3 w1 w7'
        assert decode_sequence(words, np.asarray([2, 2], np.int64)) == 'w2 w2'
        assert decode_sequence(words, []) == '' and decode_sequence(words, [0, 2]) == ''
    with pytest.raises(KeyError):
        decode_sequence({1: 'a'}, [1, 9])


def _net(variant='cycle', cap='mask', **opt):
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    net = object.__new__(resnetv1)                               # the argument checks come before anything touches a device
    net.variant, net.var, net.cap_model, net.training = variant, {'cap': cap}, ('att2in2' if cap else None), False
    net.opt = dict(dict(vocab_size=20, seq_length=6), **opt)
    return net


@pytest.mark.parametrize('kw,flag', [(dict(beam_size=0), '--beam_size'), (dict(beam_size=17), '--beam_size'), (dict(temperature=0.0), '--temperature'),
                                     (dict(temperature=-1.0, sample_max=0), '--temperature'), (dict(sample_max=2), '--sample_max'),
                                     (dict(beam_size=None), '--beam_size'), (dict(beam_size='3'), '--beam_size'), (dict(beam_size=2.5), '--beam_size'),
                                     (dict(temperature=None), '--temperature'), (dict(temperature='hot'), '--temperature')])
def test_argument_errors_name_the_flag(kw, flag):
    with pytest.raises(ValueError, match=flag):
        _net().caption_decode(None, **kw)


def test_beam_size_beyond_the_vocabulary_and_the_token_limit():
    with pytest.raises(ValueError, match='--beam_size'):
        _net(vocab_size=3).caption_decode(None, beam_size=5)
    with pytest.raises(ValueError, match='--beam_size'):
        _net(seq_length=65).caption_decode(None, beam_size=2)


def test_variant_without_a_caption_branch():
    with pytest.raises(ValueError, match='--variant baseline'):
        _net('baseline', None).caption_decode(None)
    net = _net('baseline', None)
    with pytest.raises(ValueError, match='--variant baseline'):
        net.caption_features(None)


# ------------------------------------------------------------------ decoding runs the training forward's own token function
@pytest.mark.parametrize('model', ['topdown', 'adaatt', 'adaattmo'])
def test_decoding_step_equals_training_forward_without_a_device(model, monkeypatch):
    """the entry points restated in torch (TorchOps, as in the host-order tests of tests/test_topdown_cpu.py / test_adaatt_cpu.py, at their
    SMALL sizes): the training forward in eval mode on S = 4 given tokens, then nets/decode.py's step driven with the same tokens
    (teacher-forced) on B = 1 row and on B = 2 equal rows.  Every row's logits are the forward's cap.logits row within FWD_TOL.
    (att2in2's per-token entries have no torch restatement: tests/test_decode_gpu.py test_decode_equals_training_forward holds it.)"""
    import torch
    from adaatt_util import TorchOps, ada_opt, cap_state as ada_state
    from topdown_util import CAP, TorchLinearOp, td_opt, cap_state as td_state, rel_err
    from test_topdown_cpu import SMALL as TD_SMALL, FWD_TOL
    from test_adaatt_cpu import SMALL as ADA_SMALL
    from lang2seg_amd import ops as O
    from lang2seg_amd._lib import F32
    from lang2seg_amd.nets import resnet_v1 as RN, decode
    from lang2seg_amd.nets.params import ParamStore
    for n in TorchOps.NAMES:
        monkeypatch.setattr(O, n, getattr(TorchOps, n), raising=False)
    monkeypatch.setattr(ParamStore, 'refresh_shadow_full', lambda self: None)
    opt, sd_of = (td_opt(**TD_SMALL), td_state) if model == 'topdown' else (ada_opt(model, **ADA_SMALL), ada_state)
    S, V, L = 4, opt['vocab_size'], 196
    net = RN.resnetv1(opt, batch_size=1, num_layers=50)
    net.device, net.dt = 'cpu', F32
    net.P = P = ParamStore(opt, 50, 81, 12, 1, 'cpu', F32)
    P.load_state_dict(sd_of(opt, seed=4))
    net.att_embed = TorchLinearOp(P, CAP + 'att_embed.0.weight', CAP + 'att_embed.0.bias')
    g = torch.Generator().manual_seed(11)
    fc, att = torch.randn(opt['fc_feat_size'], generator=g), torch.randn(L, opt['att_feat_size'], generator=g)
    words = torch.cat([torch.zeros(1, dtype=torch.int64), torch.randint(1, V + 1, (S,), generator=g)])
    net.training, net.keep_logprobs, net._cap_loss_weight, net.parity, net._cap_pre = False, False, 1.0, None, None
    net.t = {'fc_feats': fc.clone()}
    net._caption_fwd(dict(S=S, cap_in=words[:S].clone(), cap_tgt=words[1:].clone(), cap_mask=torch.ones(S)), att.clone(), torch.zeros(8))
    want = net.buf('cap.logits', (S, V + 1), torch.float32).clone()
    assert float(want.abs().max()) > 0
    cap = net.captioner
    for B in (1, 2):
        H = cap.decode_start(*decode._head(net, att.clone()), fc.clone())
        cur, new = cap.new_states('a', B), cap.new_states('b', B)
        for i in range(S):
            logits = decode.step(net, H, cur, new, words[i].repeat(B), B)
            for r in range(B):
                e = rel_err(logits[r], want[i])
                assert e < FWD_TOL, (model, B, i, r, e)
            cur, new = new, cur


def test_predict_tool_takes_the_caption_flags():
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    try:
        import predict
    finally:
        sys.path.pop(0)
    a = predict.parse_args(['--synthetic', '1', '--caption', '1', '--beam_size', '3', '--sample_max', '0', '--temperature', '0.5',
                            '--caption_model', 'adaatt', '--adaatt', '1', '--rnn_size', '256'])
    assert (a['caption'], a['beam_size'], a['sample_max'], a['temperature']) == (1, 3, 0, 0.5)
    assert (a['caption_model'], a['adaatt'], a['rnn_size']) == ('adaatt', 1, 256)
    d = predict.parse_args(['--synthetic', '1'])
    assert d['caption'] == 0 and d['beam_size'] == 1 and d['sample_max'] == 1 and d['caption_model'] is None
