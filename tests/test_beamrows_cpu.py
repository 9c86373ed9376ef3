"""Beam search on rows without a device: the numpy restatement (tests/beamrows_util.py) against the reference's own beam-3 run
(tests/golden/ref_decode.npz, as tests/test_decode_cpu.py holds decode_util.beam_search to it), the margins of every decision on the rows
fixture (tests/golden/ref_caprows.npz) that tests/test_beamrows_gpu.py compares routes on, the argument errors of
Network.caption_beam_rows, detect_image and tools/eval_common.py, and the tools' new flag.

The margins.  The GPU test holds log-probabilities to 1e-5 absolute and tokens exactly, so every decision of the restated search has to
be clearer than that: the smallest gap between consecutive candidates among the best B + 1 at any step, and between consecutive
completions among the best B + 1 of the final order, must exceed 1e-4 for every row of both captioners at B = 2, 3 and 5 (measured: the
lowest are 1.9e-4, topdown row 2 at B = 5, and 2.6e-4, att2in2 row 3 at B = 3 and 5)."""
import os
import sys

import numpy as np
import pytest

import beamrows_util as BU
import caprows_util as CU
import decode_util as DU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-6
MARGIN = 1e-4


@pytest.mark.parametrize('model', DU.MODELS)
def test_beam_rows_on_one_row_equals_the_references_beam_search(model):
    """the alias off (the rule the project decodes by): the kept beams are the reference's completions (legacy_p_alias=True keeps the first
    three in completion order, which tests/test_decode_cpu.py pins to the recorded run) re-ordered by p; their tokens exact, logps 1e-6"""
    opt, _, _, _, g = DU.fixture(model)
    T = opt['seq_length']
    out, index, margin = BU.beam_rows([DU.driver(model)], T, 3)
    _, every_alias, _ = DU.beam_search(DU.driver(model), T, 3, legacy_p_alias=True)
    assert out['beam_n'][0] == 3 and len(index[0]) == 3 and margin[0] > MARGIN
    for v, i in enumerate(index[0]):
        assert np.array_equal(out['beam_seq'][0, v], every_alias[i]['seq']) and np.array_equal(out['beam_logprobs'][0, v], every_alias[i]['logps'])
        if i < 3:                                                  # one of the reference's own three: the recorded values
            assert np.array_equal(out['beam_seq'][0, v], g['beam_seq'][i])
            assert np.abs(out['beam_logprobs'][0, v].astype(np.float64) - g['beam_logps'][i]).max() < TOL
    assert list(out['beam_p'][0]) == sorted(out['beam_p'][0], reverse=True)
    s = out['seq'][0]
    n = int(np.argmax(s == 0)) if (s == 0).any() else T
    assert np.array_equal(s[:n], out['beam_seq'][0, 0, :n]) and (s[n:] == 0).all() and (out['logprobs'][0, n + 1:] == 0).all()
    assert np.array_equal(out['logprobs'][0, :min(n + 1, T)], out['beam_logprobs'][0, 0, :min(n + 1, T)])


@pytest.mark.parametrize('B', [2, 3, 5])
@pytest.mark.parametrize('model', CU.MODELS)
def test_every_decision_on_the_rows_fixture_is_clear(model, B):
    opt = CU.fixture(model)[0]
    out, index, margin = BU.beam_rows(CU.drivers(model), opt['seq_length'], B)
    print('%s B = %d: margins per row %s' % (model, B, ['%.2e' % m for m in margin]))
    assert len(margin) == 5 and min(margin) > MARGIN, margin
    assert (out['beam_n'] == B).all()


def test_final_ordering_is_stable_and_keeps_the_first_b():
    T, B = 3, 2
    RW = 2 * T + 2
    done = np.zeros((2, B * T, RW), np.int32)
    p = np.asarray([-2.0, -1.0, -2.0, -1.0, -1000.5, -0.5], np.float32)
    for i in range(B * T):
        done[0, i, :T] = [i + 1, 0 if i % 2 else 7, 0]
        done[0, i, T:2 * T] = np.asarray([-0.1 * (i + 1), -0.2, 0.0], np.float32).view(np.int32)
        done[0, i, 2 * T] = p[i:i + 1].view(np.int32)[0]
        done[0, i, 2 * T + 1] = i
    out = BU.finish_rows(done, [6, 0], B, T)
    assert out['beam_n'].tolist() == [2, 0] and out['beam_p'][0].tolist() == [-0.5, -1.0]
    assert out['beam_seq'][0].tolist() == [[6, 0, 0], [2, 0, 0]]                       # -1.0 twice: the one completed first
    assert out['seq'][0].tolist() == [6, 0, 0] and np.allclose(out['logprobs'][0], [-0.6, -0.2, 0.0])
    assert not out['seq'][1].any() and not out['beam_seq'][1].any()
    out = BU.finish_rows(done, [1, 0], B, T)
    assert out['beam_n'].tolist() == [1, 0] and out['seq'][0].tolist() == [1, 7, 0] and not out['beam_seq'][0, 1].any()


def _net(variant='cycle', cap='mask', **opt):
    from lang2seg_amd.nets.resnet_v1 import resnetv1
    net = object.__new__(resnetv1)                               # the argument checks come before anything touches a device
    net.variant, net.var, net.cap_model, net.training = variant, {'cap': cap}, ('att2in2' if cap else None), False
    net.opt = dict(dict(vocab_size=20, seq_length=6), **opt)
    return net


@pytest.mark.parametrize('B', [0, 17, None, '3', 2.5, True])
def test_beam_size_errors_are_those_of_the_single_mask_path(B):
    with pytest.raises(ValueError, match='--beam_size') as e:
        _net().caption_beam_rows(None, beam_size=B)
    with pytest.raises(ValueError, match='--beam_size') as e1:
        _net().caption_decode(None, beam_size=B)
    assert str(e.value) == str(e1.value)


def test_beam_size_beyond_the_vocabulary_and_the_token_limit():
    with pytest.raises(ValueError, match='--beam_size.*words'):
        _net(vocab_size=3).caption_beam_rows(None, beam_size=5)
    with pytest.raises(ValueError, match='--beam_size.*at most 64'):
        _net(seq_length=65).caption_beam_rows(None, beam_size=2)
    with pytest.raises(ValueError, match='--beam_size.*at most 64'):
        _net(seq_length=65).caption_beam_rows(None, beam_size=1)
    with pytest.raises(ValueError, match='no caption branch'):
        _net('baseline', None).caption_beam_rows(None)


def test_caption_decode_rows_still_refuses_beams_and_samples():
    for kw in (dict(beam_size=2), dict(sample_max=0)):
        with pytest.raises(ValueError, match='--sample_max.*--beam_size'):
            _net().caption_decode_rows(None, rows=5, **kw)


def test_the_stage_checks_beam_size_before_any_launch():
    from lang2seg_amd.model import detect_device as DD
    net = _net()
    net.layers, net.att_embed = {4: True}, object()
    with pytest.raises(ValueError, match='--beam_size'):
        DD.rows_stage(net, np.asarray([[3, 1, 0]]), True, False, None, 17)
    assert DD.rows_stage(net, np.asarray([[3, 1, 0]]), False, False, None, 3) is None
    assert DD.rows_stage(net, np.asarray([[3, 1, 0]]), True, False, None, 3).beam_size == 3
    assert DD.rows_stage(net, np.asarray([[3, 1, 0]]), False, True, None, 3).beam_size == 1      # nothing to describe: the flag has no effect


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def test_eval_tool_beam_size_needs_describe():
    tool = _tool('eval_common')
    base = ['--device_eval', '1', '--synthetic', '1', '--allow_init_weights', '1']
    assert tool.parse_args(base)['beam_size'] == 1
    a = tool.parse_args(base + ['--dump_detections', 'd.json', '--describe', '1', '--beam_size', '3'])
    assert (a['describe'], a['beam_size']) == (1, 3)
    for flags in (['--beam_size', '3'], ['--dump_detections', 'd.json', '--beam_size', '2'], ['--dump_detections', 'd.json', '--expr_score', '1', '--beam_size', '2']):
        with pytest.raises(ValueError, match='--beam_size.*--describe'):
            tool.main(tool.parse_args(base + flags), 'cycle')


def test_predict_tool_takes_beam_size_with_describe():
    predict = _tool('predict')
    a = predict.parse_args(['--synthetic', '1', '--all_detections', '1', '--describe', '1', '--beam_size', '3'])
    assert (a['all_detections'], a['describe'], a['beam_size'], a['caption']) == (1, 1, 3, 0)
    assert predict.parse_args(['--synthetic', '1', '--all_detections', '1', '--describe', '1'])['beam_size'] == 1
