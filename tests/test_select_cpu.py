"""Judging the detections, without a GPU: the numpy restatement of l2s_detect_choose against a brute-force version of itself, the header's
declarations, ops' record decoders and the tools' flags."""
import os
import re
import sys

import numpy as np
import pytest

import select_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_restatement_equals_brute_force_on_200_cases():
    redrawn, n_rules = 0, 0
    for seed in range(200):
        cap = [1, 2, 5, 9, 33, 70][seed % 6]
        count = [0, 1, cap, max(cap - 1, 0)][(seed // 6) % 4]
        c, r = SU.choose_case(seed, cap, count, [0, 1, 3, 8][seed % 4], seed % 2, with_expr=seed % 5 != 0)
        redrawn += r
        a, b = SU.choose(*SU.choose_args(c)), SU.choose_brute(*SU.choose_args(c))
        assert a == b, (seed, a, b)
        assert len(a) == len(SU.rule_names(c['lambdas'], c['expr'] is not None))
        n_rules += len(a)
        if count == 0:
            assert all(x == dict(det=-1, cls=-1, hit=0, I=0, U=c['gt_area'], key=0.0) for x in a)
    print('200 cases, %d rules, %d redrawn for a margin under %g' % (n_rules, redrawn, SU.MARGIN))


def test_generator_of_the_gpu_cases_drops_no_case():
    """the cases tests/test_select_gpu.py runs: every one is produced (a redraw replaces, it never skips), and redraws are rare"""
    redrawn, n = 0, 0
    for cap in (1, 64, 65, 1500):
        for count in (0, 1, cap):
            for n_lambda in (0, 1, 8):
                for per_token in (0, 1):
                    c, r = SU.choose_case(1000 + n, cap, count, n_lambda, per_token)
                    assert c['score'].shape == (cap,) and len(c['lambdas']) == n_lambda and not SU.close_rerank(
                        c['score'], c['expr'], min(count, cap), c['lambdas'], c['per_token'], c['n_tok'])
                    redrawn += r
                    n += 1
    print('%d cases, %d redrawn' % (n, redrawn))
    assert n == 72 and redrawn <= n // 4


def test_restatement_tie_rules():
    score = np.asarray([0.5, 0.9, 0.9, 0.2], np.float32)
    I, U = np.asarray([0, 1, 2, 0]), np.asarray([0, 2, 4, 7])
    expr = np.asarray([-3.0, -1.0, -1.0, -9.0], np.float32)
    z = np.zeros(4, np.int32)
    r = SU.choose(score, z + 1, z, I, U, 4, 11, expr, [0.0, 1e12])
    assert [x['det'] for x in r] == [1, 1, 1, 1, 1]
    r = SU.choose(score[::-1].copy(), z + 1, z, I[::-1].copy(), U[::-1].copy(), 4, 11, expr[::-1].copy(), [0.0, 1e12])
    assert [x['det'] for x in r] == [1, 1, 1, 1, 1]                # the lower index of the tied pair, now the other row
    assert r[1]['key'] == 0.5 and (r[1]['I'], r[1]['U']) == (2, 4)


def test_box_hit_at_exactly_half():
    assert SU.box_hit([0, 0, 9, 9], [0, 0, 9, 19], 1.0) == 1
    assert SU.box_hit([0, 0, 9, 8], [0, 0, 9, 19], 1.0) == 0
    assert SU.box_hit([0, 0, 9, 9], [0, 0, 19, 39], 2.0) == 0      # gt / 2 = (0, 0, 9.5, 19.5): 100 / 215.25
    assert SU.box_hit([0, 0, 9, 9], [0, 0, 18, 38], 2.0) == 1      # gt / 2 = (0, 0, 9, 19)


def test_header_declares_the_entry_points_and_structs():
    hdr = open(os.path.join(ROOT, 'include', 'lang2seg_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert re.search(r'\bint\s+l2s_detect_gt_iou\s*\(', code) and re.search(r'\bint\s+l2s_detect_choose\s*\(', code)
    size = {'int': 4, 'float': 4, 'long long': 8, 'double': 8}
    for name, nbytes in (('l2s_det_gt', 16), ('l2s_det_choice', 40), ('l2s_det_record', 32)):
        m = re.search(r'typedef struct \{([^}]*)\}\s*%s;' % name, code)
        assert m, name
        total = 0
        for field in [f.strip() for f in m.group(1).split(';') if f.strip()]:
            ty, var = field.rsplit(' ', 1)
            arr = re.search(r'\[(\d+)\]', var)
            total += size[ty.strip()] * (int(arr.group(1)) if arr else 1)
        assert total == nbytes, (name, total)
    from lang2seg_amd import ops as O, _lib
    assert (O.DET_GT_BYTES, O.DET_CHOICE_BYTES, O.DET_RECORD_BYTES) == (16, 40, 32)
    assert 'l2s_detect_gt_iou' in _lib.SIGS and 'l2s_detect_choose' in _lib.SIGS


def test_ops_field_decoders_round_trip():
    from lang2seg_amd import ops as O
    rs = np.random.RandomState(0)
    g = np.zeros(5, np.dtype([('I', '<i4'), ('U', '<i4'), ('hit', '<i4'), ('reserved', '<i4')]))
    g['I'], g['U'], g['hit'] = rs.randint(0, 1 << 30, 5), rs.randint(0, 1 << 30, 5), rs.randint(0, 2, 5)
    assert g.itemsize == O.DET_GT_BYTES
    I, U, hit = O.det_gt_fields(g.view(np.int32))
    assert np.array_equal(I, g['I']) and np.array_equal(U, g['U']) and np.array_equal(hit, g['hit'])
    c = np.zeros(3, np.dtype([('det', '<i4'), ('cls', '<i4'), ('hit', '<i4'), ('reserved', '<i4'), ('I', '<i8'), ('U', '<i8'), ('key', '<f8')]))
    c['det'], c['cls'], c['hit'] = [-1, 7, 1499], [-1, 80, 3], [0, 1, 1]
    c['I'], c['U'], c['key'] = [0, 1 << 40, 5], [9, (1 << 41) + 1, 10], [0.0, -123.456789012345, 0.5]
    assert c.itemsize == O.DET_CHOICE_BYTES
    import torch
    for raw in (c.view(np.int32), torch.from_numpy(c.view(np.int32).copy())):
        det, cls, hit, I, U, key = O.det_choice_fields(raw)
        for got, name in ((det, 'det'), (cls, 'cls'), (hit, 'hit'), (I, 'I'), (U, 'U'), (key, 'key')):
            assert np.array_equal(got, c[name]) and got.dtype == c[name].dtype, name
    with pytest.raises(ValueError):
        O.det_choice_fields(np.zeros(11, np.int32))


def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import eval_common
    finally:
        sys.path.pop(0)
    return eval_common


def test_parse_args_defaults_leave_the_options_off():
    a = _tool().parse_args([])
    assert a['judge_detections'] == 0 and a['rerank'] is None and a['rerank_per_token'] == 0 and a['dump_selection'] is None
    assert _tool().selection_options(a, 'cycle') == (False, None, False)
    a = _tool().parse_args(['--dump_detections', 'd.json', '--expr_score', '1', '--rerank', '0,0.5,4'])
    assert _tool().selection_options(a, 'cycle') == (True, [0.0, 0.5, 4.0], False)         # --rerank implies judging


BASE = ['--device_eval', '1', '--synthetic', '1', '--allow_init_weights', '1']
ERRORS = [
    (['--judge_detections', '1'], 'cycle', r'--judge_detections.*--dump_detections'),
    (['--rerank', '0.5'], 'cycle', r'--rerank.*--dump_detections'),
    (['--rerank_per_token', '1'], 'cycle', r'--rerank_per_token.*--dump_detections'),
    (['--dump_selection', 's.json'], 'cycle', r'--dump_selection.*--dump_detections'),
    (['--dump_detections', 'd.json', '--rerank', '0.5'], 'cycle', r'--rerank.*--expr_score'),
    (['--dump_detections', 'd.json', '--judge_detections', '1'], 'vgg', r'--judge_detections.*vgg'),
    (['--dump_detections', 'd.json', '--expr_score', '1', '--rerank', '0.5,abc'], 'cycle', r'--rerank.*abc'),
    (['--dump_detections', 'd.json', '--expr_score', '1', '--rerank', '0.5,nan'], 'cycle', r'--rerank.*nan'),
    (['--dump_detections', 'd.json', '--expr_score', '1', '--rerank', '0.5,inf'], 'cycle', r'--rerank.*inf'),
    (['--dump_detections', 'd.json', '--expr_score', '1', '--rerank', '1,2,3,4,5,6,7,8,9'], 'cycle', r'--rerank.*8'),
    (['--dump_detections', 'd.json', '--judge_detections', '1', '--rerank_per_token', '1'], 'cycle', r'--rerank_per_token.*--rerank'),
]


@pytest.mark.parametrize('flags,variant,match', ERRORS)
def test_tool_value_errors_name_their_flags(flags, variant, match):
    """raised by main() before the network is built (no GPU is touched)"""
    tool = _tool()
    with pytest.raises(ValueError, match=match):
        tool.main(tool.parse_args(BASE + flags), variant)


def test_library_value_errors_name_their_options():
    from lang2seg_amd.model import eval_device as ED
    for kw, match in ((dict(judge=True), r'judge.*detections'), (dict(rerank=[0.5]), r'rerank.*detections'),
                      (dict(detections=True, rerank=[0.5]), r'rerank.*expr_score'), (dict(detections=True, judge=True, per_token=True), r'per_token.*rerank'),
                      (dict(detections=True, judge=True, variant='vgg'), r'judge.*vgg'),
                      (dict(detections=True, expr_score=True, rerank=[float('nan')]), r'rerank.*finite'),
                      (dict(detections=True, expr_score=True, rerank=list(range(9))), r'rerank.*at most 8')):
        args = dict(detections=False, judge=False, rerank=None, per_token=False, expr_score=False, variant=None)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            ED.check_judge_options(**args)
    assert ED.check_judge_options(True, False, [0, 0.5], True, True) == [0.0, 0.5]
    assert ED.check_judge_options(False, False, None, False, False) == []
