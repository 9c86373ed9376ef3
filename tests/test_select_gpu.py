"""Judging the detections on the device (csrc/select.hip, model/detect_device.py _JudgeStage): l2s_detect_gt_iou and l2s_detect_choose
against the numpy restatements of tests/select_util.py, exactly; then eval_split_device with the judging options on the tiny cycle network
against numpy on its own dumped detections, and the tool."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import data as OD  # noqa: E402
import select_util as SU  # noqa: E402
from test_eval_device_gpu import _ListLoader, _synthetic_blobs  # noqa: E402
from test_rle_export_gpu import _net, _same_result, _same_details  # noqa: E402

pytestmark = pytest.mark.gpu
NEW_ENTRIES = ('l2s_detect_gt_iou', 'l2s_detect_choose')
# C-ABI calls of eval_split_device(detections=[]) on _net('cycle', .) over _synthetic_blobs(_SIZES, 3), counted by _calls() on the commit
# before the judge stage existed, per compute dtype (a change that alters the default path's launches on purpose updates them)
PARENT_CALLS_DETECTIONS = {'f32': 654, 'bf16': 640}


@pytest.fixture(scope='module', autouse=True)
def _restore_cfg():
    """what the tool's main() sets process-wide (cfg.COMPUTE_DTYPE, cfg.TRAIN) ends with this file"""
    import copy
    from lang2seg_amd.model.config import cfg
    train, dtype = copy.deepcopy(dict(cfg.TRAIN)), cfg.COMPUTE_DTYPE
    yield
    for k in list(cfg.TRAIN.keys()):
        if k not in train:
            del cfg.TRAIN[k]
    for k, v in train.items():
        cfg.TRAIN[k] = v
    cfg.COMPUTE_DTYPE = dtype


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ops():
    from lang2seg_amd import ops as O
    return O


def _calls(fn):
    """the C-ABI entries fn() issues, in order (as tests/test_caprows_gpu.py counts them)"""
    O = _ops()
    names, real = [], O.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    O.call = spy
    try:
        fn()
    finally:
        O.call = real
    return names


# ---------------------------------------------------------------- l2s_detect_gt_iou
def _gt_iou(can, boxes, areas, count, gt, gt_box, scale):
    O = _ops()
    cap = can.shape[0]
    out = torch.full((cap, 4), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    area = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    O.detect_gt_iou(_dev(can), _dev(SU.records(boxes, areas)), _dev(np.asarray([count, count], np.int32)), _dev(gt), _dev(np.asarray(gt_box, np.float32)),
                    scale, out, area)
    return out.cpu().numpy(), int(area.cpu()[0])


def _check_gt_iou(can, boxes, areas, count, gt, gt_box, scale, tag):
    raw, area = _gt_iou(can, boxes, areas, count, gt, gt_box, scale)
    I, U, hit = _ops().det_gt_fields(raw)
    yI, yU, yhit, yarea = SU.gt_iou(can, boxes, count, gt, gt_box, scale)
    assert area == yarea, (tag, area, yarea)
    assert np.array_equal(I, yI) and np.array_equal(U, yU) and np.array_equal(hit, yhit), (tag, np.flatnonzero(I != yI)[:5], np.flatnonzero(U != yU)[:5])
    n = min(count, can.shape[0])
    assert (raw[n:] == 0).all() and (raw[:, 3] == 0).all(), tag                   # the zeroed tail, the reserved word
    return raw


@pytest.mark.parametrize('ih,iw,Hs,Ws', [(1, 1, 3, 2), (3, 5, 7, 4), (37, 61, 20, 31), (37, 61, 50, 80), (37, 61, 37, 61), (8, 257, 20, 100),
                                         (64, 1027, 100, 1600)])
def test_gt_iou_exact(ih, iw, Hs, Ws):
    scale = float(np.float32(1.25))
    for cap in (1, 3, 65, 300):
        rs = np.random.RandomState(cap + ih)
        can, boxes, areas = SU.box_canvases(rs, cap, ih, iw)
        gt = (rs.rand(Hs, Ws) > 0.5).astype(np.uint8)
        gt[:, :Ws // 3] = 0
        gt_box = boxes[rs.randint(cap)] * np.float32(scale) + rs.randint(-2, 3, 4)
        for count in sorted({0, 1, cap - 1, cap}):
            _check_gt_iou(can, boxes, areas, count, gt, gt_box, scale, (ih, iw, cap, count))


def test_gt_iou_empty_and_full():
    ih, iw, cap = 37, 61, 9
    rs = np.random.RandomState(4)
    for kind in ('empty', 'full', 'random'):
        can, boxes, areas = SU.box_canvases(rs, cap, ih, iw, kind)
        for gt in (np.zeros((20, 31), np.uint8), np.ones((20, 31), np.uint8), np.full((50, 80), 255, np.uint8)):
            raw = _check_gt_iou(can, boxes, areas, cap, gt, [3, 3, 30, 20], 1.0, (kind, int(gt.max())))
            I, U, _ = _ops().det_gt_fields(raw)
            if kind == 'empty':
                assert (I == 0).all() and (U == (ih * iw if gt.any() else 0)).all()
            if kind == 'full' and gt.all():
                assert np.array_equal(I, areas) and (U == ih * iw).all()


def test_gt_iou_hit_at_exactly_half():
    ih, iw = 40, 30
    boxes = np.asarray([[0, 0, 9, 9], [0, 0, 9, 8], [0, 0, 9, 19], [20, 20, 25, 25]], np.float32)
    can = np.zeros((4, ih, iw), np.uint8)
    areas = np.zeros(4, np.int32)
    gt = np.zeros((ih, iw), np.uint8)
    raw = _check_gt_iou(can, boxes, areas, 4, gt, [0, 0, 9, 19], 1.0, 'half')
    assert _ops().det_gt_fields(raw)[2].tolist() == [1, 0, 1, 0]                  # 100 / 200 hits; one pixel row less: 90 / 200 does not
    raw = _check_gt_iou(can, boxes, areas, 4, gt, [0, 0, 18, 38], 2.0, 'half, scaled')
    assert _ops().det_gt_fields(raw)[2].tolist() == [1, 0, 1, 0]


def test_gt_iou_two_runs_same_bytes_and_unaligned_canvases():
    rs = np.random.RandomState(8)
    ih, iw, cap = 19, 1027, 40
    can, boxes, areas = SU.box_canvases(rs, cap, ih, iw)
    gt = (rs.rand(33, 500) > 0.3).astype(np.uint8)
    a, aa = _gt_iou(can, boxes, areas, cap, gt, [10, 2, 400, 15], 1.0)
    b, ba = _gt_iou(can, boxes, areas, cap, gt, [10, 2, 400, 15], 1.0)
    assert a.tobytes() == b.tobytes() and aa == ba
    # the canvases from an odd byte on: every row's vector loads have a head and a tail
    O = _ops()
    flat = torch.zeros((cap * ih * iw + 3,), dtype=torch.uint8, device='cuda')
    flat[3:] = _dev(can).reshape(-1)
    out = torch.zeros((cap, 4), dtype=torch.int32, device='cuda')
    area = torch.zeros((1,), dtype=torch.int32, device='cuda')
    O.detect_gt_iou(flat[3:].view(cap, ih, iw), _dev(SU.records(boxes, areas)), _dev(np.asarray([cap, cap], np.int32)), _dev(gt),
                    _dev(np.asarray([10, 2, 400, 15], np.float32)), 1.0, out, area)
    assert out.cpu().numpy().tobytes() == a.tobytes() and int(area.cpu()[0]) == aa


def test_gt_iou_and_choose_bad_arguments():
    from lang2seg_amd import _lib
    lib = _lib.load()
    z = torch.zeros((64,), dtype=torch.int32, device='cuda')
    can = torch.zeros((2, 4, 4), dtype=torch.uint8, device='cuda')
    f = torch.zeros((4,), dtype=torch.float32, device='cuda')
    p = lambda t: t.data_ptr()                                                  # noqa: E731
    good = [p(can), p(z), p(z), 2, 4, 4, p(can), 4, 4, p(f), 1.0, p(z), p(z), None]
    assert lib.l2s_detect_gt_iou(*good) == 0
    for k, v in ((0, None), (1, None), (2, None), (6, None), (9, None), (11, None), (12, None), (3, 0), (3, 65536), (4, 0), (5, -1), (7, 0), (8, 0),
                 (10, 0.0), (10, float('nan'))):
        bad = list(good)
        bad[k] = v
        assert lib.l2s_detect_gt_iou(*bad) == 1, (k, v)
    bad = list(good)
    bad[4], bad[5] = 1 << 16, 1 << 15                                           # ih * iw = 2^31
    assert lib.l2s_detect_gt_iou(*bad) == 1
    import ctypes
    lam = (ctypes.c_float * 9)(*([0.5] * 9))
    out = torch.zeros((128,), dtype=torch.int32, device='cuda')
    good = [p(z), p(z), p(z), 2, p(z), p(f), lam, 1, 0, 3, p(out), None]
    assert lib.l2s_detect_choose(*good) == 0
    for k, v in ((0, None), (1, None), (2, None), (4, None), (10, None), (3, 0), (5, None), (7, 9), (7, -1)):
        bad = list(good)
        bad[k] = v
        assert lib.l2s_detect_choose(*bad) == 1, (k, v)                         # (5: n_lambda > 0 without expr)
    bad = list(good)
    bad[8], bad[9] = 1, 0                                                       # per_token with no tokens
    assert lib.l2s_detect_choose(*bad) == 1
    torch.cuda.synchronize()


# ---------------------------------------------------------------- l2s_detect_choose
def _choose(c):
    O = _ops()
    cap = c['score'].shape[0]
    rec = SU.records(np.zeros((cap, 4), np.float32), np.zeros(cap, np.int32), c['score'], c['cls'])
    rows = np.zeros((cap, 4), np.int32)
    rows[:, 0], rows[:, 1], rows[:, 2] = c['I'], c['U'], c['hit']
    names = SU.rule_names(c['lambdas'], c['expr'] is not None)
    out = torch.full((len(names) * 10 + 2,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    O.detect_choose(_dev(rec), _dev(rows), _dev(np.asarray([c['count'], c['count']], np.int32)), cap, _dev(np.asarray([c['gt_area']], np.int32)),
                    out, None if c['expr'] is None else _dev(c['expr']), c['lambdas'], c['per_token'], c['n_tok'])
    raw = out.cpu().numpy()
    assert (raw[len(names) * 10:] == 0x5A5A5A5A).all()                          # nothing behind the last record
    det, cls, hit, I, U, key = O.det_choice_fields(raw[:len(names) * 10])
    return [dict(det=int(det[k]), cls=int(cls[k]), hit=int(hit[k]), I=int(I[k]), U=int(U[k]), key=float(key[k])) for k in range(len(names))], names


def _assert_choice(got, names, want, tag):
    for g, name, w in zip(got, names, want):
        assert {k: g[k] for k in g if k != 'key'} == {k: w[k] for k in w if k != 'key'}, (tag, name, g, w)
        if name.startswith('rerank@'):                                         # the device's log and numpy's differ by a few ulp
            assert abs(g['key'] - w['key']) <= 1e-12 * max(1.0, abs(w['key'])), (tag, name, g, w)
        else:                                                                  # a conversion, or one division: the same bits
            assert g['key'] == w['key'], (tag, name, g, w)


@pytest.mark.parametrize('cap', [1, 64, 65, 1500])
def test_choose_exact(cap):
    n = 0
    for count in sorted({0, 1, cap}):
        for n_lambda in (0, 1, 8):
            for per_token in (0, 1):
                c, _ = SU.choose_case(1000 + n + cap, cap, count, n_lambda, per_token)
                got, names = _choose(c)
                assert len(got) == 3 + n_lambda
                _assert_choice(got, names, SU.choose(*SU.choose_args(c)), (cap, count, n_lambda, per_token))
                n += 1
    c, _ = SU.choose_case(5 + cap, cap, cap, 0, 0, with_expr=False)              # expr = None: two records
    got, names = _choose(c)
    assert names == ['detector', 'oracle']
    _assert_choice(got, names, SU.choose(*SU.choose_args(c)), (cap, 'no expr'))


def test_choose_ties_go_to_the_lowest_index():
    cap = 300
    c, _ = SU.choose_case(3, cap, cap, 1, 0, ties=False)
    c['score'][:] = np.float32(0.25)
    c['score'][[290, 7, 263]] = np.float32(0.75)                                 # three best scores, two of them in thread 7's stride
    c['I'][:], c['U'][:] = 1, 3
    c['I'][[299, 44]], c['U'][[299, 44]] = [2, 1], [4, 2]                        # 2 / 4 and 1 / 2
    c['U'][5] = c['I'][5] = 0                                                    # U = 0 counts as IoU 0, not as a tie with everything
    c['expr'][:] = np.float32(-5.0)
    c['expr'][[280, 24]] = np.float32(-1.5)
    c['lambdas'] = [0.0]
    got, names = _choose(c)
    _assert_choice(got, names, SU.choose(*SU.choose_args(c)), 'ties')
    assert [g['det'] for g in got] == [7, 44, 24, 7]
    assert (got[1]['I'], got[1]['U'], got[1]['key']) == (1, 2, 0.5)
    c['I'][:], c['U'][:] = 0, 0                                                  # every union empty: the first detection
    got, names = _choose(c)
    assert got[1]['det'] == 0 and got[1]['key'] == 0.0


def test_choose_lambda_zero_is_the_detector_and_a_large_lambda_the_speaker():
    for cap in (65, 700):
        rs = np.random.RandomState(cap)
        c, _ = SU.choose_case(11 + cap, cap, cap, 2, 0, ties=False)
        c['score'] = (rs.permutation(cap) + 1).astype(np.float32) / np.float32(cap + 1)      # distinct scores
        c['expr'] = -(rs.permutation(cap) + 1).astype(np.float32) / np.float32(8)            # distinct, at least 1 / 8 apart
        c['lambdas'] = [0.0, 1e12]
        got, names = _choose(c)
        _assert_choice(got, names, SU.choose(*SU.choose_args(c)), cap)
        assert got[3]['det'] == got[0]['det'] == int(np.argmax(c['score']))
        assert got[4]['det'] == got[2]['det'] == int(np.argmax(c['expr']))


# ---------------------------------------------------------------- end to end
_SIZES = [(224, 288), (256, 352)]
LAMBDAS = [0.0, 0.5, 4.0]
_E2E = {}


def _e2e(dtype):
    """one judged run, one plain run and their call lists per dtype, shared by the tests below (computed once, never changed)"""
    if dtype in _E2E:
        return _E2E[dtype]
    from lang2seg_amd.model.eval_device import eval_split_device
    net = _net('cycle', dtype)
    blobs = [dict(b, file_name='image%d.jpg' % j) for j, b in enumerate(_synthetic_blobs(_SIZES, 3))]      # (the results are grouped by name)
    opt = dict(verbose=False)
    r = dict(net=net, blobs=blobs)
    eval_split_device(_ListLoader(blobs), net, None, 'val', opt, detections=[], expr_score=True, rerank=LAMBDAS, selection=[])   # (buffers' first use)
    r['det0'], r['preds0'], r['dets0'] = [], [], []
    r['calls0'] = _calls(lambda: r.__setitem__('res0', eval_split_device(_ListLoader(blobs), net, None, 'val', opt, details=r['det0'],
                                                                          predictions=r['preds0'], detections=r['dets0'], expr_score=True)))
    r['det1'], r['preds1'], r['dets1'], r['sel'], r['tot'] = [], [], [], [], {}
    r['calls1'] = _calls(lambda: r.__setitem__('res1', eval_split_device(_ListLoader(blobs), net, None, 'val', opt, details=r['det1'],
                                                                          predictions=r['preds1'], detections=r['dets1'], expr_score=True,
                                                                          rerank=LAMBDAS, selection=r['sel'], selection_totals=r['tot'])))
    _E2E[dtype] = r
    return r


def _by_sentence(dets):
    out = {}
    for p in dets:
        out.setdefault((p['file_name'], p['sent_index']), []).append(p)
    return out


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_every_detection_is_judged_as_numpy_judges_its_dump(dtype):
    r = _e2e(dtype)
    groups = _by_sentence(r['dets1'])
    n = 0
    for blob in r['blobs']:
        im_info = np.asarray(blob['im_info'], np.float32).reshape(-1)[:3]
        scale = im_info[2]
        for i in range(3):
            gt_box = np.asarray(blob['gt_boxes'])[i, :4]
            for p in groups.get((blob['file_name'], i), []):
                ih, iw = p['segmentation']['size']
                m = OD.rle_decode(OD.rle_from_string(p['segmentation']['counts']), ih, iw) != 0
                g = SU.resize_gt(np.asarray(blob['gt_masks'])[i], ih, iw)
                assert (p['I'], p['U']) == (int((m & g).sum()), int((m | g).sum())), (dtype, p['file_name'], i, n)
                assert p['hit'] == SU.box_hit(p['box'], gt_box, scale)
                n += 1
    assert n == len(r['dets1']) > 6


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_choices_equal_the_restatement_on_the_dump(dtype):
    from lang2seg_amd.model.eval_device import EVAL_SEG_IOU_LIST
    r = _e2e(dtype)
    groups = _by_sentence(r['dets1'])
    names = SU.rule_names(LAMBDAS, True)
    assert len(r['sel']) == 6 and [(e['file_name'], e['sent_index']) for e in r['sel']] == [(b['file_name'], i) for b in r['blobs'] for i in range(3)]
    by_set = 0
    for e in r['sel']:
        blob = [b for b in r['blobs'] if b['file_name'] == e['file_name']][0]
        i = e['sent_index']
        lst = groups.get((e['file_name'], i), [])
        ih, iw = lst[0]['segmentation']['size'] if lst else (None, None)
        if lst:
            assert e['gt_area'] == int(SU.resize_gt(np.asarray(blob['gt_masks'])[i], ih, iw).sum())
        n_tok = int((np.asarray(blob['labels'])[i] != 0).sum()) + 1
        score = np.asarray([p['score'] for p in lst], np.float32)
        expr = np.asarray([p['expr_logprob'] for p in lst], np.float32)
        args = (score, [p['category_id'] for p in lst], [p['hit'] for p in lst], [p['I'] for p in lst], [p['U'] for p in lst], len(lst), e['gt_area'],
                expr, LAMBDAS, False, n_tok)
        want = SU.choose(*args)
        assert list(e['rules']) == names
        for k, (name, w) in enumerate(zip(names, want)):
            g = e['rules'][name]
            assert abs(g['key'] - w['key']) <= 1e-9 * max(1.0, abs(w['key'])) or g['det'] != w['det'], (name, g, w)
            if g['det'] != w['det']:                                           # only among re-rank keys closer than the margin
                assert name.startswith('rerank@') and lst
                key = SU.rerank_key(score, expr, LAMBDAS[k - 3], False, n_tok)
                assert key.max() - key[g['det']] < SU.MARGIN, (name, g, w)
                by_set += 1
                w = SU._record(g['det'], args[1], args[2], args[3], args[4], key[g['det']], e['gt_area'])
                assert abs(g['key'] - w['key']) <= 1e-9 * max(1.0, abs(w['key']))
            assert (g['det'], g['category_id'], g['hit'], g['I'], g['U']) == (w['det'], w['cls'], w['hit'], w['I'], w['U']), (name, g, w)
    print('%s: %d sentences x %d rules, %d choices taken by the set rule (keys within %g)' % (dtype, len(r['sel']), len(names), by_set, SU.MARGIN))
    # the totals are the sums of those records by _Totals' expressions
    assert r['tot'] == SU.totals(r['sel'], EVAL_SEG_IOU_LIST) and list(r['tot']) == names
    assert all(t['num_sent'] == 6 for t in r['tot'].values())
    assert r['tot']['oracle']['cum_I'] * r['tot']['detector']['cum_U'] >= 0


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_default_path_keeps_its_bits_and_its_launches(dtype):
    r = _e2e(dtype)
    assert _same_result(r['res0'], r['res1']) and _same_details(r['det0'], r['det1']) and r['preds0'] == r['preds1']
    assert len(r['dets0']) == len(r['dets1']) > 0
    for p, q in zip(r['dets0'], r['dets1']):
        assert {k: q[k] for k in p} == p and set(q) - set(p) == {'I', 'U', 'hit'}
    assert not set(r['calls0']) & set(NEW_ENTRIES)
    assert [c for c in r['calls1'] if c not in NEW_ENTRIES] == r['calls0']      # the stage adds its two launches per sentence, nothing else
    assert sum(1 for c in r['calls1'] if c in NEW_ENTRIES) == 2 * 6
    from lang2seg_amd.model.eval_device import eval_split_device
    plain = _calls(lambda: eval_split_device(_ListLoader(r['blobs']), r['net'], None, 'val', dict(verbose=False), detections=[]))
    print('%s: eval_split_device(detections=[]) issues %d C-ABI calls' % (dtype, len(plain)))
    assert len(plain) == PARENT_CALLS_DETECTIONS[dtype]


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_rule_detector_names_the_one_box_pick(dtype):
    r = _e2e(dtype)
    groups = _by_sentence(r['dets1'])
    checked = 0
    for e, pick in zip(r['sel'], r['preds1']):
        assert (e['file_name'], e['sent_index']) == (pick['file_name'], pick['sent_index'])
        lst = groups.get((e['file_name'], e['sent_index']), [])
        scores = [p['score'] for p in lst]
        if pick['category_id'] < 1 or not lst or scores.count(max(scores)) != 1 or max(scores) != pick['score']:
            continue
        d = e['rules']['detector']
        q = lst[d['det']]
        assert (q['category_id'], q['box'], q['score']) == (pick['category_id'], pick['box'], pick['score']) and d['hit'] == pick['hit']
        roi = [x[0] for x in r['det1']][r['preds1'].index(pick)]
        assert q['roi'] == roi
        print('%s %s[%d]: rule detector I / U %d / %d, the evaluation record %d / %d (difference %d / %d)' % (
            dtype, e['file_name'], e['sent_index'], d['I'], d['U'], pick['I'], pick['U'], d['I'] - pick['I'], d['U'] - pick['U']))
        checked += 1
    assert checked >= 2


def test_a_rerun_sentence_is_judged_again():
    from lang2seg_amd.model import detect_device as DD
    r = _e2e('f32')
    blob = r['blobs'][0]
    data = {k: v for k, v in blob.items() if not k.startswith('gt_') and k != 'labels'}
    kw = dict(expr_score=True, gt_masks=np.asarray(blob['gt_masks']), gt_boxes=np.asarray(blob['gt_boxes'])[:, :4], rerank=LAMBDAS)
    sel, sel1, cap = [], [], []
    lists = DD.detect_image(r['net'], data, np.asarray(blob['labels']), selection=sel, **kw)
    again = DD.detect_image(r['net'], data, np.asarray(blob['labels']), selection=sel1, _cap=1, _capture=cap, **kw)
    assert any('rerun' in c for c in cap) and max(len(l) for l in lists) > 1
    assert [[(p['roi'], p['I'], p['U'], p['hit']) for p in l] for l in lists] == [[(p['roi'], p['I'], p['U'], p['hit']) for p in l] for l in again]
    assert len(sel) == len(sel1) == 3
    for a, b in zip(sel, sel1):
        assert (a['file_name'], a['sent_index'], a['gt_area']) == (b['file_name'], b['sent_index'], b['gt_area'])
        for name in a['rules']:
            x, y = a['rules'][name], b['rules'][name]
            assert {k: x[k] for k in x if k != 'key'} == {k: y[k] for k in y if k != 'key'}, (name, x, y)
            assert abs(x['key'] - y['key']) <= 1e-5 * max(1.0, abs(x['key'])), (name, x, y)     # (the captioner on 1 row and on 128: last bits)
    # and it is what the evaluation's judged run selected for that image
    assert [e['rules']['oracle'] for e in r['sel'][:3]] == [e['rules']['oracle'] for e in sel]
    with pytest.raises(ValueError, match='gt_masks'):
        DD.detect_image(r['net'], data, np.asarray(blob['labels']), rerank=[0.5])


def test_eval_tool_judges_and_dumps_the_selection(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import eval_common
    finally:
        sys.path.pop(0)
    dpath, spath = str(tmp_path / 'det.json'), str(tmp_path / 'sel.json')
    args = eval_common.parse_args(['--synthetic', '1', '--allow_init_weights', '1', '--device_eval', '1', '--synthetic_images', '2', '--verbose', '0',
                                   '--output_postfix', 'no_such_run', '--cfg', '', '--results_dir', str(tmp_path), '--dump_detections', dpath, '--expr_score', '1',
                                   '--judge_detections', '1', '--rerank', '0.5', '--dump_selection', spath])
    eval_common.main(args, variant='cycle')
    printed = capsys.readouterr().out
    sel, dets = json.load(open(spath)), json.load(open(dpath))
    assert len(sel) == 6 and len(set((e['file_name'], e['sent_index']) for e in sel)) == 6
    for e in sel:
        assert list(e['rules']) == ['detector', 'oracle', 'speaker', 'rerank@0.5']
        assert all(set(c) == {'det', 'category_id', 'hit', 'I', 'U', 'key'} for c in e['rules'].values())
    assert all({'I', 'U', 'hit', 'expr_logprob'} <= set(p) for p in dets)
    for name in ('detector', 'oracle', 'speaker', 'rerank@0.5'):
        assert 'rule %s' % name in printed
