"""Every instance per sentence (model/detect_device.py, csrc/detect.hip, l2s_rle_from_masks) against the numpy restatement of the
reference's test.py:268-297 (tests/detect_util.py), the host paste (utils/mask_utils.recover_masks) and the single-mask encoder.
The NMS decisions are compared bit-exact on the device's own decoded boxes (boxes_dump); the decode itself is compared with the host's
separately (bit for bit with zero size deltas, within _box_close's 4 ulp otherwise: numpy's float32 exp is not correctly rounded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import data as OD
import detect_util as DU
from test_eval_device_gpu import _ListLoader, _synthetic_blobs, _box_close, make_case, host_eval
from test_rle_export_gpu import _Pool, _rand, _net, _same_result, _same_details, SENTINEL

pytestmark = pytest.mark.gpu
NMS = 0.3                                                       # cfg.TEST.NMS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _geom(im_info):
    scale = im_info[0][2]
    return scale, int(round(im_info[0][0] / scale)), int(round(im_info[0][1] / scale))


def _nms_dump(cp, bp, rois, nkeep, post, C, im_info, thresh):
    """l2s_detect_nms on device tensors -> (ws, boxes_dump [post][C][4] on the host)"""
    from lang2seg_amd import ops as O
    scale, ih, iw = _geom(im_info)
    ws = torch.empty(((O.detect_ws_bytes(post, C) + 3) // 4,), dtype=torch.int32, device='cuda')
    dump = torch.full((post, C, 4), -7.0, dtype=torch.float32, device='cuda')
    O.detect_nms(cp, bp, rois, nkeep, post, C, scale, ih, iw, True, thresh, NMS, ws, dump)
    return ws, dump.cpu().numpy()


def _select(ws, post, C, max_per_image, scale, cap):
    """l2s_detect_select into sentinel-filled buffers of cap + 2 rows -> host (rec [cap + 2][8], count, mask_rois, mask_labels)"""
    from lang2seg_amd import ops as O
    rec = torch.full((cap + 2, 8), SENTINEL, dtype=torch.int32, device='cuda')
    roi = torch.full((cap + 2, 5), -3.0, dtype=torch.float32, device='cuda')
    lab = torch.full((cap + 2,), SENTINEL, dtype=torch.int32, device='cuda')
    count = torch.full((2,), SENTINEL, dtype=torch.int32, device='cuda')
    O.detect_select(ws, post, C, max_per_image, scale, rec, roi, lab, cap, count)
    return rec.cpu().numpy(), count.cpu().numpy(), roi.cpu().numpy(), lab.cpu().numpy()


def _assert_select(got, yard, cap, scale, tag):
    """records, order, count, mask RoIs and labels equal the yardstick's first `cap`; rows behind `written` are zero; nothing behind cap"""
    from lang2seg_amd import ops as O
    rec, count, mroi, mlab = got
    y_roi, y_cls, y_score, y_box = yard
    total = y_roi.size
    written = min(total, cap)
    assert (int(count[0]), int(count[1])) == (written, total), (tag, count, total, cap)
    roi, cls, box, score, area = O.det_record_fields(rec)
    assert np.array_equal(roi[:written], y_roi[:written]) and np.array_equal(cls[:written], y_cls[:written]), tag
    assert np.array_equal(score[:written].view(np.int32), y_score[:written].view(np.int32)), tag
    assert np.array_equal(box[:written].view(np.int32), y_box[:written].view(np.int32)), tag
    assert (area[:cap] == 0).all(), tag
    assert np.array_equal(mlab[:written], y_cls[:written]) and (mroi[:written, 0] == 0).all(), tag
    assert np.array_equal(mroi[:written, 1:].view(np.int32), (y_box[:written] * np.float32(scale)).astype(np.float32).view(np.int32)), tag
    assert (rec[written:cap] == 0).all() and (mroi[written:cap] == 0).all() and (mlab[written:cap] == 0).all(), tag
    assert (rec[cap:] == SENTINEL).all() and (mroi[cap:] == -3.0).all() and (mlab[cap:] == SENTINEL).all(), tag


def _run_case(c, post, C, tag):
    """one generated case: decode against the host, then NMS + select against the yardstick on the device's own boxes, at a cap with
    room to spare and at a cap below the total"""
    from lang2seg_amd.model.test import detect_from_outputs
    n, im_info = c['n'], c['im_info']
    scale = im_info[0][2]
    nk = None if c['nkeep_null'] else torch.tensor([n], dtype=torch.int32, device='cuda')
    assert nk is not None or n == post
    ws, dump = _nms_dump(_dev(c['cls_prob']), _dev(c['bbox_pred']), _dev(c['rois']), nk, post, C, im_info, c['thresh'])
    _, hb = detect_from_outputs(c['cls_prob'][:n], c['bbox_pred'][:n], c['rois'][:n], im_info)
    hb = hb.reshape(n, C, 4)
    if c['exact']:
        assert np.array_equal(dump[:n].view(np.int32), hb.view(np.int32)), tag
    else:
        assert DU.boxes_close(dump[:n], hb).all(), tag
        flat_d, flat_h = dump[:n].reshape(-1, 4), hb.reshape(-1, 4)
        assert all(_box_close(flat_d[i], flat_h[i]) for i in range(0, flat_d.shape[0], 97)), tag      # the criterion's own text on a sample
    yard = DU.detect_yardstick(c['cls_prob'][:n], dump[:n], c['thresh'], NMS, c['max_per_image'])
    total = yard[0].size
    _assert_select(_select(ws, post, C, c['max_per_image'], scale, total + 3), yard, total + 3, scale, tag)
    if total >= 2:
        cap = max(1, total // 2)
        _assert_select(_select(ws, post, C, c['max_per_image'], scale, cap), yard, cap, scale, tag + ('cap', cap))
    return total


@pytest.mark.parametrize('post', [1, 63, 64, 65, 300])
def test_nms_select_vs_yardstick(post):
    """ten seeded cases per proposal count at C = 81 (three image geometries, nkeep < post with 2.0 in the padding rows or NULL, clustered
    RoIs, quantised / sharpened scores, thresh in {0, 0.05, 0.5, 0.95}, max_per_image in {100, 100, 1, 0, 17})"""
    rs = DU.case_rng(post)
    totals = [_run_case(DU.make_inputs(rs, k, post, 81), post, 81, (post, k)) for k in range(10)]
    assert max(totals) > 0


@pytest.mark.parametrize('post,C,k', [(1000, 3, 5), (5000, 3, 0), (64, 2, 3)])
def test_nms_select_large_and_two_classes(post, C, k):
    """post = 1000 and cfg.TEST.RPN_TOP_N = 5000 (case 0: every row a candidate of both classes, thresh 0, so the order is an 8192-slot
    sort and the boxes leave the LDS) with three classes, and a two-class case"""
    rs = DU.case_rng(post + C)
    c = DU.make_inputs(rs, k, post, C)
    if post == 5000:
        assert c['nkeep_null'] and c['thresh'] == 0.0 and int((c['cls_prob'][:, 1] > 0).sum()) > 4096
    assert _run_case(c, post, C, (post, C, k)) > 0


def test_nms_select_special_scores_and_bad_arguments():
    """NaN scores are no candidates, -0.0 ties +0.0 (thresh < 0); sizes and pointers the kernels do not support give L2SError"""
    from lang2seg_amd import _lib, ops as O
    rs = np.random.RandomState(3)
    post, C = 65, 4
    c = DU.make_inputs(rs, 4, post, C)                           # thresh 0, limit 17, nkeep NULL
    cp = c['cls_prob']
    cp[::3, 1] = np.nan; cp[1::7, 2] = np.nan
    cp[::2, 3] = 0.0; cp[1::4, 3] = -0.0
    for thresh, mpi in ((0.0, 17), (-1.0, 0), (-1.0, 30)):
        ws, dump = _nms_dump(_dev(cp), _dev(c['bbox_pred']), _dev(c['rois']), None, post, C, c['im_info'], thresh)
        with np.errstate(invalid='ignore'):
            yard = DU.detect_yardstick(cp, dump, thresh, NMS, mpi)
        assert yard[0].size > 0 and not np.isnan(yard[2]).any()
        _assert_select(_select(ws, post, C, mpi, c['im_info'][0][2], yard[0].size + 1), yard, yard[0].size + 1, c['im_info'][0][2], (thresh, mpi))
    t = torch.zeros((5200 * 8,), dtype=torch.float32, device='cuda')
    ws = torch.zeros((O.detect_ws_bytes(5120, 3) // 4 + 1,), dtype=torch.int32, device='cuda')
    a, w = t.data_ptr(), ws.data_ptr()
    good = [a, a, a, None, 64, 3, 1.0, 100, 100, 1, 0.0, 0.3, w, None, None]
    _lib.call('l2s_detect_nms', *good)
    for idx, v in [(4, 0), (4, 5121), (5, 1), (5, 1025), (0, None), (2, None), (1, None), (12, None), (6, 0.0), (7, 0), (10, float('nan'))]:
        args = list(good); args[idx] = v
        with pytest.raises(_lib.L2SError):
            _lib.call('l2s_detect_nms', *args)
    good = [w, 64, 3, 100, 1.0, a, a + 4096, a + 8192, 16, a + 12288, None]
    _lib.call('l2s_detect_select', *good)
    for idx, v in [(0, None), (1, 5121), (2, 1), (4, 0.0), (5, None), (6, None), (7, None), (8, 0), (9, None)]:
        args = list(good); args[idx] = v
        with pytest.raises(_lib.L2SError):
            _lib.call('l2s_detect_select', *args)
    good = [a, 14, a + 65536, a + 12288, 4, 8, 8, a + 32768, None]
    for idx, v in [(0, None), (1, 17), (2, None), (3, None), (4, 0), (4, 65536), (5, 0), (7, None)]:
        args = list(good); args[idx] = v
        with pytest.raises(_lib.L2SError):
            _lib.call('l2s_detect_paste', *args)
    torch.cuda.synchronize()
    assert _lib.load().l2s_detect_ws_bytes(0, 3) == 0


class _FixedSize(object):
    """a RandomState whose first two choice() calls - make_case's canvas size - return the given size"""

    def __init__(self, rs, ih, iw):
        self._rs, self._q = rs, [ih, iw]

    def choice(self, a):
        return self._q.pop(0) if self._q else self._rs.choice(a)

    def __getattr__(self, k):
        return getattr(self._rs, k)


@pytest.mark.parametrize('ih,iw', [(101, 99), (240, 320)])
def test_batched_paste(ih, iw):
    """37 make_case boxes and masks on one canvas size, device count 29, canvases pre-filled with 7: the first 29 equal
    recover_masks(...) > 122 pixel for pixel and area is their sum; the last 8 are untouched with area 0"""
    from lang2seg_amd import ops as O
    rs = np.random.RandomState(100 + ih)
    N, NV = 37, 29
    cases = [make_case(_FixedSize(rs, ih, iw), k) for k in range(N)]
    assert all(c[2] == ih and c[3] == iw for c in cases)
    rec = np.zeros((N, 8), np.int32)
    for k, c in enumerate(cases):
        rec[k, 0], rec[k, 1] = k, 1 + k % 5
        rec[k, 2:6] = c[1].view(np.int32)
    rec_d = _dev(rec)
    prob = _dev(np.stack([c[0] for c in cases]))
    count = torch.tensor([NV, NV + 5], dtype=torch.int32, device='cuda')
    canv = torch.full((N, ih, iw), 7, dtype=torch.uint8, device='cuda')
    O.detect_paste(prob, rec_d, count, ih, iw, canv)
    got, rec_h = canv.cpu().numpy(), rec_d.cpu().numpy()
    assert np.array_equal(rec_h[:, :7], rec[:, :7])
    areas = []
    for k, c in enumerate(cases[:NV]):
        pred = host_eval(c[0], c[1], ih, iw, c[4])[0]
        assert np.array_equal(got[k], pred), k
        assert int(rec_h[k, 7]) == int(pred.sum()), k
        areas.append(int(pred.sum()))
    assert (got[NV:] == 7).all() and (rec_h[NV:, 7] == 0).all()
    assert sum(a > 0 for a in areas) > 10


def _encode_batch(masks, n_valid, pool_words):
    """l2s_rle_from_masks on a sentinel-filled pool -> host (pool, cursor, spans [n][2])"""
    from lang2seg_amd import ops as O
    n, h, w = masks.shape
    pool = torch.full((max(pool_words, 1),), SENTINEL, dtype=torch.int32, device='cuda')[:pool_words]
    cursor = torch.zeros((1,), dtype=torch.int32, device='cuda')
    spans = torch.full((n, 2), SENTINEL, dtype=torch.int32, device='cuda')
    ws = torch.empty((n * O.rle_encode_ws_words(h, w),), dtype=torch.int32, device='cuda')
    O.rle_from_masks(_dev(masks), torch.tensor([n_valid], dtype=torch.int32, device='cuda'), pool, cursor, spans, ws)
    return pool.cpu().numpy().view('<u4'), int(cursor.cpu()[0]), spans.cpu().numpy()


def _encode_single(masks, n_valid, pool_words):
    """n_valid consecutive l2s_rle_from_mask calls on one pool -> host (pool, cursor, spans)"""
    p = _Pool(pool_words, spans=max(n_valid, 1))
    for m in masks[:n_valid]:
        p.encode(m)
    pool, cursor, spans = p.host()
    return pool, cursor, spans


def _assert_batch_equals_single(masks, n_valid, pool_words, tag):
    pool, cursor, spans = _encode_batch(masks, n_valid, pool_words)
    pool1, cursor1, spans1 = _encode_single(masks, n_valid, pool_words)
    assert cursor == cursor1 and [tuple(int(v) for v in s) for s in spans[:n_valid]] == spans1, (tag, cursor, cursor1, spans[:n_valid], spans1)
    assert np.array_equal(pool, pool1), tag
    assert (spans[n_valid:] == 0).all(), tag
    return pool, cursor, spans


def test_batched_encoder_decomposition_boundaries():
    """three masks per call (dense, sparse, empty) at the widths across the lane / workgroup boundaries x the heights across the chunk
    boundaries of test_encoder_decomposition_boundaries: pool bytes, spans and cursor equal consecutive l2s_rle_from_mask calls and
    the oracle's counts"""
    from lang2seg_amd import ops as O
    R = O.rle_encode_chunk_rows()
    rs = np.random.RandomState(7)
    heights = sorted(set([1, 7, 8, 9, 255, 256, 257, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1]))
    sizes = [(h, w) for w in (63, 64, 65, 257) for h in heights] + [(3, 1025), (2 * R + 5, 1030)]
    for h, w in sizes:
        masks = np.stack([_rand(rs, h, w), _rand(rs, h, w, 0.02), np.zeros((h, w), np.uint8)])
        refs = [OD.rle_encode(m) for m in masks]
        total = sum(len(r) for r in refs)
        pool, cursor, spans = _assert_batch_equals_single(masks, 3, total + 4, (h, w))
        assert cursor == total and np.array_equal(pool[:total], np.concatenate(refs)) and (pool[total:] == SENTINEL).all(), (h, w)


def test_batched_encoder_count_overflow_and_repeat():
    rs = np.random.RandomState(19)
    masks = np.stack([_rand(rs, 130, 70, d) for d in (0.5, 0.1, 0.5, 0.02, 0.3)])
    refs = [OD.rle_encode(m) for m in masks]
    lens = [len(r) for r in refs]
    # n_valid < n: the masks behind it are skipped with span (0, 0)
    for nv in (0, 1, 3):
        pool, cursor, spans = _assert_batch_equals_single(masks, nv, sum(lens) + 2, ('n_valid', nv))
        assert cursor == sum(lens[:nv])
    # a pool one word short for mask 2: its span is (-1, n), the cursor does not move and masks 3, 4 pack behind mask 1
    words = lens[0] + lens[1] + lens[2] - 1
    assert lens[3] + lens[4] <= lens[2] - 1
    pool, cursor, spans = _assert_batch_equals_single(masks, 5, words, 'short')
    off = np.concatenate([[0], np.cumsum([lens[0], lens[1], lens[3], lens[4]])])
    assert [tuple(int(v) for v in s) for s in spans] == [(0, lens[0]), (int(off[1]), lens[1]), (-1, lens[2]), (int(off[2]), lens[3]), (int(off[3]), lens[4])]
    assert cursor == int(off[4]) and np.array_equal(pool[:cursor], np.concatenate([refs[0], refs[1], refs[3], refs[4]]))
    assert (pool[cursor:] == SENTINEL).all()
    # two runs give identical bytes
    a = _encode_batch(masks, 5, sum(lens) + 2); b = _encode_batch(masks, 5, sum(lens) + 2)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and a[2].tobytes() == b[2].tobytes()
    from lang2seg_amd import _lib
    t = torch.zeros((4096,), dtype=torch.int32, device='cuda')
    a0 = t.data_ptr()
    good = [a0, 2, a0 + 64, 4, 4, a0 + 128, 16, a0 + 256, a0 + 320, a0 + 512, None]
    _lib.call('l2s_rle_from_masks', *good)
    for idx, v in [(0, None), (1, 0), (1, 65536), (2, None), (3, 0), (4, -1), (5, None), (6, -1), (7, None), (8, None), (9, None)]:
        args = list(good); args[idx] = v
        with pytest.raises(_lib.L2SError):
            _lib.call('l2s_rle_from_masks', *args)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- network level
_SIZES = [(224, 288), (256, 352)]


def _strip(blob):
    return {k: v for k, v in blob.items() if not k.startswith('gt_') and k != 'labels'}


def _yard_of_capture(cap, im_info, thresh, max_per_image):
    """the yardstick on one sentence's own head outputs (device copies), with the device's own decoded boxes"""
    n = cap['post'] if cap['nkeep'] is None else int(cap['nkeep'].cpu()[0])
    C = cap['cls_prob'].shape[1]
    _, dump = _nms_dump(cap['cls_prob'], cap['bbox_pred'], cap['rois'], cap['nkeep'], cap['post'], C, im_info, thresh)
    return DU.detect_yardstick(cap['cls_prob'].cpu().numpy()[:n], dump[:n], thresh, NMS, max_per_image), n


def _assert_lists_vs_yardstick(lists, captured, blob, thresh, max_per_image, masks):
    """masks: True (every mask against the host paste), 'present' (only that they are there), False (a network without a mask branch)"""
    from lang2seg_amd.model.test import segment_from_mask_prob
    im_info = np.asarray(blob['im_info'], np.float32).reshape(1, 3)
    scale, ih, iw = _geom(im_info)
    n_det = 0
    for i, (lst, cap) in enumerate(zip(lists, captured)):
        (y_roi, y_cls, y_score, y_box), n = _yard_of_capture(cap, im_info, thresh, max_per_image)
        assert [(p['roi'], p['category_id']) for p in lst] == list(zip(y_roi.tolist(), y_cls.tolist())), i
        assert [p['score'] for p in lst] == [float(v) for v in y_score] and [p['box'] for p in lst] == [[float(v) for v in b] for b in y_box], i
        assert all(p['sent_index'] == i and p['file_name'] == blob['file_name'] for p in lst)
        n_det += len(lst)
        if not masks:
            assert all('segmentation' not in p and 'area' not in p for p in lst)
            continue
        assert all(p['segmentation']['size'] == [ih, iw] for p in lst)
        if masks == 'present':
            continue
        mp = cap['mask_prob'].cpu().numpy()
        for k, p in enumerate(lst):
            seg = p['segmentation']
            assert seg['size'] == [ih, iw]
            m = OD.rle_decode(OD.rle_from_string(seg['counts']), ih, iw)
            host = segment_from_mask_prob(mp[k][None].copy(), np.asarray(p['box'], np.float32), im_info)
            assert np.array_equal(m, host), (i, k)
            assert p['area'] == int(host.sum()), (i, k)
    return n_det


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_detect_image_network(dtype):
    from lang2seg_amd import ops as O
    from lang2seg_amd.model import detect_device as DD, eval_device as ED
    from lang2seg_amd.model.config import cfg
    from lang2seg_amd.model.eval_device import eval_split_device
    from lang2seg_amd.model.predict_device import predict_image
    from lang2seg_amd.model.test import best_detection
    assert float(cfg.TEST.NMS) == NMS and cfg.TEST.BBOX_REG
    net = _net('cycle', dtype)
    blobs = _synthetic_blobs(_SIZES, 3)
    flat = []
    for blob in blobs:
        labels = np.asarray(blob['labels'])
        captured = []
        lists = DD.detect_image(net, _strip(blob), labels, _capture=captured)
        assert len(lists) == 3 and len(captured) == 3 and all('rerun' not in c for c in captured)
        assert _assert_lists_vs_yardstick(lists, captured, blob, 0.0, 100, True) > 3
        flat += [p for lst in lists for p in lst]
        # the one-box pick is in the list, with the same box and score bits
        picks = predict_image(net, _strip(blob), labels)
        found = 0
        for i, (q, cap) in enumerate(zip(picks, captured)):
            n = cap['post'] if cap['nkeep'] is None else int(cap['nkeep'].cpu()[0])
            r, c, _ = best_detection(cap['cls_prob'].cpu().numpy()[:n], np.zeros((n, 4 * cap['cls_prob'].shape[1]), np.float32))
            assert int(c) == q['category_id']
            if c >= 1:
                hit = [p for p in lists[i] if (p['roi'], p['category_id']) == (int(r), int(c))]
                assert len(hit) == 1 and hit[0]['box'] == q['box'] and hit[0]['score'] == q['score'], (i, hit, q)
                found += 1
        assert found >= 2
        # a cap of one row and a pool of one word: the same lists through the re-run
        for kw in (dict(_cap=1), dict(_pool_words=1)):
            cap2 = []
            again = DD.detect_image(net, _strip(blob), labels, _capture=cap2, **kw)
            assert any('rerun' in c for c in cap2), kw
            assert again == lists, kw
        # another threshold and limit, no limit at all
        for thresh, mpi in ((0.05, 3), (0.02, 0)):
            captured = []
            lists2 = DD.detect_image(net, _strip(blob), labels, max_per_image=mpi, thresh=thresh, _capture=captured)
            captured = [c for c in captured if 'rerun' not in c]
            _assert_lists_vs_yardstick(lists2, captured, blob, thresh, mpi, 'present')
    # evaluation with detections: the same metrics and details, and the lists of detect_image
    det0, det1, dets = [], [], []
    res0 = eval_split_device(_ListLoader(blobs), net, None, 'val', dict(verbose=False), details=det0)
    res1 = eval_split_device(_ListLoader(blobs), net, None, 'val', dict(verbose=False), details=det1, detections=dets)
    assert _same_result(res0, res1) and _same_details(det0, det1)
    assert dets == flat
    if dtype != 'f32':
        return
    # detect_sentence on its own: the first detection's mask probabilities against the n = 1 mask head on the same box
    blob = blobs[0]
    net.eval()
    img, lab_d, lens, _, _ = ED._upload_image(net, blob, 3)
    im_info = np.asarray(blob['im_info'], dtype=np.float32).reshape(-1)[:3]
    scale, ih, iw = ED._geometry(im_info)
    d = dict(data=img, im_info=im_info, S=1)
    net.forward_test_image(d)
    d['labels'] = lab_d[0, :lens[0]]; d['T'] = lens[0]
    s = net.forward_test_sentence(d)
    out = DD.detect_sentence(net, s, scale, ih, iw, 100, 0.0, 128)
    assert int(out['count'].cpu()[0]) >= 1
    many = out['mask_prob'][0].cpu().numpy().copy()
    roi, cls, box, score, area = O.det_record_fields(out['rec'].cpu())
    r1 = torch.zeros((1, 5), dtype=torch.float32, device='cuda')
    r1[0, 1:] = torch.from_numpy((box[0] * np.float32(scale)).astype(np.float32)).cuda()
    l1 = torch.tensor([int(cls[0])], dtype=torch.int32, device='cuda')
    Hc, Wc = s['net_conv_hw']
    one = net.predict_mask_device(s['net_conv'], Hc, Wc, r1, l1).view(14, 14).cpu().numpy()
    assert np.abs(one - many).max() <= 1e-4, np.abs(one - many).max()


def test_detect_image_vgg_boxes_only():
    from lang2seg_amd.model import detect_device as DD
    from lang2seg_amd.model.eval_device import eval_split_vgg_device
    net = _net('vgg', 'bf16')
    blobs = _synthetic_blobs(_SIZES, 2)
    flat = []
    for blob in blobs:
        captured = []
        lists = DD.detect_image(net, _strip(blob), np.asarray(blob['labels']), _capture=captured)
        assert len(lists) == 2
        assert _assert_lists_vs_yardstick(lists, captured, blob, 0.0, 100, False) > 2
        assert all(set(p) == {'file_name', 'sent_index', 'roi', 'category_id', 'box', 'score'} for lst in lists for p in lst)
        assert DD.detect_image(net, _strip(blob), np.asarray(blob['labels']), _cap=1) == lists
        flat += [p for lst in lists for p in lst]
    dets = []
    res0 = eval_split_vgg_device(_ListLoader(blobs), net, None, 'val', dict(verbose=False))
    res1 = eval_split_vgg_device(_ListLoader(blobs), net, None, 'val', dict(verbose=False), detections=dets)
    assert res0 == res1 and dets == flat


def test_eval_tool_dumps_detections(tmp_path):
    """tools/eval.py --device_eval 1 --dump_detections in a child process: valid JSON, every mask's counts cover the canvas"""
    path = str(tmp_path / 'det.json')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'eval.py'), '--synthetic', '1', '--allow_init_weights', '1', '--device_eval', '1',
           '--synthetic_images', '2', '--verbose', '0', '--results_dir', str(tmp_path), '--dump_detections', path]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    dets = json.load(open(path))
    assert len(set((p['file_name'], p['sent_index']) for p in dets)) == 6
    for p in dets:
        assert set(p) == {'file_name', 'sent_index', 'roi', 'category_id', 'box', 'score', 'area', 'segmentation'}
        h, w = p['segmentation']['size']
        assert (h, w) == (375, 625) and 1 <= p['category_id'] <= 80
        cnts = OD.rle_from_string(p['segmentation']['counts'])
        assert int(cnts.sum()) == h * w and int(cnts[1::2].sum()) == p['area']
    bad = subprocess.run(cmd[:2] + ['--synthetic', '1', '--dump_detections', path], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert bad.returncode != 0 and 'device_eval' in bad.stderr
