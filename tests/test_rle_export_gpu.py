"""Prediction export: the device run-length encoder l2s_rle_from_mask (csrc/rle_encode.hip) against the oracle's rle_encode (pinned to
the reference's maskApi.c by tests/golden/ref_rle.npz), the predictions of model/eval_device.py against its own details and the
canvases of l2s_eval_mask_iou, and model/predict_device.py against the evaluation of the same image."""
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
from data_util import load_rle_fixture
from test_eval_device_gpu import _ListLoader, _synthetic_blobs

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A


class _Pool(object):
    """a sentinel-filled pool with its cursor and one span per encode"""

    def __init__(self, words, spans=1):
        self.pool = torch.full((max(words, 1),), SENTINEL, dtype=torch.int32, device='cuda')[:words]
        self.cs = torch.zeros((1 + 2 * spans,), dtype=torch.int32, device='cuda')
        self.k = 0

    def encode(self, m):
        from lang2seg_amd import ops as O
        md = torch.from_numpy(np.ascontiguousarray(m, dtype=np.uint8)).cuda()
        ws = torch.empty((O.rle_encode_ws_words(*m.shape),), dtype=torch.int32, device='cuda')
        O.rle_from_mask(md, self.pool, self.cs[0:1], self.cs[1 + 2 * self.k:3 + 2 * self.k], ws)
        self.k += 1

    def host(self):
        cs = self.cs.cpu().numpy()
        return self.pool.cpu().numpy().view('<u4'), int(cs[0]), [(int(cs[1 + 2 * j]), int(cs[2 + 2 * j])) for j in range(self.k)]


def _check(m, ref=None, slack=5):
    """one mask alone on a fresh pool: span, cursor, counts and string equal the oracle's; no word behind the counts is written"""
    from lang2seg_amd import ops as O
    ref = OD.rle_encode(m) if ref is None else np.asarray(ref, np.uint32)
    p = _Pool(len(ref) + slack)
    p.encode(m)
    pool, cursor, spans = p.host()
    assert spans == [(0, len(ref))] and cursor == len(ref), (m.shape, spans, cursor, len(ref))
    assert np.array_equal(pool[:len(ref)], ref), m.shape
    assert (pool[len(ref):] == SENTINEL).all(), m.shape
    assert O.rle_to_string(pool[:len(ref)]) == OD.rle_to_string(ref)
    return pool[:len(ref)].copy()


def _rand(rs, h, w, density=0.5):
    return (rs.uniform(0, 1, (h, w)) < density).astype(np.uint8)


def test_encoder_reference_fixture():
    """every mask of ref_rle.npz against the reference's own counts and strings"""
    from lang2seg_amd import ops as O
    cases, _ = load_rle_fixture()
    assert len(cases) > 10
    for c in cases:
        got = _check(c['mask'], c['counts'])
        assert O.rle_to_string(got) == c['s']


def test_encoder_edge_masks():
    z, o = np.zeros((37, 41), np.uint8), np.ones((37, 41), np.uint8)
    first, last = z.copy(), z.copy()
    first[0, 0] = 1; last[-1, -1] = 1
    cb = (np.indices((37, 41)).sum(0) % 2).astype(np.uint8)
    rs = np.random.RandomState(3)
    masks = [np.zeros((1, 1), np.uint8), np.ones((1, 1), np.uint8), _rand(rs, 1, 65), _rand(rs, 65, 1), z, o, first, last, cb, 1 - cb,
             _rand(rs, 37, 41) * 255]                                              # nonzero = 1
    for m in masks:
        _check(m)
    assert len(_check(z)) == 1 and _check(z)[0] == 37 * 41
    assert list(_check(o)) == [0, 37 * 41] and list(_check(first)) == [0, 1, 37 * 41 - 1]
    assert len(_check(cb)) == 37 * 41 and len(_check(1 - cb)) == 37 * 41 + 1   # a column of odd height ends as the next one starts: every pixel a run


def test_encoder_decomposition_boundaries():
    """widths across the lane (64) and workgroup (256) boundaries x heights across the chunk (rows per lane) boundaries, random density 0.5,
    and column-constant masks whose only transitions are at y = 0 (the predecessor is the last row of the column to the left)"""
    from lang2seg_amd import ops as O
    R = O.rle_encode_chunk_rows()
    rs = np.random.RandomState(7)
    heights = sorted(set([1, 7, 8, 9, 255, 256, 257, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1]))
    for w in (63, 64, 65, 257):
        for h in heights:
            _check(_rand(rs, h, w))
    for h in (R, R + 1):
        cols = np.repeat(_rand(rs, 1, 257), h, axis=0)
        _check(cols)
        rows = np.repeat(_rand(rs, h, 1), 300, axis=1)
        _check(rows)
    _check(_rand(rs, 3, 1025))                                                   # more chunks than one pass of the scan's workgroup
    _check(_rand(rs, 2 * R + 5, 1030, density=0.02))                             # sparse: most chunks hold no transition


def test_encoder_480x640_and_round_trip():
    """~150k counts over many scan passes; two runs give identical bytes; rle_to_mask(rle_from_string(rle_to_string(counts))) is the input"""
    from lang2seg_amd import ops as O
    rs = np.random.RandomState(11)
    m = _rand(rs, 480, 640)
    ref = OD.rle_encode(m)
    assert len(ref) > 140000
    got = _check(m, ref)
    runs = []
    for _ in range(2):
        p = _Pool(len(ref) + 3)
        p.encode(m)
        torch.cuda.synchronize()
        runs.append((p.pool.cpu().numpy().tobytes(), p.cs.cpu().numpy().tobytes()))
    assert runs[0] == runs[1]
    for mm, cnts in ((m, got), (_rand(rs, 37, 41), None)):
        cnts = _check(mm) if cnts is None else cnts
        back = O.rle_from_string(O.rle_to_string(cnts))
        assert np.array_equal(back, cnts)
        h, w = mm.shape
        c = torch.from_numpy(back.view(np.int32)).cuda()
        offs = torch.tensor([0, back.size], dtype=torch.int32, device='cuda')
        ws = torch.empty((O.rle_ws_words(back.size, h, w),), dtype=torch.int32, device='cuda')
        out = torch.empty((h, w), dtype=torch.uint8, device='cuda')
        O.rle_to_mask(c, offs, 1, back.size, h, w, ws, out)
        assert np.array_equal(out.cpu().numpy(), mm)
    rle = O.mask_to_rle(torch.from_numpy(m).cuda())
    assert rle == dict(size=[480, 640], counts=OD.rle_to_string(ref))


def test_encoder_packs_one_pool():
    """three encodes on one stream and one pool: offsets accumulate, the cursor is the sum, the prefix is the concatenation"""
    rs = np.random.RandomState(13)
    masks = [_rand(rs, 70, 33), np.zeros((5, 9), np.uint8), _rand(rs, 129, 66, 0.3)]
    refs = [OD.rle_encode(m) for m in masks]
    total = sum(len(r) for r in refs)
    p = _Pool(total + 4, spans=3)
    for m in masks:
        p.encode(m)
    pool, cursor, spans = p.host()
    offs = np.concatenate([[0], np.cumsum([len(r) for r in refs])])
    assert spans == [(int(offs[j]), len(refs[j])) for j in range(3)]
    assert cursor == total
    assert np.array_equal(pool[:total], np.concatenate(refs)) and (pool[total:] == SENTINEL).all()


def test_encoder_overflow_leaves_pool_and_cursor():
    rs = np.random.RandomState(17)
    big, small = _rand(rs, 130, 70), _rand(rs, 9, 11)
    rb, rsm = OD.rle_encode(big), OD.rle_encode(small)
    # a pool one word short of the first encode
    p = _Pool(len(rb) - 1, spans=2)
    p.encode(big)
    pool, cursor, spans = p.host()
    assert spans == [(-1, len(rb))] and cursor == 0 and (pool == SENTINEL).all()
    p.encode(small)                                                              # the next one fits and starts where the cursor stayed
    pool, cursor, spans = p.host()
    assert spans[1] == (0, len(rsm)) and cursor == len(rsm)
    assert np.array_equal(pool[:len(rsm)], rsm) and (pool[len(rsm):] == SENTINEL).all()
    # behind a first encode: one word short of both
    p = _Pool(len(rsm) + len(rb) - 1, spans=3)
    for m in (small, big, small):
        p.encode(m)
    pool, cursor, spans = p.host()
    assert spans == [(0, len(rsm)), (-1, len(rb)), (len(rsm), len(rsm))] and cursor == 2 * len(rsm)
    assert np.array_equal(pool[:2 * len(rsm)], np.concatenate([rsm, rsm])) and (pool[2 * len(rsm):] == SENTINEL).all()
    # an exact fit is no overflow
    p = _Pool(len(rb))
    p.encode(big)
    pool, cursor, spans = p.host()
    assert spans == [(0, len(rb))] and np.array_equal(pool, rb)


def test_encoder_rejects_bad_arguments():
    from lang2seg_amd import _lib
    t = torch.zeros((64,), dtype=torch.int32, device='cuda')
    m = torch.zeros((4, 4), dtype=torch.uint8, device='cuda')
    a = t.data_ptr()
    good = [m.data_ptr(), 4, 4, a, 16, a + 128, a + 132, a + 160, None]
    bad = [(0, None), (3, None), (5, None), (6, None), (7, None), (1, 0), (1, -1), (2, 0), (2, -3)]
    for idx, v in bad:
        args = list(good); args[idx] = v
        with pytest.raises(_lib.L2SError):
            _lib.call('l2s_rle_from_mask', *args)
    args = list(good); args[1], args[2] = 65536, 32768                           # h * w = 2^31
    with pytest.raises(_lib.L2SError):
        _lib.call('l2s_rle_from_mask', *args)
    assert _lib.load().l2s_rle_encode_ws_words(0, 5) == 0


# ---------------------------------------------------------------- predictions
_SIZES = [(224, 288), (256, 352), (288, 224)]


def _net(variant, dtype):
    from lang2seg_amd import selftest
    from oracle import weights as OW
    opt = OW.default_opt(vocab_size=60, seq_length=6)
    if variant == 'vgg':
        opt['C4_feat_dim'] = 512
    return selftest.build_net(opt, {}, dtype, OW.make_state_dict(opt, seed=3, head_gain=4.0, variant=variant), variant=variant)


def _canvases(net, blob, S):
    """the canvas l2s_eval_mask_iou dumps for each sentence of one image, through the kernels' own entry points"""
    from lang2seg_amd import ops as O
    from lang2seg_amd.model import eval_device as ED
    from lang2seg_amd.model.config import cfg
    net.eval()
    img, lab_d, lens, box_d, gm = ED._upload_image(net, blob, S)
    im_info = np.asarray(blob['im_info'], dtype=np.float32).reshape(-1)[:3]
    scale, ih, iw = ED._geometry(im_info)
    d = dict(data=img, im_info=im_info, S=1)
    net.forward_test_image(d)
    rec = O.eval_records(S)
    roi = torch.zeros((1, 5), dtype=torch.float32, device='cuda'); lab = torch.zeros((1,), dtype=torch.int32, device='cuda')
    MS = int(cfg.MASK_SIZE)
    out = []
    for i in range(S):
        d['labels'] = lab_d[i, :lens[i]]; d['T'] = lens[i]
        s = net.forward_test_sentence(d)
        O.eval_pick(s['cls_prob'], s['bbox_pred'], s['rois'], s['nkeep'], s['post'], net._num_classes, scale, ih, iw, box_d[i],
                    cfg.TEST.BBOX_REG, rec, i, roi, lab)
        Hc, Wc = s['net_conv_hw']
        mprob = net.predict_mask_device(s['net_conv'], Hc, Wc, roi, lab).view(MS, MS)
        cv = torch.full((ih, iw), 7, dtype=torch.uint8, device='cuda')
        O.eval_mask_iou(mprob, rec, i, gm[i], ih, iw, canvas=cv)
        r, c = (int(v) for v in rec.view(torch.int32)[i, :2].cpu())
        out.append((cv.cpu().numpy(), float(s['cls_prob'][r, c])))
    return out


def _same_result(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _same_details(a, b):
    return len(a) == len(b) and all(x[:2] == y[:2] and np.array_equal(x[2], y[2]) and x[3:] == y[3:] for x, y in zip(a, b))


@pytest.mark.parametrize('variant,dtype', [('cycle', 'f32'), ('cycle', 'bf16'), ('spatial', 'f32'), ('spatial', 'bf16')])
def test_predictions_of_device_evaluation(variant, dtype):
    from lang2seg_amd.model.eval_device import eval_split_device
    from lang2seg_amd.model.predict_device import predict_image
    from lang2seg_amd.utils.mask_utils import imresize
    net = _net(variant, dtype)
    blobs = _synthetic_blobs(_SIZES, 3)
    opt = dict(verbose=False)
    det0, det1, det2, preds, preds_fb = [], [], [], [], []
    res0 = eval_split_device(_ListLoader(blobs), net, None, 'val', opt, details=det0)
    res1 = eval_split_device(_ListLoader(blobs), net, None, 'val', opt, details=det1, predictions=preds)
    assert _same_result(res0, res1) and _same_details(det0, det1)
    assert len(preds) == 9
    for k, (p, d) in enumerate(zip(preds, det1)):
        j, i = divmod(k, 3)
        assert p['file_name'] == blobs[j]['file_name'] and p['sent_index'] == i
        assert p['category_id'] == d[1] and (p['hit'], p['I'], p['U']) == d[3:]
        assert np.array_equal(np.asarray(p['box'], np.float32), d[2])
    for j, blob in enumerate(blobs):
        ih, iw = int(round(_SIZES[j][0] / 1.6)), int(round(_SIZES[j][1] / 1.6))
        for i, (cv, score) in enumerate(_canvases(net, blob, 3)):
            p = preds[3 * j + i]
            seg = p['segmentation']
            assert seg['size'] == [ih, iw] == list(cv.shape)
            m = OD.rle_decode(OD.rle_from_string(seg['counts']), ih, iw)
            assert np.array_equal(m, cv), (j, i)
            g = imresize(blob['gt_masks'][i], size=(ih, iw), interp='nearest') != 0
            assert int((m.astype(bool) & g).sum()) == p['I'] and int((m.astype(bool) | g).sum()) == p['U']
            assert p['score'] == score
    # a pool of one word: every sentence overflows and comes back through the host encoder, the same predictions
    res2 = eval_split_device(_ListLoader(blobs), net, None, 'val', opt, details=det2, predictions=preds_fb, _pool_words=1)
    assert _same_result(res0, res2) and _same_details(det0, det2)
    assert preds_fb == preds
    # the same image without its annotations
    blob = {k: v for k, v in blobs[1].items() if not k.startswith('gt_') and k != 'labels'}
    out = predict_image(net, blob, np.asarray(blobs[1]['labels']))
    assert len(out) == 3
    for q, p in zip(out, preds[3:6]):
        assert set(q) == set(p) - {'hit', 'I', 'U'} | {'area'}
        assert all(q[k] == p[k] for k in ('file_name', 'sent_index', 'category_id', 'box', 'score', 'segmentation'))
        h, w = q['segmentation']['size']
        assert q['area'] == int(OD.rle_decode(OD.rle_from_string(q['segmentation']['counts']), h, w).sum())
    with pytest.raises(ValueError):
        predict_image(net, blob, np.zeros((1, 6), np.int64))


def test_predictions_vgg_boxes_only():
    from lang2seg_amd.model.eval_device import eval_split_vgg_device
    from lang2seg_amd.model.predict_device import predict_image
    net = _net('vgg', 'bf16')
    blobs = _synthetic_blobs(_SIZES[:2], 2)
    det0, det1, preds = [], [], []
    res0 = eval_split_vgg_device(_ListLoader(blobs), net, None, 'val', dict(verbose=False), details=det0)
    res1 = eval_split_vgg_device(_ListLoader(blobs), net, None, 'val', dict(verbose=False), details=det1, predictions=preds)
    assert res0 == res1 and _same_details(det0, det1) and len(preds) == 4
    for p, d in zip(preds, det1):
        assert 'segmentation' not in p
        assert p['category_id'] == d[1] and p['hit'] == d[3] and np.array_equal(np.asarray(p['box'], np.float32), d[2])
        assert 0.0 < p['score'] <= 1.0
    blob = {k: v for k, v in blobs[0].items() if not k.startswith('gt_') and k != 'labels'}
    out = predict_image(net, blob, np.asarray(blobs[0]['labels']))
    assert [(q['category_id'], q['box'], q['score']) for q in out] == [(p['category_id'], p['box'], p['score']) for p in preds[:2]]
    assert all('segmentation' not in q for q in out)


def test_eval_tool_dumps_predictions(tmp_path):
    """tools/eval.py --device_eval 1 --dump_predictions in a child process: valid JSON, one entry per sentence"""
    path = str(tmp_path / 'pred.json')
    cmd = [sys.executable, os.path.join(ROOT, 'tools', 'eval.py'), '--synthetic', '1', '--allow_init_weights', '1', '--device_eval', '1',
           '--synthetic_images', '2', '--verbose', '0', '--results_dir', str(tmp_path), '--dump_predictions', path]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    preds = json.load(open(path))
    assert len(preds) == 6 and [p['sent_index'] for p in preds] == [0, 1, 2, 0, 1, 2]
    for p in preds:
        assert set(p) == {'file_name', 'sent_index', 'category_id', 'box', 'score', 'hit', 'I', 'U', 'segmentation'}
        h, w = p['segmentation']['size']
        assert (h, w) == (375, 625)
        cnts = OD.rle_from_string(p['segmentation']['counts'])
        assert int(cnts.sum()) == h * w and int(cnts[1::2].sum()) >= p['I']
    bad = subprocess.run(cmd[:2] + ['--synthetic', '1', '--dump_predictions', path], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert bad.returncode != 0 and 'device_eval' in bad.stderr
