"""The detection path's yardstick (tests/detect_util.py) pinned on a case worked by hand, and the host side of the new entries."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import boxes as OB
import detect_util as DU

A = [0, 0, 9, 9]          # area 100
B = [0, 0, 9, 4]          # area 50, inside A: IoU = 50 / (100 + 50 - 50) = 0.5 exactly
F = [20, 20, 29, 29]      # far from both


def _hand_case():
    """three rows, classes 1 and 2.  Class 1: A (0.9) suppresses B (0.8) at IoU == threshold, F (0.5) stays.  Class 2: row 1 scores 0.0
    (not above thresh 0), rows 2 (0.7) and 0 (0.5) are far apart.  Survivors: 0.9, 0.5 | 0.7, 0.5."""
    scores = np.array([[0.3, 0.9, 0.5], [0.9, 0.8, 0.0], [0.1, 0.5, 0.7]], np.float32)
    boxes = np.zeros((3, 3, 4), np.float32)
    boxes[:, 1] = [A, B, F]
    boxes[:, 2] = [[40, 40, 49, 49], [40, 40, 49, 49], [60, 60, 69, 69]]
    return scores, boxes


def _rows(res):
    roi, cls, score, box = res
    return [(int(r), int(c), float(np.float32(s))) for r, c, s in zip(roi, cls, score)]


def test_yardstick_hand_worked_case():
    scores, boxes = _hand_case()
    f = lambda v: float(np.float32(v))
    # the IoU of A and B is exactly the threshold: cpu_nms (>=) suppresses B, gpu_nms (>) would not
    dets = np.array([A + [0.9], B + [0.8]], np.float32)
    assert list(OB.nms(dets, 0.5, 'ge')) == [0] and list(OB.nms(dets, 0.5, 'gt')) == [0, 1]
    everything = [(0, 1, f(0.9)), (2, 1, f(0.5)), (2, 2, f(0.7)), (0, 2, f(0.5))]
    assert _rows(DU.detect_yardstick(scores, boxes, 0.0, 0.5, 0)) == everything            # no limit
    assert _rows(DU.detect_yardstick(scores, boxes, 0.0, 0.5, 4)) == everything            # not more than the limit
    # four survivors, limit three: image_thresh = 0.5 and both 0.5s stay (a tie at the threshold makes the result longer than the limit)
    assert _rows(DU.detect_yardstick(scores, boxes, 0.0, 0.5, 3)) == everything
    assert _rows(DU.detect_yardstick(scores, boxes, 0.0, 0.5, 2)) == [(0, 1, f(0.9)), (2, 2, f(0.7))]
    assert _rows(DU.detect_yardstick(scores, boxes, 0.0, 0.5, 1)) == [(0, 1, f(0.9))]
    # thresh is strict; a higher NMS threshold lets B through, in score order behind A
    assert _rows(DU.detect_yardstick(scores, boxes, 0.5, 0.5, 0)) == [(0, 1, f(0.9)), (2, 2, f(0.7))]
    assert _rows(DU.detect_yardstick(scores, boxes, 0.0, 0.6, 0))[:3] == [(0, 1, f(0.9)), (1, 1, f(0.8)), (2, 1, f(0.5))]
    roi, cls, score, box = DU.detect_yardstick(scores, boxes, 0.0, 0.5, 0)
    assert box.dtype == np.float32 and np.array_equal(box, np.array([A, F, [60, 60, 69, 69], [40, 40, 49, 49]], np.float32))
    # ties inside a class go to the lower row; a NaN score is no candidate
    s2 = np.array([[0, 0.5], [0, 0.5], [0, np.nan]], np.float32)
    b2 = np.zeros((3, 2, 4), np.float32); b2[:, 1] = [F, A, B]
    assert _rows(DU.detect_yardstick(s2, b2, 0.0, 0.5, 0)) == [(0, 1, 0.5), (1, 1, 0.5)]
    assert _rows(DU.detect_yardstick(np.zeros((4, 3), np.float32), np.zeros((4, 3, 4), np.float32), 0.0, 0.5, 100)) == []


def test_generator_reaches_every_branch():
    """the GPU cases' generator through the yardstick alone (host decode): suppression, empty results, results of one, tie overflow"""
    from lang2seg_amd.model.test import detect_from_outputs
    C = 81
    seen = dict(suppressed=0, empty=0, one=0, overflow=0, unlimited=0)
    for post, k in [(p, k) for p in (1, 63) for k in range(10)]:     # the first twenty cases of tests/test_detect_gpu.py
        rs = DU.case_rng(post) if k == 0 else rs
        c = DU.make_inputs(rs, k, post, C)
        n = c['n']
        scores, boxes = detect_from_outputs(c['cls_prob'][:n], c['bbox_pred'][:n], c['rois'][:n], c['im_info'])
        roi, cls, score, box = DU.detect_yardstick(scores, boxes, c['thresh'], 0.3, c['max_per_image'])
        free = DU.detect_yardstick(scores, boxes, c['thresh'], 0.3, 0)[0].size
        seen['suppressed'] += int((scores[:, 1:] > c['thresh']).sum()) > free
        seen['empty'] += roi.size == 0
        seen['one'] += roi.size == 1
        seen['overflow'] += c['max_per_image'] > 0 and roi.size > c['max_per_image']
        seen['unlimited'] += c['max_per_image'] == 0 and roi.size > 100
        assert (np.diff(cls) >= 0).all()
    assert all(v > 0 for v in seen.values()), seen


def test_new_entries_are_declared_and_bound():
    from lang2seg_amd import _lib, ops as O
    from lang2seg_amd.model import detect_device as DD
    hdr = open(os.path.join(ROOT, 'include/lang2seg_hip.h')).read()
    for name in ('l2s_detect_ws_bytes', 'l2s_detect_nms', 'l2s_detect_select', 'l2s_detect_paste', 'l2s_rle_from_masks'):
        assert name in _lib.SIGS and re.search(r'\b%s\s*\(' % name, hdr), name
    assert re.search(r'int roi; int cls; float box\[4\]; float score; int area; \} l2s_det_record;', hdr) and O.DET_RECORD_BYTES == 32
    assert [DD.default_cap(m) for m in (100, 64, 1, 0, -1)] == [128, 64, 64, 512, 512]
    rec = np.zeros((2, 8), np.int32)
    rec[1] = [5, 7, 0, 0, 0, 0, 0, 11]
    rec[1, 2:6] = np.array([1, 2, 3, 4], np.float32).view(np.int32); rec[1, 6:7] = np.array([0.25], np.float32).view(np.int32)
    roi, cls, box, score, area = O.det_record_fields(rec)
    assert (roi[1], cls[1], score[1], area[1]) == (5, 7, 0.25, 11) and list(box[1]) == [1, 2, 3, 4]
