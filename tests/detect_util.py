"""The yardstick of the detection path (model/detect_device.py, csrc/detect.hip): a numpy restatement of the reference's
pyutils/mask-faster-rcnn/lib/model/test.py:268-297 (threshold per class, NMS per class with cfg.TEST.NMS through cpu_nms, max_per_image
over all classes) on oracle.boxes.nms(..., 'ge') and stable_desc_order, and the generator of its GPU cases.  Nothing here reads the
code under test."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import boxes as OB

GEOMETRIES = [(600, 800, 1.6), (601, 999, 0.9375), (333, 500, 1.0)]      # test_pick_kernel_vs_host's
THRESH = [0.0, 0.05, 0.5, 0.95]
MAX_PER_IMAGE = [100, 100, 1, 0, 17]


def detect_yardstick(scores, boxes, thresh, nms_thresh, max_per_image):
    """scores float32 [n][C], boxes float32 [n][C][4] -> (roi, cls, score, box) arrays of the detections in the order the reference
    stacks them: class ascending, inside a class score descending with ties by lower row."""
    scores = np.asarray(scores, np.float32)
    n, C = scores.shape
    boxes = np.asarray(boxes, np.float32).reshape(n, C, 4)
    all_rows, all_dets = {}, {}
    for j in range(1, C):                                       # :269-277 (j = 0 is the background class)
        inds = np.where(scores[:, j] > np.float32(thresh))[0]   # (a NaN score compares false)
        cls_dets = np.hstack((boxes[inds, j], scores[inds, j][:, np.newaxis])).astype(np.float32, copy=False)
        keep = OB.nms(cls_dets, nms_thresh, 'ge') if cls_dets.size > 0 else np.zeros((0,), np.int64)
        all_dets[j] = cls_dets[keep, :]
        all_rows[j] = inds[keep]
    if max_per_image > 0:                                       # :280-290
        image_scores = np.hstack([all_dets[j][:, -1] for j in range(1, C)]) if C > 1 else np.zeros((0,), np.float32)
        if len(image_scores) > max_per_image:
            image_thresh = np.sort(image_scores)[-max_per_image]
            for j in range(1, C):
                keep = np.where(all_dets[j][:, -1] >= image_thresh)[0]
                all_dets[j] = all_dets[j][keep, :]
                all_rows[j] = all_rows[j][keep]
    roi = np.concatenate([all_rows[j] for j in range(1, C)] + [np.zeros((0,), np.int64)]).astype(np.int32)
    cls = np.concatenate([np.full(len(all_rows[j]), j) for j in range(1, C)] + [np.zeros((0,), np.int64)]).astype(np.int32)
    dets = np.concatenate([all_dets[j] for j in range(1, C)] + [np.zeros((0, 5), np.float32)]).astype(np.float32)
    return roi, cls, dets[:, 4].copy(), dets[:, :4].copy()


def case_rng(post):
    """the generator of the ten cases of one `post` (cases k = 0 .. 9 drawn in order)"""
    return np.random.RandomState(8 + post)             # (post = 1, case 7 is an empty result)


def make_inputs(rs, k, post, C):
    """case k of the NMS / select check, built like test_pick_kernel_vs_host's inputs: -> dict(cls_prob, bbox_pred, rois, n, nkeep_null,
    im_info, exact (zero size deltas: the host decode is bit-exact), thresh, max_per_image)"""
    H, W, scale = GEOMETRIES[k % 3]
    n = int(rs.randint(1, post + 1)) if k % 4 else post
    cp = rs.uniform(0, 1, (post, C)).astype(np.float32)
    if k % 5 == 1:
        cp = np.round(cp * 8).astype(np.float32) / 8            # ties inside classes and at image_thresh
    if k % 5 == 2:
        cp = cp ** 8                                            # few high scores
    cp[n:] = 2.0                                                # padding rows hold larger values
    # 60 % of the RoIs are jittered copies of post // 8 cluster boxes (heavy suppression), the rest uniform
    x1 = rs.uniform(-20, W * scale, post); y1 = rs.uniform(-20, H * scale, post)
    bw = rs.uniform(1, 300, post); bh = rs.uniform(1, 300, post)
    nc = max(post // 8, 1)
    ccx = rs.uniform(0, W * scale, nc); ccy = rs.uniform(0, H * scale, nc)
    cw = rs.uniform(20, 300, nc); ch = rs.uniform(20, 300, nc)
    member = rs.uniform(0, 1, post) < 0.6
    which = rs.randint(0, nc, post)
    jx = ccx[which] + rs.normal(0, 0.15, post) * cw[which]; jy = ccy[which] + rs.normal(0, 0.15, post) * ch[which]
    jw = cw[which] * rs.uniform(0.8, 1.25, post); jh = ch[which] * rs.uniform(0.8, 1.25, post)
    x1 = np.where(member, jx - jw / 2, x1); y1 = np.where(member, jy - jh / 2, y1)
    bw = np.where(member, jw, bw); bh = np.where(member, jh, bh)
    rois = np.stack([np.zeros(post), x1, y1, x1 + bw, y1 + bh], 1).astype(np.float32)
    bp = rs.normal(0, 0.3, (post, 4 * C)).astype(np.float32)
    exact = k % 2 == 0
    if exact:
        bp[:, 2::4] = 0; bp[:, 3::4] = 0
    return dict(cls_prob=cp, bbox_pred=bp, rois=rois, n=n, nkeep_null=k % 4 == 0, im_info=np.array([[H, W, scale]], np.float32), exact=exact,
                thresh=THRESH[k % 4], max_per_image=MAX_PER_IMAGE[k % 5])


def boxes_close(a, b, k=4):
    """tests/test_eval_device_gpu.py _box_close for arrays of boxes [...][4]: every coordinate within k ulp of its box's largest"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    big = np.maximum(np.maximum(np.abs(a).max(-1), np.abs(b).max(-1)), 1.0).astype(np.float32)
    return np.abs(a.astype(np.float64) - b) <= k * np.spacing(big)[..., None]
