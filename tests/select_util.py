"""numpy restatements of csrc/select.hip (l2s_detect_gt_iou, l2s_detect_choose) and the generators of their cases.
The gt mask is resized by oracle/boxes.py's closed form of PIL NEAREST; the box hit is computeIoU_box in float32, operation by operation;
the choice keeps, per rule, the first detection that no other one beats."""
import os
import sys
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import boxes as OB  # noqa: E402

MARGIN = 1e-6          # two re-rank keys closer than this (and not bit-equal) are no test of the choice: see choose_case


# ---------------------------------------------------------------- l2s_detect_gt_iou
def resize_gt(gt, ih, iw):
    return OB.imresize_nearest_u8(np.asarray(gt), (ih, iw)) != 0


def box_hit(box, gt_box, im_scale):
    """computeIoU_box(box, gt_box / im_scale) >= 0.5 in float32 (model/test.py's order of operations)"""
    f = np.float32
    o = [f(v) for v in box]
    g = [f(v) / f(im_scale) for v in gt_box]
    ix1, iy1, ix2, iy2 = max(o[0], g[0]), max(o[1], g[1]), min(o[2], g[2]), min(o[3], g[3])
    inter = f(0)
    if ix1 < ix2 and iy1 < iy2:
        inter = f(f(f(ix2 - ix1) + f(1)) * f(f(iy2 - iy1) + f(1)))
    a1 = f(f(f(o[2] - o[0]) + f(1)) * f(f(o[3] - o[1]) + f(1)))
    a2 = f(f(f(g[2] - g[0]) + f(1)) * f(f(g[3] - g[1]) + f(1)))
    uni = f(f(a1 + a2) - inter)
    with np.errstate(divide='ignore', invalid='ignore'):
        return int(f(inter / uni) >= f(0.5))


def gt_iou(canvases, boxes, count, gt, gt_box, im_scale):
    """-> (I [cap], U [cap], hit [cap], gt_area); rows behind the count are zero"""
    cap, ih, iw = canvases.shape
    g = resize_gt(gt, ih, iw)
    n = min(max(int(count), 0), cap)
    I, U, hit = np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.int64)
    for d in range(n):
        c = canvases[d] != 0
        I[d], U[d], hit[d] = (c & g).sum(), (c | g).sum(), box_hit(boxes[d], gt_box, im_scale)
    return I, U, hit, int(g.sum())


def box_canvases(rs, cap, ih, iw, kind='random'):
    """canvases as l2s_detect_paste leaves them: bits inside the record's box (eval_box_geometry: x = int(x1), w = int(x2 - x1 + 1)),
    zero outside.  -> (canvases uint8 [cap][ih][iw], boxes f32 [cap][4], areas).  kind: random, empty, full (every pixel of the box);
    the first boxes touch the image's edges"""
    can = np.zeros((cap, ih, iw), np.uint8)
    boxes = np.zeros((cap, 4), np.float32)
    for d in range(cap):
        x1, x2 = sorted(rs.randint(0, iw, 2))
        y1, y2 = sorted(rs.randint(0, ih, 2))
        if d % 7 == 0:
            x1, y1 = 0, 0                                          # the left and top edges
        if d % 7 == 1:
            x2, y2 = iw - 1, ih - 1                                # the right and bottom edges
        if d % 7 == 2:
            x1, y1, x2, y2 = 0, 0, iw - 1, ih - 1                  # the whole image
        frac = rs.rand(2) * 0.9                                    # (the fraction does not change int(x1) or int(x2 - x1 + 1))
        boxes[d] = [x1 + frac[0], y1 + frac[1], x2 + frac[0], y2 + frac[1]] if x2 < iw - 1 and y2 < ih - 1 else [x1, y1, x2, y2]
        b = boxes[d]
        gx, gy, gw, gh = int(b[0]), int(b[1]), int(np.float32(b[2] - b[0]) + np.float32(1)), int(np.float32(b[3] - b[1]) + np.float32(1))
        gw, gh = min(gw, iw - gx), min(gh, ih - gy)
        if kind == 'random':
            can[d, gy:gy + gh, gx:gx + gw] = rs.rand(gh, gw) > 0.4
        elif kind == 'full':
            can[d, gy:gy + gh, gx:gx + gw] = 1
    return can, boxes, can.reshape(cap, -1).sum(1).astype(np.int32)


def records(boxes, areas, scores=None, cls=None):
    """l2s_det_record rows as int32 [n][8]"""
    n = boxes.shape[0]
    r = np.zeros((n, 8), np.int32)
    r[:, 0] = np.arange(n)
    r[:, 1] = 1 if cls is None else cls
    r[:, 2:6] = np.asarray(boxes, np.float32).view(np.int32)
    r[:, 6] = (np.full(n, 0.5, np.float32) if scores is None else np.asarray(scores, np.float32)).view(np.int32)
    r[:, 7] = areas
    return r


# ---------------------------------------------------------------- l2s_detect_choose
def rule_names(lambdas, with_expr):
    return ['detector', 'oracle'] + (['speaker'] + ['rerank@%s' % float(l) for l in lambdas] if with_expr else [])


def rerank_key(score, expr, lam, per_token, n_tok):
    """log((double)score) + (double)(float)lambda * (double)expr / (per_token ? n_tok : 1), every operation rounded on its own"""
    div = np.float64(n_tok if per_token else 1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.log(np.asarray(score, np.float32).astype(np.float64)) + np.float64(np.float32(lam)) * np.asarray(expr, np.float32).astype(np.float64) / div


def _iou_pair(I, U):
    return (int(I), int(U)) if int(U) else (0, 1)                  # U = 0 counts as IoU 0


def _record(d, cls, hit, I, U, key, gt_area):
    if d < 0:
        return dict(det=-1, cls=-1, hit=0, I=0, U=int(gt_area), key=0.0)
    return dict(det=int(d), cls=int(cls[d]), hit=int(hit[d]), I=int(I[d]), U=int(U[d]), key=float(key))


def _all_keys(score, I, U, n, expr, lambdas, per_token, n_tok):
    """per rule the float64 keys of the first n detections (the oracle's are for the printout: its comparison is exact)"""
    keys = [np.asarray(score[:n], np.float32).astype(np.float64),
            np.asarray([float(I[d]) / float(U[d]) if U[d] else 0.0 for d in range(n)], np.float64)]
    if expr is not None:
        keys.append(np.asarray(expr[:n], np.float32).astype(np.float64))
        keys += [rerank_key(score[:n], expr[:n], l, per_token, n_tok) for l in lambdas]
    return keys


def choose(score, cls, hit, I, U, count, gt_area, expr=None, lambdas=(), per_token=False, n_tok=1):
    """-> one dict(det, cls, hit, I, U, key) per rule: a scan that keeps the first detection no later one strictly beats"""
    n = min(max(int(count), 0), len(score))
    out = []
    for rule, key in enumerate(_all_keys(score, I, U, n, expr, lambdas, per_token, n_tok)):
        best = -1
        for d in range(n):
            if best < 0:
                best = d
            elif rule == 1:
                (Ia, Ua), (Ib, Ub) = _iou_pair(I[d], U[d]), _iou_pair(I[best], U[best])
                if Ia * Ub > Ib * Ua:
                    best = d
            elif key[d] > key[best]:
                best = d
        out.append(_record(best, cls, hit, I, U, key[best] if best >= 0 else 0.0, gt_area))
    return out


def choose_brute(score, cls, hit, I, U, count, gt_area, expr=None, lambdas=(), per_token=False, n_tok=1):
    """the same by all pairs: the lowest index that no other detection beats (the oracle by exact fractions)"""
    n = min(max(int(count), 0), len(score))
    out = []
    for rule, key in enumerate(_all_keys(score, I, U, n, expr, lambdas, per_token, n_tok)):
        if rule == 1:
            val = [Fraction(*_iou_pair(I[d], U[d])) for d in range(n)]
        else:
            val = [float(v) for v in key]
        winners = [a for a in range(n) if not any(val[b] > val[a] for b in range(n))]
        best = min(winners) if winners else -1
        out.append(_record(best, cls, hit, I, U, key[best] if best >= 0 else 0.0, gt_area))
    return out


def close_rerank(score, expr, n, lambdas, per_token, n_tok):
    """a re-rank rule whose best two keys are closer than MARGIN without being bit-equal"""
    for l in lambdas:
        k = np.sort(rerank_key(score[:n], expr[:n], l, per_token, n_tok))[::-1]
        if k.size >= 2 and k[0] != k[1] and k[0] - k[1] < MARGIN:
            return True
    return False


def choose_case(seed, cap, count, n_lambda, per_token, with_expr=True, ties=True):
    """one case of l2s_detect_choose -> (dict of arrays and arguments, redraws).  Scores in (0, 1) and expr in (-40, 0) as float32, a few
    exact score ties, IoU ties with different counts (1/2 against 2/4), U = 0 rows and rows copied whole (bit-equal keys by construction).
    A case whose best two keys of a re-rank rule differ by less than MARGIN = 1e-6 in float64 without being bit-equal is drawn again: the
    device's and numpy's float64 log differ by a few ulp (1e-15 relative) on keys of magnitude up to 1e2, far inside the margin."""
    redraws = 0
    while True:
        rs = np.random.RandomState(seed + 7919 * redraws)
        score = (rs.rand(cap) * 0.98 + 0.01).astype(np.float32)
        expr = (-rs.rand(cap) * 40).astype(np.float32)
        U = rs.randint(1, 5000, cap).astype(np.int64)
        I = (U * rs.rand(cap)).astype(np.int64)
        if ties and cap >= 4:
            k = rs.permutation(cap)
            score[k[1]] = score[k[0]] = score.max()                       # the best score twice
            I[k[2]], U[k[2]], I[k[3]], U[k[3]] = 1, 2, 2, 4                # one IoU with different counts
            if rs.rand() < 0.5:
                I[k[2]], U[k[2]], I[k[3]], U[k[3]] = 4999, 5000, 9998, 10000   # ... as the best of the list
            U[k[0]] = I[k[0]] = 0                                         # an empty mask against an empty gt
        if ties and cap >= 8:
            a, b = rs.permutation(cap)[:2]
            score[b], expr[b], I[b], U[b] = score[a], expr[a], I[a], U[a]  # a copied row: bit-equal keys
        lambdas = [0.0, 0.5, 4.0, 1.0, 0.25, 2.0, 8.0, 16.0][:n_lambda]
        n_tok = int(rs.randint(2, 12))
        n = min(count, cap)
        if not with_expr or not close_rerank(score, expr, n, lambdas, per_token, n_tok):
            break
        redraws += 1
    c = dict(score=score, cls=rs.randint(1, 81, cap).astype(np.int32), hit=rs.randint(0, 2, cap).astype(np.int32), I=I, U=U, count=count,
             gt_area=int(rs.randint(0, 9000)), expr=expr if with_expr else None, lambdas=lambdas if with_expr else [], per_token=bool(per_token),
             n_tok=n_tok)
    return c, redraws


def choose_args(c):
    return (c['score'], c['cls'], c['hit'], c['I'], c['U'], c['count'], c['gt_area'], c['expr'], c['lambdas'], c['per_token'], c['n_tok'])


def totals(entries, seg_list):
    """per rule _Totals' sums over selection entries, by _Totals.add's expressions"""
    out = {}
    for e in entries:
        for name, ch in e['rules'].items():
            t = out.setdefault(name, dict(acc=0, num_sent=0, seg_correct=[0] * len(seg_list), cum_I=0, cum_U=0))
            t['acc'] += 1 if ch['hit'] else 0
            t['num_sent'] += 1
            I, U = np.int64(ch['I']), np.int64(ch['U'])
            t['cum_I'] += int(I); t['cum_U'] += int(U)
            with np.errstate(divide='ignore', invalid='ignore'):
                for k, th in enumerate(seg_list):
                    t['seg_correct'][k] += int(I * 1.0 / U >= th)
    return out
