"""Evaluation on the device (model/eval_device.py, csrc/eval.hip) against the host loop it restates (model/test.py eval_split,
test_vgg.eval_split) and against the reference's own loop (ref_eval_split*.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def make_case(rs, k):
    """one (mask_prob [14][14] f32, box f32[4], ih, iw, gt [Hs][Ws] u8) case of the mask / IoU check"""
    ih = int(rs.choice([37, 64, 101, 240, 333, 480, 640]))
    iw = int(rs.choice([41, 64, 99, 320, 427, 500, 640]))
    f = [1.6, 0.9375, 1 / 1.6][k % 3]
    Hs, Ws = max(1, int(round(ih * f))), max(1, int(round(iw * f)))
    sizes = [1, 2, 13, 14, 15, 100, None]
    def side(n):
        s = sizes[rs.randint(len(sizes))]
        return float(n) if s is None else float(s)
    w, h = side(iw), side(ih)
    kind = rs.randint(6)
    x1 = rs.uniform(0, max(iw - w, 1)); y1 = rs.uniform(0, max(ih - h, 1))
    if kind == 0:
        x1, y1 = float(int(x1)), float(int(y1))                           # integer corners
    elif kind == 1:
        x1 = iw - w * rs.uniform(0.2, 0.9); y1 = ih - h * rs.uniform(0.2, 0.9)   # crossing the right / bottom borders
    elif kind == 2:
        x1 = iw - 1 + rs.uniform(0.01, 30)                                # x1 > iw - 1
    elif kind == 3:
        y1 = ih - 1 + rs.uniform(0.01, 30)
    x2, y2 = x1 + w - 1 + rs.uniform(-0.5, 0.5), y1 + h - 1 + rs.uniform(-0.5, 0.5)
    x2, y2 = max(x2, x1), max(y2, y1)
    box = np.array([x1, y1, x2, y2], np.float32)
    box[0] = max(box[0], 0); box[1] = max(box[1], 0)                     # _clip_boxes (what the host loop hands over)
    box[2] = min(box[2], iw - 1); box[3] = min(box[3], ih - 1)
    m = rs.randint(4)
    if m == 0:
        prob = np.full((14, 14), rs.uniform(0, 1), np.float32)           # constant: cscale = 0
    elif m == 1:
        prob = rs.uniform(0, 1, (14, 14)).astype(np.float32)
    elif m == 2:
        yy, xx = np.mgrid[0:14, 0:14]
        prob = (1 / (1 + np.exp(-(6 - np.hypot(yy - 6.5 + rs.uniform(-2, 2), xx - 6.5 + rs.uniform(-2, 2))) * rs.uniform(0.3, 3)))).astype(np.float32)
    else:
        prob = (rs.uniform(0, 1, (14, 14)) > 0.5).astype(np.float32) * rs.uniform(0.3, 1) + rs.uniform(0, 0.1)
        prob = prob.astype(np.float32)
    gt = np.zeros((Hs, Ws), np.uint8)
    gx1, gy1 = rs.randint(0, Ws), rs.randint(0, Hs)
    gt[gy1:gy1 + rs.randint(1, Hs + 1), gx1:gx1 + rs.randint(1, Ws + 1)] = 1
    if rs.randint(2):
        gt = (rs.uniform(0, 1, (Hs, Ws)) > 0.7).astype(np.uint8) | gt
    return prob, box, ih, iw, gt


def host_eval(prob, box, ih, iw, gt):
    from lang2seg_amd.model.test import segment_from_mask_prob, computeIoU_seg
    from lang2seg_amd.utils.mask_utils import imresize
    im_info = np.array([[ih, iw, 1.0]], np.float32)
    pred = segment_from_mask_prob(prob[None].copy(), box.copy(), im_info)
    g = imresize(gt, size=pred.shape, interp='nearest')
    I, U = computeIoU_seg(pred, g)
    return pred, g, I, U


def _box_close(a, b, k=4):
    """within k ulp of the box's largest coordinate: x1 = pcx - pw / 2 cancels, so one ulp of numpy's float32 exp in pw (not correctly
    rounded; the device rounds float64 exp) moves a small x1 by many of its own ulp"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return bool((np.abs(a.astype(np.float64) - b) <= k * np.spacing(np.float32(max(np.abs(a).max(), np.abs(b).max(), 1.0)))).all())


def _ulps(a, b):
    a = np.asarray(a, np.float32).view(np.int32).astype(np.int64); b = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def test_mask_iou_kernel_vs_host():
    """l2s_eval_mask_iou vs segment_from_mask_prob + imresize(gt, nearest) + computeIoU_seg: I and U equal on 2000 seeded cases (box
    sides 1, 2, 13, 14, 15, 100, the whole image; fractional corners; boxes across / beyond the right and bottom borders; constant
    masks; odd and even image sizes; gt scale factors 1.6, 0.9375, 1/1.6), and the predicted canvas pixel for pixel on 50 of them."""
    from lang2seg_amd import ops as O
    rs = np.random.RandomState(2024)
    N, NC = 2000, 50
    rec = O.eval_records(N)
    host, canv = [], []
    seen_w, seen_h = set(), set()
    for k in range(N):
        prob, box, ih, iw, gt = make_case(rs, k)
        pred, g, I, U = host_eval(prob, box, ih, iw, gt)
        host.append((int(I), int(U)))
        r = torch.zeros(6, dtype=torch.int64)
        r.view(torch.int32)[2:6].view(torch.float32).copy_(torch.from_numpy(box))
        rec[k].copy_(r)
        cv = torch.full((ih, iw), 7, dtype=torch.uint8, device='cuda') if k < NC else None
        O.eval_mask_iou(torch.from_numpy(prob).cuda(), rec, k, torch.from_numpy(gt).cuda(), ih, iw, canvas=cv)
        if cv is not None:
            canv.append((pred, cv))
        b = box.copy(); b[0::2] = np.clip(b[0::2], 0, iw - 1); b[1::2] = np.clip(b[1::2], 0, ih - 1)
        seen_w.add(int(b[2] - b[0] + np.float32(1))); seen_h.add(int(b[3] - b[1] + np.float32(1)))
    torch.cuda.synchronize()
    _, _, _, _, Is, Us = O.eval_record_fields(rec.cpu())
    bad = [k for k in range(N) if (int(Is[k]), int(Us[k])) != host[k]]
    assert not bad, [(k, host[k], int(Is[k]), int(Us[k])) for k in bad[:10]]
    for k, (pred, cv) in enumerate(canv):
        assert np.array_equal(cv.cpu().numpy(), pred), k
    assert {1, 2, 13, 14, 15, 100} <= seen_w and {1, 2, 13, 14, 15, 100} <= seen_h, (sorted(seen_w)[:20], sorted(seen_h)[:20])


def _host_pick(cls_prob, bbox_pred, rois, n, im_info, gt):
    from lang2seg_amd.model.test import detect_from_outputs, best_detection, computeIoU_box
    scores, boxes = detect_from_outputs(cls_prob[:n], bbox_pred[:n], rois[:n], im_info)
    r, c, box = best_detection(scores, boxes)
    scale = im_info[0][2]
    iou = computeIoU_box(box, gt[:4] / scale)
    return int(r), int(c), box, int(iou >= 0.5), iou


def test_pick_kernel_vs_host():
    """l2s_eval_pick vs best_detection / detect_from_outputs / computeIoU_box: the (roi, class) exactly - duplicated maxima, the
    background column tying the foreground maximum at an earlier index, nkeep < post with larger values in the padding rows - and the
    box bit for bit with zero size deltas (exp(0) = 1 on both sides), within 4 ulp otherwise (numpy's float32 exp is not correctly
    rounded); box hit equal unless the IoU is within 1e-5 of 0.5."""
    from lang2seg_amd import ops as O
    rs = np.random.RandomState(11)
    post, C = 64, 81
    N = 300
    rec = O.eval_records(N)
    roi_d = torch.zeros((N, 5), dtype=torch.float32, device='cuda'); lab_d = torch.zeros((N,), dtype=torch.int32, device='cuda')
    host = []
    for k in range(N):
        H, W, scale = [(600, 800, 1.6), (601, 999, 0.9375), (333, 500, 1.0)][k % 3]
        im_info = np.array([[H, W, scale]], np.float32)
        n = int(rs.randint(1, post + 1)) if k % 4 else post
        cp = rs.uniform(0, 1, (post, C)).astype(np.float32)
        if k % 5 == 1:
            cp = np.round(cp * 8).astype(np.float32) / 8            # many duplicated maxima
        if k % 5 == 2:
            m = cp[:n, 1:].max(); r0 = rs.randint(n); cp[r0, 0] = m  # background ties the foreground maximum
            cp[r0, 1:] = np.minimum(cp[r0, 1:], m)
            if r0 > 0:
                cp[:r0, :] = np.minimum(cp[:r0, :], m * 0.5)
        cp[n:] = 2.0                                                # padding rows hold larger values
        x1 = rs.uniform(-20, W * scale, post); y1 = rs.uniform(-20, H * scale, post)
        rois = np.stack([np.zeros(post), x1, y1, x1 + rs.uniform(1, 300, post), y1 + rs.uniform(1, 300, post)], 1).astype(np.float32)
        bp = (rs.normal(0, 0.3, (post, 4 * C))).astype(np.float32)
        if k % 2 == 0:
            bp[:, 2::4] = 0; bp[:, 3::4] = 0
        gt = np.array([rs.uniform(0, W * scale * 0.5), rs.uniform(0, H * scale * 0.5), 0, 0, 1], np.float32)
        gt[2] = gt[0] + rs.uniform(5, W * scale * 0.5); gt[3] = gt[1] + rs.uniform(5, H * scale * 0.5)
        host.append((_host_pick(cp, bp, rois, n, im_info, gt), k % 2 == 0, np.float32(scale), n))
        t = lambda a: torch.from_numpy(a).cuda()
        ih, iw = int(round(im_info[0][0] / im_info[0][2])), int(round(im_info[0][1] / im_info[0][2]))
        nk = torch.tensor([n], dtype=torch.int32, device='cuda') if k % 4 else None
        O.eval_pick(t(cp), t(bp), t(rois), nk, post, C, im_info[0][2], ih, iw, t(gt), True, rec, k, roi_d[k:k + 1], lab_d[k:k + 1])
    torch.cuda.synchronize()
    roi, cls, box, hit, I, U = O.eval_record_fields(rec.cpu())
    mroi, mlab = roi_d.cpu().numpy(), lab_d.cpu().numpy()
    bg_wins = 0
    for k, ((r, c, b, h, iou), exact, scale, n) in enumerate(host):
        assert (roi[k], cls[k]) == (r, c), (k, roi[k], cls[k], r, c)
        bg_wins += c == 0
        d = _ulps(box[k], b)
        assert (d == 0).all() if exact else _box_close(box[k], b), (k, box[k], b)
        if abs(iou - 0.5) > 1e-5:
            assert hit[k] == h, (k, iou)
        assert I[k] == 0 and U[k] == 0
        assert mlab[k] == c and mroi[k][0] == 0
        if exact:
            assert np.array_equal(mroi[k][1:], (np.array([b]) * scale).astype(np.float32)[0])
    assert bg_wins > 0


class _ListLoader(object):
    """getTestBatch over a fixed list of blobs (optionally logging which image each call returned)"""

    def __init__(self, blobs, log=None):
        self.blobs, self.log = blobs, log
        self.split_ix = {'val': list(range(len(blobs)))}
        self.iterators = {'val': 0}

    def getTestBatch(self, split, stride=1):
        i = self.iterators[split]
        nxt = i + stride
        wrapped = nxt >= len(self.blobs)
        self.iterators[split] = 0 if wrapped else nxt
        if self.log is not None:
            self.log.append(i)
        b = dict(self.blobs[i])
        b['bounds'] = dict(it_pos_now=i + 1, it_max=len(self.blobs), wrapped=wrapped)
        return b


def _synthetic_blobs(sizes, S, seed=0):
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    out = []
    for j, (H, W) in enumerate(sizes):
        b = SyntheticLoader(num_images=1, sents_per_image=S, H=H, W=W, T=6, vocab_size=60, seed=seed + 97 * j)._image(0)
        out.append({k: v for k, v in b.items() if k in ('data', 'im_info', 'gt_boxes', 'gt_masks', 'labels', 'file_name')})
    return out


def _host_run(net, blobs, variant_vgg=False):
    """eval_split with per-sentence (roi, class, box, hit, I, U) recorded"""
    from lang2seg_amd.model import test as T
    per = []
    ob, oi, os_ = T.best_detection, T.computeIoU_box, T.computeIoU_seg

    def bd(scores, boxes):
        r = ob(scores, boxes); per.append([int(r[0]), int(r[1]), r[2].copy()]); return r

    def ib(a, b):
        v = oi(a, b); per[-1].append(int(v >= 0.5)); per[-1].append(v); return v

    def sg(a, b):
        I, U = os_(a, b); per[-1] += [int(I), int(U)]; return I, U
    T.best_detection, T.computeIoU_box, T.computeIoU_seg = bd, ib, sg
    try:
        if variant_vgg:
            from lang2seg_amd.model import test_vgg as TVG
            TVG.best_detection, TVG.computeIoU_box = bd, ib
            try:
                res = TVG.eval_split(_ListLoader(blobs), net, None, 'val', dict(verbose=False))
            finally:
                TVG.best_detection, TVG.computeIoU_box = ob, oi
        else:
            res = T.eval_split(_ListLoader(blobs), net, None, 'val', dict(verbose=False))
    finally:
        T.best_detection, T.computeIoU_box, T.computeIoU_seg = ob, oi, os_
    return res, per


def _compare(res_h, per_h, res_d, per_d, masks=True):
    """per sentence: (roi, class) equal, box within 4 ulp (_box_close).  A box bit-equal to the host's must give the same hit, I and U.
    A box that is not (numpy's float32 exp) may move a truncation of recover_masks / the mask head's RoI: hit may then differ only at an
    IoU within 1e-5 of 0.5, I and U by at most one box row plus one box column of pixels.  Without such a sentence the 7-tuples are equal."""
    assert len(per_h) == len(per_d)
    exceptions = 0
    for k, (h, d) in enumerate(zip(per_h, per_d)):
        assert (d[0], d[1]) == (h[0], h[1]), (k, d[:2], h[:2])
        assert _box_close(d[2], h[2]), (k, d[2], h[2])
        same = d[3] == h[3] and (not masks or (d[4], d[5]) == (h[5], h[6]))
        if not same:
            assert not np.array_equal(np.asarray(d[2], np.float32), h[2]), (k, d, h)
            assert d[3] == h[3] or abs(h[4] - 0.5) < 1e-5, (k, d, h)
            if masks:
                bw = int(h[2][2] - h[2][0] + 1) + int(h[2][3] - h[2][1] + 1) + 2
                assert abs(d[4] - h[5]) <= bw and abs(d[5] - h[6]) <= bw, (k, d, h)
            exceptions += 1
    if exceptions == 0:
        for a, b in zip(res_h, res_d):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (res_h, res_d)
    return exceptions


@pytest.mark.parametrize('variant,dtype', [('cycle', 'f32'), ('cycle', 'bf16'), ('spatial', 'f32'), ('spatial', 'bf16')])
def test_eval_split_device_vs_host(variant, dtype):
    """eval_split_device vs eval_split on the same network: 3 images of distinct sizes x 3 sentences.  The 7-tuples equal; per sentence
    the (roi, class) equal, the box within 4 ulp, hit / I / U equal (except next to a truncation or the 0.5 boundary, detected here)."""
    from lang2seg_amd import selftest
    from lang2seg_amd.model.eval_device import eval_split_device
    from oracle import weights as OW
    opt = OW.default_opt(vocab_size=60, seq_length=6)
    sd = OW.make_state_dict(opt, seed=3, head_gain=4.0, variant=variant)
    net = selftest.build_net(opt, {}, dtype, sd, variant=variant)
    blobs = _synthetic_blobs([(224, 288), (256, 352), (288, 224)], 3)
    res_h, per_h = _host_run(net, blobs)
    det = []
    res_d = eval_split_device(_ListLoader(blobs), net, None, 'val', dict(verbose=False), details=det)
    assert _compare(res_h, per_h, res_d, det) <= 1
    assert res_d[6] == 9 and res_d[3] == 9 and int(res_d[5]) > 0


def test_shared_backbone_is_bit_identical():
    """one backbone pass for all sentences of an image gives the same heads' outputs, bit for bit, as a backbone pass per sentence"""
    from lang2seg_amd import selftest
    from oracle import weights as OW
    opt = OW.default_opt(vocab_size=60, seq_length=6)
    net = selftest.build_net(opt, {}, 'bf16', OW.make_state_dict(opt, seed=3, head_gain=4.0))
    net.eval()
    b = _synthetic_blobs([(256, 320)], 3)[0]
    per = []
    for i in range(3):
        p = net.forward_test(net.upload_blob(dict(b), i))
        per.append((p['cls_prob'].cpu().clone(), p['bbox_pred'].cpu().clone(), p['mask_prob'].cpu().clone()))
    d = net.upload_blob(dict(b), 0)
    net.forward_test_image(d)
    for i in range(3):
        di = net.upload_blob(dict(b), i)
        s = net.forward_test_sentence(di)
        n = int(s['nkeep'].item()) if s['nkeep'] is not None else s['post']
        MS = per[i][2].shape[1]
        assert torch.equal(s['cls_prob'][:n].cpu(), per[i][0]) and torch.equal(s['bbox_pred'][:n].cpu(), per[i][1])
        assert torch.equal(s['mask_prob'].view(s['post'], MS, MS, -1)[:n].cpu(), per[i][2])


def test_eval_split_vgg_device_vs_host():
    from lang2seg_amd import selftest
    from lang2seg_amd.model.eval_device import eval_split_vgg_device
    from oracle import weights as OW
    opt = OW.default_opt(vocab_size=60, seq_length=6); opt['C4_feat_dim'] = 512
    net = selftest.build_net(opt, {}, 'bf16', OW.make_state_dict(opt, seed=3, head_gain=4.0, variant='vgg'), variant='vgg')
    blobs = _synthetic_blobs([(224, 288), (256, 352)], 2)
    res_h, per_h = _host_run(net, blobs, variant_vgg=True)
    det = []
    res_d = eval_split_vgg_device(_ListLoader(blobs), net, None, 'val', dict(verbose=False), details=det)
    assert _compare(res_h, per_h, res_d, det, masks=False) <= 1
    assert res_d[1] == 4


def _ref_setup(vgg):
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    import make_golden as MG
    from lang2seg_amd import selftest
    from oracle import weights as OW
    opt = OW.default_opt(vocab_size=60, seq_length=6)
    if vgg:
        opt['C4_feat_dim'] = 512
        net = selftest.build_net(opt, {}, 'f32', MG.eval_state_dict_vgg(opt), variant='vgg')
    else:
        net = selftest.build_net(opt, {}, 'f32', MG.eval_state_dict(opt))
    return net, MG.eval_blobs()


def test_eval_split_device_vs_reference():
    """eval_split_device on the setup of test_train_step_gpu.py test_eval_split_vs_reference, with that test's assertions"""
    from lang2seg_amd.model.eval_device import eval_split_device
    g = dict(np.load(os.path.join(HERE, 'golden', 'ref_eval_split.npz')))
    net, imgs = _ref_setup(False)
    det = []
    acc, thr, seg_correct, seg_total, cum_I, cum_U, num_sent = eval_split_device(_ListLoader(imgs), net, None, 'val', dict(verbose=False), details=det)
    assert num_sent == int(g['num_sent']) == seg_total == int(g['seg_total']) and list(thr) == list(g['thr'])
    assert [p[1] for p in det] == list(g['pred_class'])
    assert np.allclose(np.stack([p[2] for p in det]), g['pred_box'], atol=1e-2)
    assert acc == float(g['acc']) and list(seg_correct) == list(g['seg_correct'])
    assert abs(int(cum_I) - int(g['cum_I'])) <= 3 and abs(int(cum_U) - int(g['cum_U'])) <= 3, (cum_I, cum_U, int(g['cum_I']), int(g['cum_U']))
    assert int(g['cum_I']) > 0


def test_eval_split_vgg_device_vs_reference():
    """eval_split_vgg_device on the setup of test_train_step_gpu.py test_eval_split_vgg_vs_reference, with that test's assertions"""
    from lang2seg_amd.model.eval_device import eval_split_vgg_device
    g = dict(np.load(os.path.join(HERE, 'golden', 'ref_eval_split_vgg.npz')))
    net, imgs = _ref_setup(True)
    det = []
    acc, num_sent = eval_split_vgg_device(_ListLoader(imgs), net, None, 'val', dict(verbose=False), details=det)
    assert num_sent == int(g['num_sent']) and acc == float(g['acc'])
    assert [p[1] for p in det] == list(g['pred_class'])
    assert np.allclose(np.stack([p[2] for p in det]), g['pred_box'], atol=1e-2)


def _eval_net():
    from lang2seg_amd import selftest
    from oracle import weights as OW
    opt = OW.default_opt(vocab_size=60, seq_length=6)
    return selftest.build_net(opt, {}, 'bf16', OW.make_state_dict(opt, seed=3, head_gain=4.0))


_RANK_SIZES = [(224, 288), (256, 320), (288, 224), (224, 224), (256, 288)]


def _rank_worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'] = '127.0.0.1'; os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from lang2seg_amd.model.eval_device import eval_split_device
    net = _eval_net()
    log = []
    res = eval_split_device(_ListLoader(_synthetic_blobs(_RANK_SIZES, 2), log), net, None, 'val', dict(verbose=False), rank=rank, world=world)
    torch.save(dict(res=[np.asarray(r) for r in res], log=log), os.path.join(outdir, 'rank%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_eval_two_ranks_one_gpu(tmp_path):
    """two ranks through gloo on 5 images (uneven shards): the result equals the one-rank result exactly, and each rank decoded only
    the images at its positions p = rank (mod 2)"""
    import torch.multiprocessing as mp
    from lang2seg_amd.model.eval_device import eval_split_device
    ctx = mp.get_context('spawn')
    port = 29900 + os.getpid() % 500
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p_ in procs:
        p_.start()
    ref = eval_split_device(_ListLoader(_synthetic_blobs(_RANK_SIZES, 2)), _eval_net(), None, 'val', dict(verbose=False))
    for p_ in procs:
        p_.join(600)
        assert p_.exitcode == 0
    for r in range(2):
        out = torch.load(os.path.join(str(tmp_path), 'rank%d.pt' % r), weights_only=False)
        assert out['log'] == list(range(r, 5, 2)), out['log']
        for a, b in zip(out['res'], ref):
            assert np.array_equal(a, np.asarray(b)), (out['res'], ref)
    with pytest.raises(ValueError):
        eval_split_device(_ListLoader(_synthetic_blobs(_RANK_SIZES[:1], 1)), _eval_net(), None, 'val', dict(num_sents=1, verbose=False), rank=0, world=2)
