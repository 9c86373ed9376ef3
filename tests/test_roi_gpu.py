"""Every dispatch branch of the RoI crop and pool kernels (csrc/roi.hip, csrc/roi_sample.h) against the references of tests/roi_util.py,
through the elementwise bound `check` of tests/small_kernels_util.py (the references and the bound are pinned without a GPU by
tests/test_roi_cpu.py).  Each case names the kernel the dispatcher has to pick and asserts ops.last_kernel() says so; the last test asserts
that the kernels seen are exactly roi_util.KERNELS (it needs the whole file to have run in this process).

Outputs sit in sentinel-padded buffers (tests/gpu_buf.py) and have to come back bit-identical outside the written region; the map gradient
of the crop backward STARTS as the sentinel (the gather form writes every element, the scatter form clears first), that of roipool_bwd,
which accumulates, as known values the reference includes.  Inputs have to come back unchanged.  A pixel no sample touches has bound 0: it
has to be exactly 0.  Every gather case runs twice and has to give the same bits.

test_sample_positions_bit_exact holds the device to `sample32`, bit for bit, on one-hot maps; every other crop case relies on it: the
references blend in float64 on sample32's positions, so the bound has no position term.

The 'seam' RoI set is this file's own addition to the clustered one: at the 9,800 entries the clustered set puts on one pixel the rounding
bound of the sum, which grows with the square of the list's length, is as large as an entry, so an entry lost at a window's seam hardly
shows there (tried on the device with the first entry of every later window left out: 1.4 times the bound on 5 of 33,280 elements); on the
seam set's list of 2,250 the same loss is 10 to 50 times the bound on over a hundred elements.

Worst values measured on an MI355X (this file's own prints):
  sample positions                      every tap weight bit-identical to sample32: 3,791 (roialign) and 4,183 (cropalign) of 1,176 samples at P = 7,
                                        15,733 and 16,883 of 4,704 samples at P = 14
  worst check ratio per entry point     roialign_fwd 0.387 (f32), 0.996 (bf16 store), cropalign_fwd 0.395 (f32), 0.996 (bf16 store),
                                        roialign_bwd 0.317 (gather), 0.26 (scatter), cropalign_bwd 0.274 (gather), 0.282 (scatter), roipool_bwd 0.383
                                        (the scatter form and roipool_bwd add atomically: their order, and with it the last digit, varies between runs)
  (a ratio next to 1 is a bf16 store: half a unit in the last place is the whole bound there)
  roipool_fwd values and argmax, every canary, the two runs of every gather case: exact"""
import numpy as np
import pytest
import torch

import roi_util as RU
from roi_util import FWD, BWD, FORMS, MAP
from small_kernels_util import check, F32, BF16, STORE
from gpu_buf import Buf, same_bits

pytestmark = pytest.mark.gpu

SEEN = set()
WORST = {}


def ops():
    from lang2seg_amd import ops as O
    return O


def landed(kernel):
    k = ops().last_kernel()
    SEEN.add(k)
    assert k == kernel, 'the dispatcher launched %s last, this case is meant for %s' % (k, kernel)


def note(name, w):
    WORST[name] = max(WORST.get(name, 0.0), w)
    return w


def crop_fwd(form, feat, H, W, C, rois, R, P, out):
    O = ops()
    if form == 'roialign':
        O.roialign_fwd(feat, H, W, C, rois, R, P, 1.0 / 16.0, out)
    else:
        _, im_h, im_w = RU.geometry(form, H, W)
        O.cropalign_fwd(feat, H, W, C, rois, R, P, im_h, im_w, out)


def crop_bwd(form, dout, H, W, C, rois, R, P, dfeat):
    O = ops()
    if form == 'roialign':
        O.roialign_bwd(dout, H, W, C, rois, R, P, 1.0 / 16.0, dfeat)
    else:
        _, im_h, im_w = RU.geometry(form, H, W)
        O.cropalign_bwd(dout, H, W, C, rois, R, P, im_h, im_w, dfeat)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('P', [7, 14])
def test_sample_positions_bit_exact(P, form):
    """a 6 x 7 map of 42 float32 channels, channel k one at pixel k and zero elsewhere: every output of the scalar kernel is exactly one tap
    weight or 0, and has to equal the weight of `sample32` multiplied out in float32, bit for bit (P = 7, and 14 as the max-pooled forms
    crop: another step and another split of linspace's two halves)"""
    H, W = RU.ONEHOT_MAP
    C, R = H * W, 24
    rois = RU.rois_for('shared', R, H, W)
    s = RU.sample32(rois, H, W, P, *RU.geometry(form, H, W))
    pix, w = RU.taps(s, H, W, np.float32)
    want = np.zeros((R * P * P, C + 1), np.float32)
    np.put_along_axis(want, np.where(pix < 0, C, pix).reshape(-1, 4), w.reshape(-1, 4), 1)
    want = want[:, :C]
    fb, rb, ob = Buf(C, C, init=np.eye(C, dtype=np.float32)), Buf(R, 5, init=rois), Buf(R * P * P, C)
    crop_fwd(form, fb.t, H, W, C, rb.t, R, P, ob.t)
    landed(RU.SCALAR)
    got = ob.get()
    diff = got.view(np.int32) != want.view(np.int32)
    if diff.any():
        i = tuple(np.argwhere(diff)[0])
        r, py, px = i[0] // (P * P), i[0] // P % P, i[0] % P
        raise AssertionError('%d of %d weights differ; the first: RoI %d (%s) row %d column %d pixel %d: device %r, sample32 %r (x0 %d wx1 %r, y0 %d wy1 %r)' % (
            int(diff.sum()), diff.size, r, rois[r, 1:], py, px, i[1], got[i], want[i], s.x0[r, px], s.wx1[r, px], s.y0[r, py], s.wy1[r, py]))
    ob.assert_untouched_outside(); fb.assert_unchanged(); rb.assert_unchanged()
    print('%s P %d: %d weights of %d samples bit-identical to sample32 (%d taps dropped outside the map)' % (form, P, int((want != 0).sum()), R * P * P, int((pix < 0).sum())))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('c', FWD, ids=RU.fwd_id)
def test_crop_fwd(c, form):
    C, dt, P, kernel, o = c
    H, W = MAP
    R = RU.FWD_R
    what = '%s %s' % (RU.fwd_id(c), form)
    rois, feat = RU.rois_for('shared', R, H, W), RU.feat_for(H, W, C, dt)
    fb, rb = Buf(H * W, C, off=o.get('foff', 0), dt=dt, init=feat), Buf(R, 5, init=rois)
    ob = Buf(R * P * P, C, off=o.get('ooff', 0), dt=dt)
    crop_fwd(form, fb.t, H, W, C, rb.t, R, P, ob.t)
    landed(kernel)
    ref, ab, nt = RU.crop_ref(feat, RU.sample32(rois, H, W, P, *RU.geometry(form, H, W)), C, kernel)
    w = note('%s_fwd %s' % (form, STORE[dt]), check(ob.get(), ref, ab, nt, STORE[dt], what=what))
    ob.assert_untouched_outside(what); fb.assert_unchanged(what); rb.assert_unchanged(what)
    print('%s: worst ratio %.3g' % (what, w))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('c', BWD, ids=RU.bwd_id)
def test_crop_bwd(c, form):
    C, dt, P, R, kernel, kind = c
    H, W = MAP
    what = '%s %s' % (RU.bwd_id(c), form)
    rois, dout = RU.rois_for(kind, R, H, W), RU.dout_for(R, P, C, dt)
    s = RU.sample32(rois, H, W, P, *RU.geometry(form, H, W))
    if kind != 'shared':
        # from the reference alone: some pixel collects more entries than the LDS window holds inside one chunk of 256 RoIs - the window loop makes a second pass
        assert max(RU.entries_per_pixel(s, H, W, r0, r0 + RU.CHUNK).max() for r0 in range(0, R, RU.CHUNK)) > RU.WINDOW
    gb, rb = Buf(R * P * P, C, dt=dt, init=dout), Buf(R, 5, init=rois)
    runs = []
    for _ in range(1 if kernel == RU.SCATTER else 2):
        db = Buf(H * W, C)                                  # starts as the sentinel
        crop_bwd(form, gb.t, H, W, C, rb.t, R, P, db.t)
        landed(kernel)
        runs.append(db)
    ref, ab, nt = RU.crop_bwd_ref(dout, s, H, W)
    got = runs[0].get()
    w = note('%s_bwd %s' % (form, 'scatter' if kernel == RU.SCATTER else 'gather'), check(got, ref, ab, nt, 'f32', what=what))
    none = nt[:, 0] == 0
    assert not got[none].any(), '%s: a pixel no sample touches is not 0' % what
    for db in runs:
        db.assert_untouched_outside(what)
    if len(runs) == 2:
        assert same_bits(runs[0], runs[1]), '%s: two runs of the gather form differ' % what
    gb.assert_unchanged(what); rb.assert_unchanged(what)
    print('%s: worst ratio %.3g; the longest list %d entries, %d pixels untouched' % (what, w, int(RU.entries_per_pixel(s, H, W).max()), int(none.sum())))


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
def test_roipool_fwd(dt):
    """C = 264 (the second trip of the 256-thread channel loop): values and argmax are exact; the RoIs of test_roipool (a tiny RoI whose
    bins share pixels, one partly outside with empty bins) on a map of quarter integers (ties)"""
    O = ops()
    H, W = MAP
    R, C = RU.POOL_WIDE
    P = RU.POOL_P
    rois, feat = RU.pool_rois(R), RU.pool_feat(C)
    ref, arg = RU.roipool_ref(R, C)
    assert (arg < 0).any()
    fb, rb = Buf(H * W, C, dt=dt, init=feat), Buf(R, 5, init=rois)
    ob, ab = Buf(R * P * P, C, dt=dt), Buf(R * P * P, C, dtype=torch.int32)
    O.roipool_fwd(fb.t, H, W, C, rb.t, R, P, 1.0 / 16.0, ob.t, ab.t)
    landed(RU.POOL_FWD)
    assert np.array_equal(ob.get(), ref)
    assert np.array_equal(ab.region().cpu().numpy(), arg)
    ob.assert_untouched_outside(); ab.assert_untouched_outside(); fb.assert_unchanged(); rb.assert_unchanged()


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('rc', [RU.POOL_SMALL, RU.POOL_BIG], ids=lambda rc: 'R%d-C%d' % rc)
def test_roipool_bwd(rc, dt):
    """the existing small size (21,560 elements: one pass) and 48 x 49 x 1024 = 2,408,448 elements against a grid of 8192 x 256: the
    grid-stride loop runs.  dfeat starts as known values, which the reference includes"""
    O = ops()
    H, W = MAP
    R, C = rc
    P = RU.POOL_P
    assert (R * P * P * C > RU.POOL_GRID) == (rc == RU.POOL_BIG)
    _, arg = RU.roipool_ref(R, C)
    dout, d0 = RU.dout_for(R, P, C, dt), RU.feat_for(H, W, C, F32)
    gb, ab = Buf(R * P * P, C, dt=dt, init=dout), Buf(R * P * P, C, dtype=torch.int32, init=arg)
    db = Buf(H * W, C, init=d0)
    O.roipool_bwd(gb.t, ab.t, R, P, C, db.t)
    landed(RU.POOL_BWD)
    ref, absum, nt = RU.roipool_bwd_ref(dout, arg, H, W, d0)
    what = 'roipool_bwd R%d C%d %s' % (R, C, STORE[dt])
    w = note('roipool_bwd', check(db.get(), ref, absum, nt, 'f32', what=what))
    db.assert_untouched_outside(what); gb.assert_unchanged(what); ab.assert_unchanged(what)
    print('%s: worst ratio %.3g; at most %d gradients on one element' % (what, w, int(nt.max()) - 1))


def test_every_roi_kernel_ran():
    print('worst check ratios:', ', '.join('%s %.3g' % kv for kv in sorted(WORST.items())))
    tables = sorted(set([c[3] for c in FWD] + [c[4] for c in BWD] + [RU.POOL_FWD, RU.POOL_BWD]))
    assert tables == RU.KERNELS and len(RU.KERNELS) == 7
    assert sorted(SEEN) == RU.KERNELS, (sorted(set(RU.KERNELS) - SEEN), sorted(SEEN - set(RU.KERNELS)))
