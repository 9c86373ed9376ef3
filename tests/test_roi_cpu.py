"""The references of tests/roi_util.py and their bound, pinned without a GPU.  Nothing of the device enters here.

The restatement against the definition.  On every case table of the GPU file, `crop_ref` / `crop_bwd_ref` on the float32 positions of
`sample32` are compared elementwise with `crop64` (theta, affine_grid and grid_sample on doubles, autograd for the backward).  The two
differ in where the samples lie, so the bound carries a position term next to the rounding term of `check`:
  forward    dx Lx[c] + dy Ly[c]: dx, dy = this sample's |ix32 - ix64|, |iy32 - iy64|, computed here from the two references; Lx[c], Ly[c] = the
             largest horizontal / vertical neighbour difference of channel c on the zero-padded map.  These are Lipschitz constants of the
             bilinear interpolant, which is continuous, so the term holds when floor() lands on the other side of an integer.
  backward   sum of (dx + dy) |g| over the samples that touch the pixel under either position: a pixel's weight is the product of two hat
             functions of the position, each 1-Lipschitz and at most 1.

The bound is not idle: the plain torch-CPU float32 forms (F.grid_sample in float32 on the restated grid, a float32 index_add_ scatter) pass
the GPU file's own bound - rounding only, no position term - on every table, and each structural error listed in
test_bound_catches_structural_errors fails it.

Figures of this file's own prints (a 20 x 26 map and the 6 x 7 one-hot map, both forms, P = 7, 14, 32, 33):
  worst |position32 - position64| in units of 2^-24 x (map size)   dx 4.6, dy 3.09
  positions on the other side of an integer                        149 of 133,756
  worst ratio of the restatement against the definition             forward 0.989, backward 0.9992.  The position term is the whole bound there and
                                                                    it is sharp: the box with corners on multiples of 16 has samples of weight exactly 1
                                                                    on one axis, where a shift of dx moves the value by dx times the neighbour difference
  worst ratio of the float32 forms (rounding bound alone)           crop forward 0.395 (0.996 with a bf16 store: half a unit in the last place is the
                                                                    whole bound), crop backward 0.32, roipool backward 0.383"""
import numpy as np
import pytest

import roi_util as RU
from roi_util import FWD, BWD, FORMS, MAP, SCALAR
from small_kernels_util import check, f64, U24, F32, BF16, STORE

WORST = {}
POS = dict(dx=0.0, dy=0.0, flips=0, n=0)


def note(name, w):
    WORST[name] = max(WORST.get(name, 0.0), w)
    return w


def positions(s, ix64, iy64, H, W):
    """dx [R][P], dy [R][P]; the worst of each in units of 2^-24 x size goes into POS"""
    dx, dy = np.abs(f64(s.ix) - ix64), np.abs(f64(s.iy) - iy64)
    POS['dx'] = max(POS['dx'], float(dx.max() / (U24 * W))); POS['dy'] = max(POS['dy'], float(dy.max() / (U24 * H)))
    POS['flips'] += int((np.floor(ix64) != s.x0).sum() + (np.floor(iy64) != s.y0).sum()); POS['n'] += 2 * dx.size
    return dx, dy


def lipschitz(feat, H, W):
    """per channel, the largest horizontal and vertical neighbour difference of the zero-padded map"""
    Fp = np.pad(f64(feat).reshape(H, W, -1), ((1, 1), (1, 1), (0, 0)))
    return np.abs(np.diff(Fp, axis=1)).max((0, 1)), np.abs(np.diff(Fp, axis=0)).max((0, 1))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('c', FWD, ids=RU.fwd_id)
def test_crop_fwd_reference(c, form):
    C, dt, P, kernel, _ = c
    H, W = MAP
    rois, feat = RU.rois_for('shared', RU.FWD_R, H, W), RU.feat_for(H, W, C, dt)
    s = RU.sample32(rois, H, W, P, *RU.geometry(form, H, W))
    ref, ab, nt = RU.crop_ref(feat, s, C, kernel)
    out64, _, ix64, iy64 = RU.crop64(feat, rois, P, H, W, form)
    dx, dy = positions(s, ix64, iy64, H, W)
    Lx, Ly = lipschitz(feat, H, W)
    pos = (dx[:, None, :, None] * Lx + dy[:, :, None, None] * Ly).reshape(-1, C)
    a = note('definition, forward', check(ref, out64, ab, nt, 'f32', floor=pos, what='crop_ref against crop64'))
    b = note('float32 form, forward (%s)' % STORE[dt], check(RU.crop_fwd_f32(feat, s, C, dt), ref, ab, nt, STORE[dt], what='grid_sample in float32'))
    assert not ref[RU.OUTSIDE * P * P:(RU.OUTSIDE + 1) * P * P].any()                # the RoI wholly outside the map
    print('%s %s: restatement against the definition %.3g, float32 form %.3g of the bound' % (RU.fwd_id(c), form, a, b))


def touch(pos, n):
    """[R][P][n]: the hat function of the position is non-zero on the cell"""
    return (np.abs(f64(pos)[:, :, None] - np.arange(n)[None, None]) < 1).astype(np.float64)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('c', BWD, ids=RU.bwd_id)
def test_crop_bwd_reference(c, form):
    C, dt, P, R, kernel, kind = c
    H, W = MAP
    rois, dout = RU.rois_for(kind, R, H, W), RU.dout_for(R, P, C, dt)
    s = RU.sample32(rois, H, W, P, *RU.geometry(form, H, W))
    ref, ab, nt = RU.crop_bwd_ref(dout, s, H, W)
    _, g64, ix64, iy64 = RU.crop64(np.zeros((H * W, C), np.float32), rois, P, H, W, form, dout=dout)
    dx, dy = positions(s, ix64, iy64, H, W)
    G = np.abs(f64(dout)).reshape(R, P, P, C)
    y32, x32, y64, x64 = touch(s.iy, H), touch(s.ix, W), touch(iy64, H), touch(ix64, W)
    term = lambda My, Mx: RU.sep_scatter(My, Mx * dx[:, :, None], G) + RU.sep_scatter(My * dy[:, :, None], Mx, G)
    pos = (term(y32, x32) + term(y64, x64) - term(y32 * y64, x32 * x64)).reshape(H * W, C)   # either = one + the other - both
    a = note('definition, backward', check(ref, g64, ab, nt, 'f32', floor=np.maximum(pos, 0.0), what='crop_bwd_ref against autograd of crop64'))
    b = note('float32 form, backward', check(RU.crop_bwd_f32(dout, s, H, W), ref, ab, nt, 'f32', what='float32 scatter'))
    assert not ref[nt[:, 0] == 0].any() and not ab[nt[:, 0] == 0].any()
    if kind != 'shared':
        assert RU.entries_per_pixel(s, H, W, 0, RU.CHUNK).max() > RU.WINDOW
    print('%s %s: restatement against the definition %.3g, float32 form %.3g of the bound; %d pixels untouched' % (
        RU.bwd_id(c), form, a, b, int((nt == 0).sum())))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('P', [7, 14])
def test_onehot_reference(P, form):
    """the one-hot map of the GPU file's position test: every value of the reference is one tap weight or 0"""
    H, W = RU.ONEHOT_MAP
    rois = RU.rois_for('shared', 24, H, W)
    s = RU.sample32(rois, H, W, P, *RU.geometry(form, H, W))
    ref, _, _ = RU.crop_ref(np.eye(H * W, dtype=np.float32), s, H * W, SCALAR, H, W)
    pix, w = RU.taps(s, H, W, np.float64)
    want = np.zeros((pix.size // 4, H * W + 1))
    np.put_along_axis(want, np.where(pix < 0, H * W, pix).reshape(-1, 4), w.reshape(-1, 4), 1)
    assert np.array_equal(ref, want[:, :H * W])
    _, _, ix64, iy64 = RU.crop64(np.zeros((H * W, 1), np.float32), rois, P, H, W, form)
    positions(s, ix64, iy64, H, W)


def test_roipool_reference():
    H, W = MAP
    for R, C in (RU.POOL_SMALL, RU.POOL_BIG):
        _, arg = RU.roipool_ref(R, C)
        assert (arg < 0).any() and (arg >= 0).any()
        for dt in (F32, BF16):
            dout = RU.dout_for(R, RU.POOL_P, C, dt)
            zero = np.zeros((H * W, C), np.float32)
            ref, ab, nt = RU.roipool_bwd_ref(dout, arg, H, W, zero)
            check(RU.roipool_bwd_oracle(dout, arg, H, W), ref, ab, nt, 'f32', what='the oracle\'s roi_pool_bwd')
            d0 = RU.feat_for(H, W, C, F32)
            ref, ab, nt = RU.roipool_bwd_ref(dout, arg, H, W, d0)
            note('float32 form, roipool backward', check(RU.roipool_bwd_f32(dout, arg, H, W, d0), ref, ab, nt, 'f32', what='roipool backward %d x %d' % (R, C)))
            assert np.array_equal(ref[nt == 1], f64(d0)[nt == 1])                    # an element nothing chose keeps its value


def expect_caught(bad, ref, ab, nt, store, what):
    with pytest.raises(AssertionError):
        check(bad, ref, ab, nt, store)
    print('caught: %s' % what)


def test_bound_catches_structural_errors():
    H, W = MAP
    P, R = 7, 24
    geo = RU.geometry('roialign', H, W)
    # ---- forward
    C = 37
    rois, feat = RU.rois_for('shared', R, H, W), RU.feat_for(H, W, C, F32)
    s = RU.sample32(rois, H, W, P, *geo)
    ref, ab, nt = RU.crop_ref(feat, s, C)
    good = RU.crop_fwd_f32(feat, s, C, F32)
    assert check(good, ref, ab, nt, 'f32') <= 1.0
    pix, w = RU.taps(s, H, W, np.float64)
    r, py, px = RU.WHOLE, 3, 2
    cell = (r * P + py) * P + px
    assert (pix[r, py, px] >= 0).all() and w[r, py, px].min() > 0.01
    bad = good.copy(); bad[cell] -= (w[r, py, px, 3] * f64(feat[pix[r, py, px, 3]])).astype(np.float32)
    expect_caught(bad, ref, ab, nt, 'f32', 'one tap dropped')
    expect_caught(RU.crop_ref(feat, s._replace(wx1=s.wy1, wy1=s.wx1), C)[0], ref, ab, nt, 'f32', 'wx1 and wy1 exchanged')
    bad = good.copy(); bad[cell] = good[cell + 1]
    expect_caught(bad, ref, ab, nt, 'f32', 'a bin taken from its neighbour')
    edge = np.pad(feat.reshape(H, W, C), ((1, 1), (1, 1), (0, 0)), mode='edge').reshape(-1, C)
    clamped = RU.crop_ref(edge, s._replace(x0=s.x0 + 1, y0=s.y0 + 1), C, SCALAR, H + 2, W + 2)[0]
    expect_caught(clamped, ref, ab, nt, 'f32', 'an out-of-map tap clamped instead of dropped')
    # ---- the chunk seam: RoI 256 of 257
    C, R = 96, 257
    rois, dout = RU.rois_for('shared', R, H, W), RU.dout_for(R, P, C, F32)
    s = RU.sample32(rois, H, W, P, *geo)
    ref, ab, nt = RU.crop_bwd_ref(dout, s, H, W)
    assert check(RU.crop_bwd_f32(dout, s, H, W), ref, ab, nt, 'f32') <= 1.0
    less = dout.copy(); less[256 * P * P:] = 0
    expect_caught(RU.crop_bwd_f32(less, s, H, W), ref, ab, nt, 'f32', 'RoI 256 missing from the backward')
    # ---- the window seam: entry 2049 of a pixel's list
    C, R = 64, 300
    rois, dout = RU.rois_for('seam', R, H, W), RU.dout_for(R, P, C, F32)
    s = RU.sample32(rois, H, W, P, *geo)
    ref, ab, nt = RU.crop_bwd_ref(dout, s, H, W)
    good = RU.crop_bwd_f32(dout, s, H, W)
    assert check(good, ref, ab, nt, 'f32') <= 1.0
    per = RU.entries_per_pixel(s, H, W, 0, RU.CHUNK)
    y, x = np.unravel_index(int(np.where(per > RU.WINDOW, ab.sum(1).reshape(H, W), 0.0).argmax()), per.shape)     # of the long lists, the heaviest
    er, ey, ex, ew = RU.pixel_entries(s, H, W, y, x, 0, RU.CHUNK)
    assert RU.WINDOW < len(er) == per[y, x] < 2300
    k = RU.WINDOW                                                                     # the first entry of the second window
    bad = good.copy(); bad[y * W + x] -= (ew[k] * f64(dout[(er[k] * P + ey[k]) * P + ex[k]])).astype(np.float32)
    expect_caught(bad, ref, ab, nt, 'f32', 'entry 2049 of the %d of pixel (%d, %d) missing' % (per[y, x], y, x))
    # ---- a bf16 store
    C, R = 36, 24
    rois, feat = RU.rois_for('shared', R, H, W), RU.feat_for(H, W, C, BF16)
    s = RU.sample32(rois, H, W, P, *geo)
    ref, ab, nt = RU.crop_ref(feat, s, C)
    b16 = RU.crop_fwd_f32(feat, s, C, BF16)
    assert check(b16, ref, ab, nt, 'bf16') <= 1.0
    i = np.unravel_index(int(np.abs(ref).argmax()), ref.shape)
    bits = b16.view(np.uint32).copy(); bits[i] += np.uint32(2 << 16)
    expect_caught(bits.view(np.float32), ref, ab, nt, 'bf16', 'a bf16 crop stored two bf16 steps off')
    # ---- RoI max pooling: a tie
    R, C = RU.POOL_SMALL
    out, arg = RU.roipool_ref(R, C)
    dout, d0 = RU.dout_for(R, RU.POOL_P, C, F32), RU.feat_for(H, W, C, F32)
    ref, ab, nt = RU.roipool_bwd_ref(dout, arg, H, W, d0)
    assert check(RU.roipool_bwd_f32(dout, arg, H, W, d0), ref, ab, nt, 'f32') <= 1.0
    fm = RU.pool_feat(C).reshape(H, W, C)
    # bin (0, 0) of RoI 0, the whole image: rows [0, 3), columns [0, 4) (27 x 21 cells over 7 x 7 bins)
    win = fm[0:3, 0:4].reshape(12, C)
    ties = [(c, np.nonzero(win[:, c] == win[:, c].max())[0]) for c in range(C)]
    c, at = next((c, at) for c, at in ties if len(at) > 1)
    to_pix = lambda k: (k // 4) * W + k % 4
    assert arg[0, c] == to_pix(at[0]) and out[0, c] == win[at[0], c]                  # the first maximum in scan order
    other = arg.copy(); other[0, c] = to_pix(at[1])
    expect_caught(RU.roipool_bwd_f32(dout, other, H, W, d0), ref, ab, nt, 'f32', 'one roipool gradient sent to the second maximum of a tie')


def test_zz_figures():
    """prints what the docstring records (needs the whole file to have run in this process)"""
    print('worst |position32 - position64| / (2^-24 size): dx %.3g, dy %.3g; %d of %d positions on the other side of an integer' % (
        POS['dx'], POS['dy'], POS['flips'], POS['n']))
    print('worst check ratios:', ', '.join('%s %.3g' % kv for kv in sorted(WORST.items())))
    assert all(w <= 1.0 for w in WORST.values())
