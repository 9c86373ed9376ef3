"""The float64 references of tests/small_kernels_util.py and its bound, pinned without a GPU: for every operation the plain torch-CPU float32
form goes through `check` against the float64 reference on the case tables the GPU file uses, with the libm allowance L = 1.  That shows
the references state the operations (torch's own matmul, pooling and elementwise arithmetic agree with them) and that the bound is not
tighter than honest float32 arithmetic; it also shows the bound is not idle: a dropped, doubled or misplaced term fails it."""
import numpy as np
import pytest
import torch

import small_kernels_util as SU
from small_kernels_util import check, F32, BF16, STORE

WORST = {}


def note(name, w):
    WORST[name] = max(WORST.get(name, 0.0), w)
    return w


@pytest.mark.parametrize('c', SU.LIN_FWD, ids=SU.case_id)
def test_linear_fwd_reference(c):
    inp = SU.lin_fwd_make(c)
    for bias, act, acc in SU.LIN_FWD_VARIANTS:
        ref, ab, nt = SU.lin_fwd_ref(inp, bias, act, acc)
        w = note('linear_fwd', check(SU.lin_fwd_f32(inp, bias, act, acc), ref, ab, nt, 'f32', libm=1.0 if act == 2 else 0.0, what=str((c, bias, act, acc))))
    print('linear_fwd', SU.case_id(c), 'worst ratio %.3g' % w)


@pytest.mark.parametrize('c', SU.LIN_BWD_X, ids=SU.case_id_x)
def test_linear_bwd_x_reference(c):
    inp = SU.lin_bwd_x_make(c)
    for acc, mul, _ in SU.LIN_BWD_X_VARIANTS:
        ref, ab, nt = SU.lin_bwd_x_ref(inp, acc, mul)
        note('linear_bwd_x', check(SU.lin_bwd_x_f32(inp, acc, mul), ref, ab, nt, 'f32', what=str((c, acc, mul))))


@pytest.mark.parametrize('c', SU.LIN_BWD_W, ids=SU.case_id)
def test_linear_bwd_w_reference(c):
    inp = SU.lin_bwd_w_make(c)
    (dw, dwa, nt), (db, dba, _) = SU.lin_bwd_w_ref(inp)
    gw, gb = SU.lin_bwd_w_f32(inp)
    note('linear_bwd_w', check(gw, dw, dwa, nt, 'f32', what=str(c)))
    note('linear_bwd_w', check(gb, db, dba, nt, 'f32', what=str(c)))


def test_bound_catches_structural_errors():
    """one dropped term of a K = 3350 dot product, one doubled term, one row read from its neighbour, a missing bias, and a sum stored two bf16 steps off"""
    c = (5, 70, 3350, '', {})
    inp = SU.lin_fwd_make(c)
    ref, ab, nt = SU.lin_fwd_ref(inp, True, 0, False)
    good = SU.lin_fwd_f32(inp, True, 0, False)
    assert check(good, ref, ab, nt, 'f32') <= 1.0
    x, w = torch.from_numpy(inp['x']), torch.from_numpy(inp['w'])
    dropped = good - (x[:, -1:] * w[:, -1][None]).numpy()
    doubled = good + (x[:, 7:8] * w[:, 7][None]).numpy()
    shifted = good.copy(); shifted[2] = good[3]
    nobias = good - inp['b'][None]
    for bad in (dropped, doubled, shifted, nobias):
        with pytest.raises(AssertionError):
            check(bad, ref, ab, nt, 'f32')
    inp = SU.lin_fwd_make((5, 70, 37, '', {}))                                       # (a short sum: the store's half unit is the whole bound)
    ref, ab, nt = SU.lin_fwd_ref(inp, True, 0, False)
    b16 = SU.bf16r(SU.lin_fwd_f32(inp, True, 0, False))
    assert check(b16, ref, ab, nt, 'bf16') <= 1.0
    bits = b16.view(np.uint32).copy(); bits[0, 0] += np.uint32(2 << 16)              # two bf16 values on: at least 1.5 units from the reference
    with pytest.raises(AssertionError):
        check(bits.view(np.float32), ref, ab, nt, 'bf16')
    with pytest.raises(AssertionError):                                              # a ReLU-masked zero has to be exact
        check(np.array([1e-30]), np.array([0.0]), np.array([0.0]), 3, 'f32')
    with pytest.raises(AssertionError):
        check(np.array([np.nan]), np.array([0.0]), np.array([1.0]), 3, 'f32')


def test_dot_product_bound_is_not_idle_nor_tight():
    """the figures the bound was chosen on: honest float32 dot products up to K = 4096 stay well inside it, a bf16 store just inside"""
    rs = np.random.RandomState(0)
    w32 = w16 = 0.0
    for K in (4, 37, 512, 3350, 4096):
        x, w = SU.rnd(rs, (8, K)), SU.rnd(rs, (64, K))
        ref, ab = SU.f64(x) @ SU.f64(w).T, np.abs(SU.f64(x)) @ np.abs(SU.f64(w)).T
        got = (torch.from_numpy(x) @ torch.from_numpy(w).t())
        w32 = max(w32, check(got.numpy(), ref, ab, K, 'f32'))
        w16 = max(w16, check(got.bfloat16().float().numpy(), ref, ab, K, 'bf16'))
    print('dot products: f32 worst ratio %.3g, bf16 store %.3g' % (w32, w16))
    assert w32 < 0.5 and 0.25 < w16 <= 1.0


@pytest.mark.parametrize('c', SU.ADD3, ids=lambda c: '%d-%s-b%d-c%d' % (c[0], STORE[c[1]], c[2], c[3]))
def test_add3_reference(c):
    n, dt, hb, hc = c[:4]
    inp = SU.add3_make(c)
    ref, ab, nt = SU.add3_ref(inp, hb, hc)
    note('add3', check(SU.add3_f32(inp, hb, hc, dt), ref, ab, nt, STORE[dt], what=str(c)))


@pytest.mark.parametrize('n', SU.ELT_N)
def test_elementwise_references(n):
    for dt in (F32, BF16):
        inp = SU.elt_make(n, dt)
        a, b, mask = (torch.from_numpy(inp[k]) for k in ('a', 'b', 'mask'))
        for has_ref in (True, False):
            ref, ab, nt = SU.scale_mask_ref(inp, has_ref)
            z = a * mask
            if has_ref:
                z = torch.where(b > 0, z, torch.zeros(()))
            check(SU.stored_as(z, dt), ref, ab, nt, STORE[dt], what='scale_mask')
    inp = SU.elt_make(n, F32)
    f, g, y, mask = (torch.from_numpy(inp[k]) for k in ('f', 'g', 'y', 'mask'))
    for act in (0, 1, 2):
        ref, ab, nt = SU.act_bwd_ref(inp, act)
        z = f if act == 0 else torch.where(y > 0, f, torch.zeros(())) if act == 1 else f * (1 - y * y)
        check(z.numpy(), ref, ab, nt, 'f32', what='act_bwd %d' % act)
    for has_mul in (True, False):
        ref, ab, nt = SU.mask_relu_ref(inp, has_mul)
        z = torch.where(g > 0, f * mask if has_mul else f, torch.zeros(()))
        check(z.numpy(), ref, ab, nt, 'f32', what='mask_relu_cast')
        check(z.bfloat16().float().numpy(), ref, ab, nt, 'bf16', what='mask_relu_cast')


@pytest.mark.parametrize('c', SU.AVGPOOL, ids=lambda c: 'C%d-%s-hw%d-n%d' % (c[0], STORE[c[1]], c[2], c[3]))
def test_avgpool_references(c):
    dt = c[1]
    inp = SU.avgpool_make(c)
    ref, ab, nt = SU.avgpool_fwd_ref(inp)
    note('avgpool_fwd', check(SU.avgpool_fwd_f32(inp, dt), ref, ab, nt, STORE[dt], what=str(c)))
    for ha in (True, False):
        for hr in (True, False):
            ref, ab, nt = SU.avgpool_bwd_ref(inp, ha, hr)
            note('avgpool_bwd', check(SU.avgpool_bwd_f32(inp, ha, hr, dt), ref, ab, nt, STORE[dt], what=str((c, ha, hr))))


@pytest.mark.parametrize('hw', SU.POOL_MAPS, ids=lambda m: '%dx%d' % m)
def test_adaptive_pool_references(hw):
    H, W = hw
    P, nbin, nper = SU.pool_matrix(H, W, SU.POOL_OUT, SU.POOL_OUT)
    assert np.allclose(P.sum(1), 1.0) and (P > 0).sum(0).min() >= 1          # every bin is a mean, every pixel is in a bin
    for name, dt, C, ldy, has_pm in SU.POOL_FWD_FORMS:
        inp = SU.pool_make(H, W, C, dt, 1)
        ref, ab, nt = SU.pool_fwd_ref(inp, H, W, has_pm)
        note('adaptive_pool_fwd', check(SU.pool_fwd_f32(inp, H, W, has_pm, dt), ref, ab, nt, STORE[dt], what=name))
    for name, dt, C, lddy, oa, om, has_pm, has_ref, _ in SU.POOL_BWD_FORMS:
        inp = SU.pool_make(H, W, C, dt, 2)
        ref, ab, nt = SU.pool_bwd_ref(inp, H, W, has_pm, has_ref)
        note('adaptive_pool_bwd', check(SU.pool_bwd_f32(inp, H, W, has_pm, has_ref, dt), ref, ab, nt, STORE[dt], what=name))
    # the backward reference is the transpose of the forward one: autograd through torch's own pooling gives the same numbers
    inp = SU.pool_make(H, W, 5, F32, 3)
    x = torch.from_numpy(inp['x']).double().view(H, W, 5).permute(2, 0, 1)[None].requires_grad_(True)
    y = torch.nn.functional.adaptive_avg_pool2d(x, SU.POOL_OUT)
    y.backward(torch.from_numpy(inp['dy_all']).double().view(SU.POOL_OUT, SU.POOL_OUT, 5).permute(2, 0, 1)[None])
    ref, _, _ = SU.pool_bwd_ref(inp, H, W, False, False)
    assert np.abs(x.grad[0].permute(1, 2, 0).reshape(H * W, 5).numpy() - ref).max() < 1e-12


@pytest.mark.parametrize('c', SU.MASK_DOWN, ids=lambda c: '%dx%d-%dx%d' % c)
def test_mask_downsample_reference(c):
    H, W, h, w = c
    m = SU.mask_down_make(H, W, h, w)
    ref, half = SU.mask_down_ref(m, h, w)
    if (H, W) == (160, 224):
        assert half >= 3                                                     # the >= 0.5 edge is in the table
    pooled = torch.nn.functional.adaptive_avg_pool2d(torch.from_numpy(m).double()[None, None], (h, w))[0, 0]
    assert np.array_equal((pooled >= 0.5).float().numpy(), ref) and 0 < ref.sum() < ref.size


@pytest.mark.parametrize('rows', SU.COLSUM_ROWS)
def test_colsum_reference(rows):
    for cols in SU.COLSUM_COLS:
        for dt in (F32, BF16):
            inp = SU.colsum_make(rows, cols, dt)
            ref, ab, nt = SU.colsum_ref(inp)
            note('colsum', check(SU.colsum_f32(inp), ref, ab, nt, 'f32', what=str((rows, cols, dt))))
    assert [SU.colsum_ranges(r) for r in SU.COLSUM_ROWS] == [1, 1, 1, 3, 32]


def test_sgd_reference():
    chunk = 4096
    inp = SU.sgd_make(chunk)
    segs, tot = inp['segs'], inp['tot']
    assert segs[1]['offset'] % 4 != 0 and segs[2]['offset'] % 4 == 0 and [s['count'] for s in segs] == [3, chunk + 1, 36, 60, chunk]
    assert [s['chunk0'] for s in segs] == [0, 1, 3, 4, 5]
    hyper = (0.01, 0.9, 1e-2, 0.5)
    (P, PA), (M, MA), (S, SA) = SU.sgd_ref(inp, *hyper)
    p, m, s = SU.sgd_f32(inp, *hyper)
    inside = ~np.isnan(S)
    assert inside.sum() == sum(sg['count'] for sg in segs) < tot
    note('sgd', check(p, P, PA, 3, 'f32', what='param'))
    note('sgd', check(m, M, MA, 3, 'f32', what='momentum'))
    note('sgd', check(s[inside], S[inside], SA[inside], 3, 'f32', what='shadow f32'))
    note('sgd', check(SU.bf16r(s[inside]), S[inside], SA[inside], 3, 'bf16', what='shadow bf16'))
    assert np.array_equal(p[~inside], inp['p'][~inside]) and np.array_equal(m[~inside], inp['m'][~inside])


# ------------------------------------------------------------------------------------------------------------------ losses and heads
def run_outs(name, got, ref, stores=None, what=''):
    for k, o in ref.items():
        note(name, SU.check_out(got[k], o, (stores or {}).get(k, 'f32'), 1.0, '%s %s %s' % (name, what, k)))


@pytest.mark.parametrize('c', SU.LSM, ids=lambda c: 'S%d-V%d-x%g' % c)
def test_logsoftmax_nll_reference(c):
    inp = SU.lsm_make(c)
    run_outs('logsoftmax_nll', SU.lsm_f32(inp), SU.lsm_ref(inp), what=str(c))


def test_head_references():
    for c in SU.RCNN_PRED:
        inp = SU.rcnn_pred_make(c)
        run_outs('rcnn_predict', SU.rcnn_pred_f32(inp, c[1]), SU.rcnn_pred_ref(inp, c[1]), what=str(c))
    for c in SU.MASK_PROB:
        inp = SU.mask_prob_make(c)
        note('mask_prob', SU.check_out(SU.mask_prob_f32(inp, c), SU.mask_prob_ref(inp, c), 'f32', 1.0, 'mask_prob %s' % (c,)))


@pytest.mark.parametrize('c', SU.MASK_LOSS, ids=lambda c: 'ms%d-ld%d-x%g' % c)
def test_mask_loss_reference(c):
    inp = SU.mask_loss_make(c)
    for num_fg in SU.MASK_NUM_FG:
        ref = SU.mask_loss_ref(inp, c[0], num_fg)
        run_outs('mask_loss', SU.mask_loss_f32(inp, c[0], num_fg), ref, what='%s num_fg %d' % (c, num_fg))
        if num_fg == 0:
            assert ref['loss']['ref'] == 0 and not ref['dscore']['ref'].any()


@pytest.mark.parametrize('c', SU.MASKPRED, ids=lambda c: 'C%d-ms%d-%s' % (c[0], c[1], STORE[c[2]]))
def test_maskpred_bwd_reference(c):
    inp = SU.maskpred_make(c)
    for num_fg in SU.MASK_NUM_FG:
        for has_ref in (True, False):
            run_outs('maskpred_bwd', SU.maskpred_f32(inp, c[1], num_fg, has_ref, c[2]), SU.maskpred_ref(inp, c[1], num_fg, has_ref), stores=dict(dx=STORE[c[2]]),
                     what='%s num_fg %d' % (c, num_fg))


@pytest.mark.parametrize('c', SU.RPN, ids=lambda c: '%dx%dx%d' % c)
def test_rpn_loss_reference(c):
    A = c[2]
    for scale in SU.RPN_SCALES:
        for none in (False, True):
            inp = SU.rpn_make(c, scale, none)
            for ldd in (6 * A, 6 * A + 8):
                for dt in (F32, BF16):
                    ref = SU.rpn_ref(inp, c, ldd)
                    run_outs('rpn_loss', SU.rpn_f32(inp, c, ldd, dt), ref, stores=dict(dheads=STORE[dt]), what='%s x%g ldd %d' % (c, scale, ldd))
            if none:
                assert ref['loss_cls']['ref'] == 0 and ref['loss_box']['ref'] == 0 and not ref['dheads']['ref'].any()
    # the oracle's smooth L1 (mean over the batch of the sums over the other dimensions) is the box loss of the reference
    from oracle import net as ON
    inp = SU.rpn_make(c, 1.0)
    H, W = c[:2]
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64)).view(1, H, W, 4 * A)
    ora = ON.OracleNet.smooth_l1(t(inp['heads'][:, 2 * A:]), t(inp['tgt']), t(inp['inw']), t(inp['outw']), SU.RPN_SIGMA, [1, 2, 3])
    assert abs(float(ora) - SU.rpn_ref(inp, c, 6 * A)['loss_box']['ref']) < 1e-12


@pytest.mark.parametrize('c', SU.RCNN, ids=lambda c: 'R%d-ncls%d' % c)
def test_rcnn_loss_reference(c):
    for scale in (1.0, 100.0):
        inp = SU.rcnn_make(c, scale)
        for ldd in (5 * c[1], 5 * c[1] + 8):
            for dt in (F32, BF16):
                run_outs('rcnn_loss', SU.rcnn_f32(inp, c, ldd, dt), SU.rcnn_ref(inp, c, ldd), stores=dict(dheads=STORE[dt]), what='%s x%g' % (c, scale))
    from oracle import net as ON
    inp = SU.rcnn_make(c, 1.0)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    ora = ON.OracleNet.smooth_l1(t(inp['heads'][:, c[1]:]), t(inp['bt']), t(inp['bi']), t(inp['bo']), 1.0, [1])
    assert abs(float(ora) - SU.rcnn_ref(inp, c, 5 * c[1])['loss_box']['ref']) < 1e-12


@pytest.mark.parametrize('c', SU.RESPONSE, ids=lambda c: '%dx%d-%dx%d' % c)
def test_response_loss_reference(c):
    from oracle import boxes as OB
    for scale in (1.0, 100.0):
        inp = SU.response_make(c, scale)
        target = OB.imresize_nearest_u8(inp['mask'], (c[2], c[3]))
        assert target.shape == (c[2], c[3]) and 0 < target.sum() < target.size
        run_outs('response_loss', SU.response_f32(inp, c, target), SU.response_ref(inp, c, target), what=str(c))
    if c[0] == c[2]:
        assert np.array_equal(target, inp['mask'])


def test_total_loss_reference():
    l = SU.rnd(np.random.RandomState(1), (8,))
    for cap_w in (0.0, 0.5):
        t = torch.from_numpy(l)
        got = t[0] + t[1] + t[2] + t[3] + t[4] + t[7] + np.float32(cap_w) * t[5]
        SU.check_out(got.numpy(), SU.total_loss_ref(l, cap_w), 'f32', 1.0, 'total_loss')


@pytest.mark.parametrize('c', SU.EMBED, ids=lambda c: 'D%d-T%d-%s-m%d-r%d' % c)
def test_embed_reference(c):
    inp = SU.embed_make(c)
    ref = SU.embed_ref(inp, c)
    got = SU.embed_f32(inp, c)
    assert np.array_equal(got['out'], inp['out'])                          # what the backward kernel is handed is the forward's own bits
    run_outs('embed', got, ref, what=str(c))


@pytest.mark.parametrize('c', SU.DYNFILTER, ids=lambda c: '%dx%d-C%d-%s' % (c[0][0], c[0][1], c[1], STORE[c[2]]))
def test_dynfilter_reference(c):
    from oracle import net as ON
    (H, W), C, dt = c[:3]
    masks = ON.spatial_masks(H, W)
    inp = SU.dynfilter_make(c, masks)
    assert np.array_equal(inp['m'].T.reshape(7, H, W), masks)
    for gate in (0, 1):
        run_outs('dynfilter_fwd', SU.dynfilter_fwd_f32(inp, gate, dt), SU.dynfilter_fwd_ref(inp, gate), stores=dict(y=STORE[dt]), what='%s gate %d' % (c[:3], gate))
        for has_extra in (True, False):
            for has_ref in (True, False):
                run_outs('dynfilter_bwd', SU.dynfilter_bwd_f32(inp, gate, has_extra, has_ref, dt), SU.dynfilter_bwd_ref(inp, gate, has_extra, has_ref),
                         stores=dict(dx=STORE[dt]), what='%s gate %d extra %d ref %d' % (c[:3], gate, has_extra, has_ref))
    if C == 36 and dt == F32:
        # the references are the gradients of the forward: autograd through the same expression in float64
        x = torch.from_numpy(inp['x']).double().requires_grad_(True)
        filt, r = torch.from_numpy(inp['filt']).double().requires_grad_(True), torch.from_numpy(inp['r']).double().requires_grad_(True)
        m = torch.from_numpy(inp['m'])
        resp = ((x @ filt.t()) * m) @ r
        (x * resp[:, None] * torch.from_numpy(inp['dy']).double()).sum().backward()
        ref = SU.dynfilter_bwd_ref(dict(inp, resp=resp.detach().numpy(), respk=((x @ filt.t()) * m).detach().numpy()), 0, False, False)
        assert np.abs(ref['dx']['ref'] - x.grad.numpy()).max() < 1e-9
        assert np.abs(ref['dfilt']['ref'] - inp['dfilt0'] - filt.grad.numpy()).max() < 1e-9 and np.abs(ref['dr']['ref'] - inp['dr0'] - r.grad.numpy()).max() < 1e-9


def test_print_worst_ratios():
    print('worst check ratios of the torch-CPU float32 forms:', ', '.join('%s %.3g' % kv for kv in sorted(WORST.items())))
