"""Every dispatch branch of the small kernels (csrc/lang.hip linears, csrc/misc_kernels.hip elementwise / pools / column sums / SGD) against
the float64 references of tests/small_kernels_util.py, through its one elementwise bound `check` (derived there, pinned without a GPU by
tests/test_small_kernels_cpu.py).  Each case names the kernel the dispatcher has to pick and asserts ops.last_kernel() says so; the last
test of the file asserts that the kernels seen are exactly KERNELS, so a later change of a dispatch rule cannot drop a branch from the
suite without saying so (it needs the whole file to have run in this process).

Every output buffer is one row (and ld - cols columns) larger than what the call may write, pre-filled with a sentinel, and has to come
back bit-identical outside the written region; inputs carry the same padding, so a read beyond a row shows as a wrong sum.  Workspaces,
which may hold anything, start as NaN.  Integer / mask outputs, ReLU-masked zeros and everything "bit for bit" are exact.

The libm allowance L_LIBM.  tanhf is measured alone: the kernel's act = 2 output against the float64 tanh of the same kernel's act = 0
output.  The other libm-bearing entry points are measured on the outputs that ARE libm values (class and mask probabilities, caption
log-probabilities, float32 stores, ordinary N(0, 1) logits): the plain |got - ref| / (2^-23 |value|) against the float64 reference.
L_LIBM is four times the largest of these, rounded up to a power of two; the last test of the file asserts that rule on every run.
Outputs that subtract something from a libm value (p - 1) take the allowance on the libm value (`mag`), not on the difference.

Worst values measured on an MI355X (this file's own prints):
  libm, |got - ref| / (2^-23 |value|)   rcnn_predict 1.66, logsoftmax_nll log-probabilities 1.63, tanhf 1.22, mask_prob 0.923
                                        -> 4 x 1.66 = 6.6 -> L_LIBM = 8
  worst check ratio per entry point     linear_fwd 0.096, linear_bwd_x 0.264, linear_bwd_w 0.431, add3 0.996 (bf16 store), add_f32 0.333, mul 0.333,
                                        scale_mask 0 (masks of 0 and 2: exact), act_bwd 0.292, mask_relu_cast 0.996 (bf16), avgpool_fwd 0.98 (bf16),
                                        avgpool_bwd 0.996 (bf16), adaptive_pool_fwd 0.996 (bf16), adaptive_pool_bwd 0.996 (bf16), colsum 0.25,
                                        sgd 0.995 (bf16 shadow), sgd g16 0.238, rpn_loss 0.967 (bf16 dheads), rcnn_loss 0.973 (bf16 dheads),
                                        mask_loss 0.278, maskpred_bwd 0.996 (bf16 dx), response_loss 0.167, logsoftmax_nll 0.246, rcnn_predict 0.237,
                                        mask_prob 0.25, embed 0.429, dynfilter_fwd 0.984 (bf16 y), dynfilter_bwd 0.994 (bf16 dx)
  (a ratio next to 1 is a bf16 store: half a unit in the last place is the whole bound there; every float32 output stays below 0.45)
  cast, fill, mask_downsample, embed_fwd, every canary, every "bit for bit" pair (two runs of linear_bwd_x, the ranged / sharded SGD, the
  split forms of maskpred_bwd and dynfilter_bwd): exact

Kernels whose name can never be the LAST launch of an entry point (count_labels_kernel in front of rpn_loss_kernel, the first passes of the
dynamic filter's backward) are run by their cases but cannot be named here; linear_fwd_kernel<8,4,1>, <16,4,1> and <24,4,1> cannot be reached."""
import ctypes as C
import numpy as np
import pytest
import torch

import small_kernels_util as SU
from small_kernels_util import check, F32, BF16, STORE
from gpu_buf import DEV, TDT, SENTINEL, Buf, bits, same_bits

pytestmark = pytest.mark.gpu

L_LIBM = 8.0            # libm allowance (expf, logf, log1pf, tanhf), in units of 2^-23 of the value libm produced: four times the worst measured value below, rounded up to a power of two
LIBM = {}               # op -> worst measured |got - ref| / (2^-23 |value|) at ordinary logits
SEEN = set()
WORST = {}

# every kernel a case of this file lands on; TABLE_KERNELS below is what the case tables name, and the two have to agree
KERNELS = [
    'act_bwd_kernel', 'adaptive_pool_bwd_bf16x8_kernel', 'adaptive_pool_bwd_kernel', 'adaptive_pool_fwd_kernel', 'add3_bf16x8_kernel', 'add3_kernel',
    'add_f32_kernel', 'avgpool_bwd_bf16x8_kernel', 'avgpool_bwd_kernel', 'avgpool_fwd_bf16x8_kernel', 'avgpool_fwd_kernel', 'cast_kernel',
    'colsum_finish_kernel', 'colsum_kernel', 'dynfilter_bwd2_bf16_kernel', 'dynfilter_bwd2_kernel', 'dynfilter_bwd3_kernel',
    'dynfilter_fwd_bf16_kernel', 'dynfilter_fwd_kernel', 'embed_bwd_kernel', 'embed_fwd_kernel', 'fill_kernel', 'gemvT_kernel<1>', 'gemvT_kernel<8>',
    'linear_bwd_w_kernel', 'linear_fwd_kernel<1,1,1>', 'linear_fwd_kernel<1,2,1>', 'linear_fwd_kernel<1,4,1>', 'linear_fwd_kernel<16,1,1>',
    'linear_fwd_kernel<16,2,1>', 'linear_fwd_kernel<24,1,1>', 'linear_fwd_kernel<24,2,1>', 'linear_fwd_kernel<8,1,1>', 'linear_fwd_kernel<8,2,1>',
    'linear_nn_mfma_kernel<1>', 'linear_nn_mfma_kernel<2>', 'linear_nn_reduce_kernel', 'linear_nt_mfma_kernel<1>', 'linear_nt_mfma_kernel<2>',
    'linear_tn_mfma_kernel<false>', 'linear_tn_mfma_kernel<true>', 'lsm_nll_kernel', 'mask_downsample_kernel', 'mask_loss_kernel',
    'mask_prob_kernel', 'mask_relu_cast_kernel<bf16_t>', 'mask_relu_cast_kernel<float>', 'maskpred_bwd_kernel', 'maskpred_bwd_reduce_kernel',
    'mul_kernel', 'rcnn_loss_kernel', 'rcnn_predict_kernel', 'response_loss_kernel', 'rpn_loss_kernel', 'scale_mask_kernel', 'sgd_kernel',
    'total_loss_kernel',
]
TABLE_KERNELS = sorted(set(
    [c[3] for c in SU.LIN_FWD] + [c[3] for c in SU.LIN_BWD_X] + [c[3] for c in SU.LIN_BWD_W] + [c[4] for c in SU.ADD3] +
    [c[4] for c in SU.AVGPOOL] + [c[5] for c in SU.AVGPOOL] + [f[8] for f in SU.POOL_BWD_FORMS] +
    ['adaptive_pool_fwd_kernel', 'mask_downsample_kernel', 'colsum_kernel', 'colsum_finish_kernel', 'sgd_kernel', 'add_f32_kernel', 'cast_kernel',
     'mul_kernel', 'fill_kernel', 'scale_mask_kernel', 'act_bwd_kernel', 'mask_relu_cast_kernel<bf16_t>', 'mask_relu_cast_kernel<float>',
     'rpn_loss_kernel', 'rcnn_loss_kernel', 'mask_loss_kernel', 'maskpred_bwd_kernel', 'maskpred_bwd_reduce_kernel', 'response_loss_kernel', 'total_loss_kernel',
     'lsm_nll_kernel', 'rcnn_predict_kernel', 'mask_prob_kernel', 'embed_fwd_kernel', 'embed_bwd_kernel', 'dynfilter_bwd3_kernel'] +
    [c[3] for c in SU.DYNFILTER] + [c[4] for c in SU.DYNFILTER]))


def ops():
    from lang2seg_amd import ops as O
    return O


def landed(kernel):
    k = ops().last_kernel()
    SEEN.add(k)
    assert k == kernel, 'the dispatcher launched %s last, this case is meant for %s' % (k, kernel)


def note(name, w):
    WORST[name] = max(WORST.get(name, 0.0), w)


# ------------------------------------------------------------------------------------------------------------------ linears
@pytest.mark.parametrize('c', SU.LIN_FWD, ids=SU.case_id)
def test_linear_fwd(c):
    O = ops()
    M, N, K, kernel, o = c
    ldx, ldw, ldy = o.get('ldx', K), o.get('ldw', K), o.get('ldy', N)
    inp = SU.lin_fwd_make(c)
    x = Buf(M, K, ldx, o.get('xoff', 0), init=inp['x'])
    w = Buf(N, K, ldw, o.get('woff', 0), init=inp['w'])
    b = Buf(1, N, init=inp['b'])
    worst = 0.0
    for bias, act, acc in SU.LIN_FWD_VARIANTS:
        what = '%s bias %d act %d accumulate %d' % (SU.case_id(c), bias, act, acc)
        y = Buf(M, N, ldy, o.get('yoff', 0), init=inp['y0'])
        O.linear_fwd(x.t, w.t, b.t if bias else None, y.t, M, N, K, act=act, accumulate=acc, ldx=ldx, ldy=ldy, ldw=ldw)
        landed(kernel)
        ref, ab, nt = SU.lin_fwd_ref(inp, bias, act, acc)
        worst = max(worst, check(y.get(), ref, ab, nt, 'f32', libm=L_LIBM if act == 2 else 0.0, what=what))
        y.assert_untouched_outside(what)
    x.assert_unchanged(); w.assert_unchanged(); b.assert_unchanged()
    note('linear_fwd', worst)
    print('linear_fwd %s: worst ratio %.3g' % (SU.case_id(c), worst))


def test_tanhf_allowance():
    """the libm allowance: tanhf alone, the kernel's act = 2 output against the float64 tanh of the SAME kernel's act = 0 output (the same
    float32 sum), in units of 2^-23 |ref|"""
    O = ops()
    worst = 0.0
    for c in ((5, 70, 37, '', {}), (1, 70, 512, '', {}), (16, 3350, 512, '', {}), (17, 100, 2560, '', {})):
        M, N, K = c[:3]
        inp = SU.lin_fwd_make(c)
        x, w, b = Buf(M, K, init=inp['x']), Buf(N, K, init=inp['w']), Buf(1, N, init=inp['b'])
        for scale in (1.0, 3.0, 0.01):                                    # |z| up to ~12 (saturated) and down to ~1e-4 (tanh z ~ z)
            y0 = (inp['y0'] * scale).astype(np.float32)
            z, t = Buf(M, N, init=y0), Buf(M, N, init=y0)
            O.linear_fwd(x.t, w.t, b.t, z.t, M, N, K, act=0, accumulate=True)
            O.linear_fwd(x.t, w.t, b.t, t.t, M, N, K, act=2, accumulate=True)
            ref = np.tanh(SU.f64(z.get()))
            nz = ref != 0
            worst = max(worst, float((np.abs(SU.f64(t.get()) - ref)[nz] / (2.0 ** -23 * np.abs(ref[nz]))).max()))
    LIBM['tanhf (linear_fwd act 2)'] = worst
    print('tanhf: worst |got - ref| / (2^-23 |ref|) = %.3g (L_LIBM = %g)' % (worst, L_LIBM))


@pytest.mark.parametrize('c', SU.LIN_BWD_X, ids=SU.case_id_x)
def test_linear_bwd_x(c):
    O = ops()
    M, N, K, kernel, o = c
    inp = SU.lin_bwd_x_make(c)
    w = Buf(N, K, off=o.get('woff', 0), init=inp['w'])
    need = O.linear_bwd_x_ws_floats(M, N, K)
    assert need > 0 or 'ws' not in o
    worst = 0.0
    for acc, mul, strided in SU.LIN_BWD_X_VARIANTS:
        what = '%s accumulate %d mul %d strided %d' % (SU.case_id_x(c), acc, mul, strided)
        lddy, dyoff, lddx = (N + 4 * SU.R_, 4 * SU.R_, K + 3) if strided else (N, 0, K)
        dy = Buf(M, N, lddy, dyoff, init=inp['dy'])
        mb = Buf(M, K, lddx, init=inp['mul'])
        outs = []
        for rep in range(2):
            ws = None if 'ws' not in o else torch.full((need - (o['ws'] == 'short'),), float('nan'), device=DEV)
            dx = Buf(M, K, lddx, init=inp['dx0'])
            O.linear_bwd_x(dy.t, w.t, dx.t, M, N, K, accumulate=acc, lddy=lddy, lddx=lddx, mul=mb.t if mul else None, ws=ws)
            landed(kernel)
            outs.append(dx)
        ref, ab, nt = SU.lin_bwd_x_ref(inp, acc, mul)
        worst = max(worst, check(outs[0].get(), ref, ab, nt, 'f32', what=what))
        outs[0].assert_untouched_outside(what)
        assert same_bits(outs[0], outs[1]), '%s: two runs differ' % what
        dy.assert_unchanged(); mb.assert_unchanged()
    w.assert_unchanged()
    note('linear_bwd_x', worst)
    print('linear_bwd_x %s: worst ratio %.3g' % (SU.case_id_x(c), worst))


@pytest.mark.parametrize('c', SU.LIN_BWD_W, ids=SU.case_id)
def test_linear_bwd_w(c):
    O = ops()
    M, N, K, kernel, o = c
    lddy, ldx = o.get('lddy', N), o.get('ldx', K)
    inp = SU.lin_bwd_w_make(c)
    dy = Buf(M, N, lddy, o.get('dyoff', 0), init=inp['dy'])
    x = Buf(M, K, ldx, o.get('xoff', 0), init=inp['x'])
    (dwr, dwa, nt), (dbr, dba, _) = SU.lin_bwd_w_ref(inp)
    worst = 0.0
    for has_db in (True, False):
        what = '%s db %d' % (SU.case_id(c), has_db)
        dw, db = Buf(N, K, init=inp['dw0']), Buf(1, N, init=inp['db0'])
        O.linear_bwd_w(dy.t, x.t, dw.t, db.t if has_db else None, M, N, K, lddy=lddy, ldx=ldx)
        landed(kernel)
        worst = max(worst, check(dw.get(), dwr, dwa, nt, 'f32', what=what + ' dw'))
        dw.assert_untouched_outside(what)
        if has_db:
            worst = max(worst, check(db.get()[0], dbr, dba, nt, 'f32', what=what + ' db'))
            db.assert_untouched_outside(what)
        else:
            db.assert_unchanged(what)
    dy.assert_unchanged(); x.assert_unchanged()
    note('linear_bwd_w', worst)
    print('linear_bwd_w %s: worst ratio %.3g' % (SU.case_id(c), worst))


# ------------------------------------------------------------------------------------------------------------------ elementwise
@pytest.mark.parametrize('c', SU.ADD3, ids=lambda c: '%d-%s-b%d-c%d' % (c[0], STORE[c[1]], c[2], c[3]))
def test_add3(c):
    O = ops()
    n, dt, hb, hc, kernel = c
    inp = SU.add3_make(c)
    a, b, cc = Buf(1, n, dt=dt, init=inp['a'], tail=64), Buf(1, n, dt=dt, init=inp['b'], tail=64), Buf(1, n, init=inp['c'], tail=64)
    d = Buf(1, n, dt=dt, tail=64)
    O.add3(a.t, b.t if hb else None, cc.t if hc else None, d.t)
    landed(kernel)
    ref, ab, nt = SU.add3_ref(inp, hb, hc)
    w = check(d.get()[0], ref, ab, nt, STORE[dt], what=str(c))
    d.assert_untouched_outside(str(c))
    for t in (a, b, cc):
        t.assert_unchanged()
    note('add3', w)
    print('add3 %s: worst ratio %.3g' % (str(c), w))


@pytest.mark.parametrize('n', SU.ELT_N)
def test_elementwise(n):
    O = ops()
    T = 64
    for dt in (F32, BF16):
        inp = SU.elt_make(n, dt)
        a, b, mask = Buf(1, n, dt=dt, init=inp['a'], tail=T), Buf(1, n, dt=dt, init=inp['b'], tail=T), Buf(1, n, init=inp['mask'], tail=T)
        for has_ref in (True, False):
            out = Buf(1, n, dt=dt, tail=T)
            O.scale_mask(a.t, mask.t, b.t if has_ref else None, out.t)
            landed('scale_mask_kernel')
            ref, ab, nt = SU.scale_mask_ref(inp, has_ref)
            note('scale_mask', check(out.get()[0], ref, ab, nt, STORE[dt], what='scale_mask %s ref %d' % (STORE[dt], has_ref)))
            out.assert_untouched_outside('scale_mask')
        # cast: to bf16 it is one rounding of the value, every other direction is exact
        for ddt in (F32, BF16):
            out = Buf(1, n, dt=ddt, tail=T)
            O.cast(a.t, out.t)
            landed('cast_kernel')
            if dt == F32 and ddt == BF16:
                check(out.get()[0], SU.f64(inp['a']), np.abs(inp['a']), 0, 'bf16', what='cast to bf16')
                assert np.array_equal(out.get()[0], SU.bf16r(inp['a']))               # round to nearest even, the rule of every bf16 store
            else:
                assert np.array_equal(out.get()[0], inp['a'])
            out.assert_untouched_outside('cast')
        a.assert_unchanged(); b.assert_unchanged(); mask.assert_unchanged()
    inp = SU.elt_make(n, F32)
    f, g, y, mask = (Buf(1, n, init=inp[k], tail=T) for k in ('f', 'g', 'y', 'mask'))
    out = Buf(1, n, tail=T)
    O.mul(f.t, g.t, out.t)
    landed('mul_kernel')
    note('mul', check(out.get()[0], SU.f64(inp['f']) * SU.f64(inp['g']), np.abs(SU.f64(inp['f']) * SU.f64(inp['g'])), 1, 'f32', what='mul'))
    out.assert_untouched_outside('mul')
    out = Buf(1, n, tail=T)
    O.fill(out.t, 0.3)
    landed('fill_kernel')
    assert np.array_equal(out.get()[0], np.full(n, np.float32(0.3)))
    out.assert_untouched_outside('fill')
    for off in (0, 1):                                                    # an output one float off 16 bytes: the kernel's own check takes the scalar loop
        out = Buf(1, n, off=off, tail=T)
        O.add_f32(f.t, g.t, out.t)
        landed('add_f32_kernel')
        note('add_f32', check(out.get()[0], SU.f64(inp['f']) + SU.f64(inp['g']), np.abs(SU.f64(inp['f'])) + np.abs(SU.f64(inp['g'])), 1, 'f32', what='add_f32'))
        out.assert_untouched_outside('add_f32 off %d' % off)
    for act in (0, 1, 2):
        d = Buf(1, n, init=inp['f'], tail=T)
        O.act_bwd(d.t, y.t, act)
        landed('act_bwd_kernel')
        ref, ab, nt = SU.act_bwd_ref(inp, act)
        note('act_bwd', check(d.get()[0], ref, ab, nt, 'f32', what='act_bwd %d' % act))
        d.assert_untouched_outside('act_bwd')
    for odt in (F32, BF16):
        for has_mul in (True, False):
            xx, out = Buf(1, n, init=inp['f'], tail=T), Buf(1, n, dt=odt, tail=T)
            O.mask_relu_cast(xx.t, mask.t if has_mul else None, g.t, out.t)
            landed('mask_relu_cast_kernel<%s>' % ('bf16_t' if odt == BF16 else 'float'))
            ref, ab, nt = SU.mask_relu_ref(inp, has_mul)
            note('mask_relu_cast', check(xx.get()[0], ref, ab, nt, 'f32', what='mask_relu_cast x'))
            note('mask_relu_cast', check(out.get()[0], ref, ab, nt, STORE[odt], what='mask_relu_cast out'))
            xx.assert_untouched_outside('mask_relu_cast'); out.assert_untouched_outside('mask_relu_cast')
    for t in (f, g, y, mask):
        t.assert_unchanged()


# ------------------------------------------------------------------------------------------------------------------ pools
@pytest.mark.parametrize('c', SU.AVGPOOL, ids=lambda c: 'C%d-%s-hw%d-n%d' % (c[0], STORE[c[1]], c[2], c[3]))
def test_avgpool(c):
    O = ops()
    Cc, dt, hw, n, kf, kb = c
    inp = SU.avgpool_make(c)
    x, y = Buf(n * hw, Cc, dt=dt, init=inp['x']), Buf(n, Cc, dt=dt)
    O.avgpool_fwd(x.t, y.t, n, hw, Cc)
    landed(kf)
    ref, ab, nt = SU.avgpool_fwd_ref(inp)
    note('avgpool_fwd', check(y.get(), ref, ab, nt, STORE[dt], what=str(c)))
    y.assert_untouched_outside(str(c)); x.assert_unchanged()
    dy, ad, rf = Buf(n, Cc, dt=dt, init=inp['dy']), Buf(n * hw, Cc, dt=dt, init=inp['addend']), Buf(n * hw, Cc, dt=dt, init=inp['ref'])
    for ha in (True, False):
        for hr in (True, False):
            what = '%s addend %d ref %d' % (str(c), ha, hr)
            dx = Buf(n * hw, Cc, dt=dt)
            O.avgpool_bwd(dy.t, dx.t, ad.t if ha else None, rf.t if hr else None, n, hw, Cc)
            landed(kb)
            ref, ab, nt = SU.avgpool_bwd_ref(inp, ha, hr)
            note('avgpool_bwd', check(dx.get().reshape(n, hw, Cc), ref, ab, nt, STORE[dt], what=what))
            dx.assert_untouched_outside(what)
    for t in (dy, ad, rf):
        t.assert_unchanged()


@pytest.mark.parametrize('which', ['dx', 'dy', 'addend', 'ref'])
def test_avgpool_bwd_misaligned_view(which):
    """bf16, C % 8 == 0, one operand a view that starts one element (2 bytes) off: the 16-byte kernel may not take it"""
    O = ops()
    c = (8, BF16, 49, 5)
    Cc, dt, hw, n = c
    inp = SU.avgpool_make(c)
    off = {k: int(k == which) for k in ('dx', 'dy', 'addend', 'ref')}
    dy = Buf(n, Cc, dt=dt, off=off['dy'], init=inp['dy'])
    ad, rf = Buf(n * hw, Cc, dt=dt, off=off['addend'], init=inp['addend']), Buf(n * hw, Cc, dt=dt, off=off['ref'], init=inp['ref'])
    dx = Buf(n * hw, Cc, dt=dt, off=off['dx'])
    O.avgpool_bwd(dy.t, dx.t, ad.t, rf.t, n, hw, Cc)
    landed('avgpool_bwd_kernel')
    ref, ab, nt = SU.avgpool_bwd_ref(inp, True, True)
    check(dx.get().reshape(n, hw, Cc), ref, ab, nt, 'bf16', what='misaligned ' + which)
    dx.assert_untouched_outside(which)


@pytest.mark.parametrize('hw', SU.POOL_MAPS, ids=lambda m: '%dx%d' % m)
def test_adaptive_pool(hw):
    O = ops()
    H, W = hw
    OO = SU.POOL_OUT * SU.POOL_OUT
    for name, dt, Cc, ldy, has_pm in SU.POOL_FWD_FORMS:
        inp = SU.pool_make(H, W, Cc, dt, 1)
        x, pm, y = Buf(H * W, Cc, dt=dt, init=inp['x']), Buf(1, H * W, init=inp['pm']), Buf(OO, Cc, ldy, dt=dt)
        O.adaptive_pool_fwd(x.t, pm.t if has_pm else None, y.t, H, W, Cc, SU.POOL_OUT, SU.POOL_OUT, ldy)
        landed('adaptive_pool_fwd_kernel')
        ref, ab, nt = SU.pool_fwd_ref(inp, H, W, has_pm)
        note('adaptive_pool_fwd', check(y.get(), ref, ab, nt, STORE[dt], what='fwd ' + name))
        y.assert_untouched_outside('fwd ' + name); x.assert_unchanged()
    for name, dt, Cc, lddy, oa, om, has_pm, has_ref, kernel in SU.POOL_BWD_FORMS:
        inp = SU.pool_make(H, W, Cc, dt, 2)
        wide = SU.rnd(np.random.RandomState(9), (OO, lddy), dt)            # what lies beside the two column blocks is data of somebody else
        wide[:, om:om + Cc] = inp['dy_mask']                               # (without a pixel mask nothing may read this block; it may overlap the next)
        wide[:, oa:oa + Cc] = inp['dy_all']
        if not has_pm:
            wide[:, om:om + Cc][:, [j for j in range(Cc) if not oa <= om + j < oa + Cc]] = np.float32('nan')
        dy, pm = Buf(OO, lddy, dt=dt, init=wide), Buf(1, H * W, init=inp['pm'])
        rf, dx = Buf(H * W, Cc, dt=dt, init=inp['ref']), Buf(H * W, Cc, dt=dt)
        O.adaptive_pool_bwd(dy.t, lddy, oa, om, pm.t if has_pm else None, dx.t, rf.t if has_ref else None, H, W, Cc, SU.POOL_OUT, SU.POOL_OUT)
        landed(kernel)
        ref, ab, nt = SU.pool_bwd_ref(inp, H, W, has_pm, has_ref)
        note('adaptive_pool_bwd', check(dx.get(), ref, ab, nt, STORE[dt], what='bwd %s %dx%d' % (name, H, W)))
        dx.assert_untouched_outside('bwd ' + name); dy.assert_unchanged(); rf.assert_unchanged()


@pytest.mark.parametrize('c', SU.MASK_DOWN, ids=lambda c: '%dx%d-%dx%d' % c)
def test_mask_downsample(c):
    O = ops()
    H, W, h, w = c
    m = SU.mask_down_make(H, W, h, w)
    ref, _ = SU.mask_down_ref(m, h, w)
    md, out = Buf(H, W, init=m, dtype=torch.uint8, fill=1), Buf(h, w)
    O.mask_downsample(md.t, out.t, H, W, h, w)
    landed('mask_downsample_kernel')
    assert np.array_equal(out.get(), ref)
    out.assert_untouched_outside(str(c)); md.assert_unchanged()


# ------------------------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize('rows', SU.COLSUM_ROWS)
def test_colsum(rows):
    O = ops()
    nr = SU.colsum_ranges(rows)
    worst = 0.0
    for cols in SU.COLSUM_COLS:
        for dt in (F32, BF16):
            inp = SU.colsum_make(rows, cols, dt)
            ref, ab, nt = SU.colsum_ref(inp)
            for lda in (cols, cols + 3):
                a = Buf(rows, cols, lda, dt=dt, init=inp['a'])
                for wsk in (None, 'full', 'short'):
                    what = 'colsum %d x %d lda %d %s ws %s' % (rows, cols, lda, STORE[dt], wsk)
                    ws = None if wsk is None else torch.full((nr * cols - (wsk == 'short'),), float('nan'), device=DEV)
                    out = Buf(1, cols, init=inp['out0'])
                    O.colsum(a.t, rows, cols, lda, out.t, ws)
                    landed('colsum_finish_kernel' if nr > 1 and wsk == 'full' else 'colsum_kernel')
                    worst = max(worst, check(out.get()[0], ref, ab, nt, 'f32', what=what))
                    out.assert_untouched_outside(what)
                a.assert_unchanged()
    note('colsum', worst)
    print('colsum rows %d: worst ratio %.3g' % (rows, worst))


# ------------------------------------------------------------------------------------------------------------------ SGD
HYPER = (0.01, 0.9, 1e-2, 0.5)          # lr, momentum, weight decay, gradient scale


def seg_table(segs):
    from lang2seg_amd._lib import SgdSeg
    arr = (SgdSeg * len(segs))()
    for a, s in zip(arr, segs):
        for k, v in s.items():
            setattr(a, k, v)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)


def chunk_range(segs, chunk, lo, hi):
    """the chunks of the table that can hold elements of [lo, hi)"""
    c_lo = c_hi = None
    for s in segs:
        a, b = max(lo, s['offset']), min(hi, s['offset'] + s['count'])
        if a < b:
            first, last = s['chunk0'] + (a - s['offset']) // chunk, s['chunk0'] + (b - 1 - s['offset']) // chunk + 1
            c_lo, c_hi = first if c_lo is None else min(c_lo, first), last if c_hi is None else max(c_hi, last)
    return (0, 0) if c_lo is None else (c_lo, c_hi)


class SgdState(object):
    def __init__(self, inp, sdt, g16=False):
        tot = inp['tot']
        self.p, self.m = Buf(1, tot, init=inp['p'], tail=64), Buf(1, tot, init=inp['m'], tail=64)
        self.g = Buf(1, tot, dt=BF16 if g16 else F32, init=inp['g'], tail=64)
        self.sh = Buf(1, tot, dt=sdt, tail=64)
        self.rs = Buf(1, inp['rowscale'].size, init=inp['rowscale'])

    def same(self, other, grads=True):
        return same_bits(self.p, other.p) and same_bits(self.m, other.m) and same_bits(self.sh, other.sh) and (not grads or same_bits(self.g, other.g))


@pytest.mark.parametrize('sdt', [BF16, F32], ids=['shadow-bf16', 'shadow-f32'])
def test_sgd_momentum(sdt):
    O = ops()
    chunk = O.sgd_chunk()
    inp = SU.sgd_make(chunk)
    segs, tot = inp['segs'], inp['tot']
    tab = seg_table(segs)
    (P, PA), (M, MA), (S, SA) = SU.sgd_ref(inp, *HYPER)
    inside = ~np.isnan(S)
    one = SgdState(inp, sdt)
    O.sgd_momentum(one.p.t, one.g.t, one.m.t, tab, len(segs), one.rs.t, *HYPER, shadow=one.sh.t, clear_grad=True)
    landed('sgd_kernel')
    p, m, sh, g = one.p.get()[0], one.m.get()[0], one.sh.get()[0], one.g.get()[0]
    note('sgd', check(p, P, PA, 3, 'f32', what='param'))
    note('sgd', check(m, M, MA, 3, 'f32', what='momentum'))
    note('sgd', check(sh[inside], S[inside], SA[inside], 3, STORE[sdt], what='shadow'))
    # between the segments nothing is touched; the gradients are cleared except where the segment says its producer overwrites them
    assert np.array_equal(p[~inside], inp['p'][~inside]) and np.array_equal(m[~inside], inp['m'][~inside])
    assert np.array_equal(sh[~inside], one.sh.before[:tot].float().cpu().numpy()[~inside])
    kept = ~inside
    kept[segs[3]['offset']:segs[3]['offset'] + segs[3]['count']] = True
    assert np.array_equal(g[kept], inp['g'][kept]) and not g[~kept].any()
    for b in (one.p, one.m, one.sh, one.g):
        b.assert_untouched_outside('sgd')
    one.rs.assert_unchanged()
    # clear_grad = 0 leaves every gradient; the rest is the same bits
    two = SgdState(inp, sdt)
    O.sgd_momentum(two.p.t, two.g.t, two.m.t, tab, len(segs), two.rs.t, *HYPER, shadow=two.sh.t, clear_grad=False)
    two.g.assert_unchanged()
    assert two.same(one, grads=False)
    # the ranged update in pieces whose ends are no multiples of 4 and cut chunks in the middle, in any order: the single launch bit for bit
    s1, s4 = segs[1], segs[4]
    cuts = [0, 2, s1['offset'] + 1001, s1['offset'] + chunk + 1, segs[2]['offset'] + 6, segs[3]['offset'] + 7, s4['offset'] + 2049, tot]
    pieces = list(zip(cuts[:-1], cuts[1:]))
    for order in (pieces, pieces[::-1]):
        st = SgdState(inp, sdt)
        for lo, hi in order:
            c_lo, c_hi = chunk_range(segs, chunk, lo, hi)
            O.sgd_momentum_range(st.p.t, st.g.t, st.m.t, tab, len(segs), st.rs.t, *HYPER, st.sh.t, 1, lo, hi, c_lo, c_hi)
            landed('sgd_kernel')
        assert st.same(one)
    st = SgdState(inp, sdt)                                                # every chunk offered, the element range alone decides
    for lo, hi in pieces:
        O.sgd_momentum_range(st.p.t, st.g.t, st.m.t, tab, len(segs), st.rs.t, *HYPER, st.sh.t, 1, lo, hi, 0, -1)
    assert st.same(one)
    # flags = 2: the shadow alone is rewritten from the parameters
    st = SgdState(inp, sdt)
    O.sgd_momentum_range(st.p.t, st.g.t, st.m.t, tab, len(segs), st.rs.t, *HYPER, st.sh.t, 2, 0, tot, 0, -1)
    st.p.assert_unchanged(); st.m.assert_unchanged(); st.g.assert_unchanged()
    rs = np.ones(tot)
    for s in segs:
        if s['rowscale_off'] >= 0:
            rs[s['offset']:s['offset'] + s['count']] = inp['rowscale'][s['rowscale_off'] + np.arange(s['count']) // s['row_len']]
    check(st.sh.get()[0][inside], (SU.f64(inp['p']) * rs)[inside], np.abs(SU.f64(inp['p']) * rs)[inside], 1, STORE[sdt], what='shadow only')
    st.sh.assert_untouched_outside('shadow only')


@pytest.mark.parametrize('sdt', [BF16, F32], ids=['shadow-bf16', 'shadow-f32'])
def test_sgd_momentum_range_g16(sdt):
    """the gradients of [lo, hi) read from a bf16 shard that starts at grad_lo: the ranged update on the shard widened to float32, bit for bit"""
    O = ops()
    chunk = O.sgd_chunk()
    inp = SU.sgd_make(chunk, g16=True)
    segs, tot = inp['segs'], inp['tot']
    tab = seg_table(segs)
    s1 = segs[1]
    (P, PA), _, _ = SU.sgd_ref(inp, *HYPER)
    # (grad_lo, lo, hi): the whole buffer; a shard that starts inside segment 1 and ends inside segment 4, its buffer beginning before lo
    for grad_lo, lo, hi in ((0, 0, tot), (s1['offset'] + 2047 - (s1['offset'] + 2047) % 4, s1['offset'] + 2050, segs[4]['offset'] + 1001), (4, 6, s1['offset'] + 3)):
        assert grad_lo % 4 == 0 and grad_lo <= lo
        c_lo, c_hi = chunk_range(segs, chunk, lo, hi)
        ref_st = SgdState(inp, sdt)                                        # inp['g'] holds bf16 values: this is the widened shard
        O.sgd_momentum_range(ref_st.p.t, ref_st.g.t, ref_st.m.t, tab, len(segs), ref_st.rs.t, *HYPER, ref_st.sh.t, 0, lo, hi, c_lo, c_hi)
        st = SgdState(inp, sdt, g16=True)
        shard = Buf(1, hi - grad_lo, dt=BF16, init=inp['g'][grad_lo:hi], tail=64)
        O.sgd_momentum_range_g16(st.p.t, shard.t, grad_lo, st.m.t, tab, len(segs), st.rs.t, *HYPER, st.sh.t, lo, hi, c_lo, c_hi)
        landed('sgd_kernel')
        assert st.same(ref_st, grads=False), (grad_lo, lo, hi)
        shard.assert_unchanged()
        for b in (st.p, st.m, st.sh):
            b.assert_untouched_outside('g16')
        # and only [lo, hi) moved
        p = st.p.get()[0]
        out = np.ones(tot, bool); out[lo:hi] = False
        assert np.array_equal(p[out], inp['p'][out])
        note('sgd_g16', check(p[lo:hi], P[lo:hi], PA[lo:hi], 3, 'f32', what='g16 param'))


# ------------------------------------------------------------------------------------------------------------------ losses and heads
def run_outs(name, got, ref, stores=None, what='', measure=False):
    """every output of a reference through check; measure (ordinary logits only): the plain error of the outputs that ARE libm values
    (probabilities, log-probabilities; float32 stores) in units of 2^-23 of the value, the figure L_LIBM is set from"""
    for k, o in ref.items():
        g = SU.f64(got[k])
        if measure and o['pure']:
            mag = np.broadcast_to(SU.f64(o['mag']), g.shape)
            sel = mag > 1e-30
            if sel.any():
                LIBM[name] = max(LIBM.get(name, 0.0), float((np.abs(g - o['ref'])[sel] / (2.0 ** -23 * mag[sel])).max()))
        note(name, SU.check_out(g, o, (stores or {}).get(k, 'f32'), L_LIBM, '%s %s %s' % (name, what, k)))


def loss_buf():
    return Buf(1, 8, init=LOSS0)


LOSS0 = SU.rnd(np.random.RandomState(77), (8,))
SLOT = dict(rpn_cls=0, rpn_box=1, cls=2, box=3, mask=4, cap=5, total=6, response=7)


def loss_outs(loss, ref, names):
    """the slots a kernel adds to (onto what they held) as outputs; every other slot has to keep its bits"""
    got = loss.get()[0]
    res = {}
    for k, slot in names.items():
        o = ref[k]
        ref[k] = SU.out(o['ref'] + float(LOSS0[SLOT[slot]]), o['ab'] + abs(float(LOSS0[SLOT[slot]])), o['nt'] + 1, mag=o['mag'], floor=o['floor'])
        res[k] = got[SLOT[slot]]
    rest = [i for i in range(8) if i not in [SLOT[v] for v in names.values()]]
    assert np.array_equal(got[rest], LOSS0[rest])
    loss.assert_untouched_outside('loss')
    return res


@pytest.mark.parametrize('c', SU.RPN, ids=lambda c: '%dx%dx%d' % c)
def test_rpn_loss(c):
    O = ops()
    H, W, A = c
    for scale in SU.RPN_SCALES:
        for none in (False, True):
            inp = SU.rpn_make(c, scale, none)
            heads, labels = Buf(H * W, 6 * A, init=inp['heads']), Buf(1, H * W * A, init=inp['labels'].reshape(-1), dtype=torch.int32, fill=1)
            tgt, inw, outw = (Buf(1, H * W * A * 4, init=inp[k]) for k in ('tgt', 'inw', 'outw'))
            for ldd in (6 * A, 6 * A + 8):
                for dt in (F32, BF16):
                    for counted in (False, True):
                        what = '%s x%g none %d ldd %d %s counted %d' % (c, scale, none, ldd, STORE[dt], counted)
                        atl = None if counted else torch.tensor([-5, -5, inp['cnt'], -5], dtype=torch.int32, device=DEV)
                        loss, dh = loss_buf(), Buf(H * W, ldd, dt=dt)
                        O.rpn_loss(heads.t, 6 * A, labels.t, tgt.t, inw.t, outw.t, H, W, A, SU.RPN_SIGMA, SU.RPN_GSCALE, loss.t, dh.t, ldd, atl_ws=atl)
                        landed('rpn_loss_kernel')
                        ref = SU.rpn_ref(inp, c, ldd)
                        got = loss_outs(loss, ref, dict(loss_cls='rpn_cls', loss_box='rpn_box'))
                        got['dheads'] = dh.get()
                        run_outs('rpn_loss', got, ref, stores=dict(dheads=STORE[dt]), what=what, measure=scale == 1.0)
                        dh.assert_untouched_outside(what)
                        if none:
                            assert not got['dheads'].any() and got['loss_cls'] == LOSS0[0] and got['loss_box'] == LOSS0[1]
            for b in (heads, labels, tgt, inw, outw):
                b.assert_unchanged()


@pytest.mark.parametrize('c', SU.RCNN, ids=lambda c: 'R%d-ncls%d' % c)
def test_rcnn_loss(c):
    O = ops()
    R, ncls = c
    for scale in (1.0, 100.0):
        inp = SU.rcnn_make(c, scale)
        for ldh in (5 * ncls, 5 * ncls + 3):
            heads, labels = Buf(R, 5 * ncls, ldh, init=inp['heads']), Buf(1, R, init=inp['labels'], dtype=torch.int32, fill=1)
            bt, bi, bo = (Buf(R, 4 * ncls, init=inp[k]) for k in ('bt', 'bi', 'bo'))
            for ldd in (5 * ncls, 5 * ncls + 8):
                for dt in (F32, BF16):
                    what = '%s x%g ldh %d ldd %d %s' % (c, scale, ldh, ldd, STORE[dt])
                    loss, dh = loss_buf(), Buf(R, ldd, dt=dt)
                    O.rcnn_loss(heads.t, ldh, labels.t, bt.t, bi.t, bo.t, R, ncls, SU.RCNN_GSCALE, loss.t, dh.t, ldd)
                    landed('rcnn_loss_kernel')
                    ref = SU.rcnn_ref(inp, c, ldd)
                    got = loss_outs(loss, ref, dict(loss_cls='cls', loss_box='box'))
                    got['dheads'] = dh.get()
                    run_outs('rcnn_loss', got, ref, stores=dict(dheads=STORE[dt]), what=what, measure=scale == 1.0)
                    dh.assert_untouched_outside(what)
            heads.assert_unchanged()


@pytest.mark.parametrize('c', SU.MASK_LOSS, ids=lambda c: 'ms%d-ld%d-x%g' % c)
def test_mask_loss(c):
    O = ops()
    ms2, ldsc, scale = c
    inp = SU.mask_loss_make(c)
    n = SU.FG_MAX * ms2
    score, mt = Buf(n, SU.MASK_NCLS, ldsc, init=inp['score']), Buf(1, n, init=inp['mt'])
    labels = Buf(1, SU.FG_MAX, init=SU.MASK_LABELS, dtype=torch.int32, fill=1)
    for num_fg in SU.MASK_NUM_FG:
        what = '%s num_fg %d' % (c, num_fg)
        nf = torch.tensor([num_fg], dtype=torch.int32, device=DEV)
        loss, ds = loss_buf(), Buf(1, n)
        O.mask_loss(score.t, ldsc, labels.t, mt.t, nf, SU.FG_MAX, ms2, SU.MASK_GSCALE, loss.t, ds.t)
        landed('mask_loss_kernel')
        ref = SU.mask_loss_ref(inp, ms2, num_fg)
        got = loss_outs(loss, ref, dict(loss='mask'))
        got['dscore'] = ds.get()[0]
        run_outs('mask_loss', got, ref, what=what, measure=scale == 1.0)
        ds.assert_untouched_outside(what)
        if num_fg == 0:
            assert not got['dscore'].any() and got['loss'] == LOSS0[4]
    score.assert_unchanged()


@pytest.mark.parametrize('c', SU.MASKPRED, ids=lambda c: 'C%d-ms%d-%s' % (c[0], c[1], STORE[c[2]]))
def test_maskpred_bwd(c):
    """the one-call form against float64, and the dx + reduce pair against the one call bit for bit; labels repeat, differ and one (97) lies
    beyond the reduce kernel's LDS table; C = 256: the bias column is alone in the second workgroup"""
    O = ops()
    Cc, ms2, dt = c
    inp = SU.maskpred_make(c)
    n = SU.FG_MAX * ms2
    from lang2seg_amd import _lib
    need = int(_lib.load().l2s_maskpred_ws_floats(SU.FG_MAX, Cc))
    ds, w = Buf(1, n, init=inp['dscore']), Buf(SU.MASK_NCLS, Cc, init=inp['w'])
    x, rf = Buf(n, Cc, dt=dt, init=inp['x']), Buf(n, Cc, dt=dt, init=inp['ref'])
    labels = Buf(1, SU.FG_MAX, init=SU.MASK_LABELS, dtype=torch.int32, fill=1)
    for num_fg in SU.MASK_NUM_FG:
        nf = torch.tensor([num_fg], dtype=torch.int32, device=DEV)
        for has_ref in (True, False):
            what = '%s num_fg %d ref %d' % (c, num_fg, has_ref)
            runs = []
            for split in (False, True):
                dx, dw, db = Buf(n, Cc, dt=dt), Buf(SU.MASK_NCLS, Cc, init=inp['dw0']), Buf(1, SU.MASK_NCLS, init=inp['db0'])
                ws = torch.full((need,), float('nan'), device=DEV)
                if split:
                    O.maskpred_bwd_dx(ds.t, labels.t, nf, SU.FG_MAX, ms2, Cc, w.t, x.t, rf.t if has_ref else None, dx.t, ws)
                    landed('maskpred_bwd_kernel')
                    O.maskpred_bwd_reduce(ws, labels.t, nf, SU.FG_MAX, Cc, dw.t, db.t)
                else:
                    O.maskpred_bwd(ds.t, labels.t, nf, SU.FG_MAX, ms2, Cc, w.t, x.t, rf.t if has_ref else None, dx.t, dw.t, db.t, ws)
                landed('maskpred_bwd_reduce_kernel')
                runs.append((dx, dw, db))
            dx, dw, db = runs[0]
            run_outs('maskpred_bwd', dict(dx=dx.get(), dw=dw.get(), db=db.get()[0]), SU.maskpred_ref(inp, ms2, num_fg, has_ref), stores=dict(dx=STORE[dt]), what=what)
            for a, b in zip(*runs):
                a.assert_untouched_outside(what)
                assert same_bits(a, b), what + ': the two-call form differs from the one call'
    for b in (ds, w, x, rf, labels):
        b.assert_unchanged()


@pytest.mark.parametrize('c', SU.RESPONSE, ids=lambda c: '%dx%d-%dx%d' % c)
def test_response_loss(c):
    from oracle import boxes as OB
    O = ops()
    MH, MW, H, W = c
    for scale in (1.0, 100.0):
        inp = SU.response_make(c, scale)
        target = OB.imresize_nearest_u8(inp['mask'], (H, W))
        resp, mask = Buf(1, H * W, init=inp['resp']), Buf(MH, MW, init=inp['mask'], dtype=torch.uint8, fill=1)
        loss, dr = loss_buf(), Buf(1, H * W)
        O.response_loss(resp.t, mask.t, MH, MW, H, W, SU.RESP_GSCALE, loss.t, dr.t)
        landed('response_loss_kernel')
        ref = SU.response_ref(inp, c, target)
        got = loss_outs(loss, ref, dict(loss='response'))
        got['dresp'] = dr.get()[0]
        run_outs('response_loss', got, ref, what='%s x%g' % (c, scale), measure=scale == 1.0)
        dr.assert_untouched_outside(str(c)); resp.assert_unchanged(); mask.assert_unchanged()


@pytest.mark.parametrize('cap_w', [0.0, 0.5])
def test_total_loss(cap_w):
    O = ops()
    loss = loss_buf()
    O.total_loss(loss.t, cap_w)
    landed('total_loss_kernel')
    got = loss.get()[0]
    SU.check_out(got[6], SU.total_loss_ref(LOSS0, cap_w), 'f32', 0.0, 'total_loss')
    assert np.array_equal(np.delete(got, 6), np.delete(LOSS0, 6))
    loss.assert_untouched_outside('total_loss')


@pytest.mark.parametrize('c', SU.LSM, ids=lambda c: 'S%d-V%d-x%g' % c)
def test_logsoftmax_nll(c):
    O = ops()
    S, V1, scale = c
    inp = SU.lsm_make(c)
    logits, mask = Buf(S, V1, init=inp['logits']), Buf(1, S, init=inp['mask'])
    target = Buf(1, S, init=inp['target'], dtype=torch.int64, fill=0)
    for has_d, has_lp in ((True, True), (True, False), (False, True), (False, False)):
        what = '%s dlogits %d logprobs %d' % (c, has_d, has_lp)
        loss, d, lp = loss_buf(), Buf(S, V1), Buf(S, V1)
        O.logsoftmax_nll(logits.t, target.t, mask.t, S, V1, SU.LSM_GSCALE, loss.t[5:6], d.t if has_d else None, lp.t if has_lp else None)
        landed('lsm_nll_kernel')
        ref = SU.lsm_ref(inp)
        got = loss_outs(loss, ref, dict(loss='cap'))
        got.update(dlogits=d.get(), logprobs=lp.get())
        for k, given, b in (('dlogits', has_d, d), ('logprobs', has_lp, lp)):
            if given:
                b.assert_untouched_outside(what)
            else:
                b.assert_unchanged(what); del ref[k]
        run_outs('logsoftmax_nll', got, ref, what=what, measure=scale == 1.0)
        if has_d:
            assert not got['dlogits'][inp['mask'] == 0].any()              # a masked row has no gradient at all
    logits.assert_unchanged()


def test_rcnn_predict_and_mask_prob():
    O = ops()
    for c in SU.RCNN_PRED:
        R, ncls, ldh, scale = c
        inp = SU.rcnn_pred_make(c)
        heads, st, mn = Buf(R, 5 * ncls, ldh, init=inp['heads']), Buf(1, 4, init=inp['stds']), Buf(1, 4, init=inp['means'])
        cp, bp = Buf(R, ncls), Buf(R, 4 * ncls)
        O.rcnn_predict(heads.t, ldh, R, ncls, st.t, mn.t, cp.t, bp.t)
        landed('rcnn_predict_kernel')
        run_outs('rcnn_predict', dict(cls_prob=cp.get(), bbox_pred=bp.get()), SU.rcnn_pred_ref(inp, ncls), what=str(c), measure=scale == 1.0)
        cp.assert_untouched_outside(str(c)); bp.assert_untouched_outside(str(c)); heads.assert_unchanged()
    for c in SU.MASK_PROB:
        R, ms2, ncls, ldsc, per_label, scale = c
        inp = SU.mask_prob_make(c)
        score, labels = Buf(R * ms2, ncls, ldsc, init=inp['score']), Buf(1, R, init=inp['labels'], dtype=torch.int32, fill=1)
        o = Buf(1, R * ms2) if per_label else Buf(R * ms2, ncls)
        O.mask_prob(score.t, ldsc, ncls, labels.t if per_label else None, ms2, R * ms2, o.t)
        landed('mask_prob_kernel')
        got = o.get()[0] if per_label else o.get()
        run_outs('mask_prob', dict(p=got), dict(p=SU.mask_prob_ref(inp, c)), what=str(c), measure=scale == 1.0)
        o.assert_untouched_outside(str(c)); score.assert_unchanged()


@pytest.mark.parametrize('c', SU.EMBED, ids=lambda c: 'D%d-T%d-%s-m%d-r%d' % c)
def test_embed(c):
    O = ops()
    D, T, ids, has_mask, relu = c
    inp = SU.embed_make(c)
    ref = SU.embed_ref(inp, c)
    table, mask = Buf(SU.EMBED_VOCAB, D, init=inp['table']), Buf(T, D, init=inp['mask'])
    idb = Buf(1, T, init=inp['ids'], dtype=torch.int64, fill=0)
    o = Buf(T, D)
    O.embed_fwd(table.t, idb.t, mask.t if has_mask else None, o.t, T, D, relu)
    landed('embed_fwd_kernel')
    assert np.array_equal(o.get(), inp['out'])                             # a copy, a ReLU and one product: the same bits as numpy's float32
    o.assert_untouched_outside(str(c))
    dout, dtab = Buf(T, D, init=inp['dout']), Buf(SU.EMBED_VOCAB, D, init=inp['dtable0'])
    O.embed_bwd(dout.t, o.t, idb.t, mask.t if has_mask else None, dtab.t, T, D, relu)
    landed('embed_bwd_kernel')
    run_outs('embed', dict(out=o.get(), dtable=dtab.get()), ref, what=str(c))
    dtab.assert_untouched_outside(str(c))
    rows = np.ones(SU.EMBED_VOCAB, bool); rows[inp['ids']] = False
    assert np.array_equal(dtab.get()[rows], inp['dtable0'][rows])          # rows of tokens that do not occur are not touched
    for b in (table, mask, idb, dout):
        b.assert_unchanged()


@pytest.mark.parametrize('c', SU.DYNFILTER, ids=lambda c: '%dx%d-C%d-%s' % (c[0][0], c[0][1], c[1], STORE[c[2]]))
def test_dynfilter(c):
    """forward, backward in one call, and the backward as its data-gradient passes + l2s_dynfilter_bwd_finish (bit for bit the one call)"""
    from oracle import net as ON
    O = ops()
    (H, W), Cc, dt, kf, kb = c
    inp = SU.dynfilter_make(c, ON.spatial_masks(H, W))
    HW = H * W
    x, filt, r = Buf(HW, Cc, dt=dt, init=inp['x']), Buf(7, Cc, init=inp['filt']), Buf(1, 7, init=inp['r'])
    dy, rf, extra = Buf(HW, Cc, dt=dt, init=inp['dy']), Buf(HW, Cc, dt=dt, init=inp['ref']), Buf(1, HW, init=inp['extra'])
    resp_in, respk_in = Buf(1, HW, init=inp['resp']), Buf(HW, 7, init=inp['respk'])
    need = O.dynfilter_ws_floats(H, W, Cc)
    for gate in (0, 1):
        what = '%s gate %d' % (c[:3], gate)
        y, resp, respk = Buf(HW, Cc, dt=dt), Buf(1, HW), Buf(HW, 7)
        O.dynfilter_fwd(x.t, filt.t, r.t, y.t, resp.t, respk.t, H, W, Cc, gate=gate)
        landed(kf)
        run_outs('dynfilter_fwd', dict(y=y.get(), resp=resp.get()[0], respk=respk.get()), SU.dynfilter_fwd_ref(inp, gate), stores=dict(y=STORE[dt]), what=what)
        for b in (y, resp, respk):
            b.assert_untouched_outside(what)
        for has_extra in (True, False):
            for has_ref in (True, False):
                what = '%s gate %d extra %d ref %d' % (c[:3], gate, has_extra, has_ref)
                runs = []
                for split in (False, True):
                    dx, dfilt, dr = Buf(HW, Cc, dt=dt), Buf(7, Cc, init=inp['dfilt0']), Buf(1, 7, init=inp['dr0'])
                    ws = torch.full((need,), float('nan'), device=DEV)
                    O.dynfilter_bwd(dy.t, x.t, filt.t, r.t, resp_in.t, respk_in.t, dx.t, rf.t if has_ref else None, None if split else dfilt.t, None if split else dr.t,
                                    ws, H, W, Cc, gate=gate, dresp_extra=extra.t if has_extra else None)
                    if split:
                        landed(kb)
                        O.dynfilter_bwd_finish(ws, respk_in.t, dfilt.t, dr.t, H, W, Cc)
                    landed('dynfilter_bwd3_kernel')
                    runs.append((dx, dfilt, dr))
                dx, dfilt, dr = runs[0]
                run_outs('dynfilter_bwd', dict(dx=dx.get(), dfilt=dfilt.get(), dr=dr.get()[0]), SU.dynfilter_bwd_ref(inp, gate, has_extra, has_ref),
                         stores=dict(dx=STORE[dt]), what=what)
                for a, b in zip(*runs):
                    a.assert_untouched_outside(what)
                    assert same_bits(a, b), what + ': the split form differs from the one call'
    for b in (x, filt, r, dy, rf, extra, resp_in, respk_in):
        b.assert_unchanged()


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_every_listed_kernel_ran():
    print('worst check ratios:', ', '.join('%s %.3g' % kv for kv in sorted(WORST.items())))
    print('libm, worst |got - ref| / (2^-23 |value|):', ', '.join('%s %.3g' % kv for kv in sorted(LIBM.items())), '(L_LIBM = %g)' % L_LIBM)
    assert 4 * max(LIBM.values()) <= L_LIBM
    assert KERNELS == TABLE_KERNELS, sorted(set(KERNELS) ^ set(TABLE_KERNELS))
    assert sorted(SEEN) == KERNELS, (sorted(set(KERNELS) - SEEN), sorted(SEEN - set(KERNELS)))
