"""The per-token recurrence and attention kernels (csrc/caption_step.hip, csrc/rnn_step.hip, csrc/adaatt_step.hip) and the resident recurrence (csrc/cap_recur.hip), each on its own inputs, against the float64
references of tests/recur_kernels_util.py through the one elementwise bound `check` (tests/small_kernels_util.py; pinned without a GPU by
tests/test_recur_kernels_cpu.py).  One launch, no recurrence: nothing propagates, so the bound is the kernel's own.  Each case names the
kernel the dispatcher has to land on and asserts ops.last_kernel() says so; the last test asserts that the kernels seen are exactly
KERNELS (it needs the whole file to have run in this process).

Inputs and outputs sit in sentinel-padded buffers (tests/gpu_buf.py): inputs have to come back unchanged, outputs untouched outside
what the call may write; gate-major arrays ([gate][unit]) have no spare columns - their stride IS the unit count - and carry a spare row.
Every call runs twice on the same inputs and the two results have to be the same bits (no atomics, a fixed order).  The two-launch
entries are checked in stages: the second stage's reference starts from what the first launch stored (the dots in att_res + D, the
dweight in datt_h + D, the da2c of cap_gates_bwd_dw), so no output inherits the error of an earlier launch.  Selectors, exact zeros of
the d0 / d1 routing, the packer and the concat copies are bit for bit.

The libm allowance L_LIBM (sigm = 1 / (1 + expf(-x)), tanhf, the softmax's expf): measured on the outputs that ARE libm values (saved
gates, tanh_ws, attention weights) at ordinary N(0, 1) arguments that are inputs or one rounding away from one (the gates of the encoder
steps sit behind a GEMV and are not measured), |got - ref| / (2^-23 |value|) against the float64 reference; L_LIBM starts from the small
kernels' 8 and has to be at least four times the largest measured value: the last test but one asserts that on every run.

Worst values measured on an MI355X (this file's own prints):
  libm, |got - ref| / (2^-23 |value|)
    tanhf and the composite sigmoid   tanh_ws 1.42 (adaatt_att_fwd; cap_att_dots_fwd and cap_attention_fwd 1.41), saved gates 0.972 (cap_gates_fwd;
                                      cap_apply_gates_fwd 0.959, lstm_cell_fwd 0.952, cap_a2c_gates_fwd 0.946)     -> 4 x 1.42 = 5.7 -> L_LIBM = 8
    softmax weights                   cap_apply_gates_fwd 2.6, cap_att_apply_fwd 2.54, cap_attention_fwd 2.08      -> 4 x 2.6 = 10.4 -> 16 = L_LIBM * SOFTMAX_L
      (one expf, its argument x - max rounded at |x - max| up to ~5, L additions, one divide: the composite needs more than 8, so the outputs
      that carry a softmax weight take 16 by the same rule - recur_kernels_util.SOFTMAX_L = 2 multiplies expf's share of `mag` alone)
  worst check ratio per entry point   adaatt_att_bwd_batched 0.29, adaatt_att_bwd_step 0.326, adaatt_att_fwd 0.133, adaatt_cell_bwd 0.208, adaatt_cell_fwd 0.0501,
                                      cap_a2c_gates_fwd 0.118, cap_apply_gates_fwd 0.037, cap_att_apply_fwd 0.00925, cap_att_bwd_step_centered 0.109,
                                      cap_att_dots_fwd 0.132, cap_attention_bwd 0.25, cap_attention_bwd_batched 0.287, cap_attention_bwd_step 0.0682,
                                      cap_attention_bwd_step2 0.109, cap_attention_fwd 0.132, cap_gates_bwd 0.348, cap_gates_bwd_dw 0.349, cap_gates_fwd 0.143,
                                      gru_step_bwd 0.286, gru_step_fwd 0.0718, linear2_fwd 0.173, linear_sum2_fwd 0.0416, lstm_cell_bwd 0.323, lstm_cell_fwd 0.108,
                                      lstm_step_bwd 0.28, lstm_step_fwd 0.159, rnn_concat_bwd 0.333, rnn_concat_fwd 0 (exact), rnn_step_bwd 0.2, rnn_step_fwd 0.044,
                                      topdown_cell_bwd 0.109, topdown_cell_fwd 0.0776
                                      cap_recur_fwd 0.127 (token 0, h = 0: one rounding per value; 0.0042 and below at the later tokens, where the bound is
                                      the worst case of two 512-term GEMVs), cap_recur_bwd 0.231; 0 to 9 of 512 selectors undecided per token
  selectors, routed zeros, pack_rows, the concat copies, dhol, two runs of every call: exact

  (the softmax figure is NOT expf's own error: x - max is rounded once, and 2^-24 |x - max| at |x - max| ~ 5 is already 2.5 units of 2^-23 of the
  weight.  expf's rule pays for that rounding in `ab` too; the measurement rule takes the plain ratio, so the 16 counts it twice - loose, still elementwise)

Kernels that can never be the LAST launch of an entry are run by their cases but cannot be named in KERNELS: cap_att_dots_kernel in
front of cap_att_apply_kernel in l2s_cap_attention_fwd is also l2s_cap_att_dots_fwd's (named there); cap_att_bwd_dw_kernel in front of
cap_att_bwd_kernel in l2s_cap_attention_bwd and adaatt_scores_kernel in front of adaatt_apply_kernel in l2s_adaatt_att_fwd are not."""
import numpy as np
import pytest
import torch

import recur_kernels_util as RU
from small_kernels_util import check_out, f64
from gpu_buf import Buf, same_bits

pytestmark = pytest.mark.gpu

L_LIBM = 8.0            # in units of 2^-23 of the value libm produced: four times the worst measured value (docstring), rounded up to a power of two
LIBM = {}               # entry -> worst measured |got - ref| / (2^-23 |value|) at ordinary arguments
SEEN = set()
WORST = {}

KERNELS = [
    'cap_a2c_gates_kernel', 'cap_apply_gates_kernel', 'cap_att_apply_kernel', 'cap_att_bwd_batched_kernel', 'cap_att_bwd_kernel', 'cap_att_bwd_step2_kernel',
    'cap_att_bwd_step_kernel', 'cap_att_dots_kernel', 'cap_gates_bwd_dw_kernel', 'cap_gates_bwd_kernel', 'cap_gates_fwd_kernel', 'gru_step_bwd_kernel',
    'gru_step_fwd_kernel', 'linear2_fwd_kernel', 'linear_sum2_kernel', 'linear_sum2_split_kernel', 'lstm_cell_bwd_kernel', 'lstm_cell_fwd_kernel',
    'lstm_step_bwd_kernel', 'lstm_step_fwd_kernel', 'rnn_concat_bwd_kernel', 'rnn_concat_fwd_kernel', 'rnn_step_bwd_kernel', 'rnn_step_fwd_kernel',
    'topdown_att_bwd_step_kernel', 'topdown_cell_bwd_kernel<false>', 'topdown_cell_bwd_kernel<true>', 'topdown_cell_fwd_kernel<false>',
    'topdown_cell_fwd_kernel<true>', 'topdown_pack_rows_kernel',
    'adaatt_apply_kernel', 'adaatt_att_bwd_batched_kernel', 'adaatt_att_bwd_step_kernel', 'adaatt_cell_bwd_kernel<4,false>', 'adaatt_cell_bwd_kernel<4,true>',
    'adaatt_cell_bwd_kernel<5,false>', 'adaatt_cell_bwd_kernel<5,true>', 'adaatt_cell_fwd_kernel<4,false>', 'adaatt_cell_fwd_kernel<4,true>',
    'adaatt_cell_fwd_kernel<5,false>', 'adaatt_cell_fwd_kernel<5,true>', 'cap_recur_bwd_kernel', 'cap_recur_fwd_kernel',
]


def ops():
    from lang2seg_amd import ops as O
    return O


def landed(kernel):
    k = ops().last_kernel()
    SEEN.add(k)
    assert k == kernel, 'the dispatcher launched %s last, this case is meant for %s' % (k, kernel)


def vec(a, **kw):
    """a vector (or a gate-major [g][n] array) as an input buffer"""
    a = np.asarray(a, np.float32)
    a = a.reshape(1, -1) if a.ndim == 1 else a
    return Buf(a.shape[0], a.shape[1], init=a, **kw)


def twice(fresh, launch, kernel):
    """two runs on the same inputs into fresh outputs: the same bits; -> the first run's outputs"""
    o1 = fresh()
    launch(o1)
    landed(kernel)
    o2 = fresh()
    launch(o2)
    for k in o1:
        assert same_bits(o1[k], o2[k]), '%s: two runs on the same inputs differ in %s' % (kernel, k)
    return o1


def verify(name, what, outs, ref, libm_on=()):
    """every output through `check` and untouched outside its region; libm_on: (key, index or None, keep-mask or None) of the outputs that are
    libm values, for the allowance"""
    w = 0.0
    got = {}
    for k in sorted(ref):
        g = outs[k].get().reshape(np.shape(ref[k]['ref']))
        got[k] = g
        w = max(w, check_out(g, ref[k], 'f32', L_LIBM, '%s %s %s' % (name, what, k)))
        outs[k].assert_untouched_outside('%s %s %s' % (name, what, k))
    for k, idx, keep in libm_on:
        g, r = f64(got[k] if idx is None else got[k][idx]), f64(ref[k]['ref'] if idx is None else ref[k]['ref'][idx])
        m = (r != 0) if keep is None else keep & (r != 0)
        if m.any():
            key = (name, 'softmax' if k == 'weight' else 'gate')
            LIBM[key] = max(LIBM.get(key, 0.0), float((np.abs(g - r)[m] / (2.0 ** -23 * np.abs(r[m]))).max()))
    WORST[name] = max(WORST.get(name, 0.0), w)
    print('%s %s: worst ratio %.3g' % (name, what, w))
    return got


def unchanged(*bufs):
    for b in bufs:
        if b is not None:
            b.assert_unchanged()


def ordinary(s):
    """gate sums that are ordinary N(0, 1) arguments (the +-12 ones are saturated on purpose)"""
    return np.abs(f64(s)) < 6.0


def planted_exact(inp, save):
    """the selectors of the planted ties and steps, bit for bit"""
    assert (save[3][inp['ties']] == 0).all() and (save[3][inp['ups']] == 1).all() and (save[3][inp['downs']] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ attention forward
@pytest.mark.parametrize('c', RU.ATT_LD, ids=RU.ld_id)
def test_cap_att_dots_fwd(c):
    O = ops()
    L, D = c
    inp = RU.att_fwd_make(c)
    patt, att_h, aw, ab = Buf(L, D, init=inp['patt']), vec(inp['att_h']), vec(inp['aw']), vec(inp['ab'])
    outs = twice(lambda: dict(tanh_ws=Buf(L, D), dots=Buf(1, L, ld=256)),
                 lambda o: O.cap_att_dots_fwd(patt.t, att_h.t, aw.t, ab.t, L, D, o['tanh_ws'].t, o['dots'].t), 'cap_att_dots_kernel')
    verify('cap_att_dots_fwd', RU.ld_id(c), outs, RU.att_dots_ref(inp), libm_on=[('tanh_ws', None, None)])
    unchanged(patt, att_h, aw, ab)


@pytest.mark.parametrize('c', RU.ATT_LD, ids=RU.ld_id)
def test_cap_att_apply_fwd(c):
    O = ops()
    L, D = c
    inp = RU.att_fwd_make(c)
    att, dots = Buf(L, D, init=inp['att']), Buf(1, L, ld=256, init=inp['dots'])
    outs = twice(lambda: dict(weight=Buf(1, L), att_res=Buf(1, D)),
                 lambda o: O.cap_att_apply_fwd(att.t, dots.t, L, D, o['weight'].t, o['att_res'].t), 'cap_att_apply_kernel')
    verify('cap_att_apply_fwd', RU.ld_id(c), outs, RU.att_apply_ref(inp), libm_on=[('weight', None, None)])
    unchanged(att, dots)


@pytest.mark.parametrize('c', RU.ATT_LD, ids=RU.ld_id)
def test_cap_attention_fwd(c):
    """two launches: the dots land in att_res + D (scratch: only [0, D) of att_res is a result); the second stage starts from them"""
    O = ops()
    L, D = c
    inp = RU.att_fwd_make(c)
    patt, att, att_h, aw, ab = Buf(L, D, init=inp['patt']), Buf(L, D, init=inp['att']), vec(inp['att_h']), vec(inp['aw']), vec(inp['ab'])
    outs = twice(lambda: dict(tanh_ws=Buf(L, D), weight=Buf(1, L), res=Buf(1, D + L)),
                 lambda o: O.cap_attention_fwd(patt.t, att.t, att_h.t, aw.t, ab.t, L, D, o['tanh_ws'].t, o['weight'].t, o['res'].t), 'cap_att_apply_kernel')
    res = outs['res'].get().reshape(-1)
    outs['res'].assert_untouched_outside()
    first = dict(tanh_ws=outs['tanh_ws'], dots=Buf(1, L, init=res[D:]))
    verify('cap_attention_fwd', RU.ld_id(c) + ' dots', first, RU.att_dots_ref(inp), libm_on=[('tanh_ws', None, None)])
    second = dict(weight=outs['weight'], att_res=Buf(1, D, init=res[:D]))
    verify('cap_attention_fwd', RU.ld_id(c) + ' apply', second, RU.att_apply_ref(dict(inp, dots=res[D:].copy())), libm_on=[('weight', None, None)])
    unchanged(patt, att, att_h, aw, ab)


@pytest.mark.parametrize('c', RU.ATT_LD, ids=RU.ld_id)
def test_cap_apply_gates_fwd(c):
    O = ops()
    L, R = c
    inp = RU.apply_gates_make(c)
    P, dots, b, s, cp = Buf(L, 2 * R, init=inp['P']), Buf(1, L, ld=256, init=inp['dots']), vec(inp['b']), vec(inp['s']), vec(inp['c_prev'])
    outs = twice(lambda: dict(c=Buf(1, R), h=Buf(1, R), save=Buf(6, R), weight=Buf(1, L)),
                 lambda o: O.cap_apply_gates_fwd(P.t, dots.t, b.t, s.t, cp.t, o['c'].t, o['h'].t, o['save'].t, o['weight'].t, L, R), 'cap_apply_gates_kernel')
    got = verify('cap_apply_gates_fwd', RU.ld_id(c), outs, RU.apply_gates_ref(inp),
                 libm_on=[('weight', None, None)] + [('save', q, ordinary(inp['s'][q])) for q in range(3)])
    planted_exact(inp, got['save'])
    unchanged(P, dots, b, s, cp)


# ------------------------------------------------------------------------------------------------------------------ gate blocks
@pytest.mark.parametrize('R', RU.GATES_R)
def test_cap_gates_fwd(R):
    O = ops()
    inp = RU.gates_fwd_make(R)
    s, a, cp = vec(inp['s']), vec(inp['a2c']), vec(inp['c_prev'])
    outs = twice(lambda: dict(c=Buf(1, R), h=Buf(1, R), save=Buf(6, R)),
                 lambda o: O.cap_gates_fwd(s.t, a.t, cp.t, o['c'].t, o['h'].t, o['save'].t, R), 'cap_gates_fwd_kernel')
    got = verify('cap_gates_fwd', 'R%d' % R, outs, RU.gates_fwd_ref(inp), libm_on=[('save', q, ordinary(inp['s'][q])) for q in range(3)])
    planted_exact(inp, got['save'])
    unchanged(s, a, cp)


@pytest.mark.parametrize('c', RU.A2C_GATES, ids=str)
def test_cap_a2c_gates_fwd(c):
    O = ops()
    R, K = c
    inp = RU.a2c_gates_make(c)
    x, w, b, s, cp = vec(inp['x']), Buf(2 * R, K, init=inp['w']), vec(inp['b']), vec(inp['s']), vec(inp['c_prev'])
    outs = twice(lambda: dict(c=Buf(1, R), h=Buf(1, R), save=Buf(6, R)),
                 lambda o: O.cap_a2c_gates_fwd(x.t, w.t, b.t, K, s.t, cp.t, o['c'].t, o['h'].t, o['save'].t, R), 'cap_a2c_gates_kernel')
    got = verify('cap_a2c_gates_fwd', str(c), outs, RU.a2c_gates_ref(inp), libm_on=[('save', q, ordinary(inp['s'][q])) for q in range(3)])
    planted_exact(inp, got['save'])
    unchanged(x, w, b, s, cp)


def routed(inp, got):
    """d0 / d1: the selector sends dit to one, the other is an exact 0; dsums carries the same two rows"""
    first = inp['save'][3] == 0
    assert (got['da2c'][1][first] == 0).all() and (got['da2c'][0][~first] == 0).all()
    assert np.array_equal(got['dsums'][3:5].view(np.int32), got['da2c'].view(np.int32))


@pytest.mark.parametrize('c', RU.GATES_BWD, ids=str)
def test_cap_gates_bwd(c):
    O = ops()
    R, has_dh2, has_dc = c
    inp = RU.gates_bwd_make(c)
    dh, dh2, dc, sv, cp = vec(inp['dh']), vec(inp['dh2']), vec(inp['dc_in']), vec(inp['save']), vec(inp['c_prev'])
    outs = twice(lambda: dict(dsums=Buf(5, R), da2c=Buf(2, R), dc_prev=Buf(1, R)),
                 lambda o: O.cap_gates_bwd(dh.t, dc.t if has_dc else None, sv.t, cp.t, o['dsums'].t, o['da2c'].t, o['dc_prev'].t, R, dh2=dh2.t if has_dh2 else None),
                 'cap_gates_bwd_kernel')
    routed(inp, verify('cap_gates_bwd', str(c), outs, RU.gates_bwd_ref(inp, has_dh2, has_dc)))
    unchanged(dh, dh2, dc, sv, cp)


@pytest.mark.parametrize('c', RU.GATES_BWD_DW, ids=str)
def test_cap_gates_bwd_dw(c):
    """R = 1024 fills the kernel's 2R-float LDS array; dweight is checked from the da2c the same launch stored"""
    O = ops()
    R, L, has_dh2, has_dc = c
    inp = RU.gates_bwd_make(c)
    dh, dh2, dc, sv, cp, P = vec(inp['dh']), vec(inp['dh2']), vec(inp['dc_in']), vec(inp['save']), vec(inp['c_prev']), Buf(L, 2 * R, init=inp['P'])
    outs = twice(lambda: dict(dsums=Buf(5, R), da2c=Buf(2, R), dc_prev=Buf(1, R), dweight=Buf(1, L)),
                 lambda o: O.cap_gates_bwd_dw(dh.t, dc.t if has_dc else None, sv.t, cp.t, P.t, o['dsums'].t, o['da2c'].t, o['dc_prev'].t, o['dweight'].t, L, R,
                                              dh2=dh2.t if has_dh2 else None), 'cap_gates_bwd_dw_kernel')
    dwt = outs.pop('dweight')
    got = verify('cap_gates_bwd_dw', str(c), outs, RU.gates_bwd_ref(inp, has_dh2, has_dc))
    routed(inp, got)
    verify('cap_gates_bwd_dw', str(c) + ' dweight', dict(dweight=dwt), RU.dweight_ref(dict(inp, da2c=got['da2c'].reshape(-1))))
    unchanged(dh, dh2, dc, sv, cp, P)


# ------------------------------------------------------------------------------------------------------------------ attention backward
def att_bwd_inputs(inp, L, D):
    return dict(dweight=vec(inp['dweight']), tanh_ws=Buf(L, D, init=inp['tanh_ws']), weight=vec(inp['weight']), aw=vec(inp['aw']), dres=vec(inp['dres']),
                att=Buf(L, D, init=inp['att']))


@pytest.mark.parametrize('c', RU.ATT_LD, ids=RU.ld_id)
def test_cap_attention_bwd_step2(c):
    O = ops()
    L, D = c
    inp = RU.att_bwd_make(c)
    b = att_bwd_inputs(inp, L, D)
    outs = twice(lambda: dict(ddot=Buf(1, L), datt_h=Buf(1, D)),
                 lambda o: O.cap_attention_bwd_step2(b['dweight'].t, b['tanh_ws'].t, b['weight'].t, b['aw'].t, L, D, o['ddot'].t, o['datt_h'].t),
                 'cap_att_bwd_step2_kernel')
    verify('cap_attention_bwd_step2', RU.ld_id(c), outs, RU.att_bwd_step2_ref(inp))
    unchanged(*b.values())


@pytest.mark.parametrize('c', RU.ATT_LD, ids=RU.ld_id)
def test_cap_attention_bwd_step(c):
    O = ops()
    L, D = c
    inp = RU.att_bwd_make(c)
    b = att_bwd_inputs(inp, L, D)
    outs = twice(lambda: dict(ddot=Buf(1, L), datt_h=Buf(1, D)),
                 lambda o: O.cap_attention_bwd_step(b['dres'].t, b['att'].t, b['tanh_ws'].t, b['weight'].t, b['aw'].t, L, D, o['ddot'].t, o['datt_h'].t),
                 'cap_att_bwd_step_kernel')
    verify('cap_attention_bwd_step', RU.ld_id(c), outs, RU.att_bwd_step_ref(inp))
    unchanged(*b.values())


@pytest.mark.parametrize('c', RU.ATT_BWD_CENTERED, ids=str)
def test_cap_att_bwd_step_centered(c):
    """the last two cases: tanh_ws nearly constant over the locations, a dweight with a large common part - what the centring exists for"""
    O = ops()
    L, D = c[:2]
    inp = RU.att_bwd_make(c[:2], near_const=c[2])
    b = att_bwd_inputs(inp, L, D)
    outs = twice(lambda: dict(ddot=Buf(1, L), datt_h=Buf(1, D)),
                 lambda o: O.cap_att_bwd_step_centered(b['dweight'].t, b['tanh_ws'].t, b['weight'].t, b['aw'].t, L, D, o['ddot'].t, o['datt_h'].t),
                 'topdown_att_bwd_step_kernel')
    verify('cap_att_bwd_step_centered', str(c), outs, RU.att_bwd_centered_ref(inp))
    unchanged(*b.values())


@pytest.mark.parametrize('c', RU.ATT_LD, ids=RU.ld_id)
def test_cap_attention_bwd(c):
    """two launches: dweight lands in datt_h + D; the second stage starts from it.  dpatt, datt, daw, dab accumulate onto random values"""
    O = ops()
    L, D = c
    inp = RU.att_bwd_make(c)
    b = att_bwd_inputs(inp, L, D)
    outs = twice(lambda: dict(dpatt=Buf(L, D, init=inp['dpatt0']), datt=Buf(L, D, init=inp['datt0']), dh=Buf(1, D + L), daw=vec(inp['daw0']), dab=vec(inp['dab0'])),
                 lambda o: O.cap_attention_bwd(b['dres'].t, b['att'].t, b['tanh_ws'].t, b['weight'].t, b['aw'].t, L, D, o['dpatt'].t, o['datt'].t, o['dh'].t,
                                               o['daw'].t, o['dab'].t), 'cap_att_bwd_kernel')
    dh = outs.pop('dh')
    dh.assert_untouched_outside()
    dhv = dh.get().reshape(-1)
    verify('cap_attention_bwd', RU.ld_id(c) + ' dweight', dict(dweight=Buf(1, L, init=dhv[D:])), RU.att_bwd_dw_ref(inp))
    outs['datt_h'] = Buf(1, D, init=dhv[:D])
    verify('cap_attention_bwd', RU.ld_id(c), outs, RU.att_bwd_full_ref(dict(inp, dweight=dhv[D:].copy())))
    unchanged(b['dres'], b['att'], b['tanh_ws'], b['weight'], b['aw'])


@pytest.mark.parametrize('c', RU.ATT_BWD_BATCHED, ids=str)
def test_cap_attention_bwd_batched(c):
    """(the kernel keeps nothing in LDS that L or S sizes: its entry takes them unchecked)"""
    O = ops()
    S, L, D, has_dres, ldr = c
    inp = RU.att_bwd_batched_make(c)
    ddot, wgt, dres, tws, aw = Buf(S, L, init=inp['ddot']), Buf(S, L, init=inp['weight']), Buf(S, D, ld=ldr, init=inp['dres']), Buf(S * L, D, init=inp['tanh_ws'].reshape(S * L, D)), vec(inp['aw'])
    outs = twice(lambda: dict(dpatt=Buf(L, D, init=inp['dpatt0']), datt=Buf(L, D, init=inp['datt0']), daw=vec(inp['daw0']), dab=vec(inp['dab0'])),
                 lambda o: O.cap_attention_bwd_batched(ddot.t, wgt.t, dres.t if has_dres else None, ldr, tws.t, aw.t, S, L, D, o['dpatt'].t, o['datt'].t, o['daw'].t, o['dab'].t),
                 'cap_att_bwd_batched_kernel')
    if not has_dres:
        outs.pop('datt').assert_unchanged('datt without dres')
    verify('cap_attention_bwd_batched', str(c), outs, RU.att_bwd_batched_ref(inp, has_dres))
    unchanged(ddot, wgt, dres, tws, aw)


# ------------------------------------------------------------------------------------------------------------------ fused GEMVs
@pytest.mark.parametrize('c', RU.LINEAR2, ids=str)
def test_linear2_fwd(c):
    O = ops()
    N1, N2, K = c
    inp = RU.linear2_make(c)
    x, w1, b1, w2, b2 = vec(inp['x']), Buf(N1, K, init=inp['w1']), vec(inp['b1']), Buf(N2, K, init=inp['w2']), vec(inp['b2'])
    for v in RU.LINEAR2_VARIANTS:
        acc1, acc2, hb1, hb2 = v
        outs = twice(lambda: dict(y1=vec(inp['y10']), y2=vec(inp['y20'])),
                     lambda o: O.linear2_fwd(x.t, K, w1.t, b1.t if hb1 else None, o['y1'].t, N1, acc1, w2.t, b2.t if hb2 else None, o['y2'].t, N2, acc2), 'linear2_fwd_kernel')
        verify('linear2_fwd', '%s %s' % (c, v), outs, RU.linear2_ref(inp, *v))
    unchanged(x, w1, b1, w2, b2)


@pytest.mark.parametrize('c', RU.LINEAR_SUM2, ids=str)
def test_linear_sum2_fwd(c):
    O = ops()
    N, K1, K2, kernel = c
    inp = RU.linear_sum2_make(c)
    x1, w1, x2, w2 = vec(inp['x1']), Buf(N, K1, init=inp['w1']), vec(inp['x2']), Buf(N, K2, init=inp['w2'])
    for acc in (False, True):
        outs = twice(lambda: dict(y=vec(inp['y0'])), lambda o: O.linear_sum2_fwd(x1.t, w1.t, K1, x2.t, w2.t, K2, o['y'].t, N, accumulate=acc), kernel)
        verify('linear_sum2_fwd', '%s acc %d' % (c, acc), outs, RU.linear_sum2_ref(inp, acc))
    unchanged(x1, w1, x2, w2)


# ------------------------------------------------------------------------------------------------------------------ top-down cell, packer
def seg_bufs(c, inp, rows):
    segs, keep = [], []
    for k, n in enumerate(c[1]):
        ld = RU.seg_ld(c, n)
        x, w = Buf(1, n, off=c[2].get('xoff', 0) if k == 0 else 0, init=inp['xs'][k]), Buf(rows, n, ld=ld, init=inp['ws'][k])
        keep += [x, w]
        segs.append((x.t, w.t, ld, n))
    return segs, keep


@pytest.mark.parametrize('c', RU.TOPDOWN_FWD, ids=RU.topdown_id)
def test_topdown_cell_fwd(c):
    O = ops()
    R, ns, o_, kernel = c
    inp = RU.topdown_fwd_make(c)
    segs, keep = seg_bufs(c, inp, 4 * R)
    pre, add0, add1, cp = vec(inp['pre']), vec(inp['add0']), vec(inp['add1']), vec(inp['c_prev'])
    outs = twice(lambda: dict(c=Buf(1, R), h=Buf(1, R), act=Buf(4, R)),
                 lambda o: O.topdown_cell_fwd(pre.t if o_.get('pre') else None, add0.t if o_.get('add0') else None, add1.t if o_.get('add1') else None, segs, cp.t,
                                              o['c'].t, o['h'].t, o['act'].t, R), kernel)
    verify('topdown_cell_fwd', RU.topdown_id(c), outs, RU.topdown_fwd_ref(inp, o_))
    unchanged(pre, add0, add1, cp, *keep)


@pytest.mark.parametrize('c', RU.TOPDOWN_BWD, ids=RU.topdown_id)
def test_topdown_cell_bwd(c):
    O = ops()
    R, ns, o_, kernel = c
    inp = RU.topdown_bwd_make(c)
    segs, keep = seg_bufs(c, inp, R)
    add0, add1, dc, act, cp, cc = vec(inp['add0']), vec(inp['add1']), vec(inp['dc_in']), vec(inp['act']), vec(inp['c_prev']), vec(inp['c'])
    outs = twice(lambda: dict(dg=Buf(4, R), dc_prev=Buf(1, R)),
                 lambda o: O.topdown_cell_bwd(segs, add0.t if o_.get('add0') else None, add1.t if o_.get('add1') else None, dc.t if o_.get('dc_in') else None, act.t, cp.t,
                                              cc.t, o['dg'].t, o['dc_prev'].t, R), kernel)
    verify('topdown_cell_bwd', RU.topdown_id(c), outs, RU.topdown_bwd_ref(inp, o_))
    unchanged(add0, add1, dc, act, cp, cc, *keep)


@pytest.mark.parametrize('c', RU.PACK_ROWS, ids=str)
def test_pack_rows(c):
    O = ops()
    rows, cols, ldd, lds = c
    src = RU.rnd(np.random.RandomState(RU.seed(16, *c)), (1 if lds == 0 else rows, cols))
    s = Buf(src.shape[0], cols, ld=max(lds, cols), init=src)
    outs = twice(lambda: dict(dst=Buf(rows, cols, ld=ldd)), lambda o: O.pack_rows(o['dst'].t, ldd, s.t, lds, rows, cols), 'topdown_pack_rows_kernel')
    assert np.array_equal(outs['dst'].get().view(np.int32), np.ascontiguousarray(np.broadcast_to(src, (rows, cols))).view(np.int32))
    outs['dst'].assert_untouched_outside()
    unchanged(s)


# ------------------------------------------------------------------------------------------------------------------ encoder steps
STEP = dict(lstm=('lstm_step_fwd', RU.lstm_step_fwd_ref, ('c', 'h', 'act', 'g_out'), 'lstm_step_bwd', RU.lstm_step_bwd_ref),
            gru=('gru_step_fwd', RU.gru_step_fwd_ref, ('h', 'act'), 'gru_step_bwd', RU.gru_step_bwd_ref),
            rnn=('rnn_step_fwd', RU.rnn_step_fwd_ref, ('h',), 'rnn_step_bwd', RU.rnn_step_bwd_ref))
ROWS = dict(c=1, h=1, act=4, g_out=1, dg=4, dc_prev=1, dgi=3, dgh=3, carry_out=1)


def step_outs(keys, ndir, H, kind):
    def rows(k):
        return {('lstm', 'g_out'): 4, ('rnn', 'dg'): 1}.get((kind, k), ROWS[k])
    return lambda: {'%s%d' % (k, i): Buf(rows(k), H) for i in range(ndir) for k in keys}


@pytest.mark.parametrize('kind', ['lstm', 'gru', 'rnn'])
@pytest.mark.parametrize('c', RU.STEP_FWD, ids=RU.step_id)
def test_step_fwd(kind, c):
    """one step on given inputs; the two directions carry different data, so a swapped blockIdx.y shows"""
    O = ops()
    H, ndir = c
    name, ref, keys = STEP[kind][:3]
    ds = RU.step_fwd_make(kind, c)
    G = ds[0]['w'].shape[0] // H
    ins = [dict(w_hh=Buf(G * H, H, init=d['w']), b_hh=vec(d['b']), gates_in=vec(d['g_in']), h_prev=vec(d['h_prev']), c_prev=vec(d['c_prev'])) for d in ds]

    def launch(o):
        dirs = []
        for i, b in enumerate(ins):
            q = {k: v.t for k, v in b.items()}
            for field, key in (('c', 'c'), ('h', 'h'), ('act', 'act'), ('gates_out', 'g_out')):
                if key in keys:
                    q[field] = o['%s%d' % (key, i)].t
            dirs.append(q)
        getattr(O, name)(dirs, H)
    outs = twice(step_outs(keys, ndir, H, kind), launch, name + '_kernel')
    for i, d in enumerate(ds):
        verify(name, '%s dir %d' % (RU.step_id(c), i), {k: outs['%s%d' % (k, i)] for k in keys}, ref(d))
    unchanged(*[v for b in ins for v in b.values()])


@pytest.mark.parametrize('kind', ['lstm', 'gru', 'rnn'])
@pytest.mark.parametrize('c', RU.STEP_BWD, ids=RU.step_id)
def test_step_bwd(kind, c):
    """one backward step from the saved values handed to it: at the first step processed, at a later one, and with both sources of dh"""
    O = ops()
    H, ndir, nxt, ext = c
    name, ref = STEP[kind][3:]
    keys = dict(lstm=('dg', 'dc_prev'), gru=('dgi', 'dgh', 'carry_out'), rnn=('dg',))[kind]
    ds = RU.step_bwd_make(kind, c)
    ins = [{k: (Buf(H, d[k].shape[1], init=d[k]) if k == 'wT' else vec(d[k])) for k in d} for d in ds]

    def launch(o):
        dirs = []
        for i, b in enumerate(ins):
            t = {k: v.t for k, v in b.items()}
            nx, ex = (t['d_next'] if nxt else None), (t['dh_ext'] if ext else None)
            if kind == 'lstm':
                q = dict(w_hh_T=t['wT'], dgates_next=nx, dh_ext=ex, dc_in=t['dc_in'] if nxt else None, act=t['act'], c_prev=t['c_prev'], c=t['c'],
                         dgates=o['dg%d' % i].t, dc_prev=o['dc_prev%d' % i].t)
            elif kind == 'gru':
                q = dict(w_hh_T=t['wT'], dgh_next=nx, dh_ext=ex, dh_carry_in=t['carry_in'] if nxt else None, act=t['act'], h_prev=t['h_prev'],
                         dgi=o['dgi%d' % i].t, dgh=o['dgh%d' % i].t, dh_carry_out=o['carry_out%d' % i].t)
            else:
                q = dict(w_hh_T=t['wT'], dg_next=nx, dh_ext=ex, h=t['h'], dg=o['dg%d' % i].t)
            dirs.append(q)
        getattr(O, name)(dirs, H)
    outs = twice(step_outs(keys, ndir, H, kind), launch, name + '_kernel')
    for i, d in enumerate(ds):
        verify(name, '%s dir %d' % (RU.step_id(c), i), {k: outs['%s%d' % (k, i)] for k in keys}, ref(d, nxt, ext))
    unchanged(*[v for b in ins for v in b.values()])


@pytest.mark.parametrize('H', RU.LSTM_CELL_H)
def test_lstm_cell(H):
    O = ops()
    inp = RU.lstm_cell_make(H)
    g, cp, dh, dc, act, cc = vec(inp['g'].reshape(4, H)), vec(inp['c_prev']), vec(inp['dh']), vec(inp['dc_in']), vec(inp['act']), vec(inp['c'])
    outs = twice(lambda: dict(c=Buf(1, H), h=Buf(1, H), act=Buf(4, H)), lambda o: O.lstm_cell_fwd(g.t, cp.t, o['c'].t, o['h'].t, o['act'].t, H), 'lstm_cell_fwd_kernel')
    keep = ordinary(inp['g'].reshape(4, H))
    verify('lstm_cell_fwd', 'H%d' % H, outs, RU.lstm_cell_fwd_ref(inp), libm_on=[('act', q, keep[q]) for q in range(4)])
    for has_dc in (False, True):
        outs = twice(lambda: dict(dg=Buf(4, H), dc_prev=Buf(1, H)),
                     lambda o: O.lstm_cell_bwd(dh.t, dc.t if has_dc else None, act.t, cp.t, cc.t, o['dg'].t, o['dc_prev'].t, H), 'lstm_cell_bwd_kernel')
        verify('lstm_cell_bwd', 'H%d dc_in %d' % (H, has_dc), outs, RU.lstm_cell_bwd_ref(inp, has_dc))
    unchanged(g, cp, dh, dc, act, cc)


@pytest.mark.parametrize('c', RU.RNN_CONCAT, ids=str)
def test_rnn_concat(c):
    """the copies and the masked zeros bit for bit (mask values 0 and 2: exact products); the add at a direction's last row within the bound"""
    O = ops()
    T, H, ndir, has_mask, has_adds = c
    inp = RU.rnn_concat_make(c)
    hs, mask, dx, adds = [Buf(T, H, init=h) for h in inp['hs']], Buf(T, ndir * H, init=inp['mask']), Buf(T, ndir * H, init=inp['dx']), [vec(a) for a in inp['adds']]
    outs = twice(lambda: dict(out=Buf(T, ndir * H)), lambda o: O.rnn_concat_fwd([h.t for h in hs], mask.t if has_mask else None, o['out'].t, T, H), 'rnn_concat_fwd_kernel')
    ref = RU.rnn_concat_fwd_ref(inp, has_mask)
    got = verify('rnn_concat_fwd', str(c), outs, ref)
    assert np.array_equal(got['out'], ref['out']['ref'].astype(np.float32))
    outs = twice(lambda: {'d%d' % k: Buf(T, H) for k in range(ndir)},
                 lambda o: O.rnn_concat_bwd(dx.t, mask.t if has_mask else None, [a.t if has_adds else None for a in adds], [o['d%d' % k].t for k in range(ndir)], T, H),
                 'rnn_concat_bwd_kernel')
    ref = RU.rnn_concat_bwd_ref(inp, has_mask, has_adds)
    got = verify('rnn_concat_bwd', str(c), outs, ref)
    for k in range(ndir):
        rows = np.arange(T) != (T - 1 if k == 0 else 0) if has_adds else np.ones(T, bool)
        assert np.array_equal(got['d%d' % k][rows], ref['d%d' % k]['ref'][rows].astype(np.float32))
    unchanged(mask, dx, *(hs + adds))


# ------------------------------------------------------------------------------------------------------------------ adaptive attention
@pytest.mark.parametrize('c', RU.ADAATT_CELL_FWD, ids=str)
def test_adaatt_cell_fwd(c):
    O = ops()
    R, G, ld_hh, ld_r, hoff, kernel = c
    inp = RU.adaatt_cell_fwd_make(c)
    pre, fc, w_hh, b_hh, w_r, b_r = vec(inp['pre']), vec(inp['fcrow']), Buf(G * R, R, ld=ld_hh, init=inp['w_hh']), vec(inp['b_hh']), Buf(R, R, ld=ld_r, init=inp['w_r']), vec(inp['b_r'])
    hp, cp = Buf(1, R, off=hoff, init=inp['h_prev']), vec(inp['c_prev'])
    outs = twice(lambda: dict(c=Buf(1, R), h=Buf(1, R), fake=Buf(1, R), save=Buf(7, R)),
                 lambda o: O.adaatt_cell_fwd(pre.t, fc.t, w_hh.t, b_hh.t, w_r.t, b_r.t, hp.t, cp.t, o['c'].t, o['h'].t, o['fake'].t, o['save'].t, R, G, ld_hh=ld_hh, ld_r=ld_r),
                 kernel)
    got = verify('adaatt_cell_fwd', str(c), outs, RU.adaatt_cell_fwd_ref(inp, G))
    if G == 5:
        assert (got['save'][4][inp['ties']] == 0).all() and (got['save'][4][inp['ups']] == 1).all() and (got['save'][4][inp['downs']] == 0).all()
    unchanged(pre, fc, w_hh, b_hh, w_r, b_r, hp, cp)


@pytest.mark.parametrize('c', RU.ADAATT_CELL_BWD, ids=str)
def test_adaatt_cell_bwd(c):
    """with dsn (an earlier token) and without (the last one)"""
    O = ops()
    R, G, ld_thh, ld_tr, has, kernel = c
    inp = RU.adaatt_cell_bwd_make(c)
    dsn, t_hh, t_r = vec(inp['dsn']), Buf(R, G * R, ld=ld_thh, init=inp['t_hh']), Buf(R, R, ld=ld_tr, init=inp['t_r'])
    ext, dfake, dc, sv, cp = vec(inp['dh_ext']), vec(inp['dfake']), vec(inp['dc_in']), vec(inp['save']), vec(inp['c_prev'])
    outs = twice(lambda: dict(ds=Buf(G + 1, R), dc_prev=Buf(1, R)),
                 lambda o: O.adaatt_cell_bwd(dsn.t if has[0] else None, t_hh.t, t_r.t, ext.t if has[1] else None, dfake.t if has[2] else None, dc.t if has[3] else None,
                                             sv.t, cp.t, o['ds'].t, o['dc_prev'].t, R, G, ld_thh=ld_thh, ld_tr=ld_tr), kernel)
    got = verify('adaatt_cell_bwd', str(c), outs, RU.adaatt_cell_bwd_ref(inp, G, has))
    if G == 5:
        first = inp['save'][4] == 0
        assert (got['ds'][4][first] == 0).all() and (got['ds'][3][~first] == 0).all()
    unchanged(dsn, t_hh, t_r, ext, dfake, dc, sv, cp)


@pytest.mark.parametrize('c', RU.ADAATT_ATT, ids=str)
def test_adaatt_att_fwd(c):
    """two launches: the scores (tanh_ws, dots) and, from the dots they stored, PI and atten; the tokens carry different data"""
    O = ops()
    S, L, R, has_mask = c
    L1 = L + 1
    inp = RU.adaatt_att_make(c)
    b = {k: Buf(inp[k].shape[0], R, init=inp[k]) for k in ('att', 'patt', 'frl', 'fre', 'hoe', 'hol')}
    aw, ab, mask = vec(inp['aw']), vec(inp['ab']), Buf(S * L1, R, init=inp['mask'].reshape(S * L1, R))
    outs = twice(lambda: dict(tanh_ws=Buf(S * L1, R), dots=Buf(S, L1, ld=256), PI=Buf(S, L1), atten=Buf(S, R)),
                 lambda o: O.adaatt_att_fwd(b['att'].t, b['patt'].t, b['frl'].t, b['fre'].t, b['hoe'].t, b['hol'].t, aw.t, ab.t, mask.t if has_mask else None, S, L, R,
                                            o['tanh_ws'].t, o['dots'].t, o['PI'].t, o['atten'].t), 'adaatt_apply_kernel')
    got = verify('adaatt_att_fwd', str(c) + ' scores', dict(tanh_ws=outs['tanh_ws'], dots=outs['dots']), RU.adaatt_scores_ref(inp, has_mask), libm_on=[('tanh_ws', None, None)])
    verify('adaatt_att_fwd', str(c) + ' apply', dict(PI=outs['PI'], atten=outs['atten']), RU.adaatt_apply_ref(dict(inp, dots=got['dots'])))
    unchanged(aw, ab, mask, *b.values())


@pytest.mark.parametrize('c', RU.ADAATT_ATT, ids=str)
def test_adaatt_att_bwd_step(c):
    O = ops()
    S, L, R, has_mask = c
    L1 = L + 1
    inp = RU.adaatt_att_make(c)
    datten, att, frl, tws, mask, PI, aw = (Buf(S, R, init=inp['datten']), Buf(L, R, init=inp['att']), Buf(S, R, init=inp['frl']), Buf(S * L1, R, init=inp['tanh_ws'].reshape(S * L1, R)),
                                            Buf(S * L1, R, init=inp['mask'].reshape(S * L1, R)), Buf(S, L1, init=inp['PI']), vec(inp['aw']))
    keys = ('dhoe', 'dfre', 'dctx', 'dfrl', 'dhol')
    outs = twice(lambda: dict(ddot=Buf(S, L1), **{k: Buf(S, R) for k in keys}),
                 lambda o: O.adaatt_att_bwd_step(datten.t, att.t, frl.t, tws.t, mask.t if has_mask else None, PI.t, aw.t, S, L, R, o['ddot'].t, *[o[k].t for k in keys]),
                 'adaatt_att_bwd_step_kernel')
    got = verify('adaatt_att_bwd_step', str(c), outs, RU.adaatt_bwd_step_ref(inp, has_mask))
    assert np.array_equal(got['dhol'], inp['datten'])
    unchanged(datten, att, frl, tws, mask, PI, aw)


@pytest.mark.parametrize('c', RU.ADAATT_ATT, ids=str)
def test_adaatt_att_bwd_batched(c):
    O = ops()
    S, L, R, has_mask = c
    L1 = L + 1
    inp = RU.adaatt_att_make(c)
    ddot, PI, datten, tws, mask, aw = (Buf(S, L1, init=inp['ddot']), Buf(S, L1, init=inp['PI']), Buf(S, R, init=inp['datten']), Buf(S * L1, R, init=inp['tanh_ws'].reshape(S * L1, R)),
                                       Buf(S * L1, R, init=inp['mask'].reshape(S * L1, R)), vec(inp['aw']))
    outs = twice(lambda: dict(dpatt=Buf(L, R, init=inp['dpatt0']), datt=Buf(L, R, init=inp['datt0']), daw=vec(inp['daw0'])),
                 lambda o: O.adaatt_att_bwd_batched(ddot.t, PI.t, datten.t, tws.t, mask.t if has_mask else None, aw.t, S, L, R, o['dpatt'].t, o['datt'].t, o['daw'].t),
                 'adaatt_att_bwd_batched_kernel')
    verify('adaatt_att_bwd_batched', str(c), outs, RU.adaatt_bwd_batched_ref(inp, has_mask))
    unchanged(ddot, PI, datten, tws, mask, aw)


# ------------------------------------------------------------------------------------------------------------------ resident recurrence
@pytest.mark.parametrize('c', RU.RECUR, ids=str)
def test_cap_recur(c):
    """one resident launch per direction on the default stream, nothing beside it.  Forward token by token from the kernel's OWN hs[t], cs[t]
    (nothing propagates across tokens; inside the token the chain's bound is written out in recur_kernels_util.recur_token_core); backward at
    the last token, where the carries are zero, from the saved values forward stored.  The give-up flags and the launch counters as
    tests/test_kernels_gpu.py::test_captioner_resident_recurrence asserts them"""
    O = ops()
    S, L = c
    R = AH = RU.RECUR_R
    assert O.cap_recur_supported(S, R, AH, L)
    inp = RU.recur_make(c)
    dv = {k: Buf(1, inp[k].size, init=inp[k].reshape(1, -1)) for k in ('W_h2h', 'b_h2h', 'W_att', 'b_att', 'patt', 'aw', 'ab', 'P', 'b_a2c', 'sums', 'dho')}
    st = (O.cap_recur_state(False), O.cap_recur_state(True))
    nan = float('nan')
    hs, cs = Buf(S + 1, R, init=np.zeros((S + 1, R), np.float32)), Buf(S + 1, R, init=np.zeros((S + 1, R), np.float32))
    save, tws, wgt = Buf(S, 6 * R, fill=nan), Buf(S * L, AH, fill=nan), Buf(S, L, fill=nan)
    dsums, da2c, ddot, datt_h = Buf(S, 5 * R, fill=nan), Buf(S, 2 * R, fill=nan), Buf(S, L, fill=nan), Buf(S, AH, ld=AH + 256, fill=nan)
    torch.cuda.synchronize()
    O.cap_recur_fwd(dv['W_h2h'].t, dv['b_h2h'].t, dv['W_att'].t, dv['b_att'].t, dv['patt'].t, dv['aw'].t, dv['ab'].t, dv['P'].t, dv['b_a2c'].t, dv['sums'].t,
                    hs.t, cs.t, save.t, tws.t, wgt.t, st[0], S, R, AH, L)
    landed('cap_recur_fwd_kernel')
    O.cap_recur_bwd(dv['W_h2h'].t, dv['W_att'].t, dv['P'].t, dv['aw'].t, save.t, cs.t, wgt.t, tws.t, dv['dho'].t, dsums.t, da2c.t, ddot.t.view(S, L),
                    datt_h.t.view(S, AH + 256), st[1], S, R, AH, L)
    landed('cap_recur_bwd_kernel')
    torch.cuda.synchronize()
    assert int(st[0][1].item()) == 0 and int(st[1][1].item()) == 0, 'a bounded spin of the resident recurrence gave up'
    assert int(st[0][0].item()) == 1 and int(st[1][0].item()) == 1
    H, Cs, SV, TW, WG = hs.get(), cs.get(), save.get().reshape(S, 6, R), tws.get().reshape(S, L, AH), wgt.get()
    assert not H[0].any() and not Cs[0].any()
    for b in (hs, cs, save, tws, wgt, dsums, da2c, ddot, datt_h):
        b.assert_untouched_outside()
    for t in range(S):
        ref, amb = RU.recur_token_ref(dict(inp, h=H[t], c=Cs[t]), t)
        got = dict(tanh_ws=TW[t], wgt=WG[t], save=SV[t].copy(), c=Cs[t + 1], h=H[t + 1])
        got['save'][3][amb] = ref['save']['ref'][3][amb]              # a selector float32 may decide either way is not compared; its max, c and h are
        w = max(check_out(got[k], ref[k], 'f32', L_LIBM, 'cap_recur_fwd %s token %d %s' % (c, t, k)) for k in sorted(ref))
        WORST['cap_recur_fwd'] = max(WORST.get('cap_recur_fwd', 0.0), w)
        print('cap_recur_fwd %s token %d: worst ratio %.3g, %d undecided selectors' % (c, t, w, int(amb.sum())))
    ref = RU.recur_bwd_last_ref(dict(inp, save=SV[S - 1], c=Cs[S - 1], wgt=WG[S - 1], tanh_ws=TW[S - 1]))
    got = dict(dsums=dsums.get()[S - 1].reshape(5, R), da2c=da2c.get()[S - 1].reshape(2, R), ddot=ddot.get()[S - 1], datt_h=datt_h.get()[S - 1])
    w = max(check_out(got[k], ref[k], 'f32', L_LIBM, 'cap_recur_bwd %s %s' % (c, k)) for k in sorted(ref))
    WORST['cap_recur_bwd'] = max(WORST.get('cap_recur_bwd', 0.0), w)
    print('cap_recur_bwd %s last token: worst ratio %.3g' % (c, w))
    unchanged(*dv.values())


# ------------------------------------------------------------------------------------------------------------------ rejections
def test_entry_points_refuse_what_their_kernels_cannot_take():
    """each entry's first refused value, once: L2SError, every buffer untouched, ops.last_kernel() as it was.  (l2s_lstm_step_fwd / _bwd took
    H = 0 until this file: a grid of no workgroups, a failed launch after last_kernel had moved; l2s_cap_attention_bwd_step took pointers its
    float4 loads cannot: both are refused now.)"""
    O = ops()
    from lang2seg_amd._lib import L2SError
    O.pack_rows(Buf(1, 4).t, 4, Buf(1, 4).t, 4, 1, 4)
    before = O.last_kernel()
    RL, RR, RA = RU.ATT_REJECT_L, RU.GATES_BWD_DW_REJECT_R, RU.ADAATT_REJECT_L      # the first refused L, R of cap_gates_bwd_dw, L of the adaptive attention
    n = RL * RR + 64
    bufs = [Buf(1, n) for _ in range(12)]
    a, b, c_, d, e, f, g, h, i, j, k, l = [x.t for x in bufs]
    off = Buf(1, n, off=1).t                                           # one float off 16-byte alignment
    seg = lambda ld, nn: (a, b, ld, nn)
    dirs = lambda keys: [dict((key, a) for key in keys)] * 3
    LF = ('w_hh', 'b_hh', 'gates_in', 'h_prev', 'c_prev', 'c', 'h', 'act', 'gates_out')
    LB = ('w_hh_T', 'dgates_next', 'dh_ext', 'dc_in', 'act', 'c_prev', 'c', 'dgates', 'dc_prev')
    GF, GB = ('w_hh', 'b_hh', 'gates_in', 'h_prev', 'h', 'act'), ('w_hh_T', 'dgh_next', 'dh_ext', 'dh_carry_in', 'act', 'h_prev', 'dgi', 'dgh', 'dh_carry_out')
    RF, RB = ('w_hh', 'b_hh', 'gates_in', 'h_prev', 'h'), ('w_hh_T', 'dg_next', 'dh_ext', 'h', 'dg')
    calls = [
        ('cap_attention_fwd L = 257', lambda: O.cap_attention_fwd(a, b, c_, d, e, RL, 8, f, g, h)),
        ('cap_att_dots_fwd L = 257', lambda: O.cap_att_dots_fwd(a, b, c_, d, RL, 8, e, f)),
        ('cap_att_apply_fwd L = 257', lambda: O.cap_att_apply_fwd(a, b, RL, 8, c_, d)),
        ('cap_apply_gates_fwd L = 257', lambda: O.cap_apply_gates_fwd(a, b, c_, d, e, f, g, h, i, 257, 8)),
        ('cap_attention_bwd L = 257', lambda: O.cap_attention_bwd(a, b, c_, d, e, RL, 8, f, g, h, i, j)),
        ('cap_attention_bwd_step L = 257', lambda: O.cap_attention_bwd_step(a, b, c_, d, e, RL, 8, f, g)),
        ('cap_attention_bwd_step datt_res misaligned', lambda: O.cap_attention_bwd_step(off, b, c_, d, e, 3, 8, f, g)),
        ('cap_attention_bwd_step att misaligned', lambda: O.cap_attention_bwd_step(a, off, c_, d, e, 3, 8, f, g)),
        ('cap_attention_bwd_step D = 6', lambda: O.cap_attention_bwd_step(a, b, c_, d, e, 3, 6, f, g)),
        ('cap_attention_bwd_step2 L = 257', lambda: O.cap_attention_bwd_step2(a, b, c_, d, RL, 8, e, f)),
        ('cap_att_bwd_step_centered L = 257', lambda: O.cap_att_bwd_step_centered(a, b, c_, d, RL, 8, e, f)),
        ('cap_gates_bwd_dw R = 1028', lambda: O.cap_gates_bwd_dw(a, b, c_, d, e, f, g, h, i, 3, RR, dh2=j)),
        ('cap_gates_bwd_dw R = 6', lambda: O.cap_gates_bwd_dw(a, b, c_, d, e, f, g, h, i, 3, 6, dh2=j)),
        ('cap_gates_bwd_dw P misaligned', lambda: O.cap_gates_bwd_dw(a, b, c_, d, off, f, g, h, i, 3, 8, dh2=j)),
        ('cap_a2c_gates_fwd K = 6', lambda: O.cap_a2c_gates_fwd(a, b, c_, 6, d, e, f, g, h, 8)),
        ('cap_a2c_gates_fwd att_res misaligned', lambda: O.cap_a2c_gates_fwd(off, b, c_, 8, d, e, f, g, h, 8)),
        ('linear2_fwd K = 6', lambda: O.linear2_fwd(a, 6, b, c_, d, 5, 0, e, f, g, 5, 0)),
        ('linear2_fwd w2 misaligned', lambda: O.linear2_fwd(a, 8, b, c_, d, 5, 0, off, f, g, 5, 0)),
        ('linear_sum2_fwd K2 = 6', lambda: O.linear_sum2_fwd(a, b, 8, c_, d, 6, e, 5)),
        ('linear_sum2_fwd x1 misaligned', lambda: O.linear_sum2_fwd(off, b, 8, c_, d, 8, e, 5)),
        ('topdown_cell_fwd R = 6', lambda: O.topdown_cell_fwd(a, None, None, [seg(8, 8)], c_, d, e, f, 6)),
        ('topdown_cell_fwd ld < n', lambda: O.topdown_cell_fwd(a, None, None, [seg(4, 8)], c_, d, e, f, 8)),
        ('topdown_cell_bwd R = 6', lambda: O.topdown_cell_bwd([seg(8, 8)], None, None, None, c_, d, e, f, g, 6)),
        ('topdown_cell_bwd ld < n', lambda: O.topdown_cell_bwd([None, None, seg(4, 8)], None, None, None, c_, d, e, f, g, 8)),
        ('pack_rows ldd < cols', lambda: O.pack_rows(a, 7, b, 8, 3, 8)),
        ('pack_rows lds < cols', lambda: O.pack_rows(a, 8, b, 7, 3, 8)),
        ('lstm_step_fwd ndir = 3', lambda: O.lstm_step_fwd(dirs(LF), 8)), ('lstm_step_fwd H = 6', lambda: O.lstm_step_fwd(dirs(LF)[:1], 6)),
        ('lstm_step_fwd H = 0', lambda: O.lstm_step_fwd(dirs(LF)[:1], 0)),
        ('lstm_step_bwd ndir = 3', lambda: O.lstm_step_bwd(dirs(LB), 8)), ('lstm_step_bwd H = 6', lambda: O.lstm_step_bwd(dirs(LB)[:1], 6)),
        ('lstm_step_bwd H = 0', lambda: O.lstm_step_bwd(dirs(LB)[:1], 0)),
        ('gru_step_fwd ndir = 3', lambda: O.gru_step_fwd(dirs(GF), 8)), ('gru_step_fwd H = 6', lambda: O.gru_step_fwd(dirs(GF)[:1], 6)),
        ('gru_step_bwd ndir = 3', lambda: O.gru_step_bwd(dirs(GB), 8)), ('gru_step_bwd H = 0', lambda: O.gru_step_bwd(dirs(GB)[:1], 0)),
        ('rnn_step_fwd ndir = 3', lambda: O.rnn_step_fwd(dirs(RF), 8)), ('rnn_step_fwd H = 6', lambda: O.rnn_step_fwd(dirs(RF)[:1], 6)),
        ('rnn_step_bwd ndir = 3', lambda: O.rnn_step_bwd(dirs(RB), 8)), ('rnn_step_bwd H = 0', lambda: O.rnn_step_bwd(dirs(RB)[:1], 0)),
        ('adaatt_att_fwd L + 1 = 257', lambda: O.adaatt_att_fwd(a, b, c_, d, e, f, g, h, None, 1, RA, 8, i, j, k, l)),
        ('adaatt_att_bwd_step L + 1 = 257', lambda: O.adaatt_att_bwd_step(a, b, c_, d, None, e, f, 1, RA, 8, g, h, i, j, k, l)),
        ('adaatt_att_bwd_step R = 6', lambda: O.adaatt_att_bwd_step(a, b, c_, d, None, e, f, 1, 3, 6, g, h, i, j, k, l)),
        ('adaatt_att_bwd_step datten misaligned', lambda: O.adaatt_att_bwd_step(off, b, c_, d, None, e, f, 1, 3, 8, g, h, i, j, k, l)),
        ('adaatt_att_bwd_batched L + 1 = 257', lambda: O.adaatt_att_bwd_batched(a, b, c_, d, None, e, 1, RA, 8, f, g, h)),
        ('adaatt_cell_fwd R = 6', lambda: O.adaatt_cell_fwd(a, b, c_, d, e, f, g, h, i, j, k, l, 6, 4)),
        ('adaatt_cell_fwd G = 3', lambda: O.adaatt_cell_fwd(a, b, c_, d, e, f, g, h, i, j, k, l, 8, 3)),
        ('adaatt_cell_fwd ld_hh < R', lambda: O.adaatt_cell_fwd(a, b, c_, d, e, f, g, h, i, j, k, l, 8, 4, ld_hh=4)),
        ('adaatt_cell_bwd R = 6', lambda: O.adaatt_cell_bwd(a, b, c_, d, e, f, g, h, i, j, 6, 4)),
        ('adaatt_cell_bwd ld_thh < G R', lambda: O.adaatt_cell_bwd(a, b, c_, d, e, f, g, h, i, j, 8, 5, ld_thh=32)),
        ('rnn_concat_fwd ndir = 3', lambda: O.rnn_concat_fwd([a, b, c_], None, d, 3, 8)),
        ('rnn_concat_bwd ndir = 3', lambda: O.rnn_concat_bwd(a, None, [None, None, None], [b, c_, d], 3, 8)),
    ]
    for what, fn in calls:
        with pytest.raises(L2SError):
            fn()
        assert O.last_kernel() == before, '%s moved last_kernel' % what
    torch.cuda.synchronize()
    for x in bufs:
        x.assert_unchanged()


# ------------------------------------------------------------------------------------------------------------------ the file as a whole
def test_libm_allowance_rule():
    """the allowance is at least four times the worst measured error: L_LIBM for the tanhf and sigmoid values, L_LIBM * SOFTMAX_L for the
    softmax weights (needs the tests above to have run)"""
    assert RU.L_SETTLE == L_LIBM, 'the redraw margins of the gate tables assume another allowance'
    assert LIBM, 'no libm value was measured: run the whole file'
    print('libm, |got - ref| / (2^-23 |value|): ' + ', '.join('%s (%s) %.3g' % (k[0], k[1], v) for k, v in sorted(LIBM.items())))
    print('worst check ratio per entry point: ' + ', '.join('%s %.3g' % kv for kv in sorted(WORST.items())))
    for cls, L in (('gate', L_LIBM), ('softmax', L_LIBM * RU.SOFTMAX_L)):
        worst = max(v for k, v in LIBM.items() if k[1] == cls)
        assert 4 * worst <= L, 'the worst measured libm error of a %s value is %.3g: its allowance has to be %g' % (cls, worst, 2.0 ** np.ceil(np.log2(4 * worst)))


def test_every_kernel_was_seen():
    assert sorted(SEEN) == sorted(KERNELS), 'not seen: %s; not listed: %s' % (sorted(set(KERNELS) - SEEN), sorted(SEEN - set(KERNELS)))
