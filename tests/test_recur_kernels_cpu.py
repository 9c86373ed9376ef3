"""The float64 references of tests/recur_kernels_util.py and their bounds, pinned without a GPU: every plain torch-CPU float32 form goes
through `check` against its float64 reference on the case tables the GPU file uses, with the libm allowance L = 1 - no bound is tighter
than honest float32 arithmetic in another summation order.  The tie / near-tie redraws of the gate tables are capped here, and one
mutation per kernel family shows the bound is not idle: a dropped location, a missing bias, a neighbour's row, d0 / d1 swapped, a lost tie,
a centred sum taken uncentred and an accumulate turned into a store each fail it."""
import numpy as np
import pytest

import recur_kernels_util as RU
from small_kernels_util import check_out

L_CPU = 1.0
WORST = {}


def through(name, got, ref, what=''):
    """every output of one case through `check`; -> the worst ratio"""
    assert set(got) == set(ref), (name, sorted(got), sorted(ref))
    w = 0.0
    for k in sorted(ref):
        w = max(w, check_out(got[k], ref[k], 'f32', L_CPU, '%s %s %s' % (name, what, k)))
    WORST[name] = max(WORST.get(name, 0.0), w)
    return w


def fails(got, ref, key):
    with pytest.raises(AssertionError):
        check_out(got[key], ref[key], 'f32', L_CPU, key)


# ------------------------------------------------------------------------------------------------------------------ attention forward
@pytest.mark.parametrize('c', RU.ATT_LD, ids=RU.ld_id)
def test_attention_forward_references(c):
    inp = RU.att_fwd_make(c)
    through('att_dots', RU.att_dots_f32(inp), RU.att_dots_ref(inp), c)
    through('att_apply', RU.att_apply_f32(inp), RU.att_apply_ref(inp), c)
    g = RU.apply_gates_make(c)
    got = RU.apply_gates_f32(g)
    got['save'][3, g['ties']] = 0         # (a tie behind a sum is one only where both columns are summed in one order)
    through('apply_gates', got, RU.apply_gates_ref(g), c)


def test_attention_forward_mutations():
    """one dropped location of the weighted sum; the score bias missing"""
    inp = RU.att_fwd_make((50, 68))
    ref, good = RU.att_apply_ref(inp), RU.att_apply_f32(inp)
    through('att_apply', good, ref)
    bad = dict(good)
    bad['att_res'] = good['att_res'] - good['weight'][7] * inp['att'][7]
    fails(bad, ref, 'att_res')
    ref, good = RU.att_dots_ref(inp), RU.att_dots_f32(inp)
    bad = dict(good, dots=good['dots'] - inp['ab'][0])
    fails(bad, ref, 'dots')
    bad = dict(good, tanh_ws=good['tanh_ws'].copy())
    bad['tanh_ws'][3] = good['tanh_ws'][4]                             # a neighbour's location
    fails(bad, ref, 'tanh_ws')


# ------------------------------------------------------------------------------------------------------------------ gate blocks
def planted_ok(inp, R, sel):
    """no planted unit was redrawn, fewer than 1 % of the units were, and the selectors on the planted units are what torch.max gives"""
    ties, ups, downs = RU.planted(R)
    assert (inp['ties'], inp['ups'], inp['downs']) == (ties, ups, downs)
    assert np.array_equal(inp['s'][4, ties], inp['s'][3, ties])
    assert np.array_equal(inp['s'][4, ups], RU.nextf(inp['s'][3, ups], True)) and np.array_equal(inp['s'][4, downs], RU.nextf(inp['s'][3, downs], False))
    assert inp['dropped'] <= max(R // 100, 0) or inp['dropped'] < 0.01 * R, (R, inp['dropped'])
    assert (sel[ties] == 0).all() and (sel[ups] == 1).all() and (sel[downs] == 0).all()
    return len(ties)


def test_gate_tables_plant_ties_and_redraw_few():
    n = dict(gates=0, a2c=0, apply=0)
    for R in RU.GATES_R:
        inp = RU.gates_fwd_make(R)
        n['gates'] += planted_ok(inp, R, RU.gates_fwd_ref(inp)['save']['ref'][3])
    for c in RU.A2C_GATES:
        inp = RU.a2c_gates_make(c)
        n['a2c'] += planted_ok(inp, c[0], RU.a2c_gates_ref(inp)['save']['ref'][3])
    for c in RU.ATT_LD:
        inp = RU.apply_gates_make(c)
        n['apply'] += planted_ok(inp, c[1], RU.apply_gates_ref(inp)['save']['ref'][3])
    assert min(n.values()) >= 8, n


@pytest.mark.parametrize('R', RU.GATES_R)
def test_gates_fwd_reference(R):
    inp = RU.gates_fwd_make(R)
    ref, got = RU.gates_fwd_ref(inp), RU.gates_fwd_f32(inp)
    through('gates_fwd', got, ref, R)
    assert np.array_equal(got['save'][3], ref['save']['ref'][3])      # the float32 selector is the float64 one on every unit drawn


@pytest.mark.parametrize('c', RU.A2C_GATES, ids=str)
def test_a2c_gates_reference(c):
    inp = RU.a2c_gates_make(c)
    ref, got = RU.a2c_gates_ref(inp), RU.a2c_gates_f32(inp)
    got['save'][3, inp['ties']] = 0       # a tie behind a GEMV is one only where both rows are summed in one order (the kernel's wave does; torch's matmul need not)
    through('a2c_gates', got, ref, c)
    p = inp['ups'] + inp['downs']
    assert np.array_equal(got['save'][3][p], ref['save']['ref'][3][p])


@pytest.mark.parametrize('c', RU.GATES_BWD, ids=str)
def test_gates_bwd_reference(c):
    inp = RU.gates_bwd_make(c)
    through('gates_bwd', RU.gates_bwd_f32(inp, c[1], c[2]), RU.gates_bwd_ref(inp, c[1], c[2]), c)


@pytest.mark.parametrize('c', RU.GATES_BWD_DW, ids=str)
def test_gates_bwd_dw_reference(c):
    inp = RU.gates_bwd_make(c)
    got = RU.gates_bwd_f32(inp, c[2], c[3])
    through('gates_bwd_dw', got, RU.gates_bwd_ref(inp, c[2], c[3]), c)
    inp['da2c'] = got['da2c'].reshape(-1)
    through('gates_bwd_dw', RU.dweight_f32(inp), RU.dweight_ref(inp), c)


def test_gate_block_mutations():
    """backward: d0 / d1 swapped (the selector there is an input, so this is the routing, not a tie) and a saturated gate's gradient dropped;
    forward: a unit's sums read from its neighbour, the a2c bias of one unit missing, and the second operand winning an exact tie"""
    R = 260
    inp = RU.gates_bwd_make((R, True, True))
    ref, good = RU.gates_bwd_ref(inp, True, True), RU.gates_bwd_f32(inp, True, True)
    bad = dict(good, da2c=good['da2c'][::-1].copy())
    fails(bad, ref, 'da2c')
    sat = int(np.argmin(np.abs(good['dsums'][0]) + (good['dsums'][0] == 0)))
    bad = dict(good, dsums=good['dsums'].copy())
    bad['dsums'][0, sat] = 0                                          # the smallest gate gradient of the block: norm-wise invisible
    fails(bad, ref, 'dsums')
    inp = RU.a2c_gates_make((260, 260))
    ref, good = RU.a2c_gates_ref(inp), RU.a2c_gates_f32(inp)
    shifted = dict(inp, s=np.roll(inp['s'], 1, axis=1))
    fails(RU.a2c_gates_f32(shifted), ref, 'c')
    nob = dict(inp, b=inp['b'].copy())
    nob['b'][9] = 0
    fails(RU.a2c_gates_f32(nob), ref, 'save')
    # the selector on an exact tie: torch.max lets the first win; the second winning is a wrong 1 where an exact 0 is due
    bad = dict(good, save=good['save'].copy())
    bad['save'][3, inp['ties'][0]] = 1.0
    fails(bad, ref, 'save')


# ------------------------------------------------------------------------------------------------------------------ attention backward
@pytest.mark.parametrize('c', RU.ATT_LD, ids=RU.ld_id)
def test_attention_backward_references(c):
    inp = RU.att_bwd_make(c)
    through('att_bwd_step2', RU.att_bwd_step2_f32(inp), RU.att_bwd_step2_ref(inp), c)
    through('att_bwd_step', RU.att_bwd_step_f32(inp), RU.att_bwd_step_ref(inp), c)
    through('att_bwd_dw', RU.att_bwd_dw_f32(inp), RU.att_bwd_dw_ref(inp), c)
    through('att_bwd_full', RU.att_bwd_full_f32(inp), RU.att_bwd_full_ref(inp), c)


@pytest.mark.parametrize('c', RU.ATT_BWD_CENTERED, ids=str)
def test_attention_backward_centered_reference(c):
    inp = RU.att_bwd_make(c[:2], near_const=c[2])
    through('att_bwd_centered', RU.att_bwd_centered_f32(inp), RU.att_bwd_centered_ref(inp), c)


@pytest.mark.parametrize('c', RU.ATT_BWD_BATCHED, ids=str)
def test_attention_backward_batched_reference(c):
    inp = RU.att_bwd_batched_make(c)
    through('att_bwd_batched', RU.att_bwd_batched_f32(inp, c[3]), RU.att_bwd_batched_ref(inp, c[3]), c)


def test_softmax_backward_mutations():
    """a centred sum taken uncentred on the nearly-constant-tanh case; the softmax backward's inner sum short of one location; an
    accumulate turned into a store"""
    for c in RU.ATT_BWD_CENTERED:
        if c[2]:
            inp = RU.att_bwd_make(c[:2], near_const=True)
            ref = RU.att_bwd_centered_ref(inp)
            through('att_bwd_centered', RU.att_bwd_centered_f32(inp), ref, c)
            fails(RU.att_bwd_uncentered_f32(inp), ref, 'datt_h')
    inp = RU.att_bwd_make((50, 68))
    ref, good = RU.att_bwd_step2_ref(inp), RU.att_bwd_step2_f32(inp)
    w, dw = inp['weight'], inp['dweight']
    l = int(np.argmin(w))                                             # the least-weighted location: the change of every ddot is w[l] times w dw of it
    short = (w * (dw - ((w * dw).sum() - w[l] * dw[l]))).astype(np.float32)
    fails(dict(good, ddot=short), ref, 'ddot')
    ref, good = RU.att_bwd_full_ref(inp), RU.att_bwd_full_f32(inp)
    for k, k0 in (('dpatt', 'dpatt0'), ('datt', 'datt0'), ('daw', 'daw0'), ('dab', 'dab0')):
        fails(dict(good, **{k: good[k] - inp[k0]}), ref, k)


# ------------------------------------------------------------------------------------------------------------------ GEMV pair
@pytest.mark.parametrize('c', RU.LINEAR2, ids=str)
def test_linear2_reference(c):
    inp = RU.linear2_make(c)
    for v in RU.LINEAR2_VARIANTS:
        through('linear2', RU.linear2_f32(inp, *v), RU.linear2_ref(inp, *v), (c, v))


@pytest.mark.parametrize('c', RU.LINEAR_SUM2, ids=str)
def test_linear_sum2_reference(c):
    inp = RU.linear_sum2_make(c)
    for acc in (False, True):
        through('linear_sum2', RU.linear_sum2_f32(inp, acc), RU.linear_sum2_ref(inp, acc), (c, acc))


def test_gemv_pair_mutations():
    """the last four columns of the second input dropped (a wave's K range cut short); an accumulate turned into a store; a bias missing"""
    c = (300, 4, 1028, '')
    inp = RU.linear_sum2_make(c)
    ref, good = RU.linear_sum2_ref(inp, True), RU.linear_sum2_f32(inp, True)
    fails(dict(y=good['y'] - inp['w2'][:, -4:] @ inp['x2'][-4:]), ref, 'y')
    fails(RU.linear_sum2_f32(inp, False), ref, 'y')
    inp = RU.linear2_make((5, 1030, 512))
    ref = RU.linear2_ref(inp, False, True, True, True)
    fails(RU.linear2_f32(inp, False, True, True, False), ref, 'y2')
    fails(RU.linear2_f32(inp, False, False, True, True), ref, 'y2')


# ------------------------------------------------------------------------------------------------------------------ cells
@pytest.mark.parametrize('c', RU.TOPDOWN_FWD, ids=RU.topdown_id)
def test_topdown_cell_fwd_reference(c):
    inp = RU.topdown_fwd_make(c)
    through('topdown_cell_fwd', RU.topdown_fwd_f32(inp, c[2]), RU.topdown_fwd_ref(inp, c[2]), c)


@pytest.mark.parametrize('c', RU.TOPDOWN_BWD, ids=RU.topdown_id)
def test_topdown_cell_bwd_reference(c):
    inp = RU.topdown_bwd_make(c)
    through('topdown_cell_bwd', RU.topdown_bwd_f32(inp, c[2]), RU.topdown_bwd_ref(inp, c[2]), c)


@pytest.mark.parametrize('H', RU.LSTM_CELL_H)
def test_lstm_cell_reference(H):
    inp = RU.lstm_cell_make(H)
    through('lstm_cell_fwd', RU.lstm_cell_fwd_f32(inp), RU.lstm_cell_fwd_ref(inp), H)
    for dc in (False, True):
        through('lstm_cell_bwd', RU.lstm_cell_bwd_f32(inp, dc), RU.lstm_cell_bwd_ref(inp, dc), (H, dc))


def test_cell_mutations():
    """the second segment's last column dropped; add1 missing; the forget and the in gate swapped; dc_in dropped in backward"""
    c = RU.TOPDOWN_FWD[2]
    inp = RU.topdown_fwd_make(c)
    ref = RU.topdown_fwd_ref(inp, c[2])
    short = dict(inp, xs=[inp['xs'][0], np.concatenate([inp['xs'][1][:-1], np.zeros(1, np.float32)])])
    fails(RU.topdown_fwd_f32(short, c[2]), ref, 'act')
    fails(RU.topdown_fwd_f32(inp, dict(c[2], add1=0)), ref, 'act')
    good = RU.topdown_fwd_f32(inp, c[2])
    fails(dict(good, act=good['act'][[1, 0, 2, 3]]), ref, 'act')
    c = RU.TOPDOWN_BWD[3]
    inp = RU.topdown_bwd_make(c)
    fails(RU.topdown_bwd_f32(inp, dict(c[2], dc_in=0)), RU.topdown_bwd_ref(inp, c[2]), 'dc_prev')


# ------------------------------------------------------------------------------------------------------------------ encoder steps
FWD = dict(lstm=(RU.lstm_step_fwd_ref, RU.lstm_step_fwd_f32), gru=(RU.gru_step_fwd_ref, RU.gru_step_fwd_f32), rnn=(RU.rnn_step_fwd_ref, RU.rnn_step_fwd_f32))
BWD = dict(lstm=(RU.lstm_step_bwd_ref, RU.lstm_step_bwd_f32), gru=(RU.gru_step_bwd_ref, RU.gru_step_bwd_f32), rnn=(RU.rnn_step_bwd_ref, RU.rnn_step_bwd_f32))


@pytest.mark.parametrize('kind', ['lstm', 'gru', 'rnn'])
@pytest.mark.parametrize('c', RU.STEP_FWD, ids=RU.step_id)
def test_step_fwd_reference(kind, c):
    ref, f32 = FWD[kind]
    for d in RU.step_fwd_make(kind, c):
        through(kind + '_step_fwd', f32(d), ref(d), c)


@pytest.mark.parametrize('kind', ['lstm', 'gru', 'rnn'])
@pytest.mark.parametrize('c', RU.STEP_BWD, ids=RU.step_id)
def test_step_bwd_reference(kind, c):
    ref, f32 = BWD[kind]
    for d in RU.step_bwd_make(kind, c):
        through(kind + '_step_bwd', f32(d, c[2], c[3]), ref(d, c[2], c[3]), c)


@pytest.mark.parametrize('c', RU.RNN_CONCAT, ids=str)
def test_rnn_concat_reference(c):
    inp = RU.rnn_concat_make(c)
    through('rnn_concat_fwd', RU.rnn_concat_fwd_f32(inp, c[3]), RU.rnn_concat_fwd_ref(inp, c[3]), c)
    through('rnn_concat_bwd', RU.rnn_concat_bwd_f32(inp, c[3], c[4]), RU.rnn_concat_bwd_ref(inp, c[3], c[4]), c)


def test_step_mutations():
    """the two directions swapped; the recurrent bias of one unit missing; the GRU carry dropped; the last quarter of the transposed GEMV
    dropped; dh_ext missing at the first step"""
    a, b = RU.step_fwd_make('lstm', (260, 2))
    fails(RU.lstm_step_fwd_f32(b), RU.lstm_step_fwd_ref(a), 'h')
    nob = dict(a, b=a['b'].copy())
    nob['b'][3 * 260 + 17] = 0
    fails(RU.lstm_step_fwd_f32(nob), RU.lstm_step_fwd_ref(a), 'g_out')
    d = RU.step_bwd_make('gru', (260, 1, True, True))[0]
    ref = RU.gru_step_bwd_ref(d, True, True)
    fails(RU.gru_step_bwd_f32(dict(d, carry_in=np.zeros(260, np.float32)), True, True), ref, 'carry_out')
    short = dict(d, d_next=np.concatenate([d['d_next'][:-4], np.zeros(4, np.float32)]))
    fails(RU.gru_step_bwd_f32(short, True, True), ref, 'dgi')
    d = RU.step_bwd_make('rnn', (8, 1, False, True))[0]
    fails(RU.rnn_step_bwd_f32(d, False, False), RU.rnn_step_bwd_ref(d, False, True), 'dg')
    d = RU.step_bwd_make('lstm', (8, 1, True, True))[0]
    fails(RU.lstm_step_bwd_f32(d, True, False), RU.lstm_step_bwd_ref(d, True, True), 'dg')


# ------------------------------------------------------------------------------------------------------------------ adaptive attention
@pytest.mark.parametrize('c', RU.ADAATT_CELL_FWD, ids=str)
def test_adaatt_cell_fwd_reference(c):
    inp = RU.adaatt_cell_fwd_make(c)
    ref, got = RU.adaatt_cell_fwd_ref(inp, c[1]), RU.adaatt_cell_fwd_f32(inp, c[1])
    if c[1] == 5:
        # an exact tie behind a GEMV is a tie only where both rows are summed in one order (the kernel's wave does; torch's matmul need not)
        got['save'][4, inp['ties']] = 0
        assert inp['dropped'] < 0.01 * c[0] and len(inp['ties']) >= 2
        p = inp['ups'] + inp['downs']
        assert np.array_equal(got['save'][4][p], ref['save']['ref'][4][p])
    through('adaatt_cell_fwd', got, ref, c)


@pytest.mark.parametrize('c', RU.ADAATT_CELL_BWD, ids=str)
def test_adaatt_cell_bwd_reference(c):
    inp = RU.adaatt_cell_bwd_make(c)
    through('adaatt_cell_bwd', RU.adaatt_cell_bwd_f32(inp, c[1], c[4]), RU.adaatt_cell_bwd_ref(inp, c[1], c[4]), c)


@pytest.mark.parametrize('c', RU.ADAATT_ATT, ids=str)
def test_adaatt_attention_references(c):
    inp = RU.adaatt_att_make(c)
    through('adaatt_scores', RU.adaatt_scores_f32(inp, c[3]), RU.adaatt_scores_ref(inp, c[3]), c)
    through('adaatt_apply', RU.adaatt_apply_f32(inp), RU.adaatt_apply_ref(inp), c)
    through('adaatt_bwd_step', RU.adaatt_bwd_step_f32(inp, c[3]), RU.adaatt_bwd_step_ref(inp, c[3]), c)
    through('adaatt_bwd_batched', RU.adaatt_bwd_batched_f32(inp, c[3]), RU.adaatt_bwd_batched_ref(inp, c[3]), c)


def test_adaatt_mutations():
    """the dropout mask forgotten in the scores; the sentinel slot dropped from the weighted sum; the tokens swapped; dfake dropped"""
    c = (3, 10, 8, True)
    inp = RU.adaatt_att_make(c)
    fails(RU.adaatt_scores_f32(inp, False), RU.adaatt_scores_ref(inp, True), 'dots')
    ref, good = RU.adaatt_apply_ref(inp), RU.adaatt_apply_f32(inp)
    fails(dict(good, atten=good['atten'] - good['PI'][:, :1] * inp['frl']), ref, 'atten')
    ref, good = RU.adaatt_bwd_step_ref(inp, True), RU.adaatt_bwd_step_f32(inp, True)
    fails(dict(good, dhoe=good['dhoe'][::-1].copy()), ref, 'dhoe')
    c = RU.ADAATT_CELL_BWD[0]
    inp = RU.adaatt_cell_bwd_make(c)
    fails(RU.adaatt_cell_bwd_f32(inp, 4, (1, 1, 0, 1)), RU.adaatt_cell_bwd_ref(inp, 4, c[4]), 'ds')


# ------------------------------------------------------------------------------------------------------------------ resident recurrence
@pytest.mark.parametrize('c', RU.RECUR, ids=str)
def test_resident_recurrence_references(c):
    """one token from a given state, and the last token's backward from given saved values"""
    inp = RU.recur_make(c)
    for t in sorted({0, c[0] - 1}):
        ref, amb = RU.recur_token_ref(inp, t)
        got = RU.recur_token_f32(inp, t)
        assert amb.sum() < 0.05 * amb.size, 'too many units whose selector is undecided: %d' % amb.sum()
        got['save'][3][amb] = ref['save']['ref'][3][amb]
        through('cap_recur_fwd', got, ref, (c, t))
    through('cap_recur_bwd', RU.recur_bwd_last_f32(inp), RU.recur_bwd_last_ref(inp), c)


def test_resident_recurrence_mutations():
    """the h2att bias missing; the previous token's sums read; one location dropped from P . da2c; the output gradient of another token"""
    c = RU.RECUR[0]
    inp = RU.recur_make(c)
    ref, _ = RU.recur_token_ref(inp, 1)
    fails(RU.recur_token_f32(dict(inp, b_att=0 * inp['b_att']), 1), ref, 'tanh_ws')
    fails(RU.recur_token_f32(dict(inp, b_att=0 * inp['b_att']), 1), ref, 'wgt')
    fails(RU.recur_token_f32(inp, 0), ref, 'c')
    fails(RU.recur_token_f32(dict(inp, b_h2h=0 * inp['b_h2h']), 1), ref, 'h')
    ref = RU.recur_bwd_last_ref(inp)
    P = inp['P'].copy()
    P[7] = 0
    fails(RU.recur_bwd_last_f32(dict(inp, P=P)), ref, 'ddot')
    fails(RU.recur_bwd_last_f32(dict(inp, dho=inp['dho'][::-1].copy())), ref, 'dsums')


def test_worst_ratios_are_reported():
    """(runs last: prints what the float32 forms used of their bounds)"""
    print('worst |got - ref| / bound of the float32 forms: ' + ', '.join('%s %.3g' % kv for kv in sorted(WORST.items())))
    assert all(w <= 1.0 for w in WORST.values())
