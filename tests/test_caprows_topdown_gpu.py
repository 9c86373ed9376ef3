"""The top-down captioner on the batched route of the caption branch on rows, on the device (csrc/caption_rows.hip l2s_lstm_cell_rows and
csrc/caption_step.hip l2s_cap_att_apply_rows; nets/captioners.py TopDown.rows_*; nets/caption_rows.py): each kernel against its float64 restatement
(tests/caprows_topdown_util.py) and against the single-row kernel row by row, the dead rows, the reference's own batch runs
(tests/golden/ref_caprows.npz, topdown/*) through the network of tests/test_caprows_gpu.py, the production widths, the launch count and the
detection dicts end to end.

Bounds.  The kernels, every log-probability and every score: FWD_TOL = 1e-5 as tests/topdown_util.py's rel_err defines it (the largest
difference over the reference's largest magnitude), the project's bound for these kernels; the single-row cell is held to the same, and
l2s_cap_att_apply_rows to the bits of l2s_cap_att_apply_fwd, whose kernel body it instantiates.  The
cell's weights are drawn as nn.LSTMCell draws them (uniform in +-1 / sqrt(R)), so that the gates are of order 1 as a trained cell's are.
Tokens: exact.  `score`: the float32 sum of the returned log-probabilities, added left to right: exact.  Dead rows: every byte unchanged.

Worst values measured on an MI355X (this file's own prints):
  l2s_lstm_cell_rows      vs float64 h 3.5e-07, c 1.4e-07; vs l2s_topdown_cell_fwd row by row h 3.8e-07, c 1.8e-07 (another summation order;
                          that cell itself is 1.5e-07 from float64)
  l2s_cap_att_apply_rows  vs float64 3.6e-07; vs l2s_cap_att_apply_fwd per row 0: the same bits at every size
  dead rows               every byte unchanged; the live rows vs float64 2.8e-07
  fixture, tokens exact   vs sample() 1.9e-07, vs forward() 1.3e-07, batched vs loop 1.9e-07 (decode), 1.3e-07 (score)
  production widths       batched vs loop vs caption_decode 1.2e-07, scores batched vs loop 1.1e-07; five non-zero tokens in every row
  launch count            9 entries a token decoding, 7 scoring; 122 entries for 65 rows (two chunks) at seq_length 6
  detect_image            expr_logprob vs caption_score_rows on the same canvases 0 (100 detections)"""
import numpy as np
import pytest
import torch

import caprows_topdown_util as TU
import caprows_util as CU
from topdown_util import rel_err, td_opt, make_sd, CAP
from test_caprows_gpu import _restore_cfg, _fixture_net, _feature_net, _calls, _first0, dev, count_of, same_bits, ops      # noqa: F401

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FWD_TOL = 1e-5
L = 196
ROWS_ENTRIES = ('l2s_lstm_cell_rows', 'l2s_cap_att_apply_rows', 'l2s_cap_att_dots_rows', 'l2s_decode_pick_rows')
SINGLE_ROW = ('l2s_topdown_cell_fwd', 'l2s_cap_att_dots_fwd', 'l2s_cap_att_apply_fwd')


# ------------------------------------------------------------------ 1. the cell on rows
def _cell_case(R, IE, rows, seed):
    """both cells of one token at (R, IE): the operands on the host, laid out as the route lays them out"""
    rs = np.random.RandomState(seed)
    k = 1.0 / np.sqrt(R)
    u = lambda *shp: rs.uniform(-k, k, shp).astype(np.float32)
    g = lambda *shp: rs.normal(0, 1, shp).astype(np.float32)
    Ka = IE + 2 * R
    return dict(R=R, Ka=Ka, rows=rows, wa_ih=u(4 * R, Ka), wa_hh=u(4 * R, R), wl_ih=u(4 * R, 2 * R), wl_hh=u(4 * R, R), b0=u(4 * R), b1=u(4 * R),
                pre=g(rows, 4 * R), fcrow=g(rows, 4 * R), hl=g(rows, R) * 0.5, lin0=g(rows, 2 * R) * 0.5, lin1=g(rows, 2 * R) * 0.5,
                ca=g(rows, R), cl=g(rows, R))


def _att_cell(O, d, c, out, count=None, row0=0):
    """the attention cell's launch: `pre` per row + fcrow per row, segments hl and the h_att half of lin0; h into the second half of
    out [rows][2R]"""
    R, Ka, rows = d['R'], d['Ka'], d['rows']
    O.lstm_cell_rows(d['pre'], None, None, [(d['hl'], R, d['wa_ih'], Ka, R), (d['lin0'].view(-1)[R:], 2 * R, d['wa_hh'], R, R)], d['ca'], c,
                     out.view(-1)[R:], rows, R, count, row0, pre2=d['fcrow'], ld_h=2 * R)


def _lang_cell(O, d, c, h, count=None, row0=0):
    """the language cell's launch: one `pre` row for all rows (ld_pre = 0), add0 / add1, segments lin1 (2R wide) and hl"""
    R, rows = d['R'], d['rows']
    O.lstm_cell_rows(d['pre'], d['b0'], d['b1'], [(d['lin1'], 2 * R, d['wl_ih'], 2 * R, 2 * R), (d['hl'], R, d['wl_hh'], R, R)], d['cl'], c, h,
                     rows, R, count, row0, ld_pre=0)


def _cells_f64(h):
    R = h['R']
    att = TU.lstm_cell_rows(h['pre'], h['fcrow'], None, None, [(h['hl'], h['wa_ih'][:, :R]), (h['lin0'][:, R:], h['wa_hh'])], h['ca'])
    lang = TU.lstm_cell_rows(h['pre'][0], None, h['b0'], h['b1'], [(h['lin1'], h['wl_ih']), (h['hl'], h['wl_hh'])], h['cl'])
    return att, lang


CELL_SHAPES = [(R, IE, rows) for R, IE in ((32, 12), (20, 10), (512, 512)) for rows in (1, 3, 17, 65) if rows < 65 or R < 512]


@pytest.mark.parametrize('R,IE,rows', CELL_SHAPES)
def test_lstm_cell_rows_against_float64_and_the_single_row_cell(R, IE, rows):
    """(20, 10): the attention cell's leading dimension is 50, the scalar loads; 17 rows cross a 16-row tile, 65 a 32-row tile twice"""
    O = ops()
    hst = _cell_case(R, IE, rows, 100 * R + rows)
    d = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in hst.items()}
    (ca64, ha64), (cl64, hl64) = _cells_f64(hst)
    Ka = d['Ka']
    new = lambda *shp: torch.full(shp, 7.0, device=DEV)
    ca, lin, cl, hl = new(rows, R), new(rows, 2 * R), new(rows, R), new(rows, R)
    _att_cell(O, d, ca, lin)
    _lang_cell(O, d, cl, hl)
    # the single-row cell, row by row on the same operands
    ca1, ha1, cl1, hl1, act = new(rows, R), new(rows, R), new(rows, R), new(rows, R), new(4 * R)
    for r in range(rows):
        O.topdown_cell_fwd(d['pre'][r], d['fcrow'][r], None, [(d['hl'][r], d['wa_ih'], Ka, R), (d['lin0'][r][R:], d['wa_hh'], R, R)], d['ca'][r],
                           ca1[r], ha1[r], act, R)
        O.topdown_cell_fwd(d['pre'][0], d['b0'], d['b1'], [(d['lin1'][r], d['wl_ih'], 2 * R, 2 * R), (d['hl'][r], d['wl_hh'], R, R)], d['cl'][r],
                           cl1[r], hl1[r], act, R)
    torch.cuda.synchronize()
    ha = lin[:, R:]
    e64 = [rel_err(ha, ha64), rel_err(ca, ca64), rel_err(hl, hl64), rel_err(cl, cl64)]
    e1 = [rel_err(ha, ha1), rel_err(ca, ca1), rel_err(hl, hl1), rel_err(cl, cl1)]
    s64 = [rel_err(ha1, ha64), rel_err(ca1, ca64), rel_err(hl1, hl64), rel_err(cl1, cl64)]
    print('lstm_cell_rows R %d IE %d rows %d: vs float64 h %.2e c %.2e; vs the single-row cell h %.2e c %.2e (that cell vs float64 %.2e)'
          % (R, IE, rows, max(e64[0], e64[2]), max(e64[1], e64[3]), max(e1[0], e1[2]), max(e1[1], e1[3]), max(s64)))
    assert max(e64) <= FWD_TOL and max(e1) <= FWD_TOL
    assert bool((lin[:, :R] == 7.0).all())                            # the att_res half of the row is the attention's, not the cell's


# ------------------------------------------------------------------ 2. the attention's second half on rows
@pytest.mark.parametrize('rows', [1, 3, 65])
@pytest.mark.parametrize('R', [20, 32, 512])
def test_cap_att_apply_rows_against_the_single_row_kernel_and_float64(R, rows):
    O = ops()
    rs = np.random.RandomState(R + rows)
    att, dots = rs.normal(0, 1, (rows, L, R)).astype(np.float32), rs.normal(0, 2, (rows, 256)).astype(np.float32)
    ad, dd = dev(att), dev(dots)
    got = torch.full((rows, 2 * R), 7.0, device=DEV)
    O.cap_att_apply_rows(ad, dd, got, rows, L, R, ld_res=2 * R)
    ref, wgt = torch.empty((rows, R), device=DEV), torch.empty((L,), device=DEV)
    for r in range(rows):
        O.cap_att_apply_fwd(ad[r], dd[r], L, R, wgt, ref[r])
    torch.cuda.synchronize()
    e64, e1 = rel_err(got[:, :R], TU.att_apply_rows(att, dots[:, :L])), rel_err(got[:, :R], ref)
    print('cap_att_apply_rows R %d rows %d: vs float64 %.2e; vs the single-row kernel %.2e' % (R, rows, e64, e1))
    assert e64 <= FWD_TOL and same_bits(got[:, :R], ref)              # (the single-row kernel's own body: csrc/caption_step.hip)
    assert bool((got[:, R:] == 7.0).all())


# ------------------------------------------------------------------ 3. dead rows
def _sentinel(*shp):
    n = int(np.prod(shp))
    return (torch.arange(n, device=DEV, dtype=torch.float32) * 0.37 + 3.0).view(*shp)


@pytest.mark.parametrize('row0,count,live', [(0, 2, 2), (64, 65, 1)])
@pytest.mark.parametrize('R,IE', [(32, 12), (20, 10)])
def test_dead_rows_are_neither_read_nor_written(R, IE, row0, count, live):
    """5 rows of which `live` are live; the dead rows' inputs are NaN, every output array holds a sentinel pattern beforehand"""
    O = ops()
    rows = 5
    hst = _cell_case(R, IE, rows, 7 * R + row0)
    for k in ('pre', 'fcrow', 'hl', 'lin0', 'lin1', 'ca', 'cl'):
        hst[k][live:] = np.nan
    hst['pre'][0] = 0.25                                              # (the language cell's one row for all rows: live)
    d = {k: (dev(v) if isinstance(v, np.ndarray) else v) for k, v in hst.items()}
    ok = {k: (v[:live] if isinstance(v, np.ndarray) and v.shape[0] == rows and k not in ('b0', 'b1') else v) for k, v in hst.items()}
    (ca64, ha64), (cl64, hl64) = _cells_f64(ok)
    cnt = count_of(count)
    ca, lin, cl, hl = _sentinel(rows, R), _sentinel(rows, 2 * R), _sentinel(rows, R), _sentinel(rows, R)
    before = [t.clone() for t in (ca, lin, cl, hl)]
    _att_cell(O, d, ca, lin, cnt, row0)
    _lang_cell(O, d, cl, hl, cnt, row0)
    rs = np.random.RandomState(R)
    att, dots = rs.normal(0, 1, (rows, L, R)).astype(np.float32), rs.normal(0, 2, (rows, 256)).astype(np.float32)
    att[live:] = np.nan; dots[live:] = np.nan
    res = _sentinel(rows, 2 * R)
    res0 = res.clone()
    O.cap_att_apply_rows(dev(att), dev(dots), res, rows, L, R, cnt, row0, ld_res=2 * R)
    torch.cuda.synchronize()
    for got, was in zip((ca, lin, cl, hl, res), before + [res0]):
        assert same_bits(got[live:].contiguous(), was[live:].contiguous())
    assert same_bits(lin[:, :R].contiguous(), before[1][:, :R].contiguous()) and same_bits(res[:, R:].contiguous(), res0[:, R:].contiguous())
    errs = [rel_err(lin[:live, R:], ha64), rel_err(ca[:live], ca64), rel_err(hl[:live], hl64), rel_err(cl[:live], cl64),
            rel_err(res[:live, :R], TU.att_apply_rows(att[:live], dots[:live, :L]))]
    print('dead rows R %d row0 %d count %d: live rows vs float64 %.2e' % (R, row0, count, max(errs)))
    assert max(errs) <= FWD_TOL


# ------------------------------------------------------------------ 4. the reference's batch runs
def _both_routes(net, fn):
    from lang2seg_amd.nets import caption_rows
    assert caption_rows.batched(net)
    a = fn()
    a = {k: v.cpu().numpy().copy() for k, v in a.items()}
    net.rows_batched = False
    try:
        assert not caption_rows.batched(net)
        b = fn()
        b = {k: v.cpu().numpy().copy() for k, v in b.items()}
    finally:
        net.rows_batched = True
    return a, b


def test_fixture_on_the_batched_route():
    net, fc, att = _fixture_net('topdown')
    g = CU.fixture('topdown')[4]
    names = _calls(lambda: net.caption_decode_rows(att, fc, rows=5))
    assert 'l2s_lstm_cell_rows' in names and not set(names) & set(SINGLE_ROW)
    rb, rl = _both_routes(net, lambda: net.caption_decode_rows(att, fc, rows=5))
    seq, lps = rb['seq'], rb['logprobs']
    assert np.array_equal(seq, g['greedy_seq']), (seq, g['greedy_seq'])
    assert np.array_equal(seq, rl['seq'])
    worst = 0.0
    for k in range(5):
        n = _first0(seq[k])
        if n:
            worst = max(worst, rel_err(lps[k, :n], g['greedy_logprobs'][k, :n]))
        assert (lps[k, n + 1:] == 0).all() and (n == seq.shape[1] or lps[k, n] < 0)
    e_routes = rel_err(lps, rl['logprobs'])
    r3 = net.caption_decode_rows(att, fc, rows=5, count=count_of(3))
    seq3, lps3 = r3['seq'].cpu().numpy(), r3['logprobs'].cpu().numpy()
    assert np.array_equal(seq3[:3], seq[:3]) and np.array_equal(lps3[:3], lps[:3]) and (seq3[3:] == 0).all() and (lps3[3:] == 0).all()
    # the score: teacher-forced, against the reference's forward() gathered at the targets
    forced = [int(v) for v in g['forced']]
    toks, tgt = forced[1:-1], forced[1:]
    ref = g['forward_logprobs'][:, np.arange(len(tgt)), tgt]
    sb, sl = _both_routes(net, lambda: net.caption_score_rows(att, fc, toks, rows=5))
    e_fwd, e_score = rel_err(sb['logprobs'], ref), rel_err(sb['logprobs'], sl['logprobs'])
    print('topdown rows (batched) vs sample(): %.2e; vs forward(): %.2e; batched vs loop: decode %.2e, score %.2e' % (worst, e_fwd, e_routes, e_score))
    assert worst <= FWD_TOL and e_routes <= FWD_TOL and e_fwd <= FWD_TOL and e_score <= FWD_TOL
    s = np.zeros((5,), np.float32)
    for t in range(sb['logprobs'].shape[1]):
        s = (s + sb['logprobs'][:, t]).astype(np.float32)
    assert np.array_equal(sb['score'], s)
    s3 = net.caption_score_rows(att, fc, toks, rows=5, count=count_of(3))
    assert np.array_equal(s3['score'].cpu().numpy()[:3], s[:3]) and bool((s3['score'][3:] == 0).all()) and bool((s3['logprobs'][3:] == 0).all())


# ------------------------------------------------------------------ 5. production widths
_WIDE = {}


def _wide_net(dtype):
    """rnn_size = att_hid_size = input_encoding_size = 512, 3 rows.  The seeded captioner's logit layer is scaled by 4 (the head gain of
    the att2in2 network of tests/test_caprows_gpu.py): with captioner seed 13 the float64 TopDownRef then decodes five non-zero tokens in
    every row - [47 47 47 47 47], the same, [47 47 47 15 15] - and its smallest gap between the two best words is 7.5e-3, four
    orders above FWD_TOL, so the greedy tokens of two correct routes cannot differ"""
    if dtype not in _WIDE:
        from lang2seg_amd import selftest
        opt = td_opt(vocab_size=60, seq_length=5)
        sd = make_sd(opt, seed=3, head_gain=4.0, cap_seed=13)
        sd[CAP + 'logit.weight'] = sd[CAP + 'logit.weight'] * np.float32(4.0)
        net = selftest.build_net(opt, {}, dtype, sd, num_layers=50)
        net.eval()
        net.parity = None
        rs = np.random.RandomState(7)
        att = np.abs(rs.normal(0, 1, (3, L, opt['att_feat_size']))).astype(np.float32)
        fc = np.abs(rs.normal(0, 1, (3, opt['fc_feat_size']))).astype(np.float32)
        dt = torch.float32 if dtype == 'f32' else torch.bfloat16
        _WIDE[dtype] = (net, dev(att, dt), dev(fc, dt))
    return _WIDE[dtype]


def test_production_widths_routes_agree():
    net, att, fc = _wide_net('f32')
    assert net.opt['rnn_size'] == net.opt['input_encoding_size'] == net.opt['att_hid_size'] == 512
    rb, rl = _both_routes(net, lambda: net.caption_decode_rows(att, fc, rows=3))
    sb, sl = _both_routes(net, lambda: net.caption_score_rows(att, fc, [5, 9, 2], rows=3))
    assert np.array_equal(rb['seq'], rl['seq']) and (rb['seq'] != 0).all(), (rb['seq'], rl['seq'])      # five steps of both cells in every row
    worst = rel_err(rb['logprobs'], rl['logprobs'])
    for k in range(3):
        one = net.caption_decode(att[k], fc[k])
        n = _first0(rb['seq'][k])
        assert one['seq'] == [int(v) for v in rb['seq'][k, :n]]
        if n:
            worst = max(worst, rel_err(rb['logprobs'][k, :n], np.asarray(one['logprobs'], np.float32)))
    es = rel_err(sb['logprobs'], sl['logprobs'])
    print('topdown production widths: batched vs loop vs caption_decode %.2e; score batched vs loop %.2e; seq %s' % (worst, es, rb['seq'].tolist()))
    assert worst <= FWD_TOL and es <= FWD_TOL


def test_production_widths_bf16_outputs_are_finite_and_in_range():
    from lang2seg_amd.nets import caption_rows
    net, att, fc = _wide_net('bf16')
    assert caption_rows.batched(net)
    V1, T = net.opt['vocab_size'] + 1, net.opt['seq_length']
    r = net.caption_decode_rows(att, fc, rows=3)
    seq, lps = r['seq'].cpu().numpy(), r['logprobs'].cpu().numpy()
    s = net.caption_score_rows(att, fc, [5, 9, 2], rows=3)
    elp, score = s['logprobs'].cpu().numpy(), s['score'].cpu().numpy()
    assert seq.shape == (3, T) and ((seq >= 0) & (seq < V1)).all()
    assert np.isfinite(lps).all() and (lps <= 0).all() and np.isfinite(elp).all() and (elp < 0).all() and np.isfinite(score).all()


# ------------------------------------------------------------------ 6. launch count
def _per_token(names, T):
    """the entries between one decision and the next inside a chunk (the decision included)"""
    at = [i for i, n in enumerate(names) if n == 'l2s_decode_pick_rows']
    return [at[k] - at[k - 1] for k in range(1, len(at)) if k % T]


def test_batched_route_launch_count_does_not_depend_on_count():
    net, fc, att = _fixture_net('topdown')
    rs = np.random.RandomState(3)
    att65 = dev(rs.normal(0, 1, (65, L, net.opt['att_feat_size'])).astype(np.float32))
    fc65 = dev(rs.normal(0, 1, (65, net.opt['fc_feat_size'])).astype(np.float32))
    T = net.opt['seq_length']
    net.caption_decode_rows(att65, fc65, rows=65)                     # (a buffer's first use allocates it zeroed instead of clearing it)
    net.caption_score_rows(att65, fc65, [3, 7], rows=65)
    a = _calls(lambda: net.caption_decode_rows(att65, fc65, rows=65, count=count_of(2)))
    s2 = net.caption_decode_rows(att65, fc65, rows=65, count=count_of(2))['seq'].cpu().numpy().copy()
    b = _calls(lambda: net.caption_decode_rows(att65, fc65, rows=65, count=count_of(65)))
    r65 = net.caption_decode_rows(att65, fc65, rows=65, count=count_of(65))
    s65, l65 = r65['seq'].cpu().numpy().copy(), r65['logprobs'].cpu().numpy().copy()
    assert a == b and len(a) > 0
    assert a.count('l2s_decode_pick_rows') == 2 * T                   # two chunks, T decisions each
    assert not set(a) & set(SINGLE_ROW) and set(ROWS_ENTRIES) <= set(a)
    per = _per_token(a, T)
    print('topdown batched route, rows 65 (two chunks): %d C-ABI calls, %s a token' % (len(a), sorted(set(per))))
    assert len(per) == 2 * (T - 1) and max(per) <= 9
    assert np.array_equal(s2[:2], s65[:2]) and (s2[2:] == 0).all() and (l65[:, 0] < 0).all()     # (row 64: the second chunk)
    sa = _calls(lambda: net.caption_score_rows(att65, fc65, [3, 7], rows=65, count=count_of(2)))
    sb = _calls(lambda: net.caption_score_rows(att65, fc65, [3, 7], rows=65, count=count_of(65)))
    assert sa == sb and sa.count('l2s_embed_fwd') == 1 and sa.count('l2s_decode_pick_rows') == 2 * 3
    assert not set(sa) & set(SINGLE_ROW) and max(_per_token(sa, 3)) <= 7


# ------------------------------------------------------------------ 7. the detection dicts
def test_detect_image_describes_and_scores_on_the_batched_route():
    from lang2seg_amd.model import detect_device as DD
    from lang2seg_amd.nets import caption_rows
    net, blob = _feature_net('cycle')
    assert net.cap_model == 'topdown' and caption_rows.batched(net)
    V = net.opt['vocab_size']
    labels = np.asarray(blob['labels'])
    data = dict(data=blob['data'], im_info=blob['im_info'], file_name='synthetic.jpg')
    words = {str(i): 'w%d' % i for i in range(1, V + 1)}
    plain = DD.detect_image(net, dict(data), labels)
    names = _calls(lambda: DD.detect_image(net, dict(data), labels, describe=True, expr_score=True, ix_to_word=words))
    rich = DD.detect_image(net, dict(data), labels, describe=True, expr_score=True, ix_to_word=words)
    assert set(ROWS_ENTRIES) <= set(names) and not set(names) & set(SINGLE_ROW)
    assert len(rich) == len(plain) == labels.shape[0] and sum(len(l) for l in plain) > 0
    for lp, lr in zip(plain, rich):
        assert len(lp) == len(lr)
        for p, q in zip(lp, lr):
            assert {k: q[k] for k in p} == p                            # every existing field keeps its bits
    i = labels.shape[0] - 1
    n_det = len(rich[i])
    assert n_det > 0
    cap = DD.default_cap(100)
    _, ih, iw = DD.ED._geometry(np.asarray(blob['im_info'], np.float32).reshape(-1)[:3])
    canvases = net.buf('det.canvases', (cap, ih, iw), torch.uint8)
    att, fc = net.caption_features_rows(canvases, cap, (ih, iw), count=count_of(n_det))
    direct = net.caption_score_rows(att, fc, [int(w) for w in labels[i] if w], rows=cap, count=count_of(n_det))['score'].cpu().numpy()
    e = rel_err(np.asarray([q['expr_logprob'] for q in rich[i]], np.float32), direct[:n_det])
    print('topdown detect_image expr_logprob vs caption_score_rows on the same canvases: %.2e (%d detections)' % (e, n_det))
    assert e <= FWD_TOL and (direct[n_det:] == 0).all()
