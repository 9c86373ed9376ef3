"""The caption branch on rows on the device (csrc/caption_rows.hip, nets/caption_rows.py, model/detect_device.py): each kernel against the
single-mask kernel it restates, Network.caption_decode_rows / caption_score_rows on the reference's own batch runs
(tests/golden/ref_caprows.npz, which tests/test_caprows_cpu.py ties to the numpy restatement), both routes against each other and against
the merged single-mask path, the launch count, the features, and the detection dicts end to end.

Bounds.  masks_to_map, adaptive_pool_rows, the two kernels of the recurrent step and decode_pick_rows: the same bits as the single-mask
launches (a row entry is the single-mask kernel's own body with a row index).  Every log-probability of a whole route and the features:
FWD_TOL = 1e-5 as tests/topdown_util.py's rel_err defines it (the largest difference over the reference's largest magnitude), the project's
bound for these kernels.  Tokens: exact.  `score` is the float32 sum of the returned log-probabilities, added left to right: exact.

Worst values measured on an MI355X (this file's own prints):
  rows step vs the single-row kernels      h and c 0 at every size
  fixture, tokens exact; log-probabilities  vs sample() 2.2e-07 (batched), 2.2e-07 (loop), 2.8e-07 (topdown); vs forward() 1.1e-07, 1.1e-07, 1.3e-07
  rows vs caption_decode per row           1.7e-07 (att2in2), 0 (topdown); production widths 6.8e-08, scores batched vs loop 1.1e-07
  caption_features_rows per mask           0; detect_image's expr_logprob vs caption_score_rows on the same canvases 0"""
import numpy as np
import pytest
import torch

import caprows_util as CU
import decode_util as DU
from topdown_util import rel_err, CAP

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FWD_TOL = 1e-5
L = 196
NEW_ENTRIES = ('l2s_masks_to_map', 'l2s_adaptive_pool_rows', 'l2s_cap_att_dots_rows', 'l2s_cap_apply_gates_rows', 'l2s_decode_pick_rows')


@pytest.fixture(scope='module', autouse=True)
def _restore_cfg():
    """the small-step settings of the feature network (cfg.TRAIN is process-wide) end with this file"""
    import copy
    from lang2seg_amd.model.config import cfg
    train, dtype = copy.deepcopy(dict(cfg.TRAIN)), cfg.COMPUTE_DTYPE
    yield
    for k in list(cfg.TRAIN.keys()):
        if k not in train:
            del cfg.TRAIN[k]
    for k, v in train.items():
        cfg.TRAIN[k] = v
    cfg.COMPUTE_DTYPE = dtype


def ops():
    from lang2seg_amd import ops as O
    return O


def dev(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dt is None else t.to(dt)).to(DEV)


def count_of(n):
    return torch.tensor([n], dtype=torch.int32, device=DEV)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------ 1. masks -> map
@pytest.mark.parametrize('case', [(3, 37, 53, 160, 224, 10, 14), (2, 160, 224, 160, 224, 10, 14)])
def test_masks_to_map_equals_resize_then_downsample(case):
    O = ops()
    rows, mh, mw, H, W, Hc, Wc = case
    rs = np.random.RandomState(mh)
    m = (rs.rand(rows, mh, mw) > 0.5).astype(np.uint8)
    m[0, :mh // 2, :mw // 2] = 1
    m[rows - 1, mh // 3:] = 0
    md = dev(m)
    ref = torch.empty((rows, Hc * Wc), device=DEV)
    big = torch.empty((H, W), dtype=torch.uint8, device=DEV)
    for r in range(rows):
        if (mh, mw) == (H, W):
            O.mask_downsample(md[r], ref[r], H, W, Hc, Wc)
        else:
            O.mask_resize_nearest(md[r], mh, mw, big, H, W)
            O.mask_downsample(big, ref[r], H, W, Hc, Wc)
    got = torch.full((rows, Hc * Wc), 7.0, device=DEV)
    O.masks_to_map(md, rows, mh, mw, H, W, Hc, Wc, got)
    one = torch.full((rows, Hc * Wc), 7.0, device=DEV)
    O.masks_to_map(md, rows, mh, mw, H, W, Hc, Wc, one, count_of(1))
    torch.cuda.synchronize()
    assert same_bits(got, ref) and 0 < float(ref.sum()) < ref.numel()
    assert np.array_equal(ref.cpu().numpy(), CU.masks_to_map(m, H, W, Hc, Wc))
    assert same_bits(one[0], ref[0]) and bool((one[1:] == 7.0).all())


# ------------------------------------------------------------------ 2. pooled rows
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('bins', [(14, 14), (1, 1)])
@pytest.mark.parametrize('hw', [(10, 14), (38, 63)])
@pytest.mark.parametrize('C', [64, 300])
def test_adaptive_pool_rows_equals_adaptive_pool_fwd_per_row(C, hw, bins, dt):
    O = ops()
    (H, W), (OH, OW), rows = hw, bins, 3
    ldy = C + 8
    rs = np.random.RandomState(C + H)
    x = dev(rs.normal(0, 1, (H * W, C)).astype(np.float32), dt)
    pm = dev((rs.rand(rows, H * W) > 0.4).astype(np.float32))
    for m in (None, pm):
        ref = torch.full((rows, OH * OW, ldy), 7.0, dtype=dt, device=DEV)
        for r in range(rows):
            O.adaptive_pool_fwd(x, None if m is None else m[r], ref[r], H, W, C, OH, OW, ldy)
        got = torch.full((rows, OH * OW, ldy), 7.0, dtype=dt, device=DEV)
        O.adaptive_pool_rows(x, m, got, rows, H, W, C, OH, OW, ldy)
        two = torch.full((rows, OH * OW, ldy), 7.0, dtype=dt, device=DEV)
        O.adaptive_pool_rows(x, m, two, rows, H, W, C, OH, OW, ldy, count_of(2))
        torch.cuda.synchronize()
        assert same_bits(got, ref)                                       # (the 7.0 of the columns behind C included: nothing written there)
        assert same_bits(two[:2], ref[:2]) and bool((two[2] == 7.0).all())
        want = CU.adaptive_pool_rows(x.float().cpu().numpy(), None if m is None else m.cpu().numpy(), rows, H, W, OH, OW)
        assert rel_err(got[:, :, :C].float(), want) < (1e-5 if dt == torch.float32 else 8e-3)       # bf16: one rounding of the output, 2^-8


# ------------------------------------------------------------------ 3. the recurrent step on rows
# (R, AH) x rows at the module's L, and the tails: R no multiple of 16 and AH no multiple of 64 with one wave of locations, the fixture's
# 196 and the largest L
STEP_CASES = [pytest.param(RA, rows, L, id='RA%d-%d' % (i, rows)) for i, RA in enumerate([(32, 16), (512, 512)]) for rows in [1, 3, 65]] + \
             [pytest.param((20, 70), 3, nl, id='tails-L%d' % nl) for nl in (5, 196, 256)]


@pytest.mark.parametrize('RA,rows,L', STEP_CASES)
def test_rows_step_equals_the_single_row_kernels(RA, rows, L):
    """the two row kernels, issued in chunks of 64 rows with row0 as the network issues them, against cap_att_dots_fwd + cap_apply_gates_fwd
    row by row on the same inputs: the same kernel bodies (csrc/caption_step.hip), so the same bits"""
    O = ops()
    R, AH = RA
    rs = np.random.RandomState(R + rows)
    g = lambda *shp: dev(rs.normal(0, 1, shp).astype(np.float32))
    patt, att_h, aw, ab = g(rows, L, AH), g(rows, AH), g(AH) * 0.2, g(1)
    P, b, sums, c_prev = g(rows, L, 2 * R), g(2 * R), g(rows, 5 * R), g(rows, R)
    h_ref, c_ref = torch.empty((rows, R), device=DEV), torch.empty((rows, R), device=DEV)
    tanh_ws, dots1, save, wgt = torch.empty((L, AH), device=DEV), torch.empty((256,), device=DEV), torch.empty((6 * R,), device=DEV), torch.empty((L,), device=DEV)
    for r in range(rows):
        O.cap_att_dots_fwd(patt[r], att_h[r], aw, ab, L, AH, tanh_ws, dots1)
        O.cap_apply_gates_fwd(P[r], dots1, b, sums[r], c_prev[r], c_ref[r], h_ref[r], save, wgt, L, R)
    h, c, dots = torch.full((rows, R), 7.0, device=DEV), torch.full((rows, R), 7.0, device=DEV), torch.empty((rows, 256), device=DEV)
    cnt = count_of(rows)
    for r0 in range(0, rows, 64):
        n = min(64, rows - r0)
        O.cap_att_dots_rows(patt[r0:], att_h[r0:], aw, ab, n, L, AH, dots[r0:], cnt, r0)
        O.cap_apply_gates_rows(P[r0:], dots[r0:], b, sums[r0:], c_prev[r0:], c[r0:], h[r0:], n, L, R, cnt, r0)
    dots_last = dots[rows - 1, :L].clone()
    # the rows at or beyond count stay as they are
    h2, c2 = torch.full((rows, R), 7.0, device=DEV), torch.full((rows, R), 7.0, device=DEV)
    O.cap_att_dots_rows(patt, att_h, aw, ab, rows, L, AH, dots, count_of(rows - 1))
    O.cap_apply_gates_rows(P, dots, b, sums, c_prev, c2, h2, rows, L, R, count_of(rows - 1))
    torch.cuda.synchronize()
    eh, ec = rel_err(h, h_ref), rel_err(c, c_ref)
    print('rows step R %d AH %d rows %d L %d vs the single-row kernels: h %.2e c %.2e' % (R, AH, rows, L, eh, ec))
    assert same_bits(h, h_ref) and same_bits(c, c_ref)
    assert same_bits(dots_last, dots1[:L])                             # (dots1: what the single-row kernel left for the last row)
    assert bool((h2[rows - 1] == 7.0).all()) and bool((c2[rows - 1] == 7.0).all()) and (rows == 1 or same_bits(h2[:rows - 1], h_ref[:rows - 1]))


# ------------------------------------------------------------------ 4. the decision per row
def _pick_logits(V1, T=3, rows=5):
    rs = np.random.RandomState(V1)
    x = rs.normal(0, 3, (T, rows, V1)).astype(np.float32)
    hi = max(1, V1 // 2)
    x[:, 0, 0] = x[:, 0].min(-1) - 1.0                               # row 0: never ends
    x[1, 1, hi] = x[1, 1, V1 - 1] = x[1, 1].max() + 1.0              # row 1, t = 1: two equal maxima -> the lower index
    x[0, 1, 0] = x[0, 1].min() - 1.0
    if V1 == 2:
        x[1, 1] = [0.5, 0.5]                                         # (two words: the tie is between 0 and 1 -> 0, which also ends the row)
    x[0, 2, 0] = x[0, 2].max() + 2.0                                 # row 2 ends at t = 0: zeros from there, its neighbours go on
    x[2, 2, V1 - 1] = x[2, 2].max() + 5.0
    return x, hi


@pytest.mark.parametrize('V1', [2, 21, 65, 1025])
def test_decode_pick_rows(V1):
    O = ops()
    T, rows, live = 3, 5, 4
    x, hi = _pick_logits(V1, T, rows)
    xd = dev(x)
    lsm = DU.log_softmax(x)
    mk = lambda: (torch.full((rows,), 9, dtype=torch.int32, device=DEV), torch.full((rows, T), -7, dtype=torch.int64, device=DEV),
                  torch.full((rows, T), -7.0, device=DEV), torch.full((rows,), -7, dtype=torch.int64, device=DEV), torch.full((rows,), -7.0, device=DEV))
    fin, seq, lps, tok, score = mk()
    cnt = count_of(live)
    toks = []
    for t in range(T):
        O.decode_pick_rows(xd[t], V1, rows, t, T, fin, seq, lps, tok, count=cnt, score=score)
        toks.append(tok.clone())
    torch.cuda.synchronize()
    seq_h, lps_h = seq.cpu().numpy(), lps.cpu().numpy()
    scale = np.abs(lsm).max()
    for r in range(live):
        ended = False
        for t in range(T):
            k = 0 if ended else int(np.argmax(x[t, r]))               # np.argmax: the first of equal maxima
            assert seq_h[r, t] == k and int(toks[t][r]) == k, (r, t, seq_h[r], k)
            ref = 0.0 if ended else lsm[t, r, k]
            assert abs(lps_h[r, t] - ref) <= FWD_TOL * max(1.0, scale), (r, t, lps_h[r, t], ref)
            ended = ended or k == 0
        assert int(fin[r]) == int(ended)
    assert seq_h[1, 1] == (hi if V1 > 2 else 0) and (seq_h[2] == 0).all() and (lps_h[2, 1:] == 0).all() and seq_h[0, T - 1] != 0
    s = np.zeros((live,), np.float32)
    for t in range(T):
        s = (s + lps_h[:live, t]).astype(np.float32)
    assert np.array_equal(score.cpu().numpy()[:live], s)
    # the rows at or beyond count: untouched
    assert (seq_h[live:] == -7).all() and (lps_h[live:] == -7.0).all() and int(tok[live]) == -7 and int(fin[live]) == 9 and float(score[live]) == -7.0
    # teacher forcing: the forced token and its log-probability in every live row, finished or not
    fin, seq, lps, tok, score = mk()
    forced = torch.tensor([hi, 0, V1 - 1], dtype=torch.int64, device=DEV)
    for t in range(T):
        O.decode_pick_rows(xd[t], V1, rows, t, T, fin, seq, lps, tok, forced=forced[t:t + 1], count=cnt, score=score)
    torch.cuda.synchronize()
    seq_h, lps_h = seq.cpu().numpy(), lps.cpu().numpy()
    for t, k in enumerate([hi, 0, V1 - 1]):
        assert (seq_h[:live, t] == k).all() and np.abs(lps_h[:live, t] - lsm[t, :live, k]).max() <= FWD_TOL * max(1.0, scale)
    assert (tok.cpu().numpy()[:live] == V1 - 1).all() and (seq_h[live:] == -7).all()


@pytest.mark.parametrize('V1', [2, 21, 65, 1025])
def test_decode_pick_rows_on_one_row_equals_decode_pick(V1):
    """the greedy decision through both entries (csrc/decode.hip: one max / log-sum and one argmax for both), T = 3: row 1 of the logits
    above (a tie: the lower index; with two words it also ends the row), row 2 (ends at t = 0), and row 1 with an all-NaN last step, where
    nothing is a candidate and the pick is word 0.  seq, the log-probabilities, next_token and finished: the same bits after every step"""
    O = ops()
    T = 3
    x, hi = _pick_logits(V1, T)
    nan_last = x[:, 1].copy()
    nan_last[T - 1] = np.nan
    for name, seq_x in (('tie', x[:, 1]), ('early end', x[:, 2]), ('all-NaN step', nan_last)):
        xd = dev(seq_x)
        fin1, seq1, lps1, tok1 = (torch.full((1,), 9, dtype=torch.int32, device=DEV), torch.full((T,), -7, dtype=torch.int64, device=DEV),
                                  torch.full((T,), -7.0, device=DEV), torch.full((1,), -7, dtype=torch.int64, device=DEV))
        finr, seqr, lpsr, tokr = fin1.clone(), seq1.clone().view(1, T), lps1.clone().view(1, T), tok1.clone()
        for t in range(T):
            O.decode_pick(xd[t], V1, t, 1, 1.0, None, None, 0, fin1, seq1, lps1, tok1)
            O.decode_pick_rows(xd[t:t + 1], V1, 1, t, T, finr, seqr, lpsr, tokr)
            torch.cuda.synchronize()
            assert same_bits(seqr[0], seq1) and same_bits(lpsr[0], lps1) and same_bits(tokr, tok1) and same_bits(finr, fin1), (name, t, seq1, seqr, lps1, lpsr)
        s = seq1.cpu().numpy()
        if name == 'tie':
            assert s[1] == (hi if V1 > 2 else 0)
        elif name == 'early end':
            assert (s == 0).all() and int(fin1) == 1 and (lps1.cpu().numpy()[1:] == 0).all()
        elif s[:T - 1].all():                                         # (two words: the tie ended the row before the NaN step)
            assert s[T - 1] == 0 and int(tok1) == 0 and int(fin1) == 1 and bool(torch.isnan(lps1[T - 1]))


# ------------------------------------------------------------------ 5. / 6. the reference's batch runs through a network
_NETS = {}


def _opt(model, fopt):
    from oracle import weights as OW
    opt = OW.default_opt(vocab_size=fopt['vocab_size'], seq_length=fopt['seq_length'])
    opt.update(fopt)
    opt['caption_model'] = model
    return opt


def _fixture_net(model):
    """a ResNet-50 cycle network in f32 whose captioner is the fixture's (as tests/test_decode_gpu.py builds it); cached"""
    if model not in _NETS:
        from lang2seg_amd import selftest
        fopt, w, fc, att, g = CU.fixture(model)
        net = selftest.build_net(_opt(model, fopt), {}, 'f32', None, num_layers=50)
        net.load_state_dict({CAP + k: v for k, v in w.items()})
        net.eval()
        net.parity = None
        _NETS[model] = (net, dev(fc), dev(att))
    return _NETS[model]


def _first0(s):
    s = np.asarray(s)
    return int(np.argmax(s == 0)) if (s == 0).any() else s.size


ROUTES = [('att2in2', True), ('att2in2', False), ('topdown', False)]


@pytest.mark.parametrize('model,batched', ROUTES)
def test_fixture_decode_rows(model, batched):
    """tokens exact; log-probabilities within FWD_TOL of the reference's sample() on the batch; zeros from a row's first 0 on (the 0 itself
    carries its log-probability); with count = 3 the last two rows read as empty sentences"""
    from lang2seg_amd.nets import caption_rows
    net, fc, att = _fixture_net(model)
    g = CU.fixture(model)[4]
    net.rows_batched = batched
    try:
        assert caption_rows.batched(net) == batched
        r = net.caption_decode_rows(att, fc, rows=5)
        seq, lps = r['seq'].cpu().numpy(), r['logprobs'].cpu().numpy()
        r3 = net.caption_decode_rows(att, fc, rows=5, count=count_of(3))
        seq3, lps3 = r3['seq'].cpu().numpy(), r3['logprobs'].cpu().numpy()
    finally:
        net.rows_batched = True
    assert r['seq'].dtype == torch.int64 and tuple(r['seq'].shape) == (5, net.opt['seq_length']) and r['logprobs'].dtype == torch.float32
    assert np.array_equal(seq, g['greedy_seq']), (seq, g['greedy_seq'])
    worst = 0.0
    for k in range(5):
        n = _first0(seq[k])
        if n:
            worst = max(worst, rel_err(lps[k, :n], g['greedy_logprobs'][k, :n]))
        assert (lps[k, n + 1:] == 0).all() and (n == seq.shape[1] or lps[k, n] < 0)
    print('%s rows (%s) vs sample(): %.2e' % (model, 'batched' if batched else 'loop', worst))
    assert worst <= FWD_TOL
    assert np.array_equal(seq3[:3], seq[:3]) and np.array_equal(lps3[:3], lps[:3]) and (seq3[3:] == 0).all() and (lps3[3:] == 0).all()


@pytest.mark.parametrize('model,batched', ROUTES)
def test_fixture_score_rows(model, batched):
    """logprobs within FWD_TOL of the reference's forward() gathered at the targets; score their float32 sum"""
    net, fc, att = _fixture_net(model)
    g = CU.fixture(model)[4]
    forced = [int(v) for v in g['forced']]
    toks, tgt = forced[1:-1], forced[1:]
    ref = g['forward_logprobs'][:, np.arange(len(tgt)), tgt]
    net.rows_batched = batched
    try:
        r = net.caption_score_rows(att, fc, toks, rows=5)
        lps, score = r['logprobs'].cpu().numpy(), r['score'].cpu().numpy()
    finally:
        net.rows_batched = True
    e = rel_err(lps, ref)
    print('%s score rows (%s) vs forward(): %.2e; scores %s' % (model, 'batched' if batched else 'loop', e, score))
    assert lps.shape == (5, len(toks) + 1) and e <= FWD_TOL
    s = np.zeros((5,), np.float32)
    for t in range(lps.shape[1]):
        s = (s + lps[:, t]).astype(np.float32)
    assert np.array_equal(score, s)
    with pytest.raises(ValueError, match='vocab_size'):
        net.caption_score_rows(att, fc, [3, 0, 1], rows=5)
    with pytest.raises(ValueError, match='--sample_max.*--beam_size'):
        net.caption_decode_rows(att, fc, rows=5, beam_size=2)
    with pytest.raises(ValueError, match='--sample_max.*--beam_size'):
        net.caption_decode_rows(att, fc, rows=5, sample_max=0)


@pytest.mark.parametrize('model', CU.MODELS)
def test_rows_equal_the_single_mask_path(model):
    """every fixture row through the merged caption_decode: the same tokens, log-probabilities within FWD_TOL"""
    net, fc, att = _fixture_net(model)
    r = net.caption_decode_rows(att, fc, rows=5)
    seq, lps = r['seq'].cpu().numpy(), r['logprobs'].cpu().numpy()
    worst = 0.0
    for k in range(5):
        one = net.caption_decode(att[k], fc[k])
        n = _first0(seq[k])
        assert one['seq'] == [int(v) for v in seq[k, :n]], (k, one['seq'], seq[k])
        if n:
            worst = max(worst, rel_err(lps[k, :n], np.asarray(one['logprobs'], np.float32)))
    print('%s rows vs caption_decode per row: %.2e' % (model, worst))
    assert worst <= FWD_TOL


# ------------------------------------------------------------------ 7. production widths
_WIDE = {}


def _wide_net(dtype):
    if dtype not in _WIDE:
        from lang2seg_amd import selftest
        from oracle import weights as OW
        opt = OW.default_opt(vocab_size=60, seq_length=5)
        net = selftest.build_net(opt, {}, dtype, OW.make_state_dict(opt, seed=3, head_gain=4.0), num_layers=50)
        net.eval()
        net.parity = None
        rs = np.random.RandomState(7)
        att = np.abs(rs.normal(0, 1, (3, L, opt['att_feat_size']))).astype(np.float32)
        _WIDE[dtype] = (net, dev(att, torch.float32 if dtype == 'f32' else torch.bfloat16))
    return _WIDE[dtype]


def test_production_widths_routes_agree():
    """rnn_size = att_hid_size = input_encoding_size = 512, 3 rows: the batched route, the loop and caption_decode per row"""
    net, att = _wide_net('f32')
    rb = net.caption_decode_rows(att, None, rows=3)
    sb, lb = rb['seq'].cpu().numpy(), rb['logprobs'].cpu().numpy()
    net.rows_batched = False
    try:
        rl = net.caption_decode_rows(att, None, rows=3)
        sl, ll = rl['seq'].cpu().numpy(), rl['logprobs'].cpu().numpy()
    finally:
        net.rows_batched = True
    sc = net.caption_score_rows(att, None, [5, 9, 2], rows=3)['logprobs'].cpu().numpy()
    net.rows_batched = False
    try:
        scl = net.caption_score_rows(att, None, [5, 9, 2], rows=3)['logprobs'].cpu().numpy()
    finally:
        net.rows_batched = True
    worst = rel_err(lb, ll)
    assert np.array_equal(sb, sl), (sb, sl)
    for k in range(3):
        one = net.caption_decode(att[k])
        n = _first0(sb[k])
        assert one['seq'] == [int(v) for v in sb[k, :n]]
        if n:
            worst = max(worst, rel_err(lb[k, :n], np.asarray(one['logprobs'], np.float32)))
    es = rel_err(sc, scl)
    print('production widths: batched vs loop vs caption_decode %.2e; score batched vs loop %.2e; seq %s' % (worst, es, sb.tolist()))
    assert worst <= FWD_TOL and es <= FWD_TOL


def test_production_widths_bf16_outputs_are_finite_and_in_range():
    net, att = _wide_net('bf16')
    V1, T = net.opt['vocab_size'] + 1, net.opt['seq_length']
    r = net.caption_decode_rows(att, None, rows=3)
    seq, lps = r['seq'].cpu().numpy(), r['logprobs'].cpu().numpy()
    s = net.caption_score_rows(att, None, [5, 9, 2], rows=3)
    elp, score = s['logprobs'].cpu().numpy(), s['score'].cpu().numpy()
    assert seq.shape == (3, T) and ((seq >= 0) & (seq < V1)).all()
    assert np.isfinite(lps).all() and (lps <= 0).all() and np.isfinite(elp).all() and (elp < 0).all() and np.isfinite(score).all()


# ------------------------------------------------------------------ 8. launch count
def _calls(fn):
    """the C-ABI entries fn() issues, in order"""
    O = ops()
    names, real = [], O.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)
    O.call = spy
    try:
        fn()
    finally:
        O.call = real
    return names


def test_batched_route_launch_count_does_not_depend_on_count():
    net, fc, att = _fixture_net('att2in2')
    rs = np.random.RandomState(3)
    att65 = dev(rs.normal(0, 1, (65, L, net.opt['att_feat_size'])).astype(np.float32))
    T = net.opt['seq_length']
    net.caption_decode_rows(att65, None, rows=65)                     # (a buffer's first use allocates it zeroed instead of clearing it)
    net.caption_score_rows(att65, None, [3, 7], rows=65)
    a = _calls(lambda: net.caption_decode_rows(att65, None, rows=65, count=count_of(2)))
    s2 = net.caption_decode_rows(att65, None, rows=65, count=count_of(2))['seq'].cpu().numpy().copy()
    b = _calls(lambda: net.caption_decode_rows(att65, None, rows=65, count=count_of(65)))
    r65 = net.caption_decode_rows(att65, None, rows=65, count=count_of(65))
    s65, l65 = r65['seq'].cpu().numpy().copy(), r65['logprobs'].cpu().numpy().copy()
    assert a == b and len(a) > 0
    per_token = sum(1 for n in a if n == 'l2s_decode_pick_rows')
    print('batched route, rows 65 (two chunks): %d C-ABI calls, %d decisions' % (len(a), per_token))
    assert per_token == 2 * T                                        # two chunks, T decisions each: constant in rows within a chunk
    assert np.array_equal(s2[:2], s65[:2]) and (s2[2:] == 0).all() and (l65[:, 0] < 0).all()     # (row 64: the second chunk)
    sa = _calls(lambda: net.caption_score_rows(att65, None, [3, 7], rows=65, count=count_of(2)))
    sb = _calls(lambda: net.caption_score_rows(att65, None, [3, 7], rows=65, count=count_of(65)))
    assert sa == sb and sa.count('l2s_embed_fwd') == 1               # the token-only work once, not per row or per chunk


# ------------------------------------------------------------------ 9. the features
_FEAT = {}


def _feature_net(variant):
    if variant not in _FEAT:
        from lang2seg_amd import selftest
        from oracle import synth as OS
        from topdown_util import td_opt, make_sd
        opt = td_opt(word_drop_out=0.0, rnn_drop_out=0.0)
        over = dict(BATCH_SIZE=16, RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=100, RPN_BATCHSIZE=64)
        net = selftest.build_net(opt, over, 'f32', make_sd(opt, seed=3, variant=variant), num_layers=50, variant=variant)
        blob = OS.make_blob(160, 224, 6, 60, seed=5)
        _FEAT[variant] = (net, blob)
    return _FEAT[variant]


def test_caption_features_rows_equal_caption_features_per_mask():
    O = ops()
    net, blob = _feature_net('cycle')
    net.eval()
    d = net.upload_blob(dict(blob), 0)
    net.forward_test_image(d)
    net.forward_test_sentence(d)
    H, W = 160, 224
    rs = np.random.RandomState(2)
    masks = np.zeros((3, H, W), np.uint8)
    masks[0, 20:90, 30:120] = 1
    masks[1] = rs.rand(H, W) > 0.5
    masks[2, 100:, :] = 1
    small = np.zeros((3, 37, 53), np.uint8)
    small[0, 5:20, 8:30] = 1; small[1, 20:, :] = 1; small[2] = rs.rand(37, 53) > 0.3
    worst = 0.0
    for m, shape in ((masks, (H, W)), (small, (37, 53))):
        md = dev(m)
        att, fc = net.caption_features_rows(md, 3, shape)
        att, fc = att.clone(), fc.clone()
        big = torch.empty((H, W), dtype=torch.uint8, device=DEV)
        for r in range(3):
            if shape != (H, W):
                O.mask_resize_nearest(md[r], shape[0], shape[1], big, H, W)
            a1, f1 = net.caption_features(md[r] if shape == (H, W) else big)
            assert float(a1.abs().max()) > 0
            worst = max(worst, rel_err(att[r], a1), rel_err(fc[r], f1))
    print('caption_features_rows vs caption_features per mask: %.2e' % worst)
    assert worst <= FWD_TOL
    assert tuple(att.shape) == (3, L, net.opt['att_feat_size']) and tuple(fc.shape) == (3, net.opt['fc_feat_size'])


def test_caption_features_rows_reject_the_networks_that_pool_no_mask():
    net, blob = _feature_net('cycle_response')
    net.eval()
    d = net.upload_blob(dict(blob), 0)
    net.forward_test_image(d)
    net.forward_test_sentence(d)
    with pytest.raises(ValueError, match='cycle_response'):
        net.caption_features_rows(torch.zeros((2, 160, 224), dtype=torch.uint8, device=DEV), 2, (160, 224))


# ------------------------------------------------------------------ 10. the detection dicts
def test_detect_image_describes_and_scores_every_detection():
    from lang2seg_amd.model import detect_device as DD
    net, blob = _feature_net('cycle')
    V, T = net.opt['vocab_size'], net.opt['seq_length']
    labels = np.asarray(blob['labels'])
    data = dict(data=blob['data'], im_info=blob['im_info'], file_name='synthetic.jpg')
    words = {str(i): 'w%d' % i for i in range(1, V + 1)}
    plain_calls = _calls(lambda: DD.detect_image(net, dict(data), labels))
    assert not set(plain_calls) & set(NEW_ENTRIES)                    # without the options: none of the new entries
    plain = DD.detect_image(net, dict(data), labels)
    rich = DD.detect_image(net, dict(data), labels, describe=True, expr_score=True, ix_to_word=words)
    assert len(rich) == len(plain) == labels.shape[0] and sum(len(l) for l in plain) > 0
    for i, (lp, lr) in enumerate(zip(plain, rich)):
        n = int((labels[i] != 0).sum())
        assert len(lp) == len(lr)
        for p, q in zip(lp, lr):
            assert {k: q[k] for k in p} == p                            # every existing field keeps its bits
            assert all(1 <= w <= V for w in q['caption_tokens']) and len(q['caption_logprobs']) == len(q['caption_tokens']) <= T
            assert q['caption'] == ' '.join('w%d' % w for w in q['caption_tokens'])
            assert len(q['expr_logprobs']) == n + 1 and all(v < 0 for v in q['expr_logprobs'])
            assert abs(q['expr_logprob'] - float(np.sum(np.asarray(q['expr_logprobs'], np.float64)))) <= 1e-5 * max(1.0, abs(q['expr_logprob']))
    # the last sentence's canvases and TEST forward are still the network's: the score, called directly
    i = labels.shape[0] - 1
    n_det = len(rich[i])
    assert n_det > 0
    cap = DD.default_cap(100)
    _, ih, iw = DD.ED._geometry(np.asarray(blob['im_info'], np.float32).reshape(-1)[:3])
    canvases = net.buf('det.canvases', (cap, ih, iw), torch.uint8)
    att, fc = net.caption_features_rows(canvases, cap, (ih, iw), count=count_of(n_det))
    direct = net.caption_score_rows(att, fc, [int(w) for w in labels[i] if w], rows=cap, count=count_of(n_det))['score'].cpu().numpy()
    e = rel_err(np.asarray([q['expr_logprob'] for q in rich[i]], np.float32), direct[:n_det])
    print('detect_image expr_logprob vs caption_score_rows on the same canvases: %.2e (%d detections)' % (e, n_det))
    assert e <= FWD_TOL and (direct[n_det:] == 0).all()
    # a sentence that reruns with larger buffers reruns its stage
    again = DD.detect_image(net, dict(data), labels, describe=True, expr_score=True, ix_to_word=words, _cap=1)
    assert [len(l) for l in again] == [len(l) for l in rich] and max(len(l) for l in rich) > 1
    for la, lr in zip(again, rich):
        for p, q in zip(la, lr):
            assert p['caption_tokens'] == q['caption_tokens'] and p['segmentation'] == q['segmentation']
            assert rel_err(np.asarray(p['expr_logprobs'], np.float32), np.asarray(q['expr_logprobs'], np.float32)) <= FWD_TOL


class _OneImageLoader(object):
    """getTestBatch over one blob"""

    def __init__(self, blob):
        self.blob, self.split_ix, self.iterators = blob, {'val': [0]}, {'val': 0}

    def getTestBatch(self, split, stride=1):
        return dict(self.blob, bounds=dict(it_pos_now=1, it_max=1, wrapped=True))


def test_eval_split_device_dumps_described_and_scored_detections():
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    from lang2seg_amd.model.eval_device import eval_split_device
    net, _ = _feature_net('cycle')
    b = SyntheticLoader(num_images=1, sents_per_image=2, H=160, W=224, T=6, vocab_size=60, seed=3)._image(0)
    blob = {k: v for k, v in b.items() if k in ('data', 'im_info', 'gt_boxes', 'gt_masks', 'labels', 'file_name')}
    plain, rich = [], []
    res0 = eval_split_device(_OneImageLoader(blob), net, None, 'val', dict(verbose=False), detections=plain)
    res1 = eval_split_device(_OneImageLoader(blob), net, None, 'val', dict(verbose=False), detections=rich, describe=True, expr_score=True)
    assert res0[0] == res1[0] and res0[4:] == res1[4:] and len(plain) == len(rich) > 0        # the metrics do not depend on it
    labels = np.asarray(blob['labels'])
    for p, q in zip(plain, rich):
        assert {k: q[k] for k in p} == p and 'caption' not in q
        assert len(q['caption_logprobs']) == len(q['caption_tokens']) and len(q['expr_logprobs']) == int((labels[q['sent_index']] != 0).sum()) + 1
    with pytest.raises(ValueError, match='--describe.*--dump_detections'):
        eval_split_device(_OneImageLoader(blob), net, None, 'val', dict(verbose=False), describe=True)


# ------------------------------------------------------------------ 11. the predict tool
def test_predict_tool_describes_and_scores_all_detections(capsys):
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    try:
        import predict
    finally:
        sys.path.pop(0)
    common = ['--synthetic', '1', '--allow_init_weights', '1', '--output_postfix', 'no_such_run', '--cfg', '']
    with pytest.raises(ValueError, match='--describe.*--all_detections'):
        predict.main(predict.parse_args(common + ['--describe', '1']))
    with pytest.raises(ValueError, match='--expr_score.*--all_detections'):
        predict.main(predict.parse_args(common + ['--expr_score', '1']))
    capsys.readouterr()
    dets = predict.main(predict.parse_args(common + ['--all_detections', '1', '--describe', '1', '--expr_score', '1', '--max_per_image', '70']))
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(dets) == len(printed) == 3 and sum(len(l) for l in dets) > 0
    for lst, plst in zip(dets, printed):
        for p, q in zip(lst, plst):
            assert all(0 < w <= 1999 for w in p['caption_tokens']) and p['caption'] == ' '.join('w%d' % w for w in p['caption_tokens']) == q['caption']
            assert np.isfinite(p['expr_logprob']) and p['expr_logprob'] < 0 and len(p['expr_logprobs']) >= 2 and q['expr_logprob'] == p['expr_logprob']
