"""The speaker's evaluation on the device: l2s_decode_force_rows alone against tests/caption_eval_util.py's float64 restatement,
Network.caption_score_pairs on both routes against the float64 drivers (tests/decode_util.py RefDriver, one per row), and
eval_split_device(caption_eval=True) on the synthetic split of the device-evaluation tests.

Bounds.  The kernel: elementwise |got - ref| <= FWD_TOL * max(1, max |ref|), what tests/test_caprows_gpu.py applies to the forced
log-probabilities of l2s_decode_pick_rows (caption_eval_util.check_close restates it), and the same bits as that kernel's forced branch
on the same logits and token.  caption_score_pairs in f32: rel_err <= FWD_TOL = 1e-5 against the float64 driver, the bound of the
caption_score_rows tests; on a bf16 network those tests ask for finite, negative values only (the features and att_embed are bf16), and so
does this file, plus FWD_TOL against caption_score_rows on the same network.  `score` is the float32 sum of the row's log-probabilities
added left to right: exact.

caption_score_pairs against caption_score_rows with one expression in every row is asserted WITHIN FWD_TOL, not bit for bit: the pairs
route drives the token step the greedy way (embedding and the input product per step on `rows` rows), caption_score_rows computes them
once for the n + 1 inputs and adds the recurrent bias in another launch, so the sums are rounded in another order.

Row independence is asserted bit for bit among chunks of two or more rows; a one-row chunk takes the single-row (GEMV) linear kernels,
whose order of summation differs, and is held to FWD_TOL."""
import numpy as np
import pytest
import torch

import caprows_util as CU
import caption_eval_util as EU
import decode_util as DU
from topdown_util import rel_err, CAP

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FWD_TOL = EU.FWD_TOL
L = 196


@pytest.fixture(scope='module', autouse=True)
def _restore_cfg():
    """the small-step settings of the networks (cfg.TRAIN, cfg.COMPUTE_DTYPE are process-wide) end with this file"""
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


def _calls(fn):
    """the C-ABI entries fn() issues, in order (as tests/test_caprows_gpu.py counts them)"""
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


# ------------------------------------------------------------------ 1. the kernel alone
GUARD = np.float32(1e30)
T_K = 4


def _kernel_case(V1, rows):
    """logits [T][rows + 2][ld] between guard rows and guard columns of 1e30 (a read outside a row's V1 values ruins its maximum), targets
    with lengths that run through 1 .. T (1 and T included), a row whose target is the last word"""
    rs = np.random.RandomState(V1 * 7 + rows)
    ld = V1 + 3
    x = np.full((T_K, rows + 2, ld), GUARD, np.float32)
    x[:, 1:rows + 1, :V1] = rs.normal(0, 3, (T_K, rows, V1)).astype(np.float32)
    ntok = np.asarray([(1, T_K, 2, 3)[r % 4] for r in range(rows)], np.int64)
    tgt = np.zeros((rows, T_K), np.int64)
    for r in range(rows):
        tgt[r, :ntok[r] - 1] = rs.randint(1, V1, ntok[r] - 1)
    if rows > 1:
        tgt[1, 0] = V1 - 1
    return x, ld, tgt, ntok


def _run_kernel(xd, ld, V1, rows, tgt_d, ntok_d, count=None, row0=0):
    """all T launches on outputs between sentinels -> (logprobs [rows + 2][T], score [rows + 2], next_token [rows + 2], the next tokens per step)"""
    O = ops()
    lps = torch.full((rows + 2, T_K), -7.0, device=DEV)
    score = torch.full((rows + 2,), -7.0, device=DEV)
    tok = torch.full((rows + 2,), -7, dtype=torch.int64, device=DEV)
    steps = []
    for t in range(T_K):
        O.decode_force_rows(xd[t, 1:], V1, rows, t, T_K, tgt_d, ntok_d, lps[1:], tok[1:], count, row0, ld_logits=ld, score=score[1:])
        assert O.last_kernel() == 'decode_force_rows_kernel'
        steps.append(tok.clone())
    torch.cuda.synchronize()
    return lps.cpu().numpy(), score.cpu().numpy(), tok.cpu().numpy(), torch.stack(steps).cpu().numpy()


@pytest.mark.parametrize('rows', [1, 5, 65])
@pytest.mark.parametrize('V1', [37, 64, 65, 2000])
def test_decode_force_rows_against_float64(V1, rows):
    x, ld, tgt, ntok = _kernel_case(V1, rows)
    xd, tgt_d, ntok_d = dev(x), dev(tgt), dev(ntok.astype(np.int32))
    ref, ref_score, ref_steps = EU.force_rows(x[:, 1:rows + 1, :V1].astype(np.float64), tgt, ntok)
    inside = np.arange(T_K)[None, :] < ntok[:, None]
    worst = 0.0
    for count, row0 in [(None, 0), (0, 0), (3, 0), (rows, 0), (rows + 2, 2), (4, 2)]:
        live = rows if count is None else max(0, min(rows, count - row0))
        lps, score, tok, steps = _run_kernel(xd, ld, V1, rows, tgt_d, ntok_d, None if count is None else count_of(count), row0)
        got, m = lps[1:rows + 1], inside[:live]
        # the guards, the positions behind a row's length and every row at or beyond count keep their sentinels
        assert (lps[0] == -7.0).all() and (lps[rows + 1] == -7.0).all() and score[0] == score[rows + 1] == -7.0 and tok[0] == tok[rows + 1] == -7
        assert (got[:live][~m] == -7.0).all() and (got[live:] == -7.0).all() and (score[1 + live:] == -7.0).all() and (steps[:, 1 + live:] == -7).all()
        if live:
            worst = max(worst, EU.check_close(np.where(m, got[:live], 0.0), np.where(m, ref[:live], 0.0)))
            EU.check_close(score[1:1 + live], ref_score[:live], 'score')
            s = np.zeros((live,), np.float32)                              # the sum: float32, left to right, exact
            for t in range(T_K):
                s = np.where(m[:, t], (s + got[:live, t]).astype(np.float32), s)
            assert np.array_equal(score[1:1 + live], s)
            assert np.array_equal(steps[:, 1:1 + live], ref_steps[:, :live])      # the next input: the target inside the length, then 0
    print('decode_force_rows V1 %d rows %d: worst |lp - float64| %.2e' % (V1, rows, worst))
    assert rows == 1 or int(_run_kernel(xd, ld, V1, rows, tgt_d, ntok_d)[3][0, 2]) == V1 - 1


@pytest.mark.parametrize('V1', [37, 64, 65, 2000])
def test_decode_force_rows_equals_the_forced_branch_of_decode_pick_rows(V1):
    """the same logits through both kernels, the rows whose own target is the one forced token: the same bits (csrc/decode.hip: one
    max / log-sum, one clamp and one log-probability expression for both)"""
    O = ops()
    rows = 5
    x, ld, tgt, ntok = _kernel_case(V1, rows)
    ntok[:] = T_K
    forced = np.asarray([3, V1 - 1, 1, 0], np.int64)
    tgt[0], tgt[3] = forced, forced                                        # rows 0 and 3 are forced to the same tokens as the pick kernel's rows
    xd, tgt_d, ntok_d, forced_d = dev(x), dev(tgt), dev(ntok.astype(np.int32)), dev(forced)
    lps, score, tok = torch.zeros((rows, T_K), device=DEV), torch.zeros((rows,), device=DEV), torch.zeros((rows,), dtype=torch.int64, device=DEV)
    fin, seq = torch.zeros((rows,), dtype=torch.int32, device=DEV), torch.zeros((rows, T_K), dtype=torch.int64, device=DEV)
    lps2, score2, tok2 = torch.zeros_like(lps), torch.zeros_like(score), torch.zeros_like(tok)
    for t in range(T_K):
        O.decode_force_rows(xd[t, 1:], V1, rows, t, T_K, tgt_d, ntok_d, lps, tok, ld_logits=ld, score=score)
        O.decode_pick_rows(xd[t, 1:], V1, rows, t, T_K, fin, seq, lps2, tok2, forced=forced_d[t:t + 1], ld_logits=ld, score=score2)
        torch.cuda.synchronize()
        for r in (0, 3):
            assert same_bits(tok[r:r + 1], tok2[r:r + 1])
    for r in (0, 3):
        assert same_bits(lps[r], lps2[r]) and same_bits(score[r:r + 1], score2[r:r + 1]) and bool((lps[r] < 0).all())
    assert not same_bits(lps[1], lps2[1])


# ------------------------------------------------------------------ 2. caption_score_pairs: networks, drivers, cases
_NETS = {}
TMAX = 6


def _opt(model, fopt):
    from oracle import weights as OW
    opt = OW.default_opt(vocab_size=fopt['vocab_size'], seq_length=fopt['seq_length'])
    opt.update(fopt)
    opt['caption_model'] = model
    if model.startswith('adaatt'):
        opt['adaatt'] = 1
    return opt


def _fixture_net(model):
    """a ResNet-50 cycle network in f32 whose captioner is the reference fixture's (tests/golden/ref_caprows.npz for att2in2 and topdown,
    ref_decode.npz for the adaptive-attention ones), as tests/test_caprows_gpu.py and tests/test_decode_gpu.py build them; cached"""
    if model not in _NETS:
        from lang2seg_amd import selftest
        if model in CU.MODELS:
            fopt, w, _, _, _ = CU.fixture(model)
        else:
            fopt, w, _, _, _ = DU.fixture(model)
        net = selftest.build_net(_opt(model, fopt), {}, 'f32', None, num_layers=50)
        net.load_state_dict({CAP + k: v for k, v in w.items()})
        net.eval()
        net.parity = None
        _NETS[model] = (net, fopt, w)
    return _NETS[model]


def _features(net, rows, seed):
    rs = np.random.RandomState(seed)
    att = np.abs(rs.normal(0, 1, (rows, L, net.opt['att_feat_size']))).astype(np.float32)
    fc = np.abs(rs.normal(0, 1, (rows, net.opt['fc_feat_size']))).astype(np.float32) if net.captioner.reads_fc else None
    return att, fc


def _tokens(rows, V, seed):
    """rows x TMAX, lengths 1 .. TMAX in turn, zero padded"""
    rs = np.random.RandomState(seed)
    tok = np.zeros((rows, TMAX), np.int64)
    for r in range(rows):
        n = 1 + (r * 5 + 2) % TMAX if rows > 1 else 4
        tok[r, :n] = rs.randint(1, V + 1, n)
    return tok


def _drivers(model, fopt, w, att, fc, which):
    return [DU.RefDriver(model, fopt, w, None if fc is None else fc[r], att[r]) for r in which]


def _host(r):
    return {k: v.cpu().numpy().copy() for k, v in r.items()}


def _check_pairs(got, tok, drv, which):
    """rows `which` of a result against their float64 drivers; every row: zero behind n + 1, ntok, the exact float32 sum"""
    lps, score, ntok = got['logprobs'], got['score'], got['ntok']
    n1 = (tok != 0).sum(1) + 1
    assert lps.shape == (tok.shape[0], TMAX + 1) and lps.dtype == np.float32 and np.array_equal(ntok, n1.astype(np.int32))
    inside = np.arange(TMAX + 1)[None, :] < n1[:, None]
    assert (lps[~inside] == 0).all() and (lps[inside] < 0).all()
    s = np.zeros((tok.shape[0],), np.float32)
    for t in range(TMAX + 1):
        s = (s + lps[:, t]).astype(np.float32)
    assert np.array_equal(score, s)
    ref, ref_score, _ = EU.score_pairs(drv, tok[which])
    e = rel_err(lps[which], ref.astype(np.float32))
    assert e <= FWD_TOL, e
    EU.check_close(score[which], ref_score, 'score')
    return e


@pytest.mark.parametrize('rows', [1, 5, 70])
@pytest.mark.parametrize('model', ['att2in2', 'topdown'])
def test_pairs_batched_f32_against_the_float64_driver(model, rows):
    from lang2seg_amd.nets import caption_rows
    net, fopt, w = _fixture_net(model)
    assert caption_rows.batched(net)
    att, fc = _features(net, rows, 11 + rows)
    tok = _tokens(rows, fopt['vocab_size'], rows)
    which = list(range(rows)) if rows <= 5 else [0, 1, 5, 63, 64, 66, 69]             # (70 rows: both chunks, every length)
    drv = _drivers(model, fopt, w, att, fc, which)
    att_d, fc_d = dev(att), None if fc is None else dev(fc)
    got = _host(net.caption_score_pairs(att_d, fc_d, tok))
    e = _check_pairs(got, tok, drv, which)
    print('%s pairs (batched) rows %d vs the float64 driver: %.2e' % (model, rows, e))
    # device tokens, lengths counted on the device: the same bits; lengths given on the host cut a row
    again = _host(net.caption_score_pairs(att_d, fc_d, dev(tok)))
    assert all(np.array_equal(got[k], again[k]) for k in got)
    cut = np.maximum((tok != 0).sum(1) - 1, 1)
    short = _host(net.caption_score_pairs(att_d, fc_d, tok, lengths=cut))
    tok_cut = np.where(np.arange(TMAX)[None, :] < cut[:, None], tok, 0)
    _check_pairs(short, tok_cut, drv, which)
    # count: the rows at or beyond it read as zeros, the rows below it keep their bits
    if rows > 1:
        part = _host(net.caption_score_pairs(att_d, fc_d, tok, count=count_of(2)))
        assert np.array_equal(part['logprobs'][:2], got['logprobs'][:2]) and (part['logprobs'][2:] == 0).all() and (part['score'][2:] == 0).all()
        assert np.array_equal(part['score'][:2], got['score'][:2])


@pytest.mark.parametrize('model', ['att2in2', 'topdown'])
def test_pairs_rows_are_independent_bit_for_bit(model):
    """70 rows, then the same (features, expression) pairs in reverse order - every row in another chunk position, the first six in the
    other chunk - among other expressions of other lengths, then five of them in a 5-row call: a row's log-probabilities keep their bits.
    A one-row call (the single-row linear kernels) is within FWD_TOL"""
    net, fopt, w = _fixture_net(model)
    V = fopt['vocab_size']
    att, fc = _features(net, 70, 81)
    tok = _tokens(70, V, 70)
    a = _host(net.caption_score_pairs(dev(att), None if fc is None else dev(fc), tok))
    keep = [0, 3, 5, 64, 66, 69]                                      # their pairs stay; every other row gets another expression
    tok2 = _tokens(70, V, 71)[::-1].copy()
    tok2[keep] = tok[keep]
    assert (tok2 != tok).any(1).sum() > 50
    rev = np.arange(70)[::-1].copy()
    b = _host(net.caption_score_pairs(dev(att[rev]), None if fc is None else dev(fc[rev]), tok2[rev]))
    for r in keep:
        assert np.array_equal(a['logprobs'][r].view(np.uint32), b['logprobs'][69 - r].view(np.uint32)), (model, r)
        assert np.array_equal(a['score'][r:r + 1].view(np.uint32), b['score'][69 - r:70 - r].view(np.uint32))
    five = keep[:5]
    c = _host(net.caption_score_pairs(dev(att[five]), None if fc is None else dev(fc[five]), tok[five]))
    assert np.array_equal(c['logprobs'].view(np.uint32), a['logprobs'][five].view(np.uint32))
    one = _host(net.caption_score_pairs(dev(att[3:4]), None if fc is None else dev(fc[3:4]), tok[3:4]))
    assert rel_err(one['logprobs'], a['logprobs'][3:4]) <= FWD_TOL


@pytest.mark.parametrize('model', ['att2in2', 'topdown'])
def test_pairs_with_one_expression_agree_with_caption_score_rows(model):
    """every row the same expression: within FWD_TOL of caption_score_rows (not bit for bit: see the module docstring)"""
    net, fopt, w = _fixture_net(model)
    att, fc = _features(net, 5, 31)
    att_d, fc_d = dev(att), None if fc is None else dev(fc)
    toks = [3, 7, 2, 9]
    ref = _host(net.caption_score_rows(att_d, fc_d, toks, rows=5))
    tok = np.zeros((5, TMAX), np.int64)
    tok[:, :4] = toks
    got = _host(net.caption_score_pairs(att_d, fc_d, tok))
    e = rel_err(got['logprobs'][:, :5], ref['logprobs'])
    print('%s pairs vs caption_score_rows, one expression: %.2e' % (model, e))
    assert e <= FWD_TOL and (got['logprobs'][:, 5:] == 0).all() and rel_err(got['score'], ref['score']) <= FWD_TOL


@pytest.mark.parametrize('model', ['att2in2', 'topdown'])
def test_pairs_launches_do_not_depend_on_rows_count_or_lengths(model):
    net, fopt, w = _fixture_net(model)
    att, fc = _features(net, 70, 5)
    att_d, fc_d = dev(att), None if fc is None else dev(fc)
    tok = _tokens(70, fopt['vocab_size'], 3)
    net.caption_score_pairs(att_d, fc_d, tok)                              # (a buffer's first use allocates it zeroed instead of clearing it)
    a = _calls(lambda: net.caption_score_pairs(att_d, fc_d, tok, count=count_of(2)))
    full = np.random.RandomState(8).randint(1, fopt['vocab_size'] + 1, (70, TMAX))
    b = _calls(lambda: net.caption_score_pairs(att_d, fc_d, full, lengths=[TMAX] * 70, count=count_of(70)))
    assert a == b and a.count('l2s_decode_force_rows') == 2 * (TMAX + 1) and 'l2s_decode_pick_rows' not in a
    at = [i for i, n in enumerate(a) if n == 'l2s_decode_force_rows']
    per = sorted(set(at[k] - at[k - 1] for k in range(1, len(at)) if k % (TMAX + 1)))
    print('%s pairs, rows 70 (two chunks): %d C-ABI calls, %s a token' % (model, len(a), per))
    assert per == [8 if model == 'att2in2' else 9]                        # the greedy step's launches, the logits and the kernel
    small = _calls(lambda: net.caption_score_pairs(att_d[:5], None if fc_d is None else fc_d[:5], tok[:5]))
    assert small.count('l2s_decode_force_rows') == TMAX + 1 and len(small) * 2 - len(a) <= 4     # (one chunk: half the calls, give or take a cast)


_WIDE = {}


def _bf16_net(model):
    """a bf16 network at the production widths (as tests/test_caprows_gpu.py / test_caprows_topdown_gpu.py's _wide_net)"""
    if model not in _WIDE:
        from lang2seg_amd import selftest
        from oracle import weights as OW
        if model == 'att2in2':
            opt = OW.default_opt(vocab_size=60, seq_length=5)
            sd = OW.make_state_dict(opt, seed=3, head_gain=4.0)
        else:
            from topdown_util import td_opt, make_sd
            opt = td_opt(vocab_size=60, seq_length=5)
            sd = make_sd(opt, seed=3, head_gain=4.0, cap_seed=13)
        net = selftest.build_net(opt, {}, 'bf16', sd, num_layers=50)
        net.eval()
        net.parity = None
        _WIDE[model] = net
    return _WIDE[model]


@pytest.mark.parametrize('rows', [1, 5, 70])
@pytest.mark.parametrize('model', ['att2in2', 'topdown'])
def test_pairs_batched_bf16(model, rows):
    """a bf16 network: finite and negative inside a row's length, zero behind it (what the caption_score_rows tests ask of bf16), and
    every checked row within FWD_TOL of caption_score_rows on its own expression (the same network, the same bf16 features)"""
    net = _bf16_net(model)
    att, fc = _features(net, rows, 17 + rows)
    att_d, fc_d = dev(att, torch.bfloat16), None if fc is None else dev(fc, torch.bfloat16)
    tok = _tokens(rows, 60, rows + 1)
    got = _host(net.caption_score_pairs(att_d, fc_d, tok))
    n1 = (tok != 0).sum(1) + 1
    inside = np.arange(TMAX + 1)[None, :] < n1[:, None]
    lps = got['logprobs']
    assert np.isfinite(lps).all() and (lps[inside] < 0).all() and (lps[~inside] == 0).all() and np.isfinite(got['score']).all()
    worst = 0.0
    for r in ([0] if rows == 1 else [0, 1, rows - 1]):
        n = int(n1[r]) - 1
        one = net.caption_score_rows(att_d[r:r + 1], None if fc_d is None else fc_d[r:r + 1], tok[r, :n], rows=1)['logprobs'].cpu().numpy()
        worst = max(worst, rel_err(lps[r:r + 1, :n + 1], one))
    print('%s bf16 pairs rows %d vs caption_score_rows per row: %.2e' % (model, rows, worst))
    assert worst <= FWD_TOL


# ------------------------------------------------------------------ 3. the loop route
@pytest.mark.parametrize('model', ['adaatt', 'adaattmo', 'att2in2'])
def test_pairs_loop_route(model):
    """adaatt / adaattmo (no batched route) and att2in2 with rows_batched = False: the single-mask launches row by row with the new kernel
    on one row, against the float64 drivers; att2in2 also loop against batched"""
    from lang2seg_amd.nets import caption_rows
    net, fopt, w = _fixture_net(model)
    rows = 3
    att, fc = _features(net, rows, 23)
    tok = _tokens(rows, fopt['vocab_size'], 9)
    tok[0, 1:] = 0; tok[1] = np.random.RandomState(4).randint(1, fopt['vocab_size'] + 1, TMAX)      # lengths 1 and TMAX
    drv = _drivers(model, fopt, w, att, fc, range(rows))
    att_d, fc_d = dev(att), None if fc is None else dev(fc)
    if model == 'att2in2':
        batched = _host(net.caption_score_pairs(att_d, fc_d, tok))
        net.rows_batched = False
    try:
        assert not caption_rows.batched(net)
        names = _calls(lambda: net.caption_score_pairs(att_d, fc_d, tok))
        got = _host(net.caption_score_pairs(att_d, fc_d, tok))
        part = _host(net.caption_score_pairs(att_d, fc_d, tok, count=count_of(1)))
    finally:
        net.rows_batched = True
    assert names.count('l2s_decode_force_rows') == rows * (TMAX + 1)
    e = _check_pairs(got, tok, drv, list(range(rows)))
    print('%s pairs (loop) vs the float64 driver: %.2e' % (model, e))
    assert np.array_equal(part['logprobs'][:1], got['logprobs'][:1]) and (part['logprobs'][1:] == 0).all()
    if model == 'att2in2':
        assert rel_err(got['logprobs'], batched['logprobs']) <= FWD_TOL


def test_pairs_errors_on_the_device():
    net, fopt, w = _fixture_net('att2in2')
    att, _ = _features(net, 2, 1)
    att_d = dev(att)
    tok = _tokens(2, fopt['vocab_size'], 2)
    with pytest.raises(ValueError, match='caption_score_pairs.*count'):
        net.caption_score_pairs(att_d, None, tok, count=torch.tensor([2], dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match='caption_score_pairs.*att_feats'):
        net.caption_score_pairs(att_d[:1], None, tok)
    with pytest.raises(ValueError, match='caption_score_pairs.*tokens.*int64'):
        net.caption_score_pairs(att_d, None, dev(tok.astype(np.int32)))
    with pytest.raises(ValueError, match='caption_score_pairs.*lengths'):
        net.caption_score_pairs(att_d, None, dev(tok), lengths=dev(np.asarray([1, 2], np.int64)))


# ------------------------------------------------------------------ 4. the evaluation
_SIZES = [(224, 288), (256, 352)]
_E2E = {}


def _eval_net(variant, dtype):
    from lang2seg_amd import selftest
    from oracle import weights as OW
    opt = OW.default_opt(vocab_size=60, seq_length=6)
    return selftest.build_net(opt, {}, dtype, OW.make_state_dict(opt, seed=3, head_gain=4.0, variant=variant), variant=variant)


def _blobs():
    """the synthetic split of the device-evaluation tests; sentence 1 of image 0 is made longer than seq_length = 6"""
    from test_eval_device_gpu import _synthetic_blobs
    blobs = [dict(b, file_name='image%d.jpg' % j) for j, b in enumerate(_synthetic_blobs(_SIZES, 3))]
    lab = np.zeros((3, 8), np.asarray(blobs[0]['labels']).dtype)
    lab[:, :6] = np.asarray(blobs[0]['labels'])
    lab[1] = [5, 9, 2, 7, 11, 3, 8, 4]
    blobs[0]['labels'] = lab
    return blobs


def _e2e(variant, dtype):
    """a plain run, a run with the option, a run with describe, and a direct run of the rows functions behind every sentence; once"""
    key = (variant, dtype)
    if key in _E2E:
        return _E2E[key]
    from test_eval_device_gpu import _ListLoader
    from lang2seg_amd.model import eval_device as ED
    from lang2seg_amd.model.caption_eval import truncated_tokens
    net, blobs, opt = _eval_net(variant, dtype), _blobs(), dict(verbose=False)
    r = dict(net=net, blobs=blobs)
    run = lambda **kw: ED.eval_split_device(_ListLoader(blobs), net, None, 'val', opt, **kw)
    run(predictions=[], caption_eval=True, caption_describe=True)                   # (buffers' first use)
    r['det0'], r['preds0'] = [], []
    r['calls0'] = _calls(lambda: r.__setitem__('res0', run(details=r['det0'], predictions=r['preds0'])))
    r['det1'], r['preds1'], r['tot1'] = [], [], {}
    r['calls1'] = _calls(lambda: r.__setitem__('res1', run(details=r['det1'], predictions=r['preds1'], caption_eval=True, caption_totals=r['tot1'])))
    r['preds2'], r['tot2'] = [], {}
    r['res2'] = run(predictions=r['preds2'], caption_eval=True, caption_describe=True, caption_totals=r['tot2'])
    r['tot3'] = {}
    r['res3'] = run(caption_eval=True, caption_totals=r['tot3'])                    # no predictions: the totals alone
    # the direct calls, through the evaluation's own hook behind every sentence's mask
    direct = []
    for blob in blobs:
        n = int(np.asarray(blob['labels']).shape[0])
        toks = truncated_tokens(blob['labels'], net.opt['seq_length'])
        masks = dev(np.ascontiguousarray(np.asarray(blob['gt_masks'])[:n], dtype=np.uint8))

        def hook(i, s, ex):
            if variant == 'cycle':
                att, fc = net.caption_features_rows(masks[i:i + 1], 1, tuple(masks.shape[1:]))
            else:
                att, fc = net.caption_features(None)
                att, fc = att.view(1, L, -1), None if fc is None else fc.view(1, -1)
            sc = net.caption_score_rows(att, fc, toks[i], rows=1)
            d = dict(score=sc['score'].clone(), lps=sc['logprobs'].clone(), toks=toks[i])
            d['seq'] = net.caption_decode_rows(att, fc, rows=1)['seq'].clone()
            direct.append(d)
        ED._eval_image(net, blob, n, ED.O.eval_records(n, torch.device(DEV)), 0, True, caption=hook)
    torch.cuda.synchronize()
    r['direct'] = [dict(score=float(d['score'][0]), lps=d['lps'][0].cpu().numpy(), toks=d['toks'], seq=d['seq'][0].cpu().numpy()) for d in direct]
    _E2E[key] = r
    return r


CASES = [('cycle', 'f32'), ('cycle', 'bf16'), ('cycle_response', 'f32')]
NEW_FIELDS = {'gt_expr_logprob', 'gt_expr_logprobs'}
DESCRIBE_FIELDS = {'gt_caption_tokens', 'gt_caption_logprobs', 'gt_caption_exact'}


@pytest.mark.parametrize('variant,dtype', CASES)
def test_eval_keeps_the_metrics_and_the_existing_fields(variant, dtype):
    from test_rle_export_gpu import _same_result, _same_details
    r = _e2e(variant, dtype)
    assert _same_result(r['res0'], r['res1']) and _same_result(r['res0'], r['res2']) and _same_result(r['res0'], r['res3'])
    assert _same_details(r['det0'], r['det1']) and len(r['preds0']) == len(r['preds1']) == len(r['preds2']) == 6
    for p, q, d in zip(r['preds0'], r['preds1'], r['preds2']):
        assert {k: q[k] for k in p} == p and list(q)[:len(p)] == list(p) and set(q) - set(p) == NEW_FIELDS
        assert {k: d[k] for k in q} == q and set(d) - set(q) == DESCRIBE_FIELDS      # (no ix_to_word on this loader: no gt_caption string)


@pytest.mark.parametrize('variant,dtype', CASES)
def test_eval_scores_equal_the_direct_calls_and_the_totals_their_sums(variant, dtype):
    r = _e2e(variant, dtype)
    T = r['net'].opt['seq_length']
    for p, d in zip(r['preds1'], r['direct']):
        n = len(d['toks'])
        assert len(p['gt_expr_logprobs']) == n + 1 <= T + 1 and all(v < 0 for v in p['gt_expr_logprobs'])
        assert rel_err(np.asarray(p['gt_expr_logprobs'], np.float32), d['lps']) <= FWD_TOL
        assert abs(p['gt_expr_logprob'] - d['score']) <= FWD_TOL * max(1.0, abs(d['score']))
        s = np.float32(0)
        for v in p['gt_expr_logprobs']:
            s = np.float32(s + np.float32(v))
        assert np.float32(p['gt_expr_logprob']) == s
    # the expression longer than seq_length is cut to it
    long = r['preds1'][1]
    assert (long['file_name'], long['sent_index']) == ('image0.jpg', 1) and len(long['gt_expr_logprobs']) == T + 1 and r['direct'][1]['toks'] == [5, 9, 2, 7, 11, 3]
    # the totals: the host's float64 sums of the per-sentence fields
    tot = r['tot1']
    lp = [np.float64(p['gt_expr_logprob']) for p in r['preds1']]
    k = [len(p['gt_expr_logprobs']) for p in r['preds1']]
    assert tot['num_sent'] == 6 and tot['num_tok'] == sum(k) and tot['exact_match'] is None
    assert abs(tot['loss'] - (-sum(lp) / sum(k))) <= 1e-12 and abs(tot['perplexity'] - np.exp(tot['loss'])) <= 1e-9 * tot['perplexity']
    per_image = [-sum(lp[3 * j:3 * j + 3]) / sum(k[3 * j:3 * j + 3]) for j in range(2)]
    assert abs(tot['loss_per_image'] - sum(per_image) / 2) <= 1e-12
    assert r['tot3'] == tot and {k_: v for k_, v in r['tot2'].items() if k_ != 'exact_match'} == {k_: v for k_, v in tot.items() if k_ != 'exact_match'}


@pytest.mark.parametrize('variant,dtype', CASES)
def test_eval_describes_the_ground_truth_masks(variant, dtype):
    r = _e2e(variant, dtype)
    exact = 0
    for p, d in zip(r['preds2'], r['direct']):
        seq = d['seq']
        n = int(np.argmax(seq == 0)) if (seq == 0).any() else seq.size
        assert p['gt_caption_tokens'] == [int(v) for v in seq[:n]] and len(p['gt_caption_logprobs']) == n
        assert p['gt_caption_exact'] == int(p['gt_caption_tokens'] == d['toks'])
        exact += p['gt_caption_exact']
    assert r['tot2']['exact_match'] == exact / 6.0


@pytest.mark.parametrize('variant,dtype', CASES)
def test_eval_without_the_option_issues_the_launches_it_did(variant, dtype):
    """the option off: none of the stage's entries, and on `cycle` the call count of eval_split_device(detections=[]) that
    tests/test_select_gpu.py recorded on the commit before its own stage (the same network, the same blobs); the option on: the plain
    run's calls, in order, with the stage's calls between them"""
    from test_eval_device_gpu import _ListLoader, _synthetic_blobs
    from lang2seg_amd.model.eval_device import eval_split_device
    r = _e2e(variant, dtype)
    assert 'l2s_decode_force_rows' not in r['calls0'] and 'l2s_adaptive_pool_rows' not in r['calls0'] and 'l2s_adaptive_pool_fwd' not in r['calls0']
    assert r['calls1'].count('l2s_decode_force_rows') == sum(len(p['gt_expr_logprobs']) for p in r['preds1'])
    it = iter(r['calls1'])
    assert all(c in it for c in r['calls0'])                              # calls0 is a subsequence of calls1
    if variant == 'cycle':
        from test_select_gpu import PARENT_CALLS_DETECTIONS
        blobs = _synthetic_blobs(_SIZES, 3)
        eval_split_device(_ListLoader(blobs), r['net'], None, 'val', dict(verbose=False), detections=[])      # (buffers' first use)
        plain = _calls(lambda: eval_split_device(_ListLoader(blobs), r['net'], None, 'val', dict(verbose=False), detections=[]))
        assert len(plain) == PARENT_CALLS_DETECTIONS[dtype]


def test_eval_tool_prints_the_caption_line_and_writes_the_fields(tmp_path, capsys):
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    try:
        import eval_common as EC
    finally:
        sys.path.pop(0)
    out = str(tmp_path / 'preds.json')
    common = ['--synthetic', '1', '--synthetic_images', '2', '--allow_init_weights', '1', '--output_postfix', 'no_such_run', '--cfg', '', '--verbose', '0',
              '--device_eval', '1', '--results_dir', str(tmp_path)]
    EC.main(EC.parse_args(common + ['--caption_eval', '1', '--caption_eval_describe', '1', '--dump_predictions', out]), 'cycle')
    text = capsys.readouterr().out
    assert 'Captioner on the ground-truth masks (6 sents' in text and 'perplexity' in text and 'exact match' in text
    preds = json.load(open(out))
    assert len(preds) == 6
    for p in preds:
        assert NEW_FIELDS | DESCRIBE_FIELDS | {'gt_caption'} <= set(p) and p['gt_expr_logprob'] < 0
        assert p['gt_caption'] == ' '.join('w%d' % w for w in p['gt_caption_tokens'])
