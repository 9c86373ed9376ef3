"""Caption decoding on the device: the two decision kernels of csrc/decode.hip alone, Network.caption_decode on the reference fixture of
all four captioners (tests/golden/ref_decode.npz) against the numpy restatement of tests/decode_util.py (which tests/test_decode_cpu.py
pins to the reference's own runs), decoding against the training forward, determinism, and the features / public surface around it.

Bounds.  Greedy log-probabilities: FWD_TOL = 1e-5 as tests/test_topdown_gpu.py defines it (rel_err: the largest difference over the
reference's largest magnitude).  Everything of beam search is ABSOLUTE: r, p and logps within 1e-5 in the beam kernel's own test, logps
within 1e-5 and p within 1e-4 on the fixture.  The one exception is a value next to -1000 (the suppressed last word's r, the sum of a
beam that goes on from a completed one; |reference| >= 900): float32 is spaced 6.1e-5 there (1.2e-4 beyond 1024), 1e-5 does not exist, and
such a value is one f32 subtraction or addition of operands that are themselves within 1e-6, so it is held to ONE unit in the last place
of the reference (`near`).  The sampled draw is bracketed, not compared: k is right iff cdf64[k-1] - eps <= u * total < cdf64[k] + eps with
eps = 2e-6 * V1, the bound V1 * 2^-24 of a float32 accumulation of V1 terms summing to <= 1, with margin.

Worst values measured on an MI355X (this file's own prints):
  pick kernel                  every sampled draw inside its float64 bracket with no excess (eps unused); log-probabilities within the bound
  beam kernel                  every integer exact; r / p below 900 in magnitude 9.5e-07 absolute, every value next to -1000 the same bits
  fixture through the network  greedy log-probabilities 7.0e-07; beam 3 logps 1.2e-06 and p 1.9e-06 absolute (no kept beam carries a -1000)
  decode vs training forward   5.4e-08 (tiny captioners), 4.9e-08 (att2in2 at 512 against the resident launch)
  caption_features             0 against the train branch, both variants"""
import re

import numpy as np
import pytest
import torch

import decode_util as DU
from decode_util import fixture, driver, MODELS
from topdown_util import rel_err, CAP

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FWD_TOL = 1e-5
P_TOL = 1e-4
BEAM_TOL = 1e-5


def near(got, ref, tol=BEAM_TOL):
    """-> (every value within its bound, the largest absolute error below 900 in magnitude, the largest error in ulps at or beyond it):
    absolute `tol` where |ref| < 900, one unit in the last place of the float32 reference next to -1000 (see the file's docstring)"""
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float32).reshape(-1)
    big = np.abs(ref) >= 900
    err = np.abs(got - ref.astype(np.float64))
    ulp = np.spacing(np.abs(ref)).astype(np.float64)
    ok = bool(np.all(err[~big] <= tol)) and bool(np.all(err[big] <= ulp[big]))
    return ok, float(err[~big].max(initial=0.0)), float((err[big] / ulp[big]).max(initial=0.0))


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


# ------------------------------------------------------------------ 1. the pick kernel alone
PICK_V1 = [2, 21, 63, 65, 1025, 2000]


def _pick_bufs(T):
    return (torch.zeros(1, dtype=torch.int32, device=DEV), torch.full((T,), -7, dtype=torch.int64, device=DEV),
            torch.full((T,), -7.0, device=DEV), torch.full((1,), -7, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize('V1', PICK_V1)
def test_pick_greedy_ties_and_finished_flag(V1):
    """argmax and its log-probability against numpy; two equal maxima -> the lower index; after a 0 every token is 0 with log-probability 0"""
    O = ops()
    rs = np.random.RandomState(V1)
    x = (rs.normal(0, 3, (4, V1))).astype(np.float32)
    hi = max(1, V1 // 2)
    x[0, 0] = x[0].max() - 1.0                                   # step 0: a word (not 0) wins
    x[1, hi] = x[1, V1 - 1] = x[1].max() + 1.0                   # step 1: two equal maxima -> the lower index
    if V1 == 2:
        x[1] = [0.5, 0.5]                                        # (two words: the tie is between 0 and 1 -> 0, which also ends the sentence)
    x[2, 0] = x[2].max() + 2.0                                   # step 2: the end token
    x[3, V1 - 1] = x[3].max() + 2.0                              # step 3: finished: whatever the logits say
    fin, seq, lps, tok = _pick_bufs(4)
    xd = dev(x)
    toks = []
    for t in range(4):
        O.decode_pick(xd[t], V1, t, True, 1.0, None, None, 0, fin, seq, lps, tok)
        toks.append(tok.clone())
    torch.cuda.synchronize()
    lsm = DU.log_softmax(x)
    want = [int(np.argmax(lsm[0].astype(np.float32))), hi if V1 > 2 else 0, 0, 0]
    if want[0] == 0 or want[1] == 0:                             # the sentence ended earlier: zeros from there
        first0 = want.index(0)
        want = want[:first0] + [0] * (4 - first0)
    got = seq.cpu().numpy().tolist()
    print('pick greedy V1=%d: seq %s' % (V1, got))
    assert got == want and [int(t_) for t_ in toks] == want
    lp = lps.cpu().numpy()
    ended = False
    for t in range(4):
        ref = 0.0 if ended else lsm[t, want[t]]
        assert abs(lp[t] - ref) < FWD_TOL * max(1.0, np.abs(lsm[t]).max()), (t, lp[t], ref)
        ended = ended or want[t] == 0
    assert int(fin) == 1


@pytest.mark.parametrize('temperature', [1.0, 0.5])
@pytest.mark.parametrize('V1', PICK_V1)
def test_pick_sampled_brackets_the_cdf(V1, temperature):
    """injected u in {0, 1 - 2^-24} and 50 random values: the drawn k brackets u * total in the float64 CDF of numpy's log-softmax;
    the reported log-probability is the untempered one"""
    O = ops()
    rs = np.random.RandomState(1000 + V1)
    x = rs.normal(0, 2, (V1,)).astype(np.float32)
    u = np.concatenate([[0.0, 1.0 - 2.0 ** -24], rs.rand(50)]).astype(np.float32)
    n = u.size
    fin, seq, lps, tok = _pick_bufs(n)
    xd, ud = dev(x), dev(u)
    for t in range(n):
        fin.zero_()                                              # every draw on its own: a drawn 0 must not end the others
        O.decode_pick(xd, V1, t, False, temperature, ud, None, 0, fin, seq, lps, tok)
    torch.cuda.synchronize()
    lsm = DU.log_softmax(x)
    cdf = np.cumsum(np.exp(lsm / temperature))
    total, eps = cdf[-1], 2e-6 * V1
    ks, lp = seq.cpu().numpy(), lps.cpu().numpy()
    worst = 0.0
    for t in range(n):
        k = int(ks[t])
        assert 0 <= k < V1
        target = float(u[t]) * total
        lo = cdf[k - 1] if k > 0 else 0.0
        worst = max(worst, lo - target, target - cdf[k])
        assert lo - eps <= target < cdf[k] + eps, (t, k, float(u[t]), lo, target, cdf[k])
        assert abs(lp[t] - lsm[k]) < FWD_TOL * max(1.0, np.abs(lsm).max()), (t, k, lp[t], lsm[k])
    print('pick sampled V1=%d T=%.1f: worst bracket excess %.2e (eps %.2e), %d distinct words' % (V1, temperature, worst, eps, len(set(ks.tolist()))))
    assert int(ks[0]) == int(np.argmax(cdf > 0))                 # u = 0: the first word that has any mass


def test_pick_production_rng_draws_differ_per_token_and_counter():
    """without injected u the draw comes from (seed counter, salt, t): in [0, V1), different tokens for different t / counter values"""
    O = ops()
    V1, n = 2000, 16
    x = dev(np.zeros((V1,), np.float32))                         # uniform: the drawn word is u * V1
    seed = torch.zeros(1, dtype=torch.int64, device=DEV)
    out = []
    for c in range(2):
        fin, seq, lps, tok = _pick_bufs(n)
        for t in range(n):
            fin.zero_()
            O.decode_pick(x, V1, t, False, 1.0, None, seed, 12345, fin, seq, lps, tok)
        O.counter_inc(seed)
        out.append(seq.cpu().numpy())
    assert all(((o >= 0) & (o < V1)).all() for o in out)
    assert len(set(out[0].tolist())) > n // 2 and not np.array_equal(out[0], out[1])


# ------------------------------------------------------------------ 2. the beam kernel alone
def _beam_inputs(B, V1, t, T, rs):
    """logits, previous tables and sums; re-drawn until the restatement's decisions are 1e-4 clear: the candidates among the best B + 1 and
    every row's best min(B, V1) + 1 words (a condition on the inputs, numpy only)"""
    rows, cols = (1 if t == 0 else B), min(B, V1)
    while True:
        x = rs.normal(0, 3, (B, V1)).astype(np.float32)
        bsum = np.zeros((B,), np.float32)
        if t > 0:
            bsum = (-rs.rand(B) * 8).astype(np.float32)
            for q in rs.choice(B, size=min(B - 1, 1 + (B > 2)), replace=False):
                bsum[q] = -1000.0                                # one or two beams already completed
        lp = DU.log_softmax(x).astype(np.float32)
        lp[:, -1] -= np.float32(1000.0)
        srt = -np.sort(-lp[:rows], axis=1)[:, :cols + 1]
        ok = srt.shape[1] < 2 or np.min(srt[:, :-1] - srt[:, 1:]) > 1e-4
        ps = np.sort(np.concatenate([bsum[q] + srt[q, :cols] for q in range(rows)]))[::-1][:B + 1]
        ok = ok and (ps.size < 2 or np.min(ps[:-1] - ps[1:]) > 1e-4)
        if ok:
            return x, lp, bsum


@pytest.mark.parametrize('B', [1, 2, 3, 5, 16])
@pytest.mark.parametrize('V1sel', ['B', 21, 1025, 2000])
def test_beam_step_vs_restatement(B, V1sel):
    """t = 0 (one row), a middle step with completed beams in the table, and the last step (every beam completes), against
    decode_util.beam_step + completions: tokens, parents, forked histories, gathered states, records and the counter exact; r and p
    within 1e-5 absolute (one ulp next to -1000: `near`).  V1 = B exercises cols = min(B, V1); (n_state, R) alternates between (2, 8) and (4, 260)."""
    O = ops()
    V1 = B if V1sel == 'B' else V1sel
    T = 5
    n_state, R = ((2, 8), (4, 260))[(B + (0 if V1sel == 'B' else V1sel)) % 2]
    rs = np.random.RandomState(B * 7919 + V1)
    RW = O.beam_record_words(T)
    worst, worst_ulp = 0.0, 0.0

    def close(a, b):
        nonlocal worst, worst_ulp
        ok, e, u = near(a, b)
        worst, worst_ulp = max(worst, e), max(worst_ulp, u)
        return ok
    for t in (0, 2, T - 1):
        x, lp, bsum = _beam_inputs(B, V1, t, T, rs)
        bseq = np.zeros((T, B), np.int64); blp = np.zeros((T, B), np.float32)
        bseq[:t] = rs.randint(1, max(V1, 2), (t, B)); blp[:t] = -rs.rand(t, B).astype(np.float32) * 3
        bseq[t:] = 99; blp[t:] = 99.0                            # stale rows of an earlier call: never read
        prior = 0 if t == 0 else 2
        st_in = [rs.normal(0, 1, (B, R)).astype(np.float32) for _ in range(n_state)]
        # device
        d_seq, d_lp, d_sum = dev(bseq, torch.int32), dev(blp), dev(bsum)
        d_in = [dev(s) for s in st_in]
        ld_out = R + 4                                            # a leading dimension of its own on the way out
        d_out = [torch.full((B, ld_out), 7.0, device=DEV) for _ in range(n_state)]
        toks, par = torch.full((B,), -7, dtype=torch.int64, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
        done = torch.full((B * T, RW), 7, dtype=torch.int32, device=DEV)
        cnt = torch.full((1,), 5 if t == 0 else prior, dtype=torch.int32, device=DEV)     # (t = 0 resets whatever an earlier call left)
        O.decode_beam_step(dev(x), V1, B, t, T, d_seq, d_lp, d_sum, [(i, o, R, ld_out) for i, o in zip(d_in, d_out)], R, toks, par, done, cnt)
        torch.cuda.synchronize()
        # restatement
        r_seq, r_lp, r_sum = bseq.copy(), blp.copy(), bsum.copy()
        parents, cand = DU.beam_step(lp, B, t, r_seq, r_lp, r_sum)
        p_before = r_sum.copy()
        rdone = [None] * prior
        DU.completions(t, T, B, r_seq, r_lp, r_sum, rdone)
        new = rdone[prior:]
        comp = [i for i in range(B) if r_seq[t, i] == 0 or t == T - 1]
        assert len(comp) == len(new)
        g_seq, g_lp, g_sum = d_seq.cpu().numpy(), d_lp.cpu().numpy(), d_sum.cpu().numpy()
        assert toks.cpu().numpy().tolist() == r_seq[t].tolist(), (t, toks, r_seq[t])
        assert par.cpu().numpy().tolist() == parents
        assert np.array_equal(g_seq[:t + 1], r_seq[:t + 1]) and np.array_equal(g_seq[t + 1:], bseq[t + 1:])
        assert np.array_equal(g_lp[:t], r_lp[:t]) and close(g_lp[t], r_lp[t]) and close(g_sum, r_sum)
        for j in range(n_state):
            o = d_out[j].cpu().numpy()
            assert np.array_equal(o[:, :R], st_in[j][parents]) and np.all(o[:, R:] == 7.0)
        assert int(cnt) == prior + len(new)
        rec = done.cpu().numpy()
        for k, r in enumerate(new):
            row = rec[prior + k]
            assert row[:T].tolist() == [int(v) if s <= t else 0 for s, v in enumerate(r['seq'])]
            want_lp = np.where(np.arange(T) <= t, r['logps'], 0.0)
            assert close(row[T:2 * T].view(np.float32), want_lp) and np.all(row[T + t + 1:2 * T] == 0)
            assert close(row[2 * T:2 * T + 1].view(np.float32), [r['p']]) and float(r['p']) == float(p_before[comp[k]])
            assert int(row[2 * T + 1]) == prior + k == r['index']
        assert np.all(rec[:prior] == 7) and np.all(rec[prior + len(new):] == 7)
        if t == T - 1:
            assert len(new) == B
    print('beam step B=%d V1=%d n_state=%d R=%d: worst r / p error %.2e absolute, %.2f ulp next to -1000' % (B, V1, n_state, R, worst, worst_ulp))


def test_beam_step_rejects_bad_arguments_before_any_launch():
    from lang2seg_amd._lib import L2SError
    O = ops()
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=DEV)
    T, V1 = 4, 8
    args = lambda B, t=0, T=T, V1=V1: (z(16 * 64), V1, B, t, T, z(T * 16, torch.int32), z(T * 16), z(16), [], 8, z(16, torch.int64),
                                       z(16, torch.int32), z(16 * T * O.beam_record_words(T), torch.int32), z(1, torch.int32))
    with pytest.raises(ValueError, match='--beam_size'):
        O.decode_beam_step(*args(17))
    with pytest.raises(ValueError, match='--beam_size'):
        O.decode_beam_step(*args(0))
    with pytest.raises(L2SError):
        O.decode_beam_step(*args(9))                              # more beams than words
    with pytest.raises(L2SError):
        O.decode_beam_step(*args(2, t=4))                         # t beyond T - 1


# ------------------------------------------------------------------ 3. the reference fixture through caption_decode
_NETS = {}


def _opt(model, fopt):
    from oracle import weights as OW
    opt = OW.default_opt(vocab_size=fopt['vocab_size'], seq_length=fopt['seq_length'])
    opt.update(fopt)
    opt['caption_model'] = model
    if model.startswith('adaatt'):
        opt['adaatt'] = 1
    return opt


def _fixture_net(model):
    """a ResNet-50 cycle network in f32 whose captioner is the fixture's; cached"""
    if model not in _NETS:
        from lang2seg_amd import selftest
        fopt, w, fc, att, g = fixture(model)
        net = selftest.build_net(_opt(model, fopt), {}, 'f32', None, num_layers=50)
        net.load_state_dict({CAP + k: v for k, v in w.items()})
        net.eval()
        net.parity = None
        _NETS[model] = (net, None if fc is None else dev(fc), dev(att))
    return _NETS[model]


@pytest.mark.parametrize('model', MODELS)
def test_fixture_greedy(model):
    """greedy tokens exact, log-probabilities within FWD_TOL of the reference's own sample()"""
    net, fc, att = _fixture_net(model)
    g = fixture(model)[4]
    r = net.caption_decode(att, fc)
    e = rel_err(np.asarray(r['logprobs'], np.float32), g['greedy_logprobs']) if len(r['seq']) else 0.0
    print('%s greedy on the device: %s, logprobs %.2e' % (model, r['seq'], e))
    assert r['seq'] == [int(v) for v in g['greedy_seq']] and len(r['logprobs']) == len(r['seq'])
    assert e < FWD_TOL


@pytest.mark.parametrize('model', MODELS)
def test_fixture_beam3(model):
    """beam_size 3: `beams` equals the restatement with the alias off (the intended rule: by joint log-probability): sequences exact,
    logps within 1e-5 and p within 1e-4, both absolute (`near`: one ulp for a value next to -1000); seq / logprobs are beams[0]'s"""
    net, fc, att = _fixture_net(model)
    T = net.opt['seq_length']
    want, every, _ = DU.beam_search(driver(model), T, 3, legacy_p_alias=False)
    r = net.caption_decode(att, fc, beam_size=3)
    assert len(r['beams']) == 3
    e_lp = e_p = 0.0
    for b, w in zip(r['beams'], want):
        assert b['seq'] == [int(v) for v in w['seq']] and b['index'] == w['index'], (b, w)
        ok_lp, a_lp, _ = near(b['logps'], w['logps'], BEAM_TOL)
        ok_p, a_p, _ = near([b['p']], [w['p']], P_TOL)
        e_lp, e_p = max(e_lp, a_lp), max(e_p, a_p)
        assert ok_lp and ok_p, (b, w)
    print('%s beam 3 on the device: best %s p %.4f; absolute errors: logps %.2e p %.2e' % (model, r['seq'], r['beams'][0]['p'], e_lp, e_p))
    n = r['beams'][0]['seq'].index(0) if 0 in r['beams'][0]['seq'] else T
    assert r['seq'] == r['beams'][0]['seq'][:n] and r['logprobs'] == r['beams'][0]['logps'][:n]


def test_fixture_beam1_kernel_equals_greedy_pick():
    """beam_size 1 through the beam kernel's path is not offered by caption_decode (it is the greedy loop); the kernel with B = 1 on the
    greedy run's logits must pick the same word unless that word is the last column, which beam search suppresses"""
    O = ops()
    net, fc, att = _fixture_net('att2in2')
    r = net.caption_decode(att, fc)
    V1, T = net.opt['vocab_size'] + 1, net.opt['seq_length']
    logits = net.buf('dec.logits', (1, V1), torch.float32)      # the last step's
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=DEV)
    toks = z(1, torch.int64)
    O.decode_beam_step(logits, V1, 1, 0, T, z(T, torch.int32), z(T), z(1), [], 1, toks, z(1, torch.int32), z(T * O.beam_record_words(T), torch.int32),
                       z(1, torch.int32))
    lp = DU.log_softmax(logits.cpu().numpy()[0]).astype(np.float32)
    lp[-1] -= 1000.0
    assert int(toks) == int(np.argmax(lp))


# ------------------------------------------------------------------ 3b. the fixture decodes to the parent commit's bits
# recorded with decode_record on the commit before the captioners moved into nets/captioners.py (twice per captioner, equal results): greedy
# (seq, logprobs), the beam-3 `beams` as (seq, logps, p, index), and for att2in2 one sampled run with injected draws; floats as hex
PARENT_DECODE = {
    'att2in2': {
        'greedy': ([10, 20, 9, 9, 9, 9], '-0x1.066c76p+1 -0x1.e072d8p+0 -0x1.9c8edep+0 -0x1.a7fc0cp+0 -0x1.a33304p+0 -0x1.a3c15p+0'),
        'beam3': [
            ([11, 9, 9, 9, 9, 9], '-0x1.318b24p+1 -0x1.a975eep+0 -0x1.0cf682p+0 -0x1.62e71ap+0 -0x1.6fc8ecp+0 -0x1.7f4a18p+0', '-0x1.2d6f9cp+3', 0),
            ([11, 9, 9, 9, 5, 16], '-0x1.318b24p+1 -0x1.a975eep+0 -0x1.0cf682p+0 -0x1.62e71ap+0 -0x1.3559e4p+1 -0x1.77325ap+0', '-0x1.4bcap+3', 1),
            ([11, 9, 9, 9, 9, 10], '-0x1.318b24p+1 -0x1.a975eep+0 -0x1.0cf682p+0 -0x1.62e71ap+0 -0x1.6fc8ecp+0 -0x1.3a86f8p+1', '-0x1.4c2816p+3', 2),
        ],
        'sampled': ([6, 18, 5, 17, 10, 10], '-0x1.8ce8c6p+1 -0x1.1d8928p+1 -0x1.2e1be6p+1 -0x1.8ca89p+1 -0x1.54cb7p+0 -0x1.05f424p+1'),
    },
    'topdown': {
        'greedy': ([7], '-0x1.326d7ep-1'),
        'beam3': [
            ([7, 0, 0, 0, 0, 0], '-0x1.326d88p-1 -0x1.986e98p-2 0x0p+0 0x0p+0 0x0p+0 0x0p+0', '-0x1.fea4d4p-1', 1),
            ([0, 0, 0, 0, 0, 0], '-0x1.5533ccp+0 0x0p+0 0x0p+0 0x0p+0 0x0p+0 0x0p+0', '-0x1.5533ccp+0', 0),
            ([7, 7, 0, 0, 0, 0], '-0x1.326d88p-1 -0x1.2499b6p+0 -0x1.fed64p-1 0x0p+0 0x0p+0 0x0p+0', '-0x1.5e9dccp+1', 3),
        ],
    },
    'adaatt': {
        'greedy': ([6], '-0x1.12832p+0'),
        'beam3': [
            ([0, 0, 0, 0, 0, 0], '-0x1.4f6ef4p+0 0x0p+0 0x0p+0 0x0p+0 0x0p+0 0x0p+0', '-0x1.4f6ef4p+0', 0),
            ([6, 0, 0, 0, 0, 0], '-0x1.128324p+0 -0x1.09058cp+0 0x0p+0 0x0p+0 0x0p+0 0x0p+0', '-0x1.0dc458p+1', 1),
            ([18, 0, 0, 0, 0, 0], '-0x1.65aa94p+1 -0x1.5358fp-1 0x0p+0 0x0p+0 0x0p+0 0x0p+0', '-0x1.ba80dp+1', 2),
        ],
    },
    'adaattmo': {
        'greedy': ([2, 2, 2, 2, 2, 2], '-0x1.43eef6p+0 -0x1.24a19cp+0 -0x1.45854ap+0 -0x1.5f8cbcp+0 -0x1.70ab6ep+0 -0x1.78ca7ap+0'),
        'beam3': [
            ([8, 8, 8, 8, 8, 2], '-0x1.b38cp+0 -0x1.cfb1b6p-1 -0x1.08f0dp+0 -0x1.226f66p+0 -0x1.2fd32ep+0 -0x1.1fa054p+0', '-0x1.c58e24p+2', 0),
            ([8, 8, 8, 8, 8, 8], '-0x1.b38cp+0 -0x1.cfb1b6p-1 -0x1.08f0dp+0 -0x1.226f66p+0 -0x1.2fd32ep+0 -0x1.385b0cp+0', '-0x1.cbbcd4p+2', 1),
            ([8, 8, 8, 8, 2, 2], '-0x1.b38cp+0 -0x1.cfb1b6p-1 -0x1.08f0dp+0 -0x1.226f66p+0 -0x1.261872p+0 -0x1.7544e4p+0', '-0x1.d88898p+2', 2),
        ],
    },
}


def _hx(v):
    return ' '.join(re.sub(r'\.?0+p', 'p', float(x).hex()) for x in v)       # float32 values: at most six hex digits


def decode_record(model):
    net, fc, att = _fixture_net(model)
    g = net.caption_decode(att, fc)
    b = net.caption_decode(att, fc, beam_size=3)
    rec = {'greedy': (g['seq'], _hx(g['logprobs'])), 'beam3': [(q['seq'], _hx(q['logps']), _hx([q['p']]), q['index']) for q in b['beams']]}
    if model == 'att2in2':
        T = net.opt['seq_length']
        net.parity = {'sample': dev(np.random.RandomState(5).rand(T).astype(np.float32))}
        try:
            s = net.caption_decode(att, fc, sample_max=0, temperature=0.8)
        finally:
            net.parity = None
        rec['sampled'] = (s['seq'], _hx(s['logprobs']))
    return rec


@pytest.mark.parametrize('model', MODELS)
def test_fixture_decodes_the_parents_bits(model):
    """greedy seq / logprobs, beam-3 beams (seq, logps, p, index) and (att2in2) a sampled run with injected draws: equal, bit for bit, to
    what the parent commit decoded"""
    rec = decode_record(model)
    print('decode record %s: %r' % (model, rec))
    assert rec == PARENT_DECODE[model]


# ------------------------------------------------------------------ 4. decoding equals the training forward
def _teacher_forced(net, seq, fc, att):
    """cap.logp [S][V1] of Network._caption_fwd (eval mode, keep_logprobs) with the decoded words as inputs"""
    T = net.opt['seq_length']
    S = min(len(seq) + 1, T)
    words = [0] + list(seq) + [0]
    d = dict(S=S, cap_in=dev(np.asarray(words[:S], np.int64)), cap_tgt=dev(np.asarray(words[1:S + 1], np.int64)),
             cap_mask=torch.ones(S, device=DEV))
    net.keep_logprobs, net._cap_pre = True, None
    net.t = {'fc_feats': fc}
    net._caption_fwd(d, att, torch.zeros(8, device=DEV))
    torch.cuda.synchronize()
    return net.t['cap.logp'][:S].clone(), S


@pytest.mark.parametrize('model', MODELS)
def test_decode_equals_training_forward(model):
    net, fc, att = _fixture_net(model)
    r = net.caption_decode(att, fc)
    lp, S = _teacher_forced(net, r['seq'], fc, att)
    got = np.asarray(r['logprobs'], np.float32)
    ref = np.asarray([float(lp[i, w]) for i, w in enumerate(r['seq'])], np.float32)
    e = float(np.abs(got - ref).max() / max(1e-12, np.abs(lp.cpu().numpy()).max())) if len(ref) else 0.0
    print('%s decode vs teacher-forced forward: %d words, %.2e' % (model, len(ref), e))
    assert e < FWD_TOL
    # and the forward's own argmax at every step is the decoded word (or the end)
    am = lp.argmax(1).cpu().numpy().tolist()
    assert am[:len(r['seq'])] == r['seq'] and (len(r['seq']) == net.opt['seq_length'] or am[len(r['seq'])] == 0)


def test_decode_equals_resident_training_forward_att2in2_512():
    """att2in2 at R = AH = IE = 512, V = 60, T = 5: the training forward is the resident launch (csrc/cap_recur.hip), decoding the
    per-token path"""
    from lang2seg_amd import selftest
    from oracle import weights as OW
    opt = OW.default_opt(vocab_size=60, seq_length=5)
    assert opt['rnn_size'] == opt['att_hid_size'] == opt['input_encoding_size'] == 512 and opt.get('caption_model', 'att2in2') == 'att2in2'
    sd = OW.make_state_dict(opt, seed=3, head_gain=4.0)
    net = selftest.build_net(opt, {}, 'f32', sd, num_layers=50)
    net.eval()
    rs = np.random.RandomState(3)
    att = dev(rs.normal(0, 1, (196, opt['att_feat_size'])).astype(np.float32))
    r = net.caption_decode(att)
    lp, S = _teacher_forced(net, r['seq'], None, att)
    assert net.t['cap.resident'], 'the resident launch was to be the comparison'
    got = np.asarray(r['logprobs'], np.float32)
    ref = np.asarray([float(lp[i, w]) for i, w in enumerate(r['seq'])], np.float32)
    e = float(np.abs(got - ref).max() / np.abs(lp.cpu().numpy()).max()) if len(ref) else 0.0
    print('att2in2 512 decode vs resident forward: %s, %.2e' % (r['seq'], e))
    assert e < FWD_TOL
    rb = net.caption_decode(att, beam_size=3)
    assert len(rb['beams']) == 3 and rb['beams'][0]['p'] >= rb['beams'][1]['p'] >= rb['beams'][2]['p']


# ------------------------------------------------------------------ 5. determinism
def test_sampled_decoding_is_deterministic_with_injected_u_and_fresh_without():
    net, fc, att = _fixture_net('att2in2')
    T = net.opt['seq_length']
    u = dev(np.random.RandomState(5).rand(T).astype(np.float32))
    net.parity = {'sample': u}
    try:
        a = net.caption_decode(att, fc, sample_max=0, temperature=0.8)
        ba = net.buf('dec.out', (12 * T,), torch.uint8).cpu().numpy().tobytes()
        b = net.caption_decode(att, fc, sample_max=0, temperature=0.8)
        bb = net.buf('dec.out', (12 * T,), torch.uint8).cpu().numpy().tobytes()
    finally:
        net.parity = None
    assert ba == bb and a == b
    # the restatement's draw with the same u (float64 CDF): the same words unless a draw sits within rounding of a CDF step
    seq, lps, _ = DU.sample(driver('att2in2'), T, sample_max=0, temperature=0.8, u=u.cpu().numpy())
    print('sampled with injected u: device %s, restatement %s' % (a['seq'], seq))
    assert a['seq'] == seq and np.abs(np.asarray(a['logprobs']) - np.asarray(lps)).max(initial=0.0) < FWD_TOL * max(1.0, np.abs(lps).max(initial=0.0))
    c = net.caption_decode(att, fc, sample_max=0)
    d = net.caption_decode(att, fc, sample_max=0)
    print('production RNG: %s then %s' % (c['seq'], d['seq']))
    assert (c['seq'], c['logprobs']) != (d['seq'], d['logprobs'])


# ------------------------------------------------------------------ 6. caption_features against the train branch
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


@pytest.mark.parametrize('variant', ['cycle', 'cycle_response'])
def test_caption_features_equal_the_train_branch(variant):
    """the features of the TEST forward under the ground-truth mask against att_feats / fc_feats of a forward-only train step on the same
    blob (encoder dropouts 0): the same launches on the same inputs, so the difference is expected to be 0"""
    net, blob = _feature_net(variant)
    net.train()
    d = net.upload_blob(dict(blob), 0)
    net.forward_backward(d, backward=False)
    torch.cuda.synchronize()
    att_t, fc_t = net.t['att_feats'].clone(), net.t['fc_feats'].clone()
    net.eval()
    net.forward_test_image(d)
    net.forward_test_sentence(d)
    att, fc = net.caption_features(d['gt_masks'] if variant == 'cycle' else None)
    torch.cuda.synchronize()
    ea, ef = rel_err(att, att_t), rel_err(fc, fc_t)
    print('caption_features %s vs the train branch: att %.2e fc %.2e' % (variant, ea, ef))
    assert float(att_t.abs().max()) > 0 and float(fc_t.abs().max()) > 0
    assert ea < FWD_TOL and ef < FWD_TOL
    if variant == 'cycle':
        with pytest.raises(ValueError, match='mask'):
            net.caption_features(None)


# ------------------------------------------------------------------ 7. the public surface
def test_caption_image_end_to_end():
    from lang2seg_amd.model.caption_device import caption_image
    from lang2seg_amd.model.predict_device import predict_image
    net, blob = _feature_net('cycle')
    V1 = net.opt['vocab_size'] + 1
    S = int(np.asarray(blob['labels']).shape[0])
    data = dict(data=blob['data'], im_info=blob['im_info'], file_name='synthetic.jpg')
    words = {str(i): 'w%d' % i for i in range(1, V1)}
    base = predict_image(net, dict(data), blob['labels'])
    out = caption_image(net, dict(data), blob['labels'], ix_to_word=words)
    assert len(out) == len(base) == S
    for p, b in zip(out, base):
        assert {k: p[k] for k in b} == b                          # predict_image's fields unchanged
        assert all(0 < w < V1 for w in p['caption_tokens']) and len(p['caption_logprobs']) == len(p['caption_tokens']) <= net.opt['seq_length']
        assert p['caption'] == ' '.join('w%d' % w for w in p['caption_tokens'])
    gm = np.ascontiguousarray(np.asarray(blob['gt_masks'])[:S], dtype=np.uint8)
    outg = caption_image(net, dict(data), blob['labels'], masks=gm, beam_size=2, ix_to_word=words)
    assert len(outg) == S and all(len(p['caption_beams']) == 2 and p['caption_tokens'] == [w for w in p['caption_beams'][0]['seq'] if w][:len(p['caption_tokens'])]
                                  for p in outg)
    print('caption_image: %s | gt masks, beam 2: %s' % ([p['caption'] for p in out], [p['caption'] for p in outg]))
    with pytest.raises(ValueError, match='--beam_size'):
        caption_image(net, dict(data), blob['labels'], beam_size=17)
    with pytest.raises(ValueError, match='masks'):
        caption_image(net, dict(data), blob['labels'], masks=gm[:, :-1])


def test_predict_tool_captions_a_synthetic_image(capsys):
    """tools/predict.py --synthetic 1 --caption 1 in this process: one dict per sentence, the words printed as w<id>; --caption with
    --all_detections is an error that names both flags"""
    import json
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    try:
        import predict
    finally:
        sys.path.pop(0)
    common = ['--synthetic', '1', '--allow_init_weights', '1', '--output_postfix', 'no_such_run', '--cfg', '', '--caption', '1']
    with pytest.raises(ValueError, match='--caption.*--all_detections'):
        predict.main(predict.parse_args(common + ['--all_detections', '1']))
    capsys.readouterr()
    preds = predict.main(predict.parse_args(common + ['--beam_size', '2']))
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(preds) == len(printed) == 3
    for p in preds:
        assert all(0 < w <= 1999 for w in p['caption_tokens']) and len(p['caption_beams']) == 2
        assert p['caption'] == ' '.join('w%d' % w for w in p['caption_tokens'])
    assert [p['caption'] for p in printed] == [p['caption'] for p in preds]


@pytest.mark.parametrize('shape', [(37, 53, 160, 224), (480, 640, 600, 800)])
def test_mask_resize_nearest_is_pil_nearest(shape):
    from oracle import boxes as OB
    O = ops()
    ih, iw, H, W = shape
    src = (np.random.RandomState(ih).rand(ih, iw) > 0.5).astype(np.uint8)
    dst = torch.full((H, W), 9, dtype=torch.uint8, device=DEV)
    O.mask_resize_nearest(dev(src), ih, iw, dst, H, W)
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), OB.imresize_nearest_u8(src, (H, W)))
