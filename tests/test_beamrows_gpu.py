"""Beam search on rows on the device (csrc/decode.hip l2s_decode_beam_step_rows / l2s_decode_beam_finish_rows, the *_groups entries of
csrc/caption_step.hip and csrc/caption_rows.hip, nets/caption_rows.py caption_beam_rows, model/detect_device.py).

Bounds.
  kernels alone   l2s_decode_beam_step_rows against l2s_decode_beam_step per detection on copies of the same inputs, the *_groups entries
                  against the *_rows entries on operands replicated `group` times: the same bits in every output (one device function
                  each).  l2s_decode_beam_finish_rows against numpy's stable sort (tests/beamrows_util.py): exact.
  the fixture     tests/golden/ref_caprows.npz, 5 rows, att2in2 and topdown.  The loop route against Network.caption_decode(beam_size=B)
                  row by row: tokens, completion order and every float by bits (the same launches on the same buffers).  The batched route
                  against the loop route: tokens exact, logps and p within 1e-5 absolute (tests/test_decode_gpu.py's bound for beam search),
                  a value next to -1000 (|reference| >= 900, where float32 is spaced 6.1e-5) by bits.  tests/test_beamrows_cpu.py holds
                  every decision of these searches to a margin above 1e-4.
  end to end      the tiny cycle network of tests/test_caprows_gpu.py: tokens exact, p within 1e-5 of caption_decode(beam_size=3).

Worst values measured on an MI355X (this file's own prints): batched against loop route 1.9e-06 absolute (both captioners, B = 5), every
value next to -1000 the same bits; detect_image's beams against caption_decode(beam_size=3) per detection 3.8e-06 (100 detections)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import beamrows_util as BU
import caprows_util as CU
from topdown_util import CAP

pytestmark = pytest.mark.gpu

DEV = 'cuda'
TOL = 1e-5
L = 196
NEW_ENTRIES = ('l2s_decode_beam_step_rows', 'l2s_decode_beam_finish_rows', 'l2s_cap_att_dots_groups', 'l2s_cap_apply_gates_groups',
               'l2s_cap_att_apply_groups', 'l2s_lstm_cell_groups')
# detect_image(describe=True) on the tiny cycle network below: the C-ABI calls the parent commit issues, recorded on it (MI355X)
PARENT_CALLS_DESCRIBE = 240


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
    return None if n is None else torch.tensor([n], dtype=torch.int32, device=DEV)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _calls(fn):
    """the C-ABI entries fn() issues, in order (tests/test_caprows_gpu.py's spy)"""
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


def _read_backs(fn):
    """how often fn() brings a tensor to the host"""
    n, real = [0], {k: getattr(torch.Tensor, k) for k in ('cpu', 'item', 'tolist', 'numpy')}

    def wrap(k):
        def f(self, *a, **kw):
            n[0] += 1
            return real[k](self, *a, **kw)
        return f
    for k in real:
        setattr(torch.Tensor, k, wrap(k))
    try:
        fn()
    finally:
        for k, v in real.items():
            setattr(torch.Tensor, k, v)
    return n[0]


def _live(rows, row0, count):
    return rows if count is None else max(0, min(rows, count - row0))


# ------------------------------------------------------------------ 1. the beam step on rows
class _Step(object):
    """one set of the step's tables on the device, filled as tests/test_decode_gpu.py's _beam_inputs draws them (without its redraws: both
    sides are device kernels here) around sentinels: whatever a dead detection owns must come out as it went in"""

    def __init__(self, B, V1, T, t, rows, rs, n_state, R, x=None, bsum=None):
        O = ops()
        n, RW = rows * B, O.beam_record_words(T)
        self.B, self.V1, self.T, self.t, self.rows, self.R, self.ld_out = B, V1, T, t, rows, R, R + 4
        if x is None:
            x = rs.normal(0, 3, (n, V1)).astype(np.float32)
        if bsum is None:
            bsum = np.zeros((rows, B), np.float32)
            if t > 0:
                bsum = (-rs.rand(rows, B) * 8).astype(np.float32)
                for d in range(rows):
                    for q in rs.choice(B, size=min(B - 1, 1 + (B > 2)), replace=False):
                        bsum[d, q] = -1000.0                       # one or two beams already completed
        bseq, blp = np.full((rows, T, B), 99, np.int32), np.full((rows, T, B), 99.0, np.float32)
        bseq[:, :t] = rs.randint(1, max(V1, 2), (rows, t, B))
        blp[:, :t] = -rs.rand(rows, t, B).astype(np.float32) * 3
        cnt = np.full((rows,), 5, np.int32) if t == 0 else rs.randint(0, 3, (rows,)).astype(np.int32)
        self.x = dev(x)
        self.t_ = dict(seq=dev(bseq), lp=dev(blp), sum=dev(bsum), toks=torch.full((n,), -7, dtype=torch.int64, device=DEV),
                       par=torch.full((rows, B), -7, dtype=torch.int32, device=DEV),
                       done=torch.full((rows, B * T * RW), 7, dtype=torch.int32, device=DEV), cnt=dev(cnt))
        self.s_in = [dev(rs.normal(0, 1, (n, R)).astype(np.float32)) for _ in range(n_state)]
        for j in range(n_state):
            self.t_['out%d' % j] = torch.full((n, self.ld_out), 7.0, device=DEV)

    def copy(self):
        c = object.__new__(_Step)
        c.__dict__.update(self.__dict__)
        c.t_ = {k: v.clone() for k, v in self.t_.items()}
        return c

    def states(self, lo=0, hi=None):
        return [(i[lo:hi], self.t_['out%d' % j][lo:hi], self.R, self.ld_out) for j, i in enumerate(self.s_in)]

    def run_rows(self, row0, count):
        t = self.t_
        ops().decode_beam_step_rows(self.x, self.V1, self.B, self.t, self.T, self.rows, t['seq'], t['lp'], t['sum'], self.states(), self.R, t['toks'],
                                    t['par'], t['done'], t['cnt'], count_of(count), row0)
        assert ops().last_kernel() == 'decode_beam_step_rows_kernel'

    def run_single(self, d):
        t, B = self.t_, self.B
        ops().decode_beam_step(self.x[d * B:(d + 1) * B], self.V1, B, self.t, self.T, t['seq'][d], t['lp'][d], t['sum'][d],
                               self.states(d * B, (d + 1) * B), self.R, t['toks'][d * B:(d + 1) * B], t['par'][d], t['done'][d], t['cnt'][d:d + 1])
        assert ops().last_kernel() == 'decode_beam_step_kernel'


def _step_case(s, row0, count, what):
    ref, start = s.copy(), s.copy()
    s.run_rows(row0, count)
    live = _live(s.rows, row0, count)
    for d in range(live):
        ref.run_single(d)
    torch.cuda.synchronize()
    for k in s.t_:
        assert same_bits(s.t_[k], ref.t_[k]), (what, k)
        n = s.t_[k].shape[0] // s.rows                              # rows of this table per detection
        assert same_bits(s.t_[k][live * n:], start.t_[k][live * n:]), (what, k, 'a dead detection was written')
    return live


# (T, t, rows, row0, count): T in {1, 6, 64}, t in {0, 1, T - 1}, rows in {1, 5, 65}, row0 in {0, 3}, count in {none, 0, 2, rows}
STEP_COMBOS = [(1, 0, 1, 0, None), (1, 0, 5, 0, 0), (6, 0, 5, 3, 'rows'), (6, 1, 5, 0, 2), (6, 5, 65, 3, None), (6, 1, 65, 0, 'rows'),
               (64, 1, 5, 0, None), (64, 63, 5, 3, 2), (64, 0, 65, 0, 2), (64, 63, 1, 0, 'rows'), (6, 5, 1, 3, 0), (64, 63, 65, 3, 'rows')]


@pytest.mark.parametrize('B', [1, 2, 3, 16])
@pytest.mark.parametrize('V1sel', ['B', 21, 3350])
def test_beam_step_rows_equals_beam_step_per_detection(B, V1sel):
    """tables, sums, tokens, parents, records, counters and gathered states: the bits of l2s_decode_beam_step called per live detection"""
    V1 = B if V1sel == 'B' else V1sel
    rs = np.random.RandomState(B * 7919 + V1)
    lives = []
    for i, (T, t, rows, row0, count) in enumerate(STEP_COMBOS):
        n_state, R = ((2, 8), (4, 260))[i % 2]
        count = rows if count == 'rows' else count
        s = _Step(B, V1, T, t, rows, rs, n_state, R)
        lives.append(_step_case(s, row0, count, (B, V1, T, t, rows, row0, count)))
    assert lives == [1, 0, 2, 2, 65, 65, 5, 0, 2, 1, 0, 62]


def test_beam_step_rows_with_nan_logits_and_exact_ties():
    B, V1, T, t, rows = 3, 21, 6, 1, 5
    rs = np.random.RandomState(5)
    x = rs.normal(0, 3, (rows * B, V1)).astype(np.float32)
    x[1 * B + 0] = np.nan                                         # a whole row of detection 1
    x[1 * B + 2, ::2] = np.nan                                    # and half of another
    x[2 * B:3 * B] = np.round(x[2 * B:3 * B])                     # detection 2: equal logits in every row ...
    x[3 * B + 1] = x[3 * B + 0]                                   # detection 3: two equal rows ...
    bsum = (-rs.rand(rows, B) * 8).astype(np.float32)
    bsum[2] = -2.0                                                # ... under equal sums: candidates tie exactly
    bsum[3, :2] = -1.5
    bsum[4, 0] = np.nan                                           # a NaN sum ranks last
    s = _Step(B, V1, T, t, rows, rs, 2, 8, x=x, bsum=bsum)
    assert _step_case(s, 0, None, 'nan and ties') == 5
    toks = s.t_['toks'].cpu().numpy()
    assert ((toks >= 0) & (toks < V1)).all()


def test_beam_step_rows_rejects_bad_arguments_before_any_launch():
    from lang2seg_amd._lib import L2SError
    O = ops()
    z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=DEV)
    T, V1, rows = 4, 8, 2
    args = lambda B, t=0, rows=rows: (z(rows * 16 * 64), V1, B, t, T, rows, z(rows * T * 16, torch.int32), z(rows * T * 16), z(rows * 16), [], 8,
                                      z(rows * 16, torch.int64), z(rows * 16, torch.int32), z(rows * 16 * T * O.beam_record_words(T), torch.int32),
                                      z(rows, torch.int32))
    O.memset_zero(z(4))
    before = O.last_kernel()
    with pytest.raises(ValueError, match='--beam_size'):
        O.decode_beam_step_rows(*args(17))
    with pytest.raises(ValueError, match='rows'):
        O.decode_beam_step_rows(*args(2, rows=0))
    with pytest.raises(ValueError, match='row0'):
        O.decode_beam_step_rows(*args(2), row0=-1)
    with pytest.raises(ValueError, match='count'):
        O.decode_beam_step_rows(*args(2), count=z(1))
    with pytest.raises(ValueError, match='smaller'):
        O.decode_beam_step_rows(*(args(2)[:-1] + (z(1, torch.int32),)))           # one counter for two detections
    with pytest.raises(L2SError):
        O.decode_beam_step_rows(*args(9))                          # more beams than words
    with pytest.raises(L2SError):
        O.decode_beam_step_rows(*args(2, t=4))                     # t beyond T - 1
    with pytest.raises(ValueError, match='--beam_size'):
        O.decode_beam_finish_rows(z(8, torch.int32), z(1, torch.int32), 17, 4, 1, z(8, torch.int64), z(8), z(8), z(1, torch.int32), z(8, torch.int64), z(8))
    with pytest.raises(ValueError, match='--beam_size'):
        O.decode_beam_finish_rows(z(8, torch.int32), z(1, torch.int32), 1, 65, 1, z(8, torch.int64), z(8), z(8), z(1, torch.int32), z(8, torch.int64), z(8))
    assert O.last_kernel() == before


# ------------------------------------------------------------------ 2. the final ordering
@pytest.mark.parametrize('B', [1, 2, 3, 16])
@pytest.mark.parametrize('T', [1, 6, 64])
def test_beam_finish_rows_equals_a_stable_sort(B, T):
    """done_count in {0, 1, B - 1, B, B * T}, p drawn from five values (equal p: completion order decides) of which two are -1000 beams,
    zeros inside the sequences; two dead rows between sentinels"""
    O = ops()
    rs = np.random.RandomState(100 * B + T)
    RW, live, rows = O.beam_record_words(T), 5, 7
    done = np.zeros((rows, B * T, RW), np.int32)
    done[:, :, :T] = rs.randint(0, 6, (rows, B * T, T))
    done[:, :, T:2 * T] = (-rs.rand(rows, B * T, T).astype(np.float32) * 4).view(np.int32)
    done[:, :, 2 * T] = rs.choice(np.asarray([-0.5, -1.25, -3.0, -1000.75, -1002.5], np.float32), (rows, B * T)).view(np.int32)
    done[:, :, 2 * T + 1] = np.arange(B * T)[None]
    cnt = np.asarray([0, 1, B - 1, B, B * T, B, 1], np.int32)
    want = BU.finish_rows(done[:live], cnt[:live], B, T)
    got = dict(seq=torch.full((rows, T), -7, dtype=torch.int64, device=DEV), logprobs=torch.full((rows, T), 7.0, device=DEV),
               beam_seq=torch.full((rows, B, T), -7, dtype=torch.int64, device=DEV), beam_logprobs=torch.full((rows, B, T), 7.0, device=DEV),
               beam_p=torch.full((rows, B), 7.0, device=DEV), beam_n=torch.full((rows,), -7, dtype=torch.int32, device=DEV))
    for row0, count in ((0, live), (3, live + 3)):
        start = {k: v.clone() for k, v in got.items()}
        O.decode_beam_finish_rows(dev(done), dev(cnt), B, T, rows, got['beam_seq'], got['beam_logprobs'], got['beam_p'], got['beam_n'], got['seq'],
                                  got['logprobs'], count_of(count), row0)
        assert O.last_kernel() == 'decode_beam_finish_rows_kernel'
        for k, w in want.items():
            g = got[k].cpu().numpy()
            assert g.dtype == w.dtype and np.array_equal(g[:live].view(np.uint8), w.view(np.uint8)), (k, B, T, g[:live], w)
            assert same_bits(got[k][live:], start[k][live:]), (k, 'a dead row was written')
    assert want['beam_n'].tolist() == [0, min(1, B), B - 1, B, B]


# ------------------------------------------------------------------ 3. the step on groups
GROUP_COUNTS = [(0, None), (3, 'dets'), (0, 2), (0, 0)]


def _rep(a, group):
    return a.repeat_interleave(group, 0).contiguous()


@pytest.mark.parametrize('group', [1, 2, 3, 16])
@pytest.mark.parametrize('dets', [1, 5, 65])
def test_grouped_attention_equals_the_rows_entries_on_replicated_operands(group, dets):
    """l2s_cap_att_dots_groups, l2s_cap_apply_gates_groups, l2s_cap_att_apply_groups: state row r reads detection r // group's patt, P, att"""
    O = ops()
    Lr, AH, R = 37, 72, 24
    rows = dets * group
    rs = np.random.RandomState(group * 100 + dets)
    f = lambda *shp: dev(rs.normal(0, 1, shp).astype(np.float32))
    patt, P, att = f(dets, Lr, AH), f(dets, Lr, 2 * R), f(dets, Lr, R)
    att_h, aw, ab, b_a2c, sums, c_prev = f(rows, AH), f(AH), f(1), f(2 * R), f(rows, 5 * R), f(rows, R)
    patt_r, P_r, att_r = _rep(patt, group), _rep(P, group), _rep(att, group)
    for row0, count in GROUP_COUNTS:
        count = dets if count == 'dets' else count
        live = _live(dets, row0, count) * group
        flat = count_of(None if count is None else live)           # the rows entries on the replicated operands: row0 = 0, live state rows
        new = lambda *shp: (torch.full(shp, 7.0, device=DEV), torch.full(shp, 7.0, device=DEV))
        d0, d1 = new(rows, 256)
        O.cap_att_dots_groups(patt, att_h, aw, ab, rows, group, Lr, AH, d0, count_of(count), row0)
        assert O.last_kernel() == 'cap_att_dots_groups_kernel'
        O.cap_att_dots_rows(patt_r, att_h, aw, ab, rows, Lr, AH, d1, flat, 0)
        assert same_bits(d0, d1) and (d0[live:] == 7.0).all() and (live == 0 or (d0[:live, :Lr] != 7.0).any())
        (c0, c1), (h0, h1) = new(rows, R), new(rows, R)
        O.cap_apply_gates_groups(P, d0, b_a2c, sums, c_prev, c0, h0, rows, group, Lr, R, count_of(count), row0)
        assert O.last_kernel() == 'cap_apply_gates_groups_kernel'
        O.cap_apply_gates_rows(P_r, d1, b_a2c, sums, c_prev, c1, h1, rows, Lr, R, flat, 0)
        assert same_bits(c0, c1) and same_bits(h0, h1) and (h0[live:] == 7.0).all() and (live == 0 or (h0[:live] != 7.0).any())
        r0, r1 = new(rows, 2 * R)
        O.cap_att_apply_groups(att, d0, r0, rows, group, Lr, R, count_of(count), row0, ld_res=2 * R)
        assert O.last_kernel() == 'cap_att_apply_groups_kernel'
        O.cap_att_apply_rows(att_r, d1, r1, rows, Lr, R, flat, 0, ld_res=2 * R)
        assert same_bits(r0, r1) and (r0[live:] == 7.0).all() and (r0[:, R:] == 7.0).all() and (live == 0 or (r0[:live, :R] != 7.0).any())
    with pytest.raises(ValueError, match='group'):
        O.cap_att_dots_groups(patt, att_h, aw, ab, rows + 1, 2, Lr, AH, d0)


@pytest.mark.parametrize('group', [1, 2, 3, 16])
@pytest.mark.parametrize('dets', [1, 5, 65])
def test_grouped_cell_equals_the_rows_cell_on_a_replicated_fcrow(group, dets):
    """l2s_lstm_cell_groups: pre2 (the per-detection fcrow) is read at row r // group, everything else per state row; both MFMA tilings
    (rows <= 16 and beyond) and both load forms (R = 24: float4; R = 6, n = 5: scalar)"""
    O = ops()
    rows = dets * group
    rs = np.random.RandomState(group * 10 + dets)
    f = lambda *shp: dev(rs.normal(0, 1, shp).astype(np.float32))
    for R, n0, n1 in ((24, 24, 20), (6, 5, 6)):
        pre, pre2, add0, x0, x1 = f(rows, 4 * R), f(dets, 4 * R), f(4 * R), f(rows, n0), f(rows, 2 * R)
        w0, w1, c_prev = f(4 * R, n0 + 4), f(4 * R, n1), f(rows, R)          # (w0: a column block of a wider matrix)
        segs = [(x0, n0, w0, n0 + 4, n0), (x1, 2 * R, w1, n1, n1)]
        pre2_r = _rep(pre2, group)
        for row0, count in GROUP_COUNTS:
            count = dets if count == 'dets' else count
            live = _live(dets, row0, count) * group
            flat = count_of(None if count is None else live)
            c0, c1, h0, h1 = (torch.full((rows, s), 7.0, device=DEV) for s in (R, R, 2 * R, 2 * R))
            O.lstm_cell_groups(pre, add0, None, segs, c_prev, c0, h0.view(-1)[R:], rows, group, R, count_of(count), row0, pre2=pre2, ld_h=2 * R)
            assert O.last_kernel().startswith('lstm_cell_rows_kernel<')
            O.lstm_cell_rows(pre, add0, None, segs, c_prev, c1, h1.view(-1)[R:], rows, R, flat, 0, pre2=pre2_r, ld_h=2 * R)
            assert same_bits(c0, c1) and same_bits(h0, h1) and (c0[live:] == 7.0).all() and (h0[:, :R] == 7.0).all()
            assert live == 0 or ((c0[:live] != 7.0).all() and (h0[:live, R:] != 7.0).all())


# ------------------------------------------------------------------ 4. the fixture through a network
_NETS = {}
_RUNS = {}


def _opt(model, fopt):
    from oracle import weights as OW
    opt = OW.default_opt(vocab_size=fopt['vocab_size'], seq_length=fopt['seq_length'])
    opt.update(fopt)
    opt['caption_model'] = model
    return opt


def _fixture_net(model):
    """a ResNet-50 cycle network in f32 whose captioner is the fixture's (as tests/test_caprows_gpu.py builds it); cached"""
    if model not in _NETS:
        from lang2seg_amd import selftest
        fopt, w, fc, att, g = CU.fixture(model)
        net = selftest.build_net(_opt(model, fopt), {}, 'f32', None, num_layers=50)
        net.load_state_dict({CAP + k: v for k, v in w.items()})
        net.eval()
        net.parity = None
        _NETS[model] = (net, dev(fc), dev(att))
    return _NETS[model]


def _host(r):
    return {k: v.cpu().numpy().copy() for k, v in r.items()}


def _route(model, B, batched, count=None):
    """caption_beam_rows on the fixture's 5 rows by one route, as host arrays; computed once per (model, B, route, count)"""
    key = (model, B, batched, count)
    if key not in _RUNS:
        from lang2seg_amd.nets import caption_rows
        net, fc, att = _fixture_net(model)
        net.rows_batched = batched
        try:
            assert caption_rows.batched(net) == batched
            _RUNS[key] = _host(net.caption_beam_rows(att, fc, rows=5, count=count_of(count), beam_size=B))
        finally:
            net.rows_batched = True
    return _RUNS[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize('B', [2, 3, 5])
@pytest.mark.parametrize('model', CU.MODELS)
def test_loop_route_is_caption_decode_row_by_row(model, B):
    """all B beams of every row: the tokens, the order and the bits of Network.caption_decode(beam_size=B), by the same launches"""
    net, fc, att = _fixture_net(model)
    T = net.opt['seq_length']
    r = _route(model, B, False)
    assert r['seq'].dtype == np.int64 and r['beam_seq'].shape == (5, B, T) and r['beam_p'].shape == (5, B) and r['beam_n'].tolist() == [B] * 5
    for k in range(5):
        one = net.caption_decode(att[k], fc[k], beam_size=B)
        assert len(one['beams']) == B
        for v, b in enumerate(one['beams']):
            assert r['beam_seq'][k, v].tolist() == b['seq'], (k, v)
            assert np.array_equal(_bits(r['beam_logprobs'][k, v]), _bits(np.asarray(b['logps'], np.float32)))
            assert np.array_equal(_bits(r['beam_p'][k, v:v + 1]), _bits(np.asarray([b['p']], np.float32)))
        n = len(one['seq'])
        assert r['seq'][k, :n].tolist() == one['seq'] and (r['seq'][k, n:] == 0).all()
        assert np.array_equal(_bits(r['logprobs'][k, :n]), _bits(np.asarray(one['logprobs'], np.float32))) and (r['logprobs'][k, n + 1:] == 0).all()
    net.rows_batched = False
    try:
        net.caption_beam_rows(att[:1], fc[:1], rows=1, beam_size=B)      # (a buffer's first use allocates it zeroed instead of clearing it)
        loop = _calls(lambda: net.caption_beam_rows(att[:1], fc[:1], rows=1, beam_size=B))
    finally:
        net.rows_batched = True
    single = _calls(lambda: net.caption_decode(att[0], fc[0], beam_size=B))
    j = next(i for i, (x, y) in enumerate(zip(loop, single)) if x != y)
    assert loop[j] == 'l2s_memset_async' and loop[-1] == 'l2s_decode_beam_finish_rows'      # + the outputs' clear (ahead of the head), + the ordering
    assert loop[:j] + loop[j + 1:-1] == single and 'l2s_decode_beam_step' in single


@pytest.mark.parametrize('B', [2, 3, 5])
@pytest.mark.parametrize('model', CU.MODELS)
def test_batched_route_equals_the_loop_route(model, B):
    """every token of every beam; logps and p within 1e-5 absolute, next to -1000 by bits; and the CPU restatement's tokens"""
    a, b = _route(model, B, True), _route(model, B, False)
    want, _, margin = BU.beam_rows(CU.drivers(model), a['seq'].shape[1], B)
    assert min(margin) > 1e-4
    worst = 0.0
    for k in ('seq', 'beam_seq', 'beam_n'):
        assert np.array_equal(a[k], b[k]), (k, a[k], b[k])
        assert np.array_equal(a[k], want[k]), (k, a[k], want[k])
    for k in ('logprobs', 'beam_logprobs', 'beam_p'):
        big = np.abs(b[k]) >= 900
        assert np.array_equal(_bits(a[k][big]), _bits(b[k][big])), (k, a[k][big], b[k][big])
        e = float(np.abs(a[k][~big].astype(np.float64) - b[k][~big]).max(initial=0.0))
        worst = max(worst, e)
        assert e <= TOL, (k, e)
        assert float(np.abs(a[k][~big].astype(np.float64) - want[k][~big]).max(initial=0.0)) <= 10 * TOL      # (the restatement: test_decode_gpu's P_TOL)
    print('%s B = %d batched vs loop: worst %.2e absolute' % (model, B, worst))


@pytest.mark.parametrize('model', CU.MODELS)
def test_one_beam_carries_the_greedy_tokens(model):
    net, fc, att = _fixture_net(model)
    greedy = net.caption_decode_rows(att, fc, rows=5)['seq'].cpu().numpy().copy()
    for batched in (True, False):
        r = _route(model, 1, batched)
        assert np.array_equal(r['seq'], greedy), (batched, r['seq'], greedy)
        assert r['beam_n'].tolist() == [1] * 5


@pytest.mark.parametrize('count', [0, 2, 5])
@pytest.mark.parametrize('model', CU.MODELS)
def test_routes_agree_under_a_count_and_dead_rows_are_zero(model, count):
    full = _route(model, 3, True)
    a, b = _route(model, 3, True, count), _route(model, 3, False, count)
    for k in a:
        assert np.array_equal(_bits(a[k][:count]), _bits(full[k][:count])), k
        assert not a[k][count:].any() and not b[k][count:].any(), k
        if a[k].dtype == np.float32:
            big = np.abs(b[k]) >= 900
            assert np.array_equal(_bits(a[k][big]), _bits(b[k][big])) and np.abs(a[k][~big] - b[k][~big]).max(initial=0.0) <= TOL
        else:
            assert np.array_equal(a[k], b[k])


@pytest.mark.parametrize('model', CU.MODELS)
def test_batched_route_launches_do_not_depend_on_count_and_nothing_comes_back(model):
    net, fc, att = _fixture_net(model)
    rs = np.random.RandomState(3)
    att65 = dev(rs.normal(0, 1, (65, L, net.opt['att_feat_size'])).astype(np.float32))
    fc65 = dev(rs.normal(0, 1, (65, net.opt['fc_feat_size'])).astype(np.float32))
    T, B = net.opt['seq_length'], 3
    run = lambda n: net.caption_beam_rows(att65, fc65, rows=65, count=count_of(n), beam_size=B)
    run(65)                                                       # (a buffer's first use allocates it zeroed instead of clearing it)
    c2, c65 = count_of(2), count_of(65)
    a = _calls(lambda: net.caption_beam_rows(att65, fc65, rows=65, count=c2, beam_size=B))
    s2 = _host(run(2))
    b = _calls(lambda: net.caption_beam_rows(att65, fc65, rows=65, count=c65, beam_size=B))
    s65 = _host(run(65))
    assert a == b and len(a) > 0
    assert a.count('l2s_decode_beam_step_rows') == 2 * T and a.count('l2s_decode_beam_finish_rows') == 2      # two chunks
    grouped = ('l2s_cap_att_dots_groups', 'l2s_cap_apply_gates_groups') if model == 'att2in2' else \
        ('l2s_cap_att_dots_groups', 'l2s_cap_att_apply_groups', 'l2s_lstm_cell_groups')
    assert all(a.count(n) == 2 * T * (2 if n == 'l2s_lstm_cell_groups' else 1) for n in grouped)
    assert not {'l2s_decode_beam_step', 'l2s_decode_pick_rows', 'l2s_cap_att_dots_rows', 'l2s_lstm_cell_rows'} & set(a)
    print('%s beam rows, 65 rows (two chunks), B = 3: %d C-ABI calls, %d beam steps' % (model, len(a), a.count('l2s_decode_beam_step_rows')))
    assert _read_backs(lambda: net.caption_beam_rows(att65, fc65, rows=65, count=c2, beam_size=B)) == 0
    for k in s2:
        assert np.array_equal(_bits(s2[k][:2]), _bits(s65[k][:2])) and not s2[k][2:].any(), k
    assert (s65['beam_n'] == B).all() and (s65['beam_p'][:, 0] < 0).all()                                      # (row 64: the second chunk)
    assert not set(_calls(lambda: net.caption_decode_rows(att65, fc65, rows=65, count=c2))) & set(NEW_ENTRIES)  # the greedy path: none of them


# ------------------------------------------------------------------ 5. the detection dicts
_FEAT = {}
CAPTION_FIELDS = ('caption_tokens', 'caption_logprobs', 'caption')


def _feature_net():
    if 'cycle' not in _FEAT:
        from lang2seg_amd import selftest
        from oracle import synth as OS
        from topdown_util import td_opt, make_sd
        opt = td_opt(word_drop_out=0.0, rnn_drop_out=0.0)
        over = dict(BATCH_SIZE=16, RPN_PRE_NMS_TOP_N=600, RPN_POST_NMS_TOP_N=100, RPN_BATCHSIZE=64)
        net = selftest.build_net(opt, over, 'f32', make_sd(opt, seed=3, variant='cycle'), num_layers=50, variant='cycle')
        _FEAT['cycle'] = (net, OS.make_blob(160, 224, 6, 60, seed=5))
    return _FEAT['cycle']


def _first0(s):
    s = np.asarray(s)
    return int(np.argmax(s == 0)) if (s == 0).any() else s.size


def _check_beams(q, T, V):
    beams = q['caption_beams']
    assert 1 <= len(beams) <= 3 and all(set(b) == {'seq', 'logps', 'p'} and len(b['seq']) == len(b['logps']) == T for b in beams)
    assert [b['p'] for b in beams] == sorted((b['p'] for b in beams), reverse=True)
    assert beams[0]['seq'][:_first0(beams[0]['seq'])] == q['caption_tokens'] and all(1 <= w <= V for w in q['caption_tokens'])
    assert q['caption_logprobs'] == beams[0]['logps'][:len(q['caption_tokens'])]


def test_detect_image_describes_every_detection_by_beam_search():
    from lang2seg_amd.model import detect_device as DD
    net, blob = _feature_net()
    V, T = net.opt['vocab_size'], net.opt['seq_length']
    labels = np.asarray(blob['labels'])
    data = dict(data=blob['data'], im_info=blob['im_info'], file_name='synthetic.jpg')
    words = {str(i): 'w%d' % i for i in range(1, V + 1)}
    greedy = DD.detect_image(net, dict(data), labels, describe=True, ix_to_word=words)
    # beam_size = 1: today's path and launches
    one_calls = _calls(lambda: DD.detect_image(net, dict(data), labels, describe=True, ix_to_word=words, beam_size=1))
    assert one_calls == _calls(lambda: DD.detect_image(net, dict(data), labels, describe=True, ix_to_word=words)) and not set(one_calls) & set(NEW_ENTRIES)
    print('detect_image(describe=True) on the tiny cycle network: %d C-ABI calls' % len(one_calls))
    assert len(one_calls) == PARENT_CALLS_DESCRIBE
    assert DD.detect_image(net, dict(data), labels, describe=True, ix_to_word=words, beam_size=1) == greedy
    rich = DD.detect_image(net, dict(data), labels, describe=True, ix_to_word=words, beam_size=3)
    assert len(rich) == len(greedy) == labels.shape[0] and sum(len(l) for l in greedy) > 0
    for lg, lr in zip(greedy, rich):
        assert len(lg) == len(lr)
        for p, q in zip(lg, lr):
            assert {k: q[k] for k in p if k not in CAPTION_FIELDS} == {k: p[k] for k in p if k not in CAPTION_FIELDS}      # every other field keeps its bits
            assert set(q) - set(p) == {'caption_beams'}
            _check_beams(q, T, V)
            assert q['caption'] == ' '.join('w%d' % w for w in q['caption_tokens'])
    # every sentence once more on its own, so that its canvases and TEST forward are still the network's: each detection of each sentence
    # through the single-mask path
    cap = DD.default_cap(100)
    _, ih, iw = DD.ED._geometry(np.asarray(blob['im_info'], np.float32).reshape(-1)[:3])
    worst, n_all = 0.0, 0
    for i in range(labels.shape[0]):
        alone = DD.detect_image(net, dict(data), labels[i:i + 1], describe=True, ix_to_word=words, beam_size=3)[0]
        n_det = len(alone)
        assert n_det == len(rich[i])
        for p, q in zip(alone, rich[i]):
            assert [b['seq'] for b in p['caption_beams']] == [b['seq'] for b in q['caption_beams']] and p['segmentation'] == q['segmentation']
        if n_det == 0:
            continue
        canvases = net.buf('det.canvases', (cap, ih, iw), torch.uint8)
        att, fc = net.caption_features_rows(canvases, cap, (ih, iw), count=count_of(n_det))
        att, fc = att.clone(), fc.clone()
        for k in range(n_det):
            one = net.caption_decode(att[k], fc[k], beam_size=3)
            got = rich[i][k]['caption_beams']
            assert [b['seq'] for b in got] == [b['seq'] for b in one['beams']], (i, k, got, one['beams'])
            assert rich[i][k]['caption_tokens'] == one['seq']
            worst = max(worst, max(abs(a['p'] - b['p']) for a, b in zip(got, one['beams'])))
        n_all += n_det
    print('detect_image beams vs caption_decode(beam_size=3) per detection: p within %.2e (%d detections)' % (worst, n_all))
    assert worst <= TOL and n_all == sum(len(l) for l in rich) > 0
    # a sentence that reruns with larger buffers reruns its stage
    again = DD.detect_image(net, dict(data), labels, describe=True, ix_to_word=words, beam_size=3, _cap=1)
    assert [len(l) for l in again] == [len(l) for l in rich] and max(len(l) for l in rich) > 1
    for la, lr in zip(again, rich):
        for p, q in zip(la, lr):
            assert p['caption_tokens'] == q['caption_tokens'] and [b['seq'] for b in p['caption_beams']] == [b['seq'] for b in q['caption_beams']]
    with pytest.raises(ValueError, match='--beam_size'):
        DD.detect_image(net, dict(data), labels, describe=True, beam_size=17)


class _OneImageLoader(object):
    """getTestBatch over one blob"""

    def __init__(self, blob):
        self.blob, self.split_ix, self.iterators = blob, {'val': [0]}, {'val': 0}

    def getTestBatch(self, split, stride=1):
        return dict(self.blob, bounds=dict(it_pos_now=1, it_max=1, wrapped=True))


def test_eval_split_device_dumps_the_beams():
    from lang2seg_amd.loaders.synthetic_loader import SyntheticLoader
    from lang2seg_amd.model import detect_device as DD
    from lang2seg_amd.model.eval_device import eval_split_device
    net, _ = _feature_net()
    V, T = net.opt['vocab_size'], net.opt['seq_length']
    b = SyntheticLoader(num_images=1, sents_per_image=2, H=160, W=224, T=6, vocab_size=60, seed=3)._image(0)
    blob = {k: v for k, v in b.items() if k in ('data', 'im_info', 'gt_boxes', 'gt_masks', 'labels', 'file_name')}
    greedy, rich = [], []
    res0 = eval_split_device(_OneImageLoader(blob), net, None, 'val', dict(verbose=False), detections=greedy, describe=True)
    res1 = eval_split_device(_OneImageLoader(blob), net, None, 'val', dict(verbose=False), detections=rich, describe=True, beam_size=3)
    assert res0[0] == res1[0] and res0[4:] == res1[4:] and len(greedy) == len(rich) > 0        # the metrics do not depend on it
    direct = DD.detect_image(net, dict(data=blob['data'], im_info=blob['im_info'], file_name=blob.get('file_name')), np.asarray(blob['labels']),
                             describe=True, beam_size=3)
    flat = [p for lst in direct for p in lst]
    assert len(flat) == len(rich)
    for p, q, d in zip(greedy, rich, flat):
        assert {k: q[k] for k in p if k not in CAPTION_FIELDS} == {k: p[k] for k in p if k not in CAPTION_FIELDS} and set(q) - set(p) == {'caption_beams'}
        _check_beams(q, T, V)
        assert [x['seq'] for x in q['caption_beams']] == [x['seq'] for x in d['caption_beams']] and q['caption_tokens'] == d['caption_tokens']
        assert max(abs(x['p'] - y['p']) for x, y in zip(q['caption_beams'], d['caption_beams'])) <= TOL       # the same as detect_image writes


def test_predict_tool_prints_the_beams(capsys):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    try:
        import predict
    finally:
        sys.path.pop(0)
    common = ['--synthetic', '1', '--allow_init_weights', '1', '--output_postfix', 'no_such_run', '--cfg', '']
    capsys.readouterr()
    dets = predict.main(predict.parse_args(common + ['--all_detections', '1', '--describe', '1', '--beam_size', '3', '--max_per_image', '70']))
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(dets) == len(printed) == 3 and sum(len(l) for l in dets) > 0
    for lst, plst in zip(dets, printed):
        for p, q in zip(lst, plst):
            _check_beams(p, len(p['caption_beams'][0]['seq']), 1999)
            assert [b['seq'] for b in q['caption_beams']] == [b['seq'] for b in p['caption_beams']] and q['caption'] == p['caption']
    capsys.readouterr()
    plain = predict.main(predict.parse_args(common + ['--all_detections', '1', '--beam_size', '3', '--max_per_image', '70']))
    assert all('caption_beams' not in p and 'caption_tokens' not in p for lst in plain for p in lst)       # without --describe: no effect
