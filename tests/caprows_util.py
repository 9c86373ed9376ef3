"""Shared by tests/test_caprows_{cpu,gpu}.py: the caption branch on rows restated in numpy - the masks at the map's size, the pooled rows,
the batched greedy loop with a finished flag per row and the teacher-forced score - on tests/decode_util.py's RefDriver (one per row), and
the reference fixture tests/golden/ref_caprows.npz (make_golden_caprows.py: the reference's own batch runs)."""
import os

import numpy as np

import decode_util as DU

f32 = np.float32
GOLD = os.path.join(DU.ROOT, 'tests', 'golden', 'ref_caprows.npz')
MODELS = ('att2in2', 'topdown')
_Z = {}


def fixture(model):
    """-> (opt, weights, fc_feats [5][64], att_feats [5][196][64], the recorded results) of one captioner"""
    if 'z' not in _Z:
        _Z['z'] = np.load(GOLD)
    z = _Z['z']
    g = {k[len(model) + 1:]: z[k] for k in z.files if k.startswith(model + '/')}
    opt = {k[4:]: int(v) for k, v in g.items() if k.startswith('opt.')}
    w = {k[2:]: v for k, v in g.items() if k.startswith('w.')}
    return opt, w, g['fc_feats'], g['att_feats'], g


def drivers(model):
    """one next_logprobs per fixture row; cached (the restatement runs once for all tests of a process)"""
    if ('drv', model) not in _Z:
        opt, w, fc, att, _ = fixture(model)
        _Z[('drv', model)] = [DU.RefDriver(model, opt, w, None if model == 'att2in2' else fc[r], att[r]) for r in range(att.shape[0])]
    return _Z[('drv', model)]


def bins(n_in, n_out):
    """adaptive pooling's [lo, hi) per output index"""
    return [((i * n_in) // n_out, ((i + 1) * n_in + n_out - 1) // n_out) for i in range(n_out)]


def masks_to_map(masks, H, W, Hc, Wc):
    """masks uint8 [rows][mh][mw] -> float32 {0,1} [rows][Hc * Wc]: PIL NEAREST to H x W (oracle.boxes), adaptive average, >= 0.5"""
    from oracle import boxes as OB
    out = np.zeros((masks.shape[0], Hc, Wc), f32)
    for r, m in enumerate(masks):
        big = m if m.shape == (H, W) else OB.imresize_nearest_u8(m, (H, W))
        for oy, (y0, y1) in enumerate(bins(H, Hc)):
            for ox, (x0, x1) in enumerate(bins(W, Wc)):
                blk = big[y0:y1, x0:x1]
                out[r, oy, ox] = 1.0 if f32(blk.sum()) / f32(blk.size) >= f32(0.5) else 0.0
    return out.reshape(masks.shape[0], Hc * Wc)


def adaptive_pool_rows(x, pm, rows, H, W, OH, OW):
    """x [H * W][C], pm [rows][H * W] or None -> float64 [rows][OH * OW][C]"""
    x = np.asarray(x, np.float64).reshape(H, W, -1)
    out = np.zeros((rows, OH * OW, x.shape[2]))
    for r in range(rows):
        v = x if pm is None else x * np.asarray(pm[r], np.float64).reshape(H, W, 1)
        for oy, (y0, y1) in enumerate(bins(H, OH)):
            for ox, (x0, x1) in enumerate(bins(W, OW)):
                out[r, oy * OW + ox] = v[y0:y1, x0:x1].reshape(-1, x.shape[2]).mean(0)
    return out


def greedy_rows(drv, T):
    """the batched greedy loop: every row steps T times; a finished flag per row: after its first 0 a row's tokens are 0 with
    log-probability 0 (the 0 itself carries its log-probability).  -> (seq int64 [N][T], logprobs f32 [N][T], the smallest top-two gap)"""
    N = len(drv)
    seq, lps, fin, gap = np.zeros((N, T), np.int64), np.zeros((N, T), f32), [False] * N, np.inf
    for t in range(T):
        for r in range(N):
            if fin[r]:
                continue
            lp = np.asarray(drv[r](tuple(int(v) for v in seq[r, :t])), f32)
            k = int(np.argmax(lp))
            s = np.sort(lp)[::-1]
            gap = min(gap, float(s[0] - s[1]))
            seq[r, t], lps[r, t] = k, lp[k]
            fin[r] = k == 0
    return seq, lps, gap


def score_rows(drv, tokens):
    """teacher forcing: inputs [0, w_1 .. w_n], targets [w_1 .. w_n, 0] -> (logprobs f32 [N][n + 1], their sums f32 [N], added left to right)"""
    toks = [int(v) for v in tokens]
    tgt = toks + [0]
    lps = np.zeros((len(drv), len(tgt)), f32)
    for r, d in enumerate(drv):
        for t, w in enumerate(tgt):
            lps[r, t] = np.asarray(d(tuple(toks[:t])), f32)[w]
    score = np.zeros((len(drv),), f32)
    for t in range(len(tgt)):
        score = (score + lps[:, t]).astype(f32)
    return lps, score
