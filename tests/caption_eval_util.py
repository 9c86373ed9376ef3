"""Shared by tests/test_caption_eval_{cpu,gpu}.py: teacher forcing with a token row per row restated in float64 numpy - the kernel
(l2s_decode_force_rows: log-softmax, the gather at the row's own target, the length mask, the running sum, the next input) and the whole
of Network.caption_score_pairs on tests/decode_util.py's RefDriver (one per row, as tests/caprows_util.py scores one expression) - and the
reference's criterion, lib/misc/utils.py LanguageModelCriterion: sum(-logprob * mask) / sum(mask)."""
import numpy as np

f64, f32 = np.float64, np.float32
FWD_TOL = 1e-5            # tests/test_caprows_gpu.py's bound of a forced log-probability


def targets_of(tokens, lengths=None):
    """tokens int [rows][Tmax], zero padded -> (targets int64 [rows][Tmax + 1]: w_1 .. w_n, 0, zeros; ntok int64 [rows] = n + 1)"""
    tok = np.asarray(tokens, np.int64)
    n = (tok != 0).sum(1) if lengths is None else np.asarray(lengths, np.int64)
    tgt = np.zeros((tok.shape[0], tok.shape[1] + 1), np.int64)
    for r in range(tok.shape[0]):
        tgt[r, :n[r]] = tok[r, :n[r]]
    return tgt, n + 1


def log_softmax64(x):
    x = np.asarray(x, f64)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


def force_step(logits, targets, ntok, t, logprobs, score, next_token, live=None, mask_shift=0, target_shift=0):
    """one launch of the kernel on float64 [rows][V1] logits, in place on logprobs [rows][T], score [rows], next_token [rows]; live: the
    rows below count (None: all).  mask_shift / target_shift: the misplaced terms of the mutation checks (0: the kernel)"""
    rows, T = targets.shape
    lsm = log_softmax64(logits)
    for r in range(rows if live is None else min(rows, max(live, 0))):
        if t + mask_shift < ntok[r]:
            k = int(targets[r, min(t + target_shift, T - 1)])
            logprobs[r, t] = lsm[r, k]
            score[r] = lsm[r, k] if t == 0 else score[r] + lsm[r, k]
            next_token[r] = k
        else:
            next_token[r] = 0


def force_rows(logits, targets, ntok, live=None, **mut):
    """all T launches on logits [T][rows][V1] -> (logprobs f64 [rows][T], score f64 [rows], the next tokens after every step [T][rows])"""
    rows, T = targets.shape
    lps, score, tok = np.zeros((rows, T), f64), np.zeros((rows,), f64), np.zeros((rows,), np.int64)
    toks = []
    for t in range(T):
        force_step(logits[t], targets, ntok, t, lps, score, tok, live, **mut)
        toks.append(tok.copy())
    return lps, score, np.asarray(toks)


def criterion(logprobs, ntok):
    """LanguageModelCriterion on a batch whose gathered log-probabilities are logprobs [rows][T]: the mask of row r is its first ntok[r]
    positions (the tokens and the end token)"""
    lp = np.asarray(logprobs, f64)
    mask = (np.arange(lp.shape[1])[None, :] < np.asarray(ntok)[:, None]).astype(f64)
    return float((-lp * mask).sum() / mask.sum())


def score_pairs(drv, tokens, lengths=None, drop_end=False):
    """the whole pairs scoring on one next_logprobs driver per row: row r is teacher-forced with the inputs [0, w_1 .. w_n] and the targets
    [w_1 .. w_n, 0] -> (logprobs f64 [rows][Tmax + 1], zero behind n + 1; score f64 [rows]; ntok).  drop_end: the mutation whose sum
    misses the end token"""
    tgt, ntok = targets_of(tokens, lengths)
    lps = np.zeros(tgt.shape, f64)
    for r, d in enumerate(drv):
        for t in range(int(ntok[r])):
            lps[r, t] = np.asarray(d(tuple(int(v) for v in tgt[r, :t])), f64)[int(tgt[r, t])]
    score = np.asarray([lps[r, :ntok[r] - (1 if drop_end else 0)].sum() for r in range(len(drv))], f64)
    return lps, score, ntok


def check_close(got, ref, what='log-probabilities'):
    """the elementwise bound of tests/test_caprows_gpu.py's forced log-probabilities: |got - ref| <= FWD_TOL * max(1, max |ref|)"""
    got, ref = np.asarray(got, f64), np.asarray(ref, f64)
    if got.shape != ref.shape:
        raise AssertionError('%s: shape %s against %s' % (what, got.shape, ref.shape))
    bound = FWD_TOL * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    err = np.abs(got - ref)
    if not (err <= bound).all():
        at = np.unravel_index(int(np.argmax(err)), err.shape)
        raise AssertionError('%s: |%r - %r| = %.3e > %.3e at %s' % (what, got[at], ref[at], err[at], bound, at))
    return float(err.max()) if err.size else 0.0
