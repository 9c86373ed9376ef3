"""Shared by tests/test_beamrows_{cpu,gpu}.py: beam search on rows restated in numpy - decode_util.beam_search per row (one RefDriver per
row, tests/caprows_util.py) and the final ordering of CaptionModel.py:123 - in the layout Network.caption_beam_rows returns, with the
margins of every decision; and the final ordering alone on raw records, the restatement of l2s_decode_beam_finish_rows."""
import numpy as np

import decode_util as DU

f32 = np.float32


def final_order(p, B):
    """the kept completions: by p descending, equal p in completion order (a stable sort), the first B"""
    return [int(i) for i in np.argsort(-np.asarray(p, f32), kind='stable')[:B]]


def best_layout(seq, logps):
    """the best beam as caption_decode_rows lays a row out: tokens up to the first 0, the 0's log-probability kept, zeros behind it"""
    seq, logps = np.asarray(seq, np.int64), np.asarray(logps, f32)
    T = seq.size
    n = int(np.argmax(seq == 0)) if (seq == 0).any() else T
    s, lp = np.zeros((T,), np.int64), np.zeros((T,), f32)
    s[:n] = seq[:n]
    lp[:min(n + 1, T)] = logps[:min(n + 1, T)]
    return s, lp


def finish_rows(done, done_count, B, T):
    """done int32 [rows][B * T][2 T + 2], done_count [rows] -> the six arrays of l2s_decode_beam_finish_rows, every row live"""
    rows = done.shape[0]
    out = dict(seq=np.zeros((rows, T), np.int64), logprobs=np.zeros((rows, T), f32), beam_seq=np.zeros((rows, B, T), np.int64),
               beam_logprobs=np.zeros((rows, B, T), f32), beam_p=np.zeros((rows, B), f32), beam_n=np.zeros((rows,), np.int32))
    for d in range(rows):
        n = max(0, min(int(done_count[d]), B * T))
        rec = done[d, :n]
        keep = final_order(rec[:, 2 * T].copy().view(f32), B)
        out['beam_n'][d] = len(keep)
        for v, i in enumerate(keep):
            out['beam_seq'][d, v] = rec[i, :T]
            out['beam_logprobs'][d, v] = rec[i, T:2 * T].copy().view(f32)
            out['beam_p'][d, v] = rec[i, 2 * T:2 * T + 1].copy().view(f32)[0]
        if keep:
            out['seq'][d], out['logprobs'][d] = best_layout(out['beam_seq'][d, 0], out['beam_logprobs'][d, 0])
    return out


def beam_rows(drivers, T, B):
    """decode_util.beam_search per row, then the final ordering -> (the arrays of caption_beam_rows, per row the completion indices of its
    kept beams, per row the margin: the smallest gap between consecutive candidates among the best B + 1 at any step and between
    consecutive completions among the best B + 1 of the final order)"""
    N = len(drivers)
    out = dict(seq=np.zeros((N, T), np.int64), logprobs=np.zeros((N, T), f32), beam_seq=np.zeros((N, B, T), np.int64),
               beam_logprobs=np.zeros((N, B, T), f32), beam_p=np.zeros((N, B), f32), beam_n=np.zeros((N,), np.int32))
    index, margin = [], []
    for r, drv in enumerate(drivers):
        beams, every, gaps = DU.beam_search(drv, T, B)
        p = np.asarray([e['p'] for e in every], f32)
        keep = final_order(p, B)
        assert [b['index'] for b in beams] == keep                # (beam_search's own sorted(...)[:B] is that rule)
        top = np.sort(p.astype(np.float64))[::-1][:B + 1]
        margin.append(min([float(g) for g in gaps] + [float(a - b) for a, b in zip(top, top[1:])]))
        index.append(keep)
        out['beam_n'][r] = len(keep)
        for v, i in enumerate(keep):
            out['beam_seq'][r, v], out['beam_logprobs'][r, v], out['beam_p'][r, v] = every[i]['seq'], every[i]['logps'], every[i]['p']
        out['seq'][r], out['logprobs'][r] = best_layout(out['beam_seq'][r, 0], out['beam_logprobs'][r, 0])
    return out, index, margin
