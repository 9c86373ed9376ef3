"""Shared by tests/test_caprows_topdown_{cpu,gpu}.py: the two kernels of the top-down step on rows (csrc/caption_rows.hip) restated in
float64 numpy, and the stub network that nets/caption_rows.py's `batched` is asked about."""
import numpy as np

f64 = np.float64


def sigm(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_cell_rows(pre, pre2, add0, add1, segs, c_prev):
    """one nn.LSTMCell step per row, gate order i, f, g, o.  pre / pre2: None, [4R] (one row for all rows) or [rows][4R]; add0 / add1: None
    or [4R]; segs: [(x [rows][n], w [4R][n])]; c_prev [rows][R] -> (c, h) float64 [rows][R]"""
    c_prev = np.asarray(c_prev, f64)
    rows, R = c_prev.shape
    g = np.zeros((rows, 4 * R), f64)
    for x, w in segs:
        g += np.asarray(x, f64) @ np.asarray(w, f64).T
    for a in (pre, pre2, add0, add1):
        if a is not None:
            g += np.asarray(a, f64).reshape(-1, 4 * R)              # (one row broadcasts)
    i, f, gg, o = sigm(g[:, :R]), sigm(g[:, R:2 * R]), np.tanh(g[:, 2 * R:3 * R]), sigm(g[:, 3 * R:])
    c = f * c_prev + i * gg
    return c, o * np.tanh(c)


def att_apply_rows(att, dots):
    """att [rows][L][R], dots [rows][L] -> att_res float64 [rows][R] = softmax(dots[r]) . att[r]"""
    att, d = np.asarray(att, f64), np.asarray(dots, f64)
    e = np.exp(d - d.max(1, keepdims=True))
    w = e / e.sum(1, keepdims=True)
    return np.einsum('rl,rld->rd', w, att)


class StubNet(object):
    """what `batched` reads of a network: the captioner (a real one of nets/captioners.py on this stub), the options, the switches"""

    def __init__(self, model, rnn_size, projected=True, rows_batched=None):
        from lang2seg_amd.nets.captioners import CAPTIONERS
        self.cap_model = model
        self.opt = dict(rnn_size=rnn_size, input_encoding_size=rnn_size, att_hid_size=rnn_size)
        self.cap_projected = projected
        if rows_batched is not None:
            self.rows_batched = rows_batched
        self.captioner = CAPTIONERS[model](self)
