"""The top-down captioner on the batched route of the caption branch on rows, without a device: which networks nets/caption_rows.py's
`batched` sends there, and the float64 restatements of the two row kernels (tests/caprows_topdown_util.py, the GPU tests' reference) held
against torch's own nn.LSTMCell and softmax in float64."""
import numpy as np
import pytest
import torch

import caprows_topdown_util as TU


def _batched(*a, **kw):
    from lang2seg_amd.nets import caption_rows
    return caption_rows.batched(TU.StubNet(*a, **kw))


def test_topdown_takes_the_batched_route():
    assert _batched('topdown', 512) is True
    assert _batched('topdown', 1024) is True
    assert _batched('topdown', 512, rows_batched=False) is False
    assert _batched('topdown', 1028) is False


@pytest.mark.parametrize('model', ['adaatt', 'adaattmo'])
def test_adaptive_attention_stays_on_the_loop(model):
    assert _batched(model, 512) is False


def test_att2in2_routes_as_before():
    assert _batched('att2in2', 512) is True
    assert _batched('att2in2', 512, projected=False) is False
    assert _batched('att2in2', 512, rows_batched=False) is False
    assert _batched('att2in2', 1028) is False


def test_lstm_cell_rows_restatement_equals_nn_lstmcell():
    R, K0, K1, rows = 12, 7, 12, 5
    torch.manual_seed(3)
    cell = torch.nn.LSTMCell(K0 + K1, R).double()
    x, h, c = torch.randn(rows, K0 + K1).double(), torch.randn(rows, R).double(), torch.randn(rows, R).double()
    h1, c1 = cell(x, (h, c))
    w_ih, w_hh = cell.weight_ih.detach().numpy(), cell.weight_hh.detach().numpy()
    # the K0 columns as a per-row addend, the K1 columns and the recurrent product as segments, the biases as add0 / add1
    pre = x[:, :K0].numpy() @ w_ih[:, :K0].T
    got_c, got_h = TU.lstm_cell_rows(pre, None, cell.bias_ih.detach().numpy(), cell.bias_hh.detach().numpy(),
                                     [(x[:, K0:].numpy(), w_ih[:, K0:]), (h.numpy(), w_hh)], c.numpy())
    assert np.abs(got_c - c1.detach().numpy()).max() < 1e-12 and np.abs(got_h - h1.detach().numpy()).max() < 1e-12
    # one `pre` row for all rows
    one_c, _ = TU.lstm_cell_rows(pre[2], None, None, None, [], c.numpy())
    all_c, _ = TU.lstm_cell_rows(np.repeat(pre[2:3], rows, 0), None, None, None, [], c.numpy())
    assert np.array_equal(one_c, all_c)


def test_att_apply_rows_restatement_equals_softmax_times_features():
    rs = np.random.RandomState(1)
    att, dots = rs.normal(0, 1, (3, 196, 20)), rs.normal(0, 2, (3, 196))
    want = torch.einsum('rl,rld->rd', torch.softmax(torch.from_numpy(dots), 1), torch.from_numpy(att)).numpy()
    assert np.abs(TU.att_apply_rows(att, dots) - want).max() < 1e-12
