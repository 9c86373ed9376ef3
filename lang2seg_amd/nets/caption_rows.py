"""The caption branch on rows: one row per detection of a sentence (model/detect_device.py hands over a sentence's canvases and the
detector's device count).  Network.caption_features_rows pools layer4 under every mask in one launch per pooling; caption_decode_rows
decodes every row greedily; caption_score_rows scores ONE expression, teacher-forced, under every row's mask: the log-likelihood the
cycle loss minimises for the ground-truth mask (AttModel.forward + a gather, LanguageModelCriterion's mask all ones).

Two routes:
  batched   att2in2 in the projected form and topdown (L = 196 <= 256, rnn_size <= 1024), each through its captioner's rows_* functions
            (nets/captioners.py); the logits and the decision (l2s_decode_pick_rows) are this file's.  Whatever `rows` and `count` are, the
            launches per token are the same, and `count` stays on the device.
              att2in2  the head as GEMMs on rows * 196 rows (att_embed, ctx2att, P = att . W_a2c^T), then per token [embedding, i2h]
                       (greedy; scoring does both once for all n + 1 inputs) -> h2h and h2att as row-batch Linears -> the row-strided
                       attention dots and softmax + gates (csrc/caption_step.hip: the train step's kernel bodies with a row index) ->
                       logits -> decision: 8 launches a token, 6 when scoring.
              topdown  the head: att_embed and ctx2att on rows * 196 rows, fc_embed and the fc product (fcrow [rows][4 rnn_size]) on rows;
                       per token [embedding, the xt columns of att_lstm.weight_ih] (greedy; once per call when scoring) -> the attention
                       cell (l2s_lstm_cell_rows: both products on MFMA tiles of rows and the cell in one launch) -> h2att -> attention
                       dots -> softmax + weighted sum (l2s_cap_att_apply_rows) -> the language cell (l2s_lstm_cell_rows) -> logits ->
                       decision: 9 launches a token, 7 when scoring.
  loop      adaatt / adaattmo, `net.rows_batched = False`, or shapes outside the limits: the single-mask launches of nets/decode.py row
            by row (head, decode_start, T x step), the decision by l2s_decode_pick_rows on one row.  Reads `count` back once per call.
            Slow (about rows * 3 T dependent launches, 5 T for topdown) but correct for every captioner, and the cross-check of the batched route.

caption_score_pairs scores row r's OWN expression (its own length) under row r's mask: the evaluation of the speaker on a split.  Its
batched route drives the captioner's rows_step the greedy way - the step's input is the token l2s_decode_force_rows left for the row, the
row's own target of the step before - so rows_step takes nothing new and the launches per token are the greedy ones with the new kernel in
place of the pick: att2in2 8, topdown 9, whatever `rows`, `count` and the lengths are (every chunk runs Tmax + 1 steps; a row behind its
length is fed 0 and writes nothing).  Its loop route is the single-mask launches row by row with the new kernel on one row.

Rows are processed in chunks of at most CHUNK = 64, so the head's products (a, patt, P: 196 * 64 rows of 4 rnn_size + att_hid_size floats;
topdown has no P) stay near 0.1 GB at the production widths beside the chunk's 0.1 GB of features.  Every buffer is `rows.*` (the loop also uses decoding's
`dec.*`): a call between a training forward and its backward leaves what that backward reads alone.  The results are the network's buffers:
valid until the next call."""
import numpy as np
import torch

from .. import ops as O
from . import decode

f32, i32, i64 = torch.float32, torch.int32, torch.int64
L = 196
CHUNK = 64


def check_features(net):
    """ValueErrors that name the variant: only the cycle network pools under a mask"""
    variant = getattr(net, 'variant', '?')
    if variant == 'vgg' or not getattr(net, 'layers', {}).get(4):
        raise ValueError('--variant %s: the VGG network has no caption branch, nothing to pool per detection (cycle has one)' % variant)
    if getattr(net, 'var', None) is None or net.var.get('cap') is None or not hasattr(net, 'att_embed'):
        raise ValueError('--variant %s has no caption branch: nothing to pool per detection (cycle has one)' % variant)
    if net.var['cap'] != 'mask':
        raise ValueError('--variant %s pools no mask (its caption features are the map before and after the gating): every detection would get '
                         'the same features; captions per detection need --variant cycle' % variant)


def caption_features_rows(net, masks, rows, shape, count=None):
    """masks uint8 [rows][mh][mw], shape = (mh, mw): any size, resized to the blob's by PIL NEAREST as the loader's masks are.
    -> (att_feats [rows][196][att_feat_size], fc_feats [rows][fc_feat_size] or None) of the sentence whose TEST forward ran last: one
    layer4 pass on the map, the masks at the map's size in one launch, one pooling launch per half.  count: device int32 [1], the live rows."""
    check_features(net)
    p = getattr(net, '_test_sentence', None)
    if p is None:
        raise RuntimeError('caption_features_rows follows forward_test_sentence: no TEST forward has run')
    rows, (mh, mw) = int(rows), (int(shape[0]), int(shape[1]))
    if rows < 1 or masks.dtype != torch.uint8 or masks.numel() != rows * mh * mw:
        raise ValueError('caption_features_rows: masks is uint8 [rows = %d][%d][%d]' % (rows, mh, mw))
    net_conv, (Hc, Wc), (H, W) = p['net_conv'], p['net_conv_hw'], p['blob_hw']
    AF, FC = net.opt['att_feat_size'], net.opt.get('fc_feat_size')
    feats = net._l4_on_map(net_conv, Hc, Wc, 'l4m')
    gm = net.buf('rows.gm', (rows, Hc * Wc), f32)
    O.masks_to_map(masks, rows, mh, mw, H, W, Hc, Wc, gm, count)
    att, fc = net.buf('rows.att', (rows, L, AF)), None
    for j, m in enumerate((None, gm)):
        O.adaptive_pool_rows(feats, m, att.view(-1)[2048 * j:], rows, Hc, Wc, 2048, 14, 14, AF, count)
    if net.captioner.reads_fc:
        if FC != 2 * 2048:
            raise ValueError('fc_feat_size %r: fc_feats is the pair of 2048-channel means of layer4 on the map (4096)' % (FC,))
        fc = net.buf('rows.fc', (rows, FC))
        for j, m in enumerate((None, gm)):
            O.adaptive_pool_rows(feats, m, fc.view(-1)[2048 * j:], rows, Hc, Wc, 2048, 1, 1, FC, count)
    return att, fc


def batched(net):
    """the batched route serves this network: its captioner has the step on rows (att2in2 in the projected form, topdown) and the shapes
    are inside the row kernels' limits (rnn_size <= 1024; L = 196 <= 256 always holds)"""
    return bool(getattr(net, 'rows_batched', True)) and bool(net.captioner.rows_ok())


def _start(net, what, att_feats, fc_feats, rows, count):
    decode.check_args(net, 1, 1, 1.0)
    if net.training:
        raise RuntimeError('%s runs in eval mode (net.eval()): the dropouts are off' % what)
    rows = int(rows)
    AF, FC = net.opt['att_feat_size'], net.opt.get('fc_feat_size')
    if rows < 1 or att_feats.numel() != rows * L * AF:
        raise ValueError('%s: att_feats has %d values, expected rows x 196 x att_feat_size = %d' % (what, att_feats.numel(), max(rows, 0) * L * AF))
    want = O.TORCH_DT[net.dt]
    if att_feats.dtype != want:
        raise ValueError('%s: att_feats is %s, the network computes in %s' % (what, att_feats.dtype, want))
    if net.captioner.reads_fc and (fc_feats is None or fc_feats.numel() != rows * FC):
        raise ValueError('%s: --caption_model %s reads fc_feats [rows][fc_feat_size = %d]' % (what, net.cap_model, FC))
    if count is not None and (count.dtype != i32 or count.numel() < 1):
        raise ValueError('%s: count is a device int32 [1]' % what)
    net.join_update()
    net.join_transposes()
    att = att_feats.contiguous().view(rows, L * AF)
    fc = fc_feats.contiguous().view(rows, FC) if net.captioner.reads_fc else None
    return rows, att, fc


def _outputs(net, rows, T):
    """seq int64 | log-probabilities f32 | their sums f32 in one zeroed buffer (a dead row reads as an empty sentence), and the flags"""
    out = net.buf('rows.out', (rows * (12 * T + 4),), torch.uint8, zero=True)
    seq = out[:8 * rows * T].view(i64).view(rows, T)
    lps = out[8 * rows * T:12 * rows * T].view(f32).view(rows, T)
    score = out[12 * rows * T:].view(f32)
    return seq, lps, score, net.buf('rows.finished', (rows,), i32)


def _run_batched(net, att, fc, rows, count, T, seq, lps, score, fin, inputs=None, targets=None):
    """inputs / targets: device int64 [T] for teacher forcing (None: greedy).  The captioner's rows_* functions (nets/captioners.py) issue
    its head and its token step; the logits and the decision are every captioner's"""
    cap = net.captioner
    R, V1 = net.opt['rnn_size'], net.opt['vocab_size'] + 1
    nb = min(rows, CHUNK)
    b = lambda n, shp, zero=False: net.buf('rows.' + n, shp, f32, zero)
    logits = b('logits', (nb, V1))
    tokens = net.buf('rows.tokens', (nb,), i64)
    forced = inputs is not None
    # the token-only work, once for all rows
    pre = cap.rows_forced(b, inputs, T) if forced else None
    for c0 in range(0, rows, CHUNK):
        n = min(CHUNK, rows - c0)
        H = cap.rows_head(b, att[c0:c0 + n], fc[c0:c0 + n] if fc is not None else None, n, nb)
        st = cap.rows_states(b, nb)
        O.memset_zero(tokens)                                   # <bos>; a dead row's slot stays a valid index for the embedding
        for t in range(T):
            out = cap.rows_step(b, H, st[t & 1], st[1 - (t & 1)], n, nb, tokens, pre[t] if forced else None, count, c0)
            O.linear_fwd(out, cap.pv('logit.weight'), cap.pv('logit.bias'), logits, n, V1, R)
            O.decode_pick_rows(logits, V1, n, t, T, fin[c0:], seq[c0:], lps[c0:], tokens, targets[t:t + 1] if forced else None, count, c0,
                               score=score[c0:])


def _run_loop(net, att, fc, rows, count, T, seq, lps, score, fin, targets=None):
    """the single-mask launches row by row; the one read-back of `count`"""
    cap = net.captioner
    V1 = net.opt['vocab_size'] + 1
    n = rows if count is None else max(0, min(rows, int(count[0:1].cpu()[0])))
    tokens = net.buf('rows.token', (1,), i64)
    for r in range(n):
        ad, patt = decode._head(net, att[r])
        H = cap.decode_start(ad, patt, decode._fc_checked(net, fc[r]) if cap.reads_fc else None)
        O.memset_zero(tokens)
        cur, new = cap.new_states('a', 1), cap.new_states('b', 1)
        for t in range(T):
            logits = decode.step(net, H, cur, new, tokens, 1)
            O.decode_pick_rows(logits, V1, 1, t, T, fin[r:], seq[r:], lps[r:], tokens, None if targets is None else targets[t:t + 1],
                               score=score[r:])
            cur, new = new, cur


def caption_decode_rows(net, att_feats, fc_feats=None, rows=None, count=None, sample_max=1, beam_size=1):
    """greedy decoding of `rows` masks at once -> {'seq': int64 [rows][seq_length], 'logprobs': f32 [rows][seq_length]} on the device, zero
    from a row's first 0 on and in the rows at or beyond count[0]; no read-back on the batched route"""
    if not sample_max or beam_size != 1:
        raise ValueError('--sample_max %r --beam_size %r: caption_decode_rows is greedy (--sample_max 1 --beam_size 1); beam search on rows is '
                         'caption_beam_rows, sampled decoding takes one mask at a time (caption_decode)' % (sample_max, beam_size))
    rows, att, fc = _start(net, 'caption_decode_rows', att_feats, fc_feats, att_feats.shape[0] if rows is None else rows, count)
    T = int(net.opt['seq_length'])
    seq, lps, score, fin = _outputs(net, rows, T)
    if batched(net):
        _run_batched(net, att, fc, rows, count, T, seq, lps, score, fin)
    else:
        _run_loop(net, att, fc, rows, count, T, seq, lps, score, fin)
    return {'seq': seq, 'logprobs': lps}


def caption_score_rows(net, att_feats, fc_feats, tokens, rows=None, count=None):
    """one expression (tokens: ints 1 .. vocab_size, any length n >= 1) against `rows` masks, teacher-forced with the inputs
    [0, w_1 .. w_n] and the targets [w_1 .. w_n, 0] -> {'logprobs': f32 [rows][n + 1], 'score': f32 [rows] their sum} on the device"""
    toks = [int(v) for v in np.asarray(tokens).reshape(-1)]
    V = int(net.opt['vocab_size']) if getattr(net, 'opt', None) else 0
    if not toks or min(toks) < 1 or max(toks) > V:
        raise ValueError('caption_score_rows: tokens are ints 1 .. vocab_size = %d, at least one; got %r' % (V, toks[:8]))
    rows, att, fc = _start(net, 'caption_score_rows', att_feats, fc_feats, att_feats.shape[0] if rows is None else rows, count)
    T = len(toks) + 1
    io = torch.tensor([[0] + toks, toks + [0]], dtype=i64).to(net.device)
    seq, lps, score, fin = _outputs(net, rows, T)
    if batched(net):
        _run_batched(net, att, fc, rows, count, T, seq, lps, score, fin, io[0], io[1])
    else:
        _run_loop(net, att, fc, rows, count, T, seq, lps, score, fin, io[1])
    return {'logprobs': lps, 'score': score}


# ------------------------------------------------------------------ one expression per row
def _pairs_tokens(net, tokens, lengths, rows):
    """the checked targets of caption_score_pairs -> (targets int64 [rows][Tmax + 1]: w_1 .. w_n, 0, zeros; ntok int32 [rows] = n + 1;
    Tmax + 1), both on the device.  Host tokens are checked here in full; device tokens (int64) are not read back: the kernel clamps a
    token outside the table, and a length outside 1 .. Tmax is cut to that range"""
    V = int(net.opt['vocab_size']) if getattr(net, 'opt', None) else 0
    on_device = isinstance(tokens, torch.Tensor) and tokens.device.type != 'cpu'
    if on_device:
        if tokens.dtype != i64 or tokens.dim() != 2 or tokens.shape[0] < 1 or tokens.shape[1] < 1:
            raise ValueError('caption_score_pairs: tokens on the device is int64 [rows][Tmax], got %s %s' % (tokens.dtype, tuple(tokens.shape)))
        R, Tmax = int(tokens.shape[0]), int(tokens.shape[1])
    else:
        tok = np.asarray(tokens.numpy() if isinstance(tokens, torch.Tensor) else tokens)
        if tok.ndim != 2 or tok.shape[0] < 1 or tok.shape[1] < 1 or tok.dtype.kind not in 'iu':
            raise ValueError('caption_score_pairs: tokens is an int array [rows][Tmax], got %s %s' % (tok.dtype, tok.shape))
        tok = tok.astype(np.int64)
        R, Tmax = int(tok.shape[0]), int(tok.shape[1])
    if rows is not None and int(rows) != R:
        raise ValueError('caption_score_pairs: tokens has %d rows, rows = %r' % (R, rows))
    if isinstance(lengths, torch.Tensor) and lengths.device.type != 'cpu':
        if lengths.dtype != i32 or lengths.numel() != R:
            raise ValueError('caption_score_pairs: lengths on the device is int32 [rows = %d], got %s %s' % (R, lengths.dtype, tuple(lengths.shape)))
        if not on_device:
            raise ValueError('caption_score_pairs: lengths on the device goes with tokens on the device; host tokens take host lengths')
        n_d = lengths.view(-1)
    elif lengths is not None or not on_device:
        if lengths is None:
            n = (tok != 0).sum(1)
        else:
            n = np.asarray(lengths.numpy() if isinstance(lengths, torch.Tensor) else lengths)
            if n.shape != (R,) or n.dtype.kind not in 'iu':
                raise ValueError('caption_score_pairs: lengths is one int per row [rows = %d], got %s %s' % (R, n.dtype, n.shape))
        n = n.astype(np.int64)
        if n.min() < 1:
            raise ValueError('caption_score_pairs: tokens / lengths: row %d is empty, every row needs at least one token' % int(np.argmin(n)))
        if n.max() > Tmax:
            raise ValueError('caption_score_pairs: lengths: row %d has %d tokens, tokens holds Tmax = %d' % (int(np.argmax(n)), int(n.max()), Tmax))
        n_d = None
    else:
        n_d = (tokens != 0).sum(1).to(i32)
    T = Tmax + 1
    if not on_device:
        inside = np.arange(Tmax)[None, :] < n[:, None]
        bad = inside & ((tok < 1) | (tok > V))
        if bad.any():
            r = int(np.argmax(bad.any(1)))
            raise ValueError('caption_score_pairs: tokens are ints 1 .. vocab_size = %d inside a row\'s length; row %d is %r' % (V, r, tok[r, :n[r]].tolist()[:8]))
        tgt = np.zeros((R, T), np.int64)
        tgt[:, :Tmax] = np.where(inside, tok, 0)
        dev = torch.device(net.device)
        return torch.from_numpy(tgt).to(dev), torch.from_numpy((n + 1).astype(np.int32)).to(dev), T
    if n_d is None:
        n_d = torch.from_numpy(n.astype(np.int32)).to(tokens.device)
    n_d = n_d.clamp(1, Tmax)
    tgt = torch.zeros((R, T), dtype=i64, device=tokens.device)
    tgt[:, :Tmax] = torch.where(torch.arange(Tmax, device=tokens.device)[None, :] < n_d[:, None], tokens, torch.zeros_like(tokens))
    return tgt, (n_d + 1).to(i32), T


def _pairs_batched(net, att, fc, rows, count, T, targets, ntok, lps, score):
    """per chunk: the head, then per token the captioner's step driven the greedy way (its input is the token the kernel left in
    `tokens`: the row's own target of the step before), the logits and l2s_decode_force_rows.  Nothing depends on `count` or `rows`"""
    cap = net.captioner
    R, V1 = net.opt['rnn_size'], net.opt['vocab_size'] + 1
    nb = min(rows, CHUNK)
    b = lambda n, shp, zero=False: net.buf('rows.' + n, shp, f32, zero)
    logits = b('logits', (nb, V1))
    tokens = net.buf('rows.tokens', (nb,), i64)
    for c0 in range(0, rows, CHUNK):
        n = min(CHUNK, rows - c0)
        H = cap.rows_head(b, att[c0:c0 + n], fc[c0:c0 + n] if fc is not None else None, n, nb)
        st = cap.rows_states(b, nb)
        O.memset_zero(tokens)                                   # <bos>; a dead row's slot stays a valid index for the embedding
        for t in range(T):
            out = cap.rows_step(b, H, st[t & 1], st[1 - (t & 1)], n, nb, tokens, None, count, c0)
            O.linear_fwd(out, cap.pv('logit.weight'), cap.pv('logit.bias'), logits, n, V1, R)
            O.decode_force_rows(logits, V1, n, t, T, targets[c0:], ntok[c0:], lps[c0:], tokens, count, c0, score=score[c0:])


def _pairs_loop(net, att, fc, rows, count, T, targets, ntok, lps, score):
    """the single-mask launches row by row, the new kernel on one row; the one read-back of `count`.  Every row runs its T steps: behind
    its length the kernel feeds 0 and writes nothing"""
    cap = net.captioner
    V1 = net.opt['vocab_size'] + 1
    n = rows if count is None else max(0, min(rows, int(count[0:1].cpu()[0])))
    tokens = net.buf('rows.token', (1,), i64)
    for r in range(n):
        ad, patt = decode._head(net, att[r])
        H = cap.decode_start(ad, patt, decode._fc_checked(net, fc[r]) if cap.reads_fc else None)
        O.memset_zero(tokens)
        cur, new = cap.new_states('a', 1), cap.new_states('b', 1)
        for t in range(T):
            logits = decode.step(net, H, cur, new, tokens, 1)
            O.decode_force_rows(logits, V1, 1, t, T, targets[r:], ntok[r:], lps[r:], tokens, score=score[r:])
            cur, new = new, cur


def caption_score_pairs(net, att_feats, fc_feats, tokens, lengths=None, rows=None, count=None):
    """row r's own expression under row r's own mask (AttModel.forward + LanguageModelCriterion's gather for a batch of different
    sentences): tokens int [rows][Tmax], ids 1 .. vocab_size, zero padded on the right (a host array, or device int64); lengths: the tokens
    per row (default: its non-zeros), each 1 .. Tmax.  Row r is teacher-forced with the inputs [0, w_1 .. w_n] and the targets
    [w_1 .. w_n, 0] -> on the device {'logprobs': f32 [rows][Tmax + 1], zero behind a row's n + 1; 'score': f32 [rows], their sum;
    'ntok': int32 [rows] = n + 1}; zeros (ntok aside) in the rows at or beyond count[0].

    Batched route: the token step runs the greedy way, its input the token l2s_decode_force_rows left for the row, so the launches per
    token are caption_decode_rows' (att2in2 8, topdown 9) whatever `rows`, `count` and the lengths are; nothing comes back.  A row's
    values do not depend on the other rows of its chunk as long as the chunk has two rows or more (a one-row chunk takes the
    single-row linear kernels, another order of summation)."""
    targets, ntok, T = _pairs_tokens(net, tokens, lengths, rows)
    rows, att, fc = _start(net, 'caption_score_pairs', att_feats, fc_feats, targets.shape[0], count)
    out = net.buf('rows.pairs_out', (rows * (T + 1),), f32, zero=True)
    lps, score = out[:rows * T].view(rows, T), out[rows * T:]
    if batched(net):
        _pairs_batched(net, att, fc, rows, count, T, targets, ntok, lps, score)
    else:
        _pairs_loop(net, att, fc, rows, count, T, targets, ntok, lps, score)
    return {'logprobs': lps, 'score': score, 'ntok': ntok}


# ------------------------------------------------------------------ beam search on rows
def _beam_outputs(net, rows, T, B):
    """seq int64 [rows][T] | beam_seq int64 [rows][B][T] | logprobs f32 [rows][T] | beam_logprobs f32 [rows][B][T] | beam_p f32 [rows][B] |
    beam_n int32 [rows] in one zeroed buffer: a dead row reads as an empty sentence with no beams"""
    n8, n4 = rows * T * (1 + B), rows * T * (1 + B) + rows * B + rows
    out = net.buf('rows.beam_out', (8 * n8 + 4 * n4,), torch.uint8, zero=True)
    w8, w4 = out[:8 * n8].view(i64), out[8 * n8:].view(f32)
    o = [rows * T, rows * T * (1 + B), rows * T * (1 + B) + rows * B]
    return {'seq': w8[:rows * T].view(rows, T), 'beam_seq': w8[rows * T:].view(rows, B, T), 'logprobs': w4[:o[0]].view(rows, T),
            'beam_logprobs': w4[o[0]:o[1]].view(rows, B, T), 'beam_p': w4[o[1]:o[2]].view(rows, B), 'beam_n': w4[o[2]:].view(i32)}


def _beam_tables(net, nb, T, B):
    """a chunk's tables of CaptionModel.beam_search, per detection what nets/decode.py keeps for one caption"""
    RW = O.beam_record_words(T)
    ib = lambda n, shp, dt: net.buf('rows.beam.' + n, shp, dt)
    return dict(seq=ib('seq', (nb, T, B), i32), lp=ib('lp', (nb, T, B), f32), sum=ib('sum', (nb, B), f32), parents=ib('parents', (nb, B), i32),
                done=ib('done', (nb, B * T * RW), i32), cnt=ib('cnt', (nb,), i32))


def _beam_finish(out, tb, B, T, n, c0, count):
    O.decode_beam_finish_rows(tb['done'], tb['cnt'], B, T, n, out['beam_seq'][c0:], out['beam_logprobs'][c0:], out['beam_p'][c0:], out['beam_n'][c0:],
                              out['seq'][c0:], out['logprobs'][c0:], count, c0)


def _beam_batched(net, att, fc, rows, count, T, B, out):
    """per chunk of n detections: the head on n rows, then per token the captioner's step on n * B state rows in groups of B (a group shares
    its detection's head), the logits on n * B rows and the beam step on n detections, which gathers `new` back into `cur`; the final
    ordering once per chunk.  Nothing depends on `count`, nothing comes back"""
    cap = net.captioner
    R, V1 = net.opt['rnn_size'], net.opt['vocab_size'] + 1
    nb = min(rows, CHUNK)
    b = lambda n, shp, zero=False: net.buf('rows.' + n, shp, f32, zero)
    logits = b('logits', (nb * B, V1))
    tokens = net.buf('rows.tokens', (nb * B,), i64)
    tb = _beam_tables(net, nb, T, B)
    for c0 in range(0, rows, CHUNK):
        n = min(CHUNK, rows - c0)
        H = cap.rows_head(b, att[c0:c0 + n], fc[c0:c0 + n] if fc is not None else None, n, nb)
        cur, new = cap.rows_states(b, nb * B)
        O.memset_zero(tokens)
        for t in range(T):
            o = cap.rows_step(b, H, cur, new, n * B, nb * B, tokens, None, count, c0, group=B)
            O.linear_fwd(o, cap.pv('logit.weight'), cap.pv('logit.bias'), logits, n * B, V1, R)
            O.decode_beam_step_rows(logits, V1, B, t, T, n, tb['seq'], tb['lp'], tb['sum'], cap.rows_gather(new, cur), R, tokens, tb['parents'],
                                    tb['done'], tb['cnt'], count, c0)
        _beam_finish(out, tb, B, T, n, c0, count)


def _beam_loop(net, att, fc, rows, count, T, B, out):
    """per live detection the single-mask launches of nets/decode.py's beam search, the beam step on that detection's slices of the chunk's
    tables; the final ordering once per chunk that has a live detection; the one read-back of `count`"""
    cap = net.captioner
    R, V1 = net.opt['rnn_size'], net.opt['vocab_size'] + 1
    live = rows if count is None else max(0, min(rows, int(count[0:1].cpu()[0])))
    nb = min(rows, CHUNK)
    tb = _beam_tables(net, nb, T, B)
    tokens = net.buf('dec.tokens', (B,), i64)
    for c0 in range(0, live, CHUNK):
        n = min(CHUNK, live - c0)
        for k in range(n):
            r = c0 + k
            ad, patt = decode._head(net, att[r])
            H = cap.decode_start(ad, patt, decode._fc_checked(net, fc[r]) if cap.reads_fc else None)
            O.memset_zero(tokens)
            cur, new = cap.new_states('a', B), cap.new_states('b', B)
            for t in range(T):
                logits = decode.step(net, H, cur, new, tokens, B)
                O.decode_beam_step(logits, V1, B, t, T, tb['seq'][k], tb['lp'][k], tb['sum'][k],
                                   [(new[s][0], cur[s][0], new[s][1], cur[s][1]) for s in cap.states], R, tokens, tb['parents'][k], tb['done'][k],
                                   tb['cnt'][k:k + 1])
        _beam_finish(out, tb, B, T, n, c0, None)


def caption_beam_rows(net, att_feats, fc_feats=None, rows=None, count=None, beam_size=3):
    """beam search (CaptionModel.beam_search, as caption_decode(beam_size=) runs it for one mask) for `rows` masks at once -> on the device
    {'seq': int64 [rows][seq_length] and 'logprobs': f32 [rows][seq_length], the best beam in caption_decode_rows' layout;
     'beam_seq': int64 [rows][beam_size][seq_length], 'beam_logprobs': f32 likewise, 'beam_p': f32 [rows][beam_size], best first;
     'beam_n': int32 [rows], the beams a row has}; zeros in the rows at or beyond count[0].  No read-back on the batched route"""
    decode.check_args(net, 1, beam_size, 1.0)                   # the --beam_size errors of the single-mask path, before anything else
    T, B = int(net.opt['seq_length']), int(beam_size)
    if T > O.BEAM_MAX_T:                                        # (check_args lets one beam pass: the greedy single-mask path has no tables)
        raise ValueError('--beam_size %r with seq_length %d: beam search keeps at most %d tokens' % (beam_size, T, O.BEAM_MAX_T))
    rows, att, fc = _start(net, 'caption_beam_rows', att_feats, fc_feats, att_feats.shape[0] if rows is None else rows, count)
    out = _beam_outputs(net, rows, T, B)
    if batched(net):
        _beam_batched(net, att, fc, rows, count, T, B, out)
    else:
        _beam_loop(net, att, fc, rows, count, T, B, out)
    return out
