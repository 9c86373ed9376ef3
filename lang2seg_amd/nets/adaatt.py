"""The core of the adaptive-attention captioners (--caption_model adaatt | adaattmo; AttModel.py:211-368) as a sequence of launches.

Per token only the cell runs (csrc/adaatt_step.hip: one launch each way).  The attention reads the cell's outputs and feeds the token's logits,
never the next token, so it runs ONCE for all S tokens as row batches: the small R x R Linears as [S][R] products, the scores / softmax /
weighted sum with the token as a grid dimension.  Backward mirrors it: the attention's backward for all tokens first (d(att) and d(p_att) are
complete before the recurrence starts), then S cell launches from the last token to the first.

Used by nets/captioners.py (AdaAtt; decoding runs cell_fwd and att_fwd on its beam rows) and, with plain tensors, by
tests/test_adaatt_gpu.py.  `O` is lang2seg_amd.ops (or its torch restatement), pv / gv give a parameter / its gradient by the key below
'caption_model.core.', `bwd_x` is Network.bwd_x's with that key.  Masks: {'toph', 'fake', 'frl', 'hol': [S][R], 'hA': [S][L+1][R]} or None."""


def fwd_shapes(S, L, R):
    s = {k: (S, R) for k in ('fake', 'toph', 'faked', 'fra', 'frl', 'hoa', 'hol', 'fre', 'hoe', 'atten', 'outs')}
    s.update(hs=(S + 1, R), cs=(S + 1, R), save=(S, 7 * R), tanh=(S, L + 1, R), dots=(S, 256), PI=(S, L + 1))
    return s


def bwd_shapes(S, L, R, G):
    s = {k: (S, R) for k in ('datten', 'dhoe', 'dfre', 'dctx', 'dfrl', 'dhol', 'dtoph', 'dfake')}
    s.update(ddot=(S, L + 1), dall=(S, (G + 1) * R), dc=(2, R))
    return s


def _masked(O, x, m, out):
    if m is None:
        return x
    O.mul(x, m, out)
    return out


CELL_KEYS = ('lstm.h2h.0.weight', 'lstm.h2h.0.bias', 'lstm.r_h2h.weight', 'lstm.r_h2h.bias')      # what cell_fwd takes as `w`, in its order


def cell_fwd(O, w, xpre, fcrow, h0, c0, h1, c1, fake, save, R, G):
    """the cell on one row: token i of a sentence (core_fwd) or one beam of a decoding step.  (h0, c0) -> (h1, c1), the sentinel into fake"""
    O.adaatt_cell_fwd(xpre, fcrow, w[0], w[1], w[2], w[3], h0, c0, c1, h1, fake, save, R, G)


def core_fwd(O, pv, B, xpre, fcrow, att, patt, masks, S, L, R, G):
    """xpre [S][(G+1)R] = w2h(xt) | r_w2h(xt) (biases included), fcrow [(G+1)R] = v2h(fc) | r_v2h(fc); att / patt [L][R]; B: fwd_shapes buffers,
    hs / cs row 0 zero.  Leaves the outputs tanh(att2h(atten)) [S][R] in B['outs'] and returns the views backward needs."""
    hs, cs, w = B['hs'], B['cs'], tuple(pv(k) for k in CELL_KEYS)
    for i in range(S):
        cell_fwd(O, w, xpre[i], fcrow, hs[i], cs[i], hs[i + 1], cs[i + 1], B['fake'][i], B['save'][i], R, G)
    return att_fwd(O, pv, B, hs[1:], att, patt, masks, S, L, R)


def att_fwd(O, pv, B, h, att, patt, masks, S, L, R):
    """the attention half of core_fwd on S rows of cell outputs h [S][R] and B['fake'] (S tokens of one sentence, or the S beams of one
    decoding step: the rows never meet)"""
    toph = _masked(O, h, masks.get('toph'), B['toph'])
    faked = _masked(O, B['fake'], masks.get('fake'), B['faked'])
    lin = lambda x, k, y, act=0: O.linear_fwd(x, pv('attention.%s.weight' % k), pv('attention.%s.bias' % k), y, S, R, R, act=act)
    lin(faked, 'fr_linear.0', B['fra'], 1)
    frl = _masked(O, B['fra'], masks.get('frl'), B['frl'])
    lin(toph, 'ho_linear.0', B['hoa'], 2)
    hol = _masked(O, B['hoa'], masks.get('hol'), B['hol'])
    lin(frl, 'fr_embed', B['fre'])
    lin(hol, 'ho_embed', B['hoe'])
    O.adaatt_att_fwd(att, patt, frl, B['fre'], B['hoe'], hol, pv('attention.alpha_net.weight'), pv('attention.alpha_net.bias'), masks.get('hA'),
                     S, L, R, B['tanh'], B['dots'], B['PI'], B['atten'])
    lin(B['atten'], 'att2h', B['outs'], 2)
    return dict(toph=toph, faked=faked, frl=frl, hol=hol)


def core_bwd(O, pv, wT, bwd_x, B, D, V, dout, att, dpatt, datt, daw, masks, S, L, R, G):
    """dout [S][R]: d(outputs), overwritten.  B: the forward's buffers, V: what core_fwd returned, D: bwd_shapes buffers.  dpatt / datt [L][R]
    and daw [R] (alpha_net.weight's gradient) are added to.  Leaves d(sums | n5) of every token in D['dall'] [S][(G+1)R] and d(hoe) - d(fre)
    in D['dctx'] (its column sums are ctx2att.bias's gradient).  wT: (h2h.0.weight^T [R][G R], r_h2h.weight^T [R][R])."""
    mA = masks.get('hA')
    O.act_bwd(dout, B['outs'], 2)
    bwd_x(dout, 'attention.att2h.weight', D['datten'], S)
    O.adaatt_att_bwd_step(D['datten'], att, V['frl'], B['tanh'], mA, B['PI'], pv('attention.alpha_net.weight'), S, L, R, D['ddot'], D['dhoe'], D['dfre'],
                          D['dctx'], D['dfrl'], D['dhol'])
    O.adaatt_att_bwd_batched(D['ddot'], B['PI'], D['datten'], B['tanh'], mA, pv('attention.alpha_net.weight'), S, L, R, dpatt, datt, daw)
    # h-out chain: d(hol) = d(atten) + ho_embed^T d(hoe) -> dropout, tanh -> ho_linear^T -> the top_h dropout
    bwd_x(D['dhoe'], 'attention.ho_embed.weight', D['dhol'], S, accumulate=True)
    if masks.get('hol') is not None:
        O.mul(D['dhol'], masks['hol'], D['dhol'])
    O.act_bwd(D['dhol'], B['hoa'], 2)
    bwd_x(D['dhol'], 'attention.ho_linear.0.weight', D['dtoph'], S, mul=masks.get('toph'))
    # sentinel chain: d(frl) = PI[0] d(atten) + fr_embed^T d(fre) -> dropout, ReLU -> fr_linear^T -> the sentinel's dropout
    bwd_x(D['dfre'], 'attention.fr_embed.weight', D['dfrl'], S, accumulate=True)
    if masks.get('frl') is not None:
        O.mul(D['dfrl'], masks['frl'], D['dfrl'])
    O.act_bwd(D['dfrl'], B['fra'], 1)
    bwd_x(D['dfrl'], 'attention.fr_linear.0.weight', D['dfake'], S, mul=masks.get('fake'))
    # the recurrence: h(i) is read by token i + 1 through h2h.0 and r_h2h
    t_hh, t_r = wT
    dall, dc, cs = D['dall'], D['dc'], B['cs']
    k = 0
    for i in range(S - 1, -1, -1):
        last = i == S - 1
        O.adaatt_cell_bwd(None if last else dall[i + 1], t_hh, t_r, D['dtoph'][i], D['dfake'][i], None if last else dc[k], B['save'][i], cs[i],
                          dall[i], dc[1 - k], R, G)
        k = 1 - k


def core_wgrads(O, gv, B, D, V, dout, xt, fcd, dgsum, S, R, IE, G):
    """the core's parameter gradients, all as row batches over the S tokens (dout: what core_bwd left in it, d(att2h's sums); dgsum [(G+1)R]:
    the column sums of D['dall']).  alpha_net.weight's was added by core_bwd; alpha_net.bias's is exactly 0 and stays untouched."""
    W = (G + 1) * R
    dall = D['dall']
    bw = lambda dy, x, k, M=S, N=R, K=R, lddy=None: O.linear_bwd_w(dy, x, gv(k + '.weight'), gv(k + '.bias'), M, N, K, lddy=lddy)
    bw(dout, B['atten'], 'attention.att2h')
    bw(D['dhoe'], V['hol'], 'attention.ho_embed')
    bw(D['dfre'], V['frl'], 'attention.fr_embed')
    bw(D['dhol'], V['toph'], 'attention.ho_linear.0')
    bw(D['dfrl'], V['faked'], 'attention.fr_linear.0')
    bw(dall, B['hs'], 'lstm.h2h.0', N=G * R, lddy=W)
    bw(dall[:, G * R:], B['hs'], 'lstm.r_h2h', lddy=W)
    bw(dall, xt, 'lstm.w2h', N=G * R, K=IE, lddy=W)
    bw(dall[:, G * R:], xt, 'lstm.r_w2h', K=IE, lddy=W)
    bw(dgsum, fcd, 'lstm.v2h', M=1, N=G * R)
    bw(dgsum[G * R:], fcd, 'lstm.r_v2h', M=1)
