"""l2s_conv_wgrad and l2s_conv_wgrad_grouped (csrc/conv_wgrad.hip, conv_wgrad_dma.hip, conv_wgrad_dma1.hip): the case table that reaches
every weight-gradient kernel of the product library at the edges of its pixel pipeline, the float64 restatement of the weight gradient,
and the operand layout the CPU and the GPU test files share.  The comparison is small_kernels_util.check, unchanged:

    |got - ref| <= (n_terms + 2) * 2^-24 * absum,          rho = 0: dW is always stored as float, no bf16 allowance hides anything

Reference (numpy float64 on the operands as the device sees them, bf16 values rounded first), one matmul per filter tap over the gathered
pixels of every segment, out-of-image taps zero:

    dW[co][ky][kx][ci] = dW0[co][ky][kx][ci] (absent under flags = 1) + sum over segments, sum over output pixels m of dY[m][co] * X(m, ky, kx)[ci]
    absum              = |dW0| + |dY|^T |X|

Bound.  A product of two bf16 values is exact in float32 and the float32 MFMA rounds once per accumulate, so one output is a float32 sum of
M_total products taken in some order (M_total = the pixels of all segments), to which the prior content of dW is added once: M_total + 1
roundings along the longest chain (in f32 mode the product itself is rounded inside the fused accumulate, which the same count covers:
Higham, section 4.2, and the two terms of slack of `check`).  A second launch that adds partial sums costs one more float32 addition per
partial sum:
    n_terms = M_total + 1 + extra
    extra   = split                       for a problem whose pixels are split (one slab per range, added in a fixed order);
              the 64-pixel slices of the problem     for variant 5 (the stream-K launch cuts a tile's slices into pieces, every piece of a
                                          shared tile holds at least one slice, and the second launch adds one slab per piece);
              0                           otherwise.
Every case has M_total <= 2040, i.e. M (M + 4) 2^-24 < 1/4: one dropped or misplaced pixel (about absum / M) stands clear of the rounding
allowance (tests/test_wgrad_cpu.py mutates the reference and shows that `check` raises).

A CASE is one launch: the entry ('single' = l2s_conv_wgrad, 'grouped' = l2s_conv_wgrad_grouped), the dtype, the variant it has to land on
(single launches reach it through the `tile` request, grouped launches name it), and its problems (one for a single launch).  A PROBLEM
holds one or two pixel segments (n, H, W), Cin, Cout, KH, KW, stride, pad, the split, a layout ('dense', or 'pitched': lddy = Cout + pad
and ldx = Cin + pad with pads that are multiples of the 16-byte vector and differ between dY and X and between the segments) and whether
the launch overwrites dW (flags = 1) or adds to it.  Variants 4, 5 and 6 are chosen by l2s_wgrad_variant only from 8192 pixels up (variant 5:
or from 512 channels on both sides), but their launchers take small problems, so the grouped cases pass the variant; cases marked `auto`
are those whose shape l2s_wgrad_variant itself maps to the variant under the product's tile request (256 in bf16, 0 in f32).

Not in the table: the tools-build knobs (wgrad_grid_cap, row3_form, row3_plan_mode: the product library fixes them to 0, so the capped
grid's tile walk, the knock-out forms of the filter-row kernel and its XCD-lockstep plan are never taken), and operands of 2 GiB or more."""
import os
import re

import numpy as np
import torch
import torch.nn.functional as TF

from small_kernels_util import bf16r, f64, F32, BF16

SINGLE, GROUPED = 'single', 'grouped'
MAX_GROUP, MAX_SEG = 64, 2
M_MAX = 2040
GUARD = 4                  # rows of sentinels in front of and behind dY, X (per segment) and dW
V5_WGS = 160               # l2s_knobs::wgrad_row3_dma_wgs

# (tile co, tile ci, taps per workgroup) of every variant: variant_tile() of csrc/conv_wgrad.hip
TILE = {0: (64, 64, 1), 1: (128, 128, 1), 2: (64, 64, 3), 3: (128, 64, 3), 4: (256, 256, 1), 5: (128, 128, 3), 6: (256, 256, 1)}
# ring depth D of launch_single / launch_grouped per variant; tests/test_wgrad_cpu.py reads the source's own template arguments against these
RING_SINGLE = {0: 4, 1: 3, 2: 4, 3: 3}
RING_GROUPED = {0: 2, 1: 2, 2: 2, 3: 2, 4: 2}
SINGLE_TILE_REQUEST = {0: 64, 1: 128, 2: 64, 3: 128}


def slice_pixels(entry, variant, dt):
    """pixels per slice (one barrier) of the kernel behind (entry, variant, dtype)"""
    if variant == 5:
        return 64
    if variant in (4, 6):
        return 32
    if dt == F32:
        return 16
    return 32 if entry == SINGLE else 64          # grouped bf16: KSTEP = 2


def row3(variant):
    return TILE[variant][2] == 3


# every kernel instantiation of the product library, as (kernel family, variant, dtype) and the three reduce kernels by name
ALL_KERNELS = {('wgrad_kernel', v, dt) for v in range(4) for dt in (BF16, F32)} | {('wgrad_grouped_kernel', v, dt) for v in range(4) for dt in (BF16, F32)} | \
              {('wgrad_grouped_kernel', 4, BF16), ('wgrad_row3_dma_kernel', 5, BF16), ('wgrad_1x1_dma_kernel', 6, BF16),
               'wgrad_reduce_kernel', 'wgrad_reduce_grouped_kernel', 'wgrad_row3_reduce_kernel'}


# ------------------------------------------------------------------------------------------------------------------ problems
def out_hw(H, W, KH, KW, stride, pad):
    return (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1


def P(segs, Cin, Cout, k=1, KH=None, KW=None, stride=1, pad=None, split=1, lay='dense', ow=False):
    KH, KW = KH or k, KW or k
    pad = (k // 2 if KH == KW else 0) if pad is None else pad
    segs = [tuple(s) for s in segs]
    for (n, H, W) in segs:
        OH, OW = out_hw(H, W, KH, KW, stride, pad)
        assert n >= 1 and OH >= 1 and OW >= 1, (segs, KH, KW, stride, pad)
    return dict(segs=segs, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, split=split, lay=lay, ow=ow)


def seg_geometry(p, s):
    n, H, W = p['segs'][s]
    OH, OW = out_hw(H, W, p['KH'], p['KW'], p['stride'], p['pad'])
    return n, H, W, OH, OW


def pixels(p):
    return [n * OH * OW for (n, _, _, OH, OW) in (seg_geometry(p, s) for s in range(len(p['segs'])))]


def same_hw(p):
    return all(g[1] == g[3] and g[2] == g[4] for g in (seg_geometry(p, s) for s in range(len(p['segs']))))


def is_row3_shape(p):
    return p['KH'] == 3 and p['KW'] == 3 and p['stride'] == 1 and p['pad'] == 1 and same_hw(p)


def slices(c, p):
    """slices of each segment as the kernel of case c counts them (filter-row tiles: in the virtual layout, one zero column per image row)"""
    b, e = slice_pixels(c['entry'], c['variant'], c['dt']), 1 if row3(c['variant']) else 0
    return [-(-(n * OH * (OW + e)) // b) for (n, _, _, OH, OW) in (seg_geometry(p, s) for s in range(len(p['segs'])))]


def virtual_pixels(c, p):
    e = 1 if row3(c['variant']) else 0
    return [n * OH * (OW + e) for (n, _, _, OH, OW) in (seg_geometry(p, s) for s in range(len(p['segs'])))]


def eff_split(c, p):
    """the ranges the pixels of p are cut into: the grouped entry takes `split` as it is, the single entry clamps it (plan_split)"""
    if c['entry'] == GROUPED:
        return max(1, p['split'])
    return max(1, min(p['split'], slices(c, p)[0], 64))


def wg_slices(c, p):
    """NS of every (range, segment): the slice counts one workgroup's ring sees, zeros included"""
    sp = eff_split(c, p)
    out = []
    for ns in slices(c, p):
        per = -(-ns // sp)
        out += [max(0, min(ns, (i + 1) * per) - i * per) for i in range(sp)]
    return out


def tiles(variant, p):
    bm, bn, tx = TILE[variant]
    if variant == 5:
        return (p['Cout'] // bm) * (p['Cin'] // bn) * 3
    return -(-p['Cout'] // bm) * -(-p['Cin'] // bn) * (p['KH'] if tx == 3 else p['KH'] * p['KW'])


def n_terms(c, p):
    extra = 0
    if c['variant'] == 5:
        extra = sum(slices(c, p))
    elif eff_split(c, p) > 1:
        extra = eff_split(c, p)
    return sum(pixels(p)) + 1 + extra


def pitches(c, p, s):
    """(lddy, ldx) of segment s"""
    if p['lay'] == 'dense':
        return p['Cout'], p['Cin']
    ve = 8 if c['dt'] == BF16 else 4
    return p['Cout'] + ve * (1 + s), p['Cin'] + ve * (3 + 2 * s)


def v5_workgroups(U):
    """the G clamps of wgrad_row3_dma_launch for U (tile, slice) units"""
    G = min(V5_WGS, U)
    if U // 24 < G:
        G = (U // 24) & ~7
        if G < 8:
            G = U if U < 8 else 8
    return G


def main_kernel(c):
    v = c['variant']
    fam = 'wgrad_kernel' if c['entry'] == SINGLE else 'wgrad_row3_dma_kernel' if v == 5 else 'wgrad_1x1_dma_kernel' if v == 6 else 'wgrad_grouped_kernel'
    return (fam, v, c['dt'])


def last_kernel_family(c):
    """the family name ops.last_kernel() has to start with after the launch of case c"""
    if c['variant'] == 5:
        return 'wgrad_row3_reduce_kernel'
    if any(eff_split(c, p) > 1 for p in c['probs']):
        return 'wgrad_reduce_kernel' if c['entry'] == SINGLE else 'wgrad_reduce_grouped_kernel'
    return main_kernel(c)[0]


# ------------------------------------------------------------------------------------------------------------------ cases
CASES = []
DTN = {BF16: 'bf16', F32: 'f32'}


def case(entry, dt, variant, probs, tag, auto=False, pair=None):
    probs = probs if isinstance(probs, list) else [probs]
    c = dict(entry=entry, dt=dt, variant=variant, probs=probs, auto=auto, pair=pair, tile=SINGLE_TILE_REQUEST[variant] if entry == SINGLE else None,
             id='%s-v%d-%s-%s' % (entry, variant, DTN[dt], tag))
    CASES.append(c)
    return c


# tap geometries (KH, KW, stride, pad) of the per-tap tiles; K3 (the filter-row shape) only where the variant is named (grouped launches)
K1, K1S2, K3S2, K13, K5, K3P0, K3 = (1, 1, 1, 0), (1, 1, 2, 0), (3, 3, 2, 1), (1, 3, 1, 0), (5, 5, 1, 2), (3, 3, 1, 0), (3, 3, 1, 1)


def fit(ns, bkp, taps, e, style, exact=False):
    """a segment (n, H, W) whose pixels (virtual layout if e) make exactly ns slices of bkp pixels; style 'small': images smaller than a slice
    (3x3 or 7x7 outputs), 'one': one image; exact: the last slice ends on the segment's end, otherwise it is ragged"""
    KH, KW, st, pd = taps
    odd = st == 2 and KH == 1                                # 1x1 stride 2: odd H and W
    cands = []
    if style == 'small':
        for (H, W) in ((3, 3), (7, 7), (5, 5)):
            if out_hw(H, W, KH, KW, st, pd)[0] >= 1 and out_hw(H, W, KH, KW, st, pd)[1] >= 1:
                cands += [(n, H, W) for n in range(1, 400)]
    else:
        cands = [(1, H, W) for W in (9, 7, 8, 11, 13, 5, 10, 6, 15, 17, 18) for H in range(1, 300) if not odd or (H % 2 and W % 2)]
    for (n, H, W) in cands:
        OH, OW = out_hw(H, W, KH, KW, st, pd)
        if OH < 1 or OW < 1:
            continue
        mv = n * OH * (OW + e)
        if -(-mv // bkp) == ns and (mv % bkp == 0) == exact and n * OH * OW <= M_MAX:
            return (n, H, W)
    raise AssertionError((ns, bkp, taps, e, style, exact))


def ring_targets(D):
    return sorted({1, 2, D, D + 1, 2 * D - 1, 2 * D, 2 * D + 1, 3 * D + 1})


def chans(variant, dt, i=0):
    """(Cin, Cout) with a tail on both sides of the variant's tile, rotated by i: above the tile on one side, below it on the other"""
    bm, bn, _ = TILE[variant]
    if dt == BF16:
        co, ci = {64: (72, 40), 128: (200, 136), 256: (264, 280)}[bm], {64: (40, 72), 128: (136, 200), 256: (280, 264)}[bn]
    else:
        co, ci = {64: (68, 36), 128: (132, 100)}[bm], {64: (36, 68), 128: (100, 132)}[bn]
    return ci[i % 2], co[i % 2]


def _build():
    pertap = (K1, K1S2, K3S2, K13, K5, K3P0)
    # ---- single launches: every ring occupancy of every (variant, dtype), rotating the tap geometry, the image size and the layout
    for dt in (BF16, F32):
        for v in range(4):
            D, bkp, e = RING_SINGLE[v], slice_pixels(SINGLE, v, dt), 1 if row3(v) else 0
            for i, ns in enumerate(ring_targets(D)):
                taps = K3 if e else pertap[i % len(pertap)]
                exact = ns == 2 * D
                seg = (1, 3, 3) if ns == 1 and taps in (K1, K3) else fit(ns, bkp, taps, e, 'small' if i % 2 == 0 and not exact else 'one', exact)
                Cin, Cout = chans(v, dt, i)
                case(SINGLE, dt, v, P([seg], Cin, Cout, KH=taps[0], KW=taps[1], stride=taps[2], pad=taps[3], lay='pitched' if i % 2 else 'dense'), 'ring%d' % ns)
            # ---- splits: 2, 3, the slice count, and one that plan_split clamps to the slice count
            taps = K3 if e else K1
            for split, ns, tag in ((2, 2 * D + 1, 'split2'), (3, 3 * D + 1, 'split3'), (5, 5, 'spliteq'), (50, 6, 'splitclamp')):
                Cin, Cout = chans(v, dt, split)
                case(SINGLE, dt, v, P([fit(ns, bkp, taps, e, 'one')], Cin, Cout, KH=taps[0], KW=taps[1], stride=taps[2], pad=taps[3], split=split,
                                      lay='pitched' if split == 3 else 'dense'), tag)
            # ---- a row longer than a slice
            case(SINGLE, dt, v, P([(1, 2, 70)], *chans(v, dt), KH=taps[0], KW=taps[1], stride=taps[2], pad=taps[3], lay='pitched'), 'wide')
    # ---- grouped launches of the register-staged tiles
    for dt in (BF16, F32):
        for v in range(5):
            if v == 4 and dt == F32:
                continue
            D, bkp, e = RING_GROUPED[v], slice_pixels(GROUPED, v, dt), 1 if row3(v) else 0
            kinds = (K3,) if e else (K1,) if v == 4 else pertap + (K3,)
            small = (8, 8) if dt == BF16 else (4, 4)
            # ring: one problem per occupancy, different tile counts (the binary search over the tile prefix)
            probs = []
            for i, ns in enumerate(ring_targets(D)):
                taps = kinds[i % len(kinds)]
                exact = ns == 2 * D
                seg = fit(ns, bkp, taps, e, 'small' if i % 2 == 0 and not exact else 'one', exact)
                Cin, Cout = chans(v, dt, i) if i % 3 != 2 else small
                probs.append(P([seg], Cin, Cout, KH=taps[0], KW=taps[1], stride=taps[2], pad=taps[3], lay='pitched' if i % 2 else 'dense', ow=i % 2 == 1))
            case(GROUPED, dt, v, probs, 'ring')
            # the remaining tap geometries of the per-tap tiles (the ring launch has six problems)
            if len(kinds) > 6:
                case(GROUPED, dt, v, [P([fit(2, bkp, t, 0, 'one')], *chans(v, dt, j), KH=t[0], KW=t[1], stride=t[2], pad=t[3]) for j, t in enumerate(kinds[5:])], 'taps')
            # one problem
            t = kinds[0]
            case(GROUPED, dt, v, P([(1, 3, 3)], *chans(v, dt), KH=t[0], KW=t[1], stride=t[2], pad=t[3], lay='pitched'), 'one')
            # two segments (shorter first / second), splits beside unsplit problems, ws_off > 0, ranges without slices (NS == 0), overwrite
            short, long_, mid = (1, 3, 3), fit(7, bkp, t, e, 'small'), fit(3, bkp, t, e, 'one')
            kw = dict(KH=t[0], KW=t[1], stride=t[2], pad=t[3])
            case(GROUPED, dt, v, [
                P([short, long_], *chans(v, dt, 0), lay='pitched', **kw),
                P([long_, short], *chans(v, dt, 1), split=3, **kw),                        # the short segment has 1 slice: ranges 1 and 2 skip it
                P([mid], *small, **kw),
                P([mid, long_], *chans(v, dt, 1), split=2, ow=True, lay='pitched', **kw),   # the second split problem: ws_off > 0
                P([long_], *chans(v, dt, 0), split=7, ow=True, **kw),                      # split = the slice count
                P([(2, 1, 70)], *small, lay='pitched', **kw),                              # rows longer than a slice
            ], 'mix')
            # 64 problems, each as small as the variant allows
            if dt == BF16 or v == 0:
                case(GROUPED, dt, v, [P([(1, 1, 1 + i % 3)], *small, ow=i % 2 == 1, **kw) for i in range(MAX_GROUP)], '64')
    # shapes l2s_wgrad_variant itself maps to variants 0, 2 and 3 under the product's request
    for dt in (BF16, F32):
        case(GROUPED, dt, 0, P([(2, 9, 9)], *chans(0, dt), k=1), 'auto', auto=True)
        case(GROUPED, dt, 2, P([(3, 7, 7), (1, 11, 13)], *chans(2, dt), k=3), 'auto', auto=True)
        case(GROUPED, dt, 3, P([(1, 5, 6)], 40 if dt == BF16 else 36, 520, k=3), 'auto', auto=True)
    # ---- variant 5: the LDS-DMA filter-row tile with its stream-K plan (64-pixel slices of the virtual layout, 128x128 tiles)
    for S in (1, 2, 3, 4, 5):                          # fewer than, equal to and more than the slices in flight; 3 S units: below 8 for S <= 2
        seg = fit(S, 64, K3, 1, 'small' if S % 2 else 'one', exact=S == 4)
        case(GROUPED, BF16, 5, P([seg], 128, 128, k=3, lay='pitched' if S % 2 == 0 else 'dense', ow=S % 2 == 1), 'S%d' % S)
    case(GROUPED, BF16, 5, [P([(1, 3, 3)], 128, 256, k=3), P([fit(3, 64, K3, 1, 'one'), (2, 3, 3)], 256, 128, k=3, lay='pitched', ow=True),
                            P([(1, 1, 70), fit(4, 64, K3, 1, 'small')], 128, 128, k=3, lay='pitched'), P([fit(7, 64, K3, 1, 'one')], 128, 128, k=3, ow=True)], 'mix')
    case(GROUPED, BF16, 5, P([(2, 10, 12)], 512, 512, k=3), 'auto', auto=True)      # 512 channels on both sides: the filter-row tile from any pixel count
    case(GROUPED, BF16, 5, [P([(1, 1, 1 + i % 3)], 128, 128, k=3, ow=i % 2 == 1) for i in range(MAX_GROUP)], '64')
    # ---- variant 6: the LDS-DMA 256x256 tile (32-pixel slices), each beside variant 4 on the same problems
    for S in (1, 2, 3, 4):
        seg = fit(S, 32, K1, 0, 'small' if S % 2 else 'one', exact=S == 2)
        case(GROUPED, BF16, 6, P([seg], 256, 256, lay='pitched' if S % 2 == 0 else 'dense', ow=S % 2 == 1), 'S%d' % S, pair=4)
    case(GROUPED, BF16, 6, [P([(5, 3, 3), (1, 7, 9)], 256, 512, lay='pitched'), P([(1, 5, 7)], 512, 256, ow=True),
                            P([fit(7, 32, K1, 0, 'one'), (1, 3, 3)], 256, 256, ow=True, lay='pitched')], 'mix', pair=4)
    case(GROUPED, BF16, 6, [P([(1, 1, 1 + i % 3)], 256, 256, ow=i % 2 == 1) for i in range(MAX_GROUP)], '64')
    # ---- the grouped f32 entry beside the single f32 entry on the same unsplit problem
    for v in range(4):
        t = K3 if row3(v) else K1
        case(GROUPED, F32, v, P([fit(9, 16, t, 1 if row3(v) else 0, 'small')], *chans(v, F32), KH=t[0], KW=t[1], stride=t[2], pad=t[3]), 'pair', pair='single')


_build()
assert len({c['id'] for c in CASES}) == len(CASES)


# ------------------------------------------------------------------------------------------------------------------ operands and references
_INPUTS, _REFS = {}, {}


def _rnd(rs, shape, dt):
    a = rs.standard_normal(shape).astype(np.float32)
    return bf16r(a) if dt == BF16 else a


def make(c):
    """per problem: dict(x=[per segment [n][H][W][Cin]], dy=[per segment [n][OH][OW][Cout]], dw0=[Cout][KH][KW][Cin]) float32, as the device sees them"""
    if c['id'] not in _INPUTS:
        rs = np.random.RandomState(sum(ord(ch) * (i + 1) for i, ch in enumerate(c['id'])) % (2 ** 31))
        out = []
        for p in c['probs']:
            d = dict(x=[], dy=[], dw0=_rnd(rs, (p['Cout'], p['KH'], p['KW'], p['Cin']), F32))
            for s in range(len(p['segs'])):
                n, H, W, OH, OW = seg_geometry(p, s)
                d['x'].append(_rnd(rs, (n, H, W, p['Cin']), c['dt']))
                d['dy'].append(_rnd(rs, (n, OH, OW, p['Cout']), c['dt']))
            out.append(d)
        _INPUTS[c['id']] = out
    return _INPUTS[c['id']]


def gather(p, s, x, ky, kx):
    """X(m, ky, kx) of segment s as [M][Cin] float64: the input pixel under tap (ky, kx) of every output pixel, zero outside the image"""
    n, H, W, OH, OW = seg_geometry(p, s)
    pd, st = p['pad'], p['stride']
    xp = np.pad(f64(x), ((0, 0), (pd, pd), (pd, pd), (0, 0)))
    return xp[:, ky:ky + st * (OH - 1) + 1:st, kx:kx + st * (OW - 1) + 1:st, :].reshape(n * OH * OW, p['Cin'])


def seg_term(p, s, x, dy, gather_=gather):
    """(dY^T X, |dY|^T |X|) of one segment as [Cout][KH][KW][Cin]"""
    dym = f64(dy).reshape(-1, p['Cout'])
    z, ab = np.zeros((p['Cout'], p['KH'], p['KW'], p['Cin'])), np.zeros((p['Cout'], p['KH'], p['KW'], p['Cin']))
    for ky in range(p['KH']):
        for kx in range(p['KW']):
            g = gather_(p, s, x, ky, kx)
            z[:, ky, kx, :] = dym.T @ g
            ab[:, ky, kx, :] = np.abs(dym).T @ np.abs(g)
    return z, ab


def wgrad_ref64(p, inp):
    """-> (ref64, absum64) as [Cout][KH][KW][Cin]"""
    z, ab = f64(inp['dw0']), np.abs(f64(inp['dw0']))
    if p['ow']:
        z, ab = np.zeros_like(z), np.zeros_like(ab)
    for s in range(len(p['segs'])):
        zs, as_ = seg_term(p, s, inp['x'][s], inp['dy'][s])
        z, ab = z + zs, ab + as_
    return z, ab


def refs(c):
    """[(ref64, absum64, n_terms)] per problem of case c, computed once"""
    if c['id'] not in _REFS:
        _REFS[c['id']] = [wgrad_ref64(p, inp) + (n_terms(c, p),) for p, inp in zip(c['probs'], make(c))]
    return _REFS[c['id']]


def wgrad_f32(p, inp):
    """the same through torch autograd on the CPU in float32 (conv2d(...).backward), [Cout][KH][KW][Cin]"""
    w = torch.zeros(p['Cout'], p['Cin'], p['KH'], p['KW'], requires_grad=True)
    for s in range(len(p['segs'])):
        x = torch.from_numpy(inp['x'][s]).permute(0, 3, 1, 2)
        TF.conv2d(x, w, None, stride=p['stride'], padding=p['pad']).backward(torch.from_numpy(inp['dy'][s]).permute(0, 3, 1, 2))
    g = w.grad.permute(0, 2, 3, 1).contiguous()
    return (g if p['ow'] else g + torch.from_numpy(inp['dw0'])).numpy()


# ------------------------------------------------------------------------------------------------------------------ descriptors
def fill_prob(q, c, p, ptrs=None, ws_off=0):
    """l2s_wgrad_prob of problem p; ptrs: dict(dy=[..], x=[..], dw=..) of addresses (dummies of 1 MiB where absent: no launch)"""
    base = 1 << 20
    q.dw = ptrs['dw'] if ptrs else base
    q.nseg, q.Cin, q.Cout, q.KH, q.KW, q.stride, q.pad = len(p['segs']), p['Cin'], p['Cout'], p['KH'], p['KW'], p['stride'], p['pad']
    q.split, q.ws_off, q.flags = p['split'], ws_off if p['split'] > 1 else 0, 1 if p['ow'] else 0
    for s in range(len(p['segs'])):
        n, H, W, OH, OW = seg_geometry(p, s)
        q.dy[s], q.x[s] = (ptrs['dy'][s], ptrs['x'][s]) if ptrs else (base, base)
        q.n_img[s], q.IH[s], q.IW[s], q.OH[s], q.OW[s] = n, H, W, OH, OW
        q.lddy[s], q.ldx[s] = pitches(c, p, s)
    return q


def single_desc(c, p, ptrs=None, ws=None, ws_bytes=0):
    from lang2seg_amd import _lib
    base = 1 << 20
    n, H, W, OH, OW = seg_geometry(p, 0)
    d = _lib.WgradDesc()
    d.dy, d.x, d.dw = (ptrs['dy'][0], ptrs['x'][0], ptrs['dw']) if ptrs else (base, base, base)
    d.n_img, d.IH, d.IW, d.Cin, d.OH, d.OW, d.Cout = n, H, W, p['Cin'], OH, OW, p['Cout']
    d.KH, d.KW, d.stride, d.pad = p['KH'], p['KW'], p['stride'], p['pad']
    d.lddy, d.ldx = pitches(c, p, 0)
    d.split_k, d.tile, d.ws, d.ws_bytes = p['split'], c['tile'], ws, ws_bytes
    return d


def ws_layout(c):
    """(ws_off of every problem in floats, floats in all) of a grouped launch's split problems"""
    offs, off = [], 0
    for p in c['probs']:
        offs.append(off)
        if p['split'] > 1:
            off += p['split'] * p['Cout'] * p['KH'] * p['KW'] * p['Cin']
    return offs, off


def source(name):
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lang2seg_amd', 'csrc', name)).read()


def source_rings():
    """(ring of launch_single, ring of launch_grouped) per variant as (BM, BN, TX, D), the template arguments csrc/conv_wgrad.hip spells"""
    src = source('conv_wgrad.hip')
    ints = lambda args: tuple(int(a) for a in args.split(','))
    single = {3 if v == 'default' else int(v[5:]): ints(args) for v, args in re.findall(r'(case \d|default): return launch_single<T, ([\d, ]+)>', src)}
    grouped = {int(v): ints(args) for v, args in re.findall(r'case (\d): return launch_grouped<T, ([\d, ]+), KS>', src)}
    grouped[4] = ints(re.search(r'variant == 4\) return launch_grouped<bf16_t, ([\d, ]+)>', src).group(1))[:4]
    return single, grouped
