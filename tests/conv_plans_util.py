"""l2s_conv_igemm (csrc/conv_igemm.hip): the case table that reaches every plan of conv_plan(), the float64 restatement of the convolution
with each epilogue form, and the operand layout the CPU and the GPU test files share.  The comparison is small_kernels_util.check,
unchanged:

    |got - ref| <= (n_terms + 2) * 2^-24 * absum + rho * |ref|,      rho = 2^-8 for a bf16 store, 0 for f32 / out_f32

with absum = |x| * |w| + |bias| + |add| and n_terms = K + 2 (K products summed in any order, the bias, the addend), plus the number of
slabs where a split over K is forced (one more float32 addition per slab).  ReLU is 1-Lipschitz, so the bound of the sum carries over;
where the `ref > 0` mask zeroes an output absum is 0 and the value has to be exact.  Every case has K <= 2040, i.e.
K (K + 4) 2^-24 < 1/4: one dropped or misplaced term (about absum / K) stands clear of the rounding allowance, and the out_f32 form of
each plan takes rho away altogether (tests/test_conv_plans_cpu.py mutates the reference and shows that `check` raises).

A CASE is a shape, a dtype, the tile / algo / split_k request and the plan l2s_conv_plan_name has to report for it; a FORM is an epilogue
(bias, addend, ReLU, ReLU-mask operand, out_f32, strided scatter, 2x2 pixel shuffle); a LAYOUT gives the row pitches and the offsets of
the bias / add / ref views in their buffers.  Where a plan does not take a form or a layout, the case names the plan it falls back to
(`fb`), by the reason: 'f32o', 'shuffle' (scatter or pixel shuffle), 'ref', 'pitch'.

Not in the table: igemm_dma_kernel<256,128,stamped> and the stamped igemm_ws64_kernel (instrumented builds for the tools, which write
clock stamps into `ws`), and the branches that need operands of 2 GiB or more."""
import numpy as np
import torch
import torch.nn.functional as TF

from small_kernels_util import bf16r, f64, stored_as, F32, BF16

ALGO_AUTO, ALGO_STAGED, ALGO_DMA, ALGO_PATCH, ALGO_KSPLIT, ALGO_KSPLIT_D3, ALGO_PDMA, ALGO_DMA256, ALGO_DMA196 = 0, 1, 2, 3, 5, 6, 7, 9, 10
CONV_RELU, CONV_OUT_F32, CONV_DECONV2X2, CONV_SCATTER = 1, 4, 8, 16

GENERIC64, GENERIC128 = 'igemm_kernel<64,64>', 'igemm_kernel<128,128>'
RING64, RING128, RING128X64 = 'igemm_ring_kernel<64,64>', 'igemm_ring_kernel<128,128>', 'igemm_ring_kernel<128,64>'
WS64, WS64_SPLITK = 'igemm_ws64_kernel', 'igemm_ws64_kernel + splitk_reduce_kernel'
KS64_D4, KS64_D3 = 'igemm_ks64_kernel<4>', 'igemm_ks64_kernel<3>'
SP224, SP256 = 'igemm_sp_kernel<224,128>', 'igemm_sp_kernel<256,128>'
DMA, DMA196, DMA256, PDMA = 'igemm_dma_kernel<256,128>', 'igemm_dma196_kernel', 'igemm_dma256_kernel', 'igemm_pdma_kernel<256,128>'
P3_32_256, P3_32_384, P3_64_256, P3_64_384 = 'igemm_p3_kernel<32,256>', 'igemm_p3_kernel<32,384>', 'igemm_p3_kernel<64,256>', 'igemm_p3_kernel<64,384>'
P3 = (P3_32_256, P3_32_384, P3_64_256, P3_64_384)
STAMPED = ('igemm_dma_kernel<256,128,stamped>',)           # (the stamped 64x64 tile reports the name of the plain one)
# the planner's list (PLAN_NAMES of csrc/conv_igemm.hip) without 'invalid'; tests/test_conv_plans_cpu.py reads the source's own list against it
ALL_PLANS = (GENERIC64, GENERIC128, RING64, RING128, WS64, KS64_D4, KS64_D3, SP224, SP256, DMA, WS64_SPLITK) + P3 + (RING128X64, PDMA, DMA256, DMA196) + STAMPED

# ------------------------------------------------------------------------------------------------------------------ forms
# bias, add, relu, ref, out_f32, and how the rows go out: None, 'scatter' (a 2H x 2W grid, stride 2, as Conv.dgrad issues the data gradient
# of a strided 1x1 convolution, add and ref in the scattered layout) or 'deconv' (Cout = 4 Cq, pixel-shuffled, as mask_up_sampling)
FORMS = {
    'plain': dict(),
    'bias': dict(bias=1),
    'relu': dict(relu=1),
    'fwd': dict(bias=1, add=1, relu=1),
    'dgrad': dict(ref=1),
    'dgrad_add': dict(add=1, ref=1),
    'f32o': dict(f32o=1),
    'f32o_fwd': dict(f32o=1, bias=1, add=1, relu=1),
    'scatter': dict(add=1, ref=1, shuffle='scatter'),
    'deconv': dict(bias=1, relu=1, shuffle='deconv'),
    'deconv_ref': dict(bias=1, ref=1, shuffle='deconv'),
}
for _f in FORMS.values():
    for _k in ('bias', 'add', 'relu', 'ref', 'f32o'):
        _f.setdefault(_k, 0)
    _f.setdefault('shuffle', None)

# ------------------------------------------------------------------------------------------------------------------ layouts
# pad columns of y / add / ref (elements; x always has a pitch of its own: Cin + 8 for bf16, Cin + 4 for f32) and the offsets of the bias
# (floats) and add / ref (4 bytes) views in their buffers.  'dense': the 16-byte-aligned, densely pitched operands of the LDS-staged
# epilogues; 'pad8': the same epilogues with pad columns to keep clean; 'odd': pitches that are no multiple of 4 (the scalar epilogue);
# 'off': 16-byte pitches, but bias / add / ref start 4 bytes into their buffers (not `plain`: the 8-byte vector epilogue)
LAYOUTS = {
    'dense': dict(pad=(0, 0, 0), off=0),
    'pad8': dict(pad=(8, 16, 24), off=0),
    'odd': dict(pad=(3, 5, 1), off=0),
    'off': dict(pad=(8, 16, 24), off=1),
}
GUARD = 8                # rows of sentinels in front of and behind x and y


def store_of(c, form):
    return 'f32' if (c['dt'] == F32 or FORMS[form]['f32o']) else 'bf16'


def geometry(c, form, lay):
    """-> dict of M, K, the output's rows / columns and every pitch of (case, form, layout)"""
    f, L = FORMS[form], LAYOUTS[lay]
    M = c['n'] * c['OH'] * c['OW']
    ocols = c['Cout'] // 4 if f['shuffle'] == 'deconv' else c['Cout']
    orows = c['n'] * 4 * c['H'] * c['W'] if f['shuffle'] else M
    py, pa, pr = L['pad']
    esz = 2 if c['dt'] == BF16 else 4
    return dict(M=M, K=c['KH'] * c['KW'] * c['Cin'], orows=orows, ocols=ocols, ldx=c['Cin'] + 16 // esz, ldy=ocols + py, ldadd=ocols + pa, ldref=ocols + pr,
                boff=L['off'], aoff=L['off'] * 4 // esz, nbias=ocols if f['shuffle'] == 'deconv' else c['Cout'])


# ------------------------------------------------------------------------------------------------------------------ cases
def _case(plan, n, H, W, Cin, Cout, k=1, dt=BF16, **o):
    KH, KW = o.pop('KH', k), o.pop('KW', k)
    stride, pad = o.pop('stride', 1), o.pop('pad', k // 2)
    c = dict(plan=plan, n=n, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, dt=dt,
             OH=(H + 2 * pad - KH) // stride + 1, OW=(W + 2 * pad - KW) // stride + 1,
             tile=o.pop('tile', 0), algo=o.pop('algo', 0), split=o.pop('split', 0), fb=o.pop('fb', {}), forms=o.pop('forms', None),
             lays=o.pop('lays', None), noref=o.pop('noref', False), big=o.pop('big', False), tag=o.pop('tag', ''))
    assert not o, o
    one = KH == 1 and KW == 1 and stride == 1 and pad == 0
    if c['forms'] is None:
        c['forms'] = ('plain', 'bias', 'relu', 'fwd', 'dgrad', 'dgrad_add', 'f32o', 'f32o_fwd') + (('scatter',) if one else ()) + \
                     (('deconv', 'deconv_ref') if one and Cout % 16 == 0 else ())
    if c['lays'] is None:
        c['lays'] = ('dense', 'pad8', 'odd', 'off') if Cout % 8 == 0 else ('dense', 'odd', 'off')
    c['id'] = '%dx%dx%d-%dto%d-%dx%d%s-%s%s%s%s%s' % (n, H, W, Cin, Cout, KH, KW, ('s%dp%d' % (stride, pad)) if (stride, pad) != (1, KH // 2) or KH != KW else '',
                                                    'bf16' if dt == BF16 else 'f32', ('-tile%d' % c['tile']) if c['tile'] else '', ('-algo%d' % c['algo']) if c['algo'] else '',
                                                    ('-split%d' % c['split']) if c['split'] else '', ('-' + c['tag']) if c['tag'] else '')
    return c


F32O = ('f32o', 'f32o_fwd')
BIG = dict(big=True, lays=('pad8',))
CASES = [
    # ---- generic tile: K tails (Cin no multiple of the 128-byte slice), forced split-K in f32 or with a float output
    _case(GENERIC64, 1, 9, 11, 96, 40),
    _case(GENERIC64, 1, 9, 11, 36, 40, dt=F32),
    _case(GENERIC64, 1, 6, 5, 256, 72, dt=F32, tile=64, split=2, fb=dict(shuffle=RING64, pitch=RING64), lays=('dense', 'pad8', 'odd', 'off')),
    _case(GENERIC64, 1, 6, 5, 256, 72, tile=64, split=2, forms=F32O, tag='f32o'),
    _case(GENERIC128, 1, 9, 11, 96, 136, tile=128),
    _case(GENERIC128, 1, 9, 11, 36, 136, dt=F32, tile=128),
    # ---- ring tiles
    _case(RING64, 1, 33, 64, 64, 1024, lays=('dense', 'off')),                                            # 528 tiles of one slice, bf16 store
    _case(RING64, 1, 9, 11, 64, 72, dt=F32),
    _case(RING64, 1, 9, 11, 128, 72, forms=F32O, tag='f32o'),
    _case(RING128, 3, 7, 7, 128, 136, 3, tile=128),
    _case(RING128, 3, 7, 7, 128, 136, 3, dt=F32, tile=128),
    _case(RING128, 3, 7, 7, 128, 144, 1, tile=128),                                                       # scatter and pixel shuffle on the 128x128 ring
    _case(RING128, 1, 50, 128, 64, 500, lays=('pad8',)),                                                   # the automatic rule: t128 = 200, Cout % 64
    _case(RING128X64, 1, 50, 128, 64, 512, fb=dict(f32o=RING128), lays=('dense', 'off')),                  # t128 = 200
    _case(RING128X64, 83, 7, 7, 192, 1024, fb=dict(f32o=RING128), lays=('dense', 'odd')),                # below the 256x256 tile's minimum; the pixel shuffle as mask_up_sampling meets it
    # ---- wave-specialised 64x64 tile
    _case(WS64, 1, 9, 11, 128, 72, fb=dict(f32o=RING64)),
    _case(WS64, 1, 9, 11, 128, 80, fb=dict(f32o=RING64)),                                                 # Cout % 16 == 0: pixel shuffle
    _case(WS64, 1, 9, 11, 128, 38, fb=dict(f32o=RING64), lays=('odd',)),                                  # ldy 41
    _case(WS64, 1, 9, 11, 64, 40, 3, stride=2, pad=1, fb=dict(f32o=RING64)),
    _case(WS64, 1, 9, 11, 64, 40, 5, fb=dict(f32o=RING64)),
    _case(WS64, 1, 9, 11, 64, 40, KH=1, KW=3, pad=0, fb=dict(f32o=RING64)),                               # OW = W - 2
    _case(WS64_SPLITK, 1, 6, 5, 256, 72, tile=64, split=2, fb=dict(f32o=GENERIC64, shuffle=WS64)),
    _case(WS64, 5, 7, 7, 64, 36, 3, algo=ALGO_DMA196, fb=dict(f32o=RING64), tag='from196'),                # Cout % 8: the 196-row tile does not take it
    _case(WS64, 5, 3, 3, 192, 38, algo=ALGO_PDMA, fb=dict(f32o=RING64), tag='frompdma'),                   # Cout % 4: nor does the persistent one
    _case(WS64, 2, 5, 6, 128, 40, 3, forms=('dgrad', 'dgrad_add'), tag='ref'),                             # the K-split tile takes no `ref` operand automatically
    # ---- software-pipelined tiles
    _case(SP224, 5, 7, 7, 128, 136, 3, dt=F32, tile=224),                                                  # taps innermost
    _case(SP224, 5, 7, 7, 128, 136, 1, tile=224),                                                          # 2 slices: below the LDS-DMA tile's minimum
    _case(SP224, 5, 7, 7, 128, 144, 1, tile=224),                                                          # scatter and pixel shuffle
    _case(SP224, 5, 7, 7, 128, 136, 1, dt=F32, tile=224),                                                  # f32 without taps
    _case(SP224, 1, 160, 256, 1024, 128, dt=F32, forms=('fwd',), big=True, lays=('odd',)),
    _case(SP224, 5, 7, 7, 128, 136, 3, tile=224, forms=F32O, tag='f32o'),                                  # bf16 operands, float store, taps innermost (a bf16 store goes to the LDS-DMA tile)
    _case(SP256, 6, 7, 7, 128, 136, 3, tile=256, forms=F32O, tag='f32o'),                                  # the same on 256 rows
    _case(SP256, 6, 7, 7, 128, 136, 1, tile=256),                                                          # bf16 store: the LDS-staged epilogue of the 256-row tile
    _case(SP256, 6, 7, 7, 128, 136, 1, dt=F32, tile=256),                                                  # f32 without taps
    _case(SP256, 6, 7, 7, 128, 144, 1, tile=256),                                                          # scatter and pixel shuffle
    _case(SP256, 6, 7, 7, 128, 136, 3, dt=F32, tile=256),
    # ---- LDS-DMA tiles
    _case(DMA, 6, 7, 7, 192, 136, algo=ALGO_DMA, fb=dict(f32o=RING64)),                                    # 3 slices: prologue and tail only
    _case(DMA, 6, 7, 7, 192, 256, algo=ALGO_DMA, fb=dict(f32o=RING64)),                                    # two column tiles; pixel shuffle
    _case(DMA, 6, 7, 7, 192, 38, algo=ALGO_DMA, fb=dict(f32o=RING64), lays=('odd',)),                      # ldy 41
    _case(DMA, 1, 160, 256, 128, 128, 3, forms=('fwd',), fb=dict(f32o=SP224), **BIG),
    _case(DMA196, 5, 7, 7, 64, 128, 3, algo=ALGO_DMA196, fb=dict(f32o=RING64, pitch=WS64)),
    _case(DMA256, 84, 7, 7, 192, 1024, fb=dict(f32o=RING128, shuffle=RING128X64, pitch=RING128X64),        # M = 4116: a ragged 17th row tile
          lays=('dense', 'odd', 'off')),
    _case(PDMA, 5, 3, 3, 192, 64, algo=ALGO_PDMA, fb=dict(f32o=RING64, shuffle=WS64, pitch=WS64)),
    _case(PDMA, 5, 3, 3, 192, 36, algo=ALGO_PDMA, fb=dict(f32o=RING64, shuffle=WS64, pitch=WS64)),
    # ---- K-split 64x64 tile
    _case(KS64_D4, 2, 5, 6, 128, 38, 3, fb=dict(f32o=RING64, ref=WS64), noref=True),
    _case(KS64_D4, 1, 9, 11, 128, 72, algo=ALGO_KSPLIT, fb=dict(f32o=RING64)),
    _case(KS64_D4, 1, 9, 11, 128, 80, algo=ALGO_KSPLIT, fb=dict(f32o=RING64)),                             # pixel shuffle
    _case(KS64_D3, 1, 9, 11, 128, 72, algo=ALGO_KSPLIT_D3, fb=dict(f32o=RING64)),
    # ---- patch tiles (3x3 / stride 1 / pad 1 on one map)
    _case(P3_32_256, 1, 5, 9, 64, 40, 3, fb=dict(f32o=RING64)),
    _case(P3_32_256, 1, 5, 9, 64, 38, 3, fb=dict(f32o=RING64), lays=('odd',)),                             # ldy 41
    _case(P3_32_384, 1, 3, 70, 64, 40, 3, fb=dict(f32o=RING64)),
    _case(P3_64_256, 1, 32, 60, 64, 576, 3, fb=dict(f32o=RING64), lays=('dense', 'odd')),
    _case(P3_64_384, 1, 20, 100, 64, 544, 3, fb=dict(f32o=RING64), lays=('dense', 'odd')),
]
assert len({c['id'] for c in CASES}) == len(CASES)
NO_F32O = (DMA, DMA196, DMA256, PDMA, WS64, WS64_SPLITK, KS64_D4, KS64_D3, RING128X64) + P3     # bf16 stores only
NO_SHUFFLE = (DMA196, DMA256, PDMA, WS64_SPLITK)


def case_lays(c):
    return [(c, lay) for lay in c['lays']]


def pitch_ok(c, form, lay):
    """what the 196-row, 256x256 and persistent tiles and the split ask of the pitches and pointers (conv_plan(), csrc/conv_igemm.hip)"""
    g, f = geometry(c, form, lay), FORMS[form]
    lds = g['ldy'] | g['ldadd'] | g['ldref'] | c['Cout']
    if c['plan'] == PDMA:
        return lds % 4 == 0
    if c['plan'] == DMA256:
        return lds % 4 == 0 and (g['ldy'] | c['Cout']) % 8 == 0
    if c['plan'] == DMA196:
        return lds % 8 == 0 and not (g['boff'] and f['bias']) and not (g['aoff'] and (f['add'] or f['ref']))
    if c['split']:
        return c['Cout'] % 4 == 0
    return True


def expected_plan(c, form, lay):
    """the plan of (case, form, layout): the case's own, or the fallback it names for the first reason that excludes the form"""
    f = FORMS[form]
    if f['f32o'] and c['dt'] == BF16 and c['plan'] in NO_F32O:
        return c['fb']['f32o']
    if f['shuffle'] and (c['plan'] in NO_SHUFFLE or c['split']):
        return c['fb']['shuffle']
    if f['ref'] and c['noref']:
        return c['fb']['ref']
    if not pitch_ok(c, form, lay):
        return c['fb']['pitch']
    return c['plan']


def n_tiles64(c):
    return -(-(c['n'] * c['OH'] * c['OW']) // 64) * -(-c['Cout'] // 64)


# ------------------------------------------------------------------------------------------------------------------ operands and references
_INPUTS, _PRODUCTS, _TORCH = {}, {}, {}


def _rnd(rs, shape, dt, scale=1.0):
    a = (rs.standard_normal(shape) * scale).astype(np.float32)
    return bf16r(a) if dt == BF16 else a


def make(c):
    """the operands as the device sees them (bf16 values rounded first), float32: x [n][H][W][Cin], w [Cout][KH][KW][Cin], bias [Cout], and
    add / ref for each way the rows go out (None: [M][Cout]; 'scatter': [n 2H 2W][Cout]; 'deconv': [4 M][Cout / 4])"""
    if c['id'] not in _INPUTS:
        rs = np.random.RandomState(sum(ord(ch) * (i + 1) for i, ch in enumerate(c['id'])) % (2 ** 31))
        K, M, dt = c['KH'] * c['KW'] * c['Cin'], c['n'] * c['OH'] * c['OW'], c['dt']
        d = dict(x=_rnd(rs, (c['n'], c['H'], c['W'], c['Cin']), dt), w=_rnd(rs, (c['Cout'], c['KH'], c['KW'], c['Cin']), dt, K ** -0.5), bias=_rnd(rs, (c['Cout'],), F32))
        shapes = {None: (M, c['Cout'])}
        if 'scatter' in c['forms']:
            shapes['scatter'] = (c['n'] * 4 * c['H'] * c['W'], c['Cout'])
        if 'deconv' in c['forms']:
            shapes['deconv'] = (4 * M, c['Cout'] // 4)
        for s, shp in shapes.items():
            d['add', s], d['ref', s] = _rnd(rs, shp, dt), _rnd(rs, shp, dt)
        _INPUTS[c['id']] = d
    return _INPUTS[c['id']]


def product64(c, inp=None, last_tap_pad=0):
    """(x * w, |x| * |w|) as [M][Cout] float64, one matmul per filter tap; last_tap_pad: the last tap's extra pad (a mutation of the CPU tests)"""
    x, w = f64((inp or make(c))['x']), f64((inp or make(c))['w'])
    p, s, OH, OW = c['pad'] + 1, c['stride'], c['OH'], c['OW']
    xp = np.pad(x, ((0, 0), (p, p + s), (p, p + s), (0, 0)))
    M = c['n'] * OH * OW
    P, A = np.zeros((M, c['Cout'])), np.zeros((M, c['Cout']))
    for kh in range(c['KH']):
        for kw in range(c['KW']):
            o = 1 - (last_tap_pad if (kh, kw) == (c['KH'] - 1, c['KW'] - 1) else 0)
            sl = xp[:, o + kh:o + kh + s * OH:s, o + kw:o + kw + s * OW:s, :].reshape(M, c['Cin'])
            wt = w[:, kh, kw, :].T
            P += sl @ wt
            A += np.abs(sl) @ np.abs(wt)
    return P, A


def shuffle_rows(c):
    """output row of GEMM row m under the scatter form: pixel (2 oy, 2 ox) of a 2H x 2W grid"""
    img, oy, ox = np.unravel_index(np.arange(c['n'] * c['OH'] * c['OW']), (c['n'], c['OH'], c['OW']))
    return (img * 2 * c['H'] + 2 * oy) * (2 * c['W']) + 2 * ox


def pixel_shuffle(c, a):
    """[M][4 Cq] (column (dy 2 + dx) Cq + co) -> [n 2OH 2OW][Cq]"""
    n, OH, OW, Cq = c['n'], c['OH'], c['OW'], c['Cout'] // 4
    return a.reshape(n, OH, OW, 2, 2, Cq).transpose(0, 1, 3, 2, 4, 5).reshape(n * 4 * OH * OW, Cq)


def conv_ref64(c, form, inp=None, prod=None):
    """-> (ref64, absum64, n_terms) of one case and form, on the rows the launch writes: [M][Cout]; under 'scatter' the same rows (they go to
    shuffle_rows(c) of the output), under the pixel shuffle [4 M][Cout / 4] in the output's own order.  add and ref are read at the output's
    row and column, as the kernels do."""
    f = FORMS[form]
    inp = inp or make(c)
    if prod is None:
        if c['id'] not in _PRODUCTS:
            _PRODUCTS[c['id']] = product64(c)
        prod = _PRODUCTS[c['id']]
    z, ab = prod
    sh = f['shuffle']
    if sh == 'deconv':
        z, ab = pixel_shuffle(c, z), pixel_shuffle(c, ab)
    rows = shuffle_rows(c) if sh == 'scatter' else slice(None)
    if f['bias']:
        b = f64(inp['bias'])[:z.shape[1]]
        z, ab = z + b, ab + np.abs(b)
    if f['add']:
        a = f64(inp['add', sh])[rows]
        z, ab = z + a, ab + np.abs(a)
    if f['relu']:
        z = np.maximum(z, 0)
    if f['ref']:
        keep = f64(inp['ref', sh])[rows] > 0
        z, ab = np.where(keep, z, 0.0), np.where(keep, ab, 0.0)
    # a forced split adds its slabs in float32, one more rounding each (the shuffled forms are never split)
    return z, ab, c['KH'] * c['KW'] * c['Cin'] + 2 + (c['split'] if not sh else 0)


def conv_f32(c, form):
    """the same through torch on the CPU in float32 (conv2d; conv_transpose2d for the two shuffled layouts), stored as the device stores it"""
    f, inp = FORMS[form], make(c)
    n, OH, OW, Cout, sh = c['n'], c['OH'], c['OW'], c['Cout'], f['shuffle']
    if (c['id'], sh) not in _TORCH:
        x = torch.from_numpy(inp['x']).permute(0, 3, 1, 2)
        w = torch.from_numpy(inp['w'])
        if sh == 'deconv':
            z = TF.conv_transpose2d(x, w.view(2, 2, Cout // 4, c['Cin']).permute(3, 2, 0, 1), None, stride=2)            # [n][Cq][2H][2W]
        elif sh == 'scatter':
            z = TF.conv_transpose2d(x, w.view(Cout, c['Cin']).t().reshape(c['Cin'], Cout, 1, 1), None, stride=2, output_padding=1)
        else:
            z = TF.conv2d(x, w.permute(0, 3, 1, 2), None, stride=c['stride'], padding=c['pad'])
        _TORCH[c['id'], sh] = z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])
    z = _TORCH[c['id'], sh]
    if f['bias']:
        z = z + torch.from_numpy(inp['bias'])[:z.shape[1]]
    if f['add']:
        z = z + torch.from_numpy(inp['add', sh])
    if f['relu']:
        z = torch.relu(z)
    if f['ref']:
        z = torch.where(torch.from_numpy(inp['ref', sh]) > 0, z, torch.zeros(()))
    if sh == 'scatter':
        z = z[torch.from_numpy(shuffle_rows(c))]
    return stored_as(z.contiguous(), BF16 if store_of(c, form) == 'bf16' else F32)


# ------------------------------------------------------------------------------------------------------------------ descriptor without a launch
def plan_name(c, form, lay, base=1 << 20):
    """l2s_conv_plan_name on a descriptor with dummy pointers (no launch, no GPU)"""
    import ctypes as C
    from lang2seg_amd import _lib
    f, g = FORMS[form], geometry(c, form, lay)
    esz = 2 if c['dt'] == BF16 else 4
    d = _lib.ConvDesc()
    d.x = d.w = d.y = base
    d.bias = base + 4 * g['boff'] if f['bias'] else None
    d.add = base + esz * g['aoff'] if f['add'] else None
    d.ref = base + esz * g['aoff'] if f['ref'] else None
    d.n_img, d.IH, d.IW, d.Cin, d.OH, d.OW, d.Cout = c['n'], c['H'], c['W'], c['Cin'], c['OH'], c['OW'], c['Cout']
    d.KH, d.KW, d.stride, d.pad = c['KH'], c['KW'], c['stride'], c['pad']
    d.ldx, d.ldy, d.ldadd, d.ldref = g['ldx'], g['ldy'], g['ldadd'], g['ldref']
    d.flags = (CONV_RELU if f['relu'] else 0) | (CONV_OUT_F32 if f['f32o'] else 0) | (CONV_DECONV2X2 if f['shuffle'] == 'deconv' else 0) | (CONV_SCATTER if f['shuffle'] == 'scatter' else 0)
    if f['shuffle'] == 'scatter':
        d.out_h, d.out_w, d.out_stride = 2 * c['H'], 2 * c['W'], 2
    d.tile, d.split_k, d.xcd_mode, d.algo = c['tile'], c['split'], -1, c['algo']
    if c['split']:
        d.ws, d.ws_floats = base, c['split'] * g['M'] * c['Cout']
    return _lib.load().l2s_conv_plan_name(C.byref(d), _lib.BF16 if c['dt'] == BF16 else _lib.F32).decode()


def planner_names():
    """PLAN_NAMES as csrc/conv_igemm.hip spells it, in order, 'invalid' first"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lang2seg_amd', 'csrc', 'conv_igemm.hip')).read()
    body = re.search(r'PLAN_NAMES\[\]\s*=\s*\{(.*?)\};', src, re.S).group(1)
    return re.findall(r'"([^"]*)"', body)
