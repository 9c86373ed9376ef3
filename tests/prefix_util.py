"""The frozen image prefix - the stem (csrc/misc_kernels.hip stem_kernel + maxpool_kernel, csrc/stem_mfma.hip stem_pack_kernel +
stem_pool_mfma_kernel), VGG's conv1_1 (conv3x3_c3_kernel) and the fused frozen layer1 (csrc/bottleneck_fused.hip bottleneck64_kernel<DOWN>):
shapes, float64 references, bounds and the checks the CPU and the GPU test files share.  The comparison is `check` of
tests/small_kernels_util.py,

    |got - ref| <= (n_terms + 2) * 2^-24 * absum + rho * |ref| (+ an absolute term where one is derived below),

and every reference sees the operands the device sees (bf16 operands rounded first, then widened to float64) and returns
(ref64, absum64, n_terms).  U = 2^-24 below.  None of the numbers below comes from a kernel's output.

stem_conv, both store types.  ref = relu((img * w) scale + bias), absum = (|img| * |w|) |scale| + |bias|, n_terms = 147 + 2 (147 products,
the scale, the bias).  conv3x3_c3: ref = relu(img * w + bias), n_terms = 27 + 1.

The 3x3 / stride 2 pooling is a maximum: |max(u) - max(v)| <= max |u - v| over the window (1-Lipschitz in the sup norm), so the bound of a
pooled value is the same max-pool applied to the array of bounds (`check_pooled`: the whole bound is handed to `check` as its absolute
term).  The pooling kernel itself is held bit for bit to the pooling of the device's own convolution output.

stem_pool_bf16.  The same reference with the weights rounded to bf16 (stem_pack_kernel rounds them).  The image keeps two bf16 terms:
hi = bf16(x), |x - hi| <= 2^-9 |x|; lo = bf16(x - hi), |x - hi - lo| <= 2^-9 |x - hi| <= 2^-18 |x|, so the convolution sees an image that is
off by 2^-18 |x| at the most and the bound gains `extra` = 2^-18 (|img| * |w|) |scale|, returned next to the reference.  Each of the 7
k-steps of 32 (the zero-weight pad counted) runs for hi and for lo: n_terms = 2 * 7 * 32 + 2.  The store's rho applies to the convolution
value BEFORE the maximum (the kernel rounds, then pools), then the bound is pooled.

bottleneck64_fwd.  Rounding an intermediate to bf16 in float64 can fall on the other side of a rounding boundary than the kernel's
float32 value, so the references of b, y and a_next are the UNROUNDED float64 chain and the allowance is carried forward (`chain_ref`,
`check_chain`); ReLU is 1-Lipschitz throughout, so every allowance passes through it unchanged:
  b      = relu(a * w2 + b2):       e_b    = (576 + 3) U absum_2 + 2^-9 (|b64| + that)         absum_2 = |a| * |w2| + |b2|
           (576 products and the bias, two of slack; then the store of b into LDS: half a unit in the last place of the kernel's value,
           which is within the first term of b64)
  y_pre  = b w3 + b3 + shortcut:    e_ypre = |w3| e_b + (n3 + 2) U absum_3                     absum_3 = |b64| |w3| + |b3| + (|x| or |x| |wd| + |bd|)
           n3 = 64 (+ 64 for the shortcut convolution) + 2 biases + the residual, counted alike for both forms (each needs one less: the
           first block adds bd onto b3 and has no residual, the others have one bias); the error of b enters through |w3|
  y      = relu(y_pre), bf16:       e_ypre + rho |y64|
  a_pre  = y w1n + b1n:             e_apre = |w1n| (e_ypre + 2^-8 |y64|) + (256 + 3) U absum_1    absum_1 = |y64| |w1n| + |b1n|
  a_next = relu(a_pre), bf16:       e_apre + rho |a64|
In `check`'s terms: y is checked with absum_3, n3 and the absolute term |w3| e_b; a_next with absum_1, n_terms 257 and the absolute term
|w1n| (e_ypre + 2^-8 |y64|).

The carried 2^-9 |b| is about as large as one dropped product of the 3x3, so the bottleneck and the MFMA stem also get EXACT cases, in which
nothing rounds: activations in {0, 1, 2}, weights in {-1, 0, 1}, integer biases, scale 1.  Every float32 partial sum is then an integer
below 2^24, exact in any order, and every stored value is exact in bf16 as long as it does not exceed 256 - a condition on the inputs that
tests/test_prefix_cpu.py asserts on the float64 reference of every exact case.  The result has to equal the reference as a number (a zero
of either sign is zero).  For the stem a second exact case has image values n + m / 256, n < 128: 15 significant bits, so hi + lo = x
exactly and the lo MFMA carries real data; every partial sum is a multiple of 2^-8 below 2^15 (147 x 128 < 2^15: 23 bits), still exact;
the one bf16 rounding of the output is the reference's rounding of the exact value, and the maximum of rounded values follows.

PROBE weights make the bottleneck's hidden tensors visible:
  'probe_b'         w3[co][ci] = (co % 64 == ci), b3 = 0, x = 0 (and wd = bd = 0): y[:, co] == b[:, co % 64], so b falls under the plain `check`
                    bound with n_terms = 578 and a bf16 store; with grid operands b is exact
  'probe_shortcut'  w3 = 0, b3 = bd = 0, wd = the same selector (Cx = 64): y[:, co] == relu(x[:, co % 64]), exact - the shortcut's operand path
  'probe_residual'  w3 = 0 (Cx = 256): y == relu(x + b3) rounded once (one float32 addition, restated in numpy float32, then the bf16 store)
  'probe_next'      w1n = one of four selectors of 64 channels, b1n = 0: a_next == y[:, 64 q:64 q + 64] of the y the same launch stored

A `run` callable stands for the device: the GPU file launches the kernel between sentinel rows, the CPU file runs the float32 emulations
of this file (`bneck_emu`, `stem_pool_emu`, ...: torch-CPU float32 with the kernel's rounding points - the bf16 b, the unrounded shortcut
convolution, hi + lo) and their mutations through the same checks."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from small_kernels_util import BF16, U24, RHO_BF16, f64, bf16r, check

# ------------------------------------------------------------------------------------------------------------------ shapes
TH, TW = 6, 25                        # the bottleneck's tile: 6 rows x 25 columns
# (1,1) one pixel; (5,24) one ragged tile; (6,25) exactly one; (7,26) four tiles with one-pixel slivers; (6,50) / (12,25) two whole tiles side by
# side / above each other; (13,51) nine tiles, the middle one with a foreign halo on all four sides; (18,76) three whole rows of tiles, four columns
BNECK_MAPS = [(1, 1), (5, 24), (6, 25), (7, 26), (6, 50), (12, 25), (13, 51), (18, 76)]
BNECK_KINDS = ['random', 'exact', 'probe_b', 'probe_b_exact', 'probe_shortcut', 'probe_residual', 'probe_next']
# the MFMA stem's workgroup = 3 x 31 pooled = 7 x 64 conv = 19 x 134 image: H in 9..16 gives OH in 5..8 and PH in {3, 4}, W in 121..128 gives OW
# in 61..64 and PW in {31, 32}: every parity of H, OH, W and OW at the tile edge
STEM_EDGE = [(H, W) for H in range(9, 17) for W in range(121, 129)]
STEM_MORE = [(1, 1), (2, 3), (5, 250), (131, 9)]
STEM_KINDS = ['random', 'grid', 'frac']
# stem_kernel / conv3x3_c3_kernel: 64 output pixels per workgroup.  Image sizes whose OUTPUT has 1, 1, 63, 63, 64, 65 and 437 / 312 pixels
STEM_CONV_MAPS = [(1, 1), (2, 2), (13, 17), (14, 18), (15, 16), (9, 26), (37, 45), (24, 51)]
C3_MAPS = [(1, 1), (7, 9), (8, 8), (4, 16), (5, 13), (19, 23), (12, 26)]         # 1, 63, 64, 64, 65, 437 and 312 pixels


def stem_dims(H, W):
    OH, OW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    return OH, OW, (OH + 2 - 3) // 2 + 1, (OW + 2 - 3) // 2 + 1


assert sorted(set(stem_dims(H, W)[0] * stem_dims(H, W)[1] for H, W in STEM_CONV_MAPS)) == [1, 63, 64, 65, 312, 437]
assert sorted(set(H * W for H, W in C3_MAPS)) == [1, 63, 64, 65, 312, 437]
assert set(stem_dims(H, W)[2:] for H, W in STEM_EDGE) == {(3, 31), (3, 32), (4, 31), (4, 32)}


# ------------------------------------------------------------------------------------------------------------------ float64 pieces
def conv64(x, w, stride=1, pad=0):
    """x [H][W][C], w [O][KH][KW][C] -> [OH][OW][O], float64 (sums of integers below 2^53 are exact)"""
    t = F.conv2d(torch.from_numpy(f64(x)).permute(2, 0, 1)[None], torch.from_numpy(f64(w)).permute(0, 3, 1, 2), stride=stride, padding=pad)
    return t[0].permute(1, 2, 0).contiguous().numpy()


def pool64(a):
    """[OH][OW][C] -> 3x3 / stride 2 / pad 1 maximum (the padding never wins), float64"""
    t = F.max_pool2d(torch.from_numpy(f64(a)).permute(2, 0, 1)[None], 3, 2, 1)
    return t[0].permute(1, 2, 0).contiguous().numpy()


def bound_of(ref, ab, n_terms, store, extra=0.0):
    """the bound `check` applies, as an array"""
    return (n_terms + 2) * U24 * f64(ab) + (RHO_BF16 if store == 'bf16' else 0.0) * np.abs(f64(ref)) + extra


def check_pooled(got, conv_ref, conv_bound, what=''):
    """a pooled result against the pooled reference, within the pooled bound of the convolution values (this file's docstring)"""
    return check(got, pool64(conv_ref), 0.0, 0, 'f32', floor=pool64(conv_bound), what=what)


def assert_exact(got, ref64, what=''):
    got, ref = f64(got), f64(ref64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~(got == ref)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError('%s: %d of %d elements differ from the exact result; the first, %s: %.9g, exact %.9g' % (what, int(bad.sum()), bad.size, i, got[i], ref[i]))
    return 0.0


def seed_of(*k):
    return (sum((i + 1) * 7919 * int(v) for i, v in enumerate(k)) + 12345) % (2 ** 31)


# ------------------------------------------------------------------------------------------------------------------ stem and conv1_1
def stem_make(H, W, kind='random'):
    """img [H][W][3] f32, w [64][7][7][3] f32, scale, bias [64]"""
    rs = np.random.RandomState(seed_of(H, W, STEM_KINDS.index(kind)))
    if kind == 'random':
        return dict(img=(rs.standard_normal((H, W, 3)) * 60 + 10).astype(np.float32), w=(rs.standard_normal((64, 7, 7, 3)) * 0.02).astype(np.float32),
                    scale=(rs.rand(64) + 0.5).astype(np.float32), bias=(rs.standard_normal(64) * 0.3).astype(np.float32))
    if kind == 'grid':
        img = rs.randint(0, 3, (H, W, 3)).astype(np.float32)
    else:
        img = (rs.randint(0, 128, (H, W, 3)) + rs.randint(0, 256, (H, W, 3)) / 256.0).astype(np.float32)
    w = (rs.randint(-1, 2, (64, 7, 7, 3)) * (rs.rand(64, 7, 7, 3) < 0.6)).astype(np.float32)
    return dict(img=img, w=w, scale=np.ones(64, np.float32), bias=rs.randint(-3, 4, 64).astype(np.float32))


def stem_ref(inp, w_bf16=False):
    """-> (conv values after ReLU, absum, n_terms, extra): before the pooling.  w_bf16: the MFMA path (bf16 weights, the image as hi + lo)"""
    w = bf16r(inp['w']) if w_bf16 else inp['w']
    sc, bi = f64(inp['scale']), f64(inp['bias'])
    z, ab = conv64(inp['img'], w, 2, 3) * sc + bi, conv64(np.abs(inp['img']), np.abs(w), 2, 3) * np.abs(sc)
    if w_bf16:
        return np.maximum(z, 0), ab + np.abs(bi), 2 * 7 * 32 + 2, 2.0 ** -18 * ab
    return np.maximum(z, 0), ab + np.abs(bi), 147 + 2, 0.0


def c3_make(H, W):
    rs = np.random.RandomState(seed_of(H, W, 77))
    return dict(img=(rs.standard_normal((H, W, 3)) * 30).astype(np.float32), w=(rs.standard_normal((64, 3, 3, 3)) * 0.02).astype(np.float32),
                bias=(rs.standard_normal(64) * 0.1).astype(np.float32))


def c3_ref(inp):
    bi = f64(inp['bias'])
    return np.maximum(conv64(inp['img'], inp['w'], 1, 1) + bi, 0), conv64(np.abs(inp['img']), np.abs(inp['w']), 1, 1) + np.abs(bi), 27 + 1


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32))


def conv32(x, w, stride=1, pad=0):
    """torch-CPU float32: x [H][W][C] tensor, w [O][KH][KW][C] tensor -> [OH][OW][O]"""
    return F.conv2d(x.permute(2, 0, 1)[None], w.permute(0, 3, 1, 2), stride=stride, padding=pad)[0].permute(1, 2, 0).contiguous()


def rb(t):
    return t.bfloat16().float()


def stem_conv_emu(inp, dt):
    z = torch.relu(conv32(t32(inp['img']), t32(inp['w']), 2, 3) * t32(inp['scale']) + t32(inp['bias']))
    return (rb(z) if dt == BF16 else z).numpy()


def c3_emu(inp, dt):
    z = torch.relu(conv32(t32(inp['img']), t32(inp['w']), 1, 1) + t32(inp['bias']))
    return (rb(z) if dt == BF16 else z).numpy()


def maxpool_emu(y):
    """3x3 / 2 / pad 1 of [OH][OW][C] float32 values: a maximum rounds nothing"""
    return F.max_pool2d(t32(y).permute(2, 0, 1)[None], 3, 2, 1)[0].permute(1, 2, 0).contiguous().numpy()


def stem_pool_emu(inp, mut=None):
    """the MFMA stem in torch-CPU float32: bf16 weights, the image as hi + lo, affine + ReLU in float32, one rounding to bf16, then the
    maximum with conv positions outside the map counted as 0.  The convolution runs on the map extended by one position on every side
    (conv rows -1 .. OH, as the kernel's tiles compute them) and the positions outside are cleared.
    mut: 'no_lo' = the lo term dropped; 'pool_pad' = the positions outside the map are NOT cleared: they enter the windows with what the
    convolution gives there"""
    img, w = t32(inp['img']), rb(t32(inp['w']))
    H, W = img.shape[:2]
    OH, OW, PH, PW = stem_dims(H, W)
    hi = rb(img)
    lo = rb(img - hi)
    c = conv32(hi, w, 2, 5)
    if mut != 'no_lo':
        c = c + conv32(lo, w, 2, 5)
    v = rb(torch.relu(c * t32(inp['scale']) + t32(inp['bias'])))
    assert v.shape[:2] == (OH + 2, OW + 2)
    if mut != 'pool_pad':
        inside = torch.zeros(OH + 2, OW + 2, 1)
        inside[1:OH + 1, 1:OW + 1] = 1
        v = v * inside
    out = F.max_pool2d(v.permute(2, 0, 1)[None], 3, 2, 0)[0].permute(1, 2, 0).contiguous().numpy()
    assert out.shape[:2] == (PH, PW)
    return out


def stem_exact_conditions(inp, kind):
    """what makes an exact stem case exact, from the inputs and the float64 reference alone"""
    z = conv64(inp['img'], inp['w'], 2, 3) + f64(inp['bias'])
    ab = conv64(np.abs(inp['img']), np.abs(inp['w']), 2, 3) + np.abs(f64(inp['bias']))
    assert np.array_equal(bf16r(inp['w']), inp['w']) and (inp['scale'] == 1).all()
    if kind == 'grid':
        assert np.array_equal(z, np.round(z)) and np.maximum(z, 0).max() <= 256 and ab.max() < 2 ** 24
    else:
        hi = bf16r(inp['img'])
        lo = bf16r(inp['img'] - hi)
        big = inp['img'].size >= 100                                                              # (a 1 x 1 image has three values)
        assert np.array_equal(f64(hi) + f64(lo), f64(inp['img'])) and (lo != 0).mean() > (0.5 if big else 0)   # two terms carry the image exactly, and lo is real data
        assert np.array_equal(ab * 256, np.round(ab * 256)) and ab.max() < 2 ** 15              # every partial sum: a multiple of 2^-8 below 2^15
        pos = z[z > 0]
        assert pos.size and (f64(bf16r(pos.astype(np.float32))) != pos).mean() > (0.5 if big else 0)   # the output's rounding is real
    return z


def stem_pool_case(run, H, W, kind):
    """run(inp) -> pooled [PH][PW][64] float32 values; -> the worst ratio (0 for an exact case)"""
    inp = stem_make(H, W, kind)
    got = run(inp)
    what = 'stem_pool_bf16 %dx%d %s' % (H, W, kind)
    if kind == 'random':
        ref, ab, nt, extra = stem_ref(inp, True)
        return check_pooled(got, ref, bound_of(ref, ab, nt, 'bf16', extra), what)
    z = conv64(inp['img'], inp['w'], 2, 3) + f64(inp['bias'])
    return assert_exact(got, pool64(f64(bf16r(np.maximum(z, 0).astype(np.float32)))), what)


# ------------------------------------------------------------------------------------------------------------------ the fused bottleneck
def selector(rows, cols, q=0):
    """[rows][cols]: rows < cols: row r picks column cols-block q (r == k - rows q); rows > cols: row r picks column r % cols"""
    s = np.zeros((rows, cols), np.float32)
    if rows > cols:
        s[np.arange(rows), np.arange(rows) % cols] = 1
    else:
        s[np.arange(rows), rows * q + np.arange(rows)] = 1
    return s


def sparse(rs, shape, density):
    return (rs.choice([-1.0, 1.0], shape) * (rs.rand(*shape) < density)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _bneck_base(H, W, down, grid):
    rs = np.random.RandomState(seed_of(H, W, down, grid))
    Cx = 64 if down else 256
    if grid:
        act = lambda C: rs.choice([0.0, 1.0, 2.0], (H, W, C), p=[0.5, 0.3, 0.2]).astype(np.float32)
        ints = lambda n: rs.randint(-2, 3, n).astype(np.float32)
        return dict(a=act(64), x=act(Cx), w2=sparse(rs, (64, 3, 3, 64), 0.1), w3=sparse(rs, (256, 64), 0.1), wd=sparse(rs, (256, 64), 0.1),
                    w1n=sparse(rs, (64, 256), 0.03), b2=ints(64), b3=ints(256), bd=ints(256), b1n=ints(64))
    n = lambda shape, s=1.0: bf16r((rs.standard_normal(shape) * s).astype(np.float32))
    bias = lambda k: (rs.standard_normal(k) * 0.2).astype(np.float32)
    return dict(a=np.maximum(n((H, W, 64)), 0), x=np.maximum(n((H, W, Cx)), 0), w2=n((64, 3, 3, 64), 1 / 24.0), w3=n((256, 64), 1 / 8.0),
                wd=n((256, 64), 1 / 8.0), w1n=n((64, 256), 1 / 16.0), b2=bias(64), b3=bias(256), bd=bias(256), b1n=bias(64), xs=n((H, W, Cx)))


def bneck_make(H, W, down, kind, q=0):
    """the operands of one case, NHWC / [O][KH][KW][I] float32 arrays that hold bf16 values (biases: float32)"""
    d = dict(_bneck_base(H, W, down, kind in ('exact', 'probe_b_exact')))
    xs = d.pop('xs', None)
    zero = lambda k: np.zeros_like(d[k])
    if kind in ('probe_b', 'probe_b_exact'):
        d.update(w3=selector(256, 64), b3=zero('b3'), x=zero('x'), wd=zero('wd'), bd=zero('bd'))
    elif kind == 'probe_shortcut':
        d.update(w3=zero('w3'), b3=zero('b3'), wd=selector(256, 64), bd=zero('bd'), x=xs)
    elif kind == 'probe_residual':
        d.update(w3=zero('w3'), x=xs)
    elif kind == 'probe_next':
        d.update(w1n=selector(64, 256, q), b1n=zero('b1n'))
    return d


def chain_ref(inp, down, with_next=True):
    """the unrounded float64 chain and its carried allowances (this file's docstring); arrays [H W][C]"""
    H, W = inp['a'].shape[:2]
    b2, b3 = f64(inp['b2']), f64(inp['b3'])
    x = f64(inp['x']).reshape(H * W, -1)
    w3, wd, w1n = f64(inp['w3']), f64(inp['wd']), f64(inp['w1n'])
    r = dict(n_b=576 + 1, n_a=256 + 1)
    zb = conv64(inp['a'], inp['w2'], 1, 1).reshape(H * W, 64) + b2
    r['ab2'] = conv64(np.abs(inp['a']), np.abs(inp['w2']), 1, 1).reshape(H * W, 64) + np.abs(b2)
    r['b'] = b = np.maximum(zb, 0)
    e1 = (r['n_b'] + 2) * U24 * r['ab2']
    r['e_b'] = e1 + 2.0 ** -9 * (b + e1)
    zy, ab3 = b @ w3.T + b3, b @ np.abs(w3).T + np.abs(b3)
    if down:
        zy, ab3 = zy + x @ wd.T + f64(inp['bd']), ab3 + np.abs(x) @ np.abs(wd).T + np.abs(f64(inp['bd']))
    else:
        zy, ab3 = zy + x, ab3 + np.abs(x)
    r['n_y'] = 64 + (64 if down else 0) + 2 + 1
    r['ab3'], r['carry_y'] = ab3, r['e_b'] @ np.abs(w3).T
    r['e_ypre'] = r['carry_y'] + (r['n_y'] + 2) * U24 * ab3
    r['y'] = y = np.maximum(zy, 0)
    if with_next:
        r['ab1'] = y @ np.abs(w1n).T + np.abs(f64(inp['b1n']))
        r['carry_a'] = (r['e_ypre'] + 2.0 ** -8 * y) @ np.abs(w1n).T
        r['an'] = np.maximum(y @ w1n.T + f64(inp['b1n']), 0)
    return r


def check_chain(got_y, got_an, r, what=''):
    """y and a_next of one launch against the chain's references, each within its carried allowance; -> the worst ratio"""
    w = check(got_y, r['y'], r['ab3'], r['n_y'], 'bf16', floor=r['carry_y'], what=what + ' y')
    if got_an is not None:
        w = max(w, check(got_an, r['an'], r['ab1'], r['n_a'], 'bf16', floor=r['carry_a'], what=what + ' a_next'))
    return w


def exact_conditions(r):
    """every stored tensor of an exact case: integers, none beyond 256, and something to see"""
    for k in ('b', 'y', 'an'):
        assert np.array_equal(r[k], np.round(r[k])) and r[k].max() <= 256, (k, r[k].max())
    assert max(r['ab2'].max(), r['ab3'].max(), r['ab1'].max()) < 2 ** 24
    return dict((k, float(r[k].max())) for k in ('b', 'y', 'an'))


def bneck_case(run, H, W, down, kind):
    """run(inp, down, with_next) -> (y [H W][256], a_next [H W][64] or None), float32 values of what was stored; -> the worst ratio"""
    what = 'bottleneck64 %dx%d %s %s' % (H, W, 'down' if down else 'identity', kind)
    worst = 0.0
    if kind == 'probe_next':
        for q in range(4):
            y, an = run(bneck_make(H, W, down, kind, q), down, True)
            assert_exact(an, y[:, 64 * q:64 * q + 64], '%s q=%d' % (what, q))
        return worst
    inp = bneck_make(H, W, down, kind)
    if kind == 'random':
        r = chain_ref(inp, down)
        y, an = run(inp, down, True)
        worst = check_chain(y, an, r, what)
        y2, none = run(inp, down, False)
        assert none is None
        assert np.array_equal(y2, y), '%s: y differs without the next block\'s conv1' % what
    elif kind == 'exact':
        r = chain_ref(inp, down)
        y, an = run(inp, down, True)
        assert_exact(y, r['y'], what + ' y')
        assert_exact(an, r['an'], what + ' a_next')
    elif kind in ('probe_b', 'probe_b_exact'):
        r = chain_ref(inp, down, False)
        y, _ = run(inp, down, False)
        if kind == 'probe_b':
            worst = check(y, np.tile(r['b'], 4), np.tile(r['ab2'], 4), 578, 'bf16', what=what)
        else:
            assert_exact(y, np.tile(r['b'], 4), what)
    elif kind == 'probe_shortcut':
        y, _ = run(inp, down, False)
        assert_exact(y, np.tile(np.maximum(f64(inp['x']).reshape(H * W, 64), 0), 4), what)
    elif kind == 'probe_residual':
        y, _ = run(inp, down, False)
        v = inp['x'].reshape(H * W, 256).astype(np.float32) + inp['b3'].astype(np.float32)       # one float32 addition, as the kernel's
        assert_exact(y, bf16r(np.maximum(v, np.float32(0))), what)
    return worst


def bneck_kinds(down):
    return [k for k in BNECK_KINDS if k != ('probe_residual' if down else 'probe_shortcut')]


MUTATIONS = ['drop_product', 'halo_off', 'kswap', 'bias_after_relu', 'residual_twice']


def bneck_emu(inp, down, with_next, mut=None):
    """the kernel in torch-CPU float32 with its rounding points: b rounded to bf16, the shortcut convolution NOT rounded, y rounded once,
    a_next from the rounded y.  mut:
      'drop_product'     one product of the 3x3 missing at pixel (0, 0): the largest one of a channel that is positive with and without it
      'halo_off'         tap kx = 0 of the second tile column's first pixels (x = 25) reads a one pixel further left than it should
      'kswap'            input channels 3 and 4 (one 8-wide fragment) of the 3x3's centre tap exchanged in the weights
      'bias_after_relu'  b = relu(conv) + b2
      'residual_twice'   the identity shortcut added twice"""
    a, x = t32(inp['a']), t32(inp['x'])
    H, W = a.shape[:2]
    w2, b2 = t32(inp['w2']), t32(inp['b2'])
    if mut == 'kswap':
        w2 = w2.clone()
        w2[:, 1, 1, [3, 4]] = w2[:, 1, 1, [4, 3]]
    zb = conv32(a, w2, 1, 1) + b2
    if mut == 'drop_product':
        prod = a[0, 0][None, :] * w2[:, 1, 1, :]                                       # [co][ci]
        ok = (zb[0, 0] > 0)[:, None] & ((zb[0, 0][:, None] - prod) > 0) & (prod != 0)
        assert bool(ok.any()), 'no product to drop at pixel (0, 0)'
        co, ci = np.unravel_index(int((prod.abs() * ok).argmax()), prod.shape)
        zb[0, 0, co] -= prod[co, ci]
    if mut == 'halo_off':
        assert W > TW
        ap = F.pad(a, (0, 0, 2, 2, 1, 1))                                              # columns -2 .. W + 1, rows -1 .. H
        wrong, right = ap[:, TW - 2 + 2], ap[:, TW - 1 + 2]                              # columns TW - 2 and TW - 1 of the map
        for ky in range(3):
            zb[:, TW] += (wrong[ky:ky + H] - right[ky:ky + H]) @ w2[:, ky, 0, :].t()
    b = rb(torch.relu(zb - b2) + b2) if mut == 'bias_after_relu' else rb(torch.relu(zb))
    b = b.reshape(H * W, 64)
    x = x.reshape(H * W, -1)
    zy = b @ t32(inp['w3']).t() + t32(inp['b3'])
    zy = zy + (x @ t32(inp['wd']).t() + t32(inp['bd']) if down else x)
    if mut == 'residual_twice':
        assert not down
        zy = zy + x
    y = rb(torch.relu(zy))
    if not with_next:
        return y.numpy(), None
    return y.numpy(), rb(torch.relu(y @ t32(inp['w1n']).t() + t32(inp['b1n']))).numpy()
