"""The references, bounds and exact cases of tests/prefix_util.py, pinned without a GPU.  Nothing of the device enters here.

Every case table of tests/test_prefix_gpu.py runs here with a torch-CPU float32 emulation of the kernel in the device's place (the kernel's
rounding points: the bf16 b, the unrounded shortcut convolution, hi + lo): the emulations pass every bound, are bit-exact on every exact and
probe case, and the conditions that make an exact case exact (integers, nothing stored beyond 256; for the fractional stem case hi + lo == x
and partial sums that are multiples of 2^-8 below 2^15) are asserted on the float64 reference of every one of them.

Then the emulation is mutated, and every mutation has to raise.  Which cases catch which mutation (asserted below, CAUGHT_BY; 7 x 26 map for
the bottleneck, 9 x 121 image for the stem):
  one product of the 3x3 dropped at pixel (0, 0)          random, exact, probe_b, probe_b_exact.  It is the LARGEST product of that pixel (0.2 of b), and the random
                                                          chain sees it in a y next to 0, where the allowance is small (19 times the bound); probe_b sees
                                                          it at 66 times the bound, the exact cases as a whole integer
  tap kx = 0 read one pixel off at the tile seam x = 25   random, exact, probe_b, probe_b_exact
  two k-values of one fragment exchanged in w2            random, exact, probe_b, probe_b_exact
  b2 added after the ReLU                                 random, exact, probe_b, probe_b_exact
  the residual added twice                                random, exact, probe_residual (probe_next stays silent throughout: it compares two outputs of one launch)
  the lo term of the image dropped                        random, frac (on random images only where the output is small: next to a large one lo's 2^-9 is
                                                          within the bf16 store's allowance; on the integer grid lo is 0)
  an out-of-map conv position entering a pooling window   random, grid, frac

Figures of this file's own prints (test_zz_figures: the worst ratio of the float32 emulations; a ratio next to 1 is a bf16 store next to a
rounding boundary, where half a unit in the last place is the whole allowance):
  bottleneck chain 0.773 (down), 0.772 (identity); b through probe_b 0.963, 0.952; every exact and probe case identical
  stem_pool_bf16 0.978; stem_conv 0.0303 (f32), 0.98 (bf16), pooled 0.0284, 0.98; conv3x3_c3 0.146 (f32), 0.987 (bf16)
  the largest stored value of an exact bottleneck case: b 39, y 108, a_next 188 (of 256)"""
import numpy as np
import pytest

import prefix_util as PU
from prefix_util import BNECK_MAPS, STEM_EDGE, STEM_MORE, STEM_KINDS, STEM_CONV_MAPS, C3_MAPS
from small_kernels_util import check, F32, BF16, STORE

WORST = {}


def note(name, w):
    WORST[name] = max(WORST.get(name, 0.0), w)
    return w


def hw_id(hw):
    return '%dx%d' % hw


def bneck_run(mut=None):
    def run(inp, down, with_next):
        y, an = PU.bneck_emu(inp, down, with_next, mut)
        return y, an
    return run


@pytest.mark.parametrize('down', [True, False], ids=['down', 'identity'])
@pytest.mark.parametrize('hw', BNECK_MAPS, ids=hw_id)
def test_bottleneck_emulation(hw, down):
    H, W = hw
    for kind in PU.bneck_kinds(down):
        w = note('bottleneck64 %s %s' % ('down' if down else 'identity', kind), PU.bneck_case(bneck_run(), H, W, down, kind))
        print('%dx%d %s %s: worst ratio %.3g' % (H, W, 'down' if down else 'identity', kind, w))


@pytest.mark.parametrize('down', [True, False], ids=['down', 'identity'])
@pytest.mark.parametrize('hw', BNECK_MAPS, ids=hw_id)
def test_bottleneck_exact_conditions(hw, down):
    """from the float64 reference alone: every stored tensor of every exact case holds integers, none beyond 256"""
    H, W = hw
    for kind in ('exact', 'probe_b_exact'):
        r = PU.chain_ref(PU.bneck_make(H, W, down, kind), down)
        mx = PU.exact_conditions(r)
        assert r['y'].max() >= 1 and r['b'].max() >= 1
        print('%dx%d %s %s: the largest b %g, y %g, a_next %g' % (H, W, 'down' if down else 'identity', kind, mx['b'], mx['y'], mx['an']))


def test_stem_pool_emulation():
    for H, W in STEM_EDGE + STEM_MORE:
        for kind in STEM_KINDS:
            if kind != 'random':
                z = PU.stem_exact_conditions(PU.stem_make(H, W, kind), kind)
                assert z.max() > 0
            note('stem_pool_bf16 %s' % kind, PU.stem_pool_case(PU.stem_pool_emu, H, W, kind))


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('hw', STEM_CONV_MAPS, ids=hw_id)
def test_stem_conv_emulation(hw, dt):
    H, W = hw
    inp = PU.stem_make(H, W)
    ref, ab, nt, _ = PU.stem_ref(inp)
    y = PU.stem_conv_emu(inp, dt)
    note('stem_conv %s' % STORE[dt], check(y, ref, ab, nt, STORE[dt], what='stem_conv %dx%d' % hw))
    note('stem_conv + maxpool %s' % STORE[dt], PU.check_pooled(PU.maxpool_emu(y), ref, PU.bound_of(ref, ab, nt, STORE[dt]), 'maxpool %dx%d' % hw))


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('hw', C3_MAPS, ids=hw_id)
def test_conv3x3_c3_emulation(hw, dt):
    inp = PU.c3_make(*hw)
    ref, ab, nt = PU.c3_ref(inp)
    note('conv3x3_c3 %s' % STORE[dt], check(PU.c3_emu(inp, dt), ref, ab, nt, STORE[dt], what='conv3x3_c3 %dx%d' % hw))


def test_pooled_bound_is_the_pool_of_the_bound():
    """the Lipschitz argument on numbers: two maps that differ by at most e elementwise have pooled values that differ by at most the
    pooled e, and the bound is sharp (a map moved by exactly e in its maxima moves the pooled value by the pooled e)"""
    rs = np.random.RandomState(3)
    u, e = rs.standard_normal((9, 11, 4)), rs.rand(9, 11, 4) * 0.1
    for v in (u + e, u - e, u + e * rs.uniform(-1, 1, u.shape)):
        assert (np.abs(PU.pool64(v) - PU.pool64(u)) <= PU.pool64(e) + 1e-15).all()
    flat = np.zeros((9, 11, 4))
    assert np.array_equal(PU.pool64(flat + e) - PU.pool64(flat), PU.pool64(e))
    with pytest.raises(AssertionError):
        PU.check_pooled(PU.pool64(flat + 1.01 * e), flat, e)


# ------------------------------------------------------------------------------------------------------------------ mutations
MUT_MAP = (7, 26)
MUT_IMG = (9, 121)
B4 = {'random', 'exact', 'probe_b', 'probe_b_exact'}
CAUGHT_BY = {
    ('drop_product', True): B4, ('drop_product', False): B4,
    ('halo_off', True): B4, ('halo_off', False): B4,
    ('kswap', True): B4, ('kswap', False): B4,
    ('bias_after_relu', True): B4, ('bias_after_relu', False): B4,
    ('residual_twice', False): {'random', 'exact', 'probe_residual'},
    'no_lo': {'random', 'frac'},
    'pool_pad': {'random', 'grid', 'frac'},
}


def raises(fn):
    try:
        fn()
    except AssertionError as e:
        return str(e).split('\n')[0][:150]
    return None


@pytest.mark.parametrize('mut,down', sorted(k for k in CAUGHT_BY if isinstance(k, tuple)), ids=lambda v: v if isinstance(v, str) else 'down' if v else 'identity')
def test_bottleneck_mutation_raises(mut, down):
    H, W = MUT_MAP
    caught = set()
    for kind in PU.bneck_kinds(down):
        why = raises(lambda: PU.bneck_case(bneck_run(mut), H, W, down, kind))
        if why:
            caught.add(kind)
            print('%s caught by %s: %s' % (mut, kind, why))
    assert caught == CAUGHT_BY[(mut, down)], (mut, down, sorted(caught))


@pytest.mark.parametrize('mut', ['no_lo', 'pool_pad'])
def test_stem_mutation_raises(mut):
    H, W = MUT_IMG
    caught = set()
    for kind in STEM_KINDS:
        why = raises(lambda: PU.stem_pool_case(lambda inp: PU.stem_pool_emu(inp, mut), H, W, kind))
        if why:
            caught.add(kind)
            print('%s caught by %s: %s' % (mut, kind, why))
    assert caught == CAUGHT_BY[mut], (mut, sorted(caught))


def test_a_store_two_steps_off_raises():
    """the allowance of a bf16 store is half a unit in the last place: a y two bf16 steps off fails the chain, a pooled stem value likewise.
    (a_next's carried allowance, the worst case over 256 channels of y's, is wider than that: a_next is held by the exact cases and by
    the selector probes, bit for bit)"""
    H, W = MUT_MAP
    inp = PU.bneck_make(H, W, False, 'random')
    r = PU.chain_ref(inp, False)
    y, an = PU.bneck_emu(inp, False, True)
    assert PU.check_chain(y, an, r) <= 1.0
    i = np.unravel_index(int(np.abs(r['y']).argmax()), r['y'].shape)
    bits = y.view(np.uint32).copy(); bits[i] += np.uint32(2 << 16)
    with pytest.raises(AssertionError):
        PU.check_chain(bits.view(np.float32), an, r)
    inp = PU.stem_make(*MUT_IMG)
    ref, ab, nt, extra = PU.stem_ref(inp, True)
    got = PU.stem_pool_emu(inp)
    bound = PU.bound_of(ref, ab, nt, 'bf16', extra)
    assert PU.check_pooled(got, ref, bound) <= 1.0
    i = np.unravel_index(int(got.argmax()), got.shape)
    bits = got.view(np.uint32).copy(); bits[i] += np.uint32(2 << 16)
    with pytest.raises(AssertionError):
        PU.check_pooled(bits.view(np.float32), ref, bound)


def test_zz_figures():
    """prints what the docstrings record (needs the whole file to have run in this process)"""
    print('worst check ratios of the float32 emulations:', ', '.join('%s %.3g' % kv for kv in sorted(WORST.items())))
    assert all(w <= 1.0 for w in WORST.values())
