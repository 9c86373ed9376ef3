"""The frozen image prefix on the device - l2s_stem_conv + l2s_maxpool3x3s2, l2s_stem_pack + l2s_stem_pool_bf16, l2s_conv3x3_c3 and
l2s_bottleneck64_fwd - against the float64 references of tests/prefix_util.py, through the elementwise bound `check` of
tests/small_kernels_util.py (references, bounds, exact cases and the mutations they catch are pinned without a GPU by
tests/test_prefix_cpu.py).  Every case is one launch (a few for the probes) on a tiny map at the edges of the kernel's tiling:

  bottleneck64_kernel<DOWN>   maps of 1 x 1 to 18 x 76 around the 6 x 25 tile (one-pixel slivers, a tile with a foreign halo on all four sides),
                              both forms, with and without the next block's conv1.  'random': y and a_next inside the carried allowance of the
                              float64 chain; 'exact': operands on the integer grid, y and a_next equal to the reference; the probes: b, the
                              shortcut's operand path, the residual and a_next == y[:, 64 q:64 q + 64], each equal to what it must be
  stem_pool_mfma_kernel       every H in 9..16 with every W in 121..128 (every parity of H, OH, W, OW at the edge of the 3 x 31 pooled tile) and
                              four more shapes; 'random' inside the pooled bound, 'grid' and 'frac' (image values n + m / 256: the lo term
                              carries real data) equal to the reference
  stem_kernel, maxpool_kernel, conv3x3_c3_kernel   outputs of 1, 63, 64, 65 and a ragged few hundred pixels, f32 and bf16 stores; the pooling bit for
                              bit the pooling of the device's own convolution output

Every output lies between sentinel rows that have to come back bit-identical (a_next as a whole when no next conv1 is given), every input
carries the same padding and has to come back unchanged; operand views start on 16-byte boundaries, as the kernels require.

Worst values measured on an MI355X (this file's own prints, test_zz_worst_ratios; no threshold is derived from them):
  bottleneck64_fwd   'random' (y and a_next against the carried allowance) 0.773 (down), 0.772 (identity); 'probe_b' (b under the plain bound)
                     0.963, 0.952; every exact and probe case identical to its reference, every shape, both forms
  stem_pool_bf16     'random' 0.978; 'grid' and 'frac' identical at all 68 shapes
  stem_conv          0.0275 (f32), 0.98 (bf16 store); pooled 0.0257, 0.98; maxpool the exact maximum of the device's convolution output
  conv3x3_c3         0.146 (f32), 0.987 (bf16 store)
  (a ratio next to 1 is a bf16 store: half a unit in the last place is the whole allowance there)
  every sentinel intact, every input unchanged; 140 tests in 3.6 s
Tried on the device with the kernels changed (memory-safe changes, not kept): the left halo column of every tile but the first read one
pixel further left failed 'random', 'exact', 'probe_b' and 'probe_b_exact' on every map wider than one tile, with the figures the CPU
file's 'halo_off' mutation gives (7 x 26, down: 275 times the bound, 961 elements); conv row -1 let into the pooling windows failed every
kind of every stem shape.  The kernels as they are missed nothing."""
import numpy as np
import pytest
import torch

import prefix_util as PU
from prefix_util import BNECK_MAPS, STEM_EDGE, STEM_MORE, STEM_KINDS, STEM_CONV_MAPS, C3_MAPS
from small_kernels_util import check, F32, BF16, STORE
from gpu_buf import Buf, bits

pytestmark = pytest.mark.gpu

WORST = {}
SEEN = set()
KERNELS = sorted(['bottleneck64_kernel<true>', 'bottleneck64_kernel<false>', 'stem_pack_kernel', 'stem_pool_mfma_kernel', 'stem_kernel',
                  'maxpool_kernel', 'conv3x3_c3_kernel'])


def ops():
    from lang2seg_amd import ops as O
    return O


def pack_bytes():
    from lang2seg_amd import _lib
    return int(_lib.load().l2s_stem_pack_bytes())


def landed(kernel):
    k = ops().last_kernel()
    SEEN.add(k)
    assert k == kernel, 'the last launch was %s, this case is meant for %s' % (k, kernel)


def note(name, w):
    WORST[name] = max(WORST.get(name, 0.0), w)
    return w


def hw_id(hw):
    return '%dx%d' % hw


def padded(a, rows, cols, dt=F32, off=None):
    """an input between sentinel rows; off: elements before the view (a multiple of 16 bytes)"""
    off = cols if off is None else off
    assert (off * (2 if dt == BF16 else 4)) % 16 == 0
    return Buf(rows, cols, off=off, dt=dt, init=np.asarray(a, np.float32).reshape(rows, cols))


# ------------------------------------------------------------------------------------------------------------------ the fused bottleneck
def bneck_run(inp, down, with_next):
    O = ops()
    H, W = inp['a'].shape[:2]
    P, Cx = H * W, 64 if down else 256
    I = dict(a=padded(inp['a'], P, 64, BF16), x=padded(inp['x'], P, Cx, BF16), w2=padded(inp['w2'], 64, 576, BF16), w3=padded(inp['w3'], 256, 64, BF16),
             b2=padded(inp['b2'], 1, 64), b3=padded(inp['b3'], 1, 256))
    if down:
        I.update(wd=padded(inp['wd'], 256, 64, BF16), bd=padded(inp['bd'], 1, 256))
    if with_next:
        I.update(w1n=padded(inp['w1n'], 64, 256, BF16), b1n=padded(inp['b1n'], 1, 64))
    yb, anb = Buf(P, 256, off=256, dt=BF16), Buf(P, 64, off=64, dt=BF16)
    t = lambda k: I[k].t if k in I else None
    O.bottleneck64_fwd(t('a'), t('x').view(P, Cx), t('w2'), t('b2'), t('w3'), t('b3'), yb.t, H, W, wd=t('wd'), bd=t('bd'), w1n=t('w1n'), b1n=t('b1n'), a_next=anb.t)
    landed('bottleneck64_kernel<%s>' % ('true' if down else 'false'))
    y = yb.get()
    yb.assert_untouched_outside('y')
    for k, b in I.items():
        b.assert_unchanged(k)
    if with_next:
        anb.assert_untouched_outside('a_next')
        return y, anb.get()
    anb.assert_unchanged('a_next without the next conv1')
    return y, None


@pytest.mark.parametrize('down,kind', [(d, k) for d in (True, False) for k in PU.bneck_kinds(d)], ids=lambda v: v if isinstance(v, str) else 'down' if v else 'identity')
@pytest.mark.parametrize('hw', BNECK_MAPS, ids=hw_id)
def test_bottleneck64(hw, down, kind):
    H, W = hw
    w = note('bottleneck64_fwd %s %s' % ('down' if down else 'identity', kind), PU.bneck_case(bneck_run, H, W, down, kind))
    print('%dx%d %s %s: worst ratio %.3g' % (H, W, 'down' if down else 'identity', kind, w))


# ------------------------------------------------------------------------------------------------------------------ the stem
def stem_inputs(inp, H, W):
    return dict(img=padded(inp['img'], H * W, 3, off=12), w=padded(inp['w'], 64, 147, off=148), scale=padded(inp['scale'], 1, 64), bias=padded(inp['bias'], 1, 64))


def stem_pool_run(inp):
    O = ops()
    H, W = inp['img'].shape[:2]
    OH, OW, PH, PW = PU.stem_dims(H, W)
    I = stem_inputs(inp, H, W)
    nbytes = pack_bytes()
    pk = Buf(1, nbytes, off=16, dtype=torch.uint8, fill=90)
    O.stem_pack(I['w'].t, pack=pk.t)
    landed('stem_pack_kernel')
    pk.assert_untouched_outside('the packed weights')
    packed = pk.flat.clone()
    yb = Buf(PH * PW, 64, off=64, dt=BF16)
    O.stem_pool_bf16(I['img'].t, pk.t, I['scale'].t, I['bias'].t, yb.t, H, W, OH, OW, PH, PW)
    landed('stem_pool_mfma_kernel')
    got = yb.get().reshape(PH, PW, 64)
    yb.assert_untouched_outside('y')
    assert torch.equal(bits(pk.flat), bits(packed)), 'the packed weights changed'
    for k, b in I.items():
        b.assert_unchanged(k)
    return got


def test_stem_pool_tile_edges():
    """all 64 shapes around the edge of one 3 x 31 pooled tile, every kind"""
    for H, W in STEM_EDGE:
        for kind in STEM_KINDS:
            note('stem_pool_bf16 %s' % kind, PU.stem_pool_case(stem_pool_run, H, W, kind))
    print('stem_pool_bf16 at the tile edge: worst ratio %.3g' % WORST['stem_pool_bf16 random'])


@pytest.mark.parametrize('kind', STEM_KINDS)
@pytest.mark.parametrize('hw', STEM_MORE, ids=hw_id)
def test_stem_pool(hw, kind):
    w = note('stem_pool_bf16 %s' % kind, PU.stem_pool_case(stem_pool_run, hw[0], hw[1], kind))
    print('%dx%d %s: worst ratio %.3g' % (hw[0], hw[1], kind, w))


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('hw', STEM_CONV_MAPS, ids=hw_id)
def test_stem_conv_maxpool(hw, dt):
    O = ops()
    H, W = hw
    OH, OW, PH, PW = PU.stem_dims(H, W)
    what = 'stem_conv %dx%d %s' % (H, W, STORE[dt])
    inp = PU.stem_make(H, W)
    I = stem_inputs(inp, H, W)
    ref, ab, nt, _ = PU.stem_ref(inp)
    yb = Buf(OH * OW, 64, off=64, dt=dt)
    O.stem_conv(I['img'].t, I['w'].t, I['scale'].t, I['bias'].t, yb.t, H, W, OH, OW)
    landed('stem_kernel')
    y = yb.get().reshape(OH, OW, 64)
    w = note('stem_conv %s' % STORE[dt], check(y, ref, ab, nt, STORE[dt], what=what))
    yb.assert_untouched_outside(what)
    for k, b in I.items():
        b.assert_unchanged(k)
    conv_bits = yb.flat.clone()
    pb = Buf(PH * PW, 64, off=64, dt=dt)
    O.maxpool(yb.t, pb.t, OH, OW, 64, PH, PW)
    landed('maxpool_kernel')
    p = pb.get().reshape(PH, PW, 64)
    assert np.array_equal(p, PU.maxpool_emu(y)), '%s: the pooling is not the maximum of the device\'s own convolution output' % what
    wp = note('stem_conv + maxpool %s' % STORE[dt], PU.check_pooled(p, ref, PU.bound_of(ref, ab, nt, STORE[dt]), what + ' pooled'))
    pb.assert_untouched_outside(what + ' pooled')
    assert torch.equal(bits(yb.flat), bits(conv_bits)), '%s: the pooling changed its input' % what
    print('%s: worst ratio %.3g, pooled %.3g' % (what, w, wp))


@pytest.mark.parametrize('dt', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('hw', C3_MAPS, ids=hw_id)
def test_conv3x3_c3(hw, dt):
    O = ops()
    H, W = hw
    what = 'conv3x3_c3 %dx%d %s' % (H, W, STORE[dt])
    inp = PU.c3_make(H, W)
    I = dict(img=padded(inp['img'], H * W, 3, off=12), w=padded(inp['w'], 64, 27, off=28), bias=padded(inp['bias'], 1, 64))
    ref, ab, nt = PU.c3_ref(inp)
    yb = Buf(H * W, 64, off=64, dt=dt)
    O.conv3x3_c3(I['img'].t, I['w'].t, I['bias'].t, yb.t, H, W)
    landed('conv3x3_c3_kernel')
    w = note('conv3x3_c3 %s' % STORE[dt], check(yb.get().reshape(H, W, 64), ref, ab, nt, STORE[dt], what=what))
    yb.assert_untouched_outside(what)
    for k, b in I.items():
        b.assert_unchanged(k)
    print('%s: worst ratio %.3g' % (what, w))


def test_zz_worst_ratios():
    """prints what the docstring records and asserts the kernels seen (needs the whole file to have run in this process)"""
    print('worst check ratios:', ', '.join('%s %.3g' % kv for kv in sorted(WORST.items())))
    assert all(w <= 1.0 for w in WORST.values())
    assert sorted(SEEN) == KERNELS, (sorted(set(KERNELS) - SEEN), sorted(SEEN - set(KERNELS)))
