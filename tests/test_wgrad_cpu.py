"""tests/wgrad_util.py without a GPU, on the built library's host functions only (nothing is launched): the case table reaches what its
docstring lists (each item asserted from the case fields and the kernels' constants, which are read against the source), l2s_wgrad_variant
maps the automatic cases to their variants and is pinned at every boundary of variant_of, l2s_wgrad_tiles and l2s_wgrad_ws_bytes agree
with their formulas, the two entries refuse what they cannot take before their first launch, the float64 reference and its bound hold for
torch autograd on the CPU in float32 (the reference written a second way), and the bound sees structure: seven mutations of the reference,
each one misplaced term, make `check` raise.

Not covered here or on the device: the tools-build knobs (wgrad_grid_cap, row3_form, row3_plan_mode: 0 in the product library) and operands
of 2 GiB or more."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import wgrad_util as WU
from wgrad_util import SINGLE, GROUPED
from small_kernels_util import check, f64, U24, F32, BF16

EINVAL = 1


def lib():
    from lang2seg_amd import _lib
    return _lib.load()


def by(entry=None, variant=None, dt=None):
    return [c for c in WU.CASES if (entry is None or c['entry'] == entry) and (variant is None or c['variant'] == variant) and (dt is None or c['dt'] == dt)]


def probs(cases):
    return [(c, p) for c in cases for p in c['probs']]


# ------------------------------------------------------------------------------------------------------------------ the table
def test_constants_are_the_sources():
    single, grouped = WU.source_rings()
    assert {v: t[3] for v, t in single.items()} == WU.RING_SINGLE and {v: t[3] for v, t in grouped.items()} == WU.RING_GROUPED
    for v, t in list(single.items()) + list(grouped.items()):
        assert t[:3] == WU.TILE[v], (v, t)
    src = WU.source('conv_wgrad.hip')
    assert re.search(r'WGT<bf16_t> \{ static constexpr int BKP = 32;', src) and re.search(r'WGT<float> \{ static constexpr int BKP = 16;', src)
    assert 'GO(bf16_t, 2)' in src and 'GO(float, 1)' in src                       # KSTEP: 64-pixel slices in grouped bf16 launches
    assert re.search(r'launch_grouped<bf16_t, 256, 256, 1, 2, 1, 4, 2>', src)     # variant 4: KSTEP 1
    assert re.search(r'constexpr int BM = 128, BN = 128, BKP = 64', WU.source('conv_wgrad_dma.hip'))
    assert re.search(r'constexpr int BM = 256, BN = 256, KP = 32', WU.source('conv_wgrad_dma1.hip'))
    assert re.search(r'L2S_KNOB\(wgrad_row3_dma_wgs, %d\)' % WU.V5_WGS, WU.source('knobs.h'))
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'lang2seg_hip.h')).read()
    assert '#define L2S_WGRAD_MAX_GROUP %d' % WU.MAX_GROUP in hdr and '#define L2S_WGRAD_MAX_SEG %d' % WU.MAX_SEG in hdr
    for knob in ('wgrad_grid_cap', 'row3_form', 'row3_plan_mode'):
        assert re.search(r'L2S_KNOB\(%s, 0\)' % knob, WU.source('knobs.h'))


def test_every_case_is_small_and_aligned():
    for c, p in probs(WU.CASES):
        M = sum(WU.pixels(p))
        assert M <= WU.M_MAX and M * (M + 4) * U24 < 0.25, c['id']
        ve = 8 if c['dt'] == BF16 else 4
        assert p['Cin'] % ve == 0 and p['Cout'] % ve == 0 and 1 <= len(p['segs']) <= WU.MAX_SEG
        lds = [WU.pitches(c, p, s) for s in range(len(p['segs']))]
        for (lddy, ldx) in lds:
            assert lddy % ve == 0 and ldx % ve == 0                               # every row starts 16-byte aligned
            if p['lay'] == 'pitched':
                assert lddy > p['Cout'] and ldx > p['Cin'] and lddy - p['Cout'] != ldx - p['Cin']
        if p['lay'] == 'pitched' and len(lds) == 2:
            assert lds[0][0] != lds[1][0] and lds[0][1] != lds[1][1]
        assert c['entry'] == GROUPED or (len(c['probs']) == 1 and len(p['segs']) == 1 and not p['ow'])
        assert p['split'] == 1 or c['variant'] < 5
        if WU.row3(c['variant']):
            assert WU.is_row3_shape(p), c['id']
        if c['variant'] == 6:
            assert (p['KH'], p['KW'], p['stride'], p['pad']) == WU.K1 and p['Cin'] % 256 == 0 and p['Cout'] % 256 == 0
        if c['variant'] == 5:
            assert p['Cin'] % 128 == 0 and p['Cout'] % 128 == 0


def test_table_reaches_every_kernel():
    reached = set()
    for c in WU.CASES:
        reached.add(WU.main_kernel(c))
        fam = WU.last_kernel_family(c)
        if fam != WU.main_kernel(c)[0]:
            reached.add(fam)
        if c['pair'] == 4:
            reached.add(('wgrad_grouped_kernel', 4, BF16))
    assert reached == WU.ALL_KERNELS, reached ^ WU.ALL_KERNELS
    # the list itself: every instantiation the two entries can dispatch to (four variants x two dtypes each, variant 4 in bf16) and the two LDS-DMA kernels
    src = WU.source('conv_wgrad.hip')
    assert len(re.findall(r'return launch_single<T,', src)) == 4 and len(re.findall(r'return launch_grouped<T,', src)) == 4
    assert len(re.findall(r'GO\(bf16_t', src)) == 2 and len(re.findall(r'GO\(float', src)) == 2
    kernels = set(re.findall(r'__global__ .*? void (\w+)\(', src + WU.source('conv_wgrad_dma.hip') + WU.source('conv_wgrad_dma1.hip')))
    assert kernels == {k if isinstance(k, str) else k[0] for k in WU.ALL_KERNELS}, kernels


def test_ring_occupancy():
    """for every (entry, variant, dtype) of conv_wgrad.hip the slice counts NS of one workgroup and segment reach 1, 2, D, D + 1, 2D - 1, 2D, 2D + 1
    and a value of at least 3D + 1"""
    for entry, ring in ((SINGLE, WU.RING_SINGLE), (GROUPED, WU.RING_GROUPED)):
        for v, D in ring.items():
            for dt in (BF16, F32):
                if v == 4 and dt == F32:
                    continue
                seen = {ns for c, p in probs(by(entry, v, dt)) for ns in WU.wg_slices(c, p)}
                for want in (1, 2, D, D + 1, 2 * D - 1, 2 * D, 2 * D + 1):
                    assert want in seen, (entry, v, dt, want, sorted(seen))
                assert max(seen) >= 3 * D + 1, (entry, v, dt)
                assert 0 in seen or entry == SINGLE, (entry, v, dt)               # a range without slices of one segment (NS == 0)


def test_pixel_geometry():
    for entry, v, dt in sorted({(c['entry'], c['variant'], c['dt']) for c in WU.CASES}):
        b = WU.slice_pixels(entry, v, dt)
        e = 1 if WU.row3(v) else 0
        has = dict(short=False, small=False, wide=False, ragged=False, exact=False)
        for c, p in probs(by(entry, v, dt)):
            for s in range(len(p['segs'])):
                n, H, W, OH, OW = WU.seg_geometry(p, s)
                mv = n * OH * (OW + e)
                has['short'] |= mv < b
                has['small'] |= n > 1 and OH * (OW + e) <= b                      # sa >= 1
                has['wide'] |= OW + e > b                                          # sa = sb = 0
                has['ragged'] |= mv % b != 0
                has['exact'] |= mv % b == 0
        if v == 6:                                                                 # (one flat list of pixels per segment: no image walk)
            has['small'] = has['wide'] = True
        assert all(has.values()), (entry, v, dt, has)


def test_taps_and_tails():
    for dt in (BF16, F32):
        pertap = {(p['KH'], p['KW'], p['stride'], p['pad']) for v in (0, 1) for c, p in probs(by(None, v, dt))}
        assert pertap >= {WU.K1, WU.K1S2, WU.K3S2, WU.K13, WU.K5, WU.K3P0, WU.K3}, pertap      # K3: the filter-row shape forced onto the per-tap tiles
        for c, p in probs(by(None, None, dt)):
            if (p['KH'], p['KW'], p['stride'], p['pad']) == WU.K1S2:
                assert all(H % 2 and W % 2 for (_, H, W) in p['segs'])
            if (p['KH'], p['KW'], p['stride'], p['pad']) == WU.K3P0:
                assert not WU.same_hw(p) and c['variant'] in (0, 1)
            if (p['KH'], p['KW'], p['stride'], p['pad']) == WU.K13:
                assert all(WU.seg_geometry(p, s)[4] == p['segs'][s][2] - 2 for s in range(len(p['segs'])))
        for v in (2, 3):
            assert any(WU.is_row3_shape(p) for c, p in probs(by(None, v, dt)))
    # channel tails on every tile prob_ok admits (variants 5 and 6 take whole tiles only): Cout and Cin both off the tile, two values each
    ve = {BF16: 8, F32: 4}
    for entry, v, dt in sorted({(c['entry'], c['variant'], c['dt']) for c in WU.CASES if c['variant'] < 5}):
        bm, bn, _ = WU.TILE[v]
        co = {p['Cout'] for c, p in probs(by(entry, v, dt)) if p['Cout'] % bm}
        ci = {p['Cin'] for c, p in probs(by(entry, v, dt)) if p['Cin'] % bn}
        assert len(co) >= 2 and len(ci) >= 2 and (bm > 64 or min(co) < bm < max(co)) and (bn > 64 or min(ci) < bn < max(ci)), (entry, v, dt, co, ci)
        assert all(x % ve[dt] == 0 for x in co | ci)
    assert any(p['Cin'] == 36 for c, p in probs(by(None, None, F32)))
    assert {(p['Cout'], p['Cin']) for c, p in probs(by(GROUPED, 4, BF16))} >= {(264, 280), (280, 264)}


def test_segments_splits_and_tables():
    for v, dt in sorted({(c['variant'], c['dt']) for c in by(GROUPED) if c['variant'] < 5}):
        two = [(c, p) for c, p in probs(by(GROUPED, v, dt)) if len(p['segs']) == 2]
        px = [WU.pixels(p) for _, p in two]
        assert any(a < b for a, b in px) and any(a > b for a, b in px), (v, dt)
        assert any(min(WU.slices(c, p)) < p['split'] for c, p in two), (v, dt)      # NS == 0 for some ranges of the shorter segment
        mixed = [c for c in by(GROUPED, v, dt) if any(p['split'] > 1 for p in c['probs']) and any(p['split'] == 1 for p in c['probs'])]
        assert mixed and any(sum(p['split'] > 1 for p in c['probs']) >= 2 for c in mixed), (v, dt)
        for c in mixed:
            offs, total = WU.ws_layout(c)
            assert total > 0 and any(o > 0 and p['split'] > 1 for o, p in zip(offs, c['probs']))                   # ws_off > 0
        assert any(p['ow'] and p['split'] > 1 for c, p in probs(by(GROUPED, v, dt))) and any(not p['ow'] and p['split'] > 1 for c, p in probs(by(GROUPED, v, dt)))
        # tables: one problem, several problems of different tile counts, a tile total that is no multiple of 8, 64 problems
        cs = by(GROUPED, v, dt)
        assert any(len(c['probs']) == 1 for c in cs)
        assert any(len({WU.tiles(v, p) * p['split'] for p in c['probs']}) >= 3 for c in cs)
        assert any(sum(WU.tiles(v, p) * p['split'] for p in c['probs']) % 8 for c in cs if len(c['probs']) > 1)
        assert dt == F32 and v > 0 or any(len(c['probs']) == WU.MAX_GROUP for c in cs), (v, dt)
    for v, dt in sorted({(c['variant'], c['dt']) for c in by(SINGLE)}):
        sp = {(p['split'], WU.eff_split(c, p), WU.slices(c, p)[0]) for c, p in probs(by(SINGLE, v, dt))}
        assert {s[0] for s in sp} >= {1, 2, 3}
        assert any(a == b == n for a, b, n in sp if a > 1) and any(a > b == n for a, b, n in sp), sp                # equal to / clamped to the slice count


def test_variants_5_and_6():
    v5 = by(GROUPED, 5)
    S = [sum(WU.slices(c, c['probs'][0])) for c in v5 if len(c['probs']) == 1]
    assert set(S) >= {1, 2, 3, 4, 5}                                                   # four LDS stages, three slices in flight
    U = [sum(WU.tiles(5, p) * sum(WU.slices(c, p)) for p in c['probs']) for c in v5]
    assert any(u < 8 for u in U) and any(8 <= u < 24 * 8 for u in U) and any(u >= 24 * 8 for u in U)               # every G clamp of the launcher
    assert all(1 <= WU.v5_workgroups(u) <= u for u in U)
    # a tile shared by three or more workgroups: two workgroups' ranges together are shorter than the tile's slices
    assert any(len(c['probs']) == 1 and 2 * -(-u // WU.v5_workgroups(u)) < sum(WU.slices(c, c['probs'][0])) for c, u in zip(v5, U))
    assert any(len({sum(WU.slices(c, p)) for p in c['probs']}) >= 3 for c in v5)
    assert any(len(c['probs']) == WU.MAX_GROUP for c in v5)
    v6 = by(GROUPED, 6)
    assert {sum(WU.slices(c, c['probs'][0])) for c in v6 if len(c['probs']) == 1} >= {1, 2, 3, 4}
    assert any(len(p['segs']) == 2 and WU.pixels(p)[0] % 32 for c, p in probs(v6))     # a ragged last slice of segment 0, then segment 1
    assert any(len(c['probs']) == WU.MAX_GROUP for c in v6)
    assert all(c['pair'] == 4 for c in v6 if len(c['probs']) < WU.MAX_GROUP)
    for cs in (v5, v6):
        ps = [p for _, p in probs(cs)]
        assert any(len(p['segs']) == 2 for p in ps) and any(p['lay'] == 'pitched' for p in ps)
        assert any(p['ow'] for p in ps) and any(not p['ow'] for p in ps)


# ------------------------------------------------------------------------------------------------------------------ host functions
def variant_of(p, M, tile, same=None):
    return int(lib().l2s_wgrad_variant(p['Cin'], p['Cout'], p['KH'], p['KW'], p['stride'], p['pad'], int(WU.same_hw(p) if same is None else same), M, tile))


def test_variant_of_the_cases():
    autos = set()
    for c in WU.CASES:
        for p in c['probs']:
            if c['entry'] == SINGLE:
                assert variant_of(p, WU.pixels(p)[0], c['tile']) == c['variant'], c['id']
            if c['auto']:
                assert variant_of(p, max(WU.pixels(p)), 256 if c['dt'] == BF16 else 0) == c['variant'], c['id']        # as WgradQueue.flush asks
                autos.add((c['variant'], c['dt']))
    assert autos == {(0, BF16), (2, BF16), (3, BF16), (5, BF16), (0, F32), (2, F32), (3, F32)}


def test_variant_boundaries():
    """variant_of (csrc/conv_wgrad.hip) under the product's request: tile 256 in bf16, 0 in f32"""
    one = lambda Cin, Cout: WU.P([(1, 8, 8)], Cin, Cout, k=1)
    three = lambda Cin, Cout: WU.P([(1, 8, 8)], Cin, Cout, k=3)
    # 1x1: the 256x256 tile from 8192 pixels and 512 channels on both sides, multiples of 256; variant 6 is on request only (wgrad_1x1_dma = 0)
    assert variant_of(one(512, 512), 8192, 256) == 4 and variant_of(one(512, 512), 8191, 256) == 0
    assert variant_of(one(512, 768), 8192, 256) == 4 and variant_of(one(512, 640), 8192, 256) == 1               # Cout % 256
    assert variant_of(one(640, 512), 8192, 256) == 1 and variant_of(one(768, 512), 8192, 256) == 4               # Cin % 256
    assert variant_of(one(511, 512), 8192, 256) == 0 and variant_of(one(512, 511), 8192, 256) == 0               # 512 channels on both sides
    assert variant_of(one(512, 512), 8192, 0) == 1 and variant_of(one(512, 512), 8191, 0) == 0                   # f32: no 256x256 tile
    assert variant_of(one(512, 512), 8192, 256, same=0) == 4                                                      # (a strided 1x1 keeps the register-staged tile)
    # 3x3 / 1 / 1: the LDS-DMA filter-row tile from 8192 pixels, or from 512 channels on both sides; multiples of 128; same_hw
    assert variant_of(three(128, 128), 8192, 256) == 5 and variant_of(three(128, 128), 8191, 256) == 2
    assert variant_of(three(512, 512), 1, 256) == 5 and variant_of(three(511, 512), 100, 256) == 3 and variant_of(three(512, 511), 100, 256) == 2
    assert variant_of(three(128, 192), 8192, 256) == 2 and variant_of(three(192, 128), 8192, 256) == 2           # % 128
    assert variant_of(three(128, 576), 8192, 256) == 3 and variant_of(three(128, 640), 8192, 256) == 5
    assert variant_of(three(512, 512), 8192, 256, same=0) == 0 and variant_of(three(512, 512), 8192, 0) == 3 and variant_of(three(128, 128), 8192, 0) == 2
    assert variant_of(three(512, 512), 8192, 128) == 3 and variant_of(three(512, 512), 8192, 64) == 2
    assert variant_of(one(64, 64), 100, 128) == 1 and variant_of(one(64, 64), 100, 64) == 0


def test_tiles_formula():
    L = lib()
    for c, p in probs(WU.CASES):
        bm, bn, tx = WU.TILE[c['variant']]
        want = -(-p['Cout'] // bm) * -(-p['Cin'] // bn) * (p['KH'] if tx == 3 else p['KH'] * p['KW'])
        assert int(L.l2s_wgrad_tiles(c['variant'], p['Cin'], p['Cout'], p['KH'], p['KW'])) == want == WU.tiles(c['variant'], p), c['id']


def plan_split(c, p, split_k):
    """plan_split() of csrc/conv_wgrad.hip with an unbounded workspace"""
    ns = WU.slices(c, p)[0]
    split = split_k
    if split <= 0:
        split = min(-(-256 // WU.tiles(c['variant'], p)), max(ns // 8, 1))
    return min(max(min(split, ns), 1), 64)


def test_ws_bytes():
    L = lib()
    seen = set()
    for c, p in probs(by(SINGLE)):
        slab = p['Cout'] * p['KH'] * p['KW'] * p['Cin'] * 4
        for split_k in (p['split'], 0, 2, 100):
            d = WU.single_desc(c, dict(p, split=split_k))
            sp = plan_split(c, p, split_k)
            assert int(L.l2s_wgrad_ws_bytes(C.byref(d), c['dt'])) == (sp * slab if sp > 1 else 0), (c['id'], split_k)
            seen.add((split_k > WU.slices(c, p)[0], sp))
        assert plan_split(c, p, p['split']) == WU.eff_split(c, p)
    assert any(clamped and 1 < sp < 64 for clamped, sp in seen)                        # a request clamped to the slice count
    # the cap of 64: more slices than that, and a request beyond it
    c = next(c for c in by(SINGLE, 0, F32) if c['id'].endswith('ring13'))
    p = dict(c['probs'][0], segs=[(1, 70, 16)], KH=1, KW=1, stride=1, pad=0)
    assert WU.slices(c, p)[0] == 70
    for split_k, want in ((100, 64), (64, 64), (65, 64), (63, 63), (0, plan_split(c, p, 0))):
        d = WU.single_desc(c, dict(p, split=split_k))
        assert int(L.l2s_wgrad_ws_bytes(C.byref(d), F32)) == want * p['Cout'] * p['Cin'] * 4, split_k
    assert 1 < plan_split(c, p, 0) <= 70 // 8


def grouped_status(c, variant=None, dt=None, nprob=None, ws=1 << 20, ws_bytes=1 << 40, edit=None):
    """the status of l2s_conv_wgrad_grouped on dummy pointers; only for calls the entry refuses before its first launch"""
    from lang2seg_amd import _lib
    arr = (_lib.WgradProb * max(len(c['probs']), nprob or 0))()
    offs, _ = WU.ws_layout(c)
    for q, p, off in zip(arr, c['probs'], offs):
        WU.fill_prob(q, c, p, ws_off=off)
    if edit:
        edit(arr[0])
    n = len(c['probs']) if nprob is None else nprob
    return int(lib().l2s_conv_wgrad_grouped(1 << 20, C.cast(arr, C.c_void_p), n, c['variant'] if variant is None else variant,
                                            c['dt'] if dt is None else dt, ws, ws_bytes, None))


def test_refusals():
    """every refusal below returns L2S_EINVAL before the entry's first HIP call (read in l2s_conv_wgrad, l2s_conv_wgrad_grouped, wgrad_row3_dma_launch
    and wgrad_1x1_dma_launch: prob_ok and the *_ok predicates run in the loops over the host table, ahead of hipFuncSetAttribute and the launch)"""
    L = lib()
    one = lambda v, dt, **kw: dict(entry=GROUPED, dt=dt, variant=v, probs=[WU.P(**kw)], tile=None)
    ok5 = dict(segs=[(1, 4, 4)], Cin=128, Cout=128, k=3)
    ok6 = dict(segs=[(1, 4, 4)], Cin=256, Cout=256, k=1)
    # the single entry: Cin % 8 in bf16, a pitch that is no multiple of the vector
    s = dict(entry=SINGLE, dt=BF16, variant=0, tile=64)
    assert int(L.l2s_conv_wgrad(C.byref(WU.single_desc(s, WU.P([(1, 4, 4)], 12, 16))), BF16, None)) == EINVAL
    assert int(L.l2s_conv_wgrad(C.byref(WU.single_desc(s, WU.P([(1, 4, 4)], 16, 12))), BF16, None)) == EINVAL
    for field, ld in (('lddy', 20), ('ldx', 36)):
        d = WU.single_desc(s, WU.P([(1, 4, 4)], 16, 16))
        setattr(d, field, ld)
        assert int(L.l2s_conv_wgrad(C.byref(d), BF16, None)) == EINVAL
    d = WU.single_desc(dict(s, dt=F32), WU.P([(1, 4, 4)], 16, 16))
    d.ldx = 18
    assert int(L.l2s_conv_wgrad(C.byref(d), F32, None)) == EINVAL
    # the grouped entry
    assert grouped_status(one(0, BF16, segs=[(1, 4, 4)], Cin=12, Cout=16)) == EINVAL
    assert grouped_status(one(0, BF16, segs=[(1, 4, 4)], Cin=16, Cout=16), edit=lambda q: setattr(q, 'nseg', 3)) == EINVAL
    assert grouped_status(one(0, BF16, segs=[(1, 4, 4)], Cin=16, Cout=16), edit=lambda q: q.lddy.__setitem__(0, 20)) == EINVAL
    assert grouped_status(one(2, BF16, segs=[(1, 4, 4)], Cin=16, Cout=16, k=1)) == EINVAL                        # a filter-row tile on a 1x1 problem
    assert grouped_status(one(3, F32, segs=[(1, 4, 4)], Cin=16, Cout=16, k=3, stride=2)) == EINVAL
    assert grouped_status(one(5, F32, **ok5)) == EINVAL and grouped_status(one(6, F32, **ok6)) == EINVAL
    assert grouped_status(one(5, BF16, **dict(ok5, Cin=192))) == EINVAL and grouped_status(one(5, BF16, **dict(ok5, Cout=64))) == EINVAL
    assert grouped_status(one(5, BF16, **ok5), edit=lambda q: setattr(q, 'split', 2)) == EINVAL
    assert grouped_status(one(5, BF16, **ok5), ws=None) == EINVAL and grouped_status(one(5, BF16, **ok5), ws_bytes=3 * 128 * 128 * 4) == EINVAL
    assert grouped_status(one(5, BF16, **dict(ok5, k=1))) == EINVAL
    assert grouped_status(one(6, BF16, **dict(ok6, stride=2, segs=[(1, 5, 5)]))) == EINVAL                        # OH != IH
    assert grouped_status(one(6, BF16, **dict(ok6, Cin=384))) == EINVAL and grouped_status(one(6, BF16, **ok6), edit=lambda q: setattr(q, 'split', 2)) == EINVAL
    sp = one(0, BF16, segs=[(1, 8, 8)], Cin=16, Cout=16, split=2)
    assert grouped_status(sp, ws_bytes=2 * 16 * 16 * 4 - 4) == EINVAL and grouped_status(sp, ws=None) == EINVAL      # slabs overrun the workspace
    assert grouped_status(sp, edit=lambda q: setattr(q, 'ws_off', 2)) == EINVAL
    assert grouped_status(one(0, BF16, segs=[(1, 4, 4)], Cin=16, Cout=16), nprob=65) == EINVAL
    assert grouped_status(one(0, BF16, segs=[(1, 4, 4)], Cin=16, Cout=16), nprob=0) == EINVAL
    assert grouped_status(one(0, BF16, segs=[(1, 4, 4)], Cin=16, Cout=16), variant=7) == EINVAL


# ------------------------------------------------------------------------------------------------------------------ the reference a second way
@pytest.mark.parametrize('c', WU.CASES, ids=lambda c: c['id'])
def test_reference_against_torch_f32(c):
    worst = 0.0
    for p, inp, (ref, ab, nt) in zip(c['probs'], WU.make(c), WU.refs(c)):
        worst = max(worst, check(WU.wgrad_f32(p, inp), ref, ab, nt, 'f32', what=c['id']))
    assert worst > 0.0


# ------------------------------------------------------------------------------------------------------------------ the bound sees structure
def _case(cid):
    return next(c for c in WU.CASES if c['id'] == cid)


def _mutated(c, pi, gather_=None, swap=False, drop_last=None, no_dw0=False):
    p, inp = c['probs'][pi], WU.make(c)[pi]
    z = np.zeros_like(f64(inp['dw0'])) if (p['ow'] or no_dw0) else f64(inp['dw0'])
    xs = inp['x'][::-1] if swap else inp['x']
    for s in range(len(p['segs'])):
        dy = f64(inp['dy'][s]).copy()
        if drop_last == s:
            dy.reshape(-1, p['Cout'])[-1] = 0
        z = z + WU.seg_term(p, s, xs[s], dy, gather_ or WU.gather)[0]
    return z


MUTATIONS = ['last_pixel_dropped', 'row_wrap', 'tap_shifted', 'segments_swapped', 'dw0_left_out', 'stride_without_pad', 'slab_left_out']


@pytest.mark.parametrize('mut', MUTATIONS)
def test_mutations_are_seen(mut):
    """the mutated result goes through the float32 store a device result would; the unmutated one passes"""
    if mut in ('last_pixel_dropped', 'segments_swapped'):
        # two segments of the same shape, so that swapping X is a shape-preserving mistake
        c = dict(entry=GROUPED, dt=BF16, variant=2, probs=[WU.P([(3, 5, 6), (3, 5, 6)], 40, 72, k=3)], id='mut-twoseg', tile=None)
    elif mut in ('row_wrap', 'tap_shifted', 'dw0_left_out'):
        c = _case('grouped-v2-bf16-auto')
    elif mut == 'stride_without_pad':
        c = dict(entry=GROUPED, dt=BF16, variant=0, probs=[WU.P([(2, 9, 11)], 40, 72, k=3, stride=2, pad=1)], id='mut-s2', tile=None)
    else:
        c = _case('single-v2-bf16-split3')
    p, inp = c['probs'][0], WU.make(c)[0]
    ref, ab = WU.wgrad_ref64(p, inp)
    nt = WU.n_terms(c, p)
    check(ref.astype(np.float32), ref, ab, nt, 'f32', what='unmutated')
    assert np.array_equal(_mutated(c, 0), ref)

    def shifted(dy_, dx_, only=None, wrap=False, nopad=False):
        def g(p_, s, x, ky, kx):
            n, H, W, OH, OW = WU.seg_geometry(p_, s)
            if only is not None and (ky, kx) != only and not nopad:
                return WU.gather(p_, s, x, ky, kx)
            out = np.zeros((n, OH, OW, p_['Cin']))
            xx = f64(x)
            for oy in range(OH):
                for ox in range(OW):
                    if nopad:
                        iy, ix = oy * p_['stride'] + ky - p_['pad'], ox * p_['stride'] + kx          # x * stride instead of x * stride - pad
                    else:
                        iy, ix = oy * p_['stride'] - p_['pad'] + ky + dy_, ox * p_['stride'] - p_['pad'] + kx + dx_
                    if wrap:
                        # kx = 0 at column 0: the previous pixel of the row-major walk (the previous row's last pixel) instead of zero
                        iy, ix = oy - p_['pad'] + ky, ox - 1
                        if ox == 0:
                            iy, ix = iy - 1, W - 1
                    if 0 <= iy < H and 0 <= ix < W:
                        out[:, oy, ox] = xx[:, iy, ix]
            return out.reshape(n * OH * OW, p_['Cin'])
        return g

    if mut == 'last_pixel_dropped':
        bad = _mutated(c, 0, drop_last=0)
    elif mut == 'row_wrap':
        bad = _mutated(c, 0, gather_=shifted(0, 0, only=(1, 0), wrap=True))
        assert np.array_equal(bad[:, 0], ref[:, 0]) and np.array_equal(bad[:, :, 1:], ref[:, :, 1:]) and not np.array_equal(bad[:, 1, 0], ref[:, 1, 0])
    elif mut == 'tap_shifted':
        bad = _mutated(c, 0, gather_=shifted(0, 1, only=(2, 2)))
    elif mut == 'segments_swapped':
        bad = _mutated(c, 0, swap=True)
    elif mut == 'dw0_left_out':
        bad = _mutated(c, 0, no_dw0=True)
    elif mut == 'stride_without_pad':
        bad = _mutated(c, 0, gather_=shifted(0, 0, nopad=True))
    else:
        # one of the three slabs (pixel ranges) of a split problem never added: the pixels of the middle range are missing
        sp, ns = WU.eff_split(c, p), WU.slices(c, p)[0]
        assert sp == 3
        n, H, W, OH, OW = WU.seg_geometry(p, 0)
        per = -(-ns // sp) * WU.slice_pixels(c['entry'], c['variant'], c['dt'])
        dy = f64(inp['dy'][0]).copy()
        virt = np.arange(n * OH * (OW + 1)).reshape(n, OH, OW + 1)[:, :, :OW]          # virtual pixel index of every real pixel
        dy[(virt >= per) & (virt < 2 * per)] = 0
        bad = f64(inp['dw0']) + WU.seg_term(p, 0, inp['x'][0], dy)[0]
    assert bad.shape == ref.shape
    with pytest.raises(AssertionError, match='times the bound'):
        check(bad.astype(np.float32), ref, ab, nt, 'f32', what=mut)
