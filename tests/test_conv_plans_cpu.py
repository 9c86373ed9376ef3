"""tests/conv_plans_util.py without a GPU: every case, form and layout of the table lands on the plan it names (l2s_conv_plan_name launches
nothing), the table reaches every plan of the planner but the two stamped ones, the float64 reference and its bound hold for a plain
float32 convolution of torch on the CPU (whose shuffled layouts come from conv_transpose2d, i.e. are written a second way), and the bound
sees structure: five mutations of the reference, each a single misplaced term, row or column, make `check` raise.

Not covered here or on the device: igemm_dma_kernel<256,128,stamped> and the stamped igemm_ws64_kernel (instrumented builds for the tools;
they write clock stamps into `ws`), and the branches that need operands of 2 GiB or more."""
import numpy as np
import pytest
import torch

import conv_plans_util as CU
from small_kernels_util import check, f64, stored_as, U24, F32, BF16


def ids(cl):
    return '%s-%s' % (cl[0]['id'], cl[1]) if isinstance(cl, tuple) else cl['id']


ALL = [cl for c in CU.CASES for cl in CU.case_lays(c)]


def test_table_conditions():
    for c in CU.CASES:
        K = c['KH'] * c['KW'] * c['Cin']
        assert K * (K + 4) * U24 < 0.25, c['id']
        for form in c['forms']:
            f = CU.FORMS[form]
            assert not f['shuffle'] or (c['KH'] == c['KW'] == c['stride'] == 1 and c['pad'] == 0), c['id']
            assert f['shuffle'] != 'deconv' or c['Cout'] % 16 == 0, c['id']
        for lay in c['lays']:
            g = CU.geometry(c, c['forms'][0], lay)
            assert g['ldx'] > c['Cin'] and g['ldx'] % (8 if c['dt'] == BF16 else 4) == 0


@pytest.mark.parametrize('cl', ALL, ids=ids)
def test_plan_of_every_case(cl):
    c, lay = cl
    for form in c['forms']:
        assert CU.plan_name(c, form, lay) == CU.expected_plan(c, form, lay), (c['id'], form, lay)


def test_table_reaches_every_plan():
    """the case's own plan is reached by at least one of its forms and layouts, and the plans reached are the planner's list without the stamped ones"""
    reached = set()
    for c in CU.CASES:
        own = {CU.plan_name(c, form, lay) for form in c['forms'] for lay in c['lays']}
        assert c['plan'] in own, (c['id'], own)
        reached |= own
    assert reached == set(CU.ALL_PLANS) - set(CU.STAMPED), reached ^ (set(CU.ALL_PLANS) - set(CU.STAMPED))
    # the list itself is the planner's: PLAN_NAMES of the source, name for name, and as many entries as the ConvPlan enumeration has
    names = CU.planner_names()
    assert names[0] == 'invalid' and sorted(names[1:]) == sorted(CU.ALL_PLANS) and len(set(names)) == len(names), set(names[1:]) ^ set(CU.ALL_PLANS)
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lang2seg_amd', 'csrc', 'conv_igemm.hip')).read()
    enum = re.search(r'enum ConvPlan \{(.*?)\};', src, re.S).group(1)
    assert len(re.findall(r'PLAN_\w+', enum)) == len(names)


def test_dense_and_other_branch_per_plan():
    """each plan has a case on densely pitched, aligned operands (the LDS-staged or vector epilogue) and one on the other branch: Cout % 8,
    Cout % 4, an odd pitch, or a form whose bias / add / ref view starts 4 bytes into its buffer.  The 196-row tile has no other branch to
    reach: the planner admits nothing but what its staged epilogue takes (d196_ok in conv_plan() calls igemm_plain(), the predicate the kernels call), so every layout
    that would break it has to land on the fallback instead"""
    dense, other = set(), set()
    for c in CU.CASES:
        for lay in c['lays']:
            for form in c['forms']:
                f, p = CU.FORMS[form], CU.expected_plan(c, form, lay)
                if lay == 'dense' and c['Cout'] % 8 == 0:
                    dense.add(p)
                if lay == 'odd' or c['Cout'] % 8 or (lay == 'off' and (f['bias'] or f['add'] or f['ref'])):
                    other.add(p)
                if c['plan'] == CU.DMA196 and (lay == 'odd' or (lay == 'off' and (f['bias'] or f['add'] or f['ref']))):
                    assert p != CU.DMA196, (c['id'], form, lay)
    want = set(CU.ALL_PLANS) - set(CU.STAMPED)
    assert other == want - {CU.DMA196}, (want - {CU.DMA196}) ^ other
    assert dense == want, want - dense


def test_every_instantiation_of_the_float_and_tap_switches():
    """l2s_conv_igemm instantiates the ring, generic and software-pipelined kernels per operand type and store, the software-pipelined ones
    per tap order as well (taps innermost for filters of more than one tap): each combination the planner can reach has a case"""
    seen = set()
    for c in CU.CASES:
        for form in c['forms']:
            for lay in c['lays']:
                p = CU.expected_plan(c, form, lay)
                seen.add((p, c['dt'], CU.store_of(c, form), c['KH'] * c['KW'] > 1))
    for p in (CU.SP224, CU.SP256):
        for taps in (False, True):
            assert (p, F32, 'f32', taps) in seen, (p, taps)
            assert (p, BF16, 'f32', taps) in seen, (p, taps)
        assert (p, BF16, 'bf16', False) in seen, p          # (a bf16 store with taps goes to the LDS-DMA tile)
    for p in (CU.GENERIC64, CU.GENERIC128, CU.RING64, CU.RING128):
        for dt, st in ((F32, 'f32'), (BF16, 'bf16'), (BF16, 'f32')):
            assert any(k[:3] == (p, dt, st) for k in seen), (p, dt, st)


@pytest.mark.parametrize('c', CU.CASES, ids=ids)
def test_reference_against_torch_f32(c):
    worst = 0.0
    for form in c['forms']:
        ref, ab, nt = CU.conv_ref64(c, form)
        worst = max(worst, check(CU.conv_f32(c, form), ref, ab, nt, CU.store_of(c, form), what='%s %s' % (c['id'], form)))
    assert worst > 0.0


def test_scatter_rows_written_a_second_way():
    c = next(c for c in CU.CASES if 'scatter' in c['forms'] and c['n'] > 1)
    rows = CU.shuffle_rows(c)
    m = 0
    for img in range(c['n']):
        for oy in range(c['OH']):
            for ox in range(c['OW']):
                assert rows[m] == img * (2 * c['H']) * (2 * c['W']) + (2 * oy) * (2 * c['W']) + 2 * ox
                m += 1
    c = next(c for c in CU.CASES if 'deconv' in c['forms'] and c['n'] > 1)
    Cq = c['Cout'] // 4
    a = np.arange(c['n'] * c['OH'] * c['OW'] * c['Cout'], dtype=np.float64).reshape(-1, c['Cout'])
    out = CU.pixel_shuffle(c, a)
    for m in (0, 7, c['OH'] * c['OW'] + 3, a.shape[0] - 1):
        img, rem = divmod(m, c['OH'] * c['OW'])
        oy, ox = divmod(rem, c['OW'])
        for col in (0, Cq - 1, Cq, 2 * Cq + 1, 4 * Cq - 1):
            tap, co = divmod(col, Cq)
            assert out[(img * 2 * c['OH'] + 2 * oy + (tap >> 1)) * (2 * c['OW']) + 2 * ox + (tap & 1), co] == a[m, col]


# ------------------------------------------------------------------------------------------------------------------ the bound sees structure
def _find(plan, k, shuffle=False):
    return next(c for c in CU.CASES if c['plan'] == plan and c['KH'] == k and ('deconv' in c['forms']) == shuffle and not c['big'])


MUT_CASES = [(_find(CU.WS64, 1), ''), (_find(CU.RING128, 3), ''), (_find(CU.WS64, 1, True), 'deconv')]
MUTATIONS = ['channel_dropped', 'bias_shifted', 'mask_skipped', 'row_lower', 'last_tap_pad']


@pytest.mark.parametrize('mut', MUTATIONS)
@pytest.mark.parametrize('cs', MUT_CASES, ids=lambda cs: cs[0]['id'] + cs[1])
def test_mutations_are_seen(cs, mut):
    """the mutated result goes through the same float32 rounding and store as a device result would; the unmutated one passes"""
    c, sh = cs
    inp = CU.make(c)
    form = ('deconv_ref' if mut == 'mask_skipped' else 'deconv') if sh else {'mask_skipped': 'dgrad', 'bias_shifted': 'bias'}.get(mut, 'fwd')
    store = CU.store_of(c, form)
    ref, ab, nt = CU.conv_ref64(c, form)
    good = stored_as(torch.from_numpy(ref.astype(np.float32)), BF16 if store == 'bf16' else F32)
    check(good, ref, ab, nt, store, what='unmutated')
    if mut == 'channel_dropped':
        # one product x[m][k] w[n][k] left out of one output that the ReLU keeps
        P, A = CU.product64(c)
        M = P.shape[0]
        xm, wk = f64(inp['x']).reshape(M, -1), f64(inp['w'])[:, c['KH'] // 2, c['KW'] // 2, :]       # the centre tap of pixel m is x[m] itself
        pre = P + (np.tile(f64(inp['bias'])[:c['Cout'] // 4], 4) if sh else f64(inp['bias']) + f64(inp['add', None]))
        m, n = np.unravel_index(int(np.argmax(pre)), pre.shape)
        k = int(np.argmax(np.abs(xm[m] * wk[n])))
        P2 = P.copy()
        P2[m, n] -= xm[m, k] * wk[n, k]
        bad, _, _ = CU.conv_ref64(c, form, prod=(P2, A))
        assert (bad != ref).sum() == 1
    elif mut == 'bias_shifted':
        inp2 = dict(inp); inp2['bias'] = np.roll(inp['bias'], 1)
        bad, _, _ = CU.conv_ref64(c, form, inp=inp2)
    elif mut == 'mask_skipped':
        key = ('ref', 'deconv' if sh else None)
        unmasked = CU.conv_ref64(c, form, inp={**inp, key: np.ones_like(inp[key])})[0]
        gone = np.argwhere((ref == 0) & (np.abs(unmasked) > 0.1))[0]
        bad = ref.copy(); bad[tuple(gone)] = unmasked[tuple(gone)]
    elif mut == 'row_lower':
        bad = ref.copy(); r = ref.shape[0] // 2
        bad[r + 1] = ref[r]
    else:
        bad, _, _ = CU.conv_ref64(c, form, prod=CU.product64(c, last_tap_pad=1))
    bad = stored_as(torch.from_numpy(np.asarray(bad, np.float32)), BF16 if store == 'bf16' else F32)
    with pytest.raises(AssertionError, match='times the bound'):
        check(bad, ref, ab, nt, store, what=mut)
