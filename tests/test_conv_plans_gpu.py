"""Every plan of l2s_conv_igemm (conv_plan() in csrc/conv_igemm.hip) on the device, against the float64 reference of
tests/conv_plans_util.py through small_kernels_util.check, the elementwise bound

    |got - ref| <= (K + 2 [+ slabs of a forced split] + 2) * 2^-24 * (|x| * |w| + |bias| + |add|) + rho * |ref|,   rho = 2^-8 (bf16 store) or 0

(derived there; tests/test_conv_plans_cpu.py pins the table, the reference and the bound's sight of single misplaced terms without a GPU).
For every case, layout and form of the table (one test each, so a failure names its branch):
  - ops.LAST_PLAN is the plan the table names, and ops.last_kernel() is a kernel of that family (splitk_reduce_kernel behind a split);
  - x, y, add, ref and bias live inside larger buffers: y between GUARD rows of a sentinel and with pad columns (and, under the strided
    scatter, the pixels between the strides), which have to come back bit-identical; x with pad columns and guard rows of 1e30, add and bias
    with 1e30 and ref with -1e30 around them, so that a read past a row shows in the value;
  - the interior of y starts as NaN and has to come back finite and within the bound, every element of it;
  - a second launch into a fresh buffer gives the same bits, and so do xcd_mode 0 and 1 wherever the launch has more than 8 tiles;
  - the 196-row, 256x256 and persistent LDS-DMA tiles give the bits of the 256x128 LDS-DMA tile, the forced patch tile those of the
    automatic one.
The last test asserts that the plans launched are the planner's whole list but the stamped ones (it needs the whole file to have run).

Not run: igemm_dma_kernel<256,128,stamped> and the stamped igemm_ws64_kernel (instrumented builds for the tools, which write clock stamps
into `ws`), and the branches that need operands of 2 GiB or more.

Worst |got - ref| / bound per plan, measured on an MI355X (this file's own prints; a value next to 1 is a bf16 store, whose half unit in
the last place is the whole bound):
  plan                                        bf16 store   f32 / out_f32 store
  igemm_kernel<64,64>                         0.977        0.0767
  igemm_kernel<128,128>                       0.988        0.0887
  igemm_ring_kernel<64,64>                    0.994        0.0499
  igemm_ring_kernel<128,128>                  0.994        0.0321
  igemm_ring_kernel<128,64>                   0.994        -
  igemm_ws64_kernel                           0.983        -
  igemm_ws64_kernel + splitk_reduce_kernel    0.949        -
  igemm_sp_kernel<224,128>                    0.99         0.0317
  igemm_sp_kernel<256,128>                    0.987        0.0269
  igemm_ks64_kernel<4>                        0.983        -
  igemm_ks64_kernel<3>                        0.979        -
  igemm_p3_kernel<32,256>                     0.933        -
  igemm_p3_kernel<32,384>                     0.961        -
  igemm_p3_kernel<64,256>                     0.957        -
  igemm_p3_kernel<64,384>                     0.955        -
  igemm_dma_kernel<256,128>                   0.982        -
  igemm_dma196_kernel                         0.941        -
  igemm_dma256_kernel                         0.988        -
  igemm_pdma_kernel<256,128>                  0.969        -
  ("-": the plan has no such store.)  Every float store stays below 0.09 of the bound: no kernel needed a rounding added to n_terms.  Every
  sentinel, every second launch, every xcd_mode pair and every bit-for-bit pair: exact.  The file's 1479 tests (one per case, layout and form) take 16 s.
"""
import numpy as np
import pytest
import torch

import conv_plans_util as CU
from small_kernels_util import check, F32, BF16

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL = -7777.0
BIG = 1e30
LAUNCHED = set()
WORST = {}
ALL = [(c, lay, form) for c in CU.CASES for lay in c['lays'] for form in c['forms']]


def ops():
    from lang2seg_amd import ops as O
    return O


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def padded(a, ld, dtype, fill, guard=0, off=0):
    """[rows][cols] numpy -> (flat device buffer of off + (2 guard + rows) ld elements filled with `fill`, the view a kernel gets)"""
    rows, cols = a.shape
    flat = torch.full((off + (2 * guard + rows) * ld,), fill, dtype=dtype, device=DEV)
    start = off + guard * ld
    flat[start:start + rows * ld].view(rows, ld)[:, :cols] = torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)
    return flat, flat[start:]


class Out(object):
    """y: (2 GUARD + orows) rows of ldy elements of the sentinel; `rows` x ocols of it are what the launch writes and start as `interior`"""

    def __init__(self, g, rows, dtype, interior):
        self.g, self.dtype = g, dtype
        self.flat = torch.full(((2 * CU.GUARD + g['orows']) * g['ldy'],), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.flat[CU.GUARD * g['ldy']:]
        self.grid = self.view[:g['orows'] * g['ldy']].view(g['orows'], g['ldy'])
        self.rows = slice(None) if rows is None else torch.from_numpy(rows).to(DEV)
        self.written = torch.zeros(self.flat.numel(), dtype=torch.bool, device=DEV)
        w = self.written[CU.GUARD * g['ldy']:][:g['orows'] * g['ldy']].view(g['orows'], g['ldy'])
        w[self.rows, :g['ocols']] = True
        self.flat[self.written] = interior
        self.before = self.flat.clone()

    def got(self):
        return self.grid[self.rows, :self.g['ocols']].float().cpu().numpy()

    def assert_sentinels(self, what):
        same = bits(self.flat)[~self.written] == bits(self.before)[~self.written]
        if not bool(same.all()):
            first = int(torch.nonzero(~self.written).flatten()[torch.nonzero(~same).flatten()[0]]) - CU.GUARD * self.g['ldy']
            raise AssertionError('%s: %d sentinel elements of y changed, the first one at row %d, column %d (ldy %d, %d columns)' % (
                what, int((~same).sum()), first // self.g['ldy'], first % self.g['ldy'], self.g['ldy'], self.g['ocols']))


def family(c, form, plan):
    if c['split'] and not CU.FORMS[form]['shuffle']:
        return 'splitk_reduce_kernel'
    return plan.split(' ')[0].split('<')[0]


_DEVICE = {}             # operands of the (case, layout) of the latest test on the device: its forms follow one another


def operands(c, lay):
    key = (c['id'], lay)
    if key not in _DEVICE:
        _DEVICE.clear()
        inp = CU.make(c)
        tdt = torch.bfloat16 if c['dt'] == BF16 else torch.float32
        M, Kc = c['n'] * c['OH'] * c['OW'], c['KH'] * c['KW'] * c['Cin']
        xflat, xv = padded(inp['x'].reshape(-1, c['Cin']), CU.geometry(c, c['forms'][0], lay)['ldx'], tdt, BIG, guard=CU.GUARD)
        wflat, wv = padded(np.concatenate([inp['w'].reshape(c['Cout'], Kc), np.full((64, Kc), BIG, np.float32)]), Kc, tdt, BIG)
        ws = torch.full((c['split'] * M * c['Cout'],), float('nan'), device=DEV) if c['split'] else None
        _DEVICE[key] = dict(xflat=xflat, xv=xv, wflat=wflat, wv=wv, x0=xflat.clone(), w0=wflat.clone(), ws=ws, keep={})
    return _DEVICE[key]


@pytest.mark.parametrize('clf', ALL, ids=lambda clf: '%s-%s-%s' % (clf[0]['id'], clf[1], clf[2]))
def test_conv_plan(clf):
    O = ops()
    c, lay, form = clf
    inp = CU.make(c)
    tdt = torch.bfloat16 if c['dt'] == BF16 else torch.float32
    D = operands(c, lay)
    xv, wv, ws, keep = D['xv'], D['wv'], D['ws'], D['keep']
    f, g = CU.FORMS[form], CU.geometry(c, form, lay)
    what = '%s %s %s' % (c['id'], lay, form)
    plan = CU.expected_plan(c, form, lay)
    sh = f['shuffle']
    key = (sh, f['bias'], f['add'], f['ref'])
    if key not in keep:
        keep[key] = (padded(inp['bias'][None, :g['nbias']], g['nbias'] + 8, torch.float32, BIG, off=g['boff']) if f['bias'] else (None, None),
                     padded(inp['add', sh], g['ldadd'], tdt, BIG, guard=1, off=g['aoff']) if f['add'] else (None, None),
                     padded(inp['ref', sh], g['ldref'], tdt, -BIG, guard=1, off=g['aoff']) if f['ref'] else (None, None))
    (_, bias), (_, add), (_, refm) = keep[key]
    ydt = torch.float32 if CU.store_of(c, form) == 'f32' else torch.bfloat16
    rows = CU.shuffle_rows(c) if sh == 'scatter' else None

    def launch(interior, **kw):
        y = Out(g, rows, ydt, interior)
        if ws is not None:
            ws.fill_(float('nan'))
        O.conv_igemm(xv, wv, y.view, c['n'], c['H'], c['W'], c['Cin'], c['OH'], c['OW'], c['Cout'], c['KH'], c['KW'], c['stride'], c['pad'],
                     bias=bias, add=add, ref=refm, relu=bool(f['relu']), out_f32=bool(f['f32o']), deconv=sh == 'deconv',
                     scatter=(2 * c['H'], 2 * c['W'], 2) if sh == 'scatter' else None, ldx=g['ldx'], ldy=g['ldy'], ldadd=g['ldadd'], ldref=g['ldref'],
                     tile=c['tile'], dt=c['dt'], ws=ws, split_k=c['split'], xcd_mode=kw.get('xcd_mode', -1), algo=kw.get('algo', c['algo']))
        return y

    O.TRACK_PLAN = True
    try:
        y = launch(float('nan'))
        LAUNCHED.add(O.LAST_PLAN)
        assert O.LAST_PLAN == plan, (what, O.LAST_PLAN, plan)
        assert O.last_kernel().startswith(family(c, form, plan)), (what, O.last_kernel(), plan)
        ref, ab, nt = CU.conv_ref64(c, form)
        worst = check(y.got(), ref, ab, nt, CU.store_of(c, form), what=what)
        WORST[plan, CU.store_of(c, form)] = max(WORST.get((plan, CU.store_of(c, form)), 0.0), worst)
        y.assert_sentinels(what)
        y2 = launch(SENTINEL)
        assert torch.equal(bits(y2.flat)[y.written], bits(y.flat)[y.written]), '%s: a second launch gives other bits' % what
        y2.assert_sentinels(what + ' (second launch)')
        if CU.n_tiles64(c) > 8:
            for mode in (0, 1):
                ym = launch(SENTINEL, xcd_mode=mode)
                assert O.LAST_PLAN == plan
                assert torch.equal(bits(ym.flat), bits(y2.flat)), '%s: xcd_mode %d gives other bits' % (what, mode)
        other = CU.ALGO_DMA if plan in (CU.DMA196, CU.DMA256, CU.PDMA) else CU.ALGO_PATCH if plan in CU.P3 else None
        if other is not None:
            yo = launch(SENTINEL, algo=other)
            assert O.LAST_PLAN == (CU.DMA if other == CU.ALGO_DMA else plan), (what, O.LAST_PLAN)
            LAUNCHED.add(O.LAST_PLAN)
            assert torch.equal(bits(yo.flat), bits(y2.flat)), '%s: not the bits of %s' % (what, O.LAST_PLAN)
        print('%s -> %s: worst ratio %.3g' % (what, plan, worst))
    finally:
        O.TRACK_PLAN = False
    assert torch.equal(bits(D['xflat']), bits(D['x0'])) and torch.equal(bits(D['wflat']), bits(D['w0'])), '%s: an input changed' % what


def test_every_plan_was_launched():
    want = set(CU.ALL_PLANS) - set(CU.STAMPED)
    for p in sorted(want):
        print('worst ratio %-45s bf16 store %-8s float store %s' % (p, '%.3g' % WORST[p, 'bf16'] if (p, 'bf16') in WORST else '-', '%.3g' % WORST[p, 'f32'] if (p, 'f32') in WORST else '-'))
    assert LAUNCHED == want, LAUNCHED ^ want
