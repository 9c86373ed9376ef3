"""Every weight-gradient kernel of the product library (l2s_conv_wgrad and l2s_conv_wgrad_grouped: csrc/conv_wgrad.hip, conv_wgrad_dma.hip,
conv_wgrad_dma1.hip) on the device, against the float64 reference of tests/wgrad_util.py through small_kernels_util.check, the elementwise
bound

    |got - ref| <= (M_total + 1 [+ split | + the 64-pixel slices under variant 5] + 2) * 2^-24 * (|dW0| + |dY|^T |X|)

(derived there; tests/test_wgrad_cpu.py pins the table, the host functions, the reference and the bound's sight of single misplaced terms
without a GPU).  For every case of the table (one test each, so a failure names its launch):
  - ops.last_kernel() is the kernel the case names (the reduce kernel behind a split or a stream-K launch);
  - dY and X of every segment live inside larger buffers whose pad columns and guard rows, in front of and behind the segment, hold 1e30, so
    that a read past a row or a segment shows in the value; they have to come back bit-identical;
  - dW sits between guard rows of a sentinel, which have to come back bit-identical;
  - accumulate problems start dW from random values (the reference includes them), overwrite problems (flags = 1) from NaN; every element
    of dW has to be finite and within the bound;
  - a second launch into a fresh buffer gives the same bits, for split problems too;
  - an unsplit variant 6 launch gives the bits of variant 4 on the same problems (conv_wgrad_dma1.hip: every accumulator sums its pixels
    in the order of the register-staged tile), and the grouped f32 entry those of the single f32 entry on the same unsplit problem (the two
    share the 16-pixel slice and the order of the MFMAs inside it; only the ring depth differs, which moves loads, not sums).
The last test asserts that the kernels launched are the product library's whole list (it needs the whole file to have run).

Not run: the tools-build knobs (wgrad_grid_cap, row3_form, row3_plan_mode: 0 in the product library) and operands of 2 GiB or more.

Worst |got - ref| / bound per kernel, measured on an MI355X (this file's own prints; "split": the launches whose pixels were split, i.e. the
slabs went through wgrad_reduce_kernel / wgrad_reduce_grouped_kernel; the stream-K launch of variant 5 always ends in wgrad_row3_reduce_kernel):
  kernel                              bf16 unsplit   bf16 split   f32 unsplit   f32 split
  wgrad_kernel          variant 0     0.106          0.00564      0.212         0.0214
  wgrad_kernel          variant 1     0.154          0.00748      0.24          0.0219
  wgrad_kernel          variant 2     0.13           0.00834      0.26          0.028
  wgrad_kernel          variant 3     0.152          0.00988      0.265         0.0284
  wgrad_grouped_kernel  variant 0     0.248          0.0054       0.322         0.0409
  wgrad_grouped_kernel  variant 1     0.266          0.00335      0.256         0.03
  wgrad_grouped_kernel  variant 2     0.286          0.00878      0.238         0.0437
  wgrad_grouped_kernel  variant 3     0.249          0.00739      0.243         0.0372
  wgrad_grouped_kernel  variant 4     0.25           0.00896      -             -
  wgrad_row3_dma_kernel variant 5     0.283          -            -             -
  wgrad_1x1_dma_kernel  variant 6     0.362          -            -             -
  The largest values belong to the problems of a few pixels (the launches of 64 problems of 1 to 3 pixels, the 3x3 images of one slice), where
  one rounding is a large part of so small a bound; the single launches of 100 pixels and more stay below 0.06.  No kernel needed a rounding
  added to n_terms.  Every sentinel, every input, every second launch and both kinds of bit-for-bit pair (variant 6 = variant 4; grouped f32
  = single f32): exact.  The file's 166 tests take 4 s.
"""
import ctypes as C

import pytest
import torch

import wgrad_util as WU
from wgrad_util import SINGLE
from small_kernels_util import check, BF16
from test_conv_plans_gpu import padded, bits

pytestmark = pytest.mark.gpu

DEV = 'cuda'
SENTINEL = -7777.0
BIG = 1e30
LAUNCHED = set()
WORST = {}
_WS5 = {}


def ops():
    from lang2seg_amd import ops as O
    return O


class Operands(object):
    """dY, X (per segment, pitched, between guard rows of 1e30) and what dW starts from, of every problem of a case"""

    def __init__(self, c):
        self.c = c
        tdt = torch.bfloat16 if c['dt'] == BF16 else torch.float32
        self.flat, self.dy, self.x, self.dw0 = [], [], [], []
        for p, inp in zip(c['probs'], WU.make(c)):
            dys, xs = [], []
            for s in range(len(p['segs'])):
                lddy, ldx = WU.pitches(c, p, s)
                f, v = padded(inp['dy'][s].reshape(-1, p['Cout']), lddy, tdt, BIG, guard=WU.GUARD)
                self.flat.append(f); dys.append(v)
                f, v = padded(inp['x'][s].reshape(-1, p['Cin']), ldx, tdt, BIG, guard=WU.GUARD)
                self.flat.append(f); xs.append(v)
            self.dy.append(dys); self.x.append(xs)
            self.dw0.append(torch.from_numpy(inp['dw0'].reshape(p['Cout'], -1)).to(DEV))
        self.before = [f.clone() for f in self.flat]

    def assert_unchanged(self, what):
        for f, b in zip(self.flat, self.before):
            assert torch.equal(bits(f), bits(b)), '%s: an input changed' % what


class Out(object):
    """dW of every problem: [Cout][KH KW Cin] floats between GUARD rows of a sentinel; the interior starts from dW0 (accumulate) or NaN (overwrite)"""

    def __init__(self, c, D):
        self.flat, self.view, self.before = [], [], []
        for p, dw0 in zip(c['probs'], D.dw0):
            K = p['KH'] * p['KW'] * p['Cin']
            f = torch.full(((2 * WU.GUARD + p['Cout']) * K,), SENTINEL, dtype=torch.float32, device=DEV)
            v = f[WU.GUARD * K:(WU.GUARD + p['Cout']) * K].view(p['Cout'], K)
            if p['ow']:
                v.fill_(float('nan'))
            else:
                v.copy_(dw0)
            self.flat.append(f); self.view.append(v); self.before.append(f.clone())

    def assert_sentinels(self, c, what):
        for i, (p, f, b) in enumerate(zip(c['probs'], self.flat, self.before)):
            g = WU.GUARD * p['KH'] * p['KW'] * p['Cin']
            assert torch.equal(bits(f[:g]), bits(b[:g])) and torch.equal(bits(f[-g:]), bits(b[-g:])), '%s: problem %d wrote outside dW' % (what, i)


def launch(c, D, variant=None):
    """one launch of case c (grouped: of `variant` if given) into a fresh Out; the workspace starts as NaN"""
    O = ops()
    from lang2seg_amd import _lib
    out = Out(c, D)
    if c['entry'] == SINGLE:
        p = c['probs'][0]
        n, H, W, OH, OW = WU.seg_geometry(p, 0)
        lddy, ldx = WU.pitches(c, p, 0)
        nb = O.wgrad_ws_bytes(n, H, W, p['Cin'], OH, OW, p['Cout'], p['KH'], p['KW'], p['stride'], p['pad'], dt=c['dt'], split_k=p['split'], tile=c['tile'])
        assert nb == (WU.eff_split(c, p) * out.view[0].numel() * 4 if WU.eff_split(c, p) > 1 else 0)
        ws = torch.full((nb // 4,), float('nan'), device=DEV) if nb else None
        O.conv_wgrad(D.dy[0][0], D.x[0][0], out.view[0], n, H, W, p['Cin'], OH, OW, p['Cout'], p['KH'], p['KW'], p['stride'], p['pad'],
                     lddy=lddy, ldx=ldx, split_k=p['split'], tile=c['tile'], ws=ws)
    else:
        v = c['variant'] if variant is None else variant
        arr = (_lib.WgradProb * len(c['probs']))()
        offs, total = WU.ws_layout(c)
        for i, (q, p) in enumerate(zip(arr, c['probs'])):
            WU.fill_prob(q, c, p, ptrs=dict(dy=[t.data_ptr() for t in D.dy[i]], x=[t.data_ptr() for t in D.x[i]], dw=out.view[i].data_ptr()), ws_off=offs[i])
        tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
        if v == 5:
            if 'ws' not in _WS5:
                _WS5['ws'] = torch.empty(int(_lib.load().l2s_wgrad_grouped_ws_bytes(5)) // 4, dtype=torch.float32, device=DEV)
            ws = _WS5['ws']
            ws.fill_(float('nan'))
        else:
            ws = torch.full((max(total, 4),), float('nan'), device=DEV)
        O.call('l2s_conv_wgrad_grouped', tab.data_ptr(), C.cast(arr, C.c_void_p), len(c['probs']), v, c['dt'], ws.data_ptr(), ws.numel() * 4, O.stream())
    torch.cuda.synchronize()
    return out


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a.flat, b.flat))


@pytest.mark.parametrize('c', WU.CASES, ids=lambda c: c['id'])
def test_wgrad(c):
    O = ops()
    what = c['id']
    D = Operands(c)
    out = launch(c, D)
    last = O.last_kernel()
    fam = WU.last_kernel_family(c)
    assert last == fam or last.startswith(fam + '<'), (what, last)
    LAUNCHED.add(WU.main_kernel(c))
    if fam != WU.main_kernel(c)[0]:
        LAUNCHED.add(fam)
    worst = 0.0
    for i, (p, (ref, ab, nt)) in enumerate(zip(c['probs'], WU.refs(c))):
        worst = max(worst, check(out.view[i].cpu().numpy().reshape(ref.shape), ref, ab, nt, 'f32', what='%s problem %d' % (what, i)))
    key = (WU.main_kernel(c), any(WU.eff_split(c, p) > 1 for p in c['probs']))
    WORST[key] = max(WORST.get(key, 0.0), worst)
    out.assert_sentinels(c, what)
    out2 = launch(c, D)
    assert same_bits(out, out2), '%s: a second launch gives other bits' % what
    out2.assert_sentinels(c, what + ' (second launch)')
    if c['pair'] == 4:
        o4 = launch(c, D, variant=4)
        assert O.last_kernel().startswith('wgrad_grouped_kernel<'), O.last_kernel()
        LAUNCHED.add(('wgrad_grouped_kernel', 4, BF16))
        for i, (p, (ref, ab, nt)) in enumerate(zip(c['probs'], WU.refs(c))):
            w4 = check(o4.view[i].cpu().numpy().reshape(ref.shape), ref, ab, nt, 'f32', what='%s problem %d on variant 4' % (what, i))
            WORST[('wgrad_grouped_kernel', 4, BF16), False] = max(WORST.get((('wgrad_grouped_kernel', 4, BF16), False), 0.0), w4)
        assert same_bits(out, o4), '%s: not the bits of variant 4' % what
    elif c['pair'] == 'single':
        cs = dict(c, entry=SINGLE, tile=WU.SINGLE_TILE_REQUEST[c['variant']])
        os_ = launch(cs, D)
        assert O.last_kernel().startswith('wgrad_kernel<'), O.last_kernel()
        assert same_bits(out, os_), '%s: not the bits of the single entry' % what
    D.assert_unchanged(what)
    print('%s -> %s: worst ratio %.3g' % (what, last, worst))


def test_every_kernel_was_launched():
    name = lambda k: k if isinstance(k, str) else '%s variant %d %s' % (k[0], k[1], WU.DTN[k[2]])
    for (k, split), w in sorted(WORST.items(), key=lambda kv: (name(kv[0][0]), kv[0][1])):
        print('worst ratio %-45s %-8s %.3g' % (name(k), 'split' if split else 'unsplit', w))
    assert LAUNCHED == WU.ALL_KERNELS, LAUNCHED ^ WU.ALL_KERNELS
