"""The per-token recurrence and attention kernels (csrc/caption_step.hip, csrc/rnn_step.hip, csrc/adaatt_step.hip) and the resident recurrence
(csrc/cap_recur.hip, token by token): their case tables, float64 restatements and float32 forms, under the rules and the ONE comparison (`check`) of tests/small_kernels_util.py.

Every operation is stated once, as a `*_core(A, inp)` function over an arithmetic A, and run twice:

  A64  values are `V`s: a float64 value with the bookkeeping of the bound, (v, ab, nt, mag).  `ab` is the same expression on magnitudes,
       `nt` the longest chain of float32 roundings, `mag` what the libm allowance multiplies.  The rules, all first order:
         an input             ab = |v|, nt = 0, exact
         a + b, a - b         ab = ab_a + ab_b, nt = max(nt_a, nt_b) + 1, mag = mag_a + mag_b
         a * b                ab = ab_a ab_b, nt = nt_a + nt_b + 1, mag = mag_a |b| + |a| mag_b
         a / b                ab = ab_a ab_b / b^2, nt = nt_a + nt_b + 1, mag = mag_a / |b| + |a| mag_b / b^2
                              (two exact operands: the result carries only its own rounding, ab = |v|, nt = 1 - so 1 - g of a saved gate g
                              next to 1 does not inherit an error g never had)
         sum / dot over n     ab = the sum / dot of the ab's, nt = nt + n
         tanhf(a) = t         a rounded ARGUMENT: its absolute error nt_a u ab_a moves t by (1 - t^2) times it, so ab = (1 - t^2) ab_a + |t|
                              (ab_a dropped for an exact a), mag = (1 - t^2) mag_a + |t|, nt = nt_a
         expf(a) = e          the argument's absolute error is e's relative error: ab = e ab_a + e, mag = e mag_a + SOFTMAX_L e, nt = nt_a
                              (the only expf here is the softmax's: its weights take SOFTMAX_L times the allowance of tanhf and the sigmoid,
                              by the measurement of tests/test_recur_kernels_gpu.py)
         sigm(a) = s          1 / (1 + expf(-a)): ds / da = s (1 - s); ab = s (1 - s) ab_a + s, mag = s (1 - s) mag_a + s, nt = nt_a + 2 (the
                              add and the divide)
         max(t0, t1)          the operand the float64 selector picks (`make` draws no pair whose float32 selector could differ)
       `*_ref(inp)` returns a dict of small_kernels_util.out(...) entries, the arguments of `check_out`.
  AE   the same cores with the first-order error itself in place of (ab, nt): see class VE.  Only the resident recurrence uses it.
  A32  plain torch-CPU float32 tensors: `*_f32(inp)` returns a dict of float32 arrays; tests/test_recur_kernels_cpu.py runs them through
       `check` with the libm allowance L = 1.

Two kinds of output do not take the rules as they stand, and say so where they are computed (A.rebound):
  softmax backward     ddot[l] = w[l] (dw[l] - sum_l w dw) cancels; its ab is w[l] (|dw[l]| + sum_l w |dw|), which the rules give as they are.
                       What follows it is bounded by hand.  Uncentred (att_h_grad): |aw[d]| sum_l (absdd[l] (1 - t^2) + |dd[l]| t^2) - the error
                       of ddot times the factor it meets, and the rounding of t^2 on the true ddot.  Centred (topdown_att_bwd_step_kernel):
                       |aw[d]| sum_l (absdd[l] |t^2 - m| + |dd[l]| (t^2 + m)) - an error e w[l] common to every ddot[l] meets sum_l w (t^2 - m) = 0,
                       what remains is each ddot's own error on |t^2 - m| and the rounding of t^2 and of m on the true ddot.  It is NOT widened
                       to the uncentred sum_l absdd[l]: the nearly-constant-tanh case would then stop seeing the property.
  max-out selectors    save[3] is an exact 0 / 1: ab = 0.  Each gate table plants exact ties (t0 == t1: the two transforms of the unit are
                       given the same operands, so both sums take the same roundings) and pairs one float32 step apart in both directions
                       (a0 = a1 = 0 exactly, s4 = nextafter(s3)): there the float32 sums are exact and the selector is decided.  Every other
                       unit whose |t0 - t1| is within the two forward bounds, libm share included, is redrawn (`dropped` counts them)."""
import numpy as np
import torch

from small_kernels_util import U24, rnd, f64, out


SOFTMAX_L = 2.0         # the libm allowance of a softmax weight over that of a tanhf / sigmoid value (measured on the device: the GPU file's docstring)


# ------------------------------------------------------------------------------------------------------------------ the two arithmetics
class V(object):
    __slots__ = ('v', 'ab', 'nt', 'mag', 'exact')

    def __init__(self, v, ab=None, nt=0, mag=None, exact=None):
        self.v = f64(v)
        self.ab = np.abs(self.v) if ab is None else f64(ab) + 0 * self.v
        self.nt = nt
        self.mag = np.zeros(self.v.shape) if mag is None else f64(mag) + 0 * self.v
        self.exact = (ab is None and mag is None and nt == 0) if exact is None else exact

    @staticmethod
    def of(o):
        return o if isinstance(o, V) else V(o)

    def __getitem__(self, i):
        return V(self.v[i], self.ab[i], self.nt, self.mag[i], self.exact)

    def __neg__(self):
        return V(-self.v, self.ab, self.nt, self.mag, self.exact)

    def _addsub(self, o, sign):
        o = V.of(o)
        v = self.v + sign * o.v
        if self.exact and o.exact:
            return V(v, np.abs(v), 1, exact=False)
        return V(v, self.ab + o.ab, max(self.nt, o.nt) + 1, self.mag + o.mag, False)

    def __add__(self, o):
        return self._addsub(o, 1.0)

    __radd__ = __add__

    def __sub__(self, o):
        return self._addsub(o, -1.0)

    def __rsub__(self, o):
        return V.of(o)._addsub(self, -1.0)

    def __mul__(self, o):
        o = V.of(o)
        v = self.v * o.v
        if self.exact and o.exact:
            return V(v, np.abs(v), 1, exact=False)
        return V(v, self.ab * o.ab, self.nt + o.nt + 1, self.mag * np.abs(o.v) + np.abs(self.v) * o.mag, False)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        return V(self.v / o.v, self.ab * o.ab / o.v ** 2, self.nt + o.nt + 1, self.mag / np.abs(o.v) + np.abs(self.v) * o.mag / o.v ** 2, False)


class A64(object):
    name = 'f64'

    @staticmethod
    def inp(x):
        return None if x is None else V(x)

    @staticmethod
    def raw(x):
        return x.v

    @staticmethod
    def tanh(a):
        t = np.tanh(a.v)
        return V(t, (0.0 if a.exact else (1 - t * t) * a.ab) + np.abs(t), a.nt, (1 - t * t) * a.mag + np.abs(t), False)

    @staticmethod
    def exp(a):
        e = np.exp(a.v)
        return V(e, (0.0 if a.exact else e * a.ab) + e, a.nt, e * a.mag + SOFTMAX_L * e, False)

    @staticmethod
    def sigm(a):
        s = 1.0 / (1.0 + np.exp(-a.v))
        return V(s, (0.0 if a.exact else s * (1 - s) * a.ab) + s, a.nt + 2, s * (1 - s) * a.mag + s, False)

    @staticmethod
    def sum(a, axis):
        return V(a.v.sum(axis), a.ab.sum(axis), a.nt + a.v.shape[axis], a.mag.sum(axis), False)

    @staticmethod
    def dot(w, x):
        """w [N][K] . x [K]"""
        return V(w.v @ x.v, w.ab @ x.ab, w.nt + x.nt + w.v.shape[1], np.abs(w.v) @ x.mag + w.mag @ np.abs(x.v), False)

    @staticmethod
    def where(cond, a, b):
        a, b = V.of(a), V.of(b)
        return V(np.where(cond, a.v, b.v), np.where(cond, a.ab, b.ab), max(a.nt, b.nt), np.where(cond, a.mag, b.mag), False)

    @staticmethod
    def stack(xs):
        xs = [V.of(x) for x in xs]
        return V(np.stack([x.v for x in xs]), np.stack([x.ab for x in xs]), max(x.nt for x in xs), np.stack([x.mag for x in xs]), False)

    @staticmethod
    def cat(xs):
        return V(np.concatenate([x.v for x in xs]), np.concatenate([x.ab for x in xs]), max(x.nt for x in xs), np.concatenate([x.mag for x in xs]), False)

    @staticmethod
    def reshape(a, shape):
        return V(a.v.reshape(shape), a.ab.reshape(shape), a.nt, a.mag.reshape(shape), a.exact)

    @staticmethod
    def amax(a):
        return V(a.v.max())

    @staticmethod
    def zeros(shape):
        return V(np.zeros(shape))

    @staticmethod
    def rebound(a, ab, nt):
        """the hand-written bound of an output the rules would bound too widely (docstring): ab and nt are functions of raw float64 arrays"""
        return V(a.v, ab, nt, a.mag, False)


class VE(V):
    """a V whose `ab` is the first-order absolute error itself, in units of u = 2^-24 (nt = 1: `check` then allows three times it).  The
    magnitude rules above multiply the ab's of a product and a quotient, which is the standard bound where the operands are inputs; behind a
    GEMV, a tanhf and a softmax in ONE launch (the resident recurrence) the ab's are tens of times the values and their product squares that.
    Here every operation adds what its operands' errors become and its own rounding |v|:
         a + b   e_a + e_b + |v|         a * b   e_a |b| + |a| e_b + |v|         a / b   e_a / |b| + |a| e_b / b^2 + |v|
         sum / dot over n    the operands' errors carried through, + n times the sum of magnitudes
         tanhf   (1 - t^2) e_a + |t|     expf   e e_a + e     sigm   s (1 - s) e_a + 2 s        (mag as above)"""
    __slots__ = ()

    @staticmethod
    def e(x):
        return 0.0 if x.exact else x.ab

    def __getitem__(self, i):
        return VE(self.v[i], self.ab[i], self.nt, self.mag[i], self.exact)

    def __neg__(self):
        return VE(-self.v, self.ab, self.nt, self.mag, self.exact)

    def _addsub(self, o, sign):
        o = V.of(o)
        v = self.v + sign * o.v
        return VE(v, VE.e(self) + VE.e(o) + np.abs(v), 1, self.mag + o.mag, False)

    def __rsub__(self, o):
        o = V.of(o)
        v = o.v - self.v
        return VE(v, VE.e(self) + VE.e(o) + np.abs(v), 1, self.mag + o.mag, False)

    def __mul__(self, o):
        o = V.of(o)
        v = self.v * o.v
        return VE(v, VE.e(self) * np.abs(o.v) + np.abs(self.v) * VE.e(o) + np.abs(v), 1, self.mag * np.abs(o.v) + np.abs(self.v) * o.mag, False)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        v = self.v / o.v
        return VE(v, VE.e(self) / np.abs(o.v) + np.abs(self.v) * VE.e(o) / o.v ** 2 + np.abs(v), 1,
                  self.mag / np.abs(o.v) + np.abs(self.v) * o.mag / o.v ** 2, False)


class AE(A64):
    name = 'f64, first-order errors'

    @staticmethod
    def inp(x):
        return None if x is None else VE(x)

    @staticmethod
    def tanh(a):
        t = np.tanh(a.v)
        return VE(t, (1 - t * t) * VE.e(a) + np.abs(t), 1, (1 - t * t) * a.mag + np.abs(t), False)

    @staticmethod
    def exp(a):
        e = np.exp(a.v)
        return VE(e, e * VE.e(a) + e, 1, e * a.mag + SOFTMAX_L * e, False)

    @staticmethod
    def sigm(a):
        s = 1.0 / (1.0 + np.exp(-a.v))
        return VE(s, s * (1 - s) * VE.e(a) + 2 * s, 1, s * (1 - s) * a.mag + s, False)

    @staticmethod
    def sum(a, axis):
        return VE(a.v.sum(axis), (VE.e(a) + 0 * a.v).sum(axis) + a.v.shape[axis] * np.abs(a.v).sum(axis), 1, a.mag.sum(axis), False)

    @staticmethod
    def dot(w, x):
        aw_, ax = np.abs(w.v), np.abs(x.v)
        return VE(w.v @ x.v, aw_ @ (VE.e(x) + 0 * x.v) + (VE.e(w) + 0 * w.v) @ ax + w.v.shape[1] * (aw_ @ ax), 1, aw_ @ x.mag + w.mag @ ax, False)

    @staticmethod
    def where(cond, a, b):
        a, b = V.of(a), V.of(b)
        return VE(np.where(cond, a.v, b.v), np.where(cond, VE.e(a) + 0 * a.v, VE.e(b) + 0 * b.v), 1, np.where(cond, a.mag, b.mag), False)

    @staticmethod
    def stack(xs):
        xs = [V.of(x) for x in xs]
        return VE(np.stack([x.v for x in xs]), np.stack([VE.e(x) + 0 * x.v for x in xs]), 1, np.stack([x.mag for x in xs]), False)

    @staticmethod
    def reshape(a, shape):
        return VE(a.v.reshape(shape), a.ab.reshape(shape), a.nt, a.mag.reshape(shape), a.exact)

    @staticmethod
    def amax(a):
        return VE(a.v.max())

    @staticmethod
    def zeros(shape):
        return VE(np.zeros(shape))

    @staticmethod
    def rebound(a, ab, nt):
        return VE(a.v, ab, nt, a.mag, False)


class A32(object):
    name = 'f32'

    @staticmethod
    def inp(x):
        return None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32))

    @staticmethod
    def raw(x):
        return x.numpy()

    tanh = staticmethod(torch.tanh)
    exp = staticmethod(torch.exp)

    @staticmethod
    def sigm(a):
        return 1.0 / (1.0 + torch.exp(-a))

    @staticmethod
    def sum(a, axis):
        return a.sum(axis)

    @staticmethod
    def dot(w, x):
        return w @ x

    @staticmethod
    def where(cond, a, b):
        c = torch.from_numpy(np.ascontiguousarray(cond))
        a = a if torch.is_tensor(a) else torch.full((), float(a))
        b = b if torch.is_tensor(b) else torch.full((), float(b))
        return torch.where(c, a, b)

    @staticmethod
    def stack(xs):
        return torch.stack([x if torch.is_tensor(x) else torch.from_numpy(np.asarray(x, np.float32)) for x in xs])

    @staticmethod
    def cat(xs):
        return torch.cat(xs)

    @staticmethod
    def reshape(a, shape):
        return a.reshape(shape)

    @staticmethod
    def amax(a):
        return a.max()

    @staticmethod
    def zeros(shape):
        return torch.zeros(shape)

    @staticmethod
    def rebound(a, ab, nt):
        return a


def _outs(d):
    return {k: out(x.v, x.ab, x.nt, mag=x.mag if np.any(x.mag) else None) for k, x in d.items()}


def _vals(d):
    return {k: x.numpy() for k, x in d.items()}


def both(core):
    """-> (ref, f32) of one core"""
    return (lambda inp, *a, **k: _outs(core(A64, inp, *a, **k))), (lambda inp, *a, **k: _vals(core(A32, inp, *a, **k)))


L_SETTLE = 8.0          # the libm allowance the redraw margins assume: the GPU file's L_LIBM (it asserts they agree)


def bound_of(x, L=L_SETTLE):
    """the forward bound `check` gives a V, its libm share included"""
    return (x.nt + 2) * U24 * x.ab + L * 2.0 ** -23 * x.mag


def seed(*a):
    s = 12345
    for v in a:
        s = (s * 1000003 + int(v) * 7919 + 17) % (2 ** 31 - 1)
    return s


def nextf(a, up):
    return np.nextafter(np.asarray(a, np.float32), np.float32(np.inf if up else -np.inf))


# ------------------------------------------------------------------------------------------------------------------ attention forward
# (L, D or R): one live wave and lane group; a partial first workgroup; 64 + 4 channels and an L no multiple of 4, 16, 64; the LDS arrays one
# short of full and full with a ragged second float4 trip; the product's shape
ATT_LD = [(1, 4), (3, 8), (50, 68), (255, 260), (256, 260), (196, 512)]
ATT_REJECT_L = 257


def ld_id(c):
    return 'L%d-D%d' % (c[0], c[1])


def att_fwd_make(c):
    L, D = c
    rs = np.random.RandomState(seed(1, L, D))
    return dict(patt=rnd(rs, (L, D)), att_h=rnd(rs, (D,)), aw=rnd(rs, (D,), scale=D ** -0.5), ab=rnd(rs, (1,)), att=rnd(rs, (L, D)), dots=rnd(rs, (L,)))


def att_dots_core(A, inp):
    """tanh_ws[l][d] = tanhf(patt[l][d] + att_h[d]); dots[l] = sum_d tanh_ws[l][d] aw[d] + ab"""
    t = A.tanh(A.inp(inp['patt']) + A.inp(inp['att_h'])[None, :])
    return dict(tanh_ws=t, dots=A.sum(t * A.inp(inp['aw'])[None, :], 1) + A.inp(inp['ab'])[0])


def softmax_core(A, dots):
    """block_softmax: the maximum is exact, x - max one rounding in expf's argument, L additions, one divide"""
    e = A.exp(dots - A.amax(dots))
    return e / A.sum(e, 0)


def att_apply_core(A, inp):
    """weight = softmax(dots); att_res[d] = sum_l weight[l] att[l][d]"""
    w = softmax_core(A, A.inp(inp['dots']))
    return dict(weight=w, att_res=A.sum(w[:, None] * A.inp(inp['att']), 0))


att_dots_ref, att_dots_f32 = both(att_dots_core)
att_apply_ref, att_apply_f32 = both(att_apply_core)


# ------------------------------------------------------------------------------------------------------------------ gate blocks
GATES_R = [4, 8, 260, 512]
A2C_K = [4, 36, 260, 512]
GATES_BWD = [(R, dh2, dc) for R in GATES_R for dh2 in (False, True) for dc in (False, True)]
# cap_gates_bwd_dw: its LDS holds 2R values (R <= 1024)
GATES_BWD_DW = [(4, 3, False, True), (8, 50, True, False), (260, 3, True, True), (512, 50, False, False), (1024, 3, True, True), (1024, 50, False, True)]
GATES_BWD_DW_REJECT_R = 1028


def planted(R):
    """units with an exact tie, with t1 one float32 step above t0 and one below"""
    if R == 4:
        return [0], [1], [2]
    if R == 8:
        return [0, 5], [1], [2]
    if R < 260:
        return [0, 15, 16, 31, 32, 47, 63, R - 1], [1, 17, 33, 49], [2, 18, 34, 50]
    return [0, 15, 16, 63, 64, 255, 256, R - 1], [1, 17, 65, 257], [2, 18, 66, 258]


def gates_core(A, s, a0, a1, c_prev):
    """att2in_gates_fwd (recur.h): s [5][R]"""
    ig, fg, og = A.sigm(s[0]), A.sigm(s[1]), A.sigm(s[2])
    t0, t1 = s[3] + a0, s[4] + a1
    first = A.raw(t0) >= A.raw(t1)                                   # torch.max(a, b): the first operand wins a tie
    it = A.where(first, t0, t1)
    cn = fg * c_prev + ig * it
    tc = A.tanh(cn)
    return dict(c=cn, h=og * tc, save=A.stack([ig, fg, og, A.inp(np.where(first, 0.0, 1.0)), it, tc]), _t=(t0, t1))


def _gate_sums(rs, R):
    """the five sums of R units: N(0, 1), every seventh unit with one gate sum at +-12 (saturated: tiny gradients)"""
    s = rnd(rs, (5, R))
    for j in range(3, R, 7):
        s[j % 3, j] = np.float32(12.0 if (j // 7) % 2 else -12.0)
    return s


def _settle(rs, R, inp, a_of):
    """plants the ties and steps, then redraws s3 / s4 of every other unit whose selector float32 could decide differently; a_of(inp) -> the
    float64 V's (a0, a1).  Adds inp['ties' / 'ups' / 'downs' / 'dropped']"""
    ties, ups, downs = planted(R)
    s = inp['s']
    s[4, ties] = s[3, ties]
    s[4, ups], s[4, downs] = nextf(s[3, ups], True), nextf(s[3, downs], False)
    keep = np.zeros(R, bool)
    keep[ties + ups + downs] = True
    dropped = np.zeros(R, bool)
    for _ in range(20):
        a0, a1 = a_of(inp)
        t0, t1 = V(s[3]) + a0, V(s[4]) + a1
        bad = (np.abs(t0.v - t1.v) <= bound_of(t0) + bound_of(t1)) & ~keep
        if not bad.any():
            break
        dropped |= bad
        s[3:5, bad] = rnd(rs, (2, int(bad.sum())))
    else:
        raise AssertionError('the selectors did not settle')
    inp.update(ties=ties, ups=ups, downs=downs, dropped=int(dropped.sum()))
    return inp


def gates_fwd_make(R):
    rs = np.random.RandomState(seed(2, R))
    inp = dict(s=_gate_sums(rs, R), a2c=rnd(rs, (2, R)), c_prev=rnd(rs, (R,)))
    ties, ups, downs = planted(R)
    inp['a2c'][1, ties] = inp['a2c'][0, ties]
    inp['a2c'][:, ups + downs] = 0
    return _settle(rs, R, inp, lambda i: (V(i['a2c'][0]), V(i['a2c'][1])))


def gates_fwd_core(A, inp):
    a = A.inp(inp['a2c'])
    g = gates_core(A, A.inp(inp['s']), a[0], a[1], A.inp(inp['c_prev']))
    g.pop('_t')
    return g


gates_fwd_ref, gates_fwd_f32 = both(gates_fwd_core)


def a2c_gates_make(c):
    R, K = c
    rs = np.random.RandomState(seed(3, R, K))
    inp = dict(s=_gate_sums(rs, R), x=rnd(rs, (K,)), w=rnd(rs, (2 * R, K), scale=K ** -0.5), b=rnd(rs, (2 * R,)), c_prev=rnd(rs, (R,)))
    ties, ups, downs = planted(R)
    for j in ties:                                                   # the same operands in the same order: the same float32 sum
        inp['w'][R + j], inp['b'][R + j] = inp['w'][j], inp['b'][j]
    for j in ups + downs:
        inp['w'][j] = inp['w'][R + j] = 0
        inp['b'][j] = inp['b'][R + j] = 0

    def a_of(i):
        a = A64.dot(V(i['w']), V(i['x'])) + V(i['b'])
        return a[:R], a[R:]
    return _settle(rs, R, inp, a_of)


def a2c_gates_core(A, inp):
    """cap_a2c_gates_kernel: a = w x + b (rows j and R + j), then the gate block"""
    R = inp['c_prev'].shape[0]
    a = A.dot(A.inp(inp['w']), A.inp(inp['x'])) + A.inp(inp['b'])
    g = gates_core(A, A.inp(inp['s']), a[:R], a[R:], A.inp(inp['c_prev']))
    g.pop('_t')
    return g


A2C_GATES = [(R, K) for R, K in zip(GATES_R, A2C_K)] + [(260, 4), (8, 512)]
a2c_gates_ref, a2c_gates_f32 = both(a2c_gates_core)


def apply_gates_make(c):
    L, R = c
    rs = np.random.RandomState(seed(4, L, R))
    inp = dict(s=_gate_sums(rs, R), P=rnd(rs, (L, 2 * R)), b=rnd(rs, (2 * R,)), dots=rnd(rs, (L,)), c_prev=rnd(rs, (R,)))
    ties, ups, downs = planted(R)
    for j in ties:
        inp['P'][:, R + j], inp['b'][R + j] = inp['P'][:, j], inp['b'][j]
    for j in ups + downs:
        inp['P'][:, j] = inp['P'][:, R + j] = 0
        inp['b'][j] = inp['b'][R + j] = 0

    def a_of(i):
        w = softmax_core(A64, V(i['dots']))
        a = V(i['b']) + A64.sum(w[:, None] * V(i['P']), 0)
        return a[:R], a[R:]
    return _settle(rs, R, inp, a_of)


def apply_gates_core(A, inp):
    """cap_apply_gates_kernel: weight = softmax(dots); a = b + sum_l weight[l] P[l]; then the gate block"""
    R = inp['c_prev'].shape[0]
    w = softmax_core(A, A.inp(inp['dots']))
    a = A.inp(inp['b']) + A.sum(w[:, None] * A.inp(inp['P']), 0)
    g = gates_core(A, A.inp(inp['s']), a[:R], a[R:], A.inp(inp['c_prev']))
    g.pop('_t')
    g['weight'] = w
    return g


apply_gates_ref, apply_gates_f32 = both(apply_gates_core)


def saved_gates(rs, R):
    """the `save` a forward pass hands to backward, in float32: in / forget / out gates, the selector (ties, steps and the rest alike: it is an
    INPUT here), the max, tanh(c); with saturated gates"""
    s = _gate_sums(rs, R)
    sg = (1.0 / (1.0 + np.exp(-f64(s[:3])))).astype(np.float32)
    sel = (rs.rand(R) < 0.5).astype(np.float32)
    return np.concatenate([sg, sel[None], rnd(rs, (1, R)), np.tanh(rnd(rs, (1, R))).astype(np.float32)])


def gates_bwd_make(c):
    R = c[0]
    rs = np.random.RandomState(seed(5, *c))
    L = c[1] if len(c) == 4 else 1
    return dict(save=saved_gates(rs, R), dh=rnd(rs, (R,)), dh2=rnd(rs, (R,)), dc_in=rnd(rs, (R,)), c_prev=rnd(rs, (R,)), P=rnd(rs, (L, 2 * R)))


def gates_bwd_core(A, inp, has_dh2, has_dc):
    """att2in_gates_bwd (recur.h) from the saved values handed to it; dsums = (ds0, ds1, ds2, d0, d1), da2c = (d0, d1): the selector routes
    dit to one of d0 / d1, the other is an exact 0"""
    sv, c_prev = A.inp(inp['save']), A.inp(inp['c_prev'])
    ig, fg, og, it, tc = sv[0], sv[1], sv[2], sv[4], sv[5]
    first = inp['save'][3] == 0
    dhj = A.inp(inp['dh']) + A.inp(inp['dh2']) if has_dh2 else A.inp(inp['dh'])
    g = dhj * og * (1.0 - tc * tc)
    dcn = A.inp(inp['dc_in']) + g if has_dc else g
    dit = dcn * ig
    d0, d1 = A.where(first, dit, 0.0), A.where(first, 0.0, dit)
    ds = [dcn * it * ig * (1.0 - ig), dcn * c_prev * fg * (1.0 - fg), dhj * tc * og * (1.0 - og)]
    return dict(dsums=A.stack(ds + [d0, d1]), da2c=A.stack([d0, d1]), dc_prev=dcn * fg)


gates_bwd_ref, gates_bwd_f32 = both(gates_bwd_core)


def dweight_core(A, inp):
    """the second half of cap_gates_bwd_dw_kernel, from the da2c the first half stored (inp['da2c'], [2R]): dweight[l] = P[l] . da2c"""
    return dict(dweight=A.dot(A.inp(inp['P']), A.inp(inp['da2c'])))


dweight_ref, dweight_f32 = both(dweight_core)


# ------------------------------------------------------------------------------------------------------------------ attention backward
def att_bwd_make(c, near_const=False):
    """near_const: tanh_ws within 1e-3 of one value per channel over the locations and a dweight with a large common part - the sum over
    the locations of ddot (1 - tanh^2) is then the rounding error of the softmax backward's inner sum unless it is taken centred"""
    L, D = c[:2]
    rs = np.random.RandomState(seed(6, L, D, near_const))
    dots = rnd(rs, (L,))
    e = np.exp(f64(dots) - f64(dots).max())
    t = np.tanh(rnd(rs, (L, D))).astype(np.float32)
    dw = rnd(rs, (L,))
    if near_const:
        t = (np.tanh(rnd(rs, (1, D))) + 1e-3 * (rs.rand(L, D) - 0.5)).astype(np.float32)
        dw = (dw + np.float32(1000.0)).astype(np.float32)
    return dict(weight=(e / e.sum()).astype(np.float32), tanh_ws=t, dweight=dw, aw=rnd(rs, (D,), scale=D ** -0.5), dres=rnd(rs, (D,)), att=rnd(rs, (L, D)),
                dpatt0=rnd(rs, (L, D)), datt0=rnd(rs, (L, D)), daw0=rnd(rs, (D,)), dab0=rnd(rs, (1,)))


def softmax_bwd_core(A, w, dw):
    """ddot[l] = w[l] (dw[l] - sum_l w dw): the rules give ab = w[l] (|dw[l]| + sum_l w |dw|)"""
    return w * (dw - A.sum(w * dw, 0))


def att_h_grad_core(A, dd, t, aw):
    """datt_h[d] = sum_l (ddot[l] aw[d]) (1 - t^2), uncentred (att_h_grad, cap_att_bwd_kernel).  Bound: each ddot's error (nt_dd u absdd) meets
    |aw| (1 - t^2); on the true ddot, 1 - t^2 carries u t^2 + u (1 - t^2) and the products and the L additions (L + 3) u: with
    ab = |aw| sum_l (absdd (1 - t^2) + |dd| t^2) and nt = nt_dd + L + 4 every coefficient is covered"""
    L = t.shape[0] if A is A32 else t.v.shape[0]
    s = A.sum((dd[:, None] * aw[None, :]) * (1.0 - t * t), 0)
    if A is A32:
        return s
    t2 = t.v ** 2
    # (under AE dd.ab is ddot's first-order error, at least |dd|, and dd.nt = 1: the same expression covers every coefficient)
    return A.rebound(s, np.abs(aw.v) * (dd.ab[:, None] * (1 - t2) + np.abs(dd.v)[:, None] * t2).sum(0), dd.nt + L + 4)


def att_h_grad_centered_core(A, dd, w, t, aw):
    """datt_h[d] = -aw[d] sum_l ddot[l] (t^2 - m[d]), m[d] = sum_l w[l] t^2 (topdown_att_bwd_step_kernel).  Bound: each ddot's error on
    |t^2 - m| (a common e w[l] adds e (m - m) = 0 and is within it); on the true ddot the rounding of t^2 (u t^2), of m ((L + 2) u m), of the
    difference, the product and the L additions ((L + 3) u |t^2 - m|), and the last product: ab = |aw| sum_l (absdd |t^2 - m| + |dd| (t^2 + m)),
    nt = nt_dd + L + 6"""
    t2 = t * t
    m = A.sum(w[:, None] * t2, 0)
    s = (-aw) * A.sum(dd[:, None] * (t2 - m[None, :]), 0)
    if A is A32:
        return s
    L = t.v.shape[0]
    return A.rebound(s, np.abs(aw.v) * (dd.ab[:, None] * np.abs(t2.v - m.v[None]) + np.abs(dd.v)[:, None] * (t2.v + m.v[None])).sum(0), dd.nt + L + 6)


def att_bwd_step2_core(A, inp):
    dd = softmax_bwd_core(A, A.inp(inp['weight']), A.inp(inp['dweight']))
    return dict(ddot=dd, datt_h=att_h_grad_core(A, dd, A.inp(inp['tanh_ws']), A.inp(inp['aw'])))


def att_bwd_centered_core(A, inp):
    w = A.inp(inp['weight'])
    dd = softmax_bwd_core(A, w, A.inp(inp['dweight']))
    return dict(ddot=dd, datt_h=att_h_grad_centered_core(A, dd, w, A.inp(inp['tanh_ws']), A.inp(inp['aw'])))


def att_bwd_uncentered_f32(inp):
    """the mutation of tests/test_recur_kernels_cpu.py: the centred kernel's operation taken the uncentred way"""
    return _vals(att_bwd_step2_core(A32, inp))


def att_bwd_step_core(A, inp):
    """cap_att_bwd_step_kernel: dweight[l] = att[l] . dres inside the kernel (its D roundings are part of ddot's chain), then as step2"""
    dw = A.dot(A.inp(inp['att']), A.inp(inp['dres']))
    dd = softmax_bwd_core(A, A.inp(inp['weight']), dw)
    return dict(ddot=dd, datt_h=att_h_grad_core(A, dd, A.inp(inp['tanh_ws']), A.inp(inp['aw'])))


def att_bwd_dw_core(A, inp):
    """the first launch of l2s_cap_attention_bwd"""
    return dict(dweight=A.dot(A.inp(inp['att']), A.inp(inp['dres'])))


def att_bwd_full_core(A, inp):
    """cap_att_bwd_kernel from the dweight its first launch stored (inp['dweight']): dpatt += ddot aw (1 - t^2), datt += w dres,
    datt_h = the sum of the dpatt terms over l (stored), daw += sum_l ddot t, dab += sum_l ddot (which cancels: ab = sum_l absdd)"""
    w, t, aw = A.inp(inp['weight']), A.inp(inp['tanh_ws']), A.inp(inp['aw'])
    dd = softmax_bwd_core(A, w, A.inp(inp['dweight']))
    term = (dd[:, None] * aw[None, :]) * (1.0 - t * t)
    return dict(dpatt=A.inp(inp['dpatt0']) + term, datt=A.inp(inp['datt0']) + w[:, None] * A.inp(inp['dres'])[None, :],
                datt_h=att_h_grad_core(A, dd, t, aw), daw=A.inp(inp['daw0']) + A.sum(dd[:, None] * t, 0), dab=A.inp(inp['dab0']) + A.reshape(A.sum(dd, 0), (1,)))


att_bwd_step2_ref, att_bwd_step2_f32 = both(att_bwd_step2_core)
att_bwd_centered_ref, att_bwd_centered_f32 = both(att_bwd_centered_core)
att_bwd_step_ref, att_bwd_step_f32 = both(att_bwd_step_core)
att_bwd_dw_ref, att_bwd_dw_f32 = both(att_bwd_dw_core)
att_bwd_full_ref, att_bwd_full_f32 = both(att_bwd_full_core)

ATT_BWD_CENTERED = [(L, D, False) for L, D in ATT_LD] + [(12, 68, True), (196, 512, True)]
# (S, L, D, dres given, ldr)
ATT_BWD_BATCHED = [(1, 1, 4, True, 4), (3, 3, 8, False, 8), (3, 50, 68, True, 72), (1, 255, 260, True, 260), (3, 256, 260, False, 264), (1, 196, 512, True, 516),
                   (3, 196, 512, True, 512)]


def att_bwd_batched_make(c):
    S, L, D = c[:3]
    rs = np.random.RandomState(seed(7, S, L, D))
    dots = f64(rnd(rs, (S, L)))
    e = np.exp(dots - dots.max(1, keepdims=True))
    return dict(ddot=rnd(rs, (S, L), scale=0.05), weight=(e / e.sum(1, keepdims=True)).astype(np.float32), dres=rnd(rs, (S, D)),
                tanh_ws=np.tanh(rnd(rs, (S, L, D))).astype(np.float32), aw=rnd(rs, (D,), scale=D ** -0.5),
                dpatt0=rnd(rs, (L, D)), datt0=rnd(rs, (L, D)), daw0=rnd(rs, (D,)), dab0=rnd(rs, (1,)))


def att_bwd_batched_core(A, inp, has_dres):
    """cap_att_bwd_batched_kernel: ddot is an input here; dpatt += sum_t ddot aw (1 - th^2), datt += sum_t w dres, daw += sum_t sum_l ddot th,
    dab += the sum of ddot"""
    dd, th, aw = A.inp(inp['ddot']), A.inp(inp['tanh_ws']), A.inp(inp['aw'])
    r = dict(dpatt=A.inp(inp['dpatt0']) + A.sum((dd[:, :, None] * aw[None, None, :]) * (1.0 - th * th), 0),
             daw=A.inp(inp['daw0']) + A.sum(A.sum(dd[:, :, None] * th, 0), 0),
             dab=A.inp(inp['dab0']) + A.reshape(A.sum(A.sum(dd, 0), 0), (1,)))
    if has_dres:
        r['datt'] = A.inp(inp['datt0']) + A.sum(A.inp(inp['weight'])[:, :, None] * A.inp(inp['dres'])[:, None, :], 0)
    return r


att_bwd_batched_ref, att_bwd_batched_f32 = both(att_bwd_batched_core)


# ------------------------------------------------------------------------------------------------------------------ fused GEMVs
LINEAR2 = [(5, 1030, 512), (4, 4, 4), (300, 1, 260)]
LINEAR2_VARIANTS = [(acc1, acc2, b1, b2) for acc1 in (False, True) for acc2 in (False, True) for b1, b2 in ((True, True), (False, True), (True, False), (False, False))]
# (N, K1, K2, kernel): the split form gives each of its four waves ((K / 4 + 3) / 4) * 4 columns - K = 4, 36, 1028 put that boundary everywhere
LINEAR_SUM2 = [(4096, 36, 4, 'linear_sum2_split_kernel'), (4097, 36, 4, 'linear_sum2_kernel')] + \
              [(N, K1, K2, 'linear_sum2_split_kernel') for N in (1, 300) for K1, K2 in ((512, 256), (260, 4), (4, 1028))]


def linear2_make(c):
    N1, N2, K = c
    rs = np.random.RandomState(seed(8, *c))
    return dict(x=rnd(rs, (K,)), w1=rnd(rs, (N1, K), scale=K ** -0.5), b1=rnd(rs, (N1,)), y10=rnd(rs, (N1,)),
                w2=rnd(rs, (N2, K), scale=K ** -0.5), b2=rnd(rs, (N2,)), y20=rnd(rs, (N2,)))


def linear2_core(A, inp, acc1, acc2, b1, b2):
    x = A.inp(inp['x'])
    r = {}
    for k, acc, b in (('1', acc1, b1), ('2', acc2, b2)):
        y = A.dot(A.inp(inp['w' + k]), x)
        if b:
            y = y + A.inp(inp['b' + k])
        if acc:
            y = y + A.inp(inp['y%s0' % k])
        r['y' + k] = y
    return r


linear2_ref, linear2_f32 = both(linear2_core)


def linear_sum2_make(c):
    N, K1, K2 = c[:3]
    rs = np.random.RandomState(seed(9, N, K1, K2))
    return dict(x1=rnd(rs, (K1,)), w1=rnd(rs, (N, K1), scale=K1 ** -0.5), x2=rnd(rs, (K2,)), w2=rnd(rs, (N, K2), scale=K2 ** -0.5), y0=rnd(rs, (N,)))


def linear_sum2_core(A, inp, acc):
    y = A.dot(A.inp(inp['w1']), A.inp(inp['x1'])) + A.dot(A.inp(inp['w2']), A.inp(inp['x2']))
    return dict(y=y + A.inp(inp['y0']) if acc else y)


linear_sum2_ref, linear_sum2_f32 = both(linear_sum2_core)


# ------------------------------------------------------------------------------------------------------------------ LSTM cell, top-down cell
def lstm_cell_core(A, g, c_prev):
    """lstm_cell_fwd (recur.h): g [4][R], gate order i, f, g, o"""
    i, f, gg, o = A.sigm(g[0]), A.sigm(g[1]), A.tanh(g[2]), A.sigm(g[3])
    cn = f * c_prev + i * gg
    return dict(c=cn, h=o * A.tanh(cn), act=A.stack([i, f, gg, o]))


def lstm_cell_bwd_core(A, dh, dc_in, act, c_prev, c):
    """lstm_cell_bwd (recur.h) from the saved act and c handed to it; tanhf(c) is taken again: the libm allowance is on it"""
    i, f, gg, o = act[0], act[1], act[2], act[3]
    tc = A.tanh(c)
    g = dh * o * (1.0 - tc * tc)
    dcn = g if dc_in is None else dc_in + g
    return dict(dg=A.stack([dcn * gg * i * (1.0 - i), dcn * c_prev * f * (1.0 - f), dcn * i * (1.0 - gg * gg), dh * tc * o * (1.0 - o)]), dc_prev=dcn * f)


def saved_act(rs, R):
    """i, f, g, o as a forward pass stores them (float32), with saturated gates"""
    s = _gate_sums(rs, R)[:4]
    a = 1.0 / (1.0 + np.exp(-f64(s)))
    a[2] = np.tanh(f64(s[2]))
    return a.astype(np.float32)


# (R, segment lengths, options, kernel).  Options: ld = leading dimension of every segment's matrix (default: its length + 4), xoff = the
# first segment's x one float off 16-byte alignment, pre / add0 / add1 / dc_in given.  The scalar kernel is forced three ways: a length 6,
# a leading dimension 26, a misaligned x
TOPDOWN_FWD = [
    (4, (), dict(pre=1), 'topdown_cell_fwd_kernel<true>'),
    (8, (12,), dict(pre=1, add0=1), 'topdown_cell_fwd_kernel<true>'),
    (260, (264, 68), dict(pre=1, add0=1, add1=1), 'topdown_cell_fwd_kernel<true>'),
    (260, (4, 516), dict(), 'topdown_cell_fwd_kernel<true>'),
    (8, (6,), dict(pre=1), 'topdown_cell_fwd_kernel<false>'),
    (8, (12, 24), dict(add1=1, ld=26), 'topdown_cell_fwd_kernel<false>'),
    (260, (264, 68), dict(pre=1, add0=1, xoff=1), 'topdown_cell_fwd_kernel<false>'),
    (4, (70, 3), dict(add0=1), 'topdown_cell_fwd_kernel<false>'),
]
TOPDOWN_BWD = [
    (4, (), dict(add0=1), 'topdown_cell_bwd_kernel<true>'),
    (8, (12,), dict(add0=1, dc_in=1), 'topdown_cell_bwd_kernel<true>'),
    (260, (1040, 68), dict(add1=1), 'topdown_cell_bwd_kernel<true>'),
    (260, (1040, 4, 516), dict(add0=1, add1=1, dc_in=1), 'topdown_cell_bwd_kernel<true>'),
    (8, (6,), dict(add0=1), 'topdown_cell_bwd_kernel<false>'),
    (8, (12, 24, 32), dict(dc_in=1, ld=26 + 8), 'topdown_cell_bwd_kernel<false>'),
    (260, (1040, 68, 8), dict(add0=1, dc_in=1, xoff=1), 'topdown_cell_bwd_kernel<false>'),
    (4, (70, 3, 5), dict(), 'topdown_cell_bwd_kernel<false>'),
]


def topdown_id(c):
    return 'R%d-%s-%s%s' % (c[0], 'x'.join(map(str, c[1])) or 'noseg', c[3].split('<')[1][:-1], ''.join('-%s%s' % kv for kv in sorted(c[2].items())))


def seg_ld(c, n):
    ld = c[2].get('ld')
    return n + 4 if ld is None else max(ld, n)


def topdown_fwd_make(c):
    R, ns = c[:2]
    rs = np.random.RandomState(seed(10, R, *ns))
    tot = max(sum(ns), 1)
    return dict(pre=rnd(rs, (4 * R,)), add0=rnd(rs, (4 * R,), scale=0.3), add1=rnd(rs, (4 * R,), scale=0.3), c_prev=rnd(rs, (R,)),
                xs=[rnd(rs, (n,)) for n in ns], ws=[rnd(rs, (4 * R, n), scale=tot ** -0.5) for n in ns])


def topdown_fwd_core(A, inp, o):
    R = inp['c_prev'].shape[0]
    g = A.zeros(4 * R)
    for x, w in zip(inp['xs'], inp['ws']):
        g = g + A.dot(A.inp(w), A.inp(x))
    for k in ('pre', 'add0', 'add1'):
        if o.get(k):
            g = g + A.inp(inp[k])
    return lstm_cell_core(A, A.reshape(g, (4, R)), A.inp(inp['c_prev']))


topdown_fwd_ref, topdown_fwd_f32 = both(topdown_fwd_core)


def topdown_bwd_make(c):
    R, ns = c[:2]
    rs = np.random.RandomState(seed(11, R, *ns))
    tot = max(sum(ns), 1)
    return dict(add0=rnd(rs, (R,)), add1=rnd(rs, (R,)), dc_in=rnd(rs, (R,)), act=saved_act(rs, R), c_prev=rnd(rs, (R,)), c=rnd(rs, (R,)),
                xs=[rnd(rs, (n,)) for n in ns], ws=[rnd(rs, (R, n), scale=tot ** -0.5) for n in ns])


def topdown_bwd_core(A, inp, o):
    R = inp['c_prev'].shape[0]
    dh = A.zeros(R)
    for x, w in zip(inp['xs'], inp['ws']):
        dh = dh + A.dot(A.inp(w), A.inp(x))
    for k in ('add0', 'add1'):
        if o.get(k):
            dh = dh + A.inp(inp[k])
    return lstm_cell_bwd_core(A, dh, A.inp(inp['dc_in']) if o.get('dc_in') else None, A.inp(inp['act']), A.inp(inp['c_prev']), A.inp(inp['c']))


topdown_bwd_ref, topdown_bwd_f32 = both(topdown_bwd_core)

# pack_rows: (rows, cols, ldd, lds); lds = 0 repeats one source row; 513 x 512 is beyond one pass of the 1024-workgroup grid
PACK_ROWS = [(1, 1, 1, 1), (3, 5, 9, 7), (7, 36, 40, 0), (4, 260, 260, 264), (513, 512, 516, 512), (513, 512, 512, 0)]


# ------------------------------------------------------------------------------------------------------------------ encoder steps
STEP_H = [4, 8, 260, 512]
STEP_FWD = [(H, ndir) for H in STEP_H for ndir in (1, 2)]
# backward: at the first step processed (nothing from a next step; dh_ext given), at a later one (next given, dh_ext absent, carries given),
# and with both
STEP_BWD = [(H, ndir, nxt, ext) for H in STEP_H for ndir in (1, 2) for nxt, ext in ((False, True), (True, False), (True, True))]


def step_id(c):
    return 'H%d-ndir%d' % c[:2] + (''.join('-%s' % n for n, v in zip(('next', 'ext'), c[2:]) if v))


def step_fwd_make(kind, c):
    """one dict per direction; kind: 'lstm' (4 gates), 'gru' (3), 'rnn' (1)"""
    H, ndir = c
    G = dict(lstm=4, gru=3, rnn=1)[kind]
    rs = np.random.RandomState(seed(12, G, H, ndir))
    return [dict(w=rnd(rs, (G * H, H), scale=H ** -0.5), b=rnd(rs, (G * H,), scale=0.3), g_in=rnd(rs, (G * H,)), h_prev=np.tanh(rnd(rs, (H,))).astype(np.float32),
                 c_prev=rnd(rs, (H,))) for _ in range(ndir)]


def lstm_step_fwd_core(A, d):
    H = d['c_prev'].shape[0]
    g = A.inp(d['g_in']) + A.dot(A.inp(d['w']), A.inp(d['h_prev'])) + A.inp(d['b'])
    r = lstm_cell_core(A, A.reshape(g, (4, H)), A.inp(d['c_prev']))
    r['g_out'] = g
    return r


def gru_step_fwd_core(A, d):
    """r = s(gi_r + a_r + b_r), z alike, an = a_n + b_n, n = tanh(gi_n + r an), h = (1 - z) n + z h_prev; act = r, z, n, an"""
    H = d['c_prev'].shape[0]
    a, b, gi, hp = A.reshape(A.dot(A.inp(d['w']), A.inp(d['h_prev'])), (3, H)), A.reshape(A.inp(d['b']), (3, H)), A.reshape(A.inp(d['g_in']), (3, H)), A.inp(d['h_prev'])
    an = a[2] + b[2]
    r, z = A.sigm(gi[0] + a[0] + b[0]), A.sigm(gi[1] + a[1] + b[1])
    n = A.tanh(gi[2] + r * an)
    return dict(h=(1.0 - z) * n + z * hp, act=A.stack([r, z, n, an]))


def rnn_step_fwd_core(A, d):
    return dict(h=A.tanh(A.inp(d['g_in']) + A.dot(A.inp(d['w']), A.inp(d['h_prev'])) + A.inp(d['b'])))


lstm_step_fwd_ref, lstm_step_fwd_f32 = both(lstm_step_fwd_core)
gru_step_fwd_ref, gru_step_fwd_f32 = both(gru_step_fwd_core)
rnn_step_fwd_ref, rnn_step_fwd_f32 = both(rnn_step_fwd_core)


def step_bwd_make(kind, c):
    H, ndir = c[:2]
    G = dict(lstm=4, gru=3, rnn=1)[kind]
    rs = np.random.RandomState(seed(13, G, *c))
    ds = []
    for _ in range(ndir):
        act = saved_act(rs, H)
        if kind == 'gru':
            act[3] = rnd(rs, (H,))                                   # r, z (sigmoids), n (tanh), an (a sum)
        ds.append(dict(wT=rnd(rs, (H, G * H), scale=(G * H) ** -0.5), d_next=rnd(rs, (G * H,)), dh_ext=rnd(rs, (H,)), dc_in=rnd(rs, (H,)), carry_in=rnd(rs, (H,)),
                       act=act, c_prev=rnd(rs, (H,)), c=rnd(rs, (H,)), h_prev=np.tanh(rnd(rs, (H,))).astype(np.float32), h=np.tanh(rnd(rs, (H,))).astype(np.float32)))
    return ds


def _dh(A, d, nxt, ext):
    H = d['c_prev'].shape[0]
    dh = A.dot(A.inp(d['wT']), A.inp(d['d_next'])) if nxt else A.zeros(H)
    return dh + A.inp(d['dh_ext']) if ext else dh


def lstm_step_bwd_core(A, d, nxt, ext):
    """dc_in rides with the next step: absent at the first step processed"""
    return lstm_cell_bwd_core(A, _dh(A, d, nxt, ext), A.inp(d['dc_in']) if nxt else None, A.inp(d['act']), A.inp(d['c_prev']), A.inp(d['c']))


def gru_step_bwd_core(A, d, nxt, ext):
    act, hp = A.inp(d['act']), A.inp(d['h_prev'])
    dh = _dh(A, d, nxt, ext)
    if nxt:
        dh = dh + A.inp(d['carry_in'])
    r, z, n, an = act[0], act[1], act[2], act[3]
    dn, dz = dh * (1.0 - z), dh * (hp - n)
    dan, daz = dn * (1.0 - n * n), dz * z * (1.0 - z)
    dar = dan * an * r * (1.0 - r)
    return dict(dgi=A.stack([dar, daz, dan]), dgh=A.stack([dar, daz, dan * r]), carry_out=dh * z)


def rnn_step_bwd_core(A, d, nxt, ext):
    h = A.inp(d['h'])
    return dict(dg=_dh(A, d, nxt, ext) * (1.0 - h * h))


lstm_step_bwd_ref, lstm_step_bwd_f32 = both(lstm_step_bwd_core)
gru_step_bwd_ref, gru_step_bwd_f32 = both(gru_step_bwd_core)
rnn_step_bwd_ref, rnn_step_bwd_f32 = both(rnn_step_bwd_core)

# the unfused LSTM cell: H, with one beyond a 256-thread workgroup
LSTM_CELL_H = [1, 4, 260, 513]


def lstm_cell_make(H):
    rs = np.random.RandomState(seed(14, H))
    return dict(g=_gate_sums(rs, H)[:4].reshape(-1).copy(), c_prev=rnd(rs, (H,)), dh=rnd(rs, (H,)), dc_in=rnd(rs, (H,)), act=saved_act(rs, H), c=rnd(rs, (H,)))


def lstm_cell_fwd_core(A, inp):
    H = inp['c_prev'].shape[0]
    return lstm_cell_core(A, A.reshape(A.inp(inp['g']), (4, H)), A.inp(inp['c_prev']))


def lstm_cell_bwd_entry_core(A, inp, has_dc):
    return lstm_cell_bwd_core(A, A.inp(inp['dh']), A.inp(inp['dc_in']) if has_dc else None, A.inp(inp['act']), A.inp(inp['c_prev']), A.inp(inp['c']))


lstm_cell_fwd_ref, lstm_cell_fwd_f32 = both(lstm_cell_fwd_core)
lstm_cell_bwd_ref, lstm_cell_bwd_f32 = both(lstm_cell_bwd_entry_core)

# rnn_concat: (T, H, ndir, mask given, adds given); 513 x 512 is beyond one pass of the 1024-workgroup grid.  The mask holds 0 and 2 (dropout
# at p = 0.5): the products are exact, the copies bit for bit; only the add at a direction's last processed row rounds
RNN_CONCAT = [(1, 1, 1, False, False), (3, 5, 2, True, True), (7, 36, 1, True, False), (5, 260, 2, False, True), (513, 512, 1, True, True), (513, 256, 2, True, True)]


def rnn_concat_make(c):
    T, H, ndir = c[:3]
    rs = np.random.RandomState(seed(15, T, H, ndir))
    return dict(hs=[rnd(rs, (T, H)) for _ in range(ndir)], mask=(rs.rand(T, ndir * H) < 0.5).astype(np.float32) * 2.0, dx=rnd(rs, (T, ndir * H)),
                adds=[rnd(rs, (H,)) for _ in range(ndir)])


def rnn_concat_fwd_core(A, inp, has_mask):
    o = A.inp(np.concatenate(inp['hs'], 1))
    return dict(out=o * A.inp(inp['mask']) if has_mask else o)


def rnn_concat_bwd_core(A, inp, has_mask, has_adds):
    H, ndir = inp['hs'][0].shape[1], len(inp['hs'])
    v = A.inp(inp['dx']) * A.inp(inp['mask']) if has_mask else A.inp(inp['dx'])
    T = inp['dx'].shape[0]
    r = {}
    for k in range(ndir):
        row = np.zeros((T, 1), bool)
        row[T - 1 if k == 0 else 0] = True
        d = v[:, k * H:(k + 1) * H]
        r['d%d' % k] = A.where(row & np.ones((1, H), bool), d + A.inp(inp['adds'][k])[None, :], d) if has_adds else d
    return r


rnn_concat_fwd_ref, rnn_concat_fwd_f32 = both(rnn_concat_fwd_core)
rnn_concat_bwd_ref, rnn_concat_bwd_f32 = both(rnn_concat_bwd_core)


# ------------------------------------------------------------------------------------------------------------------ adaptive attention
# cell forward: (R, G, ld_hh, ld_r, h_prev's offset in floats, kernel); G = 5 is the max-out cell: ties and steps are planted there
ADAATT_CELL_FWD = [
    (4, 4, 8, 8, 0, 'adaatt_cell_fwd_kernel<4,true>'), (8, 5, 12, 12, 0, 'adaatt_cell_fwd_kernel<5,true>'),
    (260, 4, 264, 268, 0, 'adaatt_cell_fwd_kernel<4,true>'), (260, 5, 264, 264, 0, 'adaatt_cell_fwd_kernel<5,true>'),
    (8, 4, 10, 12, 0, 'adaatt_cell_fwd_kernel<4,false>'), (8, 5, 12, 12, 1, 'adaatt_cell_fwd_kernel<5,false>'),
    (260, 5, 264, 262, 0, 'adaatt_cell_fwd_kernel<5,false>'),
]
# cell backward: (R, G, ld_thh, ld_tr, dsn / dh_ext / dfake / dc_in given, kernel); without dsn (the last token) the launch is the vector one
ADAATT_CELL_BWD = [
    (4, 4, 20, 8, (1, 1, 1, 1), 'adaatt_cell_bwd_kernel<4,true>'), (8, 5, 44, 12, (1, 0, 1, 0), 'adaatt_cell_bwd_kernel<5,true>'),
    (260, 4, 1044, 264, (0, 1, 1, 0), 'adaatt_cell_bwd_kernel<4,true>'), (260, 5, 1304, 264, (1, 1, 0, 1), 'adaatt_cell_bwd_kernel<5,true>'),
    (8, 5, 40, 8, (0, 1, 0, 0), 'adaatt_cell_bwd_kernel<5,true>'),
    (8, 4, 34, 12, (1, 1, 1, 1), 'adaatt_cell_bwd_kernel<4,false>'), (260, 5, 1304, 262, (1, 0, 1, 1), 'adaatt_cell_bwd_kernel<5,false>'),
]
# attention: (S, L, R, dropout mask given); L = 255 fills the 256-slot arrays
ADAATT_ATT = [(1, 1, 4, False), (3, 10, 8, True), (1, 195, 260, True), (3, 255, 260, False), (3, 10, 260, True)]
ADAATT_REJECT_L = 256


def adaatt_cell_fwd_make(c):
    R, G = c[:2]
    rs = np.random.RandomState(seed(20, *c[:5]))
    inp = dict(pre=_gate_sums(rs, R)[np.arange(G + 1) % 5].reshape(-1).copy(), fcrow=rnd(rs, ((G + 1) * R,), scale=0.3), w_hh=rnd(rs, (G * R, R), scale=R ** -0.5),
               b_hh=rnd(rs, (G * R,), scale=0.3), w_r=rnd(rs, (R, R), scale=R ** -0.5), b_r=rnd(rs, (R,), scale=0.3),
               h_prev=np.tanh(rnd(rs, (R,))).astype(np.float32), c_prev=rnd(rs, (R,)), dropped=0)
    if G == 4:
        return inp
    ties, ups, downs = planted(R)
    pre, fc = inp['pre'].reshape(G + 1, R), inp['fcrow'].reshape(G + 1, R)
    for j in ties:
        inp['w_hh'][4 * R + j], inp['b_hh'][4 * R + j], pre[4, j], fc[4, j] = inp['w_hh'][3 * R + j], inp['b_hh'][3 * R + j], pre[3, j], fc[3, j]
    for j in ups + downs:
        inp['w_hh'][3 * R + j] = inp['w_hh'][4 * R + j] = 0
        inp['b_hh'][3 * R + j] = inp['b_hh'][4 * R + j] = 0
        fc[3, j] = fc[4, j] = 0
    pre[4, ups], pre[4, downs] = nextf(pre[3, ups], True), nextf(pre[3, downs], False)
    keep = np.zeros(R, bool)
    keep[ties + ups + downs] = True
    dropped = np.zeros(R, bool)
    for _ in range(20):
        s = _adaatt_sums(A64, inp, G)[0]
        bad = (np.abs(s.v[3] - s.v[4]) <= (bound_of(s)[3] + bound_of(s)[4])) & ~keep
        if not bad.any():
            break
        dropped |= bad
        pre[3:5, bad] = rnd(rs, (2, int(bad.sum())))
    else:
        raise AssertionError('the selectors did not settle')
    inp.update(ties=ties, ups=ups, downs=downs, dropped=int(dropped.sum()))
    return inp


def _adaatt_sums(A, inp, G):
    """sums[q] = (pre + fcrow) + (w_hh h_prev + b_hh), n5 = the row after them + (w_r h_prev + b_r): the kernel's association"""
    R = inp['c_prev'].shape[0]
    hp = A.inp(inp['h_prev'])
    pre, fc = A.reshape(A.inp(inp['pre']), (G + 1, R)), A.reshape(A.inp(inp['fcrow']), (G + 1, R))
    s = (pre[:G] + fc[:G]) + (A.reshape(A.dot(A.inp(inp['w_hh']), hp), (G, R)) + A.reshape(A.inp(inp['b_hh']), (G, R)))
    return s, (pre[G] + fc[G]) + (A.dot(A.inp(inp['w_r']), hp) + A.inp(inp['b_r']))


def adaatt_cell_fwd_core(A, inp, G):
    """adaatt_cell_fwd (recur.h); save = in, forget, out gates, transform, selector of the max, tanh(c), sigmoid(n5)"""
    s, n5 = _adaatt_sums(A, inp, G)
    ig, fg, og = A.sigm(s[0]), A.sigm(s[1]), A.sigm(s[2])
    if G == 5:
        first = A.raw(s[3]) >= A.raw(s[4])
        it, sel = A.where(first, s[3], s[4]), A.inp(np.where(first, 0.0, 1.0))
    else:
        it, sel = A.tanh(s[3]), A.inp(np.zeros(inp['c_prev'].shape[0]))
    cn = fg * A.inp(inp['c_prev']) + ig * it
    tc, sg = A.tanh(cn), A.sigm(n5)
    return dict(c=cn, h=og * tc, fake=sg * tc, save=A.stack([ig, fg, og, it, sel, tc, sg]))


adaatt_cell_fwd_ref, adaatt_cell_fwd_f32 = both(adaatt_cell_fwd_core)


def adaatt_cell_bwd_make(c):
    R, G = c[:2]
    rs = np.random.RandomState(seed(21, *c[:4]))
    sv = saved_gates(rs, R)                                            # in, forget, out, selector, a value, tanh(c)
    save = np.stack([sv[0], sv[1], sv[2], sv[4] if G == 5 else np.tanh(sv[4]).astype(np.float32), sv[3] if G == 5 else 0 * sv[3], sv[5],
                     (1.0 / (1.0 + np.exp(-f64(rnd(rs, (R,)))))).astype(np.float32)])
    return dict(save=save, dsn=rnd(rs, ((G + 1) * R,)), t_hh=rnd(rs, (R, G * R), scale=(G * R) ** -0.5), t_r=rnd(rs, (R, R), scale=R ** -0.5), dh_ext=rnd(rs, (R,)),
                dfake=rnd(rs, (R,)), dc_in=rnd(rs, (R,)), c_prev=rnd(rs, (R,)))


def adaatt_cell_bwd_core(A, inp, G, has):
    """adaatt_cell_bwd (recur.h) from the saved values handed to it; ds = d(sums | n5), [(G + 1)][R]"""
    has_dsn, has_ext, has_dfake, has_dc = has
    R = inp['c_prev'].shape[0]
    sv, c_prev = A.inp(inp['save']), A.inp(inp['c_prev'])
    ig, fg, og, it, tc, sg = sv[0], sv[1], sv[2], sv[3], sv[5], sv[6]
    dh = A.zeros(R)
    if has_dsn:
        dsn = A.inp(inp['dsn'])
        dh = A.dot(A.inp(inp['t_hh']), dsn[:G * R]) + A.dot(A.inp(inp['t_r']), dsn[G * R:])
    if has_ext:
        dh = dh + A.inp(inp['dh_ext'])
    dfake = A.inp(inp['dfake']) if has_dfake else A.zeros(R)
    dtc = og * dh + sg * dfake if has_dfake else og * dh
    g = dtc * (1.0 - tc * tc)
    dcn = A.inp(inp['dc_in']) + g if has_dc else g
    dit = dcn * ig
    ds = [dcn * it * ig * (1.0 - ig), dcn * c_prev * fg * (1.0 - fg), dh * tc * og * (1.0 - og)]
    if G == 5:
        first = inp['save'][4] == 0
        ds += [A.where(first, dit, 0.0), A.where(first, 0.0, dit)]
    else:
        ds.append(dit * (1.0 - it * it))
    return dict(ds=A.stack(ds + [dfake * tc * sg * (1.0 - sg)]), dc_prev=dcn * fg)


adaatt_cell_bwd_ref, adaatt_cell_bwd_f32 = both(adaatt_cell_bwd_core)


def adaatt_att_make(c):
    S, L, R = c[:3]
    rs = np.random.RandomState(seed(22, S, L, R))
    L1 = L + 1
    dots = f64(rnd(rs, (S, L1)))
    e = np.exp(dots - dots.max(1, keepdims=True))
    return dict(att=rnd(rs, (L, R)), patt=rnd(rs, (L, R)), frl=rnd(rs, (S, R)), fre=rnd(rs, (S, R)), hoe=rnd(rs, (S, R)), hol=rnd(rs, (S, R)), aw=rnd(rs, (R,), scale=R ** -0.5),
                ab=rnd(rs, (1,)), mask=(rs.rand(S, L1, R) < 0.5).astype(np.float32) * 2.0, dots=dots.astype(np.float32), PI=(e / e.sum(1, keepdims=True)).astype(np.float32),
                tanh_ws=np.tanh(rnd(rs, (S, L1, R))).astype(np.float32), datten=rnd(rs, (S, R)), ddot=rnd(rs, (S, L1), scale=0.05),
                dpatt0=rnd(rs, (L, R)), datt0=rnd(rs, (L, R)), daw0=rnd(rs, (R,)))


def adaatt_scores_core(A, inp, has_mask):
    """adaatt_scores_kernel: slot 0 embeds the sentinel (fre), slot l location l - 1 (patt); tanh_ws keeps the tanh BEFORE the mask"""
    S = inp['fre'].shape[0]
    ts, ds = [], []
    for s in range(S):
        t = A.tanh(A.inp(np.concatenate([inp['fre'][s][None], inp['patt']])) + A.inp(inp['hoe'][s])[None, :])
        tm = t * A.inp(inp['mask'][s]) if has_mask else t
        ts.append(t)
        ds.append(A.sum(tm * A.inp(inp['aw'])[None, :], 1) + A.inp(inp['ab'])[0])
    return dict(tanh_ws=A.stack(ts), dots=A.stack(ds))


def adaatt_apply_core(A, inp):
    """adaatt_apply_kernel from the dots handed to it: PI = softmax; atten = PI[0] frl + sum_l PI[l] att[l - 1] + hol"""
    S = inp['fre'].shape[0]
    ps, at = [], []
    for s in range(S):
        w = softmax_core(A, A.inp(inp['dots'][s]))
        ps.append(w)
        at.append(A.sum(w[:, None] * A.inp(np.concatenate([inp['frl'][s][None], inp['att']])), 0) + A.inp(inp['hol'][s]))
    return dict(PI=A.stack(ps), atten=A.stack(at))


def adaatt_bwd_step_core(A, inp, has_mask):
    """adaatt_att_bwd_step_kernel: dPI[l] = datten . slot_l, the softmax backward, and with u = mask (1 - t^2), m = sum_l PI[l] u the centred
    d(hoe) = aw sum_l ddot[l] (u - m).  Its bound is the centred one of att_h_grad_centered_core with u in place of t^2 (u itself carries three
    roundings on mask (1 + t^2)): ab = |aw| sum_l (absdd |u - m| + |dd| (mask (1 + t^2) + m)), nt = nt_dd + L1 + 8"""
    S = inp['fre'].shape[0]
    aw = A.inp(inp['aw'])
    r = dict(ddot=[], dhoe=[], dfre=[], dctx=[], dfrl=[], dhol=[])
    for s in range(S):
        da, w, t = A.inp(inp['datten'][s]), A.inp(inp['PI'][s]), A.inp(inp['tanh_ws'][s])
        dd = softmax_bwd_core(A, w, A.dot(A.inp(np.concatenate([inp['frl'][s][None], inp['att']])), da))
        u = A.inp(inp['mask'][s]) * (1.0 - t * t) if has_mask else 1.0 - t * t
        m = A.sum(w[:, None] * u, 0)
        ho = aw * A.sum(dd[:, None] * (u - m[None, :]), 0)
        if A is A64:
            uab = (f64(inp['mask'][s]) if has_mask else 1.0) * (1 + t.v ** 2)
            ho = A.rebound(ho, np.abs(aw.v) * (dd.ab[:, None] * np.abs(u.v - m.v[None]) + np.abs(dd.v)[:, None] * (uab + m.v[None])).sum(0), dd.nt + t.v.shape[0] + 8)
        fr = aw * dd[0] * u[0]
        for k, v in (('ddot', dd), ('dhoe', ho), ('dfre', fr), ('dctx', ho - fr), ('dfrl', w[0] * da), ('dhol', da)):
            r[k].append(v)
    return {k: A.stack(v) for k, v in r.items()}


def adaatt_bwd_batched_core(A, inp, has_mask):
    """adaatt_att_bwd_batched_kernel: ddot is an input; dpatt[l - 1] += sum_t dd aw (1 - th^2), datt[l - 1] += sum_t PI datten (slot 0, the sentinel,
    has no location), daw += the sum over every slot and token of dd th; dd = ddot mask"""
    th, aw = A.inp(inp['tanh_ws']), A.inp(inp['aw'])
    dd = A.inp(inp['ddot'])[:, :, None] * A.inp(inp['mask']) if has_mask else A.inp(inp['ddot'])[:, :, None]
    dp = A.sum((dd * aw[None, None, :]) * (1.0 - th * th), 0)
    da = A.sum(A.inp(inp['PI'])[:, :, None] * A.inp(inp['datten'])[:, None, :], 0)
    return dict(dpatt=A.inp(inp['dpatt0']) + dp[1:], datt=A.inp(inp['datt0']) + da[1:], daw=A.inp(inp['daw0']) + A.sum(A.sum(dd * th, 0), 0))


adaatt_scores_ref, adaatt_scores_f32 = both(adaatt_scores_core)
adaatt_apply_ref, adaatt_apply_f32 = both(adaatt_apply_core)
adaatt_bwd_step_ref, adaatt_bwd_step_f32 = both(adaatt_bwd_step_core)
adaatt_bwd_batched_ref, adaatt_bwd_batched_f32 = both(adaatt_bwd_batched_core)


# ------------------------------------------------------------------------------------------------------------------ resident recurrence
# (S, L) at R = AH = 512: the shapes l2s_cap_recur_supported accepts that tests/test_kernels_gpu.py already launches
RECUR = [(4, 50), (1, 196)]
RECUR_R = 512


def recur_make(c):
    """the weights and per-sentence inputs of one resident launch (the scales of test_captioner_resident_recurrence), and for the CPU file a
    state to start a token from (h, c) and saved values for the last token's backward"""
    S, L = c
    R = AH = RECUR_R
    rs = np.random.RandomState(seed(30, S, L))
    e = np.exp(f64(rnd(rs, (L,))))
    return dict(W_h2h=rnd(rs, (5 * R, R), scale=R ** -0.5), b_h2h=rnd(rs, (5 * R,), scale=0.1), W_att=rnd(rs, (AH, R), scale=R ** -0.5), b_att=rnd(rs, (AH,), scale=0.1),
                patt=rnd(rs, (L, AH), scale=0.5), aw=rnd(rs, (AH,), scale=0.1), ab=rnd(rs, (1,), scale=0.1), P=rnd(rs, (L, 2 * R), scale=0.5), b_a2c=rnd(rs, (2 * R,), scale=0.1),
                sums=rnd(rs, (S, 5 * R), scale=0.7), dho=rnd(rs, (S, R), scale=0.1),
                h=(np.tanh(rnd(rs, (R,))) * 0.5).astype(np.float32), c=rnd(rs, (R,)), save=saved_gates(rs, R), wgt=(e / e.sum()).astype(np.float32),
                tanh_ws=np.tanh(rnd(rs, (L, AH))).astype(np.float32))


def recur_token_core(A, inp, t):
    """one token of cap_recur_fwd_kernel from the state handed to it (inp['h'], inp['c']: the device's own hs[t], cs[t]), so nothing propagates
    across tokens.  INSIDE the token the chain is written out by the rules: att_h = W_h2att h + b (R roundings) is the ARGUMENT of tanhf with
    patt, so tanh_ws carries (1 - t^2) (ab of att_h + |patt|); the dots sum AH of those times alpha; x - max is expf's argument, so each weight
    carries w times the ab of its dot; a2c = b + sum_l w P and s = sums[t] + (W_h2h h + b) (R roundings) meet in the gates, whose sigmoids carry
    s (1 - s) times the ab of their sum.  -> the outputs, and the two transforms (t0, t1) the selector compares"""
    R = RECUR_R
    h = A.inp(inp['h'])
    att_h = A.dot(A.inp(inp['W_att']), h) + A.inp(inp['b_att'])
    th = A.tanh(A.inp(inp['patt']) + att_h[None, :])
    w = softmax_core(A, A.sum(th * A.inp(inp['aw'])[None, :], 1) + A.inp(inp['ab'])[0])
    a = A.inp(inp['b_a2c']) + A.sum(w[:, None] * A.inp(inp['P']), 0)
    s = A.reshape(A.inp(inp['sums'][t]) + (A.dot(A.inp(inp['W_h2h']), h) + A.inp(inp['b_h2h'])), (5, R))
    g = gates_core(A, s, a[:R], a[R:], A.inp(inp['c']))
    return dict(tanh_ws=th, wgt=w, save=g['save'], c=g['c'], h=g['h']), g['_t']


def recur_token_ref(inp, t):
    """-> (the outputs, the units whose selector float32 may decide either way: |t0 - t1| within the two forward bounds.  The state is the
    device's, so such a unit cannot be redrawn; its selector is not compared, its max, c and h are - the max is continuous)"""
    r, (t0, t1) = recur_token_core(AE, inp, t)
    return _outs(r), np.abs(t0.v - t1.v) <= bound_of(t0) + bound_of(t1)


def recur_token_f32(inp, t):
    return _vals(recur_token_core(A32, inp, t)[0])


def recur_bwd_last_core(A, inp):
    """the last token of cap_recur_bwd_kernel: the carries are zero, so dh = dho[S - 1] and dc = 0.  From the saved values handed to it
    (inp['save'] [6][R], inp['c'] = cs[S - 1], inp['wgt'], inp['tanh_ws'] of that token): the gate backward, dweight[l] = P[l] . da2c inside the
    launch (its 2R roundings join ddot's chain), the softmax backward and the uncentred datt_h under att_h_grad_core's bound"""
    R = RECUR_R
    g = gates_bwd_core(A, dict(save=inp['save'], dh=inp['dho'][-1], c_prev=inp['c']), False, False)
    dd = softmax_bwd_core(A, A.inp(inp['wgt']), A.dot(A.inp(inp['P']), A.reshape(g['da2c'], (2 * R,))))
    return dict(dsums=g['dsums'], da2c=g['da2c'], ddot=dd, datt_h=att_h_grad_core(A, dd, A.inp(inp['tanh_ws']), A.inp(inp['aw'])))


def recur_bwd_last_ref(inp):
    return _outs(recur_bwd_last_core(AE, inp))


def recur_bwd_last_f32(inp):
    return _vals(recur_bwd_last_core(A32, inp))
