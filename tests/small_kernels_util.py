"""The small kernels between the GEMMs (csrc/lang.hip linears, csrc/misc_kernels.hip elementwise / pools / column sums / SGD): their case
tables, float64 restatements and the ONE comparison the CPU and the GPU test files share.

Every reference sees the operands the device sees (bf16 inputs are rounded first, then widened to float64) and returns
(ref64, absum64, n_terms): `absum` is the same expression on absolute values and `n_terms` the number of float32 roundings along the
longest chain of one output, so that

    |got - ref| <= (n_terms + 2) * 2^-24 * absum + rho * |ref|                                   (check)

is the standard forward bound of a float32 sum taken in ANY order (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2,
with gamma_n replaced by its first-order value and two terms of slack): loose for rounding, tight for structure - one dropped, doubled or
misplaced term is off by a whole term, orders of magnitude beyond it.  rho = 2^-8 for a bf16 store (half a unit in the last place of an
8-bit significand) plus L * 2^-23 for a result that went through libm (L is measured on the device, see tests/test_small_kernels_gpu.py;
the torch-CPU float32 forms pass with L = 1).  Where absum is 0 (a ReLU-masked zero) the bound is 0: such values are exact.

Where a rounded value is the ARGUMENT of expf (x - lse in a softmax) its absolute error becomes a relative error of the result, so the
`absum` of such an output carries the result times the magnitudes that were rounded on the way to the argument (|x|, |lse|, the number
of terms of the sum inside the logarithm): the same first-order rule, written out next to each reference.

The `*_f32` functions are the plain torch-CPU float32 forms that tests/test_small_kernels_cpu.py runs through `check` on the same tables."""
import numpy as np
import torch

U24 = 2.0 ** -24
RHO_BF16 = 2.0 ** -8
F32, BF16 = 0, 1
STORE = {F32: 'f32', BF16: 'bf16'}


def bf16r(a):
    """float32 array rounded to the nearest bf16 value (ties to even), as float32"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def rnd(rs, shape, dt=F32, scale=1.0):
    a = (rs.standard_normal(shape) * scale).astype(np.float32)
    return bf16r(a) if dt == BF16 else a


def f64(a):
    return np.asarray(a, np.float64)


def stored_as(t, dt):
    """a float32 torch result as the device would store it"""
    return t.bfloat16().float().numpy() if dt == BF16 else t.numpy()


def check(got, ref64, absum64, n_terms, store, libm=0.0, what='', mag=None, floor=0.0):
    """asserts the elementwise bound of this file's docstring and returns the worst |got - ref| / bound (0 where both are 0).
    mag: what the libm allowance multiplies where the result is a difference of a libm value and something else (p - 1: the allowance is on
    p); floor: the absolute error of a float32 value that underflows (2^-126 times what multiplies it afterwards)"""
    got, ref = f64(got), f64(ref64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ab = np.broadcast_to(f64(absum64), ref.shape)
    assert np.isfinite(got).all(), '%s: a result is not finite' % what
    bound = (n_terms + 2) * U24 * ab + (RHO_BF16 if store == 'bf16' else 0.0) * np.abs(ref) + libm * 2.0 ** -23 * (np.abs(ref) if mag is None else f64(mag)) + floor
    err = np.abs(got - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / bound)
    worst = float(ratio.max(initial=0.0))
    if not worst <= 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.ndim else ()
        raise AssertionError('%s: element %s is %.9g, the reference %.9g: %.3g times the bound %.3g (%d of %d elements beyond it)' % (
            what, i, got[i], ref[i], worst, bound[i], int((ratio > 1).sum()), ratio.size))
    return worst


def act64(z, act):
    return np.maximum(z, 0) if act == 1 else np.tanh(z) if act == 2 else z


# ------------------------------------------------------------------------------------------------------------------ linears
# (M, N, K, the kernel the dispatcher has to pick, options).  Options: xoff / woff / yoff = offset of the operand's first element in its
# buffer, in floats; ldx / ldw / ldy = leading dimensions.  The <8,4,1>, <16,4,1> and <24,4,1> instantiations of linear_fwd_kernel cannot
# be reached (16-byte rows with M >= 2 go to the MFMA kernel) and are left alone.
R_, G_, IE_ = 64, 4, 32
LIN_FWD = [
    (1, 70, 512, 'linear_fwd_kernel<1,4,1>', {}),
    (1, 70, 3350, 'linear_fwd_kernel<1,2,1>', {}),
    (1, 70, 37, 'linear_fwd_kernel<1,1,1>', {}),
    (5, 70, 3350, 'linear_fwd_kernel<8,2,1>', {}),
    (5, 70, 37, 'linear_fwd_kernel<8,1,1>', {}),
    (13, 33, 38, 'linear_fwd_kernel<16,2,1>', {}),
    (13, 33, 37, 'linear_fwd_kernel<16,1,1>', {}),
    (50, 33, 38, 'linear_fwd_kernel<24,2,1>', {}),          # three row chunks, the last one ragged
    (50, 33, 37, 'linear_fwd_kernel<24,1,1>', {}),
    # K % 4 == 0, an operand off by one float (scalar loads) and by two floats (8-byte loads)
    (1, 70, 64, 'linear_fwd_kernel<1,1,1>', dict(xoff=1)),
    (1, 70, 64, 'linear_fwd_kernel<1,2,1>', dict(woff=2)),
    (5, 70, 64, 'linear_fwd_kernel<8,1,1>', dict(woff=1)),
    (5, 70, 64, 'linear_fwd_kernel<8,2,1>', dict(xoff=2)),
    (13, 33, 64, 'linear_fwd_kernel<16,1,1>', dict(xoff=1)),
    (13, 33, 64, 'linear_fwd_kernel<16,2,1>', dict(woff=2)),
    (2, 16, 16, 'linear_nt_mfma_kernel<1>', {}),
    (16, 17, 20, 'linear_nt_mfma_kernel<1>', {}),           # K no multiple of 16: two of the four waves have nothing to do
    (16, 3350, 512, 'linear_nt_mfma_kernel<1>', {}),
    (17, 100, 2560, 'linear_nt_mfma_kernel<2>', {}),
    (32, 50, 36, 'linear_nt_mfma_kernel<2>', {}),
    (65, 50, 36, 'linear_nt_mfma_kernel<2>', {}),
    # the network's own views: y = xpre[:, G R:] of rows (G + 1) R wide, w a column block of an [N][IE + 2 R] matrix, x = lin[1:, R:]
    (7, R_, R_, 'linear_nt_mfma_kernel<1>', dict(ldy=(G_ + 1) * R_, yoff=G_ * R_)),
    (1, 4 * R_, 2 * R_, 'linear_fwd_kernel<1,4,1>', dict(ldw=IE_ + 2 * R_, woff=IE_)),
    (6, R_, R_, 'linear_nt_mfma_kernel<1>', dict(ldx=2 * R_, xoff=2 * R_ + R_)),
]
LIN_FWD_VARIANTS = [(bias, act, acc) for bias in (True, False) for act in (0, 1, 2) for acc in (False, True)]


def case_id(c):
    return '%dx%dx%d-%s%s' % (c[0], c[1], c[2], c[3].replace('_kernel', ''), ''.join('-%s%s' % kv for kv in sorted(c[4].items())))


def seed_of(c):
    return (c[0] * 7919 + c[1] * 104729 + c[2] * 31 + sum(c[4].values()) * 7) % (2 ** 31)


def lin_fwd_make(c):
    M, N, K = c[:3]
    rs = np.random.RandomState(seed_of(c))
    return dict(x=rnd(rs, (M, K)), w=rnd(rs, (N, K), scale=K ** -0.5), b=rnd(rs, (N,)), y0=rnd(rs, (M, N)))


def lin_fwd_ref(inp, bias, act, acc):
    x, w = f64(inp['x']), f64(inp['w'])
    z, ab = x @ w.T, np.abs(x) @ np.abs(w).T
    if bias:
        z, ab = z + f64(inp['b']), ab + np.abs(f64(inp['b']))
    if acc:
        z, ab = z + f64(inp['y0']), ab + np.abs(f64(inp['y0']))
    return act64(z, act), ab, x.shape[1] + 2          # ReLU and tanh are 1-Lipschitz: the sum's bound carries over


def lin_fwd_f32(inp, bias, act, acc):
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    z = t['x'] @ t['w'].t()
    if bias:
        z = z + t['b']
    if acc:
        z = z + t['y0']
    return (torch.relu(z) if act == 1 else torch.tanh(z) if act == 2 else z).numpy()


# data gradient dx[M][K] (+)= (dy[M][N] . w[N][K]) (* mul): (M, N, K, kernel, options); ws: 'full' = the workspace the entry point asks
# for, 'short' = one float less, absent = none
LIN_BWD_X = [
    (1, 512, 512, 'gemvT_kernel<1>', {}),                   # a single row and a matrix under 2^20 elements
    (1, 100, 37, 'gemvT_kernel<1>', {}),
    (5, 70, 37, 'gemvT_kernel<8>', {}),
    (21, 64, 38, 'gemvT_kernel<8>', {}),                    # three launches, the last one ragged
    (8, 64, 64, 'gemvT_kernel<8>', dict(woff=1)),
    (5, 70, 36, 'linear_nn_mfma_kernel<1>', {}),
    (16, 64, 64, 'linear_nn_mfma_kernel<1>', {}),
    (3, 40, 4, 'linear_nn_mfma_kernel<1>', {}),
    (3, 40, 68, 'linear_nn_mfma_kernel<1>', {}),
    (4, 1, 64, 'linear_nn_mfma_kernel<1>', {}),
    (4, 15, 64, 'linear_nn_mfma_kernel<1>', {}),
    (40, 130, 200, 'linear_nn_mfma_kernel<2>', {}),
    (17, 64, 64, 'linear_nn_mfma_kernel<2>', {}),
    (21, 3350, 512, 'linear_nn_reduce_kernel', dict(ws='full')),
    (21, 3350, 512, 'linear_nn_mfma_kernel<2>', {}),
    (21, 3350, 512, 'linear_nn_mfma_kernel<2>', dict(ws='short')),
]
# (accumulate, mul, strided): strided = dy a column-offset view of wider rows (D['dall'][:, G R:]) and dx / mul rows wider than K
LIN_BWD_X_VARIANTS = [(acc, mul, st) for acc in (False, True) for mul in (False, True) for st in (False, True)]


def case_id_x(c):
    return '%dx%dx%d-%s%s' % (c[0], c[1], c[2], c[3].replace('_kernel', ''), ''.join('-%s%s' % kv for kv in sorted(c[4].items())))


def lin_bwd_x_make(c):
    M, N, K = c[:3]
    rs = np.random.RandomState((M * 7919 + N * 104729 + K * 31 + len(c[4])) % (2 ** 31))
    return dict(dy=rnd(rs, (M, N)), w=rnd(rs, (N, K), scale=N ** -0.5), mul=rnd(rs, (M, K)), dx0=rnd(rs, (M, K)))


def lin_bwd_x_ref(inp, acc, mul):
    dy, w = f64(inp['dy']), f64(inp['w'])
    z, ab = dy @ w, np.abs(dy) @ np.abs(w)
    if mul:
        z, ab = z * f64(inp['mul']), ab * np.abs(f64(inp['mul']))
    if acc:
        z, ab = z + f64(inp['dx0']), ab + np.abs(f64(inp['dx0']))
    return z, ab, dy.shape[1] + 2


def lin_bwd_x_f32(inp, acc, mul):
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    z = t['dy'] @ t['w']
    if mul:
        z = z * t['mul']
    if acc:
        z = z + t['dx0']
    return z.numpy()


# weight gradient dw[N][K] += dy[M][N]^T x[M][K], db[N] += column sums of dy: (M, N, K, kernel, options)
LIN_BWD_W = [
    (21, 512, 512, 'linear_tn_mfma_kernel<true>', {}),
    (2, 64, 64, 'linear_tn_mfma_kernel<true>', {}),
    (7, 100, 36, 'linear_tn_mfma_kernel<true>', {}),
    (21, 102, 64, 'linear_tn_mfma_kernel<true>', dict(lddy=104)),      # a lane's four columns straddle N
    (9, 300, 68, 'linear_tn_mfma_kernel<true>', {}),                    # two n-blocks, a 4-column k tail
    (21, 64, 64, 'linear_tn_mfma_kernel<false>', dict(lddy=3350)),
    (7, 100, 36, 'linear_tn_mfma_kernel<false>', dict(dyoff=1)),
    (1, 70, 64, 'linear_bwd_w_kernel', {}),
    (5, 70, 37, 'linear_bwd_w_kernel', {}),
    (5, 70, 64, 'linear_bwd_w_kernel', dict(ldx=66)),
    (5, 70, 64, 'linear_bwd_w_kernel', dict(xoff=1)),
    (5, 300, 64, 'linear_bwd_w_kernel', dict(ldx=66, lddy=304)),        # more than one column block of the fallback, both strides
]


def lin_bwd_w_make(c):
    M, N, K = c[:3]
    rs = np.random.RandomState((M * 7919 + N * 104729 + K * 31 + sum(c[4].values())) % (2 ** 31))
    return dict(dy=rnd(rs, (M, N)), x=rnd(rs, (M, K)), dw0=rnd(rs, (N, K)), db0=rnd(rs, (N,)))


def lin_bwd_w_ref(inp):
    dy, x = f64(inp['dy']), f64(inp['x'])
    M = dy.shape[0]
    return ((dy.T @ x + f64(inp['dw0']), np.abs(dy).T @ np.abs(x) + np.abs(f64(inp['dw0'])), M + 1),
            (dy.sum(0) + f64(inp['db0']), np.abs(dy).sum(0) + np.abs(f64(inp['db0'])), M + 1))


def lin_bwd_w_f32(inp):
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    return (t['dw0'] + t['dy'].t() @ t['x']).numpy(), (t['db0'] + t['dy'].sum(0)).numpy()


# ------------------------------------------------------------------------------------------------------------------ elementwise
GRID_CAP = 2048 * 256                 # elements of one pass of the capped grids (2048 workgroups of 256 threads; act_bwd / mask_relu_cast: 1024)
# (n, dtype, b given, c given, kernel)
ADD3 = [
    (1000, F32, True, True, 'add3_kernel'),
    (1000, F32, False, True, 'add3_kernel'),
    (1000, F32, True, False, 'add3_kernel'),
    (8, F32, True, True, 'add3_kernel'),
    (8, BF16, True, True, 'add3_bf16x8_kernel'),
    (1000, BF16, True, True, 'add3_bf16x8_kernel'),
    (1000, BF16, False, True, 'add3_bf16x8_kernel'),
    (1000, BF16, True, False, 'add3_bf16x8_kernel'),
    (1000, BF16, False, False, 'add3_bf16x8_kernel'),
    (1001, BF16, True, True, 'add3_kernel'),
    (1001, BF16, False, False, 'add3_kernel'),
    (GRID_CAP + 1001, BF16, True, True, 'add3_kernel'),              # beyond one pass of the capped grid
    (GRID_CAP + 1001, F32, True, True, 'add3_kernel'),
    (GRID_CAP * 8 + 8 * 37, BF16, True, True, 'add3_bf16x8_kernel'),
]


def add3_make(c):
    n, dt = c[:2]
    rs = np.random.RandomState(n % 65521 + dt)
    return dict(a=rnd(rs, (n,), dt), b=rnd(rs, (n,), dt), c=rnd(rs, (n,)))


def add3_ref(inp, has_b, has_c):
    z, ab = f64(inp['a']), np.abs(f64(inp['a']))
    if has_b:
        z, ab = z + f64(inp['b']), ab + np.abs(f64(inp['b']))
    if has_c:
        z, ab = z + f64(inp['c']), ab + np.abs(f64(inp['c']))
    return z, ab, 2


def add3_f32(inp, has_b, has_c, dt):
    z = torch.from_numpy(inp['a'])
    if has_b:
        z = z + torch.from_numpy(inp['b'])
    if has_c:
        z = z + torch.from_numpy(inp['c'])
    return stored_as(z, dt)


ELT_N = [1003, GRID_CAP + 77]         # a ragged n, and one beyond every grid cap


def elt_make(n, dt):
    rs = np.random.RandomState(n % 65521 + 17 * dt)
    return dict(a=rnd(rs, (n,), dt), b=rnd(rs, (n,), dt), f=rnd(rs, (n,)), g=rnd(rs, (n,)),
                mask=(rs.rand(n) < 0.5).astype(np.float32) * 2.0, y=np.tanh(rnd(rs, (n,))).astype(np.float32))


def scale_mask_ref(inp, has_ref):
    z = f64(inp['a']) * f64(inp['mask'])
    if has_ref:
        z = np.where(f64(inp['b']) > 0, z, 0.0)
    return z, np.abs(z), 1


def act_bwd_ref(inp, act):
    dy, y = f64(inp['f']), f64(inp['y'])
    if act == 1:
        z = np.where(y > 0, dy, 0.0)
        return z, np.abs(z), 0
    if act == 2:
        return dy * (1 - y * y), np.abs(dy) * (1 + y * y), 3
    return dy, np.abs(dy), 0


def mask_relu_ref(inp, has_mul):
    z = f64(inp['f'])
    if has_mul:
        z = z * f64(inp['mask'])
    z = np.where(f64(inp['g']) > 0, z, 0.0)
    return z, np.abs(z), 1


# ------------------------------------------------------------------------------------------------------------------ pools
# spatial mean: (C, dtype, hw, n_img, forward kernel, backward kernel)
AVGPOOL = [(C, dt, hw, n, 'avgpool_fwd_bf16x8_kernel' if dt == BF16 and C % 8 == 0 else 'avgpool_fwd_kernel',
            'avgpool_bwd_bf16x8_kernel' if dt == BF16 and C % 8 == 0 else 'avgpool_bwd_kernel')
           for C, dt in ((8, BF16), (36, BF16), (192, BF16), (2056, BF16), (36, F32), (192, F32)) for hw in (1, 49) for n in (1, 5)]


def avgpool_make(c):
    C, dt, hw, n = c[:4]
    rs = np.random.RandomState(C * 131 + hw * 7 + n + dt)
    return dict(x=rnd(rs, (n, hw, C), dt), dy=rnd(rs, (n, C), dt), addend=rnd(rs, (n, hw, C), dt), ref=rnd(rs, (n, hw, C), dt))


def avgpool_fwd_ref(inp):
    x = f64(inp['x'])
    hw = x.shape[1]
    return x.sum(1) / hw, np.abs(x).sum(1) / hw, hw + 1


def avgpool_fwd_f32(inp, dt):
    return stored_as(torch.from_numpy(inp['x']).sum(1) / inp['x'].shape[1], dt)


def avgpool_bwd_ref(inp, has_add, has_ref):
    hw = inp['x'].shape[1]
    z = np.repeat(f64(inp['dy'])[:, None, :], hw, 1) / hw
    ab = np.abs(z)
    if has_add:
        z, ab = z + f64(inp['addend']), ab + np.abs(f64(inp['addend']))
    if has_ref:
        keep = f64(inp['ref']) > 0
        z, ab = np.where(keep, z, 0.0), np.where(keep, ab, 0.0)
    return z, ab, 3                                    # 1 / hw (the x8 kernel multiplies by its rounded inverse), the product, the sum


def avgpool_bwd_f32(inp, has_add, has_ref, dt):
    hw = inp['x'].shape[1]
    z = (torch.from_numpy(inp['dy'])[:, None, :] / hw).expand(-1, hw, -1)
    if has_add:
        z = z + torch.from_numpy(inp['addend'])
    if has_ref:
        z = torch.where(torch.from_numpy(inp['ref']) > 0, z, torch.zeros(()))
    return stored_as(z.contiguous(), dt)


POOL_OUT = 14
POOL_MAPS = [(38, 63), (10, 14), (7, 9), (20, 5), (14, 14)]      # down, OH > H, both up, mixed, identity
# backward forms: (name, dtype, C, lddy, off_all, off_mask, pixel mask given, relu_ref given, kernel)
POOL_BWD_FORMS = [
    ('x8', BF16, 72, 144, 0, 72, True, True, 'adaptive_pool_bwd_bf16x8_kernel'),
    ('x8-swapped', BF16, 72, 144, 72, 0, True, True, 'adaptive_pool_bwd_bf16x8_kernel'),
    ('x8-nopm', BF16, 72, 144, 72, 0, False, True, 'adaptive_pool_bwd_bf16x8_kernel'),
    ('x8-noref', BF16, 72, 144, 0, 72, True, False, 'adaptive_pool_bwd_bf16x8_kernel'),
    ('c36', BF16, 36, 72, 0, 36, True, True, 'adaptive_pool_bwd_kernel'),
    ('lddy150', BF16, 72, 150, 0, 72, True, True, 'adaptive_pool_bwd_kernel'),
    ('offmask68', BF16, 64, 144, 0, 68, True, True, 'adaptive_pool_bwd_kernel'),
    ('f32', F32, 72, 144, 0, 72, True, True, 'adaptive_pool_bwd_kernel'),
    ('f32-nopm-noref', F32, 72, 144, 0, 72, False, False, 'adaptive_pool_bwd_kernel'),
]
# forward forms: (name, dtype, C, ldy, pixel mask given)
POOL_FWD_FORMS = [('bf16', BF16, 72, 144, True), ('bf16-nopm', BF16, 36, 36, False), ('f32', F32, 72, 80, True), ('f32-wide', F32, 300, 300, False)]


def pool_matrix(H, W, OH, OW):
    """P[bin][pixel] = 1 / |bin| on the pixels of bin [floor(i H / OH), ceil((i + 1) H / OH)) x the same in x (adaptive_avg_pool2d), and
    the largest number of pixels in a bin / of bins on a pixel"""
    P = np.zeros((OH * OW, H * W))
    for oy in range(OH):
        y0, y1 = (oy * H) // OH, -(-((oy + 1) * H) // OH)
        for ox in range(OW):
            x0, x1 = (ox * W) // OW, -(-((ox + 1) * W) // OW)
            blk = np.zeros((H, W))
            blk[y0:y1, x0:x1] = 1.0 / ((y1 - y0) * (x1 - x0))
            P[oy * OW + ox] = blk.reshape(-1)
    return P, int((P > 0).sum(1).max()), int((P > 0).sum(0).max())


def pool_make(H, W, C, dt, seed):
    rs = np.random.RandomState(seed + H * 64 + W)
    OO = POOL_OUT * POOL_OUT
    pm = (rs.rand(H * W) < 0.6).astype(np.float32)
    return dict(x=rnd(rs, (H * W, C), dt), pm=pm, dy_all=rnd(rs, (OO, C), dt), dy_mask=rnd(rs, (OO, C), dt), ref=rnd(rs, (H * W, C), dt))


def pool_fwd_ref(inp, H, W, has_pm):
    P, nbin, _ = pool_matrix(H, W, POOL_OUT, POOL_OUT)
    x = f64(inp['x']) * (f64(inp['pm'])[:, None] if has_pm else 1.0)
    return P @ x, P @ np.abs(x), nbin + 2


def pool_fwd_f32(inp, H, W, has_pm, dt):
    x = torch.from_numpy(inp['x'])
    if has_pm:
        x = x * torch.from_numpy(inp['pm'])[:, None]
    y = torch.nn.functional.adaptive_avg_pool2d(x.view(H, W, -1).permute(2, 0, 1)[None], POOL_OUT)[0]
    return stored_as(y.permute(1, 2, 0).reshape(POOL_OUT * POOL_OUT, -1).contiguous(), dt)


def pool_bwd_ref(inp, H, W, has_pm, has_ref):
    P, _, nper = pool_matrix(H, W, POOL_OUT, POOL_OUT)
    z, ab = P.T @ f64(inp['dy_all']), P.T @ np.abs(f64(inp['dy_all']))
    if has_pm:
        m = f64(inp['pm'])[:, None]
        z, ab = z + m * (P.T @ f64(inp['dy_mask'])), ab + m * (P.T @ np.abs(f64(inp['dy_mask'])))
    if has_ref:
        keep = f64(inp['ref']) > 0
        z, ab = np.where(keep, z, 0.0), np.where(keep, ab, 0.0)
    return z, ab, 4 * nper                             # per bin: the mask product, the sum of the two halves, 1 / |bin| and its product, the running sum


def pool_bwd_f32(inp, H, W, has_pm, has_ref, dt):
    P = torch.from_numpy(pool_matrix(H, W, POOL_OUT, POOL_OUT)[0].astype(np.float32))
    z = P.t() @ torch.from_numpy(inp['dy_all'])
    if has_pm:
        z = z + torch.from_numpy(inp['pm'])[:, None] * (P.t() @ torch.from_numpy(inp['dy_mask']))
    if has_ref:
        z = torch.where(torch.from_numpy(inp['ref']) > 0, z, torch.zeros(()))
    return stored_as(z, dt)


MASK_DOWN = [(160, 224, 10, 14), (37, 53, 3, 4), (600, 1000, 38, 63)]


def mask_down_make(H, W, h, w):
    """a blobby {0,1} mask; where the bins tile evenly, three of them are set to exactly half ones (the >= 0.5 edge)"""
    rs = np.random.RandomState(H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    m = ((np.sin(yy * 9.0 / H + 1) * np.cos(xx * 7.0 / W) + 0.15 * rs.standard_normal((H, W))) > 0.1).astype(np.uint8)
    if H % h == 0 and W % w == 0 and (H // h) % 2 == 0:
        bh, bw = H // h, W // w
        for by, bx in ((0, 0), (h // 2, w // 3), (h - 1, w - 1)):
            m[by * bh:(by + 1) * bh, bx * bw:(bx + 1) * bw] = 0
            m[by * bh:by * bh + bh // 2, bx * bw:(bx + 1) * bw] = 1
    return m


def mask_down_ref(m, h, w):
    H, W = m.shape
    out = np.zeros((h, w), np.float32)
    half = 0
    for oy in range(h):
        y0, y1 = (oy * H) // h, -(-((oy + 1) * H) // h)
        for ox in range(w):
            x0, x1 = (ox * W) // w, -(-((ox + 1) * W) // w)
            mean = f64(m[y0:y1, x0:x1]).mean()
            half += mean == 0.5
            out[oy, ox] = 1.0 if mean >= 0.5 else 0.0
    return out, half


# ------------------------------------------------------------------------------------------------------------------ column sums
COLSUM_ROWS = [1, 15, 64, 1176, 20000]
COLSUM_COLS = [1, 64, 65, 256]


def colsum_ranges(rows):
    """the row ranges l2s_colsum cuts a matrix into when its workspace allows: one per 512 rows, 32 at the most"""
    return min(32, (rows + 511) // 512)


def colsum_make(rows, cols, dt):
    rs = np.random.RandomState(rows * 3 + cols + dt)
    return dict(a=rnd(rs, (rows, cols), dt), out0=rnd(rs, (cols,)))


def colsum_ref(inp):
    a = f64(inp['a'])
    return a.sum(0) + f64(inp['out0']), np.abs(a).sum(0) + np.abs(f64(inp['out0'])), a.shape[0] + 1


def colsum_f32(inp):
    return (torch.from_numpy(inp['a']).sum(0) + torch.from_numpy(inp['out0'])).numpy()


# ------------------------------------------------------------------------------------------------------------------ SGD
def sgd_table(chunk):
    """five segments: (offset, count, row_len, weight_decay, rowscale_off, lr_mult, flags); offsets are filled in order"""
    segs = [
        dict(count=3, row_len=1, weight_decay=1, rowscale_off=-1, lr_mult=1.0, flags=0, pad=0),
        dict(count=chunk + 1, row_len=1, weight_decay=0, rowscale_off=-1, lr_mult=1.0, flags=0, pad=2),     # offset 3 + 2 = 5: no multiple of 4 (scalar)
        dict(count=4 * 9, row_len=4, weight_decay=1, rowscale_off=0, lr_mult=2.5, flags=0, pad=2),           # the smallest vector form with a row scale
        dict(count=6 * 10, row_len=6, weight_decay=1, rowscale_off=9, lr_mult=1.0, flags=1, pad=0),          # rows of 6: scalar; flags & 1: its gradient is never cleared
        dict(count=chunk, row_len=1, weight_decay=1, rowscale_off=-1, lr_mult=0.5, flags=0, pad=0),
    ]
    off = run = 0
    for s in segs:
        off += s.pop('pad')
        s['offset'], s['chunk0'] = off, run
        off += s['count']
        run += -(-s['count'] // chunk)
    return segs, off, 9 + 10


def sgd_make(chunk, g16=False):
    segs, tot, nrs = sgd_table(chunk)
    rs = np.random.RandomState(5)
    g = rnd(rs, (tot,), BF16 if g16 else F32)
    return dict(segs=segs, tot=tot, p=rnd(rs, (tot,)), g=g, m=rnd(rs, (tot,)), rowscale=(rs.rand(nrs) + 0.5).astype(np.float32))


def sgd_ref(inp, lr, momentum, wd, gscale):
    """-> per element (new parameter, new momentum, shadow value) with their absolute sums; elements outside every segment keep p and m
    (their shadow is not written: NaN in the returned shadow)"""
    p, g, m = f64(inp['p']), f64(inp['g']), f64(inp['m'])
    lr, momentum, wd, gscale = (float(np.float32(v)) for v in (lr, momentum, wd, gscale))
    P, M, S = p.copy(), m.copy(), np.full(p.shape, np.nan)
    PA, MA, SA = np.abs(p), np.abs(m), np.zeros(p.shape)
    for s in inp['segs']:
        o, n = s['offset'], s['count']
        sl = slice(o, o + n)
        rsc = f64(inp['rowscale'])[s['rowscale_off'] + np.arange(n) // s['row_len']] if s['rowscale_off'] >= 0 else np.ones(n)
        lwd = wd if s['weight_decay'] else 0.0
        llr = float(np.float32(lr) * np.float32(s['lr_mult']))
        gg, gga = g[sl] * gscale * rsc + lwd * p[sl], np.abs(g[sl]) * gscale * rsc + lwd * np.abs(p[sl])
        M[sl], MA[sl] = momentum * m[sl] + gg, momentum * np.abs(m[sl]) + gga
        P[sl], PA[sl] = p[sl] - llr * M[sl], np.abs(p[sl]) + llr * MA[sl]
        S[sl], SA[sl] = P[sl] * rsc, PA[sl] * rsc
    return (P, PA), (M, MA), (S, SA)


def sgd_f32(inp, lr, momentum, wd, gscale):
    p, g, m = (torch.from_numpy(inp[k]).clone() for k in ('p', 'g', 'm'))
    S = torch.full_like(p, float('nan'))
    for s in inp['segs']:
        o, n = s['offset'], s['count']
        sl = slice(o, o + n)
        rsc = torch.from_numpy(inp['rowscale'])[s['rowscale_off'] + np.arange(n) // s['row_len']] if s['rowscale_off'] >= 0 else torch.ones(n)
        gg = g[sl] * np.float32(gscale) * rsc + np.float32(wd if s['weight_decay'] else 0.0) * p[sl]
        m[sl] = np.float32(momentum) * m[sl] + gg
        p[sl] = p[sl] - (np.float32(lr) * np.float32(s['lr_mult'])) * m[sl]
        S[sl] = p[sl] * rsc
    return p.numpy(), m.numpy(), S.numpy()


# ------------------------------------------------------------------------------------------------------------------ losses and heads
FLOOR = 2.0 ** -126                   # the smallest normal float32: a probability below it, or its product with the factors behind it (all <= 1 here), may be
                                      # flushed to zero or keep a denormal's few bits


def out(ref, ab, nt, mag=None, floor=0.0, pure=False):
    """one output of a reference: the arguments of `check`; mag is None for an output libm has no part in; pure: the output IS a libm value
    (a probability, a log-probability), not a difference of one and something else - the outputs the libm allowance is measured on"""
    return dict(ref=ref, ab=ab, nt=nt, mag=mag, floor=floor, pure=pure)


def check_out(got, o, store, L, what):
    return check(got, o['ref'], o['ab'], o['nt'], store, libm=0.0 if o['mag'] is None else L, mag=o['mag'], floor=o['floor'], what=what)


def softmax_parts(x):
    """rows of x: p, lse, log(sum exp(x - max)), x - max and A = sum_v p_v |x_v - max|.  First order: the sum inside the logarithm has the
    relative error (V + 1) u of V additions, u A of the rounded arguments and one expf; the logarithm adds its own, lse = max + log one more"""
    mx = x.max(1, keepdims=True)
    a = x - mx
    e = np.exp(a)
    se = e.sum(1, keepdims=True)
    p = e / se
    return p, mx + np.log(se), np.log(se), a, (p * np.abs(a)).sum(1, keepdims=True)


def bce_parts(x, t):
    """BCE with logits max(x, 0) - x t + log1p(exp(-|x|)) and its sigmoid: values, absolute sums, what libm touches (expf's relative error e
    moves log1p(E) by e E / (1 + E) <= 2 e log1p(E))"""
    sp = np.log1p(np.exp(-np.abs(x)))
    sig = 1.0 / (1.0 + np.exp(-x))
    return np.maximum(x, 0) - x * t + sp, np.maximum(x, 0) + np.abs(x * t) + sp, 3 * sp, sig


def smooth_l1_parts(pred, tgt, iw, s2):
    """d = iw (pred - tgt) carries 2 u D, D = |iw| (|pred| + |tgt|); v = s2 d^2 / 2 below 1 / s2 (its error s2 |d| 2 u D), |d| - 1 / (2 s2) beyond;
    g = dv / dd = s2 d or the sign.  -> v, the absolute sum of v, g, the absolute sum of g"""
    d = iw * (pred - tgt)
    D = np.abs(iw) * (np.abs(pred) + np.abs(tgt))
    quad = np.abs(d) < 1.0 / s2
    v = np.where(quad, 0.5 * s2 * d * d, np.abs(d) - 0.5 / s2)
    va = np.where(quad, s2 * np.abs(d) * D + 0.5 * s2 * d * d, D + np.abs(d) + 0.5 / s2)
    g = np.where(quad, s2 * d, np.sign(d))
    ga = np.where(quad, s2 * D, np.abs(np.sign(d)))
    # next to the branch point both forms agree to first order (the function is C1): the larger allowance of the two holds for either branch
    near = np.abs(np.abs(d) * s2 - 1.0) < 1e-5
    return v, np.where(near, np.maximum(va, D + np.abs(d) + 0.5 / s2), va), g, np.where(near, np.maximum(ga, 1.0), ga)


LSM = [(S, V1, scale) for V1 in (1, 21, 1025, 3350) for S in (1, 7) for scale in (1.0, 100.0)]
LSM_GSCALE = 0.5


def lsm_make(c):
    S, V1, scale = c
    rs = np.random.RandomState(S * 10007 + V1)
    mask = np.ones(S, np.float32)
    if S > 2:
        mask[[2, S - 3]] = 0
    return dict(logits=rnd(rs, (S, V1), scale=scale), target=rs.randint(0, V1, S).astype(np.int64), mask=mask)


def lsm_ref(inp):
    x = f64(inp['logits'])
    S, V1 = x.shape
    p, lse, lg, a, A = softmax_parts(x)
    lp = x - lse
    sens = np.abs(lp) + np.abs(lse) + V1 + 1 + A
    hot = np.zeros((S, V1)); hot[np.arange(S), inp['target']] = 1
    w = (f64(inp['mask']) / f64(inp['mask']).sum())[:, None]
    c = LSM_GSCALE * w
    tg = (np.arange(S), inp['target'])
    return dict(logprobs=out(lp, sens, 1, mag=1 + np.abs(lg) + 0 * lp, pure=True),
                dlogits=out(c * (p - hot), c * (p * (sens + 1) + hot), 4, mag=c * p * (2 + np.abs(lg)), floor=FLOOR),
                loss=out(-(w[:, 0] * lp[tg]).sum(), (w[:, 0] * sens[tg]).sum(), S + 3, mag=(w[:, 0] * (1 + np.abs(lg[:, 0]))).sum()))


def lsm_f32(inp):
    x = torch.from_numpy(inp['logits'])
    lp = torch.log_softmax(x, 1)
    S = x.shape[0]
    hot = torch.zeros_like(x); hot[torch.arange(S), torch.from_numpy(inp['target'])] = 1
    w = torch.from_numpy(inp['mask']) / torch.from_numpy(inp['mask']).sum()
    return dict(logprobs=lp.numpy(), dlogits=(np.float32(LSM_GSCALE) * w[:, None] * (lp.exp() - hot)).numpy(),
                loss=(-(w * lp[torch.arange(S), torch.from_numpy(inp['target'])]).sum()).numpy())


# rcnn_predict: (R, ncls, ldh, logit scale)
RCNN_PRED = [(R, 81, 5 * 81 + pad, scale) for R in (1, 5, 37) for pad, scale in ((0, 1.0), (3, 100.0))]


def rcnn_pred_make(c):
    R, ncls, ldh, scale = c
    rs = np.random.RandomState(R + ncls)
    h = rnd(rs, (R, 5 * ncls))
    h[:, :ncls] *= np.float32(scale)
    return dict(heads=h, stds=np.array([0.1, 0.1, 0.2, 0.2], np.float32), means=np.array([0.0, 0.01, -0.02, 0.0], np.float32))


def rcnn_pred_ref(inp, ncls):
    h = f64(inp['heads'])
    p, _, _, a, A = softmax_parts(h[:, :ncls])
    st, mn = np.tile(f64(inp['stds']), ncls), np.tile(f64(inp['means']), ncls)
    return dict(cls_prob=out(p, p * (np.abs(a) + A + 1), ncls + 3, mag=2 * p, floor=FLOOR, pure=True),
                bbox_pred=out(h[:, ncls:] * st + mn, np.abs(h[:, ncls:] * st) + np.abs(mn), 2))


def rcnn_pred_f32(inp, ncls):
    h = torch.from_numpy(inp['heads'])
    return dict(cls_prob=torch.softmax(h[:, :ncls], 1).numpy(),
                bbox_pred=(h[:, ncls:] * torch.from_numpy(np.tile(inp['stds'], ncls)) + torch.from_numpy(np.tile(inp['means'], ncls))).numpy())


# mask_prob: (RoIs, ms2, ncls, ldsc, per-label form, logit scale); the last one is the all-classes form beyond one pass of its capped grid
MASK_PROB = [(R, 9, 81, 88, True, scale) for R in (1, 5, 37) for scale in (1.0, 100.0)] + [(5, 9, 81, 88, False, 1.0), (67, 196, 81, 88, False, 100.0)]


def mask_prob_make(c):
    R, ms2, ncls, ldsc, per_label, scale = c
    rs = np.random.RandomState(R * 3 + ms2)
    return dict(score=rnd(rs, (R * ms2, ncls), scale=scale), labels=rs.randint(0, ncls, R).astype(np.int32))


def mask_prob_ref(inp, c):
    R, ms2, ncls, ldsc, per_label, scale = c
    x = f64(inp['score'])
    if per_label:
        x = x[np.arange(R * ms2), np.repeat(inp['labels'], ms2)]
    sig = 1.0 / (1.0 + np.exp(-x))
    return out(sig, sig, 3, mag=sig, floor=FLOOR, pure=True)


def mask_prob_f32(inp, c):
    R, ms2, ncls, ldsc, per_label, scale = c
    x = torch.from_numpy(inp['score'])
    if per_label:
        x = x[torch.arange(R * ms2), torch.from_numpy(np.repeat(inp['labels'], ms2)).long()]
    return torch.sigmoid(x).numpy()


# mask head: fg_max RoIs of ms2 pixels, ncls = 100 score columns; labels repeat, differ and include one beyond the reduce kernel's LDS table
FG_MAX, MASK_NCLS = 6, 100
MASK_LABELS = np.array([97, 3, 3, 97, 12, 3], np.int32)
MASK_NUM_FG = [0, 1, 5, FG_MAX + 3]
MASK_LOSS = [(ms2, ldsc, scale) for ms2 in (9, 196) for ldsc, scale in ((MASK_NCLS, 1.0), (MASK_NCLS + 4, 100.0))]
MASK_GSCALE = 0.5


def mask_loss_make(c):
    ms2, ldsc, scale = c
    rs = np.random.RandomState(ms2 + ldsc)
    return dict(score=rnd(rs, (FG_MAX * ms2, MASK_NCLS), scale=scale), mt=(rs.rand(FG_MAX * ms2) < 0.4).astype(np.float32))


def mask_loss_ref(inp, ms2, num_fg):
    nfg = min(num_fg, FG_MAX)
    n = FG_MAX * ms2
    x = f64(inp['score'])[np.arange(n), np.repeat(MASK_LABELS, ms2)]
    valid = np.arange(n) < nfg * ms2
    inv = 1.0 / (nfg * ms2) if nfg else 0.0
    l, la, lm, sig = bce_parts(x, f64(inp['mt']))
    k = inv * MASK_GSCALE
    return dict(loss=out((l * valid).sum() * inv, (la * valid).sum() * inv, nfg * ms2 + 4, mag=(lm * valid).sum() * inv),
                dscore=out(np.where(valid, (sig - f64(inp['mt'])) * k, 0.0), np.where(valid, (sig + f64(inp['mt'])) * k, 0.0), 5, mag=np.where(valid, sig * k, 0.0),
                           floor=FLOOR))


def mask_loss_f32(inp, ms2, num_fg):
    nfg = min(num_fg, FG_MAX)
    n = FG_MAX * ms2
    x = torch.from_numpy(inp['score'])[torch.arange(n), torch.from_numpy(np.repeat(MASK_LABELS, ms2)).long()]
    t = torch.from_numpy(inp['mt'])
    valid = torch.arange(n) < nfg * ms2
    inv = np.float32(1.0 / (nfg * ms2)) if nfg else np.float32(0)
    l = torch.nn.functional.binary_cross_entropy_with_logits(x, t, reduction='none')
    return dict(loss=((l * valid).sum() * inv).numpy(), dscore=(torch.where(valid, (torch.sigmoid(x) - t) * inv * np.float32(MASK_GSCALE), torch.zeros(()))).numpy())


MASKPRED = [(C, ms2, dt) for C in (64, 256, 300) for ms2, dt in ((9, F32), (196, BF16), (9, BF16))]


def maskpred_make(c):
    C, ms2, dt = c
    rs = np.random.RandomState(C + ms2 + dt)
    n = FG_MAX * ms2
    return dict(dscore=rnd(rs, (n,), scale=0.01), w=rnd(rs, (MASK_NCLS, C)), x=rnd(rs, (n, C), dt), ref=rnd(rs, (n, C), dt),
                dw0=rnd(rs, (MASK_NCLS, C)), db0=rnd(rs, (MASK_NCLS,)))


def maskpred_ref(inp, ms2, num_fg, has_ref):
    nfg = min(num_fg, FG_MAX)
    n = FG_MAX * ms2
    d = f64(inp['dscore']) * (np.arange(n) < nfg * ms2)
    dx = d[:, None] * f64(inp['w'])[np.repeat(MASK_LABELS, ms2)]
    if has_ref:
        dx = np.where(f64(inp['ref']) > 0, dx, 0.0)
    dw, dwa, db, dba = f64(inp['dw0']).copy(), np.abs(f64(inp['dw0'])), f64(inp['db0']).copy(), np.abs(f64(inp['db0']))
    x = f64(inp['x'])
    for s in range(nfg):
        sl, l = slice(s * ms2, (s + 1) * ms2), MASK_LABELS[s]
        dw[l] += d[sl] @ x[sl]; dwa[l] += np.abs(d[sl]) @ np.abs(x[sl])
        db[l] += d[sl].sum(); dba[l] += np.abs(d[sl]).sum()
    return dict(dx=out(dx, np.abs(dx), 1), dw=out(dw, dwa, nfg * ms2 + 2), db=out(db, dba, nfg * ms2 + 2))


def maskpred_f32(inp, ms2, num_fg, has_ref, dt):
    nfg = min(num_fg, FG_MAX)
    n = FG_MAX * ms2
    d = torch.from_numpy(inp['dscore']) * (torch.arange(n) < nfg * ms2)
    lab = torch.from_numpy(np.repeat(MASK_LABELS, ms2)).long()
    dx = d[:, None] * torch.from_numpy(inp['w'])[lab]
    if has_ref:
        dx = torch.where(torch.from_numpy(inp['ref']) > 0, dx, torch.zeros(()))
    dw, db, x = torch.from_numpy(inp['dw0']).clone(), torch.from_numpy(inp['db0']).clone(), torch.from_numpy(inp['x'])
    for s in range(nfg):
        sl, l = slice(s * ms2, (s + 1) * ms2), int(MASK_LABELS[s])
        dw[l] += d[sl] @ x[sl]
        db[l] += d[sl].sum()
    return dict(dx=stored_as(dx, dt), dw=dw.numpy(), db=db.numpy())


# RPN loss: (H, W, A); crossed in the tests with the padding of dheads, its dtype, the logit scale and "no anchor sampled"
RPN = [(1, 1, 3), (12, 16, 12), (5, 7, 9)]
RPN_SCALES = [1.0, 40.0, 100.0]
RPN_SIGMA, RPN_GSCALE = 3.0, 0.5


def rpn_make(c, scale, none_sampled=False):
    H, W, A = c
    rs = np.random.RandomState(H * 100 + W * 10 + A)
    n = H * W * A
    heads = rnd(rs, (H * W, 6 * A))
    heads[:, :2 * A] *= np.float32(scale)
    labels = rs.choice([-1, 0, 1], size=(A, H, W), p=[0.6, 0.25, 0.15]).astype(np.int32)
    if none_sampled:
        labels[:] = -1
    lab = labels.transpose(1, 2, 0).reshape(n)                    # (h, w, a) order, the order of the targets and weights
    cnt = int((lab != -1).sum())
    inw = np.repeat((lab == 1).astype(np.float32), 4)
    return dict(heads=heads, labels=labels, tgt=rnd(rs, (n * 4,)), inw=inw, outw=(inw / np.float32(max(cnt, 1))).astype(np.float32), cnt=cnt)


def rpn_ref(inp, c, ldd):
    H, W, A = c
    n, s2, k = H * W * A, RPN_SIGMA ** 2, RPN_GSCALE
    h = f64(inp['heads'])
    lab = inp['labels'].transpose(1, 2, 0).reshape(H * W, A)
    inv = 1.0 / inp['cnt'] if inp['cnt'] else 0.0
    bg, fg = h[:, :A], h[:, A:2 * A]
    m = np.maximum(bg, fg)
    lse = m + np.log(np.exp(bg - m) + np.exp(fg - m))
    samp = lab != -1
    xl = np.where(lab == 1, fg, bg)
    sens = np.abs(bg) + np.abs(fg) + np.abs(lse) + 4              # |lse|, the chosen logit, the two-term sum and its rounded argument, with room
    pb, pf = np.exp(bg - lse), np.exp(fg - lse)
    d, da, dm = np.zeros((H * W, ldd)), np.zeros((H * W, ldd)), np.zeros((H * W, ldd))
    for col, p_, one in ((slice(0, A), pb, lab == 0), (slice(A, 2 * A), pf, lab == 1)):
        d[:, col] = np.where(samp, (p_ - one) * inv * k, 0.0)
        da[:, col] = np.where(samp, (p_ * (sens + 1) + one) * inv * k, 0.0)
        dm[:, col] = np.where(samp, 2 * p_ * inv * k, 0.0)
    pred, tgt, iw, ow = h[:, 2 * A:], f64(inp['tgt']).reshape(H * W, 4 * A), f64(inp['inw']).reshape(H * W, 4 * A), f64(inp['outw']).reshape(H * W, 4 * A)
    v, va, g, ga = smooth_l1_parts(pred, tgt, iw, s2)
    d[:, 2 * A:6 * A], da[:, 2 * A:6 * A] = ow * iw * g * k, np.abs(ow * iw) * ga * k
    return dict(loss_cls=out(((lse - xl) * samp).sum() * inv, (sens * samp).sum() * inv, n + 3, mag=float(samp.sum()) * inv),
                loss_box=out((ow * v).sum(), (np.abs(ow) * va).sum(), 4 * n + 6),
                dheads=out(d, da, 6, mag=dm, floor=FLOOR))


def rpn_f32(inp, c, ldd, dt):
    H, W, A = c
    s2, k = np.float32(RPN_SIGMA ** 2), np.float32(RPN_GSCALE)
    h = torch.from_numpy(inp['heads'])
    lab = torch.from_numpy(inp['labels'].transpose(1, 2, 0).reshape(H * W, A).copy())
    inv = np.float32(1.0 / inp['cnt']) if inp['cnt'] else np.float32(0)
    two = torch.stack([h[:, :A], h[:, A:2 * A]], 2)
    lp = torch.log_softmax(two, 2)
    samp = lab != -1
    ce = -torch.where(lab == 1, lp[..., 1], lp[..., 0])
    d = torch.zeros(H * W, ldd)
    d[:, :A] = torch.where(samp, (lp[..., 0].exp() - (lab == 0).float()) * inv * k, torch.zeros(()))
    d[:, A:2 * A] = torch.where(samp, (lp[..., 1].exp() - (lab == 1).float()) * inv * k, torch.zeros(()))
    pred, tgt, iw, ow = h[:, 2 * A:], torch.from_numpy(inp['tgt']).view(H * W, 4 * A), torch.from_numpy(inp['inw']).view(H * W, 4 * A), torch.from_numpy(inp['outw']).view(H * W, 4 * A)
    dd = iw * (pred - tgt)
    quad = dd.abs() < 1.0 / s2
    v = torch.where(quad, 0.5 * s2 * dd * dd, dd.abs() - 0.5 / s2)
    g = torch.where(quad, s2 * dd, torch.sign(dd))
    d[:, 2 * A:6 * A] = ow * iw * g * k
    return dict(loss_cls=((ce * samp).sum() * inv).numpy(), loss_box=(ow * v).sum().numpy(), dheads=stored_as(d, dt))


# RCNN loss: (R, ncls)
RCNN = [(R, ncls) for R in (1, 5, 32) for ncls in (2, 81, 130)]
RCNN_GSCALE = 0.5


def rcnn_make(c, scale):
    R, ncls = c
    rs = np.random.RandomState(R * 1000 + ncls)
    h = rnd(rs, (R, 5 * ncls))
    h[:, :ncls] *= np.float32(scale)
    labels = rs.randint(0, ncls, R).astype(np.int32)
    bi = np.zeros((R, 4 * ncls), np.float32)
    for r, l in enumerate(labels):
        if l > 0:
            bi[r, 4 * l:4 * l + 4] = 1
    return dict(heads=h, labels=labels, bt=rnd(rs, (R, 4 * ncls)), bi=bi, bo=bi.copy())


def rcnn_ref(inp, c, ldd):
    R, ncls = c
    k, invR = RCNN_GSCALE, 1.0 / R
    h = f64(inp['heads'])
    x = h[:, :ncls]
    p, lse, lg, a, A = softmax_parts(x)
    hot = np.zeros((R, ncls)); hot[np.arange(R), inp['labels']] = 1
    sens = np.abs(x - lse) + np.abs(lse) + ncls + 2 + A
    tg = (np.arange(R), inp['labels'])
    d, da, dm = np.zeros((R, ldd)), np.zeros((R, ldd)), np.zeros((R, ldd))
    d[:, :ncls], da[:, :ncls], dm[:, :ncls] = (p - hot) * invR * k, (p * (sens + 1) + hot) * invR * k, p * (2 + np.abs(lg)) * invR * k
    v, va, g, ga = smooth_l1_parts(h[:, ncls:], f64(inp['bt']), f64(inp['bi']), 1.0)
    bo, bi = f64(inp['bo']), f64(inp['bi'])
    d[:, ncls:5 * ncls], da[:, ncls:5 * ncls] = bo * bi * g * invR * k, np.abs(bo * bi) * ga * invR * k
    return dict(loss_cls=out((lse[:, 0] - x[tg]).sum() * invR, (np.abs(lse[:, 0]) + np.abs(x[tg]) + ncls + 1 + A[:, 0]).sum() * invR, R + 4, mag=(1 + np.abs(lg)).sum() * invR),
                loss_box=out((bo * v).sum() * invR, (np.abs(bo) * va).sum() * invR, 4 * ncls * R + 6),
                dheads=out(d, da, 6, mag=dm, floor=FLOOR))


def rcnn_f32(inp, c, ldd, dt):
    R, ncls = c
    k, invR = np.float32(RCNN_GSCALE), np.float32(1.0 / R)
    h = torch.from_numpy(inp['heads'])
    lp = torch.log_softmax(h[:, :ncls], 1)
    lab = torch.from_numpy(inp['labels']).long()
    hot = torch.zeros(R, ncls); hot[torch.arange(R), lab] = 1
    d = torch.zeros(R, ldd)
    d[:, :ncls] = (lp.exp() - hot) * invR * k
    bt, bi, bo = (torch.from_numpy(inp[q]) for q in ('bt', 'bi', 'bo'))
    dd = bi * (h[:, ncls:] - bt)
    quad = dd.abs() < 1.0
    v = torch.where(quad, 0.5 * dd * dd, dd.abs() - 0.5)
    d[:, ncls:5 * ncls] = bo * bi * torch.where(quad, dd, torch.sign(dd)) * invR * k
    return dict(loss_cls=(-(lp[torch.arange(R), lab]).sum() * invR).numpy(), loss_box=((bo * v).sum() * invR).numpy(), dheads=stored_as(d, dt))


# response loss: (mask height, mask width, H, W)
RESPONSE = [(600, 1000, 38, 63), (97, 131, 7, 9), (20, 30, 20, 30)]
RESP_GSCALE = 0.5


def response_make(c, scale=1.0):
    MH, MW, H, W = c
    rs = np.random.RandomState(MH + W)
    return dict(resp=rnd(rs, (H * W,), scale=scale), mask=mask_down_make(MH, MW, H, W))


def response_ref(inp, c, target):
    """target: the ground-truth mask at the map's size ([H][W] of 0 / 1), from the oracle's nearest resize"""
    n = c[2] * c[3]
    t = f64(target).reshape(n)
    l, la, lm, sig = bce_parts(f64(inp['resp']), t)
    k = RESP_GSCALE / n
    return dict(loss=out(l.sum() / n, la.sum() / n, n + 4, mag=lm.sum() / n), dresp=out((sig - t) * k, (sig + t) * k, 5, mag=sig * k, floor=FLOOR))


def response_f32(inp, c, target):
    n = c[2] * c[3]
    x, t = torch.from_numpy(inp['resp']), torch.from_numpy(np.ascontiguousarray(target, np.float32)).view(n)
    return dict(loss=torch.nn.functional.binary_cross_entropy_with_logits(x, t).numpy(), dresp=((torch.sigmoid(x) - t) * np.float32(1.0 / n) * np.float32(RESP_GSCALE)).numpy())


def total_loss_ref(loss8, cap_w):
    """loss slots: rpn_cls, rpn_box, cls, box, mask, caption, total, response"""
    l = f64(loss8)
    return out(l[0] + l[1] + l[2] + l[3] + l[4] + l[7] + float(np.float32(cap_w)) * l[5], np.abs(l[[0, 1, 2, 3, 4, 7]]).sum() + abs(cap_w * l[5]), 7)


# ------------------------------------------------------------------------------------------------------------------ embedding
# (D, T, ids: 'mixed' (a token twice) or 'equal', mask given, relu)
EMBED = [(D, T, ids, m, r) for D in (36, 512, 1000) for T, ids in ((1, 'mixed'), (6, 'mixed'), (6, 'equal')) for m, r in ((True, True), (False, True), (True, False))]
EMBED_VOCAB = 11


def embed_make(c):
    D, T, ids, has_mask, relu = c
    rs = np.random.RandomState(D + T)
    idv = np.full(T, 4, np.int64) if ids == 'equal' else np.array([7, 2, 7, 0, 10, 2][:T], np.int64)
    table = rnd(rs, (EMBED_VOCAB, D))
    mask = ((rs.rand(T, D) < 0.7) * 1.25).astype(np.float32)
    row = table[idv]
    o32 = np.maximum(row, 0) if relu else row
    if has_mask:
        o32 = (o32 * mask).astype(np.float32)
    return dict(table=table, ids=idv, mask=mask, out=o32.astype(np.float32), dout=rnd(rs, (T, D)), dtable0=rnd(rs, (EMBED_VOCAB, D)))


def embed_ref(inp, c):
    D, T, ids, has_mask, relu = c
    row = f64(inp['table'])[inp['ids']]
    o = np.maximum(row, 0) if relu else row
    if has_mask:
        o = o * f64(inp['mask'])
    g = f64(inp['dout']) * (f64(inp['mask']) if has_mask else 1.0)
    if relu:
        g = np.where(inp['out'] == 0, 0.0, g)
    dt_, da = f64(inp['dtable0']).copy(), np.abs(f64(inp['dtable0']))
    for u in range(T):
        dt_[inp['ids'][u]] += g[u]; da[inp['ids'][u]] += np.abs(g[u])
    return dict(out=out(o, np.abs(o), 1), dtable=out(dt_, da, T + 1))


def embed_f32(inp, c):
    D, T, ids, has_mask, relu = c
    table = torch.from_numpy(inp['table']).clone().requires_grad_(True)
    o = table[torch.from_numpy(inp['ids'])]
    if relu:
        o = torch.relu(o)
    if has_mask:
        o = o * torch.from_numpy(inp['mask'])
    o.backward(torch.from_numpy(inp['dout']))
    return dict(out=o.detach().numpy(), dtable=(torch.from_numpy(inp['dtable0']) + table.grad).numpy())


# ------------------------------------------------------------------------------------------------------------------ dynamic filter
# ((H, W), C, dtype, forward kernel, last kernel of the backward without / with the finishing pass)
DYNFILTER = [(hw, C, dt, 'dynfilter_fwd_bf16_kernel' if dt == BF16 and C % 8 == 0 else 'dynfilter_fwd_kernel',
              'dynfilter_bwd2_bf16_kernel' if dt == BF16 and C % 8 == 0 else 'dynfilter_bwd2_kernel')
             for hw in ((1, 1), (3, 5), (13, 17)) for C, dt in ((36, BF16), (72, BF16), (256, BF16), (36, F32), (72, F32))]


def dynfilter_make(c, masks):
    """masks: the seven {0,1} maps of the oracle, [7][H][W].  resp / respk are what the backward is handed: the forward's values in float32"""
    (H, W), C, dt = c[:3]
    rs = np.random.RandomState(H * 100 + W + C + dt)
    inp = dict(x=rnd(rs, (H * W, C), dt), filt=rnd(rs, (7, C), scale=C ** -0.5), r=rnd(rs, (7,), scale=0.6), dy=rnd(rs, (H * W, C), dt),
               ref=rnd(rs, (H * W, C), dt), extra=rnd(rs, (H * W,)), dfilt0=rnd(rs, (7, C)), dr0=rnd(rs, (7,)), m=f64(masks).reshape(7, H * W).T.copy())
    dk = (f64(inp['x']) @ f64(inp['filt']).T) * inp['m']
    inp['respk'] = dk.astype(np.float32)
    inp['resp'] = (dk @ f64(inp['r'])).astype(np.float32)
    return inp


def dynfilter_fwd_ref(inp, gate):
    x, C = f64(inp['x']), inp['x'].shape[1]
    dk, dka = (x @ f64(inp['filt']).T) * inp['m'], (np.abs(x) @ np.abs(f64(inp['filt'])).T) * inp['m']
    resp, ra = dk @ f64(inp['r']), dka @ np.abs(f64(inp['r']))
    res = dict(respk=out(dk, dka, C + 1), resp=out(resp, ra, C + 9))
    if gate:
        sig = 1.0 / (1.0 + np.exp(-resp))          # |d sigmoid| <= |d resp| / 4, plus expf on the value itself
        res['y'] = out(x * sig[:, None], np.abs(x) * (0.25 * ra + sig)[:, None], C + 12, mag=np.abs(x) * sig[:, None])
    else:
        res['y'] = out(x * resp[:, None], np.abs(x) * ra[:, None], C + 10)
    return res


def dynfilter_fwd_f32(inp, gate, dt):
    x, m = torch.from_numpy(inp['x']), torch.from_numpy(inp['m'].astype(np.float32))
    dk = (x @ torch.from_numpy(inp['filt']).t()) * m
    resp = dk @ torch.from_numpy(inp['r'])
    return dict(respk=dk.numpy(), resp=resp.numpy(), y=stored_as(x * (torch.sigmoid(resp) if gate else resp)[:, None], dt))


def dynfilter_bwd_ref(inp, gate, has_extra, has_ref):
    x, dy, m, r, filt = f64(inp['x']), f64(inp['dy']), inp['m'], f64(inp['r']), f64(inp['filt'])
    HW, C = x.shape
    resp, respk = f64(inp['resp']), f64(inp['respk'])
    G, Ga = (dy * x).sum(1), np.abs(dy * x).sum(1)
    if gate:
        sg = 1.0 / (1.0 + np.exp(-resp))
        dresp, Da, Dm, mult = G * sg * (1 - sg), Ga * sg * (1 - sg), 2 * np.abs(G) * sg, sg
    else:
        dresp, Da, Dm, mult = G, Ga, 0 * G, resp
    if has_extra:
        dresp, Da = dresp + f64(inp['extra']), Da + np.abs(f64(inp['extra']))
    t, ta = m @ (filt * r[:, None]), m @ np.abs(filt * r[:, None])                      # [HW][C]
    dx, dxa, dxm = dy * mult[:, None] + dresp[:, None] * t, np.abs(dy * mult[:, None]) + Da[:, None] * ta, (np.abs(dy) * mult[:, None] if gate else 0) + Dm[:, None] * ta
    if has_ref:
        keep = f64(inp['ref']) > 0
        dx, dxa, dxm = np.where(keep, dx, 0.0), np.where(keep, dxa, 0.0), np.where(keep, dxm, 0.0)
    wm = m * dresp[:, None]                                                             # [HW][7]
    dfilt = f64(inp['dfilt0']) + r[:, None] * (wm.T @ x)
    dfa = np.abs(f64(inp['dfilt0'])) + np.abs(r)[:, None] * ((m * Da[:, None]).T @ np.abs(x))
    dfm = np.abs(r)[:, None] * ((m * Dm[:, None]).T @ np.abs(x))
    dr, dra, drm = f64(inp['dr0']) + dresp @ respk, np.abs(f64(inp['dr0'])) + Da @ np.abs(respk), Dm @ np.abs(respk)
    lib = (lambda a: a) if gate else (lambda a: None)
    return dict(dx=out(dx, dxa, C + 16, mag=lib(dxm)), dfilt=out(dfilt, dfa, HW + C + 10, mag=lib(dfm)), dr=out(dr, dra, HW + C + 8, mag=lib(drm)))


def dynfilter_bwd_f32(inp, gate, has_extra, has_ref, dt):
    t_ = lambda k: torch.from_numpy(np.ascontiguousarray(inp[k], np.float32))
    x, dy, m, r, filt, resp, respk = (t_(k) for k in ('x', 'dy', 'm', 'r', 'filt', 'resp', 'respk'))
    G = (dy * x).sum(1)
    if gate:
        sg = torch.sigmoid(resp)
        dresp, mult = G * (sg * (1 - sg)), sg
    else:
        dresp, mult = G, resp
    if has_extra:
        dresp = dresp + t_('extra')
    dx = dy * mult[:, None] + dresp[:, None] * (m @ (filt * r[:, None]))
    if has_ref:
        dx = torch.where(t_('ref') > 0, dx, torch.zeros(()))
    dfilt = t_('dfilt0') + r[:, None] * ((m * dresp[:, None]).t() @ x)
    return dict(dx=stored_as(dx, dt), dfilt=dfilt.numpy(), dr=(t_('dr0') + dresp @ respk).numpy())
