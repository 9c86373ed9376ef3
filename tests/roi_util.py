"""The RoI crop and pool kernels (csrc/roi.hip, csrc/roi_sample.h: l2s_roialign_fwd/bwd, l2s_cropalign_fwd/bwd, l2s_roipool_fwd/bwd): their
case tables, references and the comparison the CPU and the GPU test files share.  The comparison is `check` of tests/small_kernels_util.py,

    |got - ref| <= (n_terms + 2) * 2^-24 * absum + rho * |ref| (+ an absolute term where one is derived),

and every reference returns (ref64, absum64, n_terms) as that file's references do.  The work is in two stages, because the float32 sample
position of roi_sample is up to ~9 x 2^-24 x (map size) away from the float64 one and now and then falls on the other side of an integer:

  1. `sample32` restates roi_sample in numpy float32, one IEEE operation per source operation in the source's order (no fused operation:
     contraction is off there, the divide is correctly rounded).  It is meant to be bit-exact with the device; the GPU file tests that
     on one-hot maps.  `crop_ref` / `crop_bwd_ref` blend in float64 on THOSE positions, so the device is held to a rounding bound alone.
  2. tests/test_roi_cpu.py holds `crop_ref` on `sample32` to `crop64`, the definition (theta, affine_grid, grid_sample on doubles), with
     the position difference as an explicit Lipschitz term.  Nothing of the device enters there.

Counts of float32 roundings (n_terms), from the kernels:
  forward, roialign_fwd_kernel         1 - wx1, 1 - wy1 and their product (3), the tap's product (1), three additions onto the first term (3): 7
  forward, roialign_fwd_bf16x8_kernel  the same weights (roi_taps: 3), then roi_mix8's chain of four fmaf, one rounding a link (4): 7
  backward (both forms), per pixel     the weight (3: the gather form rounds 1 - w per axis and the product, the scatter form as the forward),
                                       the product with the gradient (1), one addition per sample that touches the pixel (count), and for
                                       the gather form one addition per LDS window it merges into the pixel: one per chunk of 256 RoIs and
                                       one more per 2048 entries: count + 4 + ceil(R / 256) + count // 2048
  roipool backward, per element        one atomic addition per pooled value that chose the element, onto the value it held: count + 1
A pixel no sample touches has absum 0, hence bound 0: it has to be exactly 0.

The `*_f32` functions are the plain torch-CPU float32 forms tests/test_roi_cpu.py runs through `check` on the same tables."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import boxes as OB
from small_kernels_util import F32, BF16, STORE, f64, rnd, stored_as

SCALAR, X8 = 'roialign_fwd_kernel', 'roialign_fwd_bf16x8_kernel'
SCATTER, GATHER_F, GATHER_B = 'roialign_bwd_kernel', 'roialign_bwd_gather_kernel<float>', 'roialign_bwd_gather_kernel<bf16_t>'
POOL_FWD, POOL_BWD = 'roipool_fwd_kernel', 'roipool_bwd_kernel'
KERNELS = sorted([SCALAR, X8, SCATTER, GATHER_F, GATHER_B, POOL_FWD, POOL_BWD])
GATHER = {F32: GATHER_F, BF16: GATHER_B}
FWD_TERMS = {SCALAR: 7, X8: 7}
CHUNK, WINDOW = 256, 2048             # RoIs per pass of the gather kernel, entries of its LDS window
POOL_GRID = 8192 * 256                # elements of one pass of roipool_bwd_kernel's capped grid

MAP = (20, 26)                        # H, W of the crop cases' map: the image is 320 x 416
ONEHOT_MAP = (6, 7)
FORMS = ['roialign', 'cropalign']

# forward: (C, dtype, P, kernel, options); foff / ooff = offset of feat / out in its buffer, in elements (4 bf16 = 8 bytes: the 16-byte rule)
FWD = [
    (37, F32, 7, SCALAR, {}),                       # odd C
    (300, F32, 7, SCALAR, {}),                      # ragged second trip of the 256-thread loop
    (36, BF16, 7, SCALAR, {}),                      # C % 8 != 0
    (64, BF16, 7, SCALAR, dict(foff=4)),
    (64, BF16, 7, SCALAR, dict(ooff=4)),
    (8, BF16, 7, X8, {}),                           # one lane of 64
    (96, BF16, 14, X8, {}),
    (520, BF16, 7, X8, {}),                         # second trip of the 64-thread loop, one lane
    (1024, BF16, 7, X8, {}),                        # 128 threads
    (1032, BF16, 7, X8, {}),                        # 128 threads, second trip
]
FWD_R = 24
# backward: (C, dtype, P, R, kernel, RoI set)
BWD = ([(4, F32, 7, 24, GATHER_F, 'shared')] +
       [(96, dt, P, R, GATHER[dt], 'shared') for dt in (F32, BF16) for P in (7, 14) for R in (1, 256, 257)] +
       [(1028, BF16, 7, 24, GATHER_B, 'shared'),    # 257 float4 groups a pixel: second trip of the v loop
        (8, F32, 32, 5, GATHER_F, 'shared'),        # bit 31 of the row and column masks
        (64, F32, 7, 300, GATHER_F, 'clustered'), (64, BF16, 7, 300, GATHER_B, 'clustered'),
        (64, F32, 7, 300, GATHER_F, 'seam'), (64, BF16, 7, 300, GATHER_B, 'seam'),
        (37, F32, 7, 24, SCATTER, 'shared'), (37, BF16, 7, 24, SCATTER, 'shared'), (6, F32, 7, 24, SCATTER, 'shared'),
        (8, F32, 33, 3, SCATTER, 'shared')])        # P > 32


def fwd_id(c):
    return 'C%d-%s-P%d-%s%s' % (c[0], STORE[c[1]], c[2], 'x8' if c[3] == X8 else 'scalar', ''.join('-%s%s' % kv for kv in sorted(c[4].items())))


def bwd_id(c):
    return 'C%d-%s-P%d-R%d-%s%s' % (c[0], STORE[c[1]], c[2], c[3], 'scatter' if c[4] == SCATTER else 'gather', '' if c[5] == 'shared' else '-' + c[5])


def geometry(form, H, W):
    """-> (sscale, TH, TW) of roi_sample, and the image size of the align form (no multiple of 16: the two parameterisations differ)"""
    if form == 'roialign':
        return np.float32(1.0 / 16.0), float(H), float(W)
    return np.float32(1.0), 16.0 * H - 3.0, 16.0 * W - 7.0


# ------------------------------------------------------------------------------------------------------------------ RoI sets
def shared_rois(H, W):
    """the 24 RoIs every crop case shares, on an H x W map of a 16 H x 16 W image: (0, x1, y1, x2, y2) rows"""
    IH, IW = 16.0 * H, 16.0 * W
    rs = np.random.RandomState(11)
    b = np.zeros((24, 4))
    n = 12
    x1 = rs.uniform(0, 0.7 * IW, n); y1 = rs.uniform(0, 0.7 * IH, n)
    b[:n] = np.stack([x1, y1, np.minimum(x1 + rs.uniform(10, 0.6 * IW, n), IW - 1), np.minimum(y1 + rs.uniform(10, 0.6 * IH, n), IH - 1)], 1)
    b[10, 2:] = b[10, :2] + rs.uniform(10, 40, 2); b[11, 2:] = b[11, :2] + rs.uniform(10, 40, 2)       # two small ones
    b[12] = [0, 0, IW - 1, IH - 1]                                           # the whole image
    b[13] = [0.335 * IW, 0.534 * IH, 0.335 * IW, 0.534 * IH]                 # a point
    sx, sy = (6 * ((W - 3) // 6) or W - 3), (6 * ((H - 3) // 6) or H - 3)
    b[14] = [16, 16, 16 + 16 * sx, 16 + 16 * sy]                             # corners on multiples of 16: integer sample coordinates, exact zero weights
    b[15] = [0.6 * IW, 0.3 * IH, IW - 1, 0.7 * IH]                           # right edge beyond (W - 1) * 16
    b[16] = [0.2 * IW, 0.55 * IH, 0.5 * IW, IH - 1]                          # bottom edge beyond (H - 1) * 16
    b[17] = [0.5 * IW, 0.5 * IH, IW - 1, IH - 1]
    b[18] = [-40, -25, 0.4 * IW, 0.5 * IH]                                   # starting at negative coordinates
    b[19] = [-12.5, 0.1 * IH, 0.3 * IW, 0.45 * IH]
    b[20] = [IW + 40, IH + 40, IW + 200, IH + 150]                           # wholly outside the map: the crop is 0, nothing comes back
    b[21] = [0.31 * IW + 0.3, 0.25 * IH + 0.2, 0.31 * IW + 0.9, 0.25 * IH + 0.7]      # inside one pixel
    b[22] = b[3]; b[23] = b[15]                                              # duplicates
    return np.concatenate([np.zeros((24, 1)), b], 1).astype(np.float32)


OUTSIDE, WHOLE = 20, 12
FEW = [15, 18, 0, 12, 20, 13, 14, 21]               # what a case of fewer than 24 RoIs takes, in this order


@functools.lru_cache(maxsize=None)
def rois_for(kind, R, H, W):
    if kind != 'shared':
        return clustered_rois(R, H, W, kind == 'seam')
    base = shared_rois(H, W)
    if R <= 24:
        return base.copy() if R == 24 else base[FEW[:R]].copy()
    IH, IW = 16.0 * H, 16.0 * W
    rs = np.random.RandomState(R)
    n = R - 24
    x1 = rs.uniform(-30, IW - 20, n); y1 = rs.uniform(-30, IH - 20, n)
    more = np.stack([np.zeros(n), x1, y1, x1 + rs.uniform(1, 0.7 * IW, n), y1 + rs.uniform(1, 0.7 * IH, n)], 1).astype(np.float32)
    more[-1] = base[15]                             # the last RoI (256 of 257: alone in its chunk) reaches over the edge
    return np.concatenate([base, more], 0)


def clustered_rois(R, H, W, seam=False):
    """the set of test_roialign_bwd_clustered_rois: 200 of 300 RoIs are tiny boxes on one spot, so that every bin of each lands on the same
    few pixels and a pixel's list overflows the LDS window inside the first chunk of 256 (9829 entries on one pixel: five windows); plus
    duplicates, the whole image and a point.
    seam: 43 tiny boxes instead, next to one pixel's centre.  That pixel's list is just beyond one window (2048 < entries < 2300) and its
    entries are of one size, so that the rounding bound of the sum, which grows with the square of the list's length, stays below ONE
    entry: the case on which losing the entry at the window's seam shows (at 9829 entries the bound is larger than an entry)"""
    assert R == 300 and (H, W) == MAP
    rs = np.random.RandomState(5)
    rois = np.zeros((R, 5), np.float32)
    rois[:, 1] = rs.uniform(0, 300, R); rois[:, 2] = rs.uniform(0, 200, R)
    rois[:, 3] = np.minimum(rois[:, 1] + rs.uniform(10, 200, R), 415); rois[:, 4] = np.minimum(rois[:, 2] + rs.uniform(10, 200, R), 319)
    if seam:
        rois[:43, 1] = 96.0 + rs.uniform(0, 1, 43); rois[:43, 2] = 80.0 + rs.uniform(0, 1, 43)
        rois[:43, 3] = rois[:43, 1] + rs.uniform(1, 3, 43); rois[:43, 4] = rois[:43, 2] + rs.uniform(1, 3, 43)
    else:
        rois[:200, 1] = 100.0 + rs.uniform(0, 2, 200); rois[:200, 2] = 84.0 + rs.uniform(0, 2, 200)
        rois[:200, 3] = rois[:200, 1] + rs.uniform(1, 10, 200); rois[:200, 4] = rois[:200, 2] + rs.uniform(1, 10, 200)
    rois[200:210] = rois[210:220]
    rois[220, 1:] = [0, 0, 415, 319]
    rois[221, 1:] = [64, 32, 64, 32]
    return rois


@functools.lru_cache(maxsize=None)
def feat_for(H, W, C, dt):
    return rnd(np.random.RandomState(C * 7 + dt + H), (H * W, C), dt)


@functools.lru_cache(maxsize=None)
def dout_for(R, P, C, dt):
    return rnd(np.random.RandomState(C * 7 + dt + R * 131 + P), (R * P * P, C), dt)


# ------------------------------------------------------------------------------------------------------------------ sample positions
Samples = collections.namedtuple('Samples', 'x0 y0 wx1 wy1 ix iy gx gy')      # x0, wx1, ix, gx: [R][P] per (RoI, column); y0, wy1, iy, gy: per (RoI, row)


def sample32(rois, H, W, P, sscale, TH, TW):
    """roi_sample (csrc/roi_sample.h) in numpy float32: one IEEE operation per source operation, in the source's order, nothing fused.
    -> Samples: the cell x0 / y0 (int64), the weight wx1 / wy1 of the cell after it, the position ix / iy and the normalised grid
    coordinate gx / gy (all float32)"""
    f = np.float32
    rois = np.asarray(rois, f)
    sscale, TH, TW, one = f(sscale), f(TH), f(TW), f(1)
    x1, y1, x2, y2 = (rois[:, k] * sscale for k in (1, 2, 3, 4))
    t00, t02 = (x2 - x1) / (TW - one), (((x1 + x2) - TW) + one) / (TW - one)
    t11, t12 = (y2 - y1) / (TH - one), (((y1 + y2) - TH) + one) / (TH - one)
    step = f(2) / f(P - 1)
    i = np.arange(P)
    # torch.linspace(-1, 1, P): start-based below P / 2, end-based from there on
    base = np.where(i < P // 2, f(-1) + step * i.astype(f), one - step * (P - 1 - i).astype(f)).astype(f)
    gx, gy = t00[:, None] * base[None] + t02[:, None], t11[:, None] * base[None] + t12[:, None]
    ix, iy = ((gx + one) / f(2)) * f(W - 1), ((gy + one) / f(2)) * f(H - 1)
    fx, fy = np.floor(ix), np.floor(iy)
    out = Samples(fx.astype(np.int64), fy.astype(np.int64), ix - fx, iy - fy, ix, iy, gx, gy)
    assert all(a.dtype == f for a in out[2:]), 'an operation left float32'
    return out


def taps(s, H, W, dtype):
    """the four taps of every sample in the kernels' order (00, 01, 10, 11) -> pix[R][P][P][4] = y * W + x, -1 for a tap outside the map
    (dropped), and w[R][P][P][4] = (1 - wx1)(1 - wy1), wx1 (1 - wy1), (1 - wx1) wy1, wx1 wy1 multiplied out in `dtype`: float32 gives the
    scalar kernel's own weights bit for bit, float64 the reference's (1 - w is exact there)"""
    wx, wy = s.wx1.astype(dtype)[:, None, :], s.wy1.astype(dtype)[:, :, None]
    ax, ay = dtype(1) - wx, dtype(1) - wy
    w = np.stack(np.broadcast_arrays(ax * ay, wx * ay, ax * wy, wx * wy), -1)
    x0, y0 = s.x0[:, None, :], s.y0[:, :, None]
    x, y = np.stack(np.broadcast_arrays(x0, x0 + 1, x0, x0 + 1), -1), np.stack(np.broadcast_arrays(y0, y0, y0 + 1, y0 + 1), -1)
    ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    return np.where(ok, y * W + x, -1), w


def axis_weights(i0, w1, n):
    """A[R][P][n]: 1 - w1 on cell i0 and w1 on cell i0 + 1 in float64, cells outside [0, n) dropped: a sample's tap weights are the
    products of its row's and its column's entries"""
    A = np.zeros(i0.shape + (n,))
    w1 = f64(w1)
    for k, w in ((i0, 1.0 - w1), (i0 + 1, w1)):
        ok = (k >= 0) & (k < n)
        r, p = np.nonzero(ok)
        A[r, p, k[ok]] += w[ok]
    return A


def sep_scatter(Ay, Ax, G):
    """out[y][x][c] = sum over (r, p, q) of Ay[r][p][y] Ax[r][q][x] G[r][p][q][c], as two matrix products"""
    R, P, H = Ay.shape
    W, C = Ax.shape[2], G.shape[3]
    t = np.matmul(Ay.transpose(0, 2, 1), G.reshape(R, P, P * C)).reshape(R, H, P, C)           # [r][y][q][c]
    o = Ax.reshape(R * P, W).T @ t.transpose(0, 2, 1, 3).reshape(R * P, H * C)                  # [x][(y c)]
    return o.reshape(W, H, C).transpose(1, 0, 2)


def entries_per_pixel(s, H, W, r_lo=0, r_hi=None):
    """[H][W] samples of RoIs [r_lo, r_hi) with a non-zero weight on each pixel: the length of the gather kernel's list"""
    ny = (axis_weights(s.y0, s.wy1, H)[r_lo:r_hi] != 0).sum(1)
    nx = (axis_weights(s.x0, s.wx1, W)[r_lo:r_hi] != 0).sum(1)
    return ny.T @ nx


def pixel_entries(s, H, W, y, x, r_lo, r_hi):
    """the list of pixel (y, x) in the gather kernel's order (RoI, then row, then column) -> (r, py, px, float64 weight) arrays"""
    Ay, Ax = axis_weights(s.y0, s.wy1, H)[:, :, y], axis_weights(s.x0, s.wx1, W)[:, :, x]
    out = [(r, p, q, Ay[r, p] * Ax[r, q]) for r in range(r_lo, min(r_hi, Ay.shape[0])) for p in np.nonzero(Ay[r])[0] for q in np.nonzero(Ax[r])[0]]
    return tuple(np.array(col) for col in zip(*out))


# ------------------------------------------------------------------------------------------------------------------ crop references
def crop_ref(feat, s, C, kernel=SCALAR, H=None, W=None):
    """feat [H W][C] (the operand the device sees, bf16 already rounded) -> the float64 blend of the four taps of every sample with the
    weights of `taps` widened from float32, taps outside the map dropped: (out [R P P][C], absum, n_terms of `kernel`)"""
    H, W = MAP if H is None else (H, W)
    Fz = np.concatenate([f64(feat).reshape(H * W, C), np.zeros((1, C))], 0)       # row -1: a dropped tap
    pix, w = taps(s, H, W, np.float64)
    R, P = s.x0.shape
    out, ab = np.zeros((R, P, P, C)), np.zeros((R, P, P, C))
    for r0 in range(0, R, 32):
        for k in range(4):
            v = Fz[pix[r0:r0 + 32, :, :, k]]
            out[r0:r0 + 32] += w[r0:r0 + 32, :, :, k, None] * v
            ab[r0:r0 + 32] += w[r0:r0 + 32, :, :, k, None] * np.abs(v)
    return out.reshape(R * P * P, C), ab.reshape(R * P * P, C), FWD_TERMS[kernel]


def crop_fwd_f32(feat, s, C, dt, H=None, W=None):
    """F.grid_sample in float32 on the restated grid (gx, gy of sample32), stored as the device would"""
    H, W = MAP if H is None else (H, W)
    R, P = s.x0.shape
    grid = torch.from_numpy(np.stack(np.broadcast_arrays(s.gx[:, None, :], s.gy[:, :, None]), -1).copy())
    b = torch.from_numpy(np.ascontiguousarray(feat, np.float32)).view(H, W, C).permute(2, 0, 1)[None]
    out = F.grid_sample(b.expand(R, -1, -1, -1), grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    return stored_as(out.permute(0, 2, 3, 1).reshape(R * P * P, C).contiguous(), dt)


def crop_bwd_ref(dout, s, H, W):
    """dout [R P P][C] -> the float64 gradient of the map, every sample's four weights times its gradient added onto its four pixels (as
    sep_scatter's two matrix products: the weights are products of a row and a column factor):
    (dfeat [H W][C], absum, n_terms [H W][1] per pixel)"""
    R, P = s.x0.shape
    C = dout.shape[1]
    G = f64(dout).reshape(R, P, P, C)
    Ay, Ax = axis_weights(s.y0, s.wy1, H), axis_weights(s.x0, s.wx1, W)
    cnt = entries_per_pixel(s, H, W).reshape(H * W, 1)
    nt = np.where(cnt > 0, cnt + 4 + -(-R // CHUNK) + cnt // WINDOW, 0)
    return sep_scatter(Ay, Ax, G).reshape(H * W, C), sep_scatter(Ay, Ax, np.abs(G)).reshape(H * W, C), nt


def crop_bwd_f32(dout, s, H, W):
    """a float32 scatter: the float32 weight times the gradient, index_add_ed onto the map"""
    R, P = s.x0.shape
    C = dout.shape[1]
    pix, w = taps(s, H, W, np.float32)
    g = torch.from_numpy(np.ascontiguousarray(dout, np.float32)).view(R * P * P, C)
    df = torch.zeros(H * W + 1, C)
    for k in range(4):
        idx = torch.from_numpy(np.where(pix[..., k] < 0, H * W, pix[..., k]).reshape(-1))
        df.index_add_(0, idx, torch.from_numpy(w[..., k].reshape(-1, 1).copy()) * g)
    return df[:H * W].numpy()


def crop64(feat, rois, P, H, W, form, dout=None):
    """the reference project's definition in float64: theta as oracle/net.py:crop_pool forms it, F.affine_grid and
    F.grid_sample(align_corners=True) on double tensors; autograd gives the backward.
    -> (out [R P P][C], dfeat [H W][C] or None, ix64 [R][P], iy64 [R][P])"""
    C = feat.shape[1]
    r = torch.from_numpy(f64(rois))
    R = r.shape[0]
    b = torch.from_numpy(f64(feat)).view(H, W, C).permute(2, 0, 1)[None].clone().requires_grad_(dout is not None)
    if form == 'cropalign':
        _, height, width = geometry(form, H, W)
        x1, y1, x2, y2 = r[:, 1:2], r[:, 2:3], r[:, 3:4], r[:, 4:5]
    else:
        height, width = float(H), float(W)
        x1, y1, x2, y2 = r[:, 1:2] / 16.0, r[:, 2:3] / 16.0, r[:, 3:4] / 16.0, r[:, 4:5] / 16.0
    zero = torch.zeros(R, 1, dtype=torch.float64)
    theta = torch.cat([(x2 - x1) / (width - 1), zero, (x1 + x2 - width + 1) / (width - 1),
                       zero, (y2 - y1) / (height - 1), (y1 + y2 - height + 1) / (height - 1)], 1).view(-1, 2, 3)
    grid = F.affine_grid(theta, (R, 1, P, P), align_corners=True)
    out = F.grid_sample(b.expand(R, -1, -1, -1), grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    grad = None
    if dout is not None:
        out.backward(torch.from_numpy(f64(dout)).view(R, P, P, C).permute(0, 3, 1, 2))
        grad = b.grad[0].permute(1, 2, 0).reshape(H * W, C).numpy()
    ix, iy = (grid[:, 0, :, 0] + 1) / 2 * (W - 1), (grid[:, :, 0, 1] + 1) / 2 * (H - 1)
    return out.detach().permute(0, 2, 3, 1).reshape(R * P * P, C).numpy(), grad, ix.numpy(), iy.numpy()


# ------------------------------------------------------------------------------------------------------------------ RoI max pooling
POOL_P = 7
# (R, C): the set of test_roipool at C > 256, and one beyond a pass of the backward's capped grid (48 x 49 x 1024 = 2,408,448 > 8192 x 256)
POOL_SMALL, POOL_WIDE, POOL_BIG = (11, 40), (11, 264), (48, 1024)
assert POOL_BIG[0] * POOL_P * POOL_P * POOL_BIG[1] > POOL_GRID


@functools.lru_cache(maxsize=None)
def pool_rois(R):
    """the RoIs of test_roipool: the whole image, a tiny RoI whose bins share pixels, one partly outside (empty bins); for R > 11 more
    random ones, some of them over the border"""
    rs = np.random.RandomState(4)
    rois = np.zeros((R, 5), np.float32)
    rois[:, 1] = rs.uniform(0, 300, R); rois[:, 2] = rs.uniform(0, 200, R)
    rois[:, 3] = np.minimum(rois[:, 1] + rs.uniform(2, 250, R), 415); rois[:, 4] = np.minimum(rois[:, 2] + rs.uniform(2, 250, R), 319)
    rois[0, 1:] = [0, 0, 415, 319]; rois[1, 1:] = [100.0, 90.0, 103.0, 92.0]
    rois[2, 1:] = [400.0, 300.0, 500.0, 400.0]
    if R > 11:
        rois[11, 1:] = [-30.0, -20.0, 90.0, 70.0]; rois[12, 1:] = [380.0, 10.0, 470.0, 200.0]
    return rois


@functools.lru_cache(maxsize=None)
def pool_feat(C):
    """quarter integers in [-2, 2] (exact in bf16): ties on purpose"""
    H, W = MAP
    return (np.random.RandomState(31 + C).randint(-8, 9, (H * W, C)) * 0.25).astype(np.float32)


@functools.lru_cache(maxsize=None)
def roipool_ref(R, C):
    """oracle.boxes.roi_pool_fwd (exact) in the device's layout -> (out [R P P][C] float32, argmax [R P P][C] int32)"""
    H, W = MAP
    out, arg = OB.roi_pool_fwd(pool_feat(C).reshape(H, W, C).transpose(2, 0, 1), pool_rois(R), POOL_P, 1.0 / 16.0)
    return (np.ascontiguousarray(out.transpose(0, 2, 3, 1)).reshape(-1, C), np.ascontiguousarray(arg.transpose(0, 2, 3, 1)).reshape(-1, C))


def roipool_bwd_ref(dout, arg, H, W, dfeat0):
    """every pooled element adds its gradient to its argmax (none for -1), onto what dfeat held, in float64:
    (dfeat [H W][C], absum, n_terms [H W][C] per element)"""
    C = dout.shape[1]
    ok = arg >= 0
    flat = (arg.astype(np.int64) * C + np.arange(C)[None])[ok]
    g = f64(dout)[ok]
    n = H * W * C
    add = lambda v: np.bincount(flat, weights=v, minlength=n).reshape(H * W, C)
    return f64(dfeat0) + add(g), np.abs(f64(dfeat0)) + add(np.abs(g)), add(np.ones(g.shape)) + 1


def roipool_bwd_f32(dout, arg, H, W, dfeat0):
    C = dout.shape[1]
    ok = torch.from_numpy(arg >= 0)
    flat = torch.from_numpy(arg.astype(np.int64) * C + np.arange(C)[None])[ok]
    df = torch.from_numpy(np.ascontiguousarray(dfeat0, np.float32)).clone().view(-1)
    df.index_add_(0, flat, torch.from_numpy(np.ascontiguousarray(dout, np.float32))[ok])
    return df.view(H * W, C).numpy()


def roipool_bwd_oracle(dout, arg, H, W):
    """oracle.boxes.roi_pool_bwd (float32 accumulation from zero) in the device's layout: the same routing as roipool_bwd_ref"""
    R, C = arg.shape[0] // (POOL_P * POOL_P), dout.shape[1]
    to_rcpp = lambda a: a.reshape(R, POOL_P, POOL_P, C).transpose(0, 3, 1, 2)
    return OB.roi_pool_bwd(to_rcpp(np.asarray(dout, np.float32)), to_rcpp(arg), H, W).transpose(1, 2, 0).reshape(H * W, C)
