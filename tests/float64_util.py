"""helpers shared by the "every kernel instantiation against float64" device tests (tests/test_gpu_k2_float64.py,
tests/test_gpu_k3_float64.py, tests/test_gpu_thin_float64.py, tests/test_gpu_wino_float64.py, tests/test_gpu_direct_float64.py): deterministic
inputs, the float64 references (3x3x3, stride-2 2x2x2, 1x1x1), NaN guard bands, and the bookkeeping of (error, yardstick, scale, bar)"""
import torch
import torch.nn.functional as F

from gpu_util import report
from oracle import detgen

NAN = float('nan')
FLOOR_EW, FLOOR_RED = 2e-6, 1e-5
CAP_STAT = 1e-5
BF16_REL = 2.0 ** -8
SAMPLE_MEAN = (0.7, -0.4, 1.3)
SAMPLE_STD = (2.0, 1.5, 2.5)
_BASE_LEN = (1 << 20) - 3


# ---- inputs --------------------------------------------------------------------------------------------------------------
def _noise(seed, tag, shape):
    """float32 N(0, 1) from oracle.detgen; large tensors are rotations of ONE 2^20-value draw (detgen costs ~0.15 s per million)"""
    n = 1
    for s in shape:
        n *= s
    if n <= _BASE_LEN:
        return torch.from_numpy(detgen.normal(seed, tag, tuple(shape)))
    base = torch.from_numpy(detgen.normal(seed, tag, (_BASE_LEN,)))
    parts = [torch.roll(base, 7919 * k) for k in range((n + _BASE_LEN - 1) // _BASE_LEN)]
    return torch.cat(parts)[:n].reshape(tuple(shape))


def _activation(seed, tag, N, dims, C, offset=1.0):
    """[N, d, h, w, C] with a different mean and spread per sample"""
    x = _noise(seed, tag, (N,) + tuple(dims) + (C,))
    view = (N, 1, 1, 1, 1)
    std = torch.tensor([SAMPLE_STD[n % 3] for n in range(N)]).view(view)           # (the three pairs cycle for N > 3)
    return x * std + offset * torch.tensor([SAMPLE_MEAN[n % 3] for n in range(N)]).view(view)


def _weight(seed, tag, shape, K_):
    """N(0.5 / K, 1 / K): outputs of unit spread whose mean follows the sample's mean (sum y is not near zero)"""
    return _noise(seed, tag, shape) * (1.0 / K_) ** 0.5 + 0.5 / K_


def bf16_round(t):
    return t.bfloat16().float()


def _nan(n, device, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype, device=device)


INT_SENTINEL = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x5A5A5A5A, torch.uint8: 0x5A}   # the fill of an integer buffer
_BITS = {torch.bfloat16: torch.int16, torch.float32: torch.int32}                              # (an integer buffer is its own)


class Guarded:
    """`n` elements inside a NaN-filled buffer with `guard` elements in front and behind; an integer buffer (int64, int32, uint8)
    is filled with the fixed pattern INT_SENTINEL instead.  `shift` moves the n elements that many elements past the 16-byte
    boundary they otherwise start on (the rear guard keeps its `guard` elements)"""

    def __init__(self, n, guard, device, dtype=torch.float32, fill=None, shift=0):
        assert guard > 0 and (guard * torch.empty((), dtype=dtype).element_size()) % 16 == 0 and shift >= 0
        self.n, self.guard, self.front = n, guard, guard + shift
        if dtype in INT_SENTINEL:
            self.buf = torch.full((n + 2 * guard + shift,), INT_SENTINEL[dtype], dtype=dtype, device=device)
        else:
            self.buf = _nan(n + 2 * guard + shift, device, dtype)
        self.before = self.buf.clone()
        self.t = self.buf[self.front:self.front + n]
        if fill is not None:
            self.t.copy_(fill.reshape(-1))

    def guards_untouched(self):
        bits = _BITS.get(self.buf.dtype, self.buf.dtype)
        a, b, g = self.buf.view(bits), self.before.view(bits), self.front
        return bool(torch.equal(a[:g], b[:g])) and bool(torch.equal(a[g + self.n:], b[g + self.n:]))

    def all_nan(self):
        """every element still holds its fill (NaN, or the integer pattern)"""
        if self.buf.dtype in INT_SENTINEL:
            return bool((self.t == INT_SENTINEL[self.buf.dtype]).all())
        return bool(torch.isnan(self.t).all())

    def written(self):
        """no element still holds its fill: finite for a float buffer, not the pattern for an integer one"""
        if self.buf.dtype in INT_SENTINEL:
            return bool((self.t != INT_SENTINEL[self.buf.dtype]).all())
        return bool(torch.isfinite(self.t).all())


def _wide_slice(t, ld, device):
    """t [.., C] as the LAST C channels of a [.., ld] device buffer whose other channels are NaN"""
    C = t.shape[-1]
    wide = torch.full(t.shape[:-1] + (ld,), NAN, dtype=t.dtype, device=device)
    wide[..., ld - C:] = t.to(device)
    return wide, wide[..., ld - C:]


# ---- float64 references of the 3x3x3 convolution (on the device the operands are on) -----------------------------------------
TAPS = [(kz, ky, kx) for kz in range(3) for ky in range(3) for kx in range(3)]


def _pad(x):
    return F.pad(x, (0, 0, 1, 1, 1, 1, 1, 1))            # [N, D + 2, H + 2, W + 2, C], zeros


def _conv_def(x, w):
    """x [N, D, H, W, Ci], w [Co, Ci, 3, 3, 3], both float64"""
    N, D, H, W, Ci = x.shape
    xp = _pad(x)
    out = torch.zeros((N * D * H * W, w.shape[0]), dtype=torch.float64, device=x.device)
    for (kz, ky, kx) in TAPS:
        out += xp[:, kz:kz + D, ky:ky + H, kx:kx + W, :].reshape(-1, Ci) @ w[:, :, kz, ky, kx].t()
    return out.reshape(N, D, H, W, w.shape[0])


def _blocked(t, blocks):
    """[V, C] -> [blocks, ceil(V / blocks), C], rows of zeros behind the last one"""
    rows = (t.shape[0] + blocks - 1) // blocks
    return F.pad(t, (0, 0, 0, rows * blocks - t.shape[0])).reshape(blocks, rows, t.shape[1])


def _wgrad_def(x, dy, blocks=1):
    """x [N, D, H, W, Ci], dy [N, D, H, W, Co] -> dw [Co, Ci, 27].  blocks > 1: every product over the voxels as that many batched
    products summed in float64 (for 10^6 voxels and a handful of channels: one skinny product runs in a single workgroup)"""
    N, D, H, W, Ci = x.shape
    xp = _pad(x)
    if blocks > 1:
        dyt = _blocked(dy.reshape(-1, dy.shape[-1]), blocks).transpose(1, 2)
        return torch.stack([(dyt @ _blocked(xp[:, kz:kz + D, ky:ky + H, kx:kx + W, :].reshape(-1, Ci), blocks)).sum(0)
                            for (kz, ky, kx) in TAPS], 2)
    dyt = dy.reshape(-1, dy.shape[-1]).t().contiguous()
    return torch.stack([dyt @ xp[:, kz:kz + D, ky:ky + H, kx:kx + W, :].reshape(-1, Ci) for (kz, ky, kx) in TAPS], 2)


# ---- float64 references of the stride-2 2x2x2 operations (einsums over the 2^3 cells) and of the 1x1x1 convolution ------------------
def _k2_cells(x):
    """[N, 2D, 2H, 2W, C] -> [N, D, 2, H, 2, W, 2, C]: the 2^3 cell of every coarse voxel"""
    N, D2, H2, W2, C = x.shape
    return x.reshape(N, D2 // 2, 2, H2 // 2, 2, W2 // 2, 2, C)


def _k2_gather_def(x, w):
    """y[v][b] = sum_{t, a} x[2v + t][a] w[b][a][t].  x [N, 2D, 2H, 2W, A], w [B, A, 2, 2, 2] -> [N, D, H, W, B]"""
    return torch.einsum('nzaybxcq,oqabc->nzyxo', _k2_cells(x), w)


def _k2_scatter_def(x, w):
    """y[2i + t][b] = sum_a x[i][a] w[a][b][t].  x [N, D, H, W, A], w [A, B, 2, 2, 2] -> [N, 2D, 2H, 2W, B]"""
    N, D, H, W, _ = x.shape
    return torch.einsum('nzyxq,qoabc->nzaybxco', x, w).reshape(N, 2 * D, 2 * H, 2 * W, w.shape[1])


def _k2_wgrad_def(P, Q):
    """dW(a, b, t) = sum_v P[2v + t][a] Q[v][b].  P [N, 2D, 2H, 2W, CA], Q [N, D, H, W, CB] -> [CA, CB, 8].  The stride-2 conv's
    weight gradient with P = x, Q = dy; the transposed conv's with P = dy, Q = x"""
    return torch.einsum('nzaybxcp,nzyxq->pqabc', _k2_cells(P), Q).reshape(P.shape[-1], Q.shape[-1], 8)


def _k1_def(x, w):
    """x [N, D, H, W, Ci], w [Co, Ci] -> [N, D, H, W, Co]"""
    return (x.reshape(-1, x.shape[-1]) @ w.t()).reshape(x.shape[:-1] + (w.shape[0],))


def _k1_wgrad_def(x, dy):
    """x [N, D, H, W, Ci], dy [N, D, H, W, Co] -> dw [Co, Ci]"""
    return dy.reshape(-1, dy.shape[-1]).t() @ x.reshape(-1, x.shape[-1])


# ---- the Winograd forms of the same operations, restated from the header comments of csrc/conv_wino.hip and csrc/conv_wino2d.hip,
# in the dtype of their operands (fp32 on the CPU: the second yardstick of tests/test_gpu_wino_float64.py; float64: the same sums
# in another order, which tests/test_wino_variants.py holds against _conv_def / _wgrad_def) ------------------------------------------
def _bt(d0, d1, d2, d3):
    """B^T d of F(2, 3) and of F(3, 2): (d0 - d2, d1 + d2, d2 - d1, d1 - d3)"""
    return d0 - d2, d1 + d2, d2 - d1, d1 - d3


def _x_points(xp, W):
    """the four x points of every output pair: [N, D + 2, H + 2, W / 2, C] each"""
    return _bt(*[xp[:, :, :, k:k + W - 1:2] for k in range(4)])


def _yx_points(xp, H, W):
    """V = B^T d B of every 4 x 4 patch: V[py][px] of [N, D + 2, H / 2, W / 2, C]"""
    return [_x_points(r, W) for r in _bt(*[xp[:, :, k:k + H - 1:2] for k in range(4)])]


def _g3(g0, g1, g2):
    """G g of a 3-tap filter: (g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2)"""
    return g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2


def _wino_f23_conv(x, w):
    """F(2, 3) along x.  x [N, D, H, W, Ci], w [Co, Ci, 3, 3, 3] -> [N, D, H, W, Co]; W even"""
    N, D, H, W, Ci = x.shape
    Dp = _x_points(_pad(x), W)
    U = _g3(w[..., 0], w[..., 1], w[..., 2])                               # [Co, Ci, kz, ky] per point
    M = []
    for p in range(4):
        m = torch.zeros((N * D * H * (W // 2), w.shape[0]), dtype=x.dtype, device=x.device)
        for kz in range(3):
            for ky in range(3):
                m += Dp[p][:, kz:kz + D, ky:ky + H].reshape(-1, Ci) @ U[p][:, :, kz, ky].t()
        M.append(m.reshape(N, D, H, W // 2, -1))
    return torch.stack([M[0] + M[1] + M[2], M[1] - M[2] - M[3]], 4).reshape(N, D, H, W, -1)


def _wino_f2x2_conv(x, w):
    """F(2x2, 3x3) over (y, x): V = B^T d B, U = G g G^T, M = sum_{kz, ci} U (.) V, Y = A^T M A; H and W even"""
    N, D, H, W, Ci = x.shape
    V = _yx_points(_pad(x), H, W)
    Ur = _g3(w[:, :, :, 0], w[:, :, :, 1], w[:, :, :, 2])                   # rows: [Co, Ci, kz, kx]
    M = [[None] * 4 for _ in range(4)]
    for py in range(4):
        U = _g3(Ur[py][..., 0], Ur[py][..., 1], Ur[py][..., 2])            # [Co, Ci, kz] per px
        for px in range(4):
            m = torch.zeros((N * D * (H // 2) * (W // 2), w.shape[0]), dtype=x.dtype, device=x.device)
            for kz in range(3):
                m += V[py][px][:, kz:kz + D].reshape(-1, Ci) @ U[px][:, :, kz].t()
            M[py][px] = m.reshape(N, D, H // 2, W // 2, -1)
    at = lambda m: (m[0] + m[1] + m[2], m[1] - m[2] - m[3])               # A^T = [1 1 1 0; 0 1 -1 -1]
    rows = at([torch.stack(at(M[py]), 4) for py in range(4)])             # each [N, D, H / 2, W / 2, 2, Co]
    return torch.stack(rows, 3).reshape(N, D, H, W, -1)


def _wino_f32_wgrad(x, dy):
    """F(3, 2) along x: E = (g0, g0 + g1, g0 - g1, g1) of a dy pair, M_p = sum_pairs D_p (x) E_p,
    dW[kx = 0] = M0 + (M1 + M2) / 2, [1] = (M1 - M2) / 2, [2] = (M1 + M2) / 2 - M3 -> [Co, Ci, 27]"""
    N, D, H, W, Ci = x.shape
    Dp = _x_points(_pad(x), W)
    g0, g1 = dy[:, :, :, 0::2], dy[:, :, :, 1::2]
    E = [e.reshape(-1, dy.shape[-1]).t().contiguous() for e in (g0, g0 + g1, g0 - g1, g1)]
    taps = []
    for kz in range(3):
        for ky in range(3):
            M = [E[p] @ Dp[p][:, kz:kz + D, ky:ky + H].reshape(-1, Ci) for p in range(4)]
            hs, hd = (M[1] + M[2]) * 0.5, (M[1] - M[2]) * 0.5
            taps += [M[0] + hs, hd, hs - M[3]]
    return torch.stack(taps, 2)


def _wino_f3x3_wgrad(x, dy):
    """F(3x3, 2x2) over (y, x): V = B^T d B, E = G' g G'^T with G' = [1 0; 1 1; 1 -1; 0 1], M_p = sum_quads V_p (x) E_p,
    dW[kz] = A'^T M A' with A'^T = [1 1/2 1/2 0; 0 1/2 -1/2 0; 0 1/2 1/2 -1] -> [Co, Ci, 27]"""
    N, D, H, W, Ci = x.shape
    V = _yx_points(_pad(x), H, W)
    gp = lambda a, b: (a, a + b, a - b, b)
    rows = gp(dy[:, :, 0::2], dy[:, :, 1::2])
    E = [[e.reshape(-1, dy.shape[-1]).t().contiguous() for e in gp(r[:, :, :, 0::2], r[:, :, :, 1::2])] for r in rows]
    at = lambda m: (m[0] + (m[1] + m[2]) * 0.5, (m[1] - m[2]) * 0.5, (m[1] + m[2]) * 0.5 - m[3])
    taps = []
    for kz in range(3):
        M = [[E[py][px] @ V[py][px][:, kz:kz + D].reshape(-1, Ci) for px in range(4)] for py in range(4)]
        for r in at([torch.stack(at(M[py]), 2) for py in range(4)]):       # ky rows of [Co, Ci, kx]
            taps += [r[:, :, 0], r[:, :, 1], r[:, :, 2]]
    return torch.stack(taps, 2)


# ---- bookkeeping ---------------------------------------------------------------------------------------------------------
class Figures:
    """collects (device error, yardstick, scale, bar) per quantity of one case, reports them, then asserts"""

    def __init__(self, name):
        self.name, self.figs, self.fails = name, {}, []

    def require(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def check(self, key, dev, ref, yard, floor, cap=None, bf16_out=False, yardstick=True):
        """bar = min(4 * yardstick + floor * scale, cap).  yardstick = False drops the first term -- for a kernel whose error is
        not the yardstick's (an operand carried as a bf16 hi + lo pair) the bar is `cap` alone.  bf16_out: per element,
        2^-8 |ref| is allowed beside the bar.  `yard` may be a tuple of fp32 results: the yardstick is the largest of their errors"""
        dev = dev.detach().double().reshape(ref.shape)
        if not bool(torch.isfinite(dev).all()):
            self.fails.append('{}: {} elements were not written (or are not finite)'.format(key, int((~torch.isfinite(dev)).sum())))
            return
        scale = float(ref.abs().max())
        yards = yard if isinstance(yard, (tuple, list)) else (yard,)
        ye = max(float((y.double().to(ref.device).reshape(ref.shape) - ref).abs().max()) for y in yards)
        lim = 4.0 * ye + floor * scale if yardstick else cap
        if not ye <= 1e-4 * scale:       # (a test of the test: the fp32 restatement and the float64 formula are the same operation)
            self.fails.append('{}: the fp32 yardstick is {:.3e} away from the float64 reference (scale {:.3e})'.format(key, ye, scale))
        if cap is not None:
            lim = min(lim, cap)
        d = (dev - ref).abs()
        if bf16_out:
            d = d - BF16_REL * ref.abs()
        err = float(d.max())
        self.figs.update({key + '_err': err, key + '_yard': ye, key + '_scale': scale, key + '_bar': lim})
        if not err <= lim:
            self.fails.append('{}: err {:.3e} > bar {:.3e} (yardstick {:.3e}, scale {:.3e})'.format(key, err, lim, ye, scale))

    def done(self):
        report(self.name, **self.figs)
        assert not self.fails, '{}: {}'.format(self.name, '; '.join(self.fails))


def _check_stats(fig, stats, ref_y, yard_y, N, cap=CAP_STAT, yardstick=True):
    """slots summed per sample against sum y and sum y^2 of the float64 result.  yardstick = False (as in Figures.check): the
    bars are `cap` of sum |y| and of sum y^2 alone"""
    got = stats.t.reshape(N, -1, 2).double().sum(1)
    r = ref_y.reshape(N, -1)
    ref = torch.stack([r.sum(1), (r * r).sum(1)], 1)
    yards = []                                         # (yard_y may be a tuple of fp32 results, as in Figures.check)
    for yd in (yard_y if isinstance(yard_y, (tuple, list)) else (yard_y,)):
        yd = yd.reshape(N, -1)
        yards.append(torch.stack([yd.sum(1), (yd * yd).sum(1)], 1))
    fig.require(not bool(torch.isnan(stats.t).any()), 'stats: a slot was not written')
    fig.require(stats.guards_untouched(), 'stats: the guard bands were written')
    norm = (float(r.abs().sum(1).max()), float(ref[:, 1].abs().max()))
    for j, key in enumerate(('stat_sum', 'stat_sq')):
        fig.check(key, got[:, j], ref[:, j], tuple(y[:, j] for y in yards), FLOOR_RED, cap=None if yardstick else cap * norm[j],
                  yardstick=yardstick)
    cap_sum = float(((got[:, 0] - ref[:, 0]).abs() / r.abs().sum(1)).max())
    cap_sq = float((got[:, 1] - ref[:, 1]).abs().max() / ref[:, 1].abs().max())
    fig.figs.update(stat_sum_vs_abs=cap_sum, stat_sq_rel=cap_sq)
    fig.require(cap_sum < cap and cap_sq < cap, 'stats: above the existing {:.0e} bars ({:.3e}, {:.3e})'.format(cap, cap_sum, cap_sq))


def _engine():
    from segmentation3d import _engine as E
    E.lib()
    return E
