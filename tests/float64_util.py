"""helpers shared by the "every kernel instantiation against float64" device tests (tests/test_gpu_k2_float64.py,
tests/test_gpu_k3_float64.py): deterministic inputs, NaN guard bands, and the bookkeeping of (error, yardstick, scale, bar)"""
import torch

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
    return x * torch.tensor(SAMPLE_STD[:N]).view(view) + offset * torch.tensor(SAMPLE_MEAN[:N]).view(view)


def _weight(seed, tag, shape, K_):
    """N(0.5 / K, 1 / K): outputs of unit spread whose mean follows the sample's mean (sum y is not near zero)"""
    return _noise(seed, tag, shape) * (1.0 / K_) ** 0.5 + 0.5 / K_


def bf16_round(t):
    return t.bfloat16().float()


def _nan(n, device, dtype=torch.float32):
    return torch.full((n,), NAN, dtype=dtype, device=device)


class Guarded:
    """`n` elements inside a NaN-filled buffer with `guard` elements in front and behind"""

    def __init__(self, n, guard, device, dtype=torch.float32, fill=None):
        assert guard > 0 and (guard * (2 if dtype == torch.bfloat16 else 4)) % 16 == 0
        self.n, self.guard = n, guard
        self.buf = _nan(n + 2 * guard, device, dtype)
        self.before = self.buf.clone()
        self.t = self.buf[guard:guard + n]
        if fill is not None:
            self.t.copy_(fill.reshape(-1))

    def guards_untouched(self):
        bits = torch.int16 if self.buf.dtype == torch.bfloat16 else torch.int32
        a, b, g = self.buf.view(bits), self.before.view(bits), self.guard
        return bool(torch.equal(a[:g], b[:g])) and bool(torch.equal(a[g + self.n:], b[g + self.n:]))

    def all_nan(self):
        return bool(torch.isnan(self.t).all())


def _wide_slice(t, ld, device):
    """t [.., C] as the LAST C channels of a [.., ld] device buffer whose other channels are NaN"""
    C = t.shape[-1]
    wide = torch.full(t.shape[:-1] + (ld,), NAN, dtype=t.dtype, device=device)
    wide[..., ld - C:] = t.to(device)
    return wide, wide[..., ld - C:]


# ---- bookkeeping ---------------------------------------------------------------------------------------------------------
class Figures:
    """collects (device error, yardstick, scale, bar) per quantity of one case, reports them, then asserts"""

    def __init__(self, name):
        self.name, self.figs, self.fails = name, {}, []

    def require(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def check(self, key, dev, ref, yard, floor, cap=None, bf16_out=False):
        """cap: an absolute bar that holds on top.  bf16_out: per element, 2^-8 |ref| is allowed beside the bar"""
        dev = dev.detach().double().reshape(ref.shape)
        if not bool(torch.isfinite(dev).all()):
            self.fails.append('{}: {} elements were not written (or are not finite)'.format(key, int((~torch.isfinite(dev)).sum())))
            return
        scale = float(ref.abs().max())
        ye = float((yard.double().to(ref.device).reshape(ref.shape) - ref).abs().max())
        lim = 4.0 * ye + floor * scale
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


def _check_stats(fig, stats, ref_y, yard_y, N):
    """slots summed per sample against sum y and sum y^2 of the float64 result"""
    got = stats.t.reshape(N, -1, 2).double().sum(1)
    r = ref_y.reshape(N, -1)
    yd = yard_y.reshape(N, -1)
    ref = torch.stack([r.sum(1), (r * r).sum(1)], 1)
    yard = torch.stack([yd.sum(1), (yd * yd).sum(1)], 1)
    fig.require(not bool(torch.isnan(stats.t).any()), 'stats: a slot was not written')
    fig.require(stats.guards_untouched(), 'stats: the guard bands were written')
    for j, key in enumerate(('stat_sum', 'stat_sq')):
        fig.check(key, got[:, j], ref[:, j], yard[:, j], FLOOR_RED)
    cap_sum = float(((got[:, 0] - ref[:, 0]).abs() / r.abs().sum(1)).max())
    cap_sq = float((got[:, 1] - ref[:, 1]).abs().max() / ref[:, 1].abs().max())
    fig.figs.update(stat_sum_vs_abs=cap_sum, stat_sq_rel=cap_sq)
    fig.require(cap_sum < CAP_STAT and cap_sq < CAP_STAT, 'stats: above the existing 1e-5 bars ({:.3e}, {:.3e})'.format(cap_sum, cap_sq))


def _engine():
    from segmentation3d import _engine as E
    E.lib()
    return E
