"""Every GroupNorm kernel path of csrc/gn.hip, driven through the C ABI, against a plain float64 reference.

Layout: all tensors are NDHWC with the spatial extent flattened, i.e. [N, S, C] (the entries take N, S, C, not a 5-D shape).

Reference: stock F.group_norm (one group) in float64 with float64 autograd for dy (= dx of the unit), dgamma, dbeta, dres and
dbias (dbias from a zero bias added in front of the norm); the intermediate quantities of gn.hip's header comment (mean, rstd,
A = sum g, B = sum g*xhat, X = sum xhat per (n, c), s1, s2) are restated directly in float64 so that every stage is checked
where it is produced.

Bars: nothing is pinned to what the kernels give.  Each case also runs the SAME stock computation in fp32 on the CPU (the
yardstick) and a kernel passes when  err <= 4 * yardstick + floor * scale,  scale = max|ref| of the quantity, floor = 2e-6
for element-wise outputs and 1e-5 for reduced quantities (the floors of the convolution tests for values / statistics sums).
The bars of test_fused_conv_gn_act hold on top (`cap`).  dbias is a difference of large terms and is measured against the
float64 magnitude  sum_n rstd_n (|gamma_c A| + S |s1_n| + |s2_n X|).  bf16-stored outputs: (2^-8 + 2e-5) * scale against float64
on the bf16-rounded operands.

ReLU ties: a voxel whose float64 output lies within 8 fp32 ulps of max|out| around zero may take the other branch on the device.
Only such voxels may differ in [out > 0]; the gradient reference takes the device's decision there (read off dres = g, which is
non-zero exactly where the device kept the gradient) and its own everywhere else; the band may hold at most 1e-3 of a case.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

from gpu_util import report
from oracle import detgen

pytestmark = pytest.mark.gpu

EPS = 1e-5
NAN = float('nan')
FLOOR_EW = 2e-6          # element-wise outputs: out, dy, dres
FLOOR_RED = 1e-5         # reduced quantities: mean, rstd, part sums, abx, s12, dgamma, dbeta (and dbias against its magnitude)
BF16_BAR = 2.0 ** -8 + 2e-5
TIE_BAND = 8 * 2.0 ** -24
TIE_SHARE = 1e-3
# the bars test_fused_conv_gn_act holds today (out absolute, the rest relative to max|ref|)
CAP_OUT, CAP_GRAD, CAP_DRES = 1e-4, 2e-4, 1e-5
SAMPLE_MEAN = (0.7, -0.4, 1.3)
SAMPLE_STD = (2.0, 1.5, 2.5)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def _fields(seed, tag, N, S, C, count):
    """`count` [N, S, C] float32 N(0, 1) fields from oracle.detgen.  Large cases draw ONE sample-sized field and take the other
    samples / fields as rotations of it by distinct offsets (detgen costs ~0.15 s per million values)"""
    L = S * C
    if N * L * count <= (1 << 21):
        return [torch.from_numpy(detgen.normal(seed + j, tag, (N, S, C))) for j in range(count)]
    base = torch.from_numpy(detgen.normal(seed, tag, (L,)))
    step = L // (N * count + 1)
    assert step >= 1024
    return [torch.stack([torch.roll(base, (j * N + n) * step + 7 * (j * N + n)) for n in range(N)]).reshape(N, S, C)
            for j in range(count)]


def make_inputs(tag, N, S, C, half_negative=False):
    """y with a different mean and spread per sample, gamma ~ 1 +- 0.3, beta, residual, upstream gradient"""
    y, res, dout = _fields(700, tag, N, S, C, 3)
    y = y * torch.tensor(SAMPLE_STD[:N]).view(N, 1, 1) + torch.tensor(SAMPLE_MEAN[:N]).view(N, 1, 1)
    gamma = 1.0 + 0.3 * torch.from_numpy(detgen.normal(710, tag + '/gamma', (C,)))
    beta = 0.3 * torch.from_numpy(detgen.normal(711, tag + '/beta', (C,)))
    if half_negative:
        gamma = torch.where(torch.arange(C) % 2 == 0, gamma, -gamma)      # both signs of gamma, outputs centred on zero
        beta = 0.1 * beta
    return y, gamma, beta, res, dout


def bf16_round(t):
    return t.bfloat16().float()


# ---- float64 reference (runs on the CPU alone; dtype=torch.float32 gives the yardstick) -----------------------------------
def ref_gn(y, gamma, beta, res, relu, dout=None, mask=None, dtype=torch.float64):
    """stock F.group_norm(y, 1, gamma, beta, 1e-5) (+ res) (+ ReLU) on [N, S, C] tensors and its autograd gradients.
    mask: the [out > 0] decision to differentiate through (default: the computation's own)"""
    N, S, C = y.shape
    grad = dout is not None
    leaf = lambda t: t.detach().to(dtype, copy=True).requires_grad_(grad)      # never a view of the caller's tensor
    yl, ga, be = leaf(y), leaf(gamma), leaf(beta)
    bz = torch.zeros(C, dtype=dtype, requires_grad=grad)
    pre = F.group_norm((yl + bz).permute(0, 2, 1), 1, ga, be, EPS).permute(0, 2, 1)
    rl = None
    if res is not None:
        rl = leaf(res)
        pre = pre + rl
    if relu:
        out = F.relu(pre) if mask is None else pre * mask.to(dtype)
    else:
        out = pre
    r = dict(out=out.detach().contiguous(), pre=pre.detach().contiguous())     # [N, S, C] memory order, like the inputs
    if grad:
        gr = torch.autograd.grad(out, [yl, ga, be, bz] + ([rl] if rl is not None else []), dout.to(dtype))
        r.update(dy=gr[0], dgamma=gr[1], dbeta=gr[2], dbias=gr[3])
        if rl is not None:
            r['dres_autograd'] = gr[4]
    return r


def ref_stats(y2d, dtype=torch.float64):
    """[N, M] -> sum, sum of squares, mean, rstd (two-pass variance)"""
    x = y2d.to(dtype)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return dict(sum=x.sum(1), sumsq=(x * x).sum(1), mean=mean, rstd=(var + EPS).rsqrt())


def ref_stages(y, gamma, dout, mask, dtype=torch.float64):
    """the intermediate quantities of the backward pass, written out directly"""
    N, S, C = y.shape
    st = ref_stats(y.reshape(N, -1), dtype)
    mean, rstd = st['mean'], st['rstd']
    xhat = (y.to(dtype) - mean.view(N, 1, 1)) * rstd.view(N, 1, 1)
    g = dout.to(dtype) if mask is None else dout.to(dtype) * mask.to(dtype)
    ga = gamma.to(dtype)
    A, B, X = g.sum(1), (g * xhat).sum(1), xhat.sum(1)
    M = float(S * C)
    s1, s2 = (A * ga).sum(1) / M, (B * ga).sum(1) / M
    mag = (rstd[:, None] * ((ga * A).abs() + S * s1.abs()[:, None] + (s2[:, None] * X).abs())).sum(0)
    return dict(mean=mean, rstd=rstd, A=A, B=B, X=X, s12=torch.stack([s1, s2], 1), g=g, dbias_mag=mag)


def tie_band(pre64, out64):
    """voxels whose float64 value in front of the ReLU lies within 8 fp32 ulps of max|out| around zero"""
    return pre64.abs() <= TIE_BAND * float(out64.abs().max())


# ---- bookkeeping ----------------------------------------------------------------------------------------------------------
class Figures:
    """collects (device error, yardstick, scale, bar) per quantity of one case, reports them, then asserts"""

    def __init__(self, name):
        self.name, self.figs, self.fails = name, {}, []

    def check(self, key, dev, ref, yard, floor, cap=None, denom=None, bar=None):
        dev = dev.detach().double().cpu().reshape(ref.shape)
        ref = ref.double()
        if not bool(torch.isfinite(dev).all()):
            self.fails.append('{}: {} elements were not written (or are not finite)'.format(key, int((~torch.isfinite(dev)).sum())))
            return
        d, scale = (dev - ref).abs(), float(ref.abs().max())
        if denom is not None:        # error measured element by element against a given magnitude
            err = float((d / denom).max())
            ye = float(((yard.double().reshape(ref.shape) - ref).abs() / denom).max()) if yard is not None else 0.0
            lim, scale = 4.0 * ye + floor, float(denom.max())
        else:
            err = float(d.max())
            ye = float((yard.double().reshape(ref.shape) - ref).abs().max()) if yard is not None else 0.0
            lim = 4.0 * ye + floor * scale
        if bar is not None:
            lim = bar
        self.figs.update({key + '_err': err, key + '_yard': ye, key + '_scale': scale, key + '_bar': lim})
        if not err <= lim:
            self.fails.append('{}: err {:.3e} > bar {:.3e} (yardstick {:.3e}, scale {:.3e})'.format(key, err, lim, ye, scale))
        if cap is not None and not float(d.max()) < cap:
            self.fails.append('{}: err {:.3e} is above the existing bar {:.3e}'.format(key, float(d.max()), cap))

    def note(self, **kw):
        self.figs.update(kw)

    def done(self):
        report(self.name, **self.figs)
        assert not self.fails, '{}: {}'.format(self.name, '; '.join(self.fails))


def _nan(shape, device, dtype=torch.float32):
    return torch.full(tuple(shape), NAN, dtype=dtype, device=device)


def _vpb(S):
    return min(max((S + 127) // 128, 32), 2048)


def _wide(t, device, seed):
    """the [N, S, C] tensor as the channel slice 4 : 4 + C of a wider [N, S, C + 8] buffer whose other columns hold noise"""
    N, S, C = t.shape
    wide = torch.from_numpy(detgen.normal(seed, 'wide', (N, S, C + 8))).to(t.dtype)
    wide[..., 4:4 + C] = t
    wide = wide.to(device)
    return wide, wide[..., 4:4 + C]


# ---- device pipelines ------------------------------------------------------------------------------------------------------
def dev_stats(E, y2d):
    N, M = y2d.shape
    cnt = E.query('seg3d_gn_stats_count', M)
    assert cnt == (M + 16383) // 16384
    part = _nan((N, cnt, 2), y2d.device)
    mr = _nan((N, 2), y2d.device)
    E.call('seg3d_gn_stats_partial', E.ptr(y2d), E.ptr(part), N, M, E.stream_ptr())
    E.call('seg3d_gn_stats_finalize', E.ptr(part), E.ptr(mr), N, cnt, M, EPS, E.stream_ptr())
    return part, mr


def dev_apply(E, y, mr, gamma, beta, res, relu, out, ld=0, mixed=None):
    N, S, C = y.shape
    if mixed is None:
        E.call('seg3d_gn_apply', E.ptr(y), E.ptr(mr), E.ptr(gamma), E.ptr(beta), E.ptr(res), E.ptr(out), N, S, C, int(relu), ld,
               E.stream_ptr())
    else:
        res_bf, out_bf, y_bf = mixed
        E.call('seg3d_gn_apply_mixed', E.ptr(y), E.ptr(mr), E.ptr(gamma), E.ptr(beta), E.ptr(res), E.ptr(out), N, S, C, int(relu),
               ld, int(res_bf), int(out_bf), int(y_bf), E.stream_ptr())
    return out


def dev_reduce(E, dout, ldd, out, y, mr, gamma, beta, relu, y_bf=None):
    N, S, C = y.shape
    nblk = E.query('seg3d_gn_bwd_blocks', S)
    assert nblk == (S + _vpb(S) - 1) // _vpb(S)
    part = _nan((N, nblk, C, 3), y.device)
    if y_bf is None:
        E.call('seg3d_gn_bwd_reduce', E.ptr(dout), E.ptr(out), E.ptr(y), E.ptr(mr), E.ptr(gamma), E.ptr(beta), E.ptr(part), N, S, C,
               int(relu), ldd, E.stream_ptr())
    else:
        E.call('seg3d_gn_bwd_reduce_bf16', E.ptr(dout), E.ptr(out), E.ptr(y), E.ptr(mr), E.ptr(gamma), E.ptr(beta), E.ptr(part), N,
               S, C, int(relu), ldd, int(y_bf), E.stream_ptr())
    return part


def dev_finalize(E, part, gamma, mr, N, S, C, acc_mask=0, dests=None, want_dbias=True, ticket=None):
    dev = part.device
    abx, s12 = _nan((N, C, 3), dev), _nan((N, 2), dev)
    dgamma, dbeta, dbias = dests if dests is not None else (_nan((C,), dev), _nan((C,), dev), _nan((C,), dev))
    if not want_dbias:
        dbias = None
    if ticket is None:
        E.call('seg3d_gn_bwd_finalize', E.ptr(part), E.ptr(gamma), E.ptr(mr), E.ptr(abx), E.ptr(s12), E.ptr(dgamma), E.ptr(dbeta),
               E.ptr(dbias), N, S, C, acc_mask, E.stream_ptr())
    else:
        E.call('seg3d_gn_bwd_finalize_fused', E.ptr(part), E.ptr(gamma), E.ptr(mr), E.ptr(abx), E.ptr(s12), E.ptr(dgamma),
               E.ptr(dbeta), E.ptr(dbias), E.ptr(ticket), N, S, C, acc_mask, E.stream_ptr())
    return abx, s12, dgamma, dbeta, dbias


def dev_bwd_apply(E, dout, ldd, out, y, mr, s12, gamma, beta, relu, want_dres=True, bf16=None):
    N, S, C = y.shape
    dres = _nan((N, S, C), y.device) if want_dres else None
    if bf16 is None:
        dy = _nan((N, S, C), y.device)
        E.call('seg3d_gn_bwd_apply', E.ptr(dout), E.ptr(out), E.ptr(y), E.ptr(mr), E.ptr(s12), E.ptr(gamma), E.ptr(beta), E.ptr(dy),
               E.ptr(dres), N, S, C, int(relu), ldd, E.stream_ptr())
    else:
        dy_bf, y_bf = bf16
        dy = _nan((N, S, C), y.device, torch.bfloat16 if dy_bf else torch.float32)
        E.call('seg3d_gn_bwd_apply_bf16', E.ptr(dout), E.ptr(out), E.ptr(y), E.ptr(mr), E.ptr(s12), E.ptr(gamma), E.ptr(beta),
               E.ptr(dy), E.ptr(dres), N, S, C, int(relu), ldd, int(dy_bf), int(y_bf), E.stream_ptr())
    return dy, dres


def device_decision(fig, dres_dev, dout, fwd, ref_mask):
    """the [out > 0] decision the device took, read off dres = g (dout is never exactly zero here); asserts that it differs from
    the reference's only inside the tie band and that the band is thin; returns the mask for the gradient reference"""
    band = tie_band(fwd['pre'], fwd['out'])
    share = float(band.double().mean())
    assert bool((dout != 0).all())
    dec = dres_dev.detach().cpu() != 0
    flips_outside = int(((dec != ref_mask) & ~band).sum())
    fig.note(tie_share=share, tie_flips=float(((dec != ref_mask) & band).sum()), flips_outside_band=float(flips_outside))
    assert share <= TIE_SHARE, share
    assert flips_outside == 0, '{} voxels outside the tie band took the other ReLU branch'.format(flips_outside)
    return torch.where(band, dec, ref_mask)


# ---- 1. statistics: partial + finalize --------------------------------------------------------------------------------------
STATS_M = [(525, '2x5x3x5x7_scalar_loop'), (120, '1x4x2x3x5_below_1024'), (16384, '2x16x8x8x16_one_chunk'),
           (16380, 'chunk_minus_4'), (16388, 'chunk_plus_4'), (3 * 16384 + 20, 'three_chunks_plus_20'), (16387, 'chunk_plus_3_scalar')]


@pytest.mark.parametrize('M,what', STATS_M, ids=[w for _, w in STATS_M])
def test_stats_partial_and_finalize(hip_device, M, what):
    """flat [3][M] buffers (the entry takes N, M): per-element size M of the listed shapes, a different mean per sample"""
    from segmentation3d import _engine as E
    N = 3
    y = torch.from_numpy(detgen.normal(720, 'stats/' + what, (N, M)))
    y = y * torch.tensor(SAMPLE_STD).view(N, 1) + torch.tensor(SAMPLE_MEAN).view(N, 1)
    ref, yard = ref_stats(y), ref_stats(y, torch.float32)
    part, mr = dev_stats(E, y.to(hip_device))
    fig = Figures('gn64_stats_{}'.format(what))
    assert bool(torch.isfinite(part).all())
    sums = part.double().sum(1).cpu()
    fig.check('sum', sums[:, 0], ref['sum'], yard['sum'], FLOOR_RED)
    fig.check('sumsq', sums[:, 1], ref['sumsq'], yard['sumsq'], FLOOR_RED)
    fig.check('mean', mr[:, 0], ref['mean'], yard['mean'], FLOOR_RED)
    fig.check('rstd', mr[:, 1], ref['rstd'], yard['rstd'], FLOOR_RED)
    fig.done()


# ---- 2. statistics finalize on synthetic partials ----------------------------------------------------------------------------
@pytest.mark.parametrize('count', [1, 255, 256, 257, 1023, 1024, 1025, 2049, 7001])
def test_stats_finalize_synthetic_partials(hip_device, count):
    """partials built on the host: (sum, sum of squares) of 16384-element chunks of a N(mean_n, 1) sample, as float64 values
    rounded to fp32.  The kernel adds them in float64, so mean and rstd are exact up to their final rounding"""
    from segmentation3d import _engine as E
    N, chunk = 3, 16384
    M = count * chunk
    z = torch.from_numpy(detgen.normal(730, 'synth/{}'.format(count), (N, count, 2))).double()
    mu = torch.tensor(SAMPLE_MEAN, dtype=torch.float64).view(N, 1)
    s = chunk * mu + 128.0 * z[..., 0]
    ss = chunk * (1.0 + mu * mu) + 180.0 * z[..., 1] + 2.0 * mu * 128.0 * z[..., 0]
    part = torch.stack([s, ss], 2).float()                 # [N, count, 2]
    p64 = part.double()
    mean = p64[..., 0].sum(1) / M
    var = p64[..., 1].sum(1) / M - mean * mean
    assert float(var.min()) > 0.5                           # well conditioned: the check is about the summation, not cancellation
    rstd = (var + EPS).rsqrt()
    mr = _nan((N, 2), hip_device)
    E.call('seg3d_gn_stats_finalize', E.ptr(part.to(hip_device)), E.ptr(mr), N, count, M, EPS, E.stream_ptr())
    got = mr.double().cpu()
    assert bool(torch.isfinite(got).all())
    e_mean = float(((got[:, 0] - mean).abs() / mean.abs()).max())
    e_rstd = float(((got[:, 1] - rstd).abs() / rstd).max())
    report('gn64_stats_finalize_synthetic_{}'.format(count), mean_rel_err=e_mean, rstd_rel_err=e_rstd, bar=2.0 ** -22)
    assert e_mean <= 2.0 ** -22 and e_rstd <= 2.0 ** -22, (e_mean, e_rstd)


# ---- 3. conditioning of the one-pass variance ----------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [0, 3, 30])
def test_stats_conditioning(hip_device, r):
    """N(r, 1) samples of 16384 elements ((2, 16, 8, 8, 16)): var = ss/M - mean^2 from fp32 partials loses (1 + r^2) in relative
    accuracy.  About 30 fp32 roundings per workgroup partial bound the sum of squares to 2^-19 relative, hence
    |rstd - ref| / ref <= (1 + r^2) * 2^-20 + 2^-22"""
    from segmentation3d import _engine as E
    N, M = 2, 16 * 8 * 8 * 16
    y = torch.from_numpy(detgen.normal(740, 'cond/{}'.format(r), (N, M))) + float(r)
    ref, yard = ref_stats(y), ref_stats(y, torch.float32)
    part, mr = dev_stats(E, y.to(hip_device))
    fig = Figures('gn64_stats_conditioning_r{}'.format(r))
    rel = float(((mr[:, 1].double().cpu() - ref['rstd']).abs() / ref['rstd']).max())
    bound = (1.0 + r * r) * 2.0 ** -20 + 2.0 ** -22
    fig.note(rstd_rel_err=rel, design_bound=bound)
    fig.check('mean', mr[:, 0], ref['mean'], yard['mean'], FLOOR_RED)
    if r <= 3:
        fig.check('rstd', mr[:, 1], ref['rstd'], yard['rstd'], FLOOR_RED)
    else:
        fig.check('rstd', mr[:, 1], ref['rstd'], None, 0.0, bar=bound * float(ref['rstd'].max()))
    fig.done()
    assert rel <= bound, (rel, bound)


@pytest.mark.parametrize('value', [3.25, 0.1])
def test_constant_sample(hip_device, value):
    """variance 0: rstd = 1/sqrt(eps), xhat = 0, so out == beta within 1e-4 and every output is finite"""
    from segmentation3d import _engine as E
    N, S, C = 2, 1024, 16
    y = torch.full((N, S, C), value)
    y[1] = -2.0 * value
    _, gamma, beta, _, _ = make_inputs('const', N, S, C)
    yd, gd, bd = y.to(hip_device), gamma.to(hip_device), beta.to(hip_device)
    part, mr = dev_stats(E, yd.reshape(N, -1))
    out = dev_apply(E, yd, mr, gd, bd, None, False, _nan((N, S, C), hip_device))
    assert bool(torch.isfinite(part).all()) and bool(torch.isfinite(mr).all()) and bool(torch.isfinite(out).all())
    err = float((out.cpu() - beta.view(1, 1, C)).abs().max())
    rstd_rel = float((mr[:, 1].cpu().double() * EPS ** 0.5 - 1.0).abs().max())
    report('gn64_constant_sample_{}'.format(value), out_minus_beta=err, rstd_rel_err=rstd_rel)
    assert err <= 1e-4, err


# ---- 4. apply -------------------------------------------------------------------------------------------------------------------
def _check_forward(fig, key, out_dev, ref, yard, bf16_out=False):
    """out against float64, and [out > 0] differing only inside the tie band"""
    out64 = ref['out']
    if bf16_out:
        fig.check(key, out_dev, out64, None, 0.0, bar=BF16_BAR * float(out64.abs().max()))
    else:
        fig.check(key, out_dev, out64, yard['out'], FLOOR_EW, cap=CAP_OUT)


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('C', [1, 3, 5, 4, 8, 12, 24, 48, 256])
def test_apply(hip_device, C, N):
    """seg3d_gn_apply at (N, C, 5, 7, 9): scalar path (C % 4 != 0) and vector path, residual x ReLU, contiguous and into the
    channel slice 4 : 4 + C of a [.., C + 8] buffer (whose other channels must stay untouched)"""
    from segmentation3d import _engine as E
    S = 5 * 7 * 9
    y, gamma, beta, res, _ = make_inputs('apply', N, S, C)
    st = ref_stats(y.reshape(N, -1))
    mr = torch.stack([st['mean'], st['rstd']], 1).float()
    yd, rd, gd, bd, mrd = (t.to(hip_device) for t in (y, res, gamma, beta, mr))
    for with_res, relu in itertools.product((False, True), (False, True)):
        fig = Figures('gn64_apply_C{}_N{}_res{}_relu{}'.format(C, N, int(with_res), int(relu)))
        ref = ref_gn(y, gamma, beta, res if with_res else None, relu)
        yard = ref_gn(y, gamma, beta, res if with_res else None, relu, dtype=torch.float32)
        out = dev_apply(E, yd, mrd, gd, bd, rd if with_res else None, relu, _nan((N, S, C), hip_device))
        _check_forward(fig, 'out', out, ref, yard)
        if relu:
            band = tie_band(ref['pre'], ref['out'])
            flips = ((out.cpu() > 0) != (ref['pre'] > 0)) & ~band
            fig.note(tie_share=float(band.double().mean()))
            assert float(band.double().mean()) <= TIE_SHARE and int(flips.sum()) == 0
        if C % 4 == 0:
            wide = _nan((N, S, C + 8), hip_device)
            dev_apply(E, yd, mrd, gd, bd, rd if with_res else None, relu, wide[..., 4:4 + C], ld=C + 8)
            assert torch.equal(wide[..., 4:4 + C], out)                  # same arithmetic, another destination
            assert bool(torch.isnan(wide[..., :4]).all()) and bool(torch.isnan(wide[..., 4 + C:]).all())
        fig.done()


# ---- 6. backward, stage by stage ---------------------------------------------------------------------------------------------
MODES = ('out_given', 'recompute', 'no_relu')


def _backward_case(E, dev, fig, y, gamma, beta, res, dout, mode, sliced, bf16=None, verify=True):
    """reduce -> finalize -> backward apply for one mask source; every stage against float64.
    bf16 = (dy_bf16, y_bf16) selects the bf16 entries (dout / out bf16 storage, y bf16 when y_bf16).
    verify=False: the device results only (for a bit-for-bit comparison with a verified run)."""
    N, S, C = y.shape
    relu = mode != 'no_relu'
    with_res = mode == 'out_given'
    resx = res if with_res else None
    st = ref_stats(y.reshape(N, -1))
    mr = torch.stack([st['mean'], st['rstd']], 1).float()
    fwd = ref_gn(y, gamma, beta, resx, relu)
    ref_mask = fwd['pre'] > 0
    act = torch.bfloat16 if bf16 is not None else torch.float32
    hip = dev
    yd = y.to(hip)
    if bf16 is not None and bf16[1]:
        yd = y.bfloat16().to(hip)                     # y is exactly representable: the caller rounded it
    gd, bd, mrd = gamma.to(hip), beta.to(hip), mr.to(hip)
    # out given: the stored forward output of the unit (float64 result rounded to the storage type keeps its sign)
    outd = fwd['out'].to(act).to(hip) if mode == 'out_given' else None
    if sliced:
        _, doutd = _wide(dout.to(act), hip, 750)
        ldd = C + 8
    else:
        doutd, ldd = dout.to(act).to(hip), 0
    y_bf = None if bf16 is None else bf16[1]
    part = dev_reduce(E, doutd, ldd, outd, yd, mrd, gd, bd, relu, y_bf)
    abx, s12, dgamma, dbeta, dbias = dev_finalize(E, part, gd, mrd, N, S, C)
    dy, dres = dev_bwd_apply(E, doutd, ldd, outd, yd, mrd, s12, gd, bd, relu, True, bf16)

    got = dict(part=part, abx=abx, s12=s12, dgamma=dgamma, dbeta=dbeta, dbias=dbias, dy=dy, dres=dres)
    if not verify:
        return got
    mask = None
    if relu:
        if mode == 'recompute':
            mask = device_decision(fig, dres, dout, fwd, ref_mask)
        else:
            mask = ref_mask
            assert torch.equal(dres.cpu() != 0, ref_mask)
    ref = ref_gn(y, gamma, beta, resx, relu, dout, mask)
    yard = ref_gn(y, gamma, beta, resx, relu, dout, mask, dtype=torch.float32)
    sg, sy = ref_stages(y, gamma, dout, mask), ref_stages(y, gamma, dout, mask, torch.float32)
    psum = part.double().sum(1).cpu()                 # [N, C, 3]
    for k, name in enumerate('ABX'):
        fig.check('part_' + name, psum[..., k], sg[name], sy[name], FLOOR_RED)
        fig.check('abx_' + name, abx[..., k], sg[name], sy[name], FLOOR_RED)
    fig.check('s12', s12, sg['s12'], sy['s12'], FLOOR_RED)
    fig.check('dgamma', dgamma, ref['dgamma'], yard['dgamma'], FLOOR_RED, cap=CAP_GRAD * float(ref['dgamma'].abs().max()))
    fig.check('dbeta', dbeta, ref['dbeta'], yard['dbeta'], FLOOR_RED, cap=CAP_GRAD * float(ref['dbeta'].abs().max()))
    fig.check('dbias', dbias, ref['dbias'], yard['dbias'], FLOOR_RED, denom=sg['dbias_mag'],
              cap=1e-3 + CAP_GRAD * float(ref['dbias'].abs().max()))
    if bf16 is not None and bf16[0]:
        fig.check('dy', dy, ref['dy'], None, 0.0, bar=BF16_BAR * float(ref['dy'].abs().max()))
    else:
        fig.check('dy', dy, ref['dy'], yard['dy'], FLOOR_EW, cap=CAP_GRAD * float(ref['dy'].abs().max()))
    fig.check('dres', dres, sg['g'], sy['g'], FLOOR_EW, cap=CAP_DRES * float(sg['g'].abs().max()))
    if with_res:
        assert torch.equal(ref['dres_autograd'], sg['g'])
    dy2, none = dev_bwd_apply(E, doutd, ldd, outd, yd, mrd, s12, gd, bd, relu, False, bf16)     # dres == NULL is accepted
    assert none is None and torch.equal(dy2, dy)
    return got


VEC_C = [4, 8, 16, 64, 256, 512, 1024]
SMALL_C = [1, 2, 3, 5, 7, 12]
# (3, 1024, 17, 16, 16) is left out: 13 M elements per float64 tensor take ~6 s of CPU reference; N = 3 at this width runs
# at (5, 7, 9) and the 34-voxel blocks with N = 3 at every other width
STAGED = [(C, dims, N) for dims in ((5, 7, 9), (17, 16, 16)) for C in VEC_C + SMALL_C for N in (1, 3)
          if not (C == 1024 and dims[0] == 17 and N == 3)] + \
         [(C, (2, 2, 2), N) for C in (16, 5) for N in (1, 3)]


@pytest.mark.parametrize('C,dims,N', STAGED, ids=['C{}_{}_N{}'.format(C, 'x'.join(map(str, d)), N) for C, d, N in STAGED])
def test_backward_staged(hip_device, C, dims, N):
    """seg3d_gn_bwd_reduce -> seg3d_gn_bwd_finalize -> seg3d_gn_bwd_apply: vector path (thread = channel quad x voxel lane, from
    256 voxel lanes at C = 4 to one at C = 1024) and small-C path; S = 315 (32-voxel blocks, the last with 27), S = 4352
    (34-voxel blocks), S = 8 (one block); mask from `out`, recomputed, none; dout contiguous and a channel slice"""
    from segmentation3d import _engine as E
    S = dims[0] * dims[1] * dims[2]
    assert {315: (32, 27), 4352: (34, 34), 8: (32, 8)}[S] == (_vpb(S), S - (S - 1) // _vpb(S) * _vpb(S))
    y, gamma, beta, res, dout = make_inputs('staged', N, S, C)
    for mode in MODES:
        fig = Figures('gn64_bwd_C{}_{}_N{}_{}'.format(C, 'x'.join(map(str, dims)), N, mode))
        got = _backward_case(E, hip_device, fig, y, gamma, beta, res, dout, mode, False)
        if C % 4 == 0:
            # the same gradient values as a channel slice of a wider buffer: another address pattern, the same arithmetic
            got2 = _backward_case(E, hip_device, None, y, gamma, beta, res, dout, mode, True, verify=False)
            for k in got:
                assert torch.equal(got[k], got2[k]), k
        fig.done()


@pytest.mark.parametrize('C', VEC_C + SMALL_C)
def test_finalize_acc_mask_and_fused(hip_device, C):
    """the parameter stage at (3, C, 5, 7, 9): each of the eight acc_mask values adds into pre-filled destinations exactly where
    its bit is set, dbias == NULL is accepted, and the one-launch form equals the two-launch form bit for bit and leaves its
    ticket at zero"""
    from segmentation3d import _engine as E
    N, S = 3, 315
    y, gamma, beta, _, dout = make_inputs('acc', N, S, C)
    st = ref_stats(y.reshape(N, -1))
    mrd = torch.stack([st['mean'], st['rstd']], 1).float().to(hip_device)
    yd, gd, bd, doutd = (t.to(hip_device) for t in (y, gamma, beta, dout))
    part = dev_reduce(E, doutd, 0, None, yd, mrd, gd, bd, True)
    base = dev_finalize(E, part, gd, mrd, N, S, C)            # checked against float64 by test_backward_staged
    assert all(bool(torch.isfinite(t).all()) for t in base)
    pre = [torch.from_numpy(detgen.normal(760 + k, 'acc/pre', (C,))).to(hip_device) for k in range(3)]
    ticket = torch.zeros(1, dtype=torch.int32, device=hip_device)
    for acc in range(8):
        two = dev_finalize(E, part, gd, mrd, N, S, C, acc, [p.clone() for p in pre])
        one = dev_finalize(E, part, gd, mrd, N, S, C, acc, [p.clone() for p in pre], ticket=ticket)
        assert int(ticket.item()) == 0
        for k in range(3):
            expect = pre[k] + base[2 + k] if acc & (1 << k) else base[2 + k]     # one fp32 add, as the kernel does
            assert torch.equal(two[2 + k], expect), (acc, k)
        for a, b in zip(one, two):
            assert torch.equal(a, b), acc
        assert torch.equal(two[0], base[0]) and torch.equal(two[1], base[1])
        nb2 = dev_finalize(E, part, gd, mrd, N, S, C, acc, [p.clone() for p in pre], want_dbias=False)
        nb1 = dev_finalize(E, part, gd, mrd, N, S, C, acc, [p.clone() for p in pre], want_dbias=False, ticket=ticket)
        assert int(ticket.item()) == 0
        for a, b in zip(nb1[:4] + nb2[:4], two[:4] + two[:4]):
            assert torch.equal(a, b), acc
    report('gn64_finalize_acc_mask_fused_C{}'.format(C), acc_masks=8.0, bit_identical=1.0)


# ---- 5. the capped grid --------------------------------------------------------------------------------------------------------
def _sample64(y_n, gamma, beta, res_n, dout_n, out_dev_n):
    """float64 forward + hand-written backward of ONE sample [S, C] with in-place operations (a residual ReLU unit)"""
    S, C = y_n.shape
    ga, be = gamma.double(), beta.double()
    x = y_n.double()
    mean = float(x.mean())
    x -= mean
    rstd = float(((x * x).mean() + EPS) ** -0.5)
    x *= rstd                                              # xhat
    out = x * ga
    out += be
    out += res_n
    ref_mask = out > 0
    band = out.abs() <= TIE_BAND * float(out.max())
    out.clamp_(min=0)
    dec = out_dev_n > 0
    flips_outside = int(((dec != ref_mask) & ~band).sum())
    mask = torch.where(band, dec, ref_mask)
    g = dout_n.double()
    g *= mask
    A, X = g.sum(0), x.sum(0)
    B = (g * x).sum(0)
    s1, s2 = float((ga * A).sum()) / (S * C), float((ga * B).sum()) / (S * C)
    mag = rstd * ((ga * A).abs() + S * abs(s1) + (s2 * X).abs())
    dbias = rstd * (ga * A - S * s1 - s2 * X)
    x *= -s2                                               # x is spent: dy = rstd (gamma g - s1 - xhat s2)
    x -= s1
    x.addcmul_(g, ga.expand_as(g))
    x *= rstd
    return dict(mean=mean, rstd=rstd, out=out, mask=mask, band_count=int(band.sum()), flips_outside=flips_outside, g=g, A=A, B=B,
                X=X, s1=s1, s2=s2, dy=x, dbias=dbias, dbias_mag=mag)


def _chain_large(E, dev, name, N, C, dims, nblk_expect):
    """statistics -> apply (residual + ReLU) -> reduce -> finalize -> backward apply with dres on a tensor large enough for the
    8192-workgroup cap of the element-wise grids; float64 sample by sample, the fp32 yardstick on the whole tensor"""
    S = dims[0] * dims[1] * dims[2]
    assert N * S * (C // 4) > 8192 * 256                      # the grid is capped: the GN_U trip loop runs, and its tail
    assert (N * S * (C // 4)) % (8192 * 256) != 0
    y, gamma, beta, res, dout = make_inputs(name, N, S, C)
    yd, rd, gd, bd, doutd = (t.to(dev) for t in (y, res, gamma, beta, dout))
    part_s, mr = dev_stats(E, yd.reshape(N, -1))
    out = dev_apply(E, yd, mr, gd, bd, rd, True, _nan((N, S, C), dev))
    part = dev_reduce(E, doutd, 0, out, yd, mr, gd, bd, True)
    assert part.shape[1] == nblk_expect
    abx, s12, dgamma, dbeta, dbias = dev_finalize(E, part, gd, mr, N, S, C)
    dy, dres = dev_bwd_apply(E, doutd, 0, out, yd, mr, s12, gd, bd, True, True)
    out_c, dy_c, dres_c = out.cpu(), dy.cpu(), dres.cpu()
    del out, dy, dres, yd, rd, doutd
    fig = Figures(name)
    refs = [_sample64(y[n], gamma, beta, res[n], dout[n], out_c[n]) for n in range(N)]
    share = sum(r['band_count'] for r in refs) / float(N * S * C)
    fig.note(tie_share=share, flips_outside_band=float(sum(r['flips_outside'] for r in refs)))
    assert share <= TIE_SHARE and sum(r['flips_outside'] for r in refs) == 0
    mask = torch.stack([r['mask'] for r in refs])
    yard = ref_gn(y, gamma, beta, res, True, dout, mask, dtype=torch.float32)
    ys = ref_stages(y, gamma, dout, mask, torch.float32)
    cat = lambda k: torch.stack([torch.as_tensor(r[k], dtype=torch.float64) for r in refs])
    fig.check('mean', mr[:, 0], cat('mean'), ys['mean'], FLOOR_RED)
    fig.check('rstd', mr[:, 1], cat('rstd'), ys['rstd'], FLOOR_RED)
    fig.check('out', out_c, cat('out'), F.relu(yard['pre']), FLOOR_EW, cap=CAP_OUT)
    psum = part.double().sum(1).cpu()
    for k, nm in enumerate('ABX'):
        fig.check('part_' + nm, psum[..., k], cat(nm), ys[nm], FLOOR_RED)
        fig.check('abx_' + nm, abx[..., k], cat(nm), ys[nm], FLOOR_RED)
    fig.check('s12', s12, torch.stack([cat('s1'), cat('s2')], 1), ys['s12'], FLOOR_RED)
    dg, db, dc = cat('B').sum(0), cat('A').sum(0), cat('dbias').sum(0)
    fig.check('dgamma', dgamma, dg, yard['dgamma'], FLOOR_RED, cap=CAP_GRAD * float(dg.abs().max()))
    fig.check('dbeta', dbeta, db, yard['dbeta'], FLOOR_RED, cap=CAP_GRAD * float(db.abs().max()))
    fig.check('dbias', dbias, dc, yard['dbias'], FLOOR_RED, denom=cat('dbias_mag').sum(0), cap=1e-3 + CAP_GRAD * float(dc.abs().max()))
    dy64 = cat('dy')
    fig.check('dy', dy_c, dy64, yard['dy'], FLOOR_EW, cap=CAP_GRAD * float(dy64.abs().max()))
    fig.check('dres', dres_c, cat('g'), ys['g'], FLOOR_EW, cap=CAP_DRES * float(cat('g').abs().max()))
    fig.done()


def test_capped_grid_chain(hip_device):
    """(3, 16, 72, 72, 72): 4.48 M channel quads on 8192 x 256 threads -- every thread runs the two-quad trip loop and part of them
    the tail; the walker steps across samples; backward reduce in 2048-voxel blocks with a ragged last one (183 blocks)"""
    from segmentation3d import _engine as E
    _chain_large(E, hip_device, 'gn64_capped_grid_3x16x72x72x72', 3, 16, (72, 72, 72), 183)


def test_capped_grid_walker_wrap(hip_device):
    """(2, 12, 72, 72, 72): 2.24 M quads of C/4 = 3 on 8192 x 256 threads.  The grid stride is no multiple of 3, so the walker's
    channel-quad wrap (q >= CQ) runs, which only a capped grid reaches (below the cap a thread owns one quad), together with the
    step across the sample boundary; the backward reduce is the small-C kernel in 2048-voxel blocks"""
    from segmentation3d import _engine as E
    _chain_large(E, hip_device, 'gn64_capped_grid_wrap_2x12x72x72x72', 2, 12, (72, 72, 72), 183)


# ---- 7. refusal -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [20, 24, 48])
def test_bwd_reduce_refuses_unsupported_channel_counts(hip_device, C):
    """C > 16 with C/4 not dividing 256: SEG3D_ERR_UNSUPPORTED (NotImplementedError from _engine.call), before any launch"""
    from segmentation3d import _engine as E
    N, S = 1, 8
    y = torch.zeros((N, S, C), device=hip_device)
    mr = torch.tensor([[0.0, 1.0]], device=hip_device)
    g = torch.ones(C, device=hip_device)
    nblk = E.query('seg3d_gn_bwd_blocks', S)
    part = torch.full((N, nblk, C, 3), 7.0, device=hip_device)
    with pytest.raises(NotImplementedError):
        E.call('seg3d_gn_bwd_reduce', E.ptr(y), None, E.ptr(y), E.ptr(mr), E.ptr(g), E.ptr(g), E.ptr(part), N, S, C, 1, 0,
               E.stream_ptr())
    torch.cuda.synchronize()
    assert bool((part == 7.0).all())


# ---- 8. the recomputed ReLU mask agrees with the forward output, sign by sign ---------------------------------------------------
@pytest.mark.parametrize('C', [5, 16, 64])
def test_recompute_sign_agreement(hip_device, C):
    """a ReLU unit without residual at (3, C, 17, 16, 16): reduce and backward apply with out == NULL (mask recomputed from y) equal,
    bit for bit, the same calls given the `out` that seg3d_gn_apply wrote -- the three expressions round alike"""
    from segmentation3d import _engine as E
    N, S = 3, 17 * 16 * 16
    y, gamma, beta, _, dout = make_inputs('sign', N, S, C, half_negative=True)
    yd, gd, bd, doutd = (t.to(hip_device) for t in (y, gamma, beta, dout))
    _, mr = dev_stats(E, yd.reshape(N, -1))
    out = dev_apply(E, yd, mr, gd, bd, None, True, _nan((N, S, C), hip_device))
    frac = float((out > 0).float().mean())
    assert 0.4 < frac < 0.6, frac
    p_out = dev_reduce(E, doutd, 0, out, yd, mr, gd, bd, True)
    p_rec = dev_reduce(E, doutd, 0, None, yd, mr, gd, bd, True)
    assert bool(torch.isfinite(p_out).all()) and torch.equal(p_out, p_rec)
    _, s12, _, _, _ = dev_finalize(E, p_out, gd, mr, N, S, C)
    dy_out, dres_out = dev_bwd_apply(E, doutd, 0, out, yd, mr, s12, gd, bd, True)
    dy_rec, dres_rec = dev_bwd_apply(E, doutd, 0, None, yd, mr, s12, gd, bd, True)
    assert bool(torch.isfinite(dy_out).all())
    assert torch.equal(dy_out, dy_rec) and torch.equal(dres_out, dres_rec)
    assert torch.equal(dres_out != 0, out > 0)
    report('gn64_recompute_sign_agreement_C{}'.format(C), positive_share=frac, bit_identical=1.0)


# ---- 9. bf16 entries, called directly -------------------------------------------------------------------------------------------
BF16_SHAPES = [(2, 16, (5, 7, 9)), (1, 64, (6, 6, 6))]


@pytest.mark.parametrize('N,C,dims', BF16_SHAPES, ids=['2x16x5x7x9', '1x64x6x6x6'])
def test_apply_mixed(hip_device, N, C, dims):
    """seg3d_gn_apply_mixed: the eight res_bf16 / out_bf16 / y_bf16 combinations (residual + ReLU), operands rounded to bf16 on the
    host and float64 on exactly those; a bf16 output into a channel slice (ld counts bf16 elements)"""
    from segmentation3d import _engine as E
    S = dims[0] * dims[1] * dims[2]
    y0, gamma, beta, res0, _ = make_inputs('mixed', N, S, C)
    gd, bd = gamma.to(hip_device), beta.to(hip_device)
    for res_bf, out_bf, y_bf in itertools.product((0, 1), repeat=3):
        y = bf16_round(y0) if y_bf else y0
        res = bf16_round(res0) if res_bf else res0
        st = ref_stats(y.reshape(N, -1))
        mrd = torch.stack([st['mean'], st['rstd']], 1).float().to(hip_device)
        ref = ref_gn(y, gamma, beta, res, True)
        yard = ref_gn(y, gamma, beta, res, True, dtype=torch.float32)
        yd = (y.bfloat16() if y_bf else y).to(hip_device)
        rd = (res.bfloat16() if res_bf else res).to(hip_device)
        odt = torch.bfloat16 if out_bf else torch.float32
        fig = Figures('gn64_apply_mixed_{}_res{}_out{}_y{}'.format('x'.join(map(str, (N, C) + dims)), res_bf, out_bf, y_bf))
        out = dev_apply(E, yd, mrd, gd, bd, rd, True, _nan((N, S, C), hip_device, odt), mixed=(res_bf, out_bf, y_bf))
        _check_forward(fig, 'out', out, ref, yard, bf16_out=bool(out_bf))
        band = tie_band(ref['pre'], ref['out'])
        assert float(band.double().mean()) <= TIE_SHARE
        assert int((((out.float().cpu() > 0) != (ref['pre'] > 0)) & ~band).sum()) == 0
        if out_bf and not res_bf:
            wide = _nan((N, S, C + 8), hip_device, torch.bfloat16)
            dev_apply(E, yd, mrd, gd, bd, rd, True, wide[..., 4:4 + C], ld=C + 8, mixed=(res_bf, out_bf, y_bf))
            assert torch.equal(wide[..., 4:4 + C], out)
            assert bool(torch.isnan(wide[..., :4]).all()) and bool(torch.isnan(wide[..., 4 + C:]).all())
        fig.done()


@pytest.mark.parametrize('N,C,dims', BF16_SHAPES, ids=['2x16x5x7x9', '1x64x6x6x6'])
def test_backward_bf16(hip_device, N, C, dims):
    """seg3d_gn_bwd_reduce_bf16 -> finalize -> seg3d_gn_bwd_apply_bf16: dy_bf16 x y_bf16, ReLU mask from a bf16 `out` and recomputed"""
    from segmentation3d import _engine as E
    S = dims[0] * dims[1] * dims[2]
    y0, gamma, beta, res0, dout0 = make_inputs('bwd16', N, S, C)
    dout, res = bf16_round(dout0), bf16_round(res0)
    for dy_bf, y_bf, mode in itertools.product((0, 1), (0, 1), ('out_given', 'recompute')):
        y = bf16_round(y0) if y_bf else y0
        fig = Figures('gn64_bwd_bf16_{}_dy{}_y{}_{}'.format('x'.join(map(str, (N, C) + dims)), dy_bf, y_bf, mode))
        _backward_case(E, hip_device, fig, y, gamma, beta, res, dout, mode, False, bf16=(dy_bf, y_bf))
        fig.done()
