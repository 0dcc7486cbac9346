"""Every instantiation of the thin 3x3x3 kernel family (csrc/conv_thin.hip, csrc/conv_thin_f32.hip: the stem, Cin <= 8, and the
head, Cout <= 8 -- forward / data gradient and weight gradient, fp32 and bf16 mode), driven through the C ABI, against a plain
float64 reference.  The cases are those of tests/thin_cases.py; each one first asserts through the read-only queries that it
reaches what it is named for (row form, z extent, tiles against workgroups, slabs).

Layout: NDHWC activations, weights [Cout][Cin][3][3][3], t = (kz * 3 + ky) * 3 + kx.

Reference: float64 on the device, from the definition, as 27 shifted matmuls on a zero-padded input (float64_util._conv_def,
_wgrad_def), on operands rounded the way the mode rounds them: thin_out_bf16 and thin_out_mfma take a bf16 x and fp32 weights, the
fatbf16 weight gradient a bf16 fat operand and an fp32 thin one, thin_in_mfma16 fp32 operands.  The statistics slots are summed per
sample and compared with sum y and sum y^2 of the float64 result; the thin-in kernels take theirs before rounding y to bf16.

Bars: nothing is pinned to what the kernels give.  Each case also runs the same operation in fp32 on the CPU (F.conv3d, autograd
for the weight gradient): the yardstick.  fp32-arithmetic kernels (thin_in*, persistent, thin_out, thin_out_f32mfma, fp32 weight
gradient): err <= 4 * yardstick + 2e-6 * scale element-wise, + 1e-5 * scale for sums and gradients, scale = max|ref|, under the caps
of the existing tests, 2e-6 * scale for fp32 outputs and 2e-4 * scale for the fp32 weight gradient.  Kernels that carry an operand
as a bf16 hi + lo pair (thin_in_mfma16, thin_out_mfma, the fatbf16 weight gradient) and thin_out_bf16: their error, 2^-17 per
operand, is not the yardstick's; the bar is the existing 2e-5 * scale.  bf16-stored outputs, per element: |got - ref| <=
2^-8 |ref| + (the bar).  Statistics: the existing bars, 1e-5 (2e-5 for thin-in) of sum |y| and of sum y^2; for the fp32-arithmetic
kernels also 4 * yardstick + 1e-5 * scale (a sum of hi + lo outputs carries their error, which is not the yardstick's).

Write discipline: y, the statistics, dw and the workspace are NaN-filled inside NaN guard bands of at least one tile of rows; the
guards must come back bit-identical, no NaN may survive inside, every statistics slot is written, a second call on the same inputs
is bit-identical, and an accumulating weight gradient started from known values equals base + plain bit for bit.

Figures per kernel body, MI355X: the largest err / bar over outputs (y or dw) and over the statistics, the largest yardstick /
scale, and the slowest case (a run appends every figure to the parity report that gpu_util.report writes):
    thin_in<1..8>                 y 0.27 st 0.01;   bf16out<1..8> y 0.01 (beside 2^-8 |ref|) st 0.02        yardstick 6.2e-7   0.01 s
    thin_in_mfma16<1>             y 0.17 st 0.06;   <2> y 0.09 st 0.06                                       yardstick 2.9e-7   0.01 s
    persistent, 32 rows           fp32 y 0.32 st 0.01, bf16 y 0.04 st 0.05                                   yardstick 6.0e-7   0.13 s
    persistent, 16 rows           fp32 y 0.33 st 0.01, bf16 y 0.03 st 0.01                                   yardstick 6.6e-7   0.06 s
    thin_out<2 | 4 | 8>           y 0.50 | 0.49 | 0.41, st 0.01;   thin_out_bf16 y 0.05 st 0.01              yardstick 1.2e-6   0.01 s
    thin_out_mfma                 <16, 2> y 0.19 st 0.19;  <16, 3> 0.14 / 0.22;  <32, 2> 0.15 / 0.26;  <32, 3> 0.17 / 0.08
                                                                                                             yardstick 1.8e-6   0.01 s
    thin_out_f32mfma              masked y 0.10 st 0.04, interior y 0.10 st 0.01 (all eight (Cin, CO), six tz) yardstick 1.3e-6   0.09 s
    weight gradient               fp32 <1..8> 0.03  (yardstick 3.1e-6);   bf16 fat operand <1..8> 0.18  (yardstick 6.2e-6)      1.7 s
(yardstick: the largest yardstick / scale; seconds: the slowest case, reference and CPU yardstick included -- 1.7 s is the weight
gradient of 70 samples, 4410 tiles, and 0.8 s that of 3 x 27 x 37 x 83; the first case of a run also loads the library, 0.5 s.)
315 cases and 15 refusals; no case is above its bar.
"""
import time

import pytest
import torch
import torch.nn.functional as F

import thin_cases as T
from float64_util import (FLOOR_EW, FLOOR_RED, Figures, Guarded, _activation, _check_stats, _conv_def, _engine, _noise, _weight,
                          _wgrad_def, bf16_round)

pytestmark = pytest.mark.gpu

CAP_Y_REL, CAP_HILO_REL, CAP_WGRAD_REL, CAP_STAT_IN = 2e-6, 2e-5, 2e-4, 2e-5
HILO = ('mfma16', 'thin_out_mfma', 'thin_out_bf16')        # forward kernels under the flat 2e-5 * scale bar


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _nan_buf(n, dev, dtype=torch.float32):
    return torch.full((n,), float('nan'), dtype=dtype, device=dev)


def _operands(fig, c, A, B, seed):
    """x [N, D, H, W, A], the weight in its role's layout, the [B][A] weight the role computes with, pack strides and flip, bias"""
    fwd = c.role == 'fwd'
    x = _activation(seed, fig.name + '/x', c.N, (c.D, c.H, c.W), A)
    w = _weight(seed + 1, fig.name + '/w', (B, A, 3, 3, 3) if fwd else (A, B, 3, 3, 3), 27 * A)
    weff = w if fwd else w.transpose(0, 1).flip(2, 3, 4).contiguous()
    sa, sb, flip = (27, 27 * A, 0) if fwd else (27 * B, 27, 1)
    bias = (0.3 * _noise(seed + 2, fig.name + '/b', (B,)) + 0.2) if c.full else None
    return x, w, weff, (sa, sb, flip), bias


def _forward_case(fig, c, dev, x, weff, bias, run, cnt, guard, ydt, hilo, stat_cap):
    """reference, yardstick, two guarded runs of `run(y, stats)`, and every check of a forward case"""
    ref = _conv_def(x.to(dev).double(), weff.to(dev).double())
    yard = F.conv3d(x.permute(0, 4, 1, 2, 3), weff, bias, padding=1).permute(0, 2, 3, 4, 1)
    if c.full:
        ref = ref + bias.to(dev).double()
    runs = []
    for _ in range(2):
        y = Guarded(ref.numel(), guard, dev, ydt)
        stats = Guarded(c.N * cnt * 2, 1024, dev) if c.full else None
        run(y, stats)
        torch.cuda.synchronize()
        runs.append((y, stats))
    (y, stats), (y2, stats2) = runs
    fig.require(y.guards_untouched() and y2.guards_untouched(), 'y: the guard bands were written')
    scale = float(ref.abs().max())
    fig.check('y', y.t, ref.reshape(-1), yard.reshape(-1), FLOOR_EW, cap=(CAP_HILO_REL if hilo else CAP_Y_REL) * scale,
              bf16_out=ydt == torch.bfloat16, yardstick=not hilo)
    fig.require(torch.equal(_bits(y.t), _bits(y2.t)), 'y: the second call differs')
    if c.full:
        _check_stats(fig, stats, ref, yard, c.N, cap=stat_cap, yardstick=not hilo)
        fig.require(stats2.guards_untouched(), 'stats: the guard bands were written by the second call')
        fig.require(torch.equal(_bits(stats.t), _bits(stats2.t)), 'stats: the second call differs')


def _finish(fig, t0):
    torch.cuda.synchronize()
    fig.figs['seconds'] = time.perf_counter() - t0
    fig.done()


# ---- thin-in: stem forward, head data gradient -----------------------------------------------------------------------------
@pytest.mark.parametrize('case', T.IN_CASES, ids=T.case_id)
def test_thin_in(hip_device, case):
    E, c, dev, t0 = _engine(), case, hip_device, time.perf_counter()
    key = T.in_key(c)
    fig = Figures('thin/{}/{}'.format('-'.join(str(k) for k in key), T.case_id(c)))
    cobs = (c.Cout + 31) // 32
    if c.kernel == 'persistent':
        assert E.query('seg3d_conv3d_k3_thin_in_persistent_variant', c.Cout) == (16 if key[0] == 'thin_in_persistent16' else 32)
        wgs = E.query('seg3d_conv3d_k3_thin_in_persistent_workgroups', c.N, c.D, c.H, c.W, c.Cout)
        tiles = T.tiles(c, T.IN_TILE)
        assert (tiles > wgs and tiles % wgs != 0) if T.TILE_CLASS[c] == 'many' else tiles == wgs
        cnt = E.query('seg3d_conv3d_k3_thin_in_persistent_stats_count', c.D, c.H, c.W, cobs)
    else:
        cnt = E.query('seg3d_conv3d_k3_thin_stats_count', c.D, c.H, c.W, cobs)
    x, w, weff, (sa, sb, flip), bias = _operands(fig, c, c.CT, c.Cout, 950)
    xd, wd = x.to(dev), w.to(dev)
    bd = bias.to(dev) if c.full else None
    if c.kernel == 'mfma16':
        wp = _nan_buf(E.query('seg3d_packed_thin_in16_elems', c.CT, c.Cout), dev, torch.bfloat16)
        E.call('seg3d_pack_weights_thin_in16', E.ptr(wd), E.ptr(wp), c.CT, c.Cout, sa, sb, flip, E.stream_ptr())
    else:
        wp = _nan_buf(E.query('seg3d_packed_thin_in_floats', c.CT, c.Cout), dev)
        E.call('seg3d_pack_weights_thin_in', E.ptr(wd), E.ptr(wp), c.CT, c.Cout, sa, sb, flip, E.stream_ptr())

    def run(y, stats):
        args = (E.ptr(xd), E.ptr(wp), E.ptr(bd), E.ptr(y.t), E.ptr(stats.t) if stats else None, c.N, c.D, c.H, c.W, c.CT, c.Cout)
        if c.kernel == 'persistent':
            E.call('seg3d_conv3d_k3_thin_in_persistent_fwd', *args, c.out_bf16, E.stream_ptr())
        elif c.kernel == 'mfma16':
            E.call('seg3d_conv3d_k3_thin_in_mfma16_fwd', *args, E.stream_ptr())
        else:
            E.call('seg3d_conv3d_k3_thin_in_bf16out_fwd' if c.out_bf16 else 'seg3d_conv3d_k3_thin_in_fwd', *args, E.stream_ptr())

    _forward_case(fig, c, dev, x, weff, bias, run, cnt, 256 * c.Cout, torch.bfloat16 if c.out_bf16 else torch.float32,
                  c.kernel in HILO, CAP_STAT_IN)
    _finish(fig, t0)


# ---- thin-out: head forward, stem data gradient ----------------------------------------------------------------------------
@pytest.mark.parametrize('case', T.OUT_CASES, ids=T.case_id)
def test_thin_out(hip_device, case):
    E, c, dev, t0 = _engine(), case, hip_device, time.perf_counter()
    fig = Figures('thin/{}/{}'.format('-'.join(str(k) for k in T.out_keys(c)[-1]), T.case_id(c)))
    dims = (c.N, c.D, c.H, c.W)
    if c.kernel == 'thin_out_f32mfma':
        assert E.query('seg3d_conv3d_k3_thin_out_f32mfma_tz', *dims) == c.tz
        cnt = E.query('seg3d_conv3d_k3_thin_out_f32mfma_stats_count', *dims)
    else:
        cnt = E.query('seg3d_conv3d_k3_thin_out_stats_count', c.D, c.H, c.W)
    x, w, weff, (sa, sb, flip), bias = _operands(fig, c, c.Cin, c.Cout, 960)
    xbf = c.kernel in ('thin_out_bf16', 'thin_out_mfma')
    if xbf:
        x = bf16_round(x)
    xd = x.to(dev).bfloat16() if xbf else x.to(dev)
    wd = w.to(dev)
    bd = bias.to(dev) if c.full else None
    if c.kernel in ('thin_out', 'thin_out_bf16'):
        wp = _nan_buf(((c.Cin + 7) // 8) * 27 * 8 * c.CO, dev)
        E.call('seg3d_pack_weights_thin_out', E.ptr(wd), E.ptr(wp), c.Cin, c.Cout, c.CO, sa, sb, flip, E.stream_ptr())
    elif c.kernel == 'thin_out_mfma':
        wp = _nan_buf(E.query('seg3d_thin_out_mfma_packed_elems', c.Cin), dev, torch.bfloat16)
        E.call('seg3d_pack_weights_thin_out_mfma', E.ptr(wd), E.ptr(wp), c.Cin, c.Cout, sa, sb, flip, E.stream_ptr())
    else:
        wp = _nan_buf(E.query('seg3d_thin_out_f32mfma_packed_floats', c.Cin, c.Cout), dev)
        E.call('seg3d_pack_weights_thin_out_f32mfma', E.ptr(wd), E.ptr(wp), c.Cin, c.Cout, sa, sb, flip, E.stream_ptr())

    def run(y, stats):
        args = (E.ptr(xd), E.ptr(wp), E.ptr(bd), E.ptr(y.t), E.ptr(stats.t) if stats else None, *dims, c.Cin, c.Cout)
        if c.kernel == 'thin_out':
            E.call('seg3d_conv3d_k3_thin_out_fwd', *args, c.CO, E.stream_ptr())
        elif c.kernel == 'thin_out_bf16':
            E.call('seg3d_conv3d_k3_thin_out_bf16_fwd', *args, c.CO, E.stream_ptr())
        else:
            E.call('seg3d_conv3d_k3_{}_fwd'.format(c.kernel), *args, E.stream_ptr())

    guard = 4 * ((max(c.tz, 8) * 128 * c.Cout + 3) // 4)               # one tile of rows
    _forward_case(fig, c, dev, x, weff, bias, run, cnt, guard, torch.float32, c.kernel in HILO, 1e-5)
    _finish(fig, t0)


# ---- weight gradient -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', T.WGRAD_CASES, ids=T.case_id)
def test_thin_wgrad(hip_device, case):
    E, c, dev, t0 = _engine(), case, hip_device, time.perf_counter()
    fig = Figures('thin/{}-{}/{}'.format(*T.wg_key(c), T.case_id(c)))
    dims, sp = (c.N, c.D, c.H, c.W), (c.D, c.H, c.W)
    nws = E.query('seg3d_k3_thin_wgrad_workspace_floats', *dims, c.CT, c.CF)
    slabs = nws // (((c.CF + 31) // 32) * ((27 * c.CT + 31) // 32) * 1024)
    assert T.slab_class(slabs) == c.slabs
    stem = c.conv == 'stem'
    # stem: thin = x, fat = dy;  head: thin = dy, fat = x
    thin = _activation(970, fig.name + '/thin', c.N, sp, c.CT, offset=0.25 if stem else 0.0)
    fat = _activation(971, fig.name + '/fat', c.N, sp, c.CF, offset=0.0 if stem else 0.25)
    if c.fat_bf16:
        fat = bf16_round(fat)
    x, dy = (thin, fat) if stem else (fat, thin)
    ref = _wgrad_def(x.to(dev).double(), dy.to(dev).double())                # [Cout][Cin][27]: the layout dw is written in
    w0 = torch.zeros(dy.shape[-1], x.shape[-1], 3, 3, 3, requires_grad=True)
    yard = torch.autograd.grad(F.conv3d(x.permute(0, 4, 1, 2, 3), w0, padding=1), w0, dy.permute(0, 4, 1, 2, 3))[0]
    yard = yard.reshape(ref.shape)
    s_ct, s_cf, flip = (27, 27 * c.CT, 0) if stem else (27 * c.CF, 27, 1)
    thind = thin.to(dev)
    fatd = fat.to(dev).bfloat16() if c.fat_bf16 else fat.to(dev)
    scale = float(ref.abs().max())
    prior = (_noise(972, fig.name + '/dw0', tuple(ref.shape)) * scale * 0.5).to(dev)

    def run(accumulate):
        dw = Guarded(ref.numel(), 27 * 1024, dev, fill=prior if accumulate else None)
        ws = Guarded(nws, 32 * 1024, dev)
        E.call('seg3d_k3_thin_wgrad_fatbf16' if c.fat_bf16 else 'seg3d_k3_thin_wgrad', E.ptr(thind), E.ptr(fatd), E.ptr(dw.t),
               E.ptr(ws.t), *dims, c.CT, c.CF, s_ct, s_cf, flip, accumulate, E.stream_ptr())
        torch.cuda.synchronize()
        fig.require(dw.guards_untouched(), 'dw: the guard bands were written (accumulate = {})'.format(accumulate))
        fig.require(ws.guards_untouched(), 'workspace: the guard bands were written (accumulate = {})'.format(accumulate))
        fig.require(not bool(torch.isnan(ws.t).any()), 'workspace: a slab entry was not written')
        return dw

    dw, dw2 = run(0), run(0)
    fig.require(torch.equal(_bits(dw.t), _bits(dw2.t)), 'dw: the second call differs')
    got = dw.t
    if c.accumulate:
        acc = run(1)
        fig.require(torch.equal(_bits(acc.t), _bits(prior.reshape(-1) + dw.t)), 'dw: the accumulating call is not base + plain')
        got, ref, yard = acc.t, ref + prior.double(), yard + prior.cpu()
    fig.check('dw', got, ref.reshape(-1), yard.reshape(-1), FLOOR_RED, cap=(CAP_HILO_REL if c.fat_bf16 else CAP_WGRAD_REL) * scale,
              yardstick=not c.fat_bf16)
    _finish(fig, t0)


# ---- refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,kind,args,why', T.REFUSALS, ids=[r[3] for r in T.REFUSALS])
def test_refusals_write_nothing(hip_device, name, kind, args, why):
    """arguments outside the kernels' contract: an error whose message starts with the entry's name; the outputs stay NaN"""
    E, dev = _engine(), hip_device
    N, D, H, W = 1, 4, 8, 16
    ones = lambda ch, dt=torch.float32: torch.ones((N, D, H, W, max(ch, 1) + 8), dtype=dt, device=dev)
    wp = torch.zeros(1 << 16, dtype=torch.float32, device=dev)              # ample for any image of these channel counts
    bias = torch.zeros(64, device=dev)
    out = Guarded(N * D * H * W * 64, 4096, dev)
    aux = Guarded(1 << 16, 4096, dev)                                       # statistics, or the weight gradient's workspace
    with pytest.raises((ValueError, NotImplementedError)) as info:
        if kind == 'in':
            head = (E.ptr(ones(args[0])), E.ptr(wp), E.ptr(bias), E.ptr(out.t), E.ptr(aux.t), N, D, H, W, *args)
            E.call(name, *head, *((0,) if name.endswith('persistent_fwd') else ()), E.stream_ptr())
        elif kind == 'out':
            xdt = torch.bfloat16 if name.endswith('thin_out_mfma_fwd') else torch.float32
            E.call(name, E.ptr(ones(args[0], xdt)), E.ptr(wp), E.ptr(bias), E.ptr(out.t), E.ptr(aux.t), N, D, H, W, *args, E.stream_ptr())
        else:
            CT, CF = args
            E.call(name, E.ptr(ones(CT)), E.ptr(ones(CF)), E.ptr(out.t), E.ptr(aux.t), N, D, H, W, CT, CF, 27, 27 * max(CT, 1), 0, 0,
                   E.stream_ptr())
    assert str(info.value).startswith(name + ':') and E.last_error().startswith(name + ':'), (why, str(info.value))
    torch.cuda.synchronize()
    assert out.all_nan() and out.guards_untouched() and aux.all_nan() and aux.guards_untouched(), why
