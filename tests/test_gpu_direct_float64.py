"""Every kernel of the VALU fallback conv family (csrc/conv_direct.hip: the gather kernel at k3, k2s2 and k1, the transposed k2s2
kernel, the generic and the thin 1x1x1 weight-gradient kernels, both reducers), the tap-major weight packer, and the head's
per-voxel tail (seg3d_softmax_fwd/_bwd, seg3d_sigmoid_fwd/_bwd of csrc/loss.hip), driven through the C ABI, against a plain
float64 reference.  The cases are those of tests/direct_cases.py; each weight-gradient case first asserts through the read-only
queries that it reaches the kernel, chunk count, PAIRS and reducer it is named for.

Layout: NDHWC activations; W(a, b, t) = w[a * sa + b * sb + t], packed by seg3d_pack_weights_tapmajor with the strides and the flip
_ops.conv / _ops.conv_dgrad give each role; probabilities NCDHW [N][C][S].

Operands: float64_util._activation gives every sample its own mean and spread (a k3 halo read that lands in the neighbouring sample
is an error of the size of the data); x, dy, the weight and its packed image, and the bias sit inside NaN guard bands of more than
one z plane plus one row plus one voxel (1024 voxels' worth at least); y, dx, part and dw are NaN-filled inside NaN guard bands.

Reference: float64 from the definitions (float64_util._conv_def, _wgrad_def, _k2_*_def, _k1_*_def; torch.softmax, torch.sigmoid and
autograd in float64 for the tail).

Bars: nothing is pinned to what the kernels give.  Each case runs the same operation in fp32 on the CPU (F.conv3d,
F.conv_transpose3d, torch.softmax, torch.sigmoid, autograd): the yardstick.  err <= 4 * yardstick + 2e-6 * scale for element-wise
outputs, + 1e-5 * scale for dw, scale = max |ref|, under the caps of the existing tests: 1e-4 absolute for conv outputs, 2e-4 * scale
for dw, 1e-6 absolute for probabilities, 1e-5 * scale for the tail's gradient.  The reducer on its own sums small integers: every
order of summation is exact in fp32, and the result must equal the float64 sum.  The packer is compared bit for bit.

Write discipline: every guard bit-identical afterwards, the inputs too; no NaN left in y, dx, dw or the slabs of the reported chunks;
the slabs' padded columns exactly 0.0; the workspace beyond the reported chunks still NaN; a second call bit-identical;
accumulate = 1 from a known base equals base + plain bit for bit.

Figures per kernel body, MI355X: the largest err / bar, the largest err / scale, the largest yardstick / scale, and the slowest case
with its reference and CPU yardstick included (a run appends every figure to the parity report that gpu_util.report writes):
    k3        conv_fwd_direct_kernel<3, 1, 1>          y 0.11            err 4.5e-7   yardstick 5.0e-7   0.12 s  (1 x (32, 32, 36) 3 -> 256)
    k2s2      conv_fwd_direct_kernel<2, 2, 0>          y 0.10            err 2.7e-7   yardstick 2.5e-7   0.06 s  (1 x (64, 64, 66) 4 -> 256)
    k1        conv_fwd_direct_kernel<1, 1, 0>          y 0.07            err 2.0e-7   yardstick 2.2e-7   0.06 s  (1 x (63, 127, 131) 5 -> 9)
    convT     convT_k2s2_fwd_direct_kernel             y 0.05            err 1.1e-7   yardstick 1.5e-7   0.05 s  (1 x (32, 32, 33) 4 -> 32)
    wgrad_direct_kernel<3, 1, 1>, both reducers        dw 0.07           err 8.2e-7   yardstick 5.0e-6   0.13 s  (1 x (63, 127, 131) 3 -> 5)
    wgrad_direct_kernel<2, 2, 0>, both roles           dw 0.01           err 1.4e-7   yardstick 1.6e-7   0.01 s  (1 x (18, 22, 46) 12 -> 5)
    wgrad_direct_kernel<1, 1, 0>                       dw 0.02           err 2.4e-7   yardstick 5.2e-7   0.01 s  (1 x (9, 11, 23) 32 -> 5)
    wgrad_k1_thin_kernel, both reducers                dw 0.02           err 1.9e-7   yardstick 5.1e-7   0.09 s  (1 x (63, 127, 131) 5 -> 5)
    softmax_fwd_kernel / softmax_bwd_kernel            p 0.21  din 0.16  err 4.7e-7   yardstick 3.3e-7   0.12 s  (3 x 699 071, C = 2)
    sigmoid_fwd_kernel / sigmoid_bwd_kernel            p 0.09  din 0.08  err 2.3e-7   yardstick 2.3e-7   0.11 s  (3 x 699 071, C = 2)
The million-voxel weight gradients stay below the autograd yardstick's own error (0.04 and 0.54 of it): no second yardstick was needed.  Soft-max rows sum
to 1 within 2.5e-7 (C = 16); C = 1 gives 1.0 and a gradient of 0.0 exactly.  All 24 runs of the reducers alone and all 96 packed
images are exact.  The first forward and the first weight-gradient case also load the library and warm the device up (0.5 s and
0.8 s); the whole file takes 4.5 s.  18 forward cases, 14 weight-gradient cases, 9 refusals, 24 reducer runs, 12 packer shapes and
10 tail cases; no case is above its bar.
"""
import ctypes
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import direct_cases as K
from float64_util import (FLOOR_EW, FLOOR_RED, NAN, Figures, Guarded, _activation, _conv_def, _engine, _k1_def, _k1_wgrad_def,
                          _k2_gather_def, _k2_scatter_def, _k2_wgrad_def, _noise, _weight, _wgrad_def)
from gpu_util import report

pytestmark = pytest.mark.gpu

CAP_Y_ABS, CAP_DW_REL = 1e-4, 2e-4            # the existing tests' bars (test_conv3d_k3_fwd_bwd), as caps
CAP_P_ABS, CAP_DIN_REL = 1e-6, 1e-5           # those of test_softmax_and_cat


def _bits(t):
    return t.view(torch.int32)


def _round4(n):
    return (n + 3) // 4 * 4


def _guard(H, W, C):
    """more than one z plane, one row and one voxel of a tensor with C channels, and at least 1024 voxels (whole float4s)"""
    return _round4(max(H * W + W + 2, 1024) * C)


def _same(g, t):
    return g.guards_untouched() and bool(torch.equal(_bits(g.t), _bits(t.reshape(-1))))


def _finish(fig, t0):
    torch.cuda.synchronize()
    fig.figs['seconds'] = time.perf_counter() - t0
    fig.done()


def _cl(t):
    """NDHWC -> the NCDHW view torch's convolutions take"""
    return t.permute(0, 4, 1, 2, 3)


def _pack(E, fig, w, A, B, T, sa, sb, flip, dev):
    """the tap-major image of w inside guard bands; w itself is read from inside guard bands too"""
    BP = _round4(B)
    wd = w.to(dev)
    wg = Guarded(w.numel(), _round4(1024 * B), dev, fill=wd)
    wp = Guarded(T * A * BP, 1024 * BP, dev)
    E.call('seg3d_pack_weights_tapmajor', E.ptr(wg.t), E.ptr(wp.t), A, B, BP, T, sa, sb, flip, E.stream_ptr())
    torch.cuda.synchronize()
    fig.require(_same(wg, wd), 'the weight was written')
    fig.require(wp.guards_untouched() and not bool(torch.isnan(wp.t).any()), 'packed image: guards written, or an entry not written')
    return wp


# ---- forward / data gradient -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.FWD_CASES, ids=K.case_id)
def test_forward(hip_device, case):
    E, c, dev, t0 = _engine(), case, hip_device, time.perf_counter()
    fig = Figures('direct/{}/{}'.format(c.kernel, K.case_id(c)))
    A, B, fwd = c.Cin, c.Cout, c.role == 'fwd'
    k = {'k3': 3, 'k2s2': 2, 'k1': 1, 'convT': 2}[c.kernel]
    T = k ** 3
    x = _activation(1000, fig.name + '/x', c.N, (c.D, c.H, c.W), A)
    if c.kernel == 'convT':
        # w[a][b][t]: the transposed conv's own weight, and the stride-2 conv's weight w[co][ci][t] in its data-gradient role
        w, (sa, sb, flip) = _weight(1001, fig.name + '/w', (A, B, 2, 2, 2), A), (8 * B, 8, 0)
    elif fwd or c.kernel == 'k2s2':
        # w[b][a][t]: a conv's own weight; for k2s2 also the transposed conv's weight w[ci][co][t] in its data-gradient role
        w, (sa, sb, flip) = _weight(1001, fig.name + '/w', (B, A, k, k, k), T * A), (T, A * T, 0)
        weff = w
    else:
        # the data gradient of a k3 / k1 conv with weight w[a = co][b = ci][t]: taps reversed
        w, (sa, sb, flip) = _weight(1001, fig.name + '/w', (A, B, k, k, k), T * A), (B * T, T, int(k == 3))
        weff = w.transpose(0, 1).flip(2, 3, 4).contiguous()
    bias = (0.3 * _noise(1002, fig.name + '/b', (B,)) + 0.2) if fwd else None

    x64 = x.to(dev).double()
    if c.kernel == 'k3':
        ref = _conv_def(x64, weff.to(dev).double())
        yard = F.conv3d(_cl(x), weff, bias, padding=1)
    elif c.kernel == 'k2s2':
        ref = _k2_gather_def(x64, w.to(dev).double())
        yard = F.conv3d(_cl(x), w, bias, stride=2)
    elif c.kernel == 'k1':
        ref = _k1_def(x64, weff.to(dev).double().reshape(B, A))
        yard = F.conv3d(_cl(x), weff, bias)
    else:
        ref = _k2_scatter_def(x64, w.to(dev).double())
        yard = F.conv_transpose3d(_cl(x), w, bias, stride=2)
    del x64
    yard = yard.permute(0, 2, 3, 4, 1)
    if fwd:
        ref = ref + bias.to(dev).double()
    assert ref.numel() == K.out_voxels(c) * B and tuple(yard.shape) == tuple(ref.shape)

    xd = x.to(dev)
    xg = Guarded(x.numel(), _guard(c.H, c.W, A), dev, fill=xd)
    wp = _pack(E, fig, w, A, B, T, sa, sb, flip, dev)
    wp_before = wp.buf.clone()
    bg = Guarded(B, _round4(1024 * B), dev, fill=bias.to(dev)) if fwd else None

    def run():
        y = Guarded(ref.numel(), _guard(ref.shape[2], ref.shape[3], B), dev)
        head = (E.ptr(xg.t), E.ptr(wp.t), E.ptr(bg.t) if fwd else None, E.ptr(y.t), c.N, c.D, c.H, c.W, A, B)
        if c.kernel == 'convT':
            E.call('seg3d_convT3d_k2s2_fwd_direct', *head, E.stream_ptr())
        else:
            E.call('seg3d_conv3d_fwd_direct', *head, *K.FWD_KERNELS[c.kernel], E.stream_ptr())
        torch.cuda.synchronize()
        fig.require(y.guards_untouched(), 'y: the guard bands were written')
        return y

    y, y2 = run(), run()
    fig.check('y', y.t, ref.reshape(-1), yard.reshape(-1), FLOOR_EW, cap=CAP_Y_ABS)
    fig.require(torch.equal(_bits(y.t), _bits(y2.t)), 'y: the second call differs')
    fig.require(_same(xg, xd), 'x was written')
    fig.require(torch.equal(_bits(wp.buf), _bits(wp_before)), 'the packed image was written')
    fig.require(bg is None or _same(bg, bias.to(dev)), 'the bias was written')
    _finish(fig, t0)


# ---- weight gradient -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.WGRAD_CASES, ids=K.case_id)
def test_wgrad(hip_device, case):
    E, c, dev, t0 = _engine(), case, hip_device, time.perf_counter()
    fig = Figures('direct/wgrad_{}/{}'.format(c.kernel, K.case_id(c)))
    (ks, stride), T, CA, CB = K.WGRAD_KS[c.kernel], K.taps(c), c.CA, c.CB
    args = (c.N, c.D, c.H, c.W, CA, CB, ks, stride)
    assert E.query('seg3d_wgrad_direct_variant', *args) == K.wgrad_code(c)
    assert E.query('seg3d_wgrad_direct_chunks', *args) == c.chunks
    assert E.query('seg3d_wgrad_direct_pairs', CA, CB) == c.pairs
    assert E.query('seg3d_wgrad_reduce_variant', c.chunks, T, CA, CB) == K.reduce_code(c)
    qd = K.q_dims(c)
    P = _activation(1010, fig.name + '/P', c.N, (c.D, c.H, c.W), CA, offset=0.25)
    Q = _activation(1011, fig.name + '/Q', c.N, qd, CB, offset=0.0)
    P64, Q64 = P.to(dev).double(), Q.to(dev).double()
    if c.kernel == 'k3':
        ref = _wgrad_def(P64, Q64, blocks=1024 if P64.numel() > (1 << 20) else 1)       # [b][a][t]
    elif c.kernel == 'k2s2':
        ref = _k2_wgrad_def(P64, Q64).permute(1, 0, 2)
    else:
        ref = _k1_wgrad_def(P64, Q64).reshape(CB, CA, 1)
    del P64, Q64
    w0 = torch.zeros(CB, CA, ks, ks, ks, requires_grad=True)
    if c.role == 'convT':    # w0[ci = b][co = a][t] of the transposed conv x = Q -> dy = P
        yard = torch.autograd.grad(F.conv_transpose3d(_cl(Q), w0, stride=2), w0, _cl(P))[0]
    else:
        yard = torch.autograd.grad(F.conv3d(_cl(P), w0, stride=stride, padding=int(ks == 3)), w0, _cl(Q))[0]
    yard = yard.reshape(CB, CA, T)
    if c.swapped:
        ref, yard, (sa, sb) = ref.permute(1, 0, 2), yard.permute(1, 0, 2), (CB * T, T)
    else:
        sa, sb = T, CA * T
    ref, yard = ref.contiguous(), yard.contiguous()
    scale = float(ref.abs().max())
    prior = (_noise(1012, fig.name + '/dw0', tuple(ref.shape)) * scale * 0.5).to(dev)

    Pd, Qd = P.to(dev), Q.to(dev)
    Pg = Guarded(P.numel(), _guard(c.H, c.W, CA), dev, fill=Pd)
    Qg = Guarded(Q.numel(), _guard(qd[1], qd[2], CB), dev, fill=Qd)
    nfl = E.query('seg3d_wgrad_direct_workspace_floats', c.N, qd[0], qd[1], qd[2], CA, CB, T)
    CBP = _round4(CB)
    used = c.chunks * T * CA * CBP
    assert used <= nfl

    def run(accumulate):
        tag = ' (accumulate = {})'.format(accumulate)
        part = Guarded(nfl, 4096, dev)
        dw = Guarded(ref.numel(), _round4(1024 * T), dev, fill=prior if accumulate else None)
        n_chunks = ctypes.c_int(-7)
        E.call('seg3d_wgrad_direct', E.ptr(Pg.t), E.ptr(Qg.t), E.ptr(part.t), *args, ctypes.byref(n_chunks), E.stream_ptr())
        torch.cuda.synchronize()
        assert n_chunks.value == c.chunks
        slabs = part.t[:used].reshape(-1, CBP)
        fig.require(part.guards_untouched(), 'part: the guard bands were written' + tag)
        fig.require(not bool(torch.isnan(slabs).any()), 'part: an entry of a reported chunk was not written' + tag)
        fig.require(bool((slabs[:, CB:] == 0.0).all()), 'part: a padded column is not 0.0' + tag)
        fig.require(bool(torch.isnan(part.t[used:]).all()), 'part: written beyond the reported chunks' + tag)
        E.call('seg3d_wgrad_reduce', E.ptr(part.t), E.ptr(dw.t), n_chunks.value, T, CA, CB, sa, sb, accumulate, E.stream_ptr())
        torch.cuda.synchronize()
        fig.require(dw.guards_untouched(), 'dw: the guard bands were written' + tag)
        return dw, part

    (dw, part), (dw2, part2) = run(0), run(0)
    fig.require(torch.equal(_bits(dw.t), _bits(dw2.t)) and torch.equal(_bits(part.t[:used]), _bits(part2.t[:used])),
                'the second call differs')
    got, yard_ = dw.t, yard
    if c.accumulate:
        acc, _ = run(1)
        fig.require(torch.equal(_bits(acc.t), _bits(prior.reshape(-1) + dw.t)), 'dw: the accumulating call is not base + plain')
        got, ref, yard_ = acc.t, ref + prior.double(), yard + prior.cpu()
    fig.check('dw', got, ref.reshape(-1), yard_.reshape(-1), FLOOR_RED, cap=CAP_DW_REL * scale)
    fig.require(_same(Pg, Pd) and _same(Qg, Qd), 'P or Q was written')
    _finish(fig, t0)


@pytest.mark.parametrize('args,why', K.REFUSALS, ids=[r[1] for r in K.REFUSALS])
def test_wgrad_refusals_write_nothing(hip_device, args, why):
    """arguments the launcher refuses on the host: an error with its name in front, no launch, the workspace and the count untouched"""
    E, dev = _engine(), hip_device
    assert E.query('seg3d_wgrad_direct_variant', *args) < 0
    ones = torch.ones(1 << 14, device=dev)
    part = Guarded(1 << 16, 4096, dev)
    n_chunks = ctypes.c_int(-7)
    with pytest.raises((ValueError, NotImplementedError)) as info:
        E.call('seg3d_wgrad_direct', E.ptr(ones), E.ptr(ones), E.ptr(part.t), *args, ctypes.byref(n_chunks), E.stream_ptr())
    assert str(info.value).startswith('seg3d_wgrad_direct:'), (why, str(info.value))
    torch.cuda.synchronize()
    assert part.all_nan() and part.guards_untouched() and n_chunks.value == -7, why


# ---- the reducers on their own ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('swapped', [False, True], ids=['dw_bat', 'dw_abt'])
@pytest.mark.parametrize('tab', K.REDUCE_TAB, ids=lambda v: 'x'.join(str(i) for i in v))
@pytest.mark.parametrize('chunks', K.REDUCE_CHUNKS)
def test_reduce_alone(hip_device, chunks, tab, swapped):
    """a synthetic part of small integers (every summation order is exact in fp32) whose padded columns are NaN -- the reducers never
    read them; dw = the float64 sum over the chunks, exactly, in both layouts, with and without a base"""
    E, dev = _engine(), hip_device
    T, A, B = tab
    BP = _round4(B)
    wide = int(chunks >= 512 and T * A * B <= 2048)
    assert E.query('seg3d_wgrad_reduce_variant', chunks, T, A, B) == wide
    name = 'direct/reduce/{}-{}x{}x{}-{}'.format(chunks, T, A, B, 'abt' if swapped else 'bat')
    vals = torch.round(_noise(1020, name, (chunks, T, A, BP)) * 4.0)
    ref = vals[..., :B].double().sum(0)                                        # [t][a][b]
    vals[..., B:] = NAN
    ref = (ref.permute(1, 2, 0) if swapped else ref.permute(2, 1, 0)).contiguous().reshape(-1)
    sa, sb = (B * T, T) if swapped else (T, A * T)
    base = torch.round(_noise(1021, name + '/base', (T * A * B,)) * 100.0)
    part = Guarded(vals.numel(), 4096, dev, fill=vals.to(dev))
    part_before = part.buf.clone()
    for accumulate in (0, 1):
        dw = Guarded(T * A * B, 1024, dev, fill=base.to(dev) if accumulate else None)
        E.call('seg3d_wgrad_reduce', E.ptr(part.t), E.ptr(dw.t), chunks, T, A, B, sa, sb, accumulate, E.stream_ptr())
        torch.cuda.synchronize()
        assert dw.guards_untouched()
        want = ref + base.double() if accumulate else ref
        assert torch.equal(dw.t.cpu().double(), want), 'accumulate = {}: {} of {} outputs differ'.format(
            accumulate, int((dw.t.cpu().double() != want).sum()), want.numel())
    assert torch.equal(_bits(part.buf), _bits(part_before))
    report(name, wide=float(wide), exact=1.0)


# ---- the tap-major packer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,A,B', K.PACK_CASES)
def test_pack_tapmajor(hip_device, T, A, B):
    """wp[t][a][bp] = W(a, b, flip ? T - 1 - t : t), zero for bp >= B: bit for bit, both orientations of w, flip 0 and 1, BP =
    round_up(B, 4) and one quad more"""
    E, dev = _engine(), hip_device
    for oriented_ba in (True, False):
        shape, (sa, sb) = ((B, A, T), (T, A * T)) if oriented_ba else ((A, B, T), (B * T, T))
        w = _noise(1030, 'direct/pack/{}-{}-{}-{}'.format(T, A, B, int(oriented_ba)), shape)
        Wabt = w.numpy().transpose(1, 0, 2) if oriented_ba else w.numpy()
        wg = Guarded(w.numel(), 1024, dev, fill=w.to(dev))
        for flip in (0, 1):
            for BP in (_round4(B), _round4(B) + 4):
                want = np.zeros((T, A, BP), dtype=np.float32)
                want[:, :, :B] = (Wabt[:, :, ::-1] if flip else Wabt).transpose(2, 0, 1)
                wp = Guarded(T * A * BP, 1024, dev)
                E.call('seg3d_pack_weights_tapmajor', E.ptr(wg.t), E.ptr(wp.t), A, B, BP, T, sa, sb, flip, E.stream_ptr())
                torch.cuda.synchronize()
                assert wp.guards_untouched() and _same(wg, w.to(dev))
                got = wp.t.cpu().numpy().reshape(T, A, BP)
                assert np.array_equal(got.view(np.int32), want.view(np.int32)), (oriented_ba, flip, BP)
    report('direct/pack/{}-{}-{}'.format(T, A, B), exact=1.0)


# ---- the head's per-voxel tail -------------------------------------------------------------------------------------------------------------
def _logits(c, name):
    """N(0, 2^2) per sample around its own mean, plus: a row of equal values, a row spread over +-80, saturated and nearly saturated
    sigmoid inputs; each in another sample, the last voxel of the last sample included"""
    x = _activation(1040, name + '/x', c.N, (1, 1, c.S), c.C).reshape(c.N, c.S, c.C)
    x[0, 0, :] = 1.25
    x[0, 1, :] = torch.linspace(-80.0, 80.0, c.C) if c.C > 1 else -80.0
    sign = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(c.C)])
    x[1, 2, :] = 100.0 * sign
    x[1, c.S - 1, :] = -100.0 * sign
    x[2, 3, :] = 20.0 * sign
    x[2, c.S - 1, :] = -17.0 * sign
    return x


@pytest.mark.parametrize('case', K.TAIL_CASES, ids=K.case_id)
def test_head_tail(hip_device, case):
    E, c, dev, t0 = _engine(), case, hip_device, time.perf_counter()
    fig = Figures('direct/{}/{}'.format(c.op, K.case_id(c)))
    op = (lambda t: torch.softmax(t, -1)) if c.op == 'softmax' else torch.sigmoid
    x = _logits(c, fig.name)
    g = _noise(1041, fig.name + '/g', (c.N, c.S, c.C)) + 0.25
    refs = []
    for dt in (torch.float64, torch.float32):       # the reference, then the yardstick
        xl = x.clone().to(dt).requires_grad_(True)
        p = op(xl)
        (dx,) = torch.autograd.grad(p, (xl,), g.to(dt))
        refs.append((p.detach().permute(0, 2, 1).contiguous(), dx))             # probabilities are [N][C][S]
    (p_ref, dx_ref), (p_yard, dx_yard) = [(a.to(dev), b.to(dev)) for (a, b) in refs[:1]] + refs[1:]
    xd, gd = x.to(dev), g.permute(0, 2, 1).contiguous().to(dev)
    xg = Guarded(x.numel(), _round4(1024 * c.C), dev, fill=xd)
    gg = Guarded(g.numel(), _round4(1024 * c.C), dev, fill=gd)

    def run():
        p = Guarded(x.numel(), _round4(1024 * c.C), dev)
        din = Guarded(x.numel(), _round4(1024 * c.C), dev)
        E.call('seg3d_{}_fwd'.format(c.op), E.ptr(xg.t), E.ptr(p.t), c.N, c.C, c.S, E.stream_ptr())
        E.call('seg3d_{}_bwd'.format(c.op), E.ptr(p.t), E.ptr(gg.t), E.ptr(din.t), c.N, c.C, c.S, E.stream_ptr())
        torch.cuda.synchronize()
        fig.require(p.guards_untouched() and din.guards_untouched(), 'the guard bands of an output were written')
        return p, din

    (p, din), (p2, din2) = run(), run()
    fig.check('p', p.t, p_ref.reshape(-1), p_yard.reshape(-1), FLOOR_EW, cap=CAP_P_ABS)
    fig.check('din', din.t, dx_ref.reshape(-1), dx_yard.reshape(-1), FLOOR_EW, cap=CAP_DIN_REL * float(dx_ref.abs().max()))
    fig.require(torch.equal(_bits(p.t), _bits(p2.t)) and torch.equal(_bits(din.t), _bits(din2.t)), 'the second call differs')
    fig.require(bool(torch.isfinite(p.t).all()) and bool(((p.t >= 0.0) & (p.t <= 1.0)).all()), 'a probability is not in [0, 1]')
    if c.op == 'softmax':
        rows = p.t.reshape(c.N, c.C, c.S).double().sum(1)
        fig.figs['row_sum_err'] = float((rows - 1.0).abs().max())
        fig.require(fig.figs['row_sum_err'] <= c.C * fig.figs.get('p_bar', 0.0), 'a soft-max row does not sum to 1')
        if c.C == 1:
            fig.require(bool((p.t == 1.0).all()) and bool((din.t == 0.0).all()), 'C = 1: p is not 1.0 or its gradient not 0.0')
    fig.require(_same(xg, xd) and _same(gg, gd), 'an input was written')
    _finish(fig, t0)
