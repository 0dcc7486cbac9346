"""Every reachable kernel of csrc/conv_mfma.hip (direct 3x3x3: forward / data gradient and weight gradient, fp32 and bf16,
whole-K and split-K with its finish pass), driven through the C ABI, against a plain float64 reference.  The cases are those of
tests/k3_cases.py; each one first asserts through the variant, workspace and statistics queries that it reaches the kernels it is
named for (code, split-K or not, more or fewer work items than the persistent grid).

Layout: NDHWC activations, weights [Cout][Cin][3][3][3], t = (kz * 3 + ky) * 3 + kx, packed with T = 27.

Reference: float64 on the device, from the definition, as 27 shifted matmuls on a zero-padded input:
    forward   y[n,z,y,x,o] = bias[o] + sum_{kz,ky,kx,c} xpad[n,z+kz,y+ky,x+kx,c] w[o,c,kz,ky,kx]   (+ addend)
    dgrad     the same with the taps flipped and Cin / Cout transposed (flip = 1 pack of the forward layer's weight)
    wgrad     dw[o,c,t] = sum_{n,v} xpad[n,v+t,c] dy[n,v,o]                                          (+ the prior value)
on operands rounded the way the mode rounds them (bf16: x, w and dy; the addend stays fp32).  The GroupNorm statistics slots are
summed over the slot axis and compared with sum y and sum y^2 of the float64 result.

Bars: nothing is pinned to what the kernels give.  Each case also runs the same operation in fp32 on the CPU (F.conv3d, autograd
for the weight gradient): the yardstick.  Element-wise outputs: err <= 4 * yardstick + 2e-6 * scale, scale = max|ref|; statistics
sums and weight gradients: 4 * yardstick + 1e-5 * scale.  The bars of the existing tests hold on top as caps: 1e-4 absolute for
fp32 outputs, 2e-5 * scale for the outputs of the bf16 kernels, 1e-5 for the statistics (sum against sum|y|, squares relative),
2e-4 * scale for fp32 and 2e-5 * scale for bf16 weight gradients.  bf16-stored outputs, per element: |got - ref| <= 2^-8 |ref| +
(the fp32 bar).

Write discipline: y, the statistics, dw (an accumulating call: known values) and both workspaces are NaN-filled inside NaN guard
bands of at least one tile of rows (512 Cout floats for y; 27 * 1024 for dw); the guards must come back bit-identical, no NaN may
survive inside, and a second call on the same inputs must be bit-identical.

Largest err / bar per kernel, MI355X (y: outputs, st: statistics; a run appends every figure to the parity report that
gpu_util.report writes; the yardstick itself stayed below 3.5e-6 * scale):
    fp32 mfma<1> y 0.12 st 0.01, split-K 0.17 / 0.01;  <2> 0.13;  <3> 0.12;  <4> 0.12
    fp32 mfma2<1,1> y 0.16 st 0.01, split-K 0.11;  <1,2> 0.13, split-K 0.12;  <2,1> split-K 0.07;  <2,2> 0.18, split-K 0.08;
         <3,1> 0.21, split-K 0.07;  <4,1> split-K 0.09;  mfma2w8<1,1> 0.13;  <2,1> 0.20                  (st at most 0.01)
    bf16 mfma2_bf16<1,1> y 0.06, split-K 0.05;  <1,2> split-K 0.03;  <2,1> split-K 0.03;  <2,2> 0.10, split-K 0.03;
         <3,1> split-K 0.03;  <4,1> split-K 0.03;  mfma2w8_bf16<1,1> 0.06;  <2,1> 0.09                   (st at most 0.01)
    weight gradient, reduce<4> / reduce<16>:  wgrad2 4x4x8 0.03 / 0.02;  4x4x4 0.02 / 0.02;  2x6x6 0.03 / 0.02;
         wgrad3<8> 0.01 / 0.02;  <8, IRR> 0.01 / 0.01;  <4> 0.01 / 0.02;  <4, IRR> 0.01 / 0.01;  widening 0.02 / 0.01
"""
import pytest
import torch
import torch.nn.functional as F

import k3_cases as K
from float64_util import (FLOOR_EW, FLOOR_RED, Figures, Guarded, _activation, _check_stats, _conv_def, _engine, _noise, _weight,
                          _wgrad_def, bf16_round)

pytestmark = pytest.mark.gpu

CAP_Y_ABS, CAP_Y_BF16_REL, CAP_WGRAD_REL, CAP_WGRAD_BF16_REL = 1e-4, 2e-5, 2e-4, 2e-5


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _pack27(E, w, A, B, sa, sb, flip, bf16):
    if bf16:
        wp = torch.empty(E.query('seg3d_packed_mfma_bf16_elems', A, B, 27), dtype=torch.bfloat16, device=w.device)
        E.call('seg3d_pack_weights_mfma_bf16', E.ptr(w), E.ptr(wp), A, B, 27, sa, sb, flip, E.stream_ptr())
    else:
        wp = torch.empty(E.query('seg3d_packed_mfma_floats', A, B, 27), dtype=torch.float32, device=w.device)
        E.call('seg3d_pack_weights_mfma', E.ptr(w), E.ptr(wp), A, B, 27, sa, sb, flip, E.stream_ptr())
    return wp


def _fwd_call(E, c, xd, wp, bd, ad, y, stats, ws):
    args = (E.ptr(xd), E.ptr(wp), E.ptr(bd), E.ptr(ad), E.ptr(y.t), E.ptr(stats.t) if stats else None, E.ptr(ws.t) if ws else None,
            c.N, c.D, c.H, c.W, c.Cin, c.Cout)
    if c.bf16:
        E.call('seg3d_conv3d_k3_bf16_fwd', *args, c.out_bf16, E.stream_ptr())
    else:
        E.call('seg3d_conv3d_k3_mfma_fwd', *args, E.stream_ptr())


# ---- forward / data gradient ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.FWD_CASES, ids=K.case_id)
def test_fwd(hip_device, case):
    E, c, dev = _engine(), case, hip_device
    t = 'bf16' if c.bf16 else 'mfma'
    dims = (c.N, c.D, c.H, c.W, c.Cin, c.Cout)
    nws = E.query('seg3d_conv3d_k3_{}_fwd_workspace_floats'.format(t), *dims)
    cnt = E.query('seg3d_conv3d_k3_{}_stats_count'.format(t), *dims)
    assert E.query('seg3d_conv3d_k3_{}_variant'.format(t), *dims) == K.fwd_code(c) and (nws > 0) == c.splitk
    if K.persistent(c):
        items = c.N * cnt // K.waves(c)
        assert (items > K.CUS and items % K.CUS != 0) if K.ITEM_CLASS[c] == 'many' else items < K.CUS
    fig = Figures(K.case_id(c))
    A, B, fwd, sp = c.Cin, c.Cout, c.role == 'fwd', (c.D, c.H, c.W)
    x = _activation(930, fig.name + '/x', c.N, sp, A)
    # 'fwd': w[b][a][t]; 'dgrad': the forward layer's weight w[a][b][t], read with flipped taps
    w = _weight(931, fig.name + '/w', (B, A, 3, 3, 3) if fwd else (A, B, 3, 3, 3), 27 * A)
    bias = (0.3 * _noise(932, fig.name + '/b', (B,)) + 0.2) if c.bias else None
    addend = _activation(933, fig.name + '/add', c.N, sp, B, offset=0.5) if c.addend else None
    if c.bf16:
        x, w = bf16_round(x), bf16_round(w)
    weff = w if fwd else w.transpose(0, 1).flip(2, 3, 4).contiguous()
    sa, sb, flip = (27, 27 * A, 0) if fwd else (27 * B, 27, 1)
    # float64 reference (device) and fp32 yardstick (CPU)
    ref = _conv_def(x.to(dev).double(), weff.to(dev).double())
    yard = F.conv3d(x.permute(0, 4, 1, 2, 3), weff, bias, padding=1).permute(0, 2, 3, 4, 1)
    if c.bias:
        ref = ref + bias.to(dev).double()
    if c.addend:
        ref = ref + addend.to(dev).double()
        yard = yard + addend
    # device operands
    xd = x.to(dev).bfloat16() if c.bf16 else x.to(dev)
    wp = _pack27(E, w.to(dev), A, B, sa, sb, flip, bool(c.bf16))
    bd = bias.to(dev) if c.bias else None
    ad = addend.to(dev) if c.addend else None
    ydt = torch.bfloat16 if c.out_bf16 else torch.float32
    runs = []
    for _ in range(2):
        y = Guarded(ref.numel(), 512 * B, dev, ydt)
        stats = Guarded(c.N * cnt * 2, 1024, dev) if fwd else None
        ws = Guarded(nws, 512 * B, dev) if nws else None
        _fwd_call(E, c, xd, wp, bd, ad, y, stats, ws)
        torch.cuda.synchronize()
        runs.append((y, stats, ws))
    y, stats, ws = runs[0]
    fig.require(y.guards_untouched(), 'y: the guard bands were written')
    fig.require(ws is None or ws.guards_untouched(), 'workspace: the guard bands were written')
    scale = float(ref.abs().max())
    fig.check('y', y.t, ref.reshape(-1), yard.reshape(-1), FLOOR_EW, cap=CAP_Y_BF16_REL * scale if c.bf16 else CAP_Y_ABS,
              bf16_out=bool(c.out_bf16))
    if fwd:
        _check_stats(fig, stats, ref, yard, c.N)
    # a second call on the same inputs: bit-identical
    y2, stats2, ws2 = runs[1]
    fig.require(torch.equal(_bits(y.t), _bits(y2.t)), 'y: the second call differs')
    fig.require(y2.guards_untouched() and (ws2 is None or ws2.guards_untouched()), 'second call: the guard bands were written')
    if fwd:
        fig.require(torch.equal(_bits(stats.t), _bits(stats2.t)), 'stats: the second call differs')
    fig.done()


# ---- weight gradient -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.WGRAD_CASES, ids=K.case_id)
def test_wgrad(hip_device, case):
    E, c, dev = _engine(), case, hip_device
    dims = (c.N, c.D, c.H, c.W, c.Cin, c.Cout)
    assert E.query('seg3d_conv3d_k3_wgrad_variant', *dims, c.bf16) == K.wgrad_code(c)
    nws = E.query('seg3d_conv3d_k3_{}_wgrad_workspace_floats'.format('bf16' if c.bf16 else 'mfma'), *dims)
    npairs = ((c.Cin + 31) // 32) * ((c.Cout + 31) // 32)
    assert (nws // (npairs * 27 * 1024) >= 32) == (c.reducer == 16)
    fig = Figures(K.case_id(c))
    sp = (c.D, c.H, c.W)
    x = _activation(940, fig.name + '/x', c.N, sp, c.Cin, offset=0.25)
    dy = _activation(941, fig.name + '/dy', c.N, sp, c.Cout, offset=0.0)
    if c.bf16:
        x, dy = bf16_round(x), bf16_round(dy)
    ref = _wgrad_def(x.to(dev).double(), dy.to(dev).double())                       # [Cout][Cin][27]: the layout dw is written in
    w0 = torch.zeros(c.Cout, c.Cin, 3, 3, 3, requires_grad=True)
    yard = torch.autograd.grad(F.conv3d(x.permute(0, 4, 1, 2, 3), w0, padding=1), w0, dy.permute(0, 4, 1, 2, 3))[0]
    yard = yard.reshape(c.Cout, c.Cin, 27)
    prior = None
    if c.accumulate:
        prior = _noise(942, fig.name + '/dw0', tuple(ref.shape)) * float(ref.abs().max()) * 0.5
        ref = ref + prior.to(dev).double()
        yard = yard + prior
    xd, dyd = (x.to(dev).bfloat16(), dy.to(dev).bfloat16()) if c.bf16 else (x.to(dev), dy.to(dev))
    runs = []
    for _ in range(2):
        dw = Guarded(ref.numel(), 27 * 1024, dev, fill=prior.to(dev) if c.accumulate else None)
        ws = Guarded(nws, 27 * 1024, dev)
        E.call('seg3d_conv3d_k3_bf16_wgrad' if c.bf16 else 'seg3d_conv3d_k3_mfma_wgrad', E.ptr(xd), E.ptr(dyd), E.ptr(dw.t),
               E.ptr(ws.t), *dims, c.accumulate, E.stream_ptr())
        torch.cuda.synchronize()
        runs.append((dw, ws))
    (dw, ws), (dw2, ws2) = runs
    fig.require(dw.guards_untouched() and dw2.guards_untouched(), 'dw: the guard bands were written')
    fig.require(ws.guards_untouched() and ws2.guards_untouched(), 'workspace: the guard bands were written')
    scale = float(ref.abs().max())
    fig.check('dw', dw.t, ref.reshape(-1), yard.reshape(-1), FLOOR_RED, cap=(CAP_WGRAD_BF16_REL if c.bf16 else CAP_WGRAD_REL) * scale)
    fig.require(torch.equal(_bits(dw.t), _bits(dw2.t)), 'dw: the second call differs')
    fig.done()


# ---- refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family,dims,why', K.REFUSALS, ids=[r[2] for r in K.REFUSALS])
def test_refusals_write_nothing(hip_device, family, dims, why):
    """arguments outside the kernels' contract: non-zero return with a message; y, the statistics and the workspace stay NaN"""
    E, dev = _engine(), hip_device
    N, D, H, W, A, B = dims
    bf16 = family.startswith('bf16')
    x = torch.ones((N, D, H, W, A + 4), dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)
    wp = torch.zeros(1 << 20, dtype=torch.float32, device=dev)              # ample for any image of these channel counts
    bias = torch.zeros(B + 4, device=dev)
    y = Guarded(N * D * H * W * (B + 4), 512 * 8, dev)
    stats = Guarded(1 << 14, 1024, dev)
    ws = None if family.endswith('_no_ws') else Guarded(16 * N * D * H * W * (B + 4), 512 * 8, dev)
    args = (E.ptr(x), E.ptr(wp), E.ptr(bias), None, E.ptr(y.t), E.ptr(stats.t), E.ptr(ws.t) if ws else None, *dims)
    with pytest.raises(ValueError):
        if bf16:
            E.call('seg3d_conv3d_k3_bf16_fwd', *args, 0, E.stream_ptr())
        else:
            E.call('seg3d_conv3d_k3_mfma_fwd', *args, E.stream_ptr())
    assert E.last_error(), why
    torch.cuda.synchronize()
    assert y.all_nan() and y.guards_untouched() and stats.all_nan() and stats.guards_untouched(), why
    assert ws is None or (ws.all_nan() and ws.guards_untouched()), why
