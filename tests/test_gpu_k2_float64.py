"""Every kernel instantiation of csrc/conv_k2_mfma.hip (stride-2 2x2x2 gather, scatter and weight gradient), driven through the
C ABI, against a plain float64 reference.  The cases are those of tests/k2_cases.py; each one first asserts through the
seg3d_*k2*_variant queries that it reaches the instantiation it is named for.

Layout: NDHWC activations; W(a, b, t) = w[a * sa + b * sb + t], t = (kz * 2 + ky) * 2 + kx, packed with T = 8.

Reference: float64 einsums over the 2^3 cells (on the device), written from the three formulas of the kernel file's header:
    gather   y[v][b]      = bias[b] + sum_{t,a} x[2v + t][a] W(a,b,t)
    scatter  y[2i + t][b] = bias[b] + sum_a x[i][a] W(a,b,t)  (+ addend)
    wgrad    dW(t,a,b)    = sum_v P[2v + t][a] Q[v][b]
on operands rounded the way the mode rounds them (modes 1, 2: bf16 x; mode 2: bf16 W; bf16 weight gradient: bf16 P and Q; a
bf16 addend).  The GroupNorm statistics slots are summed over the slot axis and compared with sum y and sum y^2 of the float64
result (the kernels take them from the fp32 value in front of any bf16 rounding of y).

Bars: nothing is pinned to what the kernels give.  Each case also runs the same operation in fp32 on the CPU (F.conv3d,
F.conv_transpose3d, autograd for the weight gradient): the yardstick.  Element-wise outputs: err <= 4 * yardstick + 2e-6 * scale,
scale = max|ref|; statistics sums and weight gradients: 4 * yardstick + 1e-5 * scale.  The bars of the existing stride-2 tests
hold on top: 2e-6 * scale + 1e-6 for fp32 outputs, 1e-5 for the statistics (sum against sum|y|, squares relative), 2e-5
relative for the bf16 weight gradient.  bf16-stored outputs, per element: |got - ref| <= 2^-8 |ref| + (the fp32 bar).

Write discipline: outputs are NaN-filled (dw of an accumulating call: known values) inside NaN guard bands of at least a tile's
rows on both sides; the guards must come back bit-identical and no NaN may survive inside.  Channel-slice operands (x of
_fwd_ld, addends) live in wider buffers whose other channels are NaN.
"""
import pytest
import torch
import torch.nn.functional as F

import k2_cases as K
from float64_util import (FLOOR_EW, FLOOR_RED, Figures, Guarded, _activation, _check_stats, _engine, _k2_gather_def, _k2_scatter_def,
                          _k2_wgrad_def, _noise, _weight, _wide_slice, bf16_round)

pytestmark = pytest.mark.gpu

CAP_EW_REL, CAP_EW_ABS, CAP_WGRAD_BF16 = 2e-6, 1e-6, 2e-5


def _check_output(fig, y, ref, yard, out_bf16):
    fig.require(y.guards_untouched(), 'y: the guard bands were written')
    scale = float(ref.abs().max())
    fig.check('y', y.t, ref.reshape(-1), yard.reshape(-1), FLOOR_EW, cap=CAP_EW_REL * scale + CAP_EW_ABS, bf16_out=bool(out_bf16))


def _pack(E, w, A, B, sa, sb, bf16):
    if bf16:
        wp = torch.empty(E.query('seg3d_packed_mfma_bf16_elems', A, B, 8), dtype=torch.bfloat16, device=w.device)
        E.call('seg3d_pack_weights_mfma_bf16', E.ptr(w), E.ptr(wp), A, B, 8, sa, sb, 0, E.stream_ptr())
    else:
        wp = torch.empty(E.query('seg3d_packed_mfma_floats', A, B, 8), dtype=torch.float32, device=w.device)
        E.call('seg3d_pack_weights_mfma', E.ptr(w), E.ptr(wp), A, B, 8, sa, sb, 0, E.stream_ptr())
    return wp


# ---- gather --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.GATHER_CASES, ids=K.case_id)
def test_gather(hip_device, case):
    E, c, dev = _engine(), case, hip_device
    assert E.query('seg3d_conv3d_k2s2_variant', c.N, c.D, c.H, c.W, c.Cin, c.Cout, c.mode, c.out_bf16) == K.gather_code(c)
    fig = Figures(K.case_id(c))
    A, B, fwd = c.Cin, c.Cout, c.role == 'fwd'
    x = _activation(900, fig.name + '/x', c.N, (2 * c.D, 2 * c.H, 2 * c.W), A)
    w = _weight(901, fig.name + '/w', (B, A, 2, 2, 2), 8 * A)              # w[b][a][t]: sa = 8, sb = 8 A
    bias = (0.3 * _noise(902, fig.name + '/b', (B,)) + 0.2) if fwd else None
    if c.mode:
        x = bf16_round(x)
    wr = bf16_round(w) if c.mode == 2 else w
    # float64 reference (device) and fp32 yardstick (CPU)
    ref = _k2_gather_def(x.to(dev).double(), wr.to(dev).double())
    yard = F.conv3d(x.permute(0, 4, 1, 2, 3), wr, bias, stride=2).permute(0, 2, 3, 4, 1)
    if fwd:
        ref = ref + bias.to(dev).double()
    # device operands
    if c.ld_x:
        wide, xd = _wide_slice(x, c.ld_x, dev)
    else:
        xd = x.to(dev).bfloat16() if c.mode else x.to(dev)
    wd = w.to(dev)
    wp = _pack(E, wd, A, B, 8, 8 * A, c.mode == 2)
    bd = bias.to(dev) if fwd else None
    y = Guarded(ref.numel(), 128 * B, dev, torch.bfloat16 if c.out_bf16 else torch.float32)
    stats = None
    if fwd:
        cnt = E.query('seg3d_conv3d_k2s2_mfma_stats_count', c.D, c.H, c.W, B)
        stats = Guarded(c.N * cnt * 2, 1024, dev)
    dims = (c.N, c.D, c.H, c.W, A, B)
    sp = E.ptr(stats.t) if fwd else None
    if c.mode:
        E.call('seg3d_conv3d_k2s2_bf16_fwd', E.ptr(xd), E.ptr(wp), E.ptr(bd), E.ptr(y.t), sp, *dims, c.out_bf16, int(c.mode == 2),
               E.stream_ptr())
    elif c.ld_x:
        E.call('seg3d_conv3d_k2s2_mfma_fwd_ld', E.ptr(xd), c.ld_x, E.ptr(wp), E.ptr(bd), E.ptr(y.t), sp, *dims, E.stream_ptr())
    else:
        E.call('seg3d_conv3d_k2s2_mfma_fwd', E.ptr(xd), E.ptr(wp), E.ptr(bd), E.ptr(y.t), sp, *dims, E.stream_ptr())
    torch.cuda.synchronize()
    _check_output(fig, y, ref, yard, c.out_bf16)
    if fwd:
        _check_stats(fig, stats, ref, yard, c.N)
    fig.done()


# ---- scatter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.SCATTER_CASES, ids=K.case_id)
def test_scatter(hip_device, case):
    E, c, dev = _engine(), case, hip_device
    assert E.query('seg3d_convT3d_k2s2_variant', c.N, c.D, c.H, c.W, c.Cin, c.Cout, c.mode, c.out_bf16, int(c.add),
                   c.ld_addend) == K.scatter_code(c)
    fig = Figures(K.case_id(c))
    A, B, fwd = c.Cin, c.Cout, c.role == 'fwd'
    x = _activation(910, fig.name + '/x', c.N, (c.D, c.H, c.W), A)
    w = _weight(911, fig.name + '/w', (A, B, 2, 2, 2), A)                  # w[a][b][t]: sa = 8 B, sb = 8
    bias = (0.3 * _noise(912, fig.name + '/b', (B,)) + 0.2) if fwd else None
    if c.mode:
        x = bf16_round(x)
    wr = bf16_round(w) if c.mode == 2 else w
    ref = _k2_scatter_def(x.to(dev).double(), wr.to(dev).double())
    yard = F.conv_transpose3d(x.permute(0, 4, 1, 2, 3), wr, bias, stride=2).permute(0, 2, 3, 4, 1)
    if fwd:
        ref = ref + bias.to(dev).double()
    addend = None
    if c.add:
        addend = _activation(913, fig.name + '/add', c.N, (2 * c.D, 2 * c.H, 2 * c.W), B, offset=0.5)
        if c.out_bf16:
            addend = bf16_round(addend)
        ref = ref + addend.to(dev).double()
        yard = yard + addend
        wide, ad = _wide_slice(addend.bfloat16() if c.out_bf16 else addend, c.ld_addend, dev)
    xd = x.to(dev).bfloat16() if c.mode else x.to(dev)
    wp = _pack(E, w.to(dev), A, B, 8 * B, 8, c.mode == 2)
    bd = bias.to(dev) if fwd else None
    y = Guarded(ref.numel(), 1024 * B, dev, torch.bfloat16 if c.out_bf16 else torch.float32)
    stats = None
    if fwd:
        cnt = E.query('seg3d_convT3d_k2s2_mfma_stats_count', c.D, c.H, c.W, B)
        stats = Guarded(c.N * cnt * 2, 1024, dev)
    dims = (c.N, c.D, c.H, c.W, A, B)
    sp = E.ptr(stats.t) if fwd else None
    if c.add:
        E.call('seg3d_convT3d_k2s2_scatter_addend', E.ptr(xd), c.mode, E.ptr(wp), E.ptr(ad), c.ld_addend, E.ptr(y.t), *dims,
               c.out_bf16, E.stream_ptr())
    elif c.mode:
        E.call('seg3d_convT3d_k2s2_bf16_fwd', E.ptr(xd), E.ptr(wp), E.ptr(bd), E.ptr(y.t), sp, *dims, c.out_bf16, int(c.mode == 2),
               E.stream_ptr())
    else:
        E.call('seg3d_convT3d_k2s2_mfma_fwd', E.ptr(xd), E.ptr(wp), E.ptr(bd), E.ptr(y.t), sp, *dims, E.stream_ptr())
    torch.cuda.synchronize()
    _check_output(fig, y, ref, yard, c.out_bf16)
    if fwd:
        _check_stats(fig, stats, ref, yard, c.N)
    fig.done()


# ---- weight gradient -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.WGRAD_CASES, ids=K.case_id)
def test_wgrad(hip_device, case):
    E, c, dev = _engine(), case, hip_device
    assert E.query('seg3d_k2_wgrad_variant', c.N, c.D, c.H, c.W, c.CA, c.CB, c.bf16) == K.wgrad_code(c)
    fig = Figures(K.case_id(c))
    CA, CB = c.CA, c.CB
    P = _activation(920, fig.name + '/P', c.N, (2 * c.D, 2 * c.H, 2 * c.W), CA, offset=0.25)
    Q = _activation(921, fig.name + '/Q', c.N, (c.D, c.H, c.W), CB, offset=0.0)
    if c.bf16:
        P, Q = bf16_round(P), bf16_round(Q)
    ref = _k2_wgrad_def(P.to(dev).double(), Q.to(dev).double())                                   # dW(a, b, t)
    w0 = torch.zeros(CB, CA, 2, 2, 2, requires_grad=True)
    yard = torch.autograd.grad(F.conv3d(P.permute(0, 4, 1, 2, 3), w0, stride=2), w0, Q.permute(0, 4, 1, 2, 3))[0]
    yard = yard.reshape(CB, CA, 8).permute(1, 0, 2)
    if c.swapped:
        sa, sb = 8 * CB, 8                                                   # dw[a][b][t]
    else:
        sa, sb = 8, 8 * CA                                                   # dw[b][a][t], as the reference stores a Conv3d weight
        ref, yard = ref.permute(1, 0, 2), yard.permute(1, 0, 2)
    ref, yard = ref.contiguous(), yard.contiguous()
    prior = None
    if c.accumulate:
        prior = _noise(922, fig.name + '/dw0', tuple(ref.shape)) * float(ref.abs().max()) * 0.5
        ref = ref + prior.to(dev).double()
        yard = yard + prior
    dw = Guarded(ref.numel(), 8 * 1024, dev, fill=prior.to(dev) if c.accumulate else None)
    nws = E.query('seg3d_k2_mfma_wgrad_workspace_floats', c.N, c.D, c.H, c.W, CA, CB)
    ws = Guarded(nws, 8 * 1024, dev)
    Pd, Qd = (P.to(dev).bfloat16(), Q.to(dev).bfloat16()) if c.bf16 else (P.to(dev), Q.to(dev))
    E.call('seg3d_k2_bf16_wgrad' if c.bf16 else 'seg3d_k2_mfma_wgrad', E.ptr(Pd), E.ptr(Qd), E.ptr(dw.t), E.ptr(ws.t), c.N, c.D,
           c.H, c.W, CA, CB, sa, sb, c.accumulate, E.stream_ptr())
    torch.cuda.synchronize()
    fig.require(dw.guards_untouched(), 'dw: the guard bands were written')
    fig.require(ws.guards_untouched(), 'workspace: the guard bands were written')
    scale = float(ref.abs().max())
    fig.check('dw', dw.t, ref.reshape(-1), yard.reshape(-1), FLOOR_RED, cap=CAP_WGRAD_BF16 * scale if c.bf16 else None)
    fig.done()


# ---- refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('family,args,why', K.REFUSALS, ids=[r[2] for r in K.REFUSALS])
def test_refusals_write_nothing(hip_device, family, args, why):
    """arguments outside the kernels' contract: non-zero return with a message, y and the statistics stay NaN"""
    E, dev = _engine(), hip_device
    query = 'seg3d_conv3d_k2s2_variant' if family == 'gather' else 'seg3d_convT3d_k2s2_variant'
    assert E.query(query, *args) < 0
    N, D, H, W, A, B, mode, out_bf16 = args[:8]
    has_addend, ld = (args[8], args[9]) if family == 'scatter' else (0, 0)
    fine = family == 'gather'
    xdt = torch.bfloat16 if mode else torch.float32
    ydt = torch.bfloat16 if out_bf16 else torch.float32
    x = torch.ones((N, D * (2 if fine else 1), H * (2 if fine else 1), W * (2 if fine else 1), A + 4), dtype=xdt, device=dev)
    wp = torch.zeros(1 << 16, dtype=torch.float32, device=dev)              # ample for any image of these channel counts
    bias = torch.zeros(B + 4, device=dev)
    y = Guarded(N * D * H * W * (1 if fine else 8) * (B + 4), 1024 * 16, dev, ydt)
    stats = Guarded(1 << 14, 1024, dev)
    addend = torch.ones((N * D * H * W * 8, max(ld, B) + 4), dtype=ydt, device=dev)
    dims = (N, D, H, W, A, B)
    with pytest.raises(ValueError):
        if has_addend:
            E.call('seg3d_convT3d_k2s2_scatter_addend', E.ptr(x), mode, E.ptr(wp), E.ptr(addend), ld, E.ptr(y.t), *dims, out_bf16,
                   E.stream_ptr())
        elif mode:
            E.call('seg3d_conv3d_k2s2_bf16_fwd' if fine else 'seg3d_convT3d_k2s2_bf16_fwd', E.ptr(x), E.ptr(wp), E.ptr(bias), E.ptr(y.t),
                   E.ptr(stats.t), *dims, out_bf16, int(mode == 2), E.stream_ptr())
        else:
            E.call('seg3d_conv3d_k2s2_mfma_fwd' if fine else 'seg3d_convT3d_k2s2_mfma_fwd', E.ptr(x), E.ptr(wp), E.ptr(bias), E.ptr(y.t),
                   E.ptr(stats.t), *dims, E.stream_ptr())
    assert E.last_error(), why
    torch.cuda.synchronize()
    assert y.all_nan() and y.guards_untouched() and stats.all_nan() and stats.guards_untouched(), why
