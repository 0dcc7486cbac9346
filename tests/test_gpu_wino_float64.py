"""Every kernel of the Winograd 3x3x3 family (csrc/conv_wino.hip: F(2, 3) forward / data gradient and F(3, 2) weight gradient
along x; csrc/conv_wino2d.hip: F(2x2, 3x3) on tiles, with and without stream-K, and on cells, and the F(3x3, 2x2) weight gradient),
driven through the C ABI, against a plain float64 reference.  The cases are those of tests/wino_cases.py; each one first asserts
through the read-only queries, on the device, that it reaches what it is named for (tile or cell kernel, cells per item, stream-K
chunks, tile width, slabs, reducer): a device with another CU count than the table's 256 fails there.

Layout: NDHWC activations, weights [Cout][Cin][3][3][3], t = (kz * 3 + ky) * 3 + kx.

Operands: float64_util._activation gives every sample its own mean and spread (a halo read that lands in the neighbouring sample
is an error of the size of the data, not noise of equal statistics); x, dy, the addend and the packed weight image sit inside NaN
guard bands of more than one z plane (the kernels get their z padding from a buffer resource's range check: a read of plane -1 or
plane D that reached memory would bring a NaN); y, the statistics, dw and both workspaces are NaN-filled inside NaN guard bands of
at least one tile of rows.

Reference: float64 on the device, from the definition (float64_util._conv_def, _wgrad_def), plus bias and addend.

Bars: nothing is pinned to what the kernels give, and the yardstick is never HIP code.  Each case runs the operation twice in
fp32 on the CPU -- F.conv3d / autograd, and a restatement in plain torch of the Winograd form itself as written out in the two
files' header comments (float64_util._wino_*; tests/test_wino_variants.py holds them against the definition in float64) -- and the
yardstick is the larger of the two errors.  err <= 4 * yardstick + 2e-6 * scale for y, + 1e-5 * scale for dw, scale = max |ref|,
both under the existing tests' cap of 1e-5 * scale.  Statistics: float64_util._check_stats with its 1e-5 caps of sum |y| and of
sum y^2, and the same yardstick rule; also per item of the tile kernels (its eight slots) and per (cell, column block) of the cell
kernel (its two slots) against the float64 sums over that item's or cell's voxels, with the same 1e-5 caps -- a slot that holds
another item's sum, or a cut item's piece alone, fails there.

Write discipline: all guards bit-identical afterwards, the inputs' too; no NaN left in y, dw, a statistics slot or the weight
gradient's workspace; a second call bit-identical; accumulate = 1 from a known base equals base + plain bit for bit.  Stream-K: the
same shape without a workspace walks whole items -- its y differs from the stream-K y in at least one cut item and in no uncut one
(the cut items follow from the chunk count the query reports); a workspace the plan declines changes no bit.

Figures per kernel body, MI355X: the largest err / bar over outputs (y or dw) and over the statistics, the largest err / scale,
the largest yardstick / scale, and the slowest case, reference and both CPU yardsticks included (a run appends every figure to the
parity report that gpu_util.report writes):
    wino      conv3d_k3_wino_kernel                   y 0.09  st 0.002   err 6.2e-7   yardstick 1.2e-6   0.23 s  (1 x (32, 32, 64) 8 -> 128)
    tile      conv3d_k3_wino2d_kernel, whole items    y 0.11  st 0.010   err 6.8e-7   yardstick 1.5e-6   0.13 s  (1 x (40, 56, 24) 40 -> 96)
    tile_sk   ... stream-K and its finish kernel      y 0.10  st 0.001   err 6.9e-7   yardstick 1.3e-6   0.16 s  (1 x (48, 48, 32) 32 -> 64)
    c4_4      conv3d_k3_wino2d_c4_kernel<., ., 4>     y 0.11  st 0.004   err 5.8e-7   yardstick 1.7e-6   0.06 s  (3 x (16, 28, 24) 64 -> 96)
    c4_2      conv3d_k3_wino2d_c4_kernel<., ., 2>     y 0.17  st 0.001   err 1.2e-6   yardstick 1.3e-6   0.06 s  (1 x (16, 28, 8) 64 -> 320)
    F(3, 2) weight gradient, both tiles and reducers  dw 0.05            err 4.6e-7   yardstick 4.9e-6   0.14 s  (1 x (32, 32, 36) 8 -> 24)
    F(3x3, 2x2) weight gradient, both reducers        dw 0.04            err 3.2e-7   yardstick 2.1e-6   0.12 s  (1 x 32^3 8 -> 24)
Statistics per sample stay below 8e-9 of sum |y| and of sum y^2 (cap 1e-5), per item of the tile kernels below 7e-8, per cell
and column block below 1e-7.  Every cut item of every stream-K case (189 at most) differs from the whole-item walk, no uncut one
does.  The first case of each kind also loads the library and warms the device up (0.9 s and 0.8 s); the whole file takes 6.7 s.
31 forward cases, 17 weight-gradient cases and 14 refusals; no case is above its bar.
"""
import time

import pytest
import torch
import torch.nn.functional as F

import wino_cases as T
from float64_util import (FLOOR_EW, FLOOR_RED, CAP_STAT, Figures, Guarded, _activation, _check_stats, _conv_def, _engine, _noise,
                          _weight, _wgrad_def, _wino_f23_conv, _wino_f2x2_conv, _wino_f32_wgrad, _wino_f3x3_wgrad)

pytestmark = pytest.mark.gpu

CAP_REL = 1e-5                  # the existing Winograd tests' cap, of the scale: outputs and weight gradients


def _bits(t):
    return t.view(torch.int32)


def _dims(c):
    return c.N, c.D, c.H, c.W, c.Cin, c.Cout


def _in_guard(c, C):
    """more than one z plane, one row and one voxel of an input with C channels (what a halo read in front of, or behind, the
    tensor would touch), and at least 1024 voxels"""
    return max(c.H * c.W + c.W + 2, 1024) * C


def _per_item(t, c):
    """[N, D, H, W, Cout] -> [units, e * e * e * 32] in the order (sample, tile or cell z, y, x, column block): the items of the
    tile kernels (e = 8), the (cell, column block) units of the cell kernel (e = 4), which own the statistics slots"""
    nz, ny, nx = T.counts(c)
    e = T.edge(c)
    v = t.reshape(c.N, nz, e, ny, e, nx, e, c.Cout // 32, 32).permute(0, 1, 3, 5, 7, 2, 4, 6, 8)
    return v.reshape(c.N * nz * ny * nx * (c.Cout // 32), -1)


def _finish(fig, t0):
    torch.cuda.synchronize()
    fig.figs['seconds'] = time.perf_counter() - t0
    fig.done()


# ---- forward / data gradient -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', T.FWD_CASES, ids=T.case_id)
def test_wino_forward(hip_device, case):
    E, c, dev, t0 = _engine(), case, hip_device, time.perf_counter()
    fig = Figures('wino/{}/{}'.format(c.body, T.case_id(c)))
    form = 'wino' if c.body == 'wino' else 'wino2d'
    assert E.query('seg3d_conv3d_k3_{}_supported'.format(form), *_dims(c)) == 1
    sk = 0
    if form == 'wino2d':
        assert E.query('seg3d_conv3d_k3_wino2d_fwd_variant', *_dims(c)) == T.BODY_VARIANT[c.body]
        sk = E.query('seg3d_conv3d_k3_wino2d_fwd_sk_chunks', *_dims(c))
        assert (sk > 0) if c.body == 'tile_sk' else (sk == 0 or c.ws == 0)
    assert T.item_class(T.n_items(c)) == c.items
    nws = E.query('seg3d_conv3d_k3_wino2d_fwd_workspace_floats', *_dims(c)) if form == 'wino2d' else 0
    assert (nws > 0) == (sk > 0)
    if c.ws and not sk:                             # a declined plan wants no workspace: the case passes one of the stream-K size
        nws = 2 * T.CUS * 512 * 32
    cnt = E.query('seg3d_conv3d_k3_{}_stats_count'.format(form), *_dims(c))

    fwd = c.role == 'fwd'
    A, B = c.Cin, c.Cout
    x = _activation(980, fig.name + '/x', c.N, (c.D, c.H, c.W), A)
    w = _weight(981, fig.name + '/w', (B, A, 3, 3, 3) if fwd else (A, B, 3, 3, 3), 27 * A)
    weff = w if fwd else w.transpose(0, 1).flip(2, 3, 4).contiguous()
    sa, sb, flip = (27, 27 * A, 0) if fwd else (27 * B, 27, 1)
    bias = (0.3 * _noise(982, fig.name + '/b', (B,)) + 0.2) if c.bias else None
    addend = _activation(983, fig.name + '/a', c.N, (c.D, c.H, c.W), B, offset=-0.5) if c.addend else None

    ref = _conv_def(x.to(dev).double(), weff.to(dev).double())
    yards = [F.conv3d(x.permute(0, 4, 1, 2, 3), weff, None, padding=1).permute(0, 2, 3, 4, 1),
             (_wino_f23_conv if form == 'wino' else _wino_f2x2_conv)(x, weff)]
    if c.bias:
        ref = ref + bias.to(dev).double()
        yards = [y + bias for y in yards]
    if c.addend:
        ref = ref + addend.to(dev).double()
        yards = [y + addend for y in yards]
    yards = tuple(yards)

    xg = Guarded(x.numel(), _in_guard(c, A), dev, fill=x.to(dev))
    ag = Guarded(addend.numel(), _in_guard(c, B), dev, fill=addend.to(dev)) if c.addend else None
    wd = w.to(dev)
    bd = bias.to(dev) if c.bias else None
    Tn = 36 if form == 'wino' else 48
    wp = Guarded(E.query('seg3d_packed_mfma_floats', A, B, Tn), 48 * 256, dev)
    E.call('seg3d_pack_weights_mfma', E.ptr(wd), E.ptr(wp.t), A, B, Tn, sa, sb, flip, E.stream_ptr())
    torch.cuda.synchronize()
    fig.require(wp.guards_untouched() and not bool(torch.isnan(wp.t).any()), 'packed image: guards written, or an entry not written')
    wp_before = wp.buf.clone()

    def run(workspace):
        y = Guarded(ref.numel(), 1024 * B, dev)
        stats = Guarded(c.N * cnt * 2, 1024, dev) if c.stats else None
        ws = Guarded(nws, 32 * 1024, dev) if workspace else None
        head = (E.ptr(xg.t), E.ptr(wp.t), E.ptr(bd), E.ptr(ag.t) if ag else None, E.ptr(y.t), E.ptr(stats.t) if stats else None)
        if form == 'wino':
            E.call('seg3d_conv3d_k3_wino_fwd', *head, *_dims(c), E.stream_ptr())
        elif workspace or c.ws:
            E.call('seg3d_conv3d_k3_wino2d_fwd_ws', *head, E.ptr(ws.t) if ws else None, *_dims(c), E.stream_ptr())
        else:
            E.call('seg3d_conv3d_k3_wino2d_fwd', *head, *_dims(c), E.stream_ptr())
        torch.cuda.synchronize()
        fig.require(y.guards_untouched(), 'y: the guard bands were written')
        fig.require(stats is None or stats.guards_untouched(), 'stats: the guard bands were written')
        fig.require(ws is None or ws.guards_untouched(), 'workspace: the guard bands were written')
        return y, stats, ws

    (y, stats, ws), (y2, stats2, _) = run(c.ws), run(c.ws)
    scale = float(ref.abs().max())
    fig.check('y', y.t, ref.reshape(-1), tuple(v.reshape(-1) for v in yards), FLOOR_EW, cap=CAP_REL * scale)
    fig.require(torch.equal(_bits(y.t), _bits(y2.t)), 'y: the second call differs')
    if c.stats:
        _check_stats(fig, stats, ref, yards, c.N, cap=CAP_STAT)
        fig.require(torch.equal(_bits(stats.t), _bits(stats2.t)), 'stats: the second call differs')
        # per item (eight slots, one per wave) / per cell and column block (two slots: the channel halves)
        r = _per_item(ref, c)
        assert stats.t.numel() == r.shape[0] * (4 if T.edge(c) == 4 else 16)
        got = stats.t.reshape(r.shape[0], -1, 2).double().sum(1)
        rel = torch.maximum((got[:, 0] - r.sum(1)).abs() / r.abs().sum(1), (got[:, 1] - (r * r).sum(1)).abs() / (r * r).sum(1))
        fig.figs['stat_item_worst'] = float(rel.max())
        fig.require(bool((rel <= CAP_STAT).all()), 'stats: the slots of items {} are not the sums over their voxels'.format(
            (~(rel <= CAP_STAT)).nonzero().reshape(-1)[:8].tolist()))
    if c.ws:
        # the same call without a workspace walks whole items
        y0, stats0, _ = run(0)
        differ = (_per_item(y.t, c) != _per_item(y0.t, c)).any(1)
        if sk:
            cut = torch.zeros_like(differ)
            cut[torch.tensor(T.cut_items(c, sk), device=dev)] = True
            fig.figs['cut_items'], fig.figs['cut_items_that_differ'] = float(cut.sum()), float((differ & cut).sum())
            fig.require(bool((differ & cut).any()), 'no cut item differs from the whole-item walk: the stream-K form did not run')
            fig.require(not bool((differ & ~cut).any()), 'uncut items {} differ from the whole-item walk'.format(
                (differ & ~cut).nonzero().reshape(-1)[:8].tolist()))
            fig.check('y_whole_items', y0.t, ref.reshape(-1), tuple(v.reshape(-1) for v in yards), FLOOR_EW, cap=CAP_REL * scale)
        else:
            fig.require(not bool(differ.any()), 'a workspace that the plan declines changed y')
            fig.require(ws.all_nan(), 'a workspace that the plan declines was written')
            fig.require(stats0 is None or torch.equal(_bits(stats.t), _bits(stats0.t)), 'a declined workspace changed the statistics')
    fig.require(xg.guards_untouched() and torch.equal(_bits(xg.t), _bits(x.to(dev).reshape(-1))), 'x was written')
    fig.require(ag is None or (ag.guards_untouched() and torch.equal(_bits(ag.t), _bits(addend.to(dev).reshape(-1)))), 'the addend was written')
    fig.require(torch.equal(_bits(wp.buf), _bits(wp_before)), 'the packed image was written')
    _finish(fig, t0)


# ---- weight gradient -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', T.WGRAD_CASES, ids=T.case_id)
def test_wino_wgrad(hip_device, case):
    E, c, dev, t0 = _engine(), case, hip_device, time.perf_counter()
    fig = Figures('wino/wgrad_{}-{}/{}'.format(c.form, c.variant, T.case_id(c)))
    entry = 'seg3d_conv3d_k3_{}_wgrad'.format(c.form)
    assert E.query(entry + '_supported', *_dims(c)) == 1 and E.query(entry + '_variant', *_dims(c)) == c.variant
    nws = E.query(entry + '_workspace_floats', *_dims(c))
    slabs = nws // (T.npairs(c) * T.WS_PER_SLAB[c.form])
    assert T.slab_class(c, slabs) == c.slabs
    sp = (c.D, c.H, c.W)
    x = _activation(990, fig.name + '/x', c.N, sp, c.Cin, offset=0.25)
    dy = _activation(991, fig.name + '/dy', c.N, sp, c.Cout, offset=0.0)
    ref = _wgrad_def(x.to(dev).double(), dy.to(dev).double())                # [Cout][Cin][27]: the layout dw is written in
    w0 = torch.zeros(c.Cout, c.Cin, 3, 3, 3, requires_grad=True)
    yard = torch.autograd.grad(F.conv3d(x.permute(0, 4, 1, 2, 3), w0, padding=1), w0, dy.permute(0, 4, 1, 2, 3))[0].reshape(ref.shape)
    yards = (yard, (_wino_f32_wgrad if c.form == 'wino' else _wino_f3x3_wgrad)(x, dy))
    scale = float(ref.abs().max())
    prior = (_noise(992, fig.name + '/dw0', tuple(ref.shape)) * scale * 0.5).to(dev)
    xg = Guarded(x.numel(), _in_guard(c, c.Cin), dev, fill=x.to(dev))
    dyg = Guarded(dy.numel(), _in_guard(c, c.Cout), dev, fill=dy.to(dev))

    def run(accumulate):
        dw = Guarded(ref.numel(), 27 * 1024, dev, fill=prior if accumulate else None)
        ws = Guarded(nws, 48 * 1024, dev)
        E.call(entry, E.ptr(xg.t), E.ptr(dyg.t), E.ptr(dw.t), E.ptr(ws.t), *_dims(c), accumulate, E.stream_ptr())
        torch.cuda.synchronize()
        fig.require(dw.guards_untouched(), 'dw: the guard bands were written (accumulate = {})'.format(accumulate))
        fig.require(ws.guards_untouched(), 'workspace: the guard bands were written (accumulate = {})'.format(accumulate))
        fig.require(not bool(torch.isnan(ws.t).any()), 'workspace: a slab entry was not written')
        return dw

    dw, dw2 = run(0), run(0)
    fig.require(torch.equal(_bits(dw.t), _bits(dw2.t)), 'dw: the second call differs')
    got, yards_ = dw.t, yards
    if c.accumulate:
        acc = run(1)
        fig.require(torch.equal(_bits(acc.t), _bits(prior.reshape(-1) + dw.t)), 'dw: the accumulating call is not base + plain')
        got, ref, yards_ = acc.t, ref + prior.double(), tuple(v + prior.cpu() for v in yards)
    fig.check('dw', got, ref.reshape(-1), tuple(v.reshape(-1) for v in yards_), FLOOR_RED, cap=CAP_REL * scale)
    fig.require(xg.guards_untouched() and torch.equal(_bits(xg.t), _bits(x.to(dev).reshape(-1))), 'x was written')
    fig.require(dyg.guards_untouched() and torch.equal(_bits(dyg.t), _bits(dy.to(dev).reshape(-1))), 'dy was written')
    _finish(fig, t0)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prefix,entry,kind,change,why', T.REFUSALS, ids=[r[4] for r in T.REFUSALS])
def test_refusals_write_nothing(hip_device, prefix, entry, kind, change, why):
    """arguments outside the kernels' contract: an error whose message starts with the entry's name, before any launch; the outputs
    stay NaN"""
    E, dev = _engine(), hip_device
    N, D, H, W, Cin, Cout = T.refusal_dims(change)
    ones = lambda ch: torch.ones((N, D, H, W, ch + 8), device=dev)
    wp = torch.zeros(1 << 18, device=dev)                                   # ample for any image of these channel counts
    bias = torch.zeros(64, device=dev)
    out = Guarded(N * D * H * W * 64, 4096, dev)                            # y, or dw (27 * 18 * 32 elements at most)
    aux = Guarded(1 << 16, 4096, dev)                                       # statistics
    wsp = Guarded(1 << 21, 4096, dev)                                       # a workspace
    null = change[1] if change[0] == 'null' else None
    with pytest.raises((ValueError, NotImplementedError)) as info:
        if kind == 'fwd':
            xs = None if null == 'x' else E.ptr(ones(Cin))
            head = (xs, E.ptr(wp), E.ptr(bias), None, E.ptr(out.t), E.ptr(aux.t))
            if entry.endswith('_ws'):
                E.call(entry, *head, E.ptr(wsp.t), N, D, H, W, Cin, Cout, E.stream_ptr())
            else:
                E.call(entry, *head, N, D, H, W, Cin, Cout, E.stream_ptr())
        else:
            E.call(entry, E.ptr(ones(Cin)), E.ptr(ones(Cout)), E.ptr(out.t), None if null == 'workspace' else E.ptr(wsp.t),
                   N, D, H, W, Cin, Cout, 0, E.stream_ptr())
    assert str(info.value).startswith(prefix + ':') and E.last_error().startswith(prefix + ':'), (why, str(info.value))
    torch.cuda.synchronize()
    assert out.all_nan() and out.guards_untouched() and aux.all_nan() and aux.guards_untouched(), why
    assert wsp.all_nan() and wsp.guards_untouched(), why
