"""The deep-supervision head and the label pyramid driven through the C ABI (seg3d_ds_head_fwd / _bwd / _bwd_finalize,
seg3d_label_pyramid) against the plain float64 reference of tests/ds_head_cases.py.  The cases are those of tests/ds_head_cases.py;
tests/test_ds_head_cases.py shows on the host that every <C, VPI, NQ> of both kernels (C = 1..8 x NQ = 1, 2, 4) is named once with a
full channel count (64 / 128 / 256) and once with a partly filled lane group (Cin of 4, 36, 60, 68, 100, 124, 132, 200, 252: the
`q < nq` guards and the staging loop's tail), and that every case has the tiles, the voxel tail, the slab count and the trip it claims.

V = N * S of 1, tile - 1, tile + 1, 2 tile + 2 and 2 tile + 3 of the case's own forward and backward tile, N = 1..3 with an odd S (a
sample boundary inside a group's run of voxels); x read in place at ldx = 0, Cin + 4 and 2 Cin out of a buffer whose other floats are
NaN, dx written at ld_dx = 0, Cin + 8 and 2 Cin + 4 -- the floats between its rows keep their NaN; b NULL; dw or db NULL in the
finalize; accumulate 0..3 onto pre-filled buffers, where the finalize must add exactly the float32 it writes without accumulate
(bit-equal to filled + plain); logit rows that are equal (probabilities of exactly 1 / C), logits spread over +-80, a zero weight matrix
(exactly 1 / C everywhere, dx exactly 0), dprobs dense and on one plane.  Four cases take the second grid-stride trip, their sizes
derived from the restated rules and held against the device's own CU count: forward at Cin = 4 (262 150 voxels, 2049 tiles of 128) and
Cin = 68 (131 077 voxels, 2049 tiles of 64), backward at VPI = 1 (16 397 voxels, 1025 tiles of 16) and VPI = 8 (131 193 voxels, 1025
tiles of 128).  The backward runs on the reference's probabilities rounded to float32, so its reference does not depend on the forward
kernel.  probs, dx, the workspace (exactly the queried floats), dw and db sit in NaN-filled buffers inside guard bands; every guard is
bit-identical afterwards and every input unchanged.

Bars (Figures.check): err <= min(4 * yardstick + floor * scale, cap), the yardstick the same reference in float32 on the CPU; floor 2e-6
for probs (per voxel) and dx (against the case's max |ref|), 1e-5 for dw and db; caps of tests/test_gpu_deep_supervision.py: probs 1e-4,
dx / dw / db 1e-4 of max |ref| and relative L2 1e-4.  The label pyramid is compared as int32 bit patterns, NaN payloads included.

Figures, MI355X, the largest over the 52 cases (a run appends every figure to the parity report that gpu_util.report writes):
    probs  err 2.7e-6  yardstick 2.2e-6  bar 8.8e-6  (logits spread over +-80)                             err / bar 0.30
    dx     err / scale 7.6e-7  yardstick / scale 7.6e-7  bar / scale 5.0e-6; relative L2 7.5e-7              err / bar 0.15
    dw     err / scale 1.2e-6  yardstick / scale 8.1e-6  bar / scale 4.2e-5; relative L2 7.5e-7              err / bar 0.08
    db     err / scale 1.4e-6  yardstick / scale 3.6e-6  bar / scale 2.4e-5; relative L2 9.6e-7              err / bar 0.07
Every exact comparison holds and every guard is intact; no defect was found in csrc/deep_supervision.hip.  The slowest case is the
131 077-voxel forward trip at Cin = 68 (0.33 s); the file takes 3 s: 52 head cases, 3 pyramid cases and the refusals.

The `q < nq` guards, tried one at a time on scratch copies of the library where the mutation stays inside LDS and the buffers: without
the guard of the slab reduction at the end of ds_head_bwd_kernel, wave 0's share of dw is overwritten for the first quads of class
c + 1 and the 16 cases with a partly filled group, NQ >= 2 and C >= 2 fail on dw.  Without the guard around the dot products of
ds_head_fwd_kernel the idle lanes multiply their zero x quads with whatever LDS holds behind the staged weights: one case failed (NaN
in probs), by the chance of that content -- the guard keeps reads inside the staged weights and no test can hold it to a value.  By
reading, not run (they leave the buffers): without the guard around the backward's dx stores the idle lanes write behind the row --
into the NaN between the rows of a strided dx or into the rear guard band, both of which the test checks; the two guards on the loads
of x only keep the reads inside the row, their values are used under the guards above.
"""
import time

import pytest
import torch

import ds_head_cases as H
from float64_util import FLOOR_EW, FLOOR_RED, NAN, Figures, Guarded, _engine
from test_gpu_compound_float64 import GUARD, Inputs, _finish, _rel_l2, _untouched

pytestmark = pytest.mark.gpu

CAP = 1e-4                                # tests/test_gpu_deep_supervision.py::test_head_matches_float64
F64, F32 = torch.float64, torch.float32


def _bits_equal(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _rows_in(x, stride, dev):
    """x [V, Cin] as the LAST Cin floats of the rows of a [V, stride] device buffer whose other floats are NaN -> (buffer, pointer tensor)"""
    V, Cin = x.shape
    wide = torch.full((V, stride), NAN, dtype=F32, device=dev)
    wide[:, stride - Cin:] = x.to(dev)
    flat = wide.reshape(-1)
    view = flat[stride - Cin:]
    assert view.data_ptr() % 16 == 0
    return wide, view


def _guards(fig, bufs):
    for k, g in bufs.items():
        fig.require(g.guards_untouched(), '{}: the guard bands were written'.format(k))


@pytest.mark.parametrize('case', H.CASES + H.TRIP_CASES, ids=H.case_id)
def test_head(hip_device, case):
    E, dev, c, t0 = _engine(), hip_device, case, time.perf_counter()
    N, S, Cin, C, V = c.N, c.S, c.Cin, c.C, c.N * c.S
    fig = Figures('dshead/' + H.case_id(c))
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    if c in H.TRIP_CASES:
        fig.require(H.fwd_plan(c, cus)[3] or H.bwd_plan(c, cus)[3], 'no second grid-stride trip on a device with {} compute units'.format(cus))
        fig.require(H.fwd_plan(c, cus)[3] == H.fwd_plan(c)[3] and H.bwd_plan(c, cus)[3] == H.bwd_plan(c)[3],
                    'the trips of the table (built for {} compute units) are not this device\'s ({})'.format(H.CUS, cus))
    x, w, b, d, dw0, db0 = H.inputs(c)
    bias = b if c.bias else None
    ldx, sx, ldd, sd = H.strides(c)
    p, py = [H.fwd_ref(x, w, bias, N, S, dt) for dt in (F64, F32)]
    i = Inputs(dev)
    xwide, xd = _rows_in(x, sx, dev)
    xkeep = xwide.clone()
    wd, bd = i.put('w', w), (i.put('b', b) if c.bias else None)
    # ---- forward
    o = {'probs': Guarded(N * C * S, GUARD, dev)}
    E.call('seg3d_ds_head_fwd', E.ptr(xd), ldx, E.ptr(wd), E.ptr(bd), E.ptr(o['probs'].t), N, S, Cin, C, E.stream_ptr())
    torch.cuda.synchronize()
    _guards(fig, o)
    got = o['probs'].t.cpu()
    fig.check('probs', got, p, py, FLOOR_EW, cap=CAP)
    if bool(torch.isfinite(got).all()):
        fig.require(float(got.min()) >= 0.0 and float(got.max()) <= 1.0, 'probs: outside [0, 1]')
        rows = got.reshape(N, C, S).permute(0, 2, 1).reshape(V, C)
        if c.values == 'zero':
            fig.require(bool(torch.equal(rows, torch.full_like(rows, 1.0) / C)), 'probs: not exactly 1 / C with a zero weight matrix')
        if c.values == 'equal':
            fig.require(bool(torch.equal(rows[0::2], torch.full_like(rows[0::2], 1.0) / C)), 'probs: not exactly 1 / C on rows of equal logits')
    # ---- backward, on the reference's probabilities
    p32 = p.float()
    ref, yard = [H.bwd_ref(p32, d, x, w, dt) for dt in (F64, F32)]
    pd, dd = i.put('probs', p32), i.put('dprobs', d)
    nws = E.query('seg3d_ds_head_bwd_workspace_floats', N, S, Cin, C)
    assert nws == H.workspace_floats(c)
    ob = {'dx': Guarded((V - 1) * sd + Cin, GUARD, dev), 'workspace': Guarded(nws, GUARD, dev), 'dw': Guarded(C * Cin, GUARD, dev),
          'db': Guarded(C, GUARD, dev), 'dw_acc': Guarded(C * Cin, GUARD, dev, fill=dw0.to(dev)), 'db_acc': Guarded(C, GUARD, dev, fill=db0.to(dev))}
    E.call('seg3d_ds_head_bwd', E.ptr(pd), E.ptr(dd), E.ptr(xd), ldx, E.ptr(wd), E.ptr(ob['dx'].t), ldd, E.ptr(ob['workspace'].t), N, S, Cin, C,
           E.stream_ptr())
    E.call('seg3d_ds_head_bwd_finalize', E.ptr(ob['workspace'].t), E.ptr(ob['dw'].t), E.ptr(ob['db'].t), N, S, Cin, C, 0, E.stream_ptr())
    E.call('seg3d_ds_head_bwd_finalize', E.ptr(ob['workspace'].t), E.ptr(ob['dw_acc'].t) if c.dw else None,
           E.ptr(ob['db_acc'].t) if c.db else None, N, S, Cin, C, c.accumulate, E.stream_ptr())
    torch.cuda.synchronize()
    _guards(fig, ob)
    i.unchanged(fig)
    fig.require(_bits_equal(xwide, xkeep), 'x: the input was written')
    dxbuf = torch.full((V * sd,), NAN)
    dxbuf[:(V - 1) * sd + Cin] = ob['dx'].t.cpu()
    dxrows = dxbuf.reshape(V, sd)
    fig.require(bool(torch.isnan(dxrows[:, Cin:]).all()), 'dx: the floats between the rows were written')
    dx, dw, db = dxrows[:, :Cin], ob['dw'].t.cpu(), ob['db'].t.cpu()
    for key, g, r, y, floor in (('dx', dx, ref[0], yard[0], FLOOR_EW), ('dw', dw, ref[1], yard[1], FLOOR_RED), ('db', db, ref[2], yard[2], FLOOR_RED)):
        fig.check(key, g, r, y, floor, cap=CAP * float(r.abs().max()))
        _rel_l2(fig, key, g, r, cap=CAP)
    if c.values == 'zero' or C == 1:
        fig.require(not bool(dx.any()), 'dx: not exactly 0')
    # the finalize's variants: NULL leaves the buffer as it was, accumulate adds exactly the float32 that the plain finalize writes
    for key, on, bit, fill, plain in (('dw_acc', c.dw, 1, dw0.reshape(-1), dw), ('db_acc', c.db, 2, db0, db)):
        want = fill if not on else (fill + plain if c.accumulate & bit else plain)
        fig.require(_bits_equal(ob[key].t.cpu(), want), '{}: accumulate = {}, passed = {}: not bit-equal to what the plain finalize gives'.format(
            key, c.accumulate, bool(on)))
    _finish(fig, t0)


# ---- label pyramid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('levels', [1, 2, 3])
def test_label_pyramid_copies_bit_patterns(hip_device, levels):
    E, dev = _engine(), hip_device
    N, D, H_, W = H.PYRAMID_SHAPE
    m = H.pyramid_input()
    i = Inputs(dev)
    md = i.put('mask', m)
    outs = [Guarded(N * (D >> k) * (H_ >> k) * (W >> k), GUARD, dev) for k in (1, 2, 3)]
    ptrs = [E.ptr(g.t) if k < levels else None for k, g in enumerate(outs)]
    E.call('seg3d_label_pyramid', E.ptr(md), ptrs[0], ptrs[1], ptrs[2], N, D, H_, W, levels, E.stream_ptr())
    torch.cuda.synchronize()
    fig = Figures('dshead/pyramid-{}'.format(levels))
    i.unchanged(fig)
    for k, g in enumerate(outs):
        f = 2 << k
        assert g.guards_untouched()
        if k < levels:
            assert _bits_equal(g.t.cpu(), m[:, ::f, ::f, ::f].contiguous().reshape(-1)), 'level {}'.format(k + 1)
        else:
            assert g.all_nan()
    fig.done()


# ---- one refusal per entry: the error comes back and nothing is written -----------------------------------------------------------------
def test_refusals(hip_device):
    E, dev = _engine(), hip_device
    N, S, Cin, C = 1, 8, 8, 2
    ones, st = torch.ones(1024, device=dev), E.stream_ptr
    o = {k: Guarded(n, GUARD, dev) for k, n in dict(probs=C * S, dx=S * Cin, workspace=C * Cin + C, dw=C * Cin, db=C, out1=3 * 4 * 4, out2=64).items()}
    P, q = E.ptr(ones), {k: E.ptr(g.t) for k, g in o.items()}
    calls = {
        'seg3d_ds_head_fwd': (P, Cin + 2, P, P, q['probs'], N, S, Cin, C, st()),
        'seg3d_ds_head_bwd': (P, P, P, 0, P, q['dx'], Cin - 4, q['workspace'], N, S, Cin, C, st()),
        'seg3d_ds_head_bwd_finalize': (P, q['dw'], q['db'], N, S, Cin, C, 4, st()),
        'seg3d_label_pyramid': (P, q['out1'], q['out2'], None, 1, 6, 8, 8, 2, st()),
    }
    assert sorted(calls) == sorted(H.REFUSALS)
    for name, args in calls.items():
        with pytest.raises(ValueError) as info:
            E.call(name, *args)
        assert str(info.value).startswith(name + ':'), (name, H.REFUSALS[name], str(info.value))
    torch.cuda.synchronize()
    assert _untouched(o)
