"""The drop-in replacements of the reference project's own losses (csrc/loss.hip: dice_partial_kernel, dice_finalize_kernel,
dice_bwd_kernel, bdice_partial_kernel, bdice_bwd_kernel, focal_partial_kernel, focal_finalize_kernel, focal_bwd_kernel), driven
through the C ABI, against the plain float64 references of tests/loss_cases.py.  The cases are those of tests/loss_cases.py;
tests/test_loss_cases.py shows on the host that each reaches the block count, finalize round and grid-stride trip it is named for,
and that the references reproduce the reference project's recorded results.

Layout: probabilities NCDHW planar [N][C][S], targets float class ids [N][S]; focal also reads [sample, class] matrices through the
strides (sn, sc, ss) = (0, 1, C) and writes its gradient through the same strides.

Operands: soft-max probabilities with, per case, voxels AT the Dice gate and one float above and below it, a class absent from a
sample, tied binary channels, float targets that are no class id (-1, C, C + 3, 0.5, 1.7, -0.5, 0.3, 2.0), selected focal
probabilities of 0, 1e-30, 1e-12 and 0.5, a zero class weight, unnormalised weights and gout != 1 (loss_cases.dice_inputs,
bdice_inputs, focal_inputs).  Every output and workspace (part, sums, loss, dprobs) is a NaN-filled buffer of exactly the documented
size inside NaN guard bands: afterwards every element is finite and every guard bit-identical.

Bars: nothing is pinned to what the kernels give.  Each case evaluates the same reference function in float32 on the CPU: the
yardstick.  err <= 4 * yardstick + floor * scale, floor = 1e-5 for loss and sums and 2e-6 for dprobs, scale = max |ref|, under the
caps of the existing tests: loss 1e-5 absolute for Dice, 1e-5 of max(1, |loss|) for focal, 1e-6 for binary Dice; gradient 1e-4
relative L2 for Dice and focal, 1e-7 absolute for binary Dice.  The focal gradient spans twenty orders of magnitude (-alpha / 1e-10
beside ordinary values), so it is compared PER ELEMENT relative to |ref|, the yardstick taken the same way: ordinary voxels do not
hide behind one huge entry.  What must be exactly 0.0 is compared exactly: the Dice gradient wherever p <= float32(1 / C); I, den
and the gradient plane of a class that is absent and below the gate; plane 0 of the binary Dice gradient; every focal plane c != k
and every plane of a voxel whose class is outside [0, C).

Figures, MI355X, the largest over the cases of a family (a run appends every figure to the parity report that gpu_util.report
writes); err, yardstick and bar as fractions of the scale, except where marked absolute:
    Dice         loss    err 5.2e-8  yardstick 8.2e-8  bar 1.0e-5  (4.6e-7 absolute, cap 1e-5)          err / bar 0.05
                 I, den  err 1.0e-7  yardstick 1.1e-7  bar 1.0e-5                                       err / bar 0.01
                 dprobs  err 2.0e-7  yardstick 2.4e-7  bar 2.9e-6  relative L2 7.9e-8 (cap 1e-4)        err / bar 0.07
    binary Dice  loss    err 6.2e-8  yardstick 7.3e-8  bar 2.9e-6  (3.7e-8 absolute, cap 1e-6)          err / bar 0.04
                 I, den  err 1.2e-7  yardstick 1.4e-7  bar 1.1e-5                                       err / bar 0.01
                 dprobs  err 1.5e-7  yardstick 2.4e-7  bar 3.0e-6  (5.1e-8 absolute at N = S = 1, cap 1e-7: err / bar 0.51)
    focal        loss    err 1.6e-7  yardstick 1.2e-7  bar 1.0e-5                                       err / bar 0.02
                 dprobs  per element: err 3.0e-7  yardstick 2.7e-7  bar 3.1e-6; relative L2 8.8e-8 (cap 1e-4)
Every exact-zero check holds.  The slowest cases are the 2 097 229-voxel ones (0.24 s Dice, 0.16 s focal, their references and
yardsticks included); the first case also loads the library (0.5 s); the file takes 3 s.  6 Dice, 4 binary Dice and 31 focal cases
and one refusal; no case is above its bar.
"""
import time

import pytest
import torch

import loss_cases as K
from float64_util import FLOOR_EW, FLOOR_RED, Figures, Guarded, _engine

pytestmark = pytest.mark.gpu

GUARD = 1024
CAP_LOSS, CAP_LOSS_BDICE = 1e-5, 1e-6              # test_losses_against_oracle, test_small_losses_match_reference_fixtures
CAP_GRAD_L2, CAP_GRAD_BDICE = 1e-4, 1e-7


def _outputs(dev, **sizes):
    return {k: Guarded(n, GUARD, dev) for k, n in sizes.items()}


def _written(fig, bufs):
    for k, g in bufs.items():
        fig.require(bool(torch.isfinite(g.t).all()), '{}: {} elements not written (or not finite)'.format(k, int((~torch.isfinite(g.t)).sum())))
        fig.require(g.guards_untouched(), '{}: the guard bands were written'.format(k))


def _untouched(bufs):
    return all(g.all_nan() and g.guards_untouched() for g in bufs.values())


def _rel_l2(fig, key, dev, ref, cap):
    """the existing tests' gradient bar, beside Figures.check"""
    norm = float(ref.norm())
    fig.figs[key + '_rel_l2'] = float((dev.double().reshape(ref.shape) - ref).norm()) / norm if norm > 0.0 else 0.0
    fig.require(fig.figs[key + '_rel_l2'] <= cap, '{}: relative L2 {:.3e} > {:.0e}'.format(key, fig.figs[key + '_rel_l2'], cap))


def _check_per_element(fig, key, dev, ref, yard, floor, cap):
    """|dev - ref| <= bar * |ref| for every element, bar = min(4 * yardstick + floor, cap), the yardstick the largest relative error of
    the fp32 evaluation; an element whose reference is 0 must be 0"""
    dev, yard = dev.double().reshape(ref.shape), yard.double().reshape(ref.shape)
    nz = ref != 0.0
    fig.require(bool((dev[~nz] == 0.0).all()), '{}: {} elements are not 0.0 where the reference is'.format(key, int((dev[~nz] != 0.0).sum())))
    if not bool(nz.any()):
        return
    mag = ref[nz].abs()
    ye, err = float(((yard[nz] - ref[nz]).abs() / mag).max()), float(((dev[nz] - ref[nz]).abs() / mag).max())
    bar = min(4.0 * ye + floor, cap)
    fig.figs.update({key + '_relerr': err, key + '_relyard': ye, key + '_relbar': bar})
    fig.require(ye <= 1e-4, '{}: the fp32 yardstick is {:.3e} (relative) away from the float64 reference'.format(key, ye))
    fig.require(err <= bar, '{}: per-element relative err {:.3e} > bar {:.3e} (yardstick {:.3e})'.format(key, err, bar, ye))


def _finish(fig, t0):
    torch.cuda.synchronize()
    fig.figs['seconds'] = time.perf_counter() - t0
    fig.done()


# ---- multi-class Dice ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.DICE_CASES, ids=K.case_id)
def test_dice(hip_device, case):
    E, dev, t0 = _engine(), hip_device, time.perf_counter()
    N, C, S = case
    fig = Figures('loss/' + K.case_id(case))
    p, t, w, gout = K.dice_inputs(case)
    (L, sums_r, d_r, _), (Ly, sums_y, d_y, _) = [K.dice_ref(p, t, w, gout, dt) for dt in (torch.float64, torch.float32)]
    nblk = E.query('seg3d_dice_blocks', S)
    pd, td, wd, gd = p.to(dev), t.to(dev), w.to(dev), torch.tensor([gout], dtype=torch.float32, device=dev)
    o = _outputs(dev, part=N * nblk * C * 3, sums=N * C * 2, loss=1, dprobs=N * C * S)
    E.call('seg3d_dice_fwd', E.ptr(pd), E.ptr(td), E.ptr(wd), E.ptr(o['part'].t), E.ptr(o['sums'].t), E.ptr(o['loss'].t), N, C, S,
           E.stream_ptr())
    E.call('seg3d_dice_bwd', E.ptr(pd), E.ptr(td), E.ptr(o['sums'].t), E.ptr(wd), E.ptr(gd), E.ptr(o['dprobs'].t), N, C, S,
           E.stream_ptr())
    torch.cuda.synchronize()
    _written(fig, o)
    sums, d = o['sums'].t.cpu().reshape(N, C, 2), o['dprobs'].t.cpu().reshape(N, C, S)
    fig.check('loss', o['loss'].t.cpu(), L.reshape(1), Ly.reshape(1), FLOOR_RED, cap=CAP_LOSS)
    fig.check('sum_I', sums[..., 0], sums_r[..., 0], sums_y[..., 0], FLOOR_RED)
    fig.check('sum_den', sums[..., 1], sums_r[..., 1], sums_y[..., 1], FLOOR_RED)
    fig.check('dprobs', d, d_r, d_y, FLOOR_EW)
    _rel_l2(fig, 'dprobs', d, d_r, CAP_GRAD_L2)
    fig.require(bool((d[p <= K.dice_thr(C)] == 0.0).all()), 'dprobs: not 0.0 somewhere at or below the gate')
    if C == 5:
        n, cls = K.ABSENT
        I, den = sums[n, cls, 0], sums[n, cls, 1]
        fig.require(float(I) == 0.0 and float(den) == 0.0, 'the absent class: I, den = {}, {}'.format(float(I), float(den)))
        eps = torch.tensor(K.EPS, dtype=torch.float32)
        fig.require(float(1.0 - (2.0 * I + eps) / (den + eps)) == 0.0, 'the absent class: its term of the loss is not 0.0')
        fig.require(bool((d[n, cls] == 0.0).all()), 'the absent class: a gradient is not 0.0')
    _finish(fig, t0)


def test_dice_refuses_seventeen_classes(hip_device):
    E, dev = _engine(), hip_device
    N, C, S = 1, K.MAXC + 1, 8
    ones = torch.ones(N * C * S, device=dev)
    o = _outputs(dev, part=N * C * 3, sums=N * C * 2, loss=1, dprobs=N * C * S)
    with pytest.raises(ValueError) as info:
        E.call('seg3d_dice_fwd', E.ptr(ones), E.ptr(ones), E.ptr(ones), E.ptr(o['part'].t), E.ptr(o['sums'].t), E.ptr(o['loss'].t),
               N, C, S, E.stream_ptr())
    assert str(info.value).startswith('seg3d_dice_fwd:')
    with pytest.raises(ValueError) as info:
        E.call('seg3d_dice_bwd', E.ptr(ones), E.ptr(ones), E.ptr(ones), E.ptr(ones), E.ptr(ones), E.ptr(o['dprobs'].t), N, C, S,
               E.stream_ptr())
    assert str(info.value).startswith('seg3d_dice_bwd:')
    torch.cuda.synchronize()
    assert _untouched(o)


# ---- binary Dice -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.BDICE_CASES, ids=K.case_id)
def test_binary_dice(hip_device, case):
    E, dev, t0 = _engine(), hip_device, time.perf_counter()
    N, S = case
    fig = Figures('loss/' + K.case_id(case))
    p, t, gout = K.bdice_inputs(case)
    (L, sums_r, d_r), (Ly, sums_y, d_y) = [K.bdice_ref(p, t, gout, dt) for dt in (torch.float64, torch.float32)]
    nblk = E.query('seg3d_dice_blocks', S)
    pd, td = p.to(dev), t.to(dev)
    one, gd = torch.ones(1, dtype=torch.float32, device=dev), torch.tensor([gout], dtype=torch.float32, device=dev)
    o = _outputs(dev, part=N * nblk * 3, sums=N * 2, loss=1, dprobs=N * 2 * S)
    E.call('seg3d_binary_dice_fwd', E.ptr(pd), E.ptr(td), E.ptr(one), E.ptr(o['part'].t), E.ptr(o['sums'].t), E.ptr(o['loss'].t), N, S,
           E.stream_ptr())
    E.call('seg3d_binary_dice_bwd', E.ptr(pd), E.ptr(td), E.ptr(o['sums'].t), E.ptr(gd), E.ptr(o['dprobs'].t), N, S, E.stream_ptr())
    torch.cuda.synchronize()
    _written(fig, o)
    sums, d = o['sums'].t.cpu().reshape(N, 2), o['dprobs'].t.cpu().reshape(N, 2, S)
    fig.check('loss', o['loss'].t.cpu(), L.reshape(1), Ly.reshape(1), FLOOR_RED, cap=CAP_LOSS_BDICE)
    fig.check('sum_I', sums[:, 0], sums_r[:, 0], sums_y[:, 0], FLOOR_RED)
    fig.check('sum_den', sums[:, 1], sums_r[:, 1], sums_y[:, 1], FLOOR_RED)
    fig.check('dprobs', d, d_r, d_y, FLOOR_EW, cap=CAP_GRAD_BDICE)
    fig.require(bool((d[:, 0] == 0.0).all()), 'dprobs: plane 0 is not 0.0')
    fig.require(bool((d[:, 1][p[:, 1] <= p[:, 0]] == 0.0).all()), 'dprobs: not 0.0 somewhere p1 <= p0')
    _finish(fig, t0)


# ---- focal -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.FOCAL_CASES, ids=K.case_id)
def test_focal(hip_device, case):
    E, dev, c, t0 = _engine(), hip_device, case, time.perf_counter()
    N, C, S = c.N, c.C, c.S
    fig = Figures('loss/' + K.case_id(c))
    p, t, alpha, gout = K.focal_inputs(c)
    (L, d_r, sel), (Ly, d_y, _) = [K.focal_ref(p, t, alpha, c.gamma, c.size_average, gout, dt) for dt in (torch.float64, torch.float32)]
    if c.layout == 'planar':
        phys, strides = p.contiguous(), (C * S, S, 1)
        logical = lambda flat: flat.reshape(N, C, S)
    else:                                               # [sample, class]: element (0, c, s) at s * C + c
        phys, strides = p[0].t().contiguous(), (0, 1, C)
        logical = lambda flat: flat.reshape(S, C).t().unsqueeze(0)
    nblk = E.query('seg3d_focal_blocks', N * S)
    pd, td, ad = phys.to(dev), t.to(dev), alpha.to(dev)
    gd = torch.tensor([gout], dtype=torch.float32, device=dev)
    o = _outputs(dev, part=nblk, loss=1, dprobs=N * C * S)
    E.call('seg3d_focal_fwd', E.ptr(pd), E.ptr(td), E.ptr(ad), E.ptr(o['part'].t), E.ptr(o['loss'].t), N, C, S, *strides, c.gamma,
           c.size_average, E.stream_ptr())
    E.call('seg3d_focal_bwd', E.ptr(pd), E.ptr(td), E.ptr(ad), E.ptr(gd), E.ptr(o['dprobs'].t), N, C, S, *strides, c.gamma,
           c.size_average, E.stream_ptr())
    torch.cuda.synchronize()
    _written(fig, o)
    d = logical(o['dprobs'].t.cpu())
    fig.check('loss', o['loss'].t.cpu(), L.reshape(1), Ly.reshape(1), FLOOR_RED, cap=CAP_LOSS * max(1.0, abs(float(L))))
    fig.require(bool((d[~sel] == 0.0).all()), 'dprobs: {} elements outside the selected planes are not 0.0'.format(int((d[~sel] != 0.0).sum())))
    _check_per_element(fig, 'dprobs', d, d_r, d_y, FLOOR_EW, CAP_GRAD_L2)
    _rel_l2(fig, 'dprobs', d, d_r, CAP_GRAD_L2)
    _finish(fig, t0)
