"""seg3d_augment_blur and seg3d_augment_lowres (csrc/augment_filter.hip) driven through the C ABI against the plain float64
references of tests/filter_cases.py.  The cases are those of tests/filter_cases.py; tests/test_filter_cases.py shows on the host that
each reaches the launch <MC, VEC>, radius set, tile counts and patch extents it is named for: every radius 0..6 in each of the three
blur launches (0 beside 6 and 1 beside 5 in one vector launch), Gaussian and free taps (distinct, not monotone, an exact 0 inside the
radius), axes of 1, axes shorter than the radius, exact tiles, one voxel more, three tiles along z, X = 65; every instantiation
lowres_launch can pick, the LDS patch exactly full at 35 x 11 x 11 on full and on partial tiles, n' = 1 on each axis and on all,
n' = n on one and two axes, a copied modality beside reduced ones, the runtime width at M = 3, 5 and 8, and the zooms {0.5, 0.26,
0.99} of tests/test_gpu_resolution_augment.py on a shape where 0.99 is no copy (it is the identity on every axis of that test's
shapes).

dst is a buffer of exactly X Y Z M floats filled with NaN inside guard bands: afterwards the guards are bit-identical, every element
is finite and src is bit-identical to what it was.  A case on vector rows is launched a second time with src and dst one float past
alignment (the scalar path): bit-equal to the aligned launch, under the same bar.  A blur channel of radius 0 and a low-resolution
modality with n' = n on every axis are bit-equal to the input on both paths; two runs are bit-equal.

Bars: nothing is pinned to what the kernels give.  Each case evaluates the same reference function in float32 on the CPU: the
yardstick.  |dev - ref64| <= min(4 * yardstick + 2e-6 * max|x|, 1e-5 * max|x|) for every element; the cap is the derived bar of
tests/test_gpu_resolution_augment.py, and tests/test_filter_cases.py holds every yardstick at or below a quarter of it.  The number of
elements whose bits differ from the float32 evaluation is recorded, not asserted.

Figures, MI355X, the largest over the cases of a family, shifted relaunches included (a run appends every figure to the parity report
that gpu_util.report writes), in units of max|x|:
    blur    err 1.4e-7  yardstick 1.4e-7  bar 2.6e-6  (M = 3, radii 3 / 4 / 1 on one exact tile)               err / bar 0.056
    lowres  err 2.2e-7  yardstick 2.2e-7  bar 2.9e-6  (M = 5, one modality copied, the runtime width)         err / bar 0.077
In all 17 blur and all 13 low-resolution cases, shifted relaunches included, no element differs in bits from the float32 evaluation
of the reference (recorded, not asserted: the order of operations is documented, but it is no contract of this test); every exact
comparison holds and every guard is intact.  Nothing was found wrong in csrc/augment_filter.hip.  The older test's zoom 0.99 is the
identity on every axis of (5, 7, 9), (16, 16, 16) and (1, 8, 33): a zoom near 1 that is no copy first runs here (X = 64 -> 63).
Mutations of a scratch copy of the library, each kept inside its buffers, and the cases that fail: blur_taps sending radius 5 to
blur_taps_n<4> and radius 1 to the pass-through -- exactly the eleven blur cases that hold a radius of 1 or 5; `ak <= rc[c]` as `<`
in the z pass -- all seventeen; filter_reflect with p - r (clamped to n - 1) -- all seventeen; lowres_source clamped to n - 2, and
the fraction taken with k + 1 -- each every low-resolution case but m1_one_low_voxel (one low voxel on every axis: all taps read it,
the weights sum to 1).
The slowest case takes 0.34 s (the first one: it loads the library), every other at most 0.09 s; the file takes 2.2 s on its own
(32 tests, start-up included).
"""
import time

import numpy as np
import pytest
import torch

import filter_cases as K
from float64_util import Figures, Guarded, _engine
from test_gpu_compound_float64 import GUARD, Inputs

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _blur_params(E, radii, taps):
    prm = E.BlurParams()
    for m, R in enumerate(radii):
        prm.radius[m] = int(R)
        for k in range(7):
            prm.taps[m][k] = float(taps[m][k])
    return prm


def _lowres_params(E, lows):
    prm = E.LowresParams()
    for m, (nx, ny, nz) in enumerate(lows):
        prm.nx[m], prm.ny[m], prm.nz[m] = int(nx), int(ny), int(nz)
    return prm


def _run(E, dev, fig, entry, x, prm, shift):
    """one launch into a fresh guarded dst; returns the result [Z][Y][X][M] (numpy) after the buffer checks"""
    Z, Y, X, M = x.shape
    i = Inputs(dev)
    src = i.put('src', torch.from_numpy(x), shift)
    dst = Guarded(x.size, GUARD, dev, shift=shift)
    assert src.data_ptr() % 16 == 4 * shift and dst.t.data_ptr() % 16 == 4 * shift
    E.call(entry, E.ptr(src), E.ptr(dst.t), X, Y, Z, M, prm, E.stream_ptr())
    torch.cuda.synchronize()
    fig.require(dst.guards_untouched(), 'dst: the guard bands were written')
    fig.require(dst.written(), 'dst: an element was not written (or is not finite)')
    i.unchanged(fig)
    return dst.t.cpu().numpy().reshape(x.shape)


def _compare(fig, tag, got, ref, yard, x, exact):
    """the bar of the module docstring; `exact`: the modalities that must equal the input bit for bit"""
    scale = float(np.abs(x).max())
    ye = float(np.abs(yard.astype(F64) - ref).max())
    lim = K.bar(ye, scale)
    if not np.isfinite(got).all():
        return
    err = float(np.abs(got.astype(F64) - ref).max())
    fig.figs.update({tag + 'err': err / scale, tag + 'yard': ye / scale, tag + 'bar': lim / scale, tag + 'err_over_bar': err / lim,
                     tag + 'bits_differ_from_fp32': float((_bits(got) != _bits(yard)).sum()), tag + 'elements': float(got.size)})
    fig.require(ye <= 0.25 * K.CAP * scale, '{}the fp32 yardstick {:.3e} is above a quarter of the cap'.format(tag, ye))
    if not err <= lim:
        at = np.unravel_index(int(np.abs(got.astype(F64) - ref).argmax()), got.shape)
        fig.fails.append('{}err {:.3e} > bar {:.3e} (yardstick {:.3e}, max|x| {:.3e}) at (z, y, x, m) = {}; {} elements above the bar'.format(
            tag, err, lim, ye, scale, at, int((np.abs(got.astype(F64) - ref) > lim).sum())))
    for m in exact:
        fig.require(np.array_equal(_bits(got[..., m]), _bits(x[..., m])), '{}modality {} is not bit-equal to the input'.format(tag, m))


def _case(hip_device, name, entry, c, x, prm, ref, yard, exact):
    E, dev, t0 = _engine(), hip_device, time.perf_counter()
    fig = Figures(name + '/' + c.name)
    first = None
    for tag, shift in K.launches(c):
        got = _run(E, dev, fig, entry, x, prm, shift)
        _compare(fig, tag, got, ref, yard, x, exact)
        again = _run(E, dev, fig, entry, x, prm, shift)
        fig.require(np.array_equal(_bits(again), _bits(got)), tag + 'two runs differ in bits')
        if first is None:
            first = got
        else:
            fig.require(np.array_equal(_bits(got), _bits(first)), tag + 'the launch one float past alignment differs in bits from the aligned one')
    fig.figs['seconds'] = time.perf_counter() - t0
    fig.done()


@pytest.mark.parametrize('case', K.BLUR_CASES, ids=K.case_id)
def test_blur(hip_device, case):
    c = case
    x, taps = K.crop(c), K.blur_taps(c)
    ref, yard = K.blur_ref(x, c.radii, taps, F64), K.blur_ref(x, c.radii, taps, F32)
    _case(hip_device, 'blur', 'seg3d_augment_blur', c, x, _blur_params(_engine(), c.radii, taps), ref, yard,
          [m for m, R in enumerate(c.radii) if R == 0])


@pytest.mark.parametrize('case', K.LOWRES_CASES, ids=K.case_id)
def test_lowres(hip_device, case):
    c = case
    x = K.crop(c)
    Z, Y, X = c.zyx
    ref, yard = K.lowres_ref(x, c.lows, F64), K.lowres_ref(x, c.lows, F32)
    _case(hip_device, 'lowres', 'seg3d_augment_lowres', c, x, _lowres_params(_engine(), c.lows), ref, yard,
          [m for m, low in enumerate(c.lows) if tuple(low) == (X, Y, Z)])


# ---- refusals: the entry's name in the message, dst untouched --------------------------------------------------------------------------
def _refused(E, entry, src, dst, X, Y, Z, M, prm):
    with pytest.raises(ValueError) as info:
        E.call(entry, E.ptr(src), E.ptr(dst.t), X, Y, Z, M, prm, E.stream_ptr())
    assert str(info.value).startswith(entry + ':'), str(info.value)
    torch.cuda.synchronize()
    assert dst.all_nan() and dst.guards_untouched()


def test_blur_refusals(hip_device):
    E, dev = _engine(), hip_device
    X, Y, Z = 6, 5, 4
    src = torch.ones(X * Y * Z * 9, device=dev)
    dst = Guarded(X * Y * Z * 9, GUARD, dev)
    good = K.gaussian_taps(3)
    trials = {}
    prm = _blur_params(E, (3, 7), [good, good])
    trials['radius 7'] = (src, X, Y, Z, 2, prm)
    prm = _blur_params(E, (3, 3), [good, good])
    prm.taps[1][2] = 1.5
    trials['a tap of 1.5'] = (src, X, Y, Z, 2, prm)
    prm = _blur_params(E, (3, 3), [good, good])
    trials['src and dst overlap'] = (dst.buf[dst.front + 8:dst.front + 8 + X * Y * Z * 2], X, Y, Z, 2, prm)
    trials['M = 9'] = (src, X, Y, Z, 9, prm)
    assert sorted(trials) == sorted(K.REFUSALS['seg3d_augment_blur'])
    for what, (s, *args) in trials.items():
        _refused(E, 'seg3d_augment_blur', s, dst, *args)


def test_lowres_refusals(hip_device):
    E, dev = _engine(), hip_device
    X, Y, Z = 6, 5, 4
    big = K.LOWRES_MAX_AXIS + 1
    src = torch.ones(max(X * Y * Z * 2, big), device=dev)
    dst = Guarded(max(X * Y * Z * 2, big), GUARD, dev)
    trials = {
        "n' = 0": (X, Y, Z, 2, _lowres_params(E, ((3, 3, 2), (3, 0, 2)))),
        "n' = n + 1": (X, Y, Z, 2, _lowres_params(E, ((3, 3, 2), (3, 3, Z + 1)))),
        'an axis of 16385': (big, 1, 1, 1, _lowres_params(E, ((8000, 1, 1),))),
    }
    assert sorted(trials) == sorted(K.REFUSALS['seg3d_augment_lowres'])
    for what, args in trials.items():
        _refused(E, 'seg3d_augment_lowres', src, dst, *args)
