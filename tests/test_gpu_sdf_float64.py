"""seg3d_signed_distance (sdf_x_kernel<J>, sdf_line_kernel<false / true> of csrc/boundary_loss.hip) driven through the C ABI against
the float64 brute force of tests/sdf_cases.py (the one of tests/boundary_oracle.py).  The cases are those of tests/sdf_cases.py;
tests/test_sdf_cases.py shows on the host that each reaches the J, tiles, LDS bytes and grids it is named for: X = 64, 128, 129, 192,
193 (J = 1..4 at both edges of each), a 256-voxel line in pass z, one and two 32-line tiles full and partial in pass y and pass z,
lines that are no multiple of 4; unit and (0.7, 1.3, 2.5) spacing everywhere, (1e-6, 1e-6, 1e-6), (1e6, 1e6, 1e6) and (1e6, 1e-6, 1)
on (9, 7, 5) and (193, 2, 1); the label patterns of tests/test_gpu_boundary_loss.py plus in-contract fractional targets (0.5, 1.7,
num_class - 0.25, -0.0), -0.5, and an ignore label that is itself fractional; one class id, a permuted list with an id >= num_class
(its plane is all zero), 16 ids; N = 3 with one sample entirely ignored; N K = 65520 on (2, 1, 1), grid y next to its limit.

phi is a buffer of exactly N K X Y Z floats filled with NaN, the workspace one of exactly seg3d_signed_distance_workspace_bytes bytes
filled with a fixed pattern, both inside guard bands: afterwards the guards are bit-identical, every element of phi is finite and the
target is bit-identical to what it was.  Two runs are bit-equal.

Bars: nothing is pinned to what the kernels give.  Signs and zeros are exact in every case.  Unit spacing: round(phi^2) is the exact
integer and |phi| within 1 ulp of the rounded root (the rule of tests/test_gpu_boundary_loss.py).  Any other spacing: the relative
error of every non-zero element <= min(4 * yardstick + 2e-7, 1e-6), the yardstick the largest relative error of the float32 evaluation
of the same brute force (weights rounded once to float32, as the entry does), the cap the derived bar of the existing test;
tests/test_sdf_cases.py holds every yardstick at or below a quarter of the cap.  The number of elements whose bits differ from the
float32 evaluation is recorded, not asserted.

Figures, MI355X, the largest over the cases (a run appends every figure to the parity report that gpu_util.report writes):
    unit spacing    round(phi^2) the exact integer and |phi| 0 ulp off the rounded root in every case; signs and zeros exact
    other spacing   relative err 8.8e-8  yardstick 8.8e-8  bar 5.5e-7  ((193, 2, 1), (0.7, 1.3, 2.5), 16 ids)     err / bar 0.16
                    spacing 1e-6: 5.6e-8 (bar 4.3e-7); 1e6: 8.4e-8 (bar 5.3e-7); (1e6, 1e-6, 1): 3.5e-8 (bar 3.4e-7)
7 of the 1680 elements of the (5, 7, 3) anisotropic case differ in bits from the float32 evaluation (passes y and z fuse each
product with its sum, the brute force rounds both), none anywhere else (recorded, not asserted).  Every guard is intact, two runs are
bit-equal in every case.  Nothing was found wrong in the distance kernels of csrc/boundary_loss.hip.
Mutations of a scratch copy of the library, each kept inside its buffers, and the cases that fail: sdf_x_kernel<3> dispatched as <2> --
exactly the four cases with X = 129 and X = 192; `ct == c ? hv : gv` swapped -- every case; (int)t replaced by a rounding in the map's
class -- every case with a fractional pattern (all but n4095_k16_grid_y_aniso, whose targets are integers).
The slowest case takes 0.04 s (N K = 65520, anisotropic); the file takes 2.6 s on its own (28 tests, start-up and the
brute-force references included).
"""
import time

import numpy as np
import pytest
import torch

import sdf_cases as K
from float64_util import Figures, Guarded, _engine
from test_gpu_compound_float64 import GUARD, Inputs
from test_sdf_cases import _case_seed

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32


def _class_list(E, ids):
    cls = E.ClassList()
    for i, c in enumerate(ids):
        cls.id[i] = int(c)
    return cls


def _run(E, dev, fig, t, ids, nlab, spacing, ignore):
    N, Z, Y, X = t.shape
    k = len(ids)
    nbytes = E.query('seg3d_signed_distance_workspace_bytes', N, k, X, Y, Z)
    assert nbytes == K.workspace_bytes(N, k, X, Y, Z)
    i = Inputs(dev)
    td = i.put('target', torch.from_numpy(t))
    phi, work = Guarded(N * k * X * Y * Z, GUARD, dev), Guarded(nbytes, GUARD, dev, dtype=torch.uint8)
    E.call('seg3d_signed_distance', E.ptr(td), E.ptr(phi.t), E.ptr(work.t), N, X, Y, Z, _class_list(E, ids), k, nlab,
           float(spacing[0]), float(spacing[1]), float(spacing[2]), float(ignore), E.stream_ptr())
    torch.cuda.synchronize()
    fig.require(phi.guards_untouched(), 'phi: the guard bands were written')
    fig.require(work.guards_untouched(), 'workspace: the guard bands were written')
    fig.require(phi.written(), 'phi: an element was not written (or is not finite)')
    i.unchanged(fig)
    return phi.t.cpu().numpy().reshape(N, k, Z, Y, X)


@pytest.mark.parametrize('case', K.CASES, ids=K.case_id)
def test_signed_distance(hip_device, case):
    E, dev, c, t0 = _engine(), hip_device, case, time.perf_counter()
    ids, nlab = K.CLASS_LISTS[c.classes]
    fig = Figures('sdf/' + c.name)
    worst = {'err': 0.0, 'yard': 0.0, 'bar': K.bar(0.0), 'err_over_bar': 0.0, 'ulps': 0.0, 'bits_differ_from_fp32': 0.0, 'elements': 0.0}
    for p in c.patterns:
        t, ignore = K.labels(p, c, _case_seed(c, p))
        (ref, d2), yard = K.sdf_ref(t, ids, c.spacing, nlab, ignore, F64, squared=True), K.sdf_ref(t, ids, c.spacing, nlab, ignore, F32)
        got = _run(E, dev, fig, t, ids, nlab, c.spacing, ignore)
        again = _run(E, dev, fig, t, ids, nlab, c.spacing, ignore)
        fig.require(np.array_equal(got.view(np.int32), again.view(np.int32)), p + ': two runs differ in bits')
        if not np.isfinite(got).all():
            continue
        fig.require(np.array_equal(np.sign(got), np.sign(ref)), p + ': a sign or a zero is wrong')
        worst['bits_differ_from_fp32'] += float((got.view(np.int32) != yard.view(np.int32)).sum())
        worst['elements'] += float(got.size)
        g64 = got.astype(F64)
        if c.spacing == K.UNIT:
            fig.require(np.array_equal(np.rint(g64 * g64), d2), p + ': round(phi^2) is not the exact integer')
            root = np.sqrt(d2).astype(F32)
            ulps = float((np.abs(np.abs(got) - root) / np.spacing(np.maximum(root, F32(1e-30)))).max())
            worst['ulps'] = max(worst['ulps'], ulps)
            fig.require(ulps <= 1.0, '{}: |phi| is {} ulp off the rounded root'.format(p, ulps))
        else:
            ye, err = K.rel_err(yard, ref), K.rel_err(got, ref)
            lim = K.bar(ye)
            fig.require(ye <= 0.25 * K.CAP, '{}: the fp32 yardstick {:.3e} is above a quarter of the cap'.format(p, ye))
            fig.require(err <= lim, '{}: relative err {:.3e} > bar {:.3e} (yardstick {:.3e})'.format(p, err, lim, ye))
            if err / lim >= worst['err_over_bar']:
                worst.update(err=err, yard=ye, bar=lim, err_over_bar=err / lim)
    fig.figs.update(worst)
    fig.figs['seconds'] = time.perf_counter() - t0
    fig.done()


# ---- refusals: the entry's name in the message, phi and the workspace untouched --------------------------------------------------------
def test_refusals(hip_device):
    E, dev, name = _engine(), hip_device, 'seg3d_signed_distance'
    big_n = 4096                                                      # N * K = 65536 with 16 ids
    target = torch.ones(max(big_n, 2 * 257), device=dev)
    phi = Guarded(max(big_n * 16, 2 * 17 * 257), GUARD, dev)
    work = Guarded(K.workspace_bytes(big_n, 16, 1, 1, 1), GUARD, dev, dtype=torch.uint8)
    assert K.workspace_bytes(big_n, 16, 1, 1, 1) >= K.workspace_bytes(2, 17, 257, 1, 1)
    T, P, W = E.ptr(target), E.ptr(phi.t), E.ptr(work.t)
    cls, nan = _class_list(E, range(16)), float('nan')
    trials = {
        'an axis of 257': (T, P, W, 2, 257, 1, 1, cls, 1, 3, 1.0, 1.0, 1.0),
        'K = 0': (T, P, W, 2, 4, 3, 2, cls, 0, 3, 1.0, 1.0, 1.0),
        'K = 17': (T, P, W, 2, 4, 3, 2, cls, 17, 3, 1.0, 1.0, 1.0),
        'spacing 0': (T, P, W, 2, 4, 3, 2, cls, 1, 3, 1.0, 0.0, 1.0),
        'spacing NaN': (T, P, W, 2, 4, 3, 2, cls, 1, 3, 1.0, 1.0, nan),
        'spacing 1e7': (T, P, W, 2, 4, 3, 2, cls, 1, 3, 1e7, 1.0, 1.0),
        'N * K = 65536': (T, P, W, big_n, 1, 1, 1, cls, 16, 16, 1.0, 1.0, 1.0),
        'a null workspace': (T, P, None, 2, 4, 3, 2, cls, 1, 3, 1.0, 1.0, 1.0),
    }
    assert sorted(trials) == sorted(K.REFUSALS)
    for what, args in trials.items():
        with pytest.raises(ValueError) as info:
            E.call(name, *args, K.NO_IGNORE, E.stream_ptr())
        assert str(info.value).startswith(name + ':'), (what, str(info.value))
    torch.cuda.synchronize()
    assert phi.all_nan() and phi.guards_untouched() and work.all_nan() and work.guards_untouched()
