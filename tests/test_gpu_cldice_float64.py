"""The soft skeleton and the Dice + clDice loss driven through the C ABI (seg3d_soft_skeleton, seg3d_cldice_loss_fwd / _bwd) against the
selection-rule reference of tests/cldice_cases.py in float64.  The cases are those of tests/cldice_cases.py; tests/test_cldice_cases.py
shows on the host that each has the tiles per axis, the block count, the column-sum length and the <CT, VEC> instantiation it is named
for, and that on every case the float32 and the float64 evaluation of the reference take the same selections and gates.

Skeleton: (1,1,1), a full row and one past it, exactly one tile, one voxel into a second tile on every axis, three tiles per axis (an
interior workgroup whose halo comes from neighbours on both sides), every axis at the limit of 256, 600 planes; iters 1, 3, 16; planes
that are pairwise distinct (under bars), 0 / 1 masks and multiples of 1/8 with plateaus and saturated slabs (bit-equal to the reference).
Loss: 25 920 voxels in 7 blocks on the 16-byte path (launched a second time with probs, target and dprobs one float past a 16-byte
boundary: the scalar path, same bars), 18 785 voxels in 5 blocks on the scalar path, (9,9,33), (1,1,33); C = 1..7 and 16, K up to 16 in
a permuted order, unsorted class lists, N = 1..3, batch_dice over 21 column entries, iters 1, 2, 3, 10, 16, every term-weight pair,
gout != 1, unnormalised weights with a zero entry; targets with ids -1, C, 1000, a counted 1.7, the ignore label inside and outside
[0, C), an ignored wall across z, a sample and a whole case with nothing counted.  The tied value classes are the test of the selection
rule: the autograd oracle of the existing tests is whole units away from the header's lowest-index rule there
(test_cldice_cases.py::test_autograd_oracle_parts_from_the_selection_rule_on_tied_planes), the reference here follows the rule and the
gradient passes the same bars as on distinct planes.

Every output and workspace is a buffer of exactly the documented size inside guard bands, NaN-filled (the workspaces with a byte
pattern): afterwards every guard is bit-identical, every output element is finite and every input is bit-identical to what it was.
Bars (Figures.check): err <= min(4 * yardstick + floor * scale, cap), the yardstick the same reference in float32 on the CPU; floor
1e-5 for loss figures and coef, 2e-6 for the skeleton (per voxel) and the gradient (against the case's max |ref|); caps of the existing
tests: loss 1e-4 of max(1, |ref|), gradient relative L2 1e-4.  Exact: the skeleton of masks and of the dyadic classes; zeros on every
plane of a voxel that does not count and on planes outside the class list when dice_weight = 0; loss[1] bit-equal to
seg3d_compound_loss_fwd's on the same inputs and path; loss[0] == loss[1] * dice_weight when cldice_weight = 0; two runs bit-equal; a
refused call (iters 17, an axis of 257, a class id listed twice, a misaligned workspace, both term weights 0) writes nothing.

Figures, MI355X, the largest over the cases of a family, the scalar relaunches included (a run appends every figure to the parity
report that gpu_util.report writes):
    skeleton  ranked planes, per voxel  err 1.0e-7  yardstick 1.0e-7  bar 2.2e-6                         err / bar 0.048
              masks, dyadic and plateau planes: bit-equal in all 30 cases
    loss      loss    err 8.8e-7  yardstick 1.0e-6  (scale 20.1)                                         err / bar 0.006
              coef    err 2.6e-3  yardstick 5.6e-3  (scale 1.2e5: a sample with nothing counted)         err / bar 0.007
              dprobs  err / scale 2.1e-7  yardstick / scale 3.3e-7  bar / scale 3.3e-6; relative L2 1.3e-7 (cap 1e-4)  err / bar 0.074
Every exact comparison holds and every guard is intact; no defect was found in csrc/cldice_loss.hip.  The slowest case is the 16-stage
one at 25 920 voxels (0.25 s, both references, the scalar relaunch and the repeat runs included); the file takes 4 s: 40 skeleton cases,
21 loss cases and the refusals.

Mutations of csrc/cldice_loss.hip tried on scratch copies of the library, one at a time (every one stays inside its buffers); each
makes test_loss fail and nothing else: the first minimum of E turned into the last (`v <= e`) and the first maximum of D into the last
(`>=`) -- the 8 tied-class cases with the clDice term on fail, every ranked case passes, which is why the autograd oracle could not
see them; `want = 26 - code` turned into `code`, and `6 - p` into `p`, in cld_bwd_stage_kernel -- the 16 cases with the clDice term
on, C >= 2 and a counted voxel fail (with C = 1 every counted voxel is of the class, so dL/dSP = a1 + a2 = 0 there and next to nothing
enters the skeleton's backward); the `blockIdx.x` term of cld_sums_kernel's store dropped -- the 14 cases with more than one block fail.
"""
import ctypes
import time

import pytest
import torch

import cldice_cases as L
import compound_cases as K
from float64_util import FLOOR_EW, FLOOR_RED, Figures, _engine
from test_gpu_compound_float64 import Inputs, _finish, _loss_cap, _outputs, _rel_l2, _untouched, _written

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def _class_list(E, ids):
    return E.ClassList((ctypes.c_int * 16)(*(list(ids) + [0] * (16 - len(ids)))))


def _bits_equal(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ---- the skeleton entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', L.SKEL_CASES, ids=L.case_id)
def test_skeleton(hip_device, case):
    E, dev, c, t0 = _engine(), hip_device, case, time.perf_counter()
    fig = Figures('cldice/' + L.case_id(c))
    x = L.skel_input(c)
    ref, yard = [L.skeleton_ref(x, c.iters, dt) for dt in (F64, F32)]
    i = Inputs(dev)
    xd = i.put('x', x)
    nbytes = E.query('seg3d_soft_skeleton_workspace_bytes', c.planes, c.X, c.Y, c.Z)
    assert nbytes == L.skel_workspace_bytes(c)
    o = _outputs(dev, workspace=nbytes, skel=c.planes * L.voxels(c))
    E.call('seg3d_soft_skeleton', E.ptr(xd), E.ptr(o['skel'].t), E.ptr(o['workspace'].t), c.planes, c.X, c.Y, c.Z, c.iters, E.stream_ptr())
    torch.cuda.synchronize()
    _written(fig, o)
    i.unchanged(fig)
    got = o['skel'].t.cpu().reshape(ref.shape)
    if c.fill == 'ranked':
        fig.check('skel', got, ref, yard, FLOOR_EW)
    else:
        wrong = int((got.view(torch.int32) != ref.float().view(torch.int32)).sum())
        fig.figs['skel_wrong_bits'] = float(wrong)
        fig.require(wrong == 0, 'skel: {} voxels are not bit-equal to the reference'.format(wrong))
    _finish(fig, t0)


# ---- the loss --------------------------------------------------------------------------------------------------------------------------
def _run_loss(E, dev, c, p, t, wdice, wcl, gout, shift):
    N, C, nk = c.N, c.C, len(c.classes)
    i = Inputs(dev)
    pd, td = i.put('probs', p, shift), i.put('target', t, shift)
    wd, wk, gd = i.put('wdice', wdice), i.put('wcl', wcl), i.put('gout', torch.tensor([gout]))
    nbytes = E.query('seg3d_cldice_loss_workspace_bytes', N, C, nk, c.X, c.Y, c.Z, c.iters)
    assert nbytes == L.loss_workspace_bytes(c)
    o = _outputs(dev, shift, ('dprobs',), workspace=nbytes, coef=L.coef_floats(c), loss=3, dprobs=N * C * L.voxels(c))
    cl = _class_list(E, c.classes)
    E.call('seg3d_cldice_loss_fwd', E.ptr(pd), E.ptr(td), E.ptr(wd), E.ptr(wk), E.ptr(o['workspace'].t), E.ptr(o['coef'].t), E.ptr(o['loss'].t),
           N, C, c.X, c.Y, c.Z, cl, nk, c.iters, c.dice_weight, c.cldice_weight, c.batch_dice, c.ignore, E.stream_ptr())
    E.call('seg3d_cldice_loss_bwd', E.ptr(td), E.ptr(o['workspace'].t), E.ptr(o['coef'].t), E.ptr(gd), E.ptr(o['dprobs'].t), N, C, c.X, c.Y, c.Z,
           cl, nk, c.iters, c.cldice_weight, c.batch_dice, c.ignore, E.stream_ptr())
    torch.cuda.synchronize()
    return i, o, (pd, td, wd)


def _dice_bits(E, dev, c, pd, td, wd, got_lr, fig, tag):
    """loss[1] of the compound loss on the same inputs and path, bit for bit"""
    N, C, S = c.N, c.C, L.voxels(c)
    ones = torch.ones(C, device=dev)
    o = _outputs(dev, part=K.part_floats(N, C, S), coef=2 * L.coef_rows(c) * C + 1, loss=3)
    E.call('seg3d_compound_loss_fwd', E.ptr(pd), E.ptr(td), E.ptr(wd), E.ptr(ones), E.ptr(o['part'].t), E.ptr(o['coef'].t), E.ptr(o['loss'].t),
           N, C, S, 0.0, 1.0, 1.0, c.batch_dice, c.ignore, E.stream_ptr())
    torch.cuda.synchronize()
    mine = o['loss'].t.cpu()[1:2]
    fig.require(_bits_equal(mine, got_lr.reshape(1)),
                '{}loss[1] {:.9e} is not bit-equal to the compound loss\'s {:.9e}'.format(tag, float(got_lr), float(mine)))


@pytest.mark.parametrize('case', L.LOSS_CASES, ids=L.case_id)
def test_loss(hip_device, case):
    E, dev, c, t0 = _engine(), hip_device, case, time.perf_counter()
    N, C, S = c.N, c.C, L.voxels(c)
    fig = Figures('cldice/' + L.case_id(c))
    p, t, wdice, wcl, gout = L.loss_inputs(c)
    ref, yard = [L.cldice_ref(p, t, wdice, wcl, c, gout, dt) for dt in (F64, F32)]
    for tag, shift in [('', 0)] + ([('scalar_', 1)] if L.vec(c) else []):
        i, o, (pd, td, wd) = _run_loss(E, dev, c, p, t, wdice, wcl, gout, shift)
        _written(fig, o)
        i.unchanged(fig)
        loss, d = o['loss'].t.cpu(), o['dprobs'].t.cpu()
        fig.check(tag + 'loss', loss, ref['loss'], yard['loss'], FLOOR_RED, cap=_loss_cap(ref['loss']))
        fig.check(tag + 'coef', o['coef'].t.cpu(), ref['coef'], yard['coef'], FLOOR_RED)
        fig.check(tag + 'dprobs', d, ref['dprobs'], yard['dprobs'], FLOOR_EW)
        _rel_l2(fig, tag + 'dprobs', d, ref['dprobs'])
        d = d.reshape(N, C, S)
        off = ~ref['valid'].unsqueeze(1).expand(N, C, S)
        fig.require(bool((d[off] == 0.0).all()), tag + 'dprobs: not 0.0 on a voxel that does not count')
        if c.dice_weight == 0.0:
            others = [k for k in range(C) if k not in c.classes]
            fig.require(bool((d[:, others] == 0.0).all()), tag + 'dprobs: dice_weight is 0, a plane outside the class list is not 0.0')
        if c.cldice_weight == 0.0:
            want = (loss[1:2].double() * c.dice_weight).float()
            fig.require(_bits_equal(loss[0:1], want), tag + 'loss[0] != loss[1] * dice_weight with the clDice term off')
        _dice_bits(E, dev, c, pd, td, wd, loss[1], fig, tag)
        # a second run of the same launch: bit-equal
        _, o2, _ = _run_loss(E, dev, c, p, t, wdice, wcl, gout, shift)
        for k in ('loss', 'coef', 'dprobs'):
            fig.require(_bits_equal(o[k].t, o2[k].t), '{}{}: two runs differ'.format(tag, k))
    _finish(fig, t0)


# ---- one refusal per SEG3D_REQUIRE family of every entry: the error comes back and every output is still untouched ----------------------
def test_refusals(hip_device):
    E, dev = _engine(), hip_device
    N, C, X, Y, Z, it = 1, 3, 8, 4, 2, 2
    S = X * Y * Z
    ones, st = torch.ones(4 * 257 * 4 + 8, device=dev), E.stream_ptr
    nbytes = E.query('seg3d_cldice_loss_workspace_bytes', N, C, 2, 257, Y, Z, it)
    o = _outputs(dev, workspace=nbytes + 16, skel=257 * Y * Z, coef=2 * C + 3 * 2, loss=3, dprobs=C * 257 * Y * Z)
    P, q = E.ptr(ones), {k: E.ptr(g.t) for k, g in o.items()}
    off4 = ctypes.c_void_p(o['workspace'].t.data_ptr() + 4)
    ok, twice = _class_list(E, (1, 2)), _class_list(E, (2, 2))
    calls = [
        ('seg3d_soft_skeleton', (P, q['skel'], q['workspace'], 1, X, Y, Z, 17, st())),
        ('seg3d_soft_skeleton', (P, q['skel'], q['workspace'], 1, 257, Y, Z, it, st())),
        ('seg3d_cldice_loss_fwd', (P, P, P, P, q['workspace'], q['coef'], q['loss'], N, C, X, Y, Z, twice, 2, it, 1.0, 1.0, 0, -1.0, st())),
        ('seg3d_cldice_loss_fwd', (P, P, P, P, off4, q['coef'], q['loss'], N, C, X, Y, Z, ok, 2, it, 1.0, 1.0, 0, -1.0, st())),
        ('seg3d_cldice_loss_fwd', (P, P, P, P, q['workspace'], q['coef'], q['loss'], N, C, X, Y, Z, ok, 2, it, 0.0, 0.0, 0, -1.0, st())),
        ('seg3d_cldice_loss_bwd', (P, q['workspace'], P, P, q['dprobs'], N, C, 257, Y, Z, ok, 2, it, 1.0, 0, -1.0, st())),
        ('seg3d_cldice_loss_bwd', (P, off4, P, P, q['dprobs'], N, C, X, Y, Z, ok, 2, it, 1.0, 0, -1.0, st())),
    ]
    assert sorted({n for n, _ in calls}) == sorted(L.REFUSALS) and all(sum(n == k for n, _ in calls) == len(v) for k, v in L.REFUSALS.items())
    assert S * C <= ones.numel()
    for name, args in calls:
        with pytest.raises(ValueError) as info:
            E.call(name, *args)
        assert str(info.value).startswith(name + ':'), (name, str(info.value))
    torch.cuda.synchronize()
    assert _untouched(o)
