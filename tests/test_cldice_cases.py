"""Host-only: (1) the layout restated in tests/cldice_cases.py equals the library's workspace queries; (2) every case of its tables has
the property it is named for -- tiles per axis, an interior tile, an axis at the limit, the block count of the sums kernel, the entries
of the column sum, the 16-byte or the scalar path -- and every <CT, VEC> instantiation of cld_region_partial_kernel and cld_bwd_kernel
is named by a case, the scalar one once by S % 4 != 0 and (in the device test's relaunch) once by a misaligned base; (3) the
selection-rule reference equals tests/cldice_oracle.py, values and autograd gradient, where that oracle is defined: on pairwise-distinct
planes -- and parts from it by whole units on tied planes; (4) on EVERY case the float32 and the float64 evaluation take the same
selection indices and the same gates (a > 0, b == 1), so the float32 yardstick of the device test measures rounding and nothing else;
(5) on the 'dyadic' and 'plateau' classes the float32 forward is bit-equal to float64 and at least 10 % of the skeleton is positive."""
import ctypes
import os

import pytest
import torch

import cldice_cases as L
import compound_cases as K
from cldice_oracle import cldice_oracle, soft_skeleton_oracle

QUERIES = ('seg3d_cldice_loss_workspace_bytes', 'seg3d_soft_skeleton_workspace_bytes', 'seg3d_dice_blocks')
F64, F32 = torch.float64, torch.float32
ALL_PAIRS = {(ct, v) for ct in (1, 2, 3, 4, 5, 16) for v in (False, True)}
_REFS = {}


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__  # noqa: F401  (repo root is on sys.path)
    from segmentation3d import _engine
    if not os.path.isfile(_engine.LIB_PATH):
        __graft_entry__.build()
    handle = ctypes.CDLL(_engine.LIB_PATH)
    for name in QUERIES:
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _engine._SIGNATURES[name]
    return handle


def _loss_refs(c):
    """(float64, float32) evaluation of a loss case, computed once"""
    if c not in _REFS:
        p, t, wd, wc, go = L.loss_inputs(c)
        _REFS[c] = tuple(L.cldice_ref(p, t, wd, wc, c, go, dt) for dt in (F64, F32))
    return _REFS[c]


def _same_gates(a, b):
    return all(torch.equal(x, y) for ga, gb in zip(L.gates(a), L.gates(b)) for x, y in zip(ga, gb))


# ---- sizes -------------------------------------------------------------------------------------------------------------------------
def test_constants_and_workspace_sizes(lib):
    assert (L.TX, L.TY, L.TZ, L.MAX_AXIS, L.MAX_ITERS, L.DICE_VPB) == (32, 8, 8, 256, 16, 4096)
    for c in L.LOSS_CASES:
        assert lib.seg3d_dice_blocks(L.voxels(c)) == K.blocks(L.voxels(c))
        assert lib.seg3d_cldice_loss_workspace_bytes(c.N, c.C, len(c.classes), c.X, c.Y, c.Z, c.iters) == L.loss_workspace_bytes(c)
        lay = L.layout(c.N, c.C, len(c.classes), L.voxels(c), c.iters)
        assert all(lay[k] % 4 == 0 for k in ('cpart', 'sp', 'st', 'buf', 'sa', 'sb', 'sel'))             # 16-byte offsets
    for c in L.SKEL_CASES:
        assert lib.seg3d_soft_skeleton_workspace_bytes(c.planes, c.X, c.Y, c.Z) == L.skel_workspace_bytes(c)


# ---- the tables --------------------------------------------------------------------------------------------------------------------
def test_skeleton_table():
    shapes = {(c.Z, c.Y, c.X): c for c in L.SKEL_CASES}
    assert {(z, y, x) for z, y, x, _ in L.SKEL_SHAPES} == set(shapes)
    want = {(1, 1, 1): (1, 1, 1), (1, 1, 32): (1, 1, 1), (1, 1, 33): (2, 1, 1), (8, 8, 32): (1, 1, 1), (9, 9, 33): (2, 2, 2),
            (17, 17, 65): (3, 3, 3), (2, 3, 256): (8, 1, 1), (256, 1, 2): (1, 1, 32), (1, 256, 3): (1, 32, 1), (2, 3, 5): (1, 1, 1)}
    for shape, c in shapes.items():
        assert L.tiles(c) == want[shape], shape
    assert {ax for c in L.SKEL_CASES for ax in range(3) if (c.Z, c.Y, c.X)[ax] == L.MAX_AXIS} == {0, 1, 2}
    assert max(c.planes for c in L.SKEL_CASES) == 600
    for fill in L.SKEL_FILLS:
        mine = [c for c in L.SKEL_CASES if c.fill == fill]
        assert len(mine) == len(L.SKEL_SHAPES)
        assert {c.iters for c in mine} == ({1, 3, 16} if fill in ('ranked', 'mask') else {1, 3, L.DYADIC_MAX_ITERS})
        assert any(min(L.tiles(c)) == 3 for c in mine)                # an interior tile with neighbours on both sides of every axis
    assert all(c.planes * L.voxels(c) <= 40000 for c in L.SKEL_CASES)


def test_loss_table_names_every_instantiation_block_count_and_option():
    cs = L.LOSS_CASES
    assert {(K.ct(c.C), L.vec(c)) for c in cs} == ALL_PAIRS
    assert {c.C for c in cs if L.vec(c)} == {1, 2, 3, 4, 5, 6, 7, 16}                    # <CT, true> at C = 1, 4 and the generic one
    assert {K.ct(c.C) for c in cs if not L.vec(c)} == {1, 2, 3, 4, 5, 16}               # the scalar path by S % 4 != 0
    plan = {L.BIG: ((3, 3, 3), 7, True), L.MID: ((3, 3, 3), 5, False), L.SMALL: ((2, 2, 2), 1, False), L.ROW: ((2, 1, 1), 1, False)}
    for c in cs:
        tiles, nblk, v = plan[(c.Z, c.Y, c.X)]
        assert (L.tiles(c), K.blocks(L.voxels(c)), L.vec(c)) == (tiles, nblk, v), c
        assert sorted(set(c.classes)) == sorted(c.classes) and all(0 <= k < c.C for k in c.classes)
    assert L.voxels(cs[0]) == 25920 and L.voxels(cs[0]) % L.DICE_VPB != 0 and 18785 % 4 == 1
    assert {L.column_entries(c) for c in cs if c.batch_dice} >= {21, 15, 7, 1}         # N * nblk under batch_dice
    assert {c.batch_dice for c in cs if K.blocks(L.voxels(c)) > 1 and c.N > 1} == {0, 1}
    assert {c.N for c in cs} == {1, 2, 3} and {c.iters for c in cs} >= {1, 2, 3, 16}
    assert {(c.dice_weight, c.cldice_weight) for c in cs} == {(1.0, 1.0), (0.0, 1.0), (0.7, 0.3), (1.0, 0.0)}
    assert any(len(c.classes) == 16 and list(c.classes) != sorted(c.classes) for c in cs)
    unsorted = [c for c in cs if list(c.classes) != sorted(c.classes) and c.cldice_weight > 0]
    assert {(c.C, c.classes) for c in unsorted} >= {(5, (3, 1)), (7, (6, 2))} and any(L.vec(c) for c in unsorted)
    assert any(0 <= c.ignore < c.C for c in cs) and any(c.ignore >= c.C for c in cs) and any(c.ignore < 0 for c in cs)
    assert sum(c.fill == 'empty' for c in cs) == 1
    assert {c.fill for c in cs if L.vec(c)} >= {'ranked', 'dyadic', 'plateau'} and {c.fill for c in cs if not L.vec(c)} >= {'ranked', 'plateau'}
    assert all(c.N * len(c.classes) * L.voxels(c) <= 420000 for c in cs)


def test_loss_inputs_hold_their_edges():
    for c in L.LOSS_CASES:
        p, t, wd, wc, go = L.loss_inputs(c)
        valid, cls = K.counting(t.reshape(c.N, -1), c.C, c.ignore)
        tf = t.reshape(-1)
        if c.fill == 'empty':
            assert not bool(valid.any())
            continue
        assert {-1.0, float(c.C), 1000.0} <= set(tf[-8:].tolist()) and go != 1.0
        if c.C >= 2:
            i = int((tf == 1.7).nonzero()[0])
            assert bool(valid.reshape(-1)[i]) and int(cls.reshape(-1)[i]) == 1 and float(wd[0]) == 0.0
        if c.N > 2:
            assert not bool(valid[1].any()) and bool(valid[0].any()) and bool(valid[2].any())
        if c.ignore >= c.C and c.Z >= 3:
            assert bool((t[0, c.Z // 2] == c.ignore).all())          # a wall across z
        if len(c.classes) >= 2:
            assert float(wc[1]) == 0.0 and float(wc[0]) > 0.0
        if c.fill == 'ranked':                                       # pairwise distinct per plane
            flat = p.reshape(c.N * c.C, -1)
            assert all(int(torch.unique(row).numel()) == row.numel() for row in flat)
        else:
            assert bool((p * 8.0 == torch.round(p * 8.0)).all()) and float(p.min()) == 0.0 and float(p.max()) == 1.0


# ---- the reference against the autograd oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('iters', [1, 3, 16])
def test_skeleton_reference_equals_the_autograd_oracle_on_distinct_planes(iters):
    x = L.planes_input(3150, 'cldice/host-{}'.format(iters), 2, 9, 10, 37, 'ranked')
    g = K._noise(3151, 'cldice/host-g-{}'.format(iters), (2, 9 * 10 * 37)).double()
    xa = x.double().requires_grad_(True)
    s = soft_skeleton_oracle(xa, iters)
    (s.reshape(2, -1) * g).sum().backward()
    mine, stages = L.skeleton_ref(x, iters, F64, keep=True)
    gx = L.skeleton_bwd_ref(stages, g).reshape(x.shape)
    assert float((mine - s.detach()).abs().max()) <= 1e-12 and float((gx - xa.grad).abs().max()) <= 1e-12
    assert float((mine > 0).double().mean()) > 0.3 and float(gx.abs().max()) > 0.1


@pytest.mark.parametrize('iters', [1, 3, 16])
def test_loss_reference_equals_the_autograd_oracle_on_distinct_planes(iters):
    c = L.Loss(2, 3, 9, 10, 37, (2, 1), iters, 0.7, 0.3, 0, L.NO_IGNORE, 'ranked')
    p = L.planes_input(3152, 'cldice/host-p-{}'.format(iters), 6, 9, 10, 37, 'ranked').reshape(2, 3, 9, 10, 37)
    t = K._labels(3153, 'cldice/host-t-{}'.format(iters), (2, 9, 10, 37), 3)            # every voxel counts: P_c stays distinct
    wd, wc = torch.tensor([0.25, 0.5, 0.25]), torch.tensor([0.75, 0.25])
    ref = L.cldice_ref(p, t, wd, wc, c, 1.0, F64)
    pa = p.double().requires_grad_(True)
    # the oracle normalises its weights: hand it normalised ones, and the clDice weights per class id
    w_of = [0.0, 0.25, 0.75]
    tot, ld, _ = cldice_oracle(pa, t.unsqueeze(1), weights=wd.tolist(), dice_weight=0.7, cldice_weight=0.0, iters=iters, cldice_classes=[2, 1])
    _, _, lc = cldice_oracle(pa, t.unsqueeze(1), weights=w_of, iters=iters, cldice_classes=[2, 1])
    (0.7 * ld + 0.3 * lc).backward()
    assert abs(float(ref["loss"][1]) - float(ld.detach())) <= 1e-12 and abs(float(ref["loss"][2]) - float(lc.detach())) <= 1e-12
    assert float((ref['dprobs'].reshape(p.shape) - pa.grad).abs().max()) <= 1e-12
    assert float(ref['dprobs'].abs().max()) > 1e-4


def test_autograd_oracle_parts_from_the_selection_rule_on_tied_planes():
    """what the existing oracle cannot notice: on multiples of 1/8 its gradient is whole units away from the lowest-index rule"""
    x = L.planes_input(3154, 'cldice/host-tie', 2, 9, 10, 37, 'plateau')
    g = torch.ones(2, 9 * 10 * 37, dtype=F64)
    xa = x.double().requires_grad_(True)
    s = soft_skeleton_oracle(xa, 3)
    s.sum().backward()
    mine, stages = L.skeleton_ref(x, 3, F64, keep=True)
    gx = L.skeleton_bwd_ref(stages, g).reshape(x.shape)
    assert torch.equal(mine, s.detach())                                               # the values agree: only the gradient's routing differs
    assert float((gx - xa.grad).abs().max()) >= 1.0
    assert abs(float(gx.sum()) - float(xa.grad.sum())) <= 1e-9                          # the same total, distributed differently


# ---- the conditions of the device test: no case excluded ----------------------------------------------------------------------------------
@pytest.mark.parametrize('case', L.SKEL_CASES, ids=L.case_id)
def test_skeleton_case_selections_do_not_depend_on_the_precision(case):
    c = case
    x = L.skel_input(c)
    (s64, st64), (s32, st32) = [L.skeleton_ref(x, c.iters, dt, keep=True) for dt in (F64, F32)]
    assert _same_gates(st64, st32)
    if c.fill == 'ranked':
        assert all(int(torch.unique(row).numel()) == row.numel() for row in x.reshape(c.planes, -1))
        assert float((s32.double() - s64).abs().max()) <= 1e-6
    else:
        assert torch.equal(s32.double(), s64)                         # 0 / 1 and multiples of 1/8: float32 is exact
    if c.fill == 'mask':
        assert bool(((s64 == 0) | (s64 == 1)).all())
    if c.fill in ('dyadic', 'plateau') and L.voxels(c) > 1:
        assert float((s64 > 0).double().mean()) >= 0.10
    if L.voxels(c) == 1:
        assert not bool(s64.any())                                    # a single voxel is its own opening


@pytest.mark.parametrize('case', L.LOSS_CASES, ids=L.case_id)
def test_loss_case_selections_do_not_depend_on_the_precision(case):
    c = case
    r64, r32 = _loss_refs(c)
    assert _same_gates(r64['stages'], r32['stages']) and len(r64['stages']) == c.iters + 1
    if c.fill in ('dyadic', 'plateau'):
        assert torch.equal(r32['sp'].double(), r64['sp']) and torch.equal(r32['st'].double(), r64['st'])
        assert float((r64['sp'] > 0).double().mean()) >= 0.10
    # the self-check of Figures.check: the yardstick stays within 1e-4 of the reference, relative to the scale
    for key in ('loss', 'coef', 'dprobs'):
        scale = float(r64[key].abs().max())
        assert float((r32[key].double() - r64[key]).abs().max()) <= 1e-4 * scale, key
    if c.fill == 'empty':
        assert not bool(r64['dprobs'].any()) and float(r64['loss'][0]) == 0.0
    else:
        assert float(r64['dprobs'].abs().max()) > 0.0
        off = ~r64['valid'].unsqueeze(1).expand_as(r64['dprobs'])
        assert not bool(r64['dprobs'][off].any())
        if c.dice_weight == 0.0:
            others = [k for k in range(c.C) if k not in c.classes]
            assert not bool(r64['dprobs'][:, others].any())
        if c.cldice_weight == 0.0:
            assert not bool(r64['coef'][2 * L.coef_rows(c) * c.C:].any())
