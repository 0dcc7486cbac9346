"""Host-only: (1) the rules restated in tests/ds_head_cases.py give the slab count of seg3d_ds_head_bwd_workspace_floats for every case;
(2) every <C, VPI, NQ> of ds_head_fwd_kernel and of ds_head_bwd_kernel (C = 1..8 x NQ = 1, 2, 4, VPI a function of the two) is named
by a case with a full channel count and by one with a partly filled lane group, whose `q < nq` guards are taken; (3) every case has the
tile count, the voxel tail, the strides, the optional operands and the grid-stride trip it is named for -- for 256 compute units, the
count the table is built for; (4) tests/test_gpu_deep_supervision.py::test_head_grid_stride_loop takes the trip its docstring claims;
(5) the float64 reference equals autograd through conv3d + softmax, and the float32 yardstick stays within 1e-4 of it."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import ds_head_cases as H

F64, F32 = torch.float64, torch.float32
ALL_CASES = H.CASES + H.TRIP_CASES


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__  # noqa: F401  (repo root is on sys.path)
    from segmentation3d import _engine
    if not os.path.isfile(_engine.LIB_PATH):
        __graft_entry__.build()
    handle = ctypes.CDLL(_engine.LIB_PATH)
    for name in ('seg3d_ds_head_bwd_workspace_floats', 'seg3d_ds_head_supported'):
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _engine._SIGNATURES[name]
    return handle


def test_constants_and_workspace_sizes(lib):
    assert (H.MAX_CIN, H.MAX_C, H.GROUP, H.GROUPS, H.BWD_MAX_BLOCKS) == (256, 8, 16, 16, 1024)
    assert [H.nq(c) for c in (4, 64, 68, 128, 132, 256)] == [1, 1, 2, 2, 4, 4]
    assert [H.fwd_vpi(q) for q in H.NQS] == [8, 4, 4]
    assert {(C, q): H.bwd_vpi(C, q) for C in (1, 2, 4, 5, 8) for q in (1, 4)} == {
        (1, 1): 8, (1, 4): 8, (2, 1): 8, (2, 4): 4, (4, 1): 8, (4, 4): 2, (5, 1): 4, (5, 4): 1, (8, 1): 4, (8, 4): 1}
    for c in ALL_CASES:
        assert lib.seg3d_ds_head_supported(c.Cin, c.C) == 1
        assert lib.seg3d_ds_head_bwd_workspace_floats(c.N, c.S, c.Cin, c.C) == H.workspace_floats(c), c
        assert H.workspace_floats(c) == H.bwd_slabs(c.N * c.S, c.Cin, c.C) * (c.C * c.Cin + c.C)


def test_every_instantiation_is_named_full_and_partial():
    every = {(C, q) for C in range(1, H.MAX_C + 1) for q in H.NQS}
    fwd = {(C, H.fwd_vpi(q), q) for C, q in every}
    bwd = {(C, H.bwd_vpi(C, q), q) for C, q in every}
    assert len(fwd) == len(bwd) == 24 and {v for _, v, _ in bwd} == {8, 4, 2, 1}
    for partial in (False, True):
        mine = [c for c in H.CASES if H.partial_group(c) == partial]
        assert {H.fwd_plan(c)[0] for c in mine} == fwd and {H.bwd_plan(c)[0] for c in mine} == bwd
    assert {c.Cin for c in H.CASES if not H.partial_group(c)} == {64, 128, 256}
    assert {c.Cin for c in H.CASES} >= {4, 36, 60, 68, 100, 124, 132, 200, 252}
    # a partly filled group: with Cin / 4 quads, lane j of 16 holds quad j + 16 i only while that is below Cin / 4
    for c in H.CASES:
        quads = c.Cin // 4
        idle = [(j, i) for j in range(H.GROUP) for i in range(H.nq(c.Cin)) if j + H.GROUP * i >= quads]
        assert bool(idle) == H.partial_group(c)
        assert c.C * quads <= 256 * 8                                # the staging loop: C * Cin / 4 quads, 256 threads a step
    assert any(c.C * c.Cin // 4 > 256 for c in H.CASES) and any(c.C * c.Cin // 4 < 256 and (c.C * c.Cin // 4) % 256 for c in H.CASES)


def test_voxel_counts_strides_and_operands():
    for vpi_of, name in ((lambda c: H.fwd_plan(c)[0][1], 'forward'), (lambda c: H.bwd_plan(c)[0][1], 'backward')):
        for vpi in ((8, 4) if name == 'forward' else (8, 4, 2, 1)):
            mine = [c for c in H.CASES if vpi_of(c) == vpi]
            tile = H.GROUPS * vpi
            tails = {(c.N * c.S) % tile for c in mine}
            assert len(tails - {0}) >= 2, (name, vpi)                                                   # a tile that ends early
            assert vpi == 1 or any((c.N * c.S) % vpi for c in mine), (name, vpi)                        # ... inside a group's run
            assert any(c.N * c.S > tile for c in mine), (name, vpi)                                     # more than one tile
    vs = {c.N * c.S for c in H.CASES}
    assert 1 in vs and {c.N for c in H.CASES} == {1, 2, 3}
    assert all(c.S % 2 == 1 for c in H.CASES if c.N > 1)                 # a sample boundary inside a run of voxels
    for c in H.CASES:
        q = H.nq(c.Cin)
        tf, tb = H.GROUPS * H.fwd_vpi(q), H.GROUPS * H.bwd_vpi(c.C, q)
        assert c.N * c.S in (1, tf - 1, tf + 1, 2 * tf + 3, tb - 1, tb + 1, 2 * tb + 3, 2 * tb + 2), c
        assert not H.fwd_plan(c)[3] and not H.bwd_plan(c)[3] and c.N * c.S * c.Cin <= 70000
        ldx, sx, ldd, sd = H.strides(c)
        assert (ldx == 0 or (ldx >= c.Cin and ldx % 4 == 0)) and (ldd == 0 or (ldd >= c.Cin and ldd % 4 == 0))
        assert c.dw or c.db
        assert c.bias or c.values in ('zero', 'std', 'equal', 'wide')
    assert {(c.ldx, c.ld_dx) for c in H.CASES} >= {('packed', 'pad'), ('pad', 'slice'), ('slice', 'packed'), ('pad', 'packed')}
    assert any(H.strides(c)[1] != H.strides(c)[3] for c in H.CASES)
    assert {c.accumulate for c in H.CASES} == {0, 1, 2, 3} and {c.accumulate for c in H.CASES if c.dw and c.db} == {0, 1, 2, 3}
    assert {(c.dw, c.db) for c in H.CASES} == {(1, 1), (0, 1), (1, 0)} and {c.bias for c in H.CASES} == {0, 1}
    assert {c.values for c in H.CASES} == set(H.VALUES) and {c.dprobs for c in H.CASES} == {'dense', 'plane'}
    assert all(not c.bias for c in H.CASES if c.values == 'zero')


def test_trip_cases_take_the_second_trip():
    f4, f68, b1, b8 = H.TRIP_CASES
    assert H.fwd_plan(f4) == ((2, 8, 1), 8 * H.CUS + 1, 8 * H.CUS, True) and f4.Cin == 4 and f4.N * f4.S == 262150
    assert H.fwd_plan(f68) == ((3, 4, 2), 8 * H.CUS + 1, 8 * H.CUS, True) and f68.Cin == 68 and f68.N * f68.S == 131077
    assert H.bwd_plan(b1) == ((5, 1, 4), H.BWD_MAX_BLOCKS + 1, H.BWD_MAX_BLOCKS, True) and b1.N * b1.S == 16397
    assert H.bwd_plan(b8) == ((4, 8, 1), H.BWD_MAX_BLOCKS + 1, H.BWD_MAX_BLOCKS, True) and H.partial_group(b8)
    assert all((c.N * c.S) % (H.GROUPS * H.fwd_vpi(H.nq(c.Cin))) for c in (f4, f68))               # the last tile is partial
    assert H.bwd_plan(f4)[3] and not H.fwd_plan(b1)[3] and not H.fwd_plan(b8)[3]
    assert f4.S % 2 == 1 and b8.S % 2 == 1 and b8.N == 3
    # a device with fewer compute units only lowers the grids: the trips stay
    for cus in (64, 128, 256):
        assert H.fwd_plan(f4, cus)[3] and H.fwd_plan(f68, cus)[3] and H.bwd_plan(b1, cus)[3] and H.bwd_plan(b8, cus)[3]


def test_existing_grid_stride_test_is_what_its_docstring_says():
    """tests/test_gpu_deep_supervision.py::test_head_grid_stride_loop: 52^3 voxels of 64 channels, C = 2"""
    c = H.Head(1, 52 ** 3, 64, 2, 'packed', 'packed', 1, 0, 1, 1, 'std', 'dense')
    assert H.fwd_plan(c) == ((2, 8, 1), 1099, 1099, False)            # 128 voxels a tile: one tile per workgroup, no trip
    assert H.bwd_plan(c) == ((2, 8, 1), 1099, 1024, True)             # 1099 tiles on 1024 workgroups: 75 of them walk two
    assert 52 ** 3 % 128 == 64


# ---- the reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [H.CASES[5], H.CASES[18], H.CASES[41]], ids=H.case_id)
def test_reference_equals_autograd(case):
    c = case
    x, w, b, d, _, _ = H.inputs(c)
    xa, wa, ba = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    vol = xa.reshape(c.N, c.S, 1, 1, c.Cin).permute(0, 4, 1, 2, 3)
    p = F.softmax(F.conv3d(vol, wa.reshape(c.C, c.Cin, 1, 1, 1), ba), dim=1).reshape(c.N, c.C, c.S)
    (p * d.double()).sum().backward()
    mine = H.fwd_ref(x, w, b, c.N, c.S, F64)
    assert float((mine - p.detach()).abs().max()) <= 1e-14
    dx, dw, db = H.bwd_ref(p.detach(), d, x, w, F64)
    for got, want in ((dx, xa.grad), (dw, wa.grad), (db, ba.grad)):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize('case', ALL_CASES, ids=H.case_id)
def test_inputs_and_yardstick(case):
    c = case
    x, w, b, d, dw0, db0 = H.inputs(c)
    bb = b if c.bias else None
    p64, p32 = [H.fwd_ref(x, w, bb, c.N, c.S, dt) for dt in (F64, F32)]
    assert float((p32.double() - p64).abs().max()) <= 1e-4
    logits = x.double() @ w.double().t()
    if c.values == 'zero':
        assert torch.equal(p32, torch.full_like(p32, 1.0) / c.C)
    elif c.values == 'equal':
        flat = p32.permute(0, 2, 1).reshape(-1, c.C)
        assert not bool(logits[0::2].any()) and torch.equal(flat[0::2], torch.full_like(flat[0::2], 1.0) / c.C)
    elif c.values == 'wide' and c.N * c.S * c.C >= 64:
        assert float(logits.abs().max()) > 40.0
    if c.dprobs == 'plane':
        assert bool(((d != 0).sum(1) <= 1).all()) and bool(d.any())
    g64, g32 = [H.bwd_ref(p64.float(), d, x, w, dt) for dt in (F64, F32)]
    for a, r in zip(g32, g64):
        assert float((a.double() - r).abs().max()) <= 1e-4 * float(r.abs().max())


def test_pyramid_input_carries_bit_patterns():
    m = H.pyramid_input()
    assert tuple(m.shape) == H.PYRAMID_SHAPE and all(s % 8 == 0 for s in H.PYRAMID_SHAPE[1:])
    coarse = m[:, ::8, ::8, ::8]
    assert bool(torch.isnan(m).any()) and bool(torch.isinf(m).any()) and bool(torch.isnan(coarse).any())
    assert int(torch.unique(m.view(torch.int32)[torch.isnan(m)]).numel()) >= 3                    # NaNs with different payloads
