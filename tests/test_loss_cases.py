"""Host-only: (1) the float64 references of tests/loss_cases.py reproduce what the reference project's own loss modules recorded in
tests/golden/loss_* and small_losses (the keys tests/test_gpu_kernels.py reads), within 1e-6 relative to max(1, |.|) -- the oracle of
tests/test_gpu_loss_float64.py is pinned to the reference itself; (2) every case of the tables has the property it is named for:
the block count the library reports, whether the Dice finalize takes its second strided step, its number of (n, c) rounds, whether
an element-wise kernel takes a second grid-stride trip, which copy cases take the 16-byte path."""
import ctypes
import os

import pytest
import torch

import loss_cases as K
from conftest import golden_npz

QUERIES = ('seg3d_dice_blocks', 'seg3d_focal_blocks')


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


def _close(got, want, what):
    want = torch.as_tensor(want).double().reshape(got.shape)
    err = ((got.double() - want).abs() / want.abs().clamp(min=1.0)).max()
    assert float(err) <= 1e-6, '{}: {:.3e}'.format(what, float(err))


def _normalised(w):
    w = torch.tensor(w, dtype=torch.float32)
    return w / w.sum()                               # what MultiDiceLoss / FocalLoss do with the weights they are given


# ---- the references against the reference project's recorded results -------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ties2', 'allbg4', 'rand2', 'rand5'])
def test_dice_and_focal_references_reproduce_the_fixtures(name):
    gold = golden_npz('loss_' + name)
    N, C = gold['probs'].shape[:2]
    p = torch.from_numpy(gold['probs']).reshape(N, C, -1)
    t = torch.from_numpy(gold['target']).reshape(N, -1)
    for wname, w in (('uniform', [1.0] * C), ('ramp', [1.0 + i for i in range(C)])):
        loss, _, d, _ = K.dice_ref(p, t, _normalised(w), 1.0, torch.float64)
        _close(loss, gold['dice_' + wname], (name, wname))
        _close(d, gold['dice_{}_grad'.format(wname)], (name, wname, 'grad'))
    for gname, gamma, alpha in (('g2', 2.0, [1.0] * C), ('g0', 0.0, [1.0] * C), ('g1p5_alpha', 1.5, [1.0 + i for i in range(C)])):
        loss, d, _ = K.focal_ref(p, t, _normalised(alpha), gamma, 1, 1.0, torch.float64)
        _close(loss, gold['focal_' + gname], (name, gname))
        _close(d, gold['focal_{}_grad'.format(gname)], (name, gname, 'grad'))


@pytest.mark.parametrize('name', ['b2', 'b3_ties'])
def test_binary_dice_reference_reproduces_the_fixtures(name):
    gold = golden_npz('small_losses')
    N = gold['bdice_{}/probs'.format(name)].shape[0]
    p = torch.from_numpy(gold['bdice_{}/probs'.format(name)]).reshape(N, 2, -1)
    t = torch.from_numpy(gold['bdice_{}/target'.format(name)]).reshape(N, -1)
    loss, _, d = K.bdice_ref(p, t, 1.0, torch.float64)
    _close(loss, gold['bdice_{}/loss'.format(name)], name)
    _close(d, gold['bdice_{}/grad'.format(name)], (name, 'grad'))
    assert bool((d[:, 0] == 0.0).all())


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
def _dice_plan(N, C, S):
    """(blocks, second strided step of the finalize, finalize rounds, second trip of the backward)"""
    nblk = (S + K.DICE_VPB - 1) // K.DICE_VPB
    return nblk, nblk > K.FIN_LANES, (N * C + K.FIN_PAIRS - 1) // K.FIN_PAIRS, N * S > K.ITEMS_PER_TRIP


DICE_PLANS = [(1, False, 1, False), (1, False, 1, False), (1, False, 2, False), (2, False, 4, False), (34, True, 2, False),
              (513, True, 1, True)]
BDICE_PLANS = [(1, False, 1, False), (1, False, 1, False), (2, False, 2, False), (34, True, 1, False)]


def test_constants():
    assert (K.DICE_VPB, K.FIN_LANES, K.FIN_PAIRS, K.ITEMS_PER_TRIP, K.MAXC) == (4096, 32, 8, 8192 * 256, 16)


@pytest.mark.parametrize('case,plan', list(zip(K.DICE_CASES, DICE_PLANS)), ids=[K.case_id(c) for c in K.DICE_CASES])
def test_dice_case_reaches_its_plan(lib, case, plan):
    assert lib.seg3d_dice_blocks(case.S) == plan[0]
    assert _dice_plan(*case) == plan and case.C <= K.MAXC


@pytest.mark.parametrize('case,plan', list(zip(K.BDICE_CASES, BDICE_PLANS)), ids=[K.case_id(c) for c in K.BDICE_CASES])
def test_binary_dice_case_reaches_its_plan(lib, case, plan):
    assert lib.seg3d_dice_blocks(case.S) == plan[0]
    assert _dice_plan(case.N, 1, case.S) == plan            # the finalize runs with C = 1: a second round needs N > 8


def test_dice_tables_cover_the_edges():
    cs = K.DICE_CASES
    assert {c.S for c in cs} >= {1, K.DICE_VPB - 1, K.DICE_VPB, K.DICE_VPB + 1} and {1, K.MAXC, 3, 5} <= {c.C for c in cs}
    pairs = [c.N * c.C for c in cs]
    assert any(n % 8 == 0 and n <= 8 for n in pairs) and any(n > 16 for n in pairs) and any(n % 8 == 1 for n in pairs)
    big = [c for c in cs if c.S == 33 * K.DICE_VPB + 5][0]
    assert big.C == 5 and K.ABSENT[0] not in (0, big.N - 1) and big.S % K.DICE_VPB
    assert any(c.N > K.FIN_PAIRS for c in K.BDICE_CASES)
    # the gate values of every case land on distinct voxels in front of the invalid targets
    for c in cs:
        vox = [K.gate_voxel(c.S, c.C, cls, j) for cls in range(c.C) for j in range(3)]
        vox = [v for v in vox if v is not None]
        assert len(set(vox)) == len(vox) >= 1 and (c.S == 1 or (len(vox) == 3 * c.C and max(vox) < c.S - 3))
    assert {len({K.gate_voxel(c.S, c.C, cls, j) // K.DICE_VPB for cls in range(c.C) for j in range(3)}) > 1
            for c in cs if c.S > 2 * K.DICE_VPB} == {True}


@pytest.mark.parametrize('case', K.DICE_CASES[:5], ids=K.case_id)
def test_dice_inputs_have_their_edges(case):
    p, t, w, gout = K.dice_inputs(case)
    N, C, S = case
    thr = K.dice_thr(C)
    assert p.dtype == t.dtype == w.dtype == torch.float32 and float(w[0]) == 0.0 and bool((w[1:] >= 0.2).all())
    for cls in range(C):
        got = [float(p[0, cls, K.gate_voxel(S, C, cls, j)]) for j in range(3) if K.gate_voxel(S, C, cls, j) is not None]
        if S > 1:
            assert got[0] == float(thr) and got[1] > got[0] > got[2] and got[1] - got[2] < 3e-7 * got[0]
            assert float(t[0, K.gate_voxel(S, C, cls, cls % 3)]) == float(cls)
    if S == 1:
        assert float(p[0, 0, 0]) > float(thr) == 1.0 and float(t[0, 0]) == 0.0          # the smallest call: one voxel, above the gate
    else:
        assert [float(v) for v in t[N - 1, S - 3:]] == [0.5, float(C), -1.0]
    loss, sums, d, l = K.dice_ref(p, t, w, gout, torch.float64)
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(loss))
    assert bool((d[p <= thr] == 0.0).all())
    if C == 5:
        n, cls = K.ABSENT
        assert float(sums[n, cls, 0]) == 0.0 and float(sums[n, cls, 1]) == 0.0 and float(l[n, cls]) == 0.0
        assert not bool((t[n] == float(cls)).any()) and bool((d[n, cls] == 0.0).all())


def _focal_blocks(total):
    return min((total + K.FOCAL_VPB - 1) // K.FOCAL_VPB, 8192)


def test_focal_table(lib):
    blocks = {1: 1, 2047: 1, 2048: 1, 2049: 2, 70001: 35, K.BIG: 1025}
    for layout in ('planar', 'matrix'):
        cs = [c for c in K.FOCAL_CASES if c.layout == layout]
        assert {(c.C, c.N * c.S) for c in cs} >= {(C, total) for C in K.FOCAL_C for total in K.FOCAL_TOTALS}
        assert {c.gamma for c in cs} == set(K.GAMMAS) and {c.size_average for c in cs} == {0, 1}
        for C in K.FOCAL_C:
            assert len({c.gamma for c in cs if c.C == C}) == 5 and {c.size_average for c in cs if c.C == C} == {0, 1}
        assert all(c.N == 1 for c in cs) or layout == 'planar'
    for c in K.FOCAL_CASES:
        total = c.N * c.S
        assert lib.seg3d_focal_blocks(total) == blocks[total] == _focal_blocks(total)
        assert (total > K.ITEMS_PER_TRIP) == (total == K.BIG)
    big = [c for c in K.FOCAL_CASES if c.N * c.S == K.BIG]
    assert [(c.layout, c.C, c.gamma) for c in big] == [('planar', 2, 2.0)]
    assert any(c.layout == 'planar' and c.N > 1 and c.S % 2 for c in K.FOCAL_CASES)
    assert 30 <= len(K.FOCAL_CASES) <= 40


@pytest.mark.parametrize('case', [c for c in K.FOCAL_CASES if c.N * c.S < K.BIG], ids=K.case_id)
def test_focal_inputs_have_their_edges(case):
    c = case
    p, t, alpha, gout = K.focal_inputs(c)
    total = c.N * c.S
    assert float(alpha[c.C - 1]) == 0.0 and bool((alpha[:-1] >= 0.1).all())
    tf = t.reshape(-1)
    sel = [float(p[v // c.S, int(tf[v]), v % c.S]) for v in range(min(total, 4))]
    assert sel == [float(torch.tensor(x, dtype=torch.float32)) for x in K.FOCAL_PROBS[:len(sel)]]
    if total > 1:
        assert bool(torch.equal(tf[-5:], torch.tensor([-0.5, 1.7, c.C + 3.0, float(c.C), -1.0])))
    if 0.0 < c.gamma < 1.0:
        assert float(p.max()) < 1.0
    loss, d, sel = K.focal_ref(p, t, alpha, c.gamma, c.size_average, gout, torch.float64)
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(loss)) and bool((d[~sel] == 0.0).all())
    if total > 1:
        # -1, C, C + 3 are outside [0, C): nothing selected; 1.7 selects class 1 and -0.5 class 0
        cols = sel.permute(1, 0, 2).reshape(c.C, total)[:, -5:].long().sum(0).tolist()
        assert cols == [1, 1, 0, 0, 0] and bool(sel.permute(1, 0, 2).reshape(c.C, total)[0, -5]) \
            and bool(sel.permute(1, 0, 2).reshape(c.C, total)[1, -4])
        assert int(sel.sum()) == total - 3


def test_layout_and_copy_tables():
    assert [c.N * c.S > K.ITEMS_PER_TRIP for c in K.LAYOUT_CASES] == [False, False, False, True]
    assert {c.C for c in K.LAYOUT_CASES} >= {1, 16, 33}
    names = ('C', 'src_ld', 'src_off', 'dst_ld', 'dst_off')
    assert all(v % 4 == 0 for v in K.COPY_VEC)
    for i, name in enumerate(names):
        tab = K.COPY_BROKEN[name]
        assert [v % 4 != 0 for v in tab] == [j == i for j in range(5)], name
    for c in K.COPY_CASES:
        assert c.src_off + c.C <= c.src_ld and c.dst_off + c.C <= c.dst_ld and c.C > 0
        if c.in_place:          # the slices of one row do not overlap
            assert c.src_ld == c.dst_ld and (c.src_off + c.C <= c.dst_off or c.dst_off + c.C <= c.src_off)
    small = [c for c in K.COPY_CASES if c.nvox <= 257 and not c.shift]
    assert {c.nvox for c in small} == {1, 255, 257} and len(small) == 18 and sum(K.copy_vec(c) for c in small) == 3
    trips = [c for c in K.COPY_CASES if K.copy_items(c) > K.ITEMS_PER_TRIP]
    assert sorted(K.copy_vec(c) for c in trips) == [False, True] and all(K.copy_items(c) < 2 * K.ITEMS_PER_TRIP for c in trips)
    assert [(c.nvox, c.C, c.in_place) for c in trips] == [(131075, 64, True), (699053, 3, False)]
    shifted = [c for c in K.COPY_CASES if c.shift]
    assert len(shifted) == 1 and shifted[0][1:6] == K.COPY_VEC and shifted[0].shift == 1 and not K.copy_vec(shifted[0])
    for args, why in K.COPY_REFUSALS:
        nvox, C, src_ld, src_off, dst_ld, dst_off = args
        assert C <= 0 or src_off + C > src_ld or dst_off + C > dst_ld, why
