"""Host-only: (1) the constants restated in tests/compound_cases.py equal the library's host queries; (2) every case of its tables has
the property it is named for -- block count, finalize rounds, the lanes' second step, the second 256-stride of the column sum, the
16-byte or the scalar path as compound_vec_ok decides it, a grid against its cap (a second grid-stride trip or not), the top-k
margin -- and every <CT, VEC> instantiation of every dispatched kernel is named by a case, the scalar one once by S % 4 != 0 and
once by a misaligned base; (3) the float64 references agree with the existing oracles (tests/test_compound_loss.py,
tests/test_topk_loss.py, tests/boundary_oracle.py) on integer class ids, and part from them exactly where the header says "its class
is (int)t"; (4) on every case the float32 yardstick stays within 1e-4 of the float64 reference (the self-check of Figures.check)
and the inputs hold the edges they are documented with."""
import ctypes
import os

import pytest
import torch

import compound_cases as K
from boundary_oracle import boundary_oracle
from test_compound_loss import _case, oracle
from test_topk_loss import TIE_CASES, topk_oracle

QUERIES = ('seg3d_dice_blocks', 'seg3d_compound_loss_part_floats', 'seg3d_topk_loss_workspace_bytes',
           'seg3d_boundary_loss_workspace_bytes')
F64, F32 = torch.float64, torch.float32
LOSS_TABLES = {'compound': K.COMPOUND_CASES, 'topk': K.TOPK_CASES, 'boundary': K.BOUNDARY_CASES}
ALL_PAIRS = {(ct, v) for ct in (1, 2, 3, 4, 5, 16) for v in (False, True)}


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


# ---- constants and sizes ---------------------------------------------------------------------------------------------------------------
def test_constants():
    assert (K.DICE_VPB, K.FIN_LANES, K.FIN_ITEMS, K.COLUMN_THREADS, K.MAXC) == (4096, 32, 8, 256, 16)
    assert (K.BWD_MAX_GRID, K.BWD_THREADS, K.TOPK_MAX_GRID, K.CONF_THREADS, K.ITEMS_PER_TRIP) == (8192, 256, 512, 1024, 8192 * 256)
    assert K.TOPK_BITS == (11, 11, 10) and sum(K.TOPK_BITS) == 32 and K.TOPK_HIST_BYTES == 3 * (1 << 11) * 4
    assert K.TRIP_N == 4097 and K.BWD_MAX_GRID // K.TRIP_N == 1 and K.BWD_MAX_GRID // (K.TRIP_N - 1) == 2


def test_sizes_equal_the_library_queries(lib):
    shapes = {(c.N, c.C, c.S) for cases in LOSS_TABLES.values() for c in cases}
    assert len(shapes) >= 25
    for N, C, S in shapes:
        assert lib.seg3d_dice_blocks(S) == K.blocks(S)
        assert lib.seg3d_compound_loss_part_floats(N, C, S) == K.part_floats(N, C, S)
        assert lib.seg3d_topk_loss_workspace_bytes(N, C, S) == K.topk_workspace_bytes(N, C, S)
        assert lib.seg3d_boundary_loss_workspace_bytes(N, C, S) == K.boundary_workspace_bytes(N, C, S)
    assert K.TOPK_CTRL_BYTES % 8 == 0 and (K.TOPK_CTRL_BYTES + K.TOPK_HIST_BYTES) % 8 == 0


# ---- the tables ----------------------------------------------------------------------------------------------------------------------
def _by_shape(cases, N, C, S, shift=0):
    (c,) = [c for c in cases if (c.N, c.C, c.S, c.shift) == (N, C, S, shift)]
    return c


@pytest.mark.parametrize('family', sorted(LOSS_TABLES))
def test_loss_tables_name_every_instantiation_and_trip(family):
    cases = LOSS_TABLES[family]
    assert {(K.ct(c.C), K.vec(c)) for c in cases} == ALL_PAIRS
    for C in (1, 2, 3, 4, 5, 6, 16):
        mine = [c for c in cases if c.C == C]
        assert any(K.vec(c) for c in mine), C
        assert any(c.S % 4 != 0 and c.shift == 0 for c in mine), C                   # the scalar path by the size ...
        assert any(c.S % 4 == 0 and c.shift == 1 for c in mine), C                   # ... and by a base one float past a boundary
    assert {c.S for c in cases} >= {1, K.DICE_VPB - 1, K.DICE_VPB, K.DICE_VPB + 1, K.BLOCKS34, K.BLOCKS34 + 1}
    assert K.BLOCKS34 % 4 == 0 and K.blocks(K.BLOCKS34) == 34 == K.blocks(K.BLOCKS34 + 1)
    items = {K.coef_rows(c) * c.C for c in cases}
    assert items >= {1, 8, 9, 48} and {c.batch_dice for c in cases} == {0, 1}
    # (blocks, entries per item, rounds, the lanes' second step, the column sum's second stride)
    plans = {(1, 1, 1): (1, 1, 1, False, False), (4, 2, 4096): (1, 1, 1, False, False), (3, 3, 4096): (1, 1, 2, False, False),
             (3, 3, 4097): (2, 2, 2, False, False), (2, 4, K.BLOCKS34): (34, 34, 1, True, False),
             (2, 4, K.BLOCKS34 + 1): (34, 68, 1, True, False), (3, 16, 4096): (1, 1, 6, False, False),
             (129, 2, 4100): (2, 258, 1, True, True), (K.TRIP_N, 1, 1028): (1, 1, 513, False, True)}
    for (N, C, S), plan in plans.items():
        assert K.finalize_plan(_by_shape([c for c in cases if c.fill == 'std'], N, C, S)) == plan, (N, C, S)
    assert sum(K.finalize_plan(c)[4] for c in cases if c.N < K.TRIP_N) == 1
    # the backward: the two trip cases take a second grid-stride trip with one workgroup per sample, one on each path; no other does
    trips = [c for c in cases if K.bwd_plan(c)[1]]
    assert [(c.N, c.C, c.S, K.vec(c), K.bwd_plan(c)[0]) for c in trips] == [(4097, 1, 1028, True, 1), (4097, 2, 257, False, 1)]
    assert all(c.N * c.S < 4.3e6 and c.C <= 2 for c in trips)
    # without the trip cases and the histogram trips nothing is large
    assert all(c.N * c.C * c.S <= 1.1e6 for c in cases if c not in trips and c not in K.TOPK_HIST_TRIPS)
    assert sum(c.fill == 'empty' for c in cases) == 1 and any(not (0 <= c.ignore < c.C) for c in cases)
    assert sum(0 <= c.ignore < c.C for c in cases) >= 5


def test_option_rotations_reach_every_value():
    cs = K.COMPOUND_CASES
    assert {c.gamma for c in cs} == set(K.GAMMAS) and {(c.dice_weight, c.ce_weight) for c in cs} == set(K.TERM_WEIGHTS)
    for v in (False, True):
        assert {c.gamma for c in cs if K.vec(c) == v} == set(K.GAMMAS)
    ts = K.TOPK_CASES
    assert {c.k_percent for c in ts} == set(K.K_PERCENTS) and {(c.dice_weight, c.ce_weight) for c in ts} == set(K.TOPK_TERM_WEIGHTS)
    bs = K.BOUNDARY_CASES
    assert {c.include_background for c in bs} == {0, 1} and {c.dice_weight for c in bs} == {0.0, 1.0}
    assert all(c.C >= 2 for c in bs if not c.include_background)
    assert {K.vec(c) for c in bs if not c.include_background} == {False, True}
    # the cases that separate the two backward paths: a counted non-integer target, the distribution term on, C <= 5, 16-byte path
    assert {c.C for c in cs if K.vec(c) and c.C <= 5 and c.ce_weight > 0 and c.fill == 'std' and c.N * c.S >= 32} == {1, 2, 3, 4, 5}
    assert {c.C for c in ts if K.vec(c) and c.C <= 5 and c.ce_weight > 0 and c.k_percent == 100.0} >= {2}


def test_topk_histogram_trips():
    aligned, shifted = K.TOPK_HIST_TRIPS
    assert K.topk_hist_plan(aligned) == (K.TOPK_MAX_GRID, True, True) and K.topk_hist_plan(shifted) == (K.TOPK_MAX_GRID, False, True)
    assert aligned.N > 1 and all(c.N * c.S < 2 * K.TOPK_MAX_GRID * 256 * (4 if c.shift == 0 else 1) for c in K.TOPK_HIST_TRIPS)
    # beside them only the three largest shapes of the shared table stride, all with 16-byte loads
    others = [c for c in K.TOPK_CASES if c not in K.TOPK_HIST_TRIPS and K.topk_hist_plan(c)[2]]
    assert [(c.N, c.S, K.topk_hist_plan(c)[1]) for c in others] == [(129, 4100, True), (K.TRIP_N, 1028, True), (K.TRIP_N, 257, True)]
    # tests/test_gpu_topk_loss.py, the 2 x 33 x 32 x 32 cases: 66 workgroups against a cap of 512 -- they never stride
    assert K.topk_hist_plan(K.TopK(2, 2, 33 * 32 * 32, 0, 0, K.NO_IGNORE, 'std', 10.0, 1.0, 1.0)) == (66, True, False)
    assert K.topk_hist_plan(K.TIE_CASE)[2] is False and K.vec(K.TIE_CASE)


def test_confusion_table():
    cs = K.CONFUSION_CASES
    assert {(K.ct(c.C), K.vec(c)) for c in cs} == ALL_PAIRS
    for C in (1, 2, 3, 4, 5, 6, 16):
        mine = [c for c in cs if c.C == C]
        assert any(K.vec(c) for c in mine) and any(c.S % 4 and not c.shift for c in mine) and any(c.S % 4 == 0 and c.shift == 1 for c in mine)
    trips = [c for c in cs if K.confusion_plan(c)[1]]
    assert [(K.vec(c), K.confusion_plan(c)[0]) for c in trips] == [(True, 256), (False, 256)] and all(c.C == 2 for c in trips)
    assert any(c.S > K.CONF_THREADS * 4 and K.vec(c) and not K.confusion_plan(c)[1] for c in cs)      # several workgroups, one trip
    assert any(0 <= c.ignore < c.C for c in cs) and any(c.ignore >= c.C for c in cs) and any(c.S == 1 for c in cs)


def test_head_table():
    for kind in ('softmax', 'sigmoid'):
        cs = [c for c in K.HEAD_CASES if c.kind == kind]
        assert {c.C for c in cs} == set(K.HEAD_C) and any(c.S == 1 for c in cs)
        trips = [c for c in cs if K.head_trip(c)]
        assert len(trips) == 1 and trips[0].N == 2 and trips[0].C == 2 and trips[0].N * trips[0].S < K.ITEMS_PER_TRIP + 256
        # voxel ITEMS_PER_TRIP, the first of the second trip, lies in sample 1
        assert K.ITEMS_PER_TRIP // trips[0].S == 1
    assert sorted(K.REFUSALS) == sorted(
        'seg3d_' + n for n in ('softmax_fwd', 'softmax_bwd', 'sigmoid_fwd', 'sigmoid_bwd', 'compound_loss_fwd', 'compound_loss_bwd',
                               'topk_loss_fwd', 'topk_loss_bwd', 'boundary_loss_fwd', 'boundary_loss_bwd', 'confusion_counts'))


# ---- the references against the existing oracles, on integer class ids -----------------------------------------------------------------
WEIGHTS = [0.2, 1.0, 3.0]


def _integer_inputs(seed, ignore, include_background):
    p, t = _case(seed, (2, 5, 6, 7), 3, ignore_frac=0.2 if ignore is not None else 0.0)
    p = p.float()
    w = torch.tensor(WEIGHTS)
    wdice = w.clone()
    if not include_background:
        wdice[0] = 0.0
    return p, t, (wdice / wdice.sum()).float(), w.float()


def _autograd(fn, p):
    q = p.double().clone().requires_grad_(True)
    out = fn(q)
    (g,) = torch.autograd.grad(out[0] if isinstance(out, tuple) else out['total'], q)
    return out, g.reshape(p.shape[0], p.shape[1], -1)


@pytest.mark.parametrize('batch_dice', [0, 1])
@pytest.mark.parametrize('ignore', [None, 255])
@pytest.mark.parametrize('gamma', [0.0, 2.0, 1.5])
def test_compound_reference_agrees_with_the_oracle(gamma, ignore, batch_dice):
    include_background = batch_dice == 0
    p, t, wdice, alpha = _integer_inputs(21, ignore, include_background)
    c = K.Compound(2, 3, 210, 0, batch_dice, K.NO_IGNORE if ignore is None else float(ignore), 'std', gamma, 0.5, 2.0)
    ref = K.compound_ref(p.reshape(2, 3, -1), t.reshape(2, -1).float(), wdice, alpha, c, 1.0, F64)
    out, g = _autograd(lambda q: oracle(q, t, weights=WEIGHTS, dice_weight=0.5, ce_weight=2.0, gamma=gamma,
                                        include_background=include_background, batch_dice=bool(batch_dice), ignore_label=ignore), p)
    # (wdice and alpha reach the reference as float32, the oracle normalises in float64: 1e-7, not 1e-12)
    assert float((ref['loss'] - torch.stack([o.detach() for o in out])).abs().max()) < 2e-7
    assert float((ref['dprobs'] - g).abs().max()) < 2e-7 * float(g.abs().max())


@pytest.mark.parametrize('k_percent', [0.01, 10.0, 100.0])
@pytest.mark.parametrize('ignore', [None, 255])
def test_topk_reference_agrees_with_the_oracle(ignore, k_percent):
    p, t, wdice, alpha = _integer_inputs(22, ignore, True)
    c = K.TopK(2, 3, 210, 0, 0, K.NO_IGNORE if ignore is None else float(ignore), 'std', k_percent, 1.0, 1.0)
    ref = K.topk_ref(p.reshape(2, 3, -1), t.reshape(2, -1).float(), wdice, alpha, c, 1.0, F64)
    out, g = _autograd(lambda q: topk_oracle(q, t, weights=WEIGHTS, k_percent=k_percent, ignore_label=ignore), p)
    assert ref['selection'] == out['selection'] and abs(float(ref['tau']) - out['tau']) < 1e-6 * max(1.0, out['tau'])
    got = torch.stack([out['total'].detach(), out['region'].detach(), out['topk'].detach()])
    assert float((ref['loss'] - got).abs().max()) < 2e-7 * float(got.abs().max())
    assert float((ref['dprobs'] - g).abs().max()) < 2e-7 * float(g.abs().max())
    assert bool(torch.equal(ref['valid'], out['valid'])) and float((ref['ell'][ref['valid']] - out['ell'][out['valid']]).abs().max()) < 1e-6


def test_topk_reference_on_the_tie_fixture():
    p, t, wdice, alpha, gout = K.loss_inputs(K.TIE_CASE)
    for k_percent, sel in TIE_CASES.items():
        ref = K.topk_ref(p, t, wdice, alpha, K.TIE_CASE._replace(k_percent=k_percent), gout, F64)
        assert ref['selection'] == sel
    ref = K.topk_ref(p, t, wdice, alpha, K.TIE_CASE._replace(dice_weight=0.0), gout, F64)
    g1, p1 = ref['dprobs'][0, 1], p[0, 1].double()
    n, k, m, n_eq, r = ref['selection']
    assert bool(torch.allclose(g1[p1 == 0.125], torch.full((30,), -1.0 / (k * 0.125), dtype=F64), rtol=1e-12))
    assert bool(torch.allclose(g1[p1 == 0.25], torch.full((50,), -(r / n_eq) / (k * 0.25), dtype=F64), rtol=1e-12))
    assert float(g1[p1 == 0.5].abs().max()) == 0.0 and float(ref['dprobs'][0, 0].abs().max()) == 0.0
    assert abs(float(ref['loss'][2]) - 1.9061547465398494) < 1e-7


@pytest.mark.parametrize('include_background', [0, 1])
@pytest.mark.parametrize('ignore', [None, 255])
def test_boundary_reference_agrees_with_the_oracle(ignore, include_background):
    p, t, wdice, _ = _integer_inputs(23, ignore, bool(include_background))
    c = K.Boundary(2, 3, 210, 0, 0, K.NO_IGNORE if ignore is None else float(ignore), 'std', include_background, 1.0)
    tt = t.reshape(2, -1).float()
    phi = K.phi_input(c, tt)
    ref = K.boundary_ref(p.reshape(2, 3, -1), tt, phi, wdice, c, 1.0, F64)
    out, g = _autograd(lambda q: boundary_oracle(q, t, phi.reshape((2, -1) + tuple(t.shape[2:])).numpy(), weights=WEIGHTS,
                                                 boundary_weight=K.BOUNDARY_WEIGHT, include_background=bool(include_background),
                                                 ignore_label=ignore), p)
    assert float((ref['loss'] - torch.stack([o.detach() for o in out])).abs().max()) < 2e-7
    assert float((ref['dprobs'] - g).abs().max()) < 2e-7 * float(g.abs().max())


def test_references_take_the_class_of_a_non_integer_target_by_truncation():
    """the header: "a voxel counts iff 0 <= t < C and t != ignore_label", "its class is (int)t"."""
    p = torch.tensor([[[0.2, 0.3, 0.6, 0.5, 0.1], [0.8, 0.7, 0.4, 0.5, 0.9]]])
    t = torch.tensor([[1.7, 0.5, -0.5, -0.0, 2.0]])
    valid, cls = K.counting(t, 2, K.NO_IGNORE)
    assert valid.tolist() == [[True, True, False, True, False]] and cls.tolist() == [[1, 0, 0, 0, 0]]
    c = K.Compound(1, 2, 5, 0, 0, K.NO_IGNORE, 'std', 0.0, 0.0, 1.0)
    ref = K.compound_ref(p, t, torch.tensor([0.5, 0.5]), torch.ones(2), c, 1.0, F64)
    want = -(torch.log(torch.tensor([0.8, 0.3, 0.5]).double())).mean()
    assert abs(float(ref['loss'][2]) - float(want)) < 1e-7
    d = ref['dprobs'][0]
    assert float(d[1, 0]) == pytest.approx(-1.0 / (3 * 0.8), rel=1e-6) and float(d[0, 1]) == pytest.approx(-1.0 / (3 * 0.3), rel=1e-6)
    assert float(d[0, 0]) == 0.0 and bool((d[:, 2] == 0.0).all()) and bool((d[:, 4] == 0.0).all())
    assert valid.tolist() == K.counting(t, 2, 1.0)[0].tolist()              # 1.7 != 1.0: still counted under ignore_label = 1


def test_confusion_reference_takes_the_first_maximum():
    p = torch.tensor([[[0.5, 0.2, 0.25, 0.1], [0.5, 0.7, 0.25, 0.1], [0.0, 0.1, 0.25, 0.8]]])
    t = torch.tensor([[1.0, 1.7, 2.0, 3.0]])
    assert K.confusion_ref(p, t, K.NO_IGNORE).tolist() == [[0, 2, 0], [1, 0, 1], [0, 0, 1]]
    assert K.confusion_ref(p, t, 2.0).tolist() == [[0, 1, 0], [1, 0, 1], [0, 0, 0]]


# ---- every case: its inputs hold their edges, the yardstick is the reference's operation -----------------------------------------------
def _rel(y, r):
    """the largest error per element relative to |ref| (K.per_element: to K.TINY below it); exactly 0 where the reference is"""
    assert bool((y[r == 0] == 0).all())
    return float(K.per_element(y, r).max())


def _scaled(y, r):
    return float((y.double() - r).abs().max()) / max(float(r.abs().max()), 1e-300)


def _check_loss_case(c, ref, yard, p, t):
    N, C, S, total = c.N, c.C, c.S, c.N * c.S
    assert p.dtype == t.dtype == F32 and p.shape == (N, C, S) and t.shape == (N, S)
    assert bool(torch.isfinite(ref['dprobs']).all()) and bool(torch.isfinite(ref['loss']).all()) and bool(torch.isfinite(ref['coef']).all())
    assert _scaled(yard['loss'], ref['loss']) <= 1e-4 and _scaled(yard['coef'], ref['coef']) <= 1e-4
    assert _rel(yard['dprobs'], ref['dprobs']) <= 1e-4
    valid, cls = ref['valid'], ref['cls']
    assert bool((ref['dprobs'][~valid.unsqueeze(1).expand(N, C, S)] == 0.0).all())
    tf, vf, cf = t.reshape(-1), valid.reshape(-1), cls.reshape(-1)
    if c.fill == 'empty':
        assert int(valid.sum()) == 0 and float(ref['loss'].abs().max()) == 0.0 and float(ref['dprobs'].abs().max()) == 0.0
        return
    if c.fill == 'tie':
        return
    if total >= 32:
        vals = K.target_values(C)
        assert [float(v) for v in tf[total - len(vals):].flip(0)] == [float(torch.tensor(v, dtype=F32)) for v in vals]
        assert torch.signbit(tf[total - len(vals)]) and float(tf[total - len(vals)]) == 0.0            # -0.0
        got = [(bool(vf[total - 1 - i]), int(cf[total - 1 - i])) for i in range(len(vals))]
        want = [(False, 0)] * 4 + [(0.5 < C, 0), (1.7 < C, 1 if 1.7 < C else 0), (True, C - 1), (True, 0), (False, 0), (c.ignore != 0.0, 0)]
        assert got == want
        sc = K.safe_class(c)
        sel = [float(p[0, sc, v]) for v in range(5)]
        assert sel[:3] == [0.0, float(torch.tensor(1e-30, dtype=F32)), float(K.PMIN)] and sel[4] == 0.5
        assert sel[3] == (1.0 if not 0.0 < getattr(c, 'gamma', 0.0) < 1.0 else float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))))
        assert bool(vf[:5].all())
    if 0.0 < getattr(c, 'gamma', 0.0) < 1.0:
        assert float(p.max()) < 1.0
    if N > 1 and C > 1:
        assert not bool(((cls[0] == 1) & valid[0]).any()) and bool(valid[0].any())
    if N > 2:
        assert not bool(valid[1].any())
    if not 0 <= c.ignore < C and c.ignore >= 0 and total >= 32:
        assert int((t == c.ignore).sum()) >= total // 30
    assert int(valid.sum()) > 0


@pytest.mark.parametrize('case', K.COMPOUND_CASES, ids=K.case_id)
def test_compound_case(case):
    p, t, wdice, alpha, gout = K.loss_inputs(case)
    ref, yard = [K.compound_ref(p, t, wdice, alpha, case, gout, dt) for dt in (F64, F32)]
    _check_loss_case(case, ref, yard, p, t)
    assert ref['coef'].numel() == 2 * K.coef_rows(case) * case.C + 1
    if case.C > 2:
        assert float(alpha[case.C - 1]) == 0.0
    assert abs(float(alpha.sum()) - 1.0) > 1e-3 and gout != 1.0
    if case.ce_weight == 0.0:
        assert float(ref['coef'][-1]) == 0.0
    if case.dice_weight == 0.0:
        assert float(ref['coef'][:-1].abs().max()) == 0.0 and bool((ref['dprobs'][ref['onehot'] == 0] == 0.0).all())


@pytest.mark.parametrize('case', K.TOPK_CASES + [K.TIE_CASE], ids=K.case_id)
def test_topk_case(case):
    p, t, wdice, alpha, gout = K.loss_inputs(case)
    ref, yard = [K.topk_ref(p, t, wdice, alpha, case, gout, dt) for dt in (F64, F32)]
    _check_loss_case(case, ref, yard, p, t)
    assert ref['coef'].numel() == 2 * K.coef_rows(case) * case.C + 3
    # the rule on the inputs: the float64 ell next to tau on either side are at least MARGIN away (relative) or equal to it
    assert all(m == 0.0 or m >= K.MARGIN for m in ref['margin']), ref['margin']
    assert yard['selection'] == ref['selection']
    n, k, m, n_eq, r = ref['selection']
    assert n == int(ref['valid'].sum()) and k == K.device_count(n, case.k_percent) and (n == 0 or 1 <= r <= n_eq)
    assert _rel(yard['ell'], ref['ell']) <= 1e-4 and bool((ref['ell'][~ref['valid']] == -1.0).all()) and bool((ref['ell'][ref['valid']] >= 0.0).all())
    assert K.quantised(case) == (case.N * case.S > 20000)


@pytest.mark.parametrize('case', K.BOUNDARY_CASES, ids=K.case_id)
def test_boundary_case(case):
    p, t, wdice, alpha, gout = K.loss_inputs(case)
    phi = K.phi_input(case, t)
    ref, yard = [K.boundary_ref(p, t, phi, wdice, case, gout, dt) for dt in (F64, F32)]
    _check_loss_case(case, ref, yard, p, t)
    c0 = 0 if case.include_background else 1
    assert phi.shape == (case.N, case.C - c0, case.S) and ref['coef'].numel() == 2 * K.coef_rows(case) * case.C + case.C
    if not case.include_background:
        assert float(wdice[0]) == 0.0
    if case.dice_weight == 0.0:
        assert float(ref['coef'][:2 * K.coef_rows(case) * case.C].abs().max()) == 0.0


@pytest.mark.parametrize('case', K.HEAD_CASES, ids=K.case_id)
def test_head_case(case):
    x, d = K.head_inputs(case)
    p, py = [K.head_fwd_ref(case.kind, x, dt) for dt in (F64, F32)]
    assert p.shape == (case.N, case.C, case.S) and _scaled(py, p) <= 1e-4 and float(p.min()) >= 0.0 and float(p.max()) <= 1.0
    if case.kind == 'softmax':
        want = torch.softmax(x.double(), 2).permute(0, 2, 1)
        assert float((p - want).abs().max()) < 1e-15 and float((p.sum(1) - 1.0).abs().max()) < 1e-12
    else:
        assert float((p - torch.sigmoid(x.double()).permute(0, 2, 1)).abs().max()) < 1e-15
    if case.N * case.S >= 100:
        flat = p.permute(0, 2, 1).reshape(-1, case.C)
        assert bool((flat[12] == (1.0 / case.C if case.kind == 'softmax' else 0.5)).all())                  # x = 0
        assert float(flat[6, case.C // 2]) == 1.0 and (case.C == 1 or float(flat[10, 0]) == 0.0)              # +-1e4
        assert len(set(flat[4].tolist())) == 1
    p32 = p.float()
    for dd in (d, K.sparse_dprobs(p32, d)):
        g, gy = [K.head_bwd_ref(case.kind, p32, dd, dt) for dt in (F64, F32)]
        assert g.shape == (case.N, case.S, case.C) and _scaled(gy, g) <= 1e-4
    assert _rel(gy, g) <= 1e-4                   # the sparse gradient: per element


@pytest.mark.parametrize('case', K.CONFUSION_CASES, ids=K.case_id)
def test_confusion_case(case):
    p, t, counts0 = K.confusion_inputs(case)
    ref = K.confusion_ref(p, t, case.ignore)
    valid, _ = K.counting(t, case.C, case.ignore)
    assert int(ref[:, 0].sum() + ref[:, 1].sum()) == int(valid.sum()) == int(ref[:, 0].sum() + ref[:, 2].sum())
    assert bool((counts0 > 0).all()) and counts0.numel() == 3 * case.C
    if case.C > 1 and case.N * case.S >= 32:
        top = p.max(1).values
        assert int(((p == top.unsqueeze(1)).sum(1) > 1).sum()) >= case.N * case.S // 5
