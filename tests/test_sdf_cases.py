"""Host-only: (1) every case of tests/sdf_cases.py reaches what it is named for -- the sdf_x_kernel<J> instantiation, the tile counts,
full and partial tiles, the LDS bytes and the grids of pass y and pass z -- and over the table J = 1, 2, 3, 4 occur at both edges of
each, a 256-voxel line occurs in pass z and grid y comes next to its limit; the workspace size equals the library's query; (2) sdf_ref
in float64 agrees with the brute force of tests/boundary_oracle.py to rounding, fractional targets included; (3) on every case with
non-unit spacing the float32 yardstick stays at or below a quarter of the cap, and with unit spacing the squared distances are
integers below 2^24; (4) the targets hold the edges they are documented with.  Prints one line per case (run with -s)."""
import ctypes
import os

import numpy as np
import pytest

import sdf_cases as K
from boundary_oracle import signed_distance_oracle

F64, F32 = np.float64, np.float32


def _case_seed(c, pattern):
    return 1000 + 7 * K.PATTERNS.index(pattern) + K.CASES.index(c)


def test_table_reaches_every_instantiation_and_tile():
    by_x = {}
    for c in K.CASES:
        p = K.plan(c)
        X, Y, Z = c.xyz
        ids, nlab = K.CLASS_LISTS[c.classes]
        assert 1 <= min(c.xyz) and max(c.xyz) <= K.MAX_AXIS and 1 <= len(ids) <= K.MAXK and c.N * len(ids) <= K.MAX_NK
        assert all(K.MIN_SPACING <= s <= K.MAX_SPACING for s in c.spacing) and c.N * X * Y * Z < 2 ** 31
        assert max(p['lds_y'], p['lds_z']) <= 64 * 1024 and max(p['grid_y'][1], p['grid_z'][1]) <= 65535
        by_x.setdefault(p['J'], set()).add(X)
        print('sdf {:28s} J {}  grid x {}  pass y: {} tiles{} x {} lines of {}, LDS {} B, grid {}  pass z: {} tiles{} of {}, LDS {} B, '
              'grid {}'.format(c.name, p['J'], p['grid_x'], p['tiles_y'], ' (last partial)' if p['partial_y'] else '', Z, Y, p['lds_y'],
                               p['grid_y'], p['tiles_z'], ' (last partial)' if p['partial_z'] else '', Z, p['lds_z'], p['grid_z']))
    assert {J: sorted(v & {64, 128, 129, 192, 193, 2, 33, 31, 5, 9}) for J, v in by_x.items()} == {
        1: [2, 5, 9, 31, 33, 64], 2: [128], 3: [129, 192], 4: [193]}
    assert {c.xyz for c in K.CASES} >= set(K.SHAPES) and len(K.SHAPES) == 9
    plans = {c.xyz: K.plan(c) for c in K.CASES}
    assert plans[(2, 1, 256)]['lds_z'] == 64 * 1024                                        # the longest line in pass z
    # one and two tiles, full and partial, in pass y (tiles over X) and in pass z (tiles over X Y)
    assert {(p['tiles_y'], p['partial_y']) for p in plans.values()} >= {(1, True), (2, False), (2, True)}
    assert {(p['tiles_z'], p['partial_z']) for p in plans.values()} >= {(1, True), (2, False), (2, True)}
    assert not plans[(5, 7, 3)]['line4_y'] and not plans[(5, 7, 3)]['line4_z'] and plans[(2, 1, 256)]['line4_z']
    for sp in (K.UNIT, K.ANISO):
        assert {c.xyz for c in K.CASES if c.spacing == sp} >= set(K.SHAPES)
    for s in ((9, 7, 5), (193, 2, 1)):
        assert {c.spacing for c in K.CASES if c.xyz == s} >= set(K.EXTREME)
    assert {c.classes for c in K.CASES} == set(K.CLASS_LISTS)
    ids, nlab = K.CLASS_LISTS['k3']
    assert max(ids) >= nlab and list(ids) != sorted(ids) and len(K.CLASS_LISTS['k1'][0]) == 1 and len(K.CLASS_LISTS['k16'][0]) == 16
    big = [c for c in K.CASES if c.N * len(K.CLASS_LISTS[c.classes][0]) == 65520]
    assert big and all(c.N == 4095 and c.xyz == (2, 1, 1) and K.plan(c)['grid_y'] == (1, 65520) == K.plan(c)['grid_z'] for c in big)
    assert any(c.N == 3 for c in K.CASES)
    assert {p for c in K.CASES for p in c.patterns} == set(K.PATTERNS)


def test_workspace_bytes_equal_the_library_query():
    import __graft_entry__  # noqa: F401  (repo root is on sys.path)
    from segmentation3d import _engine
    if not os.path.isfile(_engine.LIB_PATH):
        __graft_entry__.build()
    handle = ctypes.CDLL(_engine.LIB_PATH)
    fn = handle.seg3d_signed_distance_workspace_bytes
    fn.restype, fn.argtypes = _engine._SIGNATURES['seg3d_signed_distance_workspace_bytes']
    for c in K.CASES:
        k = len(K.CLASS_LISTS[c.classes][0])
        assert fn(c.N, k, *c.xyz) == K.workspace_bytes(c.N, k, *c.xyz)
    assert fn(0, 1, 1, 1, 1) == 0 and fn(1, 1, 256, 256, 256) == 8 * 256 ** 3


def test_targets_hold_their_edges():
    c = [c for c in K.CASES if c.name.startswith('5x7x3_unit')][0]
    ids, nlab = K.CLASS_LISTS[c.classes]
    t, ignore = K.labels('fractional', c, 1)
    vals = set(t.ravel().tolist())
    assert {0.5, float(F32(1.7)), nlab - 0.25, -0.5} <= vals and ignore == K.NO_IGNORE
    assert bool(np.signbit(t[t == 0]).any()) and not bool(np.signbit(t[t == 0]).all())           # -0.0 beside 0.0
    t, ignore = K.labels('fractional_ignore', c, 1)
    assert ignore != int(ignore) and (t == ignore).any() and (np.trunc(t[t != ignore]) == int(ignore)).any()
    c3 = [c for c in K.CASES if c.N == 3][0]
    for p in c3.patterns:
        t, ignore = K.labels(p, c3, 2)
        ids, nlab = K.CLASS_LISTS[c3.classes]
        ref = K.sdf_ref(t, ids, c3.spacing, nlab, ignore, F64)
        assert not ref[1].any() and ref[0].any() and ref[2].any()


def test_reference_equals_the_oracle():
    """integer, out-of-range and fractional targets, with and without an ignore label; the oracle's own rule is trunc(t)"""
    for c in K.CASES:
        if c.N > 3 or max(c.xyz) > 64:
            continue
        ids, nlab = K.CLASS_LISTS[c.classes]
        for p in c.patterns:
            t, ignore = K.labels(p, c, _case_seed(c, p))
            mine, d2 = K.sdf_ref(t, ids, c.spacing, nlab, ignore, F64, squared=True)
            want, w2 = signed_distance_oracle(t, ids, c.spacing, num_class=nlab, ignore_label=None if ignore == K.NO_IGNORE else ignore,
                                              squared=True)
            assert np.array_equal(np.sign(mine), np.sign(want)), (c.name, p)
            assert K.rel_err(mine, want) <= 4 * np.finfo(F64).eps and K.rel_err(d2, w2) <= 4 * np.finfo(F64).eps, (c.name, p)


@pytest.mark.parametrize('case', K.CASES, ids=K.case_id)
def test_yardstick(case):
    c = case
    ids, nlab = K.CLASS_LISTS[c.classes]
    worst = 0.0
    for p in c.patterns:
        t, ignore = K.labels(p, c, _case_seed(c, p))
        (ref, d2), yard = K.sdf_ref(t, ids, c.spacing, nlab, ignore, F64, squared=True), K.sdf_ref(t, ids, c.spacing, nlab, ignore, F32)
        assert yard.dtype == F32 and np.array_equal(np.sign(yard), np.sign(ref)), p
        if p in ('random', 'fractional', 'single_voxel'):
            assert ref.any(), p
        if c.spacing == K.UNIT:
            assert np.array_equal(d2, np.rint(d2)) and d2.max() < 2 ** 24
            assert np.array_equal(yard, np.sign(ref).astype(F32) * np.sqrt(d2).astype(F32))      # one correctly rounded root
        else:
            ye = K.rel_err(yard, ref)
            worst = max(worst, ye)
            assert ye <= 0.25 * K.CAP, (p, ye)
    print('sdf {:28s} yardstick {:.3e}  bar {:.3e}'.format(c.name, worst, K.bar(worst)))
