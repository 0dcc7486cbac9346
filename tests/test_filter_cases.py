"""Host-only: (1) every case of tests/filter_cases.py reaches what it is named for -- the blur launch <MC, VEC>, its radius set, the
staged halo, the tile counts and the LDS bytes; the low-resolution instantiation <KC, VEC>, the patch extents of every tile against
the LDS patch of 35 x 11 x 11 -- and over the tables every radius 0..6 occurs in each of the three blur launches, every
instantiation lowres_launch can pick occurs, and the extents 35 / 11 / 11 occur; (2) the references agree with oracle_blur /
oracle_lowres of tests/test_resolution_augment.py on Gaussian taps and zoom-derived sizes to float64 rounding; (3) on every case the
float32 yardstick stays at or below a quarter of the cap, so that no bar saturates at its cap; (4) swapped free taps and a low grid off
by one move the reference by more than the bar: the cases can see such errors.  Prints one line per case (run with -s)."""
import numpy as np
import pytest

import filter_cases as K
from test_resolution_augment import oracle_blur, oracle_lowres, oracle_lowres_sizes, oracle_taps

F64, F32 = np.float64, np.float32


# ---- blur ----------------------------------------------------------------------------------------------------------------------------
def test_blur_table_reaches_every_radius_in_every_launch():
    seen = set()
    for c in K.BLUR_CASES:
        assert len(c.radii) == len(c.kinds) == c.M and 1 <= c.M <= K.MAX_M and all(0 <= r <= K.MAX_RADIUS for r in c.radii)
        assert c.zyx[0] <= 17 and c.zyx[1] <= 17 and c.zyx[2] <= 65
        for tag, shift in K.launches(c):
            launch, gy, R, lds = K.blur_launch(c, shift)
            assert launch != 'copy' and R == max(c.radii) and lds <= 64 * 1024
            assert launch == ((c.M, True) if c.M in (2, 4) and shift == 0 else (1, False)) and gy * launch[0] == c.M
            seen |= {(r, launch) for r in c.radii}
            print('blur {:24s} {}launch <{}, {}> grid ({} x {} x {} tiles, {})  radii {}  halo {}  LDS {} B'.format(
                c.name, tag, launch[0], str(launch[1]).lower(), *K.tiles(c.zyx), gy, c.radii, R, lds))
    assert seen == {(r, l) for r in range(7) for l in K.BLUR_LAUNCHES}
    # the scalar launch at every M the issue names: 1, 3, 5, 8 by the width, 4 and 2 by the shifted base
    assert {c.M for c in K.BLUR_CASES} == {1, 2, 3, 4, 5, 8}
    vec = [c for c in K.BLUR_CASES if c.M in (2, 4)]
    for M in (2, 4):
        mixed = [set(c.radii) for c in vec if c.M == M]
        assert any({0, 6} <= s for s in mixed) and any({1, 5} <= s for s in mixed), M     # the halo is 6 / 5, a channel filters with 0 / 1
    assert any({0, 6, 1, 5} <= set(c.radii) for c in vec if c.M == 4)


def test_blur_table_geometry():
    shapes = {c.zyx for c in K.BLUR_CASES}
    assert (8, 8, 32) in shapes and (9, 9, 33) in shapes
    assert any(1 in s for s in shapes)
    assert any(c.zyx[0] == 17 and K.tiles(c.zyx)[2] == 3 for c in K.BLUR_CASES) and any(c.zyx[2] == 65 for c in K.BLUR_CASES)
    assert any(min(c.zyx) == 2 and max(c.radii) == 6 and max(c.zyx) < 6 for c in K.BLUR_CASES)          # several reflections
    # an axis below the radius folds more than once: 2 voxels under R = 6 visit -6..7
    assert K.reflect(np.arange(-6, 8), 2).tolist() == [1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0]
    for launch in K.BLUR_LAUNCHES:          # every launch sees an exact tile, a partial one and three tiles along z
        mine = [c for c in K.BLUR_CASES for _, s in K.launches(c) if K.blur_launch(c, s)[0] == launch]
        assert any(c.zyx == (8, 8, 32) for c in mine) and any(c.zyx == (9, 9, 33) for c in mine), launch
        assert any(K.tiles(c.zyx)[2] == 3 and K.tiles(c.zyx)[0] == 3 for c in mine), launch


def test_taps():
    for R in range(1, 7):
        g = K.gaussian_taps(R)
        sigma = R / 3.0
        assert int(np.ceil(3.0 * sigma)) == R
        assert np.array_equal(g[:R + 1].astype(F64), oracle_taps(sigma)[1][R:]) and not g[R + 1:].any()
        assert np.all(np.diff(g[:R + 1]) < 0)
        for m in range(8):
            f = K.free_taps(R, m).astype(F64)
            assert abs(f[0] + 2.0 * f[1:].sum() - 1.0) <= 4e-7 and f.min() >= 0.0 and f.max() <= 1.0 and not f[R + 1:].any()
            assert len(set(f[:R + 1].tolist())) == R + 1                                  # distinct
            d = np.diff(f[:R + 1])
            assert R < 2 or (d.min() < 0 < d.max())                                       # not monotone
            assert R < 2 or f[2] == 0.0                                                   # an exact 0 inside the radius
    for c in K.BLUR_CASES:
        t = K.blur_taps(c)
        assert t.shape == (c.M, 7) and t.dtype == F32
    assert any(k == 'f' and r >= 2 for c in K.BLUR_CASES for r, k in zip(c.radii, c.kinds))
    assert {(r, k) for c in K.BLUR_CASES for r, k in zip(c.radii, c.kinds) if r} >= {(r, k) for r in range(1, 7) for k in 'gf'}


@pytest.mark.parametrize('zyx', [(5, 7, 9), (2, 3, 5), (17, 9, 33)], ids=str)
def test_blur_reference_equals_the_oracle_on_gaussian_taps(zyx):
    x = np.random.RandomState(3).randn(*zyx, 6)
    radii = (1, 2, 3, 4, 5, 6)
    taps = np.stack([K.gaussian_taps(R) for R in radii])
    got = K.blur_ref(x, radii, taps, F64)
    for m, R in enumerate(radii):
        want = oracle_blur(x[..., m], R / 3.0)
        assert np.abs(got[..., m] - want).max() <= 8 * np.finfo(F64).eps * np.abs(x).max(), R
    assert np.array_equal(K.blur_ref(x, (0,) * 6, taps, F64), x)


@pytest.mark.parametrize('case', K.BLUR_CASES, ids=K.case_id)
def test_blur_yardstick_and_disagreement(case):
    c = case
    x, taps = K.crop(c), K.blur_taps(c)
    scale = float(np.abs(x).max())
    ref, yard = K.blur_ref(x, c.radii, taps, F64), K.blur_ref(x, c.radii, taps, F32)
    assert yard.dtype == F32 and ref.dtype == F64
    ye = float(np.abs(yard.astype(F64) - ref).max())
    print('blur {:24s} yardstick {:.3e} = {:.3e} x max|x|, bar {:.3e} x max|x|'.format(c.name, ye, ye / scale, K.bar(ye, scale) / scale))
    assert ye <= 0.25 * K.CAP * scale
    for m, R in enumerate(c.radii):
        if R == 0:
            assert np.array_equal(ref[..., m], x[..., m].astype(F64)) and np.array_equal(yard[..., m].view(np.int32), x[..., m].view(np.int32))
    if any(k == 'f' and r >= 2 for r, k in zip(c.radii, c.kinds)):
        moved = K.blur_ref(x, c.radii, K.swapped_taps(taps, [r if k == 'f' else 0 for r, k in zip(c.radii, c.kinds)]), F64)
        for m, (r, k) in enumerate(zip(c.radii, c.kinds)):
            d = float(np.abs(moved[..., m] - ref[..., m]).max())
            assert (d > 100 * K.bar(ye, scale)) == (k == 'f' and r >= 2), (m, d)
    if len(set(c.radii)) > 1:               # a channel filtered with its neighbour's radius (the staged halo, say) is seen
        rolled = K.blur_ref(x, np.roll(c.radii, 1), np.roll(taps, 1, axis=0), F64)
        assert float(np.abs(rolled - ref).max()) > 100 * K.bar(ye, scale)


# ---- low-resolution simulation -------------------------------------------------------------------------------------------------------
def test_lowres_table_reaches_every_instantiation_and_the_patch_bound():
    seen, extents = set(), set()
    for c in K.LOWRES_CASES:
        Z, Y, X = c.zyx
        assert len(c.lows) == c.M and all(1 <= nl <= n for low in c.lows for nl, n in zip(low, (X, Y, Z)))
        for tag, shift in K.launches(c):
            launch = K.lowres_launch(c, shift)
            assert launch != 'copy'
            seen.add((launch, c.M) if launch[0] == 0 else (launch, None))
        patches = [K.lowres_patch(c, m) for m in range(c.M)]
        for m, low in enumerate(c.lows):
            for n, nl, tile, bound in zip((X, Y, Z), low, (K.TX, K.TY, K.TZ), K.LR_P):
                assert all(4 <= e <= bound for e in K.lowres_extents(n, nl, tile)), (c.name, m)      # every tile fits the LDS patch
            extents.add(patches[m])
        print('lowres {:24s} launches {}  tiles {} x {} x {}  low grids {}  largest patch (x, y, z) {}'.format(
            c.name, ['<{}, {}>'.format(l[0], str(l[1]).lower()) for l in (K.lowres_launch(c, s) for _, s in K.launches(c))],
            *K.tiles(c.zyx), c.lows, patches))
    assert {l for l, _ in seen} == set(K.LOWRES_LAUNCHES)
    assert {M for l, M in seen if l == (0, False)} == {3, 5, 8}
    assert K.LR_P in extents and K.LR_P == (35, 11, 11)
    # the issue's worked examples
    assert int(K.lowres_k(31, 64, 63)) - int(K.lowres_k(0, 64, 63)) + 4 == 35 and K.lowres_extents(16, 15, 8) == [11, 11]
    assert K.lowres_extents(64, 63, 32) == [35, 35] and K.lowres_extents(65, 64, 32)[:2] == [35, 35]


def test_lowres_table_edges():
    by = {c.name: c for c in K.LOWRES_CASES}
    c = by['m4_one_low_voxel']
    assert c.zyx == (9, 9, 33) and [tuple(n == 1 for n in low) for low in c.lows] == [(True, False, False), (False, True, False),
                                                                                      (False, False, True), (True, True, True)]
    assert all(int(K.lowres_k(i, 33, 1)) == (-1 if i < 16 else 0) for i in range(33))        # the k = -1 branch on the first half
    full = lambda c, low: sum(nl == n for nl, n in zip(low, c.zyx[::-1]))
    assert sorted(full(by['m2_full_axes'], low) for low in by['m2_full_axes'].lows) == [1, 2]
    for name, launches in (('m4_one_copied', [(4, True), (4, False)]), ('m5_one_copied', [(0, False)])):
        c = by[name]
        assert [K.lowres_launch(c, s) for _, s in K.launches(c)] == launches
        assert sum(full(c, low) == 3 for low in c.lows) == 1 and sum(full(c, low) < 3 for low in c.lows) == c.M - 1
    # the zooms of tests/test_gpu_resolution_augment.py: 0.99 is the identity on every axis of its three shapes, not on X = 64
    for zyx in ((5, 7, 9), (16, 16, 16), (1, 8, 33)):
        assert oracle_lowres_sizes(zyx[::-1], 0.99) == zyx[::-1]
    assert by['m3_zooms'].lows == ((32, 8, 5), (17, 4, 2), (63, 16, 9))
    for zoom in (0.5, 0.26, 0.99):
        assert K.zoom_sizes((64, 16, 9), zoom) == oracle_lowres_sizes((64, 16, 9), zoom)


@pytest.mark.parametrize('zyx', [(5, 7, 9), (9, 16, 64), (17, 17, 65)], ids=str)
def test_lowres_reference_equals_the_oracle(zyx):
    x = np.random.RandomState(4).randn(*zyx, 5)
    size = zyx[::-1]
    lows = [oracle_lowres_sizes(size, z) for z in (0.5, 0.26, 0.99, 0.75)] + [(1, 1, 1)]
    got = K.lowres_ref(x, lows, F64)
    for m, low in enumerate(lows):
        assert np.abs(got[..., m] - oracle_lowres(x[..., m], low)).max() <= 8 * np.finfo(F64).eps * np.abs(x).max(), low
    assert np.array_equal(K.lowres_ref(x, [size] * 5, F64), x)


@pytest.mark.parametrize('case', K.LOWRES_CASES, ids=K.case_id)
def test_lowres_yardstick_and_disagreement(case):
    c = case
    x = K.crop(c)
    Z, Y, X = c.zyx
    scale = float(np.abs(x).max())
    ref, yard = K.lowres_ref(x, c.lows, F64), K.lowres_ref(x, c.lows, F32)
    assert yard.dtype == F32 and ref.dtype == F64
    ye = float(np.abs(yard.astype(F64) - ref).max())
    print('lowres {:24s} yardstick {:.3e} = {:.3e} x max|x|, bar {:.3e} x max|x|'.format(c.name, ye, ye / scale, K.bar(ye, scale) / scale))
    assert ye <= 0.25 * K.CAP * scale
    moved = K.lowres_ref(x, K.off_by_one(c), F64)
    for m, low in enumerate(c.lows):
        d = float(np.abs(moved[..., m] - ref[..., m]).max())
        if tuple(low) == (X, Y, Z):
            assert d == 0.0 and np.array_equal(yard[..., m].view(np.int32), x[..., m].view(np.int32))
        else:
            assert d > 100 * K.bar(ye, scale), (m, d)
