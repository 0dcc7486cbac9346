"""CPU checks of the case-level normalisers (VolumeNormalizer type 2, ClipZScoreNormalizer type 3): dictionaries, the host
restatement, the nearest-rank rule and the device struct."""
import ctypes
import math

import numpy as np
import pytest

from segmentation3d.utils.normalizer import (AdaptiveNormalizer, ClipZScoreNormalizer, FixedNormalizer, VolumeNormalizer,
                                             host_volume_stats, nearest_rank, normalizer_from_dict, resolved_normalizer)


def _image(seed=3, shape=(9, 11, 13)):
    rng = np.random.RandomState(seed)
    a = rng.normal(120.0, 40.0, size=shape).astype(np.float32)
    a[rng.uniform(size=shape) < 0.35] = 0.0           # background
    return a


@pytest.mark.parametrize('norm', [VolumeNormalizer(), VolumeNormalizer('all'), VolumeNormalizer('nonzero', (0.5, 99.5)),
                                  VolumeNormalizer('all', [1, 99], 5), VolumeNormalizer(clip_sigma=3.5),
                                  ClipZScoreNormalizer(100.0, 25.0), ClipZScoreNormalizer(-3.5, 0.25, -1000, 3000.5),
                                  ClipZScoreNormalizer(0.0, 1.0, None, 2.0), ClipZScoreNormalizer(0.0, 1.0, -2.0)])
def test_dict_round_trip(norm):
    d = norm.to_dict()
    back = normalizer_from_dict(d)
    assert type(back) is type(norm) and back.to_dict() == d
    if isinstance(norm, VolumeNormalizer):
        assert d['type'] == 2 and sorted(d) == ['clip_percentiles', 'clip_sigma', 'foreground', 'type']
    else:
        assert d['type'] == 3 and sorted(d) == ['lower', 'mean', 'stddev', 'type', 'upper']


def test_existing_types_still_round_trip():
    for norm in (FixedNormalizer(1.0, 2.0, True), AdaptiveNormalizer(4)):
        assert normalizer_from_dict(norm.to_dict()).to_dict() == norm.to_dict()
    with pytest.raises(ValueError):
        normalizer_from_dict({'type': 4})


@pytest.mark.parametrize('make', [
    lambda: VolumeNormalizer('mask'), lambda: VolumeNormalizer('nonzero', (99.5, 0.5)), lambda: VolumeNormalizer(clip_percentiles=(5, 5)),
    lambda: VolumeNormalizer(clip_percentiles=(-1, 50)), lambda: VolumeNormalizer(clip_percentiles=(0, 100.5)),
    lambda: VolumeNormalizer(clip_percentiles=(1, 2, 3)), lambda: VolumeNormalizer(clip_percentiles='ab'),
    lambda: VolumeNormalizer(clip_sigma=0), lambda: VolumeNormalizer(clip_sigma=-2), lambda: VolumeNormalizer(clip_sigma='x'),
    lambda: ClipZScoreNormalizer(0.0, 0.0), lambda: ClipZScoreNormalizer(0.0, -1.0), lambda: ClipZScoreNormalizer(0.0, 1.0, 2.0, 1.0),
    lambda: ClipZScoreNormalizer(float('nan'), 1.0), lambda: ClipZScoreNormalizer(0.0, float('inf')),
    lambda: ClipZScoreNormalizer('m', 1.0), lambda: ClipZScoreNormalizer(0.0, 1.0, float('nan'), None),
    lambda: normalizer_from_dict({'type': 2, 'foreground': 'air', 'clip_percentiles': None, 'clip_sigma': None}),
    lambda: normalizer_from_dict({'type': 3, 'mean': 0.0, 'stddev': 0.0, 'lower': None, 'upper': None}),
])
def test_invalid_arguments_raise_value_error(make):
    with pytest.raises(ValueError):
        make()


def test_nearest_rank_rule():
    for n in (1, 2, 3, 10, 201, 1000, 12345):
        assert nearest_rank(0.0, n) == 0 and nearest_rank(1.0, n) == n - 1
        for q in (0.005, 0.25, 0.5, 0.75, 0.995):
            assert nearest_rank(q, n) == int(math.floor(q * (n - 1) + 0.5))
    assert nearest_rank(0.5, 1) == 0
    assert nearest_rank(0.5, 2) == 1            # 0.5 + 0.5 rounds half up
    assert nearest_rank(0.5, 3) == 1
    assert nearest_rank(0.005, 201) == 1 and nearest_rank(0.995, 201) == 199
    # less than one gap between neighbouring order statistics away from numpy's linear interpolation
    s = np.sort(np.random.RandomState(0).normal(size=777))
    for q in (0.005, 0.3, 0.5, 0.995):
        k = nearest_rank(q, s.size)
        lin = np.percentile(s, 100.0 * q)
        assert s[max(k - 1, 0)] <= lin <= s[min(k + 1, s.size - 1)]
    with pytest.raises(ValueError):
        nearest_rank(1.5, 10)
    with pytest.raises(ValueError):
        nearest_rank(0.5, 0)


def test_host_volume_stats_against_direct_float64():
    a = _image()
    fg = np.sort(a[a != 0]).astype(np.float64)
    st = host_volume_stats(a, 'nonzero', [0.005, 0.995], clip=True)
    lo, hi = fg[int(math.floor(0.005 * (fg.size - 1) + 0.5))], fg[int(math.floor(0.995 * (fg.size - 1) + 0.5))]
    c = np.clip(fg, lo, hi)
    assert st['n'] == fg.size and st['min'] == fg[0] and st['max'] == fg[-1] and st['q'] == [lo, hi]
    assert st['mean'] == pytest.approx(c.mean(), rel=1e-13) and st['std'] == pytest.approx(c.std(), rel=1e-13)
    allv = host_volume_stats(a, 'all')
    assert allv['n'] == a.size and allv['mean'] == pytest.approx(a.astype(np.float64).mean(), rel=1e-13)
    empty = host_volume_stats(np.zeros((3, 3, 3), np.float32), 'nonzero', [0.5])
    assert empty == {'n': 0, 'min': 0.0, 'max': 0.0, 'mean': 0.0, 'std': 1e-6, 'q': [0.0]}
    neg0 = host_volume_stats(np.array([-0.0, 0.0, -0.0], np.float32), 'all', [0.0, 1.0])
    assert neg0['n'] == 3 and not np.signbit(neg0['min']) and not np.signbit(neg0['q'][0])
    assert host_volume_stats(np.array([-0.0, 0.0], np.float32), 'nonzero')['n'] == 0


def test_volume_normalizer_call_against_direct_float64():
    a = _image(5)
    v = a.astype(np.float64)
    fg = np.sort(v[v != 0])
    out = VolumeNormalizer()(a.copy())
    assert out.dtype == np.float32
    np.testing.assert_array_equal(out, ((v - fg.mean()) / fg.std()).astype(np.float32))
    # percentiles: clip to the nearest-rank order statistics, moments of the clipped foreground; every voxel normalised
    lo, hi = fg[nearest_rank(0.02, fg.size)], fg[nearest_rank(0.98, fg.size)]
    c = np.clip(fg, lo, hi)
    out = VolumeNormalizer('nonzero', (2, 98))(a.copy())
    np.testing.assert_array_equal(out, ((np.clip(v, lo, hi) - c.mean()) / c.std()).astype(np.float32))
    # foreground 'all' + clip_sigma
    out = VolumeNormalizer('all', None, 1.5)(a.copy())
    m, s = np.sort(v.ravel()).mean(), np.sort(v.ravel()).std()      # (the restatement sums the sorted values)
    np.testing.assert_array_equal(out, ((np.clip(v, m - 1.5 * s, m + 1.5 * s) - m) / s).astype(np.float32))
    assert abs(out).max() <= 1.5 + 1e-6
    # an empty selection falls back to 'all'; a constant image has std = the floor
    z = np.zeros((4, 4, 4), np.float32)
    np.testing.assert_array_equal(VolumeNormalizer()(z.copy()), z)
    # Image3d in, Image3d out
    from segmentation3d.utils.image3d import Image3d
    im = VolumeNormalizer()(Image3d(a.copy()))
    np.testing.assert_array_equal(im.array, VolumeNormalizer()(a.copy()))


def test_clip_zscore_call_against_direct_float64():
    a = _image(7)
    v = a.astype(np.float64)
    np.testing.assert_array_equal(ClipZScoreNormalizer(90.0, 30.0, 10.0, 180.0)(a.copy()),
                                  ((np.clip(v, 10.0, 180.0) - 90.0) / 30.0).astype(np.float32))
    np.testing.assert_array_equal(ClipZScoreNormalizer(90.0, 30.0)(a.copy()), ((v - 90.0) / 30.0).astype(np.float32))
    np.testing.assert_array_equal(ClipZScoreNormalizer(90.0, 30.0, None, 100.0)(a.copy()),
                                  ((np.minimum(v, 100.0) - 90.0) / 30.0).astype(np.float32))


def test_resolve_gives_the_case_numbers():
    a = _image(11)
    vn = VolumeNormalizer('nonzero', (1, 99), 4)
    st = host_volume_stats(a, 'nonzero', [0.01, 0.99], clip=True)
    r = resolved_normalizer(vn.to_dict(), st)
    assert isinstance(r, ClipZScoreNormalizer) and r.mean == st['mean'] and r.stddev == st['std']
    assert r.lower == max(st['q'][0], st['mean'] - 4 * st['std']) and r.upper == min(st['q'][1], st['mean'] + 4 * st['std'])
    np.testing.assert_array_equal(r(a.copy()), vn(a.copy()))


# ---- the device struct --------------------------------------------------------------------------------------------------
def _fields(p):
    return [(p.n[m].type, p.n[m].mean, p.n[m].stddev, p.n[m].clip, p.n[m].clip_lo, p.n[m].clip_hi) for m in range(8)]


def test_normalizer_params_unresolved_type2_raises():
    from segmentation3d.utils.image_tools import normalizer_params
    with pytest.raises(ValueError, match='resolve'):
        normalizer_params([VolumeNormalizer()], 1)
    with pytest.raises(ValueError, match='resolve'):
        normalizer_params([None, VolumeNormalizer().to_dict()], 2)


def test_normalizer_params_existing_types_are_byte_identical():
    """types 0, 1 and None: the struct is what the code before this feature built (restated here field by field)"""
    from segmentation3d import _engine as E
    from segmentation3d.utils.image_tools import normalizer_params
    norms = [FixedNormalizer(20.5, 50.25, True), AdaptiveNormalizer(2.5), None, FixedNormalizer(-3.0, 0.1, False).to_dict(),
             AdaptiveNormalizer().to_dict()]
    got = normalizer_params(norms, 5)
    want = E.Normalizers()
    rows = [(0, 20.5, 50.25, 1, -1.0, 1.0), (1, 0.0, 1.0, 1, -2.5, 2.5), (-1, 0.0, 1.0, 0, -1.0, 1.0),
            (0, -3.0, 0.1, 0, -1.0, 1.0), (1, 0.0, 1.0, 1, -3.0, 3.0)] + [(-1, 0.0, 1.0, 0, -1.0, 1.0)] * 3
    for m, row in enumerate(rows):
        n = want.n[m]
        n.type, n.mean, n.stddev, n.clip, n.clip_lo, n.clip_hi = row
    assert bytes(got) == bytes(want) and ctypes.sizeof(got) == 8 * 24


def test_normalizer_params_type3_maps_to_struct_type0():
    from segmentation3d.utils.image_tools import normalizer_params, has_volume_normalizer, resolve_normalizers
    p = normalizer_params([ClipZScoreNormalizer(100.0, 30.0, -50.0, 400.0), ClipZScoreNormalizer(1.0, 2.0),
                           ClipZScoreNormalizer(1.0, 2.0, None, 9.0)], 3)
    f = _fields(p)
    lo = float((np.float32(-50.0) - np.float32(100.0)) / np.float32(30.0))
    hi = float((np.float32(400.0) - np.float32(100.0)) / np.float32(30.0))
    assert f[0] == (0, 100.0, 30.0, 1, lo, hi)
    assert f[1] == (0, 1.0, 2.0, 0, -1.0, 1.0)
    assert f[2] == (0, 1.0, 2.0, 1, float('-inf'), 4.0)
    assert has_volume_normalizer([None, VolumeNormalizer()]) and not has_volume_normalizer([None, AdaptiveNormalizer()])
    # no type 2 in the list: returned as it is, no device work (this test runs without a GPU)
    norms = [AdaptiveNormalizer(), None]
    assert resolve_normalizers(norms, None) == norms
