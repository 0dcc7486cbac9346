"""Host side of the Gaussian blur and the low-resolution simulation of training crops: the
float64 numpy oracles of both transforms, written from the definitions and pinned here on the CPU (the blur against
scipy), the tap / low-grid helpers, the option checks of the `resolution_augmentation` section and the RNG order of
`SegmentationDataset.sample_resolution_augmentation`.  The oracles are shared with tests/test_gpu_resolution_augment.py."""
import numpy as np
import pytest
import torch

from test_augment import _dataset, _same_state, ALL_ON


# ---------------------------------------------------------------------------------------------------------------------
# numpy oracles, float64
# ---------------------------------------------------------------------------------------------------------------------
def oracle_reflect(i, n):
    """half-sample reflection d c b a | a b c d | d c b a of integer indices, any n >= 1"""
    r = np.mod(np.asarray(i, dtype=np.int64), 2 * n)
    return np.where(r >= n, 2 * n - 1 - r, r)


def oracle_taps(sigma, as_float32=True):
    """(R, w[-R..R]) float64; as_float32: every tap rounded to float32 as the host passes it to the kernel"""
    R = int(np.ceil(3.0 * sigma))
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-k * k / (2.0 * sigma * sigma))
    w = w / w.sum()
    return R, (w.astype(np.float32).astype(np.float64) if as_float32 else w)


def oracle_blur(x, sigma, as_float32=True):
    """x [Z, Y, X] -> float64 blurred volume: separable x, y, z with reflected borders; sigma 0 returns x"""
    y = np.asarray(x, dtype=np.float64)
    if sigma == 0:
        return y.copy()
    R, w = oracle_taps(sigma, as_float32)
    for axis in (2, 1, 0):
        n = y.shape[axis]
        acc = np.zeros_like(y)
        for k in range(-R, R + 1):
            acc += w[k + R] * np.take(y, oracle_reflect(np.arange(n) + k, n), axis=axis)
        y = acc
    return y


def oracle_lowres_sizes(size, zoom):
    return tuple(max(1, int(np.floor(n * zoom + 0.5))) for n in size)


def _lowres_axis(n, nl):
    """source indices [4, n] and weights [4, n] of one axis"""
    i = np.arange(n, dtype=np.int64)
    t = (2 * i + 1) * nl - n
    k = np.floor_divide(t, 2 * n)
    f = (t - 2 * n * k).astype(np.float64) / (2 * n)
    w = np.stack([-0.5 * f ** 3 + f ** 2 - 0.5 * f, 1.5 * f ** 3 - 2.5 * f ** 2 + 1.0,
                  -1.5 * f ** 3 + 2.0 * f ** 2 + 0.5 * f, 0.5 * f ** 3 - 0.5 * f ** 2])
    q = np.clip(np.stack([k - 1, k, k + 1, k + 2]), 0, nl - 1)
    s = np.minimum(n - 1, ((2 * q + 1) * n) // (2 * nl))
    return s, w


def oracle_lowres(x, low_xyz):
    """x [Z, Y, X], low-grid sizes (nx', ny', nz') -> float64: nearest down-sampling, Keys cubic up-sampling"""
    y = np.asarray(x, dtype=np.float64)
    for axis, nl in ((2, low_xyz[0]), (1, low_xyz[1]), (0, low_xyz[2])):
        n = y.shape[axis]
        s, w = _lowres_axis(n, int(nl))
        shape = [1, 1, 1]
        shape[axis] = n
        y = sum(w[j].reshape(shape) * np.take(y, s[j], axis=axis) for j in range(4))
    return y


# ---------------------------------------------------------------------------------------------------------------------
# taps, sizes, oracle properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma,R', [(0.34, 2), (0.5, 2), (1.0, 3), (2.0, 6)])
def test_gaussian_taps(sigma, R):
    from segmentation3d.utils.image_tools import gaussian_taps
    r, w = gaussian_taps(sigma)
    assert r == R == int(np.ceil(3 * sigma)) and w.shape == (2 * R + 1,) and w.dtype == np.float64
    assert np.array_equal(w, w[::-1])
    assert abs(w.sum() - 1.0) <= 1e-7 and abs(w.astype(np.float32).astype(np.float64).sum() - 1.0) <= 1e-7
    assert np.allclose(w, oracle_taps(sigma, False)[1], rtol=0, atol=1e-15)
    assert np.all(np.diff(w[:R + 1]) > 0)


@pytest.mark.parametrize('bad', [0.0, -1.0, 2.0001, 3.0, float('nan'), float('inf')])
def test_gaussian_taps_refuse_bad_sigma(bad):
    from segmentation3d.utils.image_tools import gaussian_taps
    with pytest.raises(ValueError):
        gaussian_taps(bad)


@pytest.mark.parametrize('shape,sigma', [((5, 7, 9), 2.0), ((1, 1, 17), 2.0), ((1, 1, 17), 0.8)])
def test_blur_oracle_equals_scipy(shape, sigma):
    ndimage = pytest.importorskip('scipy.ndimage')
    x = np.random.RandomState(1).randn(*shape)
    R = int(np.ceil(3 * sigma))
    want = ndimage.gaussian_filter(x, sigma, radius=R, mode='reflect')
    got = oracle_blur(x, sigma, as_float32=False)
    assert np.abs(got - want).max() <= 1e-12


def test_reflection_is_defined_for_every_length_and_radius():
    assert oracle_reflect(np.arange(-6, 7), 1).tolist() == [0] * 13
    assert oracle_reflect(np.arange(-4, 8), 4).tolist() == [3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0]
    assert oracle_reflect(np.arange(-6, 8), 2).tolist() == [1, 0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1, 1, 0]


def test_lowres_sizes():
    from segmentation3d.utils.image_tools import lowres_sizes
    assert lowres_sizes((96, 96, 96), 0.5) == (48, 48, 48)
    assert lowres_sizes((5, 7, 9), 0.5) == (3, 4, 5)              # 2.5, 3.5, 4.5 round half up
    assert lowres_sizes((5, 7, 9), 0.3) == (2, 2, 3)              # 1.5 -> 2, 2.1 -> 2, 2.7 -> 3
    assert lowres_sizes((1, 3, 33), 0.01) == (1, 1, 1)            # floor of 1
    assert lowres_sizes((5, 7, 9), 1.0) == (5, 7, 9)
    assert all(isinstance(v, int) for v in lowres_sizes((5, 7, 9), 0.7))
    for size, zoom in (((16, 16, 16), 0.26), ((33, 8, 1), 0.99)):
        assert lowres_sizes(size, zoom) == oracle_lowres_sizes(size, zoom)
    for bad in (0.0, -0.5, 1.01, float('nan')):
        with pytest.raises(ValueError):
            lowres_sizes((5, 7, 9), bad)


def test_lowres_oracle_properties():
    x = np.random.RandomState(2).randn(5, 7, 9)
    assert np.array_equal(oracle_lowres(x, (9, 7, 5)), x)                      # n' = n: weights (0, 1, 0, 0)
    const = np.full((5, 7, 9), 3.25)
    for low in ((4, 3, 2), (1, 1, 1), (9, 2, 5)):
        assert np.abs(oracle_lowres(const, low) - 3.25).max() <= 1e-12
    y = oracle_lowres(x, (1, 7, 5))                                            # one low voxel along x
    assert np.abs(y - y[:, :, :1]).max() <= 1e-12 and np.ptp(y) > 0.1
    y = oracle_lowres(x, (9, 7, 1))
    assert np.abs(y - y[:1]).max() <= 1e-12
    # nearest, centre-aligned down-sampling of 8 -> 4 takes the voxels 1, 3, 5, 7
    s, _ = _lowres_axis(8, 4)
    assert sorted(set(s.ravel().tolist())) == [1, 3, 5, 7]


# ---------------------------------------------------------------------------------------------------------------------
# struct builders
# ---------------------------------------------------------------------------------------------------------------------
def test_blur_params_struct():
    from segmentation3d.utils.image_tools import blur_params, gaussian_taps
    p = blur_params([1.0, 0.0, None, 2.0], 4)
    assert list(p.radius) == [3, 0, 0, 6, 0, 0, 0, 0]
    for m, s in ((0, 1.0), (3, 2.0)):
        R, w = gaussian_taps(s)
        assert [p.taps[m][k] for k in range(R + 1)] == [float(np.float32(w[R + k])) for k in range(R + 1)]
    for bad, M in (([1.0], 2), ([2.5], 1), ([-1.0], 1), ([float('nan')], 1), ([1.0] * 9, 9), ([], 0)):
        with pytest.raises(ValueError):
            blur_params(bad, M)


def test_lowres_params_struct():
    from segmentation3d.utils.image_tools import lowres_params
    p = lowres_params([(3, 4, 5), None], 2, (9, 7, 5))
    assert (p.nx[0], p.ny[0], p.nz[0], p.nx[1], p.ny[1], p.nz[1]) == (3, 4, 5, 9, 7, 5)
    assert lowres_params([(3, 4, 5)], 1).nz[0] == 5
    for bad, M, size in (([(3, 4, 5)], 2, None), ([(0, 4, 5)], 1, None), ([(3, 4)], 1, None), ([(3.5, 4, 5)], 1, None),
                         ([(10, 4, 5)], 1, (9, 7, 5)), ([None], 1, None), ([(1, 1, 1)] * 9, 9, None)):
        with pytest.raises(ValueError):
            lowres_params(bad, M, size)


# ---------------------------------------------------------------------------------------------------------------------
# the section
# ---------------------------------------------------------------------------------------------------------------------
BOTH_ON = {'blur_sigma_vox': [0.5, 1.5], 'blur_prob': 0.6, 'lowres_zoom': [0.5, 0.9], 'lowres_prob': 0.6}


def test_defaults_are_off_and_apart_from_the_augmentation_section():
    from segmentation3d.dataloader.dataset import (AUGMENTATION_DEFAULTS, RESOLUTION_AUGMENTATION_DEFAULTS,
                                                   validate_resolution_augmentation)
    assert RESOLUTION_AUGMENTATION_DEFAULTS == {'blur_sigma_vox': [0.0, 0.0], 'blur_prob': 0.0, 'lowres_zoom': [1.0, 1.0],
                                                'lowres_prob': 0.0}
    assert not set(AUGMENTATION_DEFAULTS) & set(RESOLUTION_AUGMENTATION_DEFAULTS)
    assert validate_resolution_augmentation(None) is None
    assert validate_resolution_augmentation({}) is None
    assert validate_resolution_augmentation(dict(RESOLUTION_AUGMENTATION_DEFAULTS)) is None
    assert validate_resolution_augmentation(dict(BOTH_ON, blur_prob=0.0, lowres_prob=0)) is None
    assert validate_resolution_augmentation({'blur_prob': 1.0, 'lowres_prob': 1.0}) is None      # neutral ranges
    assert validate_resolution_augmentation({'lowres_zoom': [1.0, 1.0], 'lowres_prob': 1.0}) is None
    full = validate_resolution_augmentation(BOTH_ON)
    assert full['enabled'] == {'blur': True, 'lowres': True} and full['blur_sigma_vox'] == [0.5, 1.5]
    assert validate_resolution_augmentation(dict(BOTH_ON, blur_prob=0.0))['enabled'] == {'blur': False, 'lowres': True}
    assert validate_resolution_augmentation({'blur_sigma_vox': [1, 2], 'blur_prob': 1})['enabled'] == {
        'blur': True, 'lowres': False}


@pytest.mark.parametrize('bad', [
    {'blur': 1.0}, {'brightness': [1.0, 1.0]},                                # unknown keys
    [1, 2], 'on',                                                            # not a dict
    {'blur_prob': 1.5}, {'blur_prob': -0.1}, {'lowres_prob': 2}, {'lowres_prob': 'often'},
    {'blur_sigma_vox': [-0.1, 1.0]}, {'blur_sigma_vox': [1.5, 1.0]}, {'blur_sigma_vox': [0.5, 2.5]}, {'blur_sigma_vox': 1.0},
    {'blur_sigma_vox': [0.5, float('nan')]}, {'blur_sigma_vox': [0.5, 1.0, 1.5]},
    {'blur_sigma_vox': [0.0, 1.0], 'blur_prob': 0.5},                         # on, but a drawn sigma may be 0
    {'lowres_zoom': [0.0, 1.0]}, {'lowres_zoom': [0.8, 0.5]}, {'lowres_zoom': [0.5, 1.2]}, {'lowres_zoom': 'half'},
    {'lowres_zoom': [-0.5, 0.5]},
])
def test_invalid_sections_raise(tmp_path, bad):
    from segmentation3d.dataloader.dataset import validate_resolution_augmentation
    with pytest.raises(ValueError):
        validate_resolution_augmentation(bad)
    with pytest.raises(ValueError):
        _dataset(tmp_path, resolution_augmentation=bad)


# ---------------------------------------------------------------------------------------------------------------------
# the draws
# ---------------------------------------------------------------------------------------------------------------------
def _draw_all(ds, with_resolution):
    _, sp = ds.sample_crop_geometry(0)
    ds.sample_mirror()
    ds.sample_augmentation(sp)
    return ds.sample_resolution_augmentation() if with_resolution else None


@pytest.mark.parametrize('aug', [None, ALL_ON])
def test_rng_stream_with_the_section_absent_or_off_is_unchanged(tmp_path, aug):
    from segmentation3d.utils.file_io import ensure_easydict
    ensure_easydict()
    from easydict import EasyDict as edict
    ref = _dataset(tmp_path, augmentation=aug, random_mirror_axes=('x',))
    np.random.seed(7)
    for _ in range(3):
        _draw_all(ref, False)
    want = np.random.get_state()
    for section in (None, {}, edict(dict(BOTH_ON, blur_prob=0.0, lowres_prob=0.0)), {'blur_prob': 1.0, 'lowres_prob': 1.0}):
        ds = _dataset(tmp_path, augmentation=aug, random_mirror_axes=('x',), resolution_augmentation=section)
        assert ds.resolution_augmentation is None
        np.random.seed(7)
        for _ in range(3):
            assert _draw_all(ds, True) is None
        assert _same_state(np.random.get_state(), want)


def test_rng_order_with_both_on(tmp_path):
    """the documented order, restated draw by draw, after every existing draw of the sample"""
    from segmentation3d.utils.image_tools import lowres_sizes
    ds = _dataset(tmp_path, augmentation=ALL_ON, random_mirror_axes=('x',), resolution_augmentation=BOTH_ON)
    ref = _dataset(tmp_path, augmentation=ALL_ON, random_mirror_axes=('x',))
    ds._num_modality = ref._num_modality = 2                    # the draws depend on the modality count alone
    seen = {'blur': 0, 'lowres': 0, 'blur_one_modality': 0, 'lowres_off': 0}
    for seed in range(16):
        np.random.seed(seed)
        got = _draw_all(ds, True)
        state = np.random.get_state()
        np.random.seed(seed)
        _draw_all(ref, False)
        sigmas, sizes = [], []
        for m in range(2):
            sigma, low = 0.0, None
            if np.random.uniform() < BOTH_ON['blur_prob']:
                sigma = np.random.uniform(0.5, 1.5)
            if np.random.uniform() < BOTH_ON['lowres_prob']:
                low = lowres_sizes((16, 16, 16), np.random.uniform(0.5, 0.9))
            sigmas.append(sigma)
            sizes.append(low)
        assert _same_state(state, np.random.get_state()), seed
        assert got['blur'] == (sigmas if any(sigmas) else None)
        assert got['lowres'] == (sizes if any(s is not None for s in sizes) else None)
        seen['blur'] += got['blur'] is not None
        seen['lowres'] += got['lowres'] is not None
        seen['blur_one_modality'] += got['blur'] is not None and 0.0 in got['blur']
        seen['lowres_off'] += got['lowres'] is None
    assert all(v > 0 for v in seen.values()), seen


def test_each_modality_draws_independently_and_an_off_transform_draws_nothing(tmp_path):
    ds = _dataset(tmp_path, resolution_augmentation={'blur_sigma_vox': [0.5, 2.0], 'blur_prob': 1.0})
    ds._num_modality = 3
    np.random.seed(3)
    got = ds.sample_resolution_augmentation()
    state = np.random.get_state()
    np.random.seed(3)
    want = []
    for _ in range(3):
        assert np.random.uniform() < 1.0
        want.append(np.random.uniform(0.5, 2.0))
    assert _same_state(state, np.random.get_state())
    assert got == {'blur': want, 'lowres': None} and len(set(want)) == 3
    ds = _dataset(tmp_path, resolution_augmentation={'lowres_zoom': [0.3, 0.6], 'lowres_prob': 1.0})
    ds._num_modality = 2
    np.random.seed(4)
    got = ds.sample_resolution_augmentation()
    state = np.random.get_state()
    np.random.seed(4)
    zooms = []
    for _ in range(2):
        assert np.random.uniform() < 1.0
        zooms.append(np.random.uniform(0.3, 0.6))
    assert _same_state(state, np.random.get_state())
    assert got['blur'] is None and got['lowres'] == [oracle_lowres_sizes((16, 16, 16), z) for z in zooms]


def test_device_entries_refuse_host_tensors():
    """there is no CPU path: the filters raise on a tensor that is not on a ROCm device"""
    from segmentation3d import _engine as E
    from segmentation3d.utils.image_tools import blur_device, lowres_device
    x = torch.zeros(4, 4, 4)
    with pytest.raises(E.Seg3dEngineError):
        blur_device(x, [1.0])
    with pytest.raises(E.Seg3dEngineError):
        lowres_device(x, [0.5])
