"""CPU side of the cubic B-spline interpolation: the float64 oracle of tests/bspline_oracle.py
pinned against scipy.ndimage and against its own definition, and the host-side switches of the third interpolation mode."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import bspline_oracle as O
from test_blend_tta import _toy_case

SHAPES = [(1, 1, 1), (2, 3, 5), (5, 1, 7), (1, 2, 40), (9, 17, 33)]         # z, y, x


def _volume(shape, seed=0):
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=shape)


@pytest.mark.parametrize('n', [1, 2, 3, 5, 8])
def test_mirror_is_the_whole_sample_mirror(n):
    want = np.pad(np.arange(n), 3 * n + 3, mode='reflect') if n > 1 else np.zeros(7 * n + 6, dtype=np.int64)
    got = O.mirror(np.arange(-(3 * n + 3), n + 3 * n + 3), n)
    assert np.array_equal(got, want)
    if n > 1:
        assert int(O.mirror(-1, n)) == 1 and int(O.mirror(n, n)) == n - 2


@pytest.mark.parametrize('shape', SHAPES)
def test_dense_prefilter_is_scipys_spline_filter(shape):
    s = _volume(shape)
    want = ndi.spline_filter(s, order=3, mode='mirror', output=np.float64)
    assert float(np.abs(O.prefilter(s) - want).max()) <= 1e-12


@pytest.mark.parametrize('n', [2, 3, 5, 40, 200])
def test_recursive_form_equals_the_dense_solve(n):
    s = _volume((1, 3, n), seed=n)
    assert float(np.abs(O.prefilter_recursive(s) - O.prefilter(s)).max()) <= 1e-12


def test_prefilter_channels_are_independent():
    s = _volume((4, 5, 6, 3))
    c = O.prefilter(s)
    for m in range(3):
        assert np.array_equal(c[..., m], O.prefilter(s[..., m]))


@pytest.mark.parametrize('shape', [(2, 3, 5), (9, 17, 33)])
def test_evaluation_is_scipys_map_coordinates(shape):
    """mirror mode and whole-sample mirror agree wherever the inside test lets a sample through"""
    s = _volume(shape, seed=3)
    Z, Y, X = shape
    rng = np.random.RandomState(4)
    cx, cy, cz = (rng.uniform(-0.5, n - 0.5 - 1e-9, size=(6, 7, 8)) for n in (X, Y, Z))
    got = O.evaluate(O.prefilter(s), (cx, cy, cz), 0.0)
    want = ndi.map_coordinates(s, np.stack([cz, cy, cx]), order=3, mode='mirror', output=np.float64)
    # the oracle rounds to float once, as the definition says
    assert float(np.abs(got - want.astype(np.float32)).max()) <= 1e-12 + 2.0 ** -24 * float(np.abs(want).max())
    assert float(np.abs(got - want).max()) <= 2.0 ** -23 * float(np.abs(want).max())


@pytest.mark.parametrize('shape', SHAPES)
def test_the_interpolant_passes_through_the_samples(shape):
    s = _volume(shape, seed=5).astype(np.float32)
    Z, Y, X = shape
    coords = O.affine_coords(np.eye(3, 4), (X, Y, Z))
    got = O.evaluate(O.prefilter(s), coords, -3.5)
    assert np.array_equal(got.astype(np.float32), s)


def test_inside_test_and_padding():
    s = _volume((3, 4, 5), seed=6)
    A = np.eye(3, 4)
    A[:, 3] = (-0.75, 0.25, -0.5)
    cx, cy, cz = O.affine_coords(A, (6, 5, 4))
    got = O.evaluate(O.prefilter(s), (cx, cy, cz), -3.5)
    inside = (cx >= -0.5) & (cx < 4.5) & (cy >= -0.5) & (cy < 3.5) & (cz >= -0.5) & (cz < 2.5)
    assert 0 < int(inside.sum()) < inside.size
    assert np.all(got[~inside] == -3.5) and not np.any(got[inside] == -3.5)
    assert bool(inside[0, 0, 1]) and not bool(inside[0, 0, 0])              # cz = -0.5 is inside, cx = -0.75 is not


def test_affine_coords_are_written_left_to_right():
    A = np.random.RandomState(7).uniform(-1, 1, size=(3, 4))
    cx, cy, cz = O.affine_coords(A, (3, 4, 5))
    for (x, y, z) in ((2, 3, 4), (1, 0, 2)):
        for r, c in enumerate((cx, cy, cz)):
            assert c[z, y, x] == ((A[r, 0] * x + A[r, 1] * y) + A[r, 2] * z) + A[r, 3]


def test_fp32_run_is_close_but_not_equal():
    s = _volume((6, 7, 8), seed=8).astype(np.float32)
    c32, c64 = O.prefilter_recursive(s, np.float32), O.prefilter(s)
    assert c32.dtype == np.float32
    err = float(np.abs(c32.astype(np.float64) - c64).max())
    assert 0.0 < err < 1e-5


def test_dataset_accepts_bspline_and_rejects_cubic(tmp_path):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    lst = _toy_case(tmp_path)
    args = lambda interp: (lst, 3, [1.0, 1.0, 1.0], [16, 16, 16], 'GLOBAL', [3, 3, 3], [0.9, 1.1], interp,
                           [AdaptiveNormalizer()])
    ds = SegmentationDataset(*args('BSPLINE'), device=torch.device('cpu'))
    assert ds.interpolation == 'BSPLINE'
    with pytest.raises(AssertionError):
        SegmentationDataset(*args('CUBIC'), device=torch.device('cpu'))
    # a case of this mode is prefiltered at load, and that has no CPU path
    from segmentation3d import _engine as E
    with pytest.raises(E.Seg3dEngineError):
        ds.case(0)
    assert SegmentationDataset(*args('LINEAR'), device=torch.device('cpu')).case(0).volume.shape == (20, 24, 28, 1)


def test_unknown_method_still_raises():
    from segmentation3d.utils import image_tools
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    src = torch.zeros((4, 4, 4, 1))
    for method in ('CUBIC', 'bspline', None):
        with pytest.raises(ValueError, match='Unsupported interpolation type.'):
            image_tools.resample_device_mc(src, frame, (4, 4, 4), frame, method)
    # the mode itself is known: the next check (a host tensor) is what refuses
    from segmentation3d import _engine as E
    with pytest.raises(E.Seg3dEngineError):
        image_tools.resample_device_mc(src, frame, (4, 4, 4), frame, 'BSPLINE')


def test_default_interpolation_stays_linear():
    import os
    from conftest import PKG
    with open(os.path.join(PKG, 'segmentation3d', 'config', 'train_config.py')) as f:
        lines = [ln for ln in f if ln.startswith('__C.dataset.interpolation')]
    assert len(lines) == 1 and lines[0].split('#')[0].split('=')[1].strip() == "'LINEAR'"
    assert 'BSPLINE' in lines[0].split('#')[1]
