"""CPU side of the 'LABEL_LINEAR' label interpolation: the numpy oracle of
tests/label_interp_oracle.py on hand-computed cases and against scipy's order-1 interpolation of the indicator planes, the
config validator and the two C-ABI signatures.  The device entries are compared with this oracle, bit for bit, in
tests/test_gpu_label_interp.py."""
import os
import re

import numpy as np
import pytest

import label_interp_oracle as O
from conftest import REPO


def _shift(tx=0.0, ty=0.0, tz=0.0, sx=1.0, sy=1.0, sz=1.0):
    return np.array([[sx, 0.0, 0.0, tx], [0.0, sy, 0.0, ty], [0.0, 0.0, sz, tz]], dtype=np.float64)


def _random_labels(seed, shape=(11, 10, 9), labels=(0, 1, 2, 5, 255)):
    return np.random.RandomState(seed).choice(np.array(labels, dtype=np.float32), size=shape)


# ---- hand-computed cases ---------------------------------------------------------------------------------------------
def test_the_tie_goes_to_the_smallest_label():
    """[1, 2] sampled half way: both memberships are exactly 0.5 -> 1, in either order; 'NN' rounds half up"""
    at_half = _shift(tx=0.5)
    for row, nn in (([1, 2], 2.0), ([2, 1], 1.0)):
        vol = np.array(row, dtype=np.float32).reshape(1, 1, 2)
        labels, planes = O.memberships(vol, at_half, (1, 1, 1))
        assert labels.tolist() == [0.0, 1.0, 2.0] and planes[:, 0, 0, 0].tolist() == [0.0, 0.5, 0.5]
        assert O.label_linear(vol, at_half, (1, 1, 1)).tolist() == [[[1.0]]]
        assert O.nearest(vol, at_half, (1, 1, 1)).tolist() == [[[nn]]]


def test_three_labels_without_a_majority():
    """weights 0.4 / 0.35 / 0.25: no label reaches 0.5 and the strongest one -- the LARGEST value, on the first tap -- wins"""
    vol = np.array([[[5, 2], [1, 1]]], dtype=np.float32)             # y = 1 holds label 1 twice: weight dy = 0.25
    A = _shift(tx=7.0 / 15.0, ty=0.25)                               # (1 - dx) 0.75 = 0.4, dx 0.75 = 0.35
    labels, planes = O.memberships(vol, A, (1, 1, 1))
    assert labels.tolist() == [0.0, 1.0, 2.0, 5.0]
    np.testing.assert_allclose(planes[:, 0, 0, 0], [0.0, 0.25, 0.35, 0.4], rtol=0, atol=1e-7)
    assert O.label_linear(vol, A, (1, 1, 1)).tolist() == [[[5.0]]]
    # with the two strongest labels swapped in value the same tap wins: the rule is the membership, not the value
    assert O.label_linear(np.array([[[2, 5], [1, 1]]], dtype=np.float32), A, (1, 1, 1)).tolist() == [[[2.0]]]


def test_uniform_neighbourhood_returns_its_value():
    vol = np.full((3, 4, 5), 3.0, dtype=np.float32)
    A = _shift(0.37, 0.61, 0.29, 0.9, 0.8, 0.7)
    labels, planes = O.memberships(vol, A, (4, 3, 2), pad=3.0)
    assert labels.tolist() == [3.0] and bool((planes == 1.0).all())  # 1 + (1 - 1) d is exactly 1
    assert bool((O.label_linear(vol, A, (4, 3, 2), pad=0.0) == 3.0).all())


def test_outside_the_buffer_gives_pad():
    vol = _random_labels(1, (3, 4, 5))
    for A in (_shift(tx=-0.75), _shift(tx=4.5), _shift(ty=-0.51), _shift(tz=2.5)):
        out = O.label_linear(vol, A, (1, 1, 1), pad=7.0)
        assert out.tolist() == [[[7.0]]]
    for A in (_shift(tx=-0.5), _shift(tx=4.25), _shift(tz=2.49)):   # the half-open interval's inside edge: clamped taps
        assert float(O.label_linear(vol, A, (1, 1, 1), pad=7.0)[0, 0, 0]) in vol


def test_identity_map_returns_the_source():
    vol = _random_labels(2)
    Z, Y, X = vol.shape
    assert np.array_equal(O.label_linear(vol, _shift(), (X, Y, Z), pad=7.0), vol)


def test_integer_translation_equals_the_shifted_source():
    vol = _random_labels(3)
    Z, Y, X = vol.shape
    out = O.label_linear(vol, _shift(tx=2.0, ty=-1.0, tz=3.0), (X, Y, Z), pad=7.0)
    want = np.full_like(vol, 7.0)
    want[:Z - 3, 1:, :X - 2] = vol[3:, :Y - 1, 2:]
    assert np.array_equal(out, want)
    assert np.array_equal(out, O.nearest(vol, _shift(tx=2.0, ty=-1.0, tz=3.0), (X, Y, Z), pad=7.0))


# ---- against scipy ---------------------------------------------------------------------------------------------------
def test_oracle_against_scipy_order_1_planes():
    """per-label map_coordinates(order=1) + arg-max on the interior voxels where the two best memberships differ by more
    than 1e-6 (scipy's arithmetic order differs from trilinear_lerp's); at least 95 % of the interior voxels qualify"""
    from scipy import ndimage
    vol = np.random.RandomState(4).randint(0, 5, size=(11, 10, 9)).astype(np.float32)      # x = 9, y = 10, z = 11
    Z, Y, X = vol.shape
    A = _shift(0.31, 0.47, 0.23, 0.83, 0.91, 0.77)
    size = (10, 10, 13)
    c = O.coordinates(A, size)
    interior = (c[0] >= 0) & (c[0] <= X - 1) & (c[1] >= 0) & (c[1] <= Y - 1) & (c[2] >= 0) & (c[2] <= Z - 1)
    assert int(interior.sum()) > 800
    labels = np.unique(vol)
    planes = np.stack([ndimage.map_coordinates((vol == l).astype(np.float64), [c[2], c[1], c[0]], order=1) for l in labels])
    top = np.sort(planes, axis=0)
    clear = interior & (top[-1] - top[-2] > 1e-6)
    share = float(clear.sum()) / float(interior.sum())
    print('interior voxels {}, with a clear winner {} ({:.2%})'.format(int(interior.sum()), int(clear.sum()), share))
    assert share >= 0.95
    want = labels[np.argmax(planes, axis=0)]
    got = O.label_linear(vol, A, size)
    assert np.array_equal(got[clear], want[clear])
    _, mine = O.memberships(vol, A, size, pad=0.0)                    # the planes themselves agree to float32 rounding
    assert float(np.abs(mine[:, interior] - planes[:, interior]).max()) < 1e-6


# ---- the config key and the C ABI --------------------------------------------------------------------------------------
def test_validate_mask_interpolation():
    from segmentation3d.dataloader.dataset import validate_mask_interpolation
    assert validate_mask_interpolation('NN') == 'NN' and validate_mask_interpolation('LABEL_LINEAR') == 'LABEL_LINEAR'
    for bad in ('LINEAR', 'BSPLINE', 'nn', 'label_linear', '', None, 1, ['NN']):
        with pytest.raises(ValueError):
            validate_mask_interpolation(bad)


def test_the_two_entries_are_in_the_ctypes_table():
    from segmentation3d import _engine
    text = open(os.path.join(REPO, 'include', 'seg3d_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name, count in (('seg3d_resample_label', 12), ('seg3d_resample_label_deform', 19)):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;{]*?)\)\s*;', text, flags=re.S)
        assert m is not None, name
        assert len(m.group(1).split(',')) == count == len(_engine._SIGNATURES[name][1]), name
        assert name in _engine.symbols()
    assert _engine.lib().seg3d_abi_version() == 2
