"""The voxel-row accessor and the width dispatch of the multi-modality kernels (csrc/mc_device.h) at the two places the
other GPU tests are thin: bases one float past an aligned allocation (the only way to the <4, false> and <2, false>
instantiations of the gather and the intensity pass) and 5 <= M <= 8 (the runtime-width instantiation, whose fill and guard
rule lives in that header).  One property throughout: channel m of the M-channel call equals the M = 1 call on plane m, bit
for bit.  All widths cut their channels out of one 8-channel array, so the M = 1 reference of a plane is computed once.

Shapes: a crop of (X, Y, Z) = (37, 19, 13) is 9139 voxels -- two statistics chunks of 8192, the second partial -- and
leaves a partial 32 x 8 x 8 filter tile on every axis; the gather takes two boxes of that size out of a (41, 23, 17) volume."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 5, 8)
CROP = (13, 19, 37)                      # z, y, x
VOLUME = (17, 23, 41)
STARTS = ((0, 0, 0), (4, 4, 4))          # x, y, z


@functools.lru_cache(maxsize=None)
def _planes(shape, seed):
    return np.random.RandomState(seed).randn(*shape, 8).astype(np.float32) * 1.5 + 0.25


def _at(x, shifted, device):
    """x (numpy) on the device at an aligned base, or one float past one"""
    flat = torch.empty(x.size + int(shifted), dtype=torch.float32, device=device)[int(shifted):]
    t = flat.view(x.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert t.data_ptr() % 16 == (4 if shifted else 0)
    return t


def _empty(shape, shifted, device):
    return _at(np.full(shape, np.nan, np.float32), shifted, device)


def _equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# gather: modality 0 adaptive, 1 fixed with clip, the rest without a normaliser
# ---------------------------------------------------------------------------------------------------------------------
_NORMS = [{'type': 1, 'clip_sigma': 1.5}, {'type': 0, 'mean': 0.5, 'stddev': 1.25, 'clip': True}] + [None] * 6


def _gather(vol, norms, flip, shifted, device):
    from segmentation3d import _engine as E
    from segmentation3d.utils.image_tools import normalizer_params
    Z, Y, X, M = vol.shape
    bz, by, bx = CROP
    P = len(STARTS)
    src = _at(vol, shifted, device)
    out = _empty((P, bz, by, bx, M), shifted, device)
    starts = torch.tensor(STARTS, dtype=torch.int32, device=device)
    ws = torch.empty((E.query('seg3d_patch_stats_mc_doubles', bx, by, bz, P, M),), dtype=torch.float64, device=device)
    mean_std = torch.empty((P * M, 2), dtype=torch.float32, device=device)
    args = (E.ptr(src), E.ptr(starts), E.ptr(out), E.ptr(ws), E.ptr(mean_std), Z, Y, X, bx, by, bz, P, M,
            normalizer_params(norms, M))
    if flip:
        E.call('seg3d_patch_gather_normalize_mc_flip', *args, flip, E.stream_ptr())
    else:
        E.call('seg3d_patch_gather_normalize_mc', *args, E.stream_ptr())
    return out


@functools.lru_cache(maxsize=None)
def _gather_plane(m, flip):
    return _gather(_planes(VOLUME, 41)[..., m:m + 1], _NORMS[m:m + 1], flip, False, torch.device('cuda:0'))


@pytest.mark.parametrize('shifted', [False, True])
@pytest.mark.parametrize('flip', [0, 5])
@pytest.mark.parametrize('M', WIDTHS)
def test_gather_channel_equals_the_planar_gather(hip_device, M, flip, shifted):
    got = _gather(_planes(VOLUME, 41)[..., :M], _NORMS[:M], flip, shifted, hip_device)
    assert not bool(torch.isnan(got).any())
    for m in range(M):
        assert _equal(got[..., m], _gather_plane(m, flip)[..., 0]), m


# ---------------------------------------------------------------------------------------------------------------------
# resampler: an oblique destination grid that leaves the source on one side
# ---------------------------------------------------------------------------------------------------------------------
def _resample(src_np, linear, stride, shifted, device):
    """rows of `stride` floats per destination voxel; the floats past M keep their -3"""
    from segmentation3d import _engine as E
    from segmentation3d.utils import image_tools
    from test_multimodal import _oblique
    Zi, Yi, Xi, M = src_np.shape
    Zo, Yo, Xo = CROP
    src_frame = ((0.7, 1.1, 2.3), (-5.0, 3.0, 1.0), tuple(float(v) for v in np.ravel(_oblique(20.0))))
    dst_frame = ((0.9, 0.8, 1.7), (-2.0, 8.0, 6.0), tuple(float(v) for v in np.ravel(_oblique(-35.0))))
    A = np.ascontiguousarray(image_tools.index_affine(src_frame, dst_frame), dtype=np.float64)
    src = _at(src_np, shifted, device)
    rows = _at(np.full((Zo * Yo * Xo, stride), -3.0, np.float32), shifted, device)
    E.call('seg3d_resample_affine_mc', E.ptr(src), E.ptr(rows), M, stride, Xi, Yi, Zi, Xo, Yo, Zo,
           A.ctypes.data_as(ctypes.c_void_p), int(linear), 0.25, E.stream_ptr())
    assert bool((rows[:, M:] == -3.0).all())
    return rows[:, :M]


@functools.lru_cache(maxsize=None)
def _resample_plane(m, linear):
    return _resample(_planes(VOLUME, 42)[..., m:m + 1], linear, 1, False, torch.device('cuda:0'))


@pytest.mark.parametrize('layout', ['aligned', 'shifted', 'padded'])        # padded: aligned base, dst_stride = M + 1
@pytest.mark.parametrize('linear', [True, False])
@pytest.mark.parametrize('M', WIDTHS)
def test_resample_channel_equals_the_planar_resample(hip_device, M, linear, layout):
    got = _resample(_planes(VOLUME, 42)[..., :M], linear, M + (layout == 'padded'), layout == 'shifted', hip_device)
    inside = int((got[:, 0] != 0.25).sum())
    assert 0 < inside < got.shape[0]                                          # inside and padded voxels
    for m in range(M):
        assert _equal(got[:, m], _resample_plane(m, linear)[:, 0]), m


# ---------------------------------------------------------------------------------------------------------------------
# intensity: brightness, contrast, gamma and noise on in every modality
# ---------------------------------------------------------------------------------------------------------------------
_SEED = 20240607
_INTENSITY = [{'brightness': 0.8 + 0.06 * m, 'contrast': 1.3 - 0.07 * m, 'gamma': 0.7 + 0.1 * m, 'invert': bool(m & 1),
               'sigma': 0.05 + 0.01 * m} for m in range(8)]


def _intensity(x, params, shifted, device):
    from segmentation3d.utils.image_tools import augment_intensity_device
    return augment_intensity_device(_at(x, shifted, device), params, seed=_SEED)


@functools.lru_cache(maxsize=None)
def _intensity_plane(m, noise):
    """the M = 1 call on plane m with modality m's parameters; noise = False: sigma 0"""
    p = dict(_INTENSITY[m]) if noise else dict(_INTENSITY[m], sigma=0.0)
    return _intensity(_planes(CROP, 43)[..., m], [p], False, torch.device('cuda:0'))


@functools.lru_cache(maxsize=None)
def _noise_terms():
    """sigma_m n(voxel, m) of every modality: the noise-only pass over zeros, whose sum 0 + sigma n is the product itself"""
    return _intensity(np.zeros(CROP + (8,), np.float32), [{'sigma': p['sigma']} for p in _INTENSITY], False,
                      torch.device('cuda:0'))


@pytest.mark.parametrize('shifted', [False, True])
@pytest.mark.parametrize('M', WIDTHS)
def test_intensity_channel_equals_the_planar_pass(hip_device, M, shifted):
    """The noise of a voxel is a function of (seed, voxel, modality index) -- test_gpu_augment.py pins that -- so the
    M = 1 call on plane m, whose modality index is 0, draws channel 0's noise.  Channel 0 is therefore compared with the
    M = 1 call with all four transforms on; channel m >= 1 with the M = 1 call on plane m without noise plus modality m's
    noise term sigma_m n(voxel, m), one rounded float32 addition as in the kernel (no FMA contraction)."""
    x = _planes(CROP, 43)[..., :M]
    got = _intensity(x[..., 0] if M == 1 else x, _INTENSITY[:M], shifted, hip_device).view(CROP + (M,))
    assert _equal(_noise_terms()[..., 0] + _intensity_plane(0, False), _intensity_plane(0, True))
    assert _equal(got[..., 0], _intensity_plane(0, True))
    for m in range(1, M):
        assert _equal(got[..., m], _intensity_plane(m, False) + _noise_terms()[..., m]), m
    assert not _equal(got[..., 0], _intensity_plane(0, False))


# ---------------------------------------------------------------------------------------------------------------------
# blur and low-resolution simulation
# ---------------------------------------------------------------------------------------------------------------------
_SIGMAS = [2.0, 0.34, 0.5, 1.3, 1.0, 1.7, 0.8, 0.6]          # radii 6, 2, 2, 4, 3, 6, 3, 2
_ZOOMS = [0.5, 0.26, 0.99, 0.7, 0.4, 0.85, 0.3, 0.6]


def _filter(name, x, prm, shifted, device):
    from segmentation3d.utils import image_tools
    return getattr(image_tools, name)(_at(x, shifted, device), prm, out=_empty(x.shape, shifted, device))


@functools.lru_cache(maxsize=None)
def _filter_plane(name, m):
    prm = _SIGMAS if name == 'blur_device' else _ZOOMS
    return _filter(name, _planes(CROP, 44)[..., m], prm[m:m + 1], False, torch.device('cuda:0'))


@pytest.mark.parametrize('shifted', [False, True])
@pytest.mark.parametrize('M', WIDTHS)
@pytest.mark.parametrize('name', ['blur_device', 'lowres_device'])
def test_filter_channel_equals_the_planar_filter(hip_device, name, M, shifted):
    x = _planes(CROP, 44)[..., :M]
    prm = (_SIGMAS if name == 'blur_device' else _ZOOMS)[:M]
    got = _filter(name, x[..., 0] if M == 1 else x, prm, shifted, hip_device).view(CROP + (M,))
    assert not bool(torch.isnan(got).any())
    for m in range(M):
        assert _equal(got[..., m], _filter_plane(name, m)), m
