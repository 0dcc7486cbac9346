"""GPU side of the 'LABEL_LINEAR' label interpolation: seg3d_resample_label and
seg3d_resample_label_deform through image_tools, the data set and train().  Every comparison is bit equality of label maps
(int32 bit patterns of the float crops); there is no tolerance in this file.

Two references.  The COMPOSITION from existing operators: for every label of the volume in ascending order (with the padding
value in its sorted place) resample_device((src == l).float(), 'LINEAR', padding_value = 1 if l == pad else 0), then the
first maximum over the planes.  The numpy ORACLE of tests/label_interp_oracle.py (pinned on the CPU by
tests/test_label_interp.py), affine maps only.

Shapes are tiny: a 9 x 11 x 13 source (x, y, z), outputs 8 x 12 x 10 and 7 x 5 x 3 (odd sizes, one workgroup and a part of one)
and 16^3 (16 workgroups) for the deformed cases."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest
import torch

import label_interp_oracle as O
from conftest import PKG  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu

SRC = (13, 11, 9)                        # z, y, x
OUTS = {'8x12x10': (8, 12, 10), '7x5x3': (7, 5, 3)}          # x, y, z
EYE = tuple(np.eye(3).ravel())
_NP = {'float32': np.float32, 'uint8': np.uint8, 'int16': np.int16, 'int8': np.int8}


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _source(name):
    """float32 [Z, Y, X] label volumes.  random: labels drawn uniformly from {0, 1, 2, 5, 255} per voxel, so most
    neighbourhoods hold several labels; signed: the same with -3 for 255 (fits an int8); eight: (x + 2y + 4z) % 8, eight
    distinct taps in every neighbourhood"""
    if name == 'eight':
        z, y, x = np.meshgrid(np.arange(SRC[0]), np.arange(SRC[1]), np.arange(SRC[2]), indexing='ij')
        return ((x + 2 * y + 4 * z) % 8).astype(np.float32)
    labels = (0, 1, 2, 5, 255) if name == 'random' else (0, 1, 2, 5, -3)
    return np.random.RandomState(11).choice(np.array(labels, dtype=np.float32), size=SRC)


# (source, dtype): every dtype sees both kinds of source; int8 takes the labels that fit it
SOURCES = [('random', 'float32'), ('random', 'uint8'), ('random', 'int16'), ('signed', 'int8'), ('signed', 'int16'),
           ('eight', 'float32'), ('eight', 'uint8'), ('eight', 'int16'), ('eight', 'int8')]


def _frames(geometry, out_size):
    """(src_frame, dst_frame) of the affine cases"""
    if geometry == 'scale0.9':
        return ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), EYE), ((0.9, 0.9, 0.9), (0.21, 0.43, 0.37), EYE)
    if geometry == 'scale1.1':
        return ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), EYE), ((1.1, 1.1, 1.1), (-0.3, 0.15, 0.4), EYE)
    if geometry == 'aniso':               # thick slices, (1, 1, 3) mm, resampled to 1 mm
        return ((1.0, 1.0, 3.0), (0.0, 0.0, 0.0), EYE), ((1.0, 1.0, 1.0), (0.3, 0.6, 1.7), EYE)
    if geometry == 'outside':             # the first three x positions -- about a third of the output -- miss the buffer
        return ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), EYE), ((1.0, 1.0, 1.0), (-(out_size[0] / 3.0 + 0.7), 0.4, 0.6), EYE)
    raise ValueError(geometry)


GEOMETRIES = ('scale0.9', 'scale1.1', 'aniso', 'outside')
PADS = (0.0, 7.0)                         # 7 is among the labels of `eight` only


def _first_maximum(labels, planes):
    """label of the first maximum over the planes, spelled out: a later plane takes over only when strictly greater"""
    best = planes[0].clone()
    out = torch.full_like(best, float(labels[0]))
    for l, p in zip(labels[1:], planes[1:]):
        take = p > best
        best = torch.where(take, p, best)
        out = torch.where(take, torch.full_like(out, float(l)), out)
    return out


def _composition(src, src_frame, out_size, dst_frame, pad, **spatial):
    """the reference from existing operators; src a float32 device volume"""
    from segmentation3d.utils import image_tools
    labels = O.label_list(src.cpu().numpy(), pad)
    planes = [image_tools.resample_device((src == float(l)).float(), src_frame, out_size, dst_frame, 'LINEAR',
                                          padding_value=1.0 if float(l) == float(pad) else 0.0, **spatial) for l in labels]
    return _first_maximum(labels, planes)


@functools.lru_cache(maxsize=None)
def _affine_references(source, geometry, out_name, pad):
    """(composition on the device, numpy oracle as a device tensor): once per case, left alone"""
    from segmentation3d.utils import image_tools
    dev = torch.device('cuda:0')
    out_size = OUTS[out_name]
    src_frame, dst_frame = _frames(geometry, out_size)
    comp = _composition(torch.from_numpy(_source(source)).to(dev), src_frame, out_size, dst_frame, pad)
    oracle = O.label_linear(_source(source), image_tools.index_affine(src_frame, dst_frame), out_size, pad)
    return comp, torch.from_numpy(oracle).to(dev)


def _label_linear(src, src_frame, out_size, dst_frame, pad, **spatial):
    from segmentation3d.utils import image_tools
    return image_tools.resample_device(src, src_frame, out_size, dst_frame, 'LABEL_LINEAR', padding_value=pad, **spatial)


# ---------------------------------------------------------------------------------------------------------------------
# 1. affine: the fused launch against the composition and the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('out_name', sorted(OUTS))
@pytest.mark.parametrize('geometry', GEOMETRIES)
@pytest.mark.parametrize('source, dtype', SOURCES)
def test_fused_launch_equals_the_composition_and_the_oracle(hip_device, source, dtype, geometry, out_name):
    from segmentation3d.utils import image_tools
    out_size = OUTS[out_name]
    src_frame, dst_frame = _frames(geometry, out_size)
    src = torch.from_numpy(_source(source).astype(_NP[dtype])).to(hip_device)
    assert torch.equal(src.float().cpu(), torch.from_numpy(_source(source)))          # the labels fit the type
    missed = ~O.inside(O.coordinates(image_tools.index_affine(src_frame, dst_frame), out_size), SRC)
    if geometry == 'outside':
        assert 0.25 < float(missed.mean()) < 0.5
    for pad in PADS:
        comp, oracle = _affine_references(source, geometry, out_name, pad)
        got = _label_linear(src, src_frame, out_size, dst_frame, pad)
        assert got.dtype == torch.float32 and tuple(got.shape) == out_size[::-1]
        differs = int((_bits(got) != _bits(comp)).sum()), int((_bits(got) != _bits(oracle)).sum())
        print('{} {} {} {} pad {}: voxels differing from composition / oracle: {}'.format(source, dtype, geometry, out_name,
                                                                                         pad, differs))
        assert torch.equal(_bits(got), _bits(comp))
        assert torch.equal(_bits(got), _bits(oracle))
        if source != 'eight' and pad == 7.0:   # 7 is no label of these volumes: it appears exactly where c is outside
            assert np.array_equal((got == 7.0).cpu().numpy(), missed)


def test_the_cases_are_not_trivial(hip_device):
    """most voxels of the random source have a mixed neighbourhood, and the vote differs from 'NN' there"""
    from segmentation3d.utils import image_tools
    out_size = OUTS['8x12x10']
    src_frame, dst_frame = _frames('scale0.9', out_size)
    src = torch.from_numpy(_source('random')).to(hip_device)
    got = _label_linear(src, src_frame, out_size, dst_frame, 0.0)
    nn = image_tools.resample_device(src, src_frame, out_size, dst_frame, 'NN', 0.0)
    assert 0.02 < float((got != nn).float().mean()) < 0.9
    _, planes = O.memberships(_source('random'), image_tools.index_affine(src_frame, dst_frame), out_size)
    assert float((planes.max(0) < 0.5).mean()) > 0.1          # voxels where no label reaches 0.5: arg-max, not a threshold


def test_the_exact_tie(hip_device):
    """[1, 2] and [2, 1] sampled at c = 0.5: both memberships are 0.5 and the smaller label wins; 'NN' rounds half up"""
    from segmentation3d.utils import image_tools
    src_frame, dst_frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), EYE), ((1.0, 1.0, 1.0), (0.5, 0.0, 0.0), EYE)
    for row, nn in (([1, 2], 2.0), ([2, 1], 1.0)):
        for dtype in ('float32', 'uint8', 'int16', 'int8'):
            src = torch.tensor(row, dtype=getattr(torch, dtype), device=hip_device).view(1, 1, 2)
            assert _label_linear(src, src_frame, (1, 1, 1), dst_frame, 0.0).tolist() == [[[1.0]]]
            assert image_tools.resample_device(src, src_frame, (1, 1, 1), dst_frame, 'NN', 0.0).tolist() == [[[nn]]]
        comp = _composition(torch.tensor(row, dtype=torch.float32, device=hip_device).view(1, 1, 2), src_frame, (1, 1, 1),
                            dst_frame, 0.0)
        assert comp.tolist() == [[[1.0]]]


# ---------------------------------------------------------------------------------------------------------------------
# 2. rotation + elastic field + mirror: against the device composition
# ---------------------------------------------------------------------------------------------------------------------
WARP_OUT = (16, 16, 16)
WARP_FRAMES = (((1.0, 1.1, 0.9), (-4.0, 2.0, 7.0), EYE), ((0.55, 0.6, 0.65), (-3.6, 2.8, 7.9), EYE))
GRID_MM = 4.0


@functools.lru_cache(maxsize=None)
def _control(zero=False):
    from segmentation3d.utils.image_tools import bspline_control_dims
    gx, gy, gz = bspline_control_dims(WARP_OUT, WARP_FRAMES[1][0], GRID_MM)
    ctrl = np.random.RandomState(5).uniform(-0.6, 0.6, size=(gz, gy, gx, 3)).astype(np.float32)
    return np.zeros_like(ctrl) if zero else ctrl


def _warp(device, zero=False, deform=True):
    """rotation + mirror mask 5 (x and z) and, with `deform`, the elastic field (all zeros with `zero`)"""
    spatial = {'rotation': (0.2, -0.15, 0.3), 'mirror': (True, False, True)}
    if deform:
        spatial['deform'] = (torch.from_numpy(_control(zero)).to(device), GRID_MM)
    return spatial


@pytest.mark.parametrize('source, dtype', [('random', 'float32'), ('random', 'uint8'), ('eight', 'float32'), ('eight', 'uint8')])
def test_deformed_launch_equals_the_composition(hip_device, source, dtype):
    as_float = torch.from_numpy(_source(source)).to(hip_device)
    src = torch.from_numpy(_source(source).astype(_NP[dtype])).to(hip_device)
    for pad in PADS:
        comp = _composition(as_float, WARP_FRAMES[0], WARP_OUT, WARP_FRAMES[1], pad, **_warp(hip_device))
        got = _label_linear(src, WARP_FRAMES[0], WARP_OUT, WARP_FRAMES[1], pad, **_warp(hip_device))
        print('{} {} pad {}: {} voxels differ, {:.1%} padded'.format(source, dtype, pad, int((_bits(got) != _bits(comp)).sum()),
                                                                   float((got == pad).float().mean())))
        assert torch.equal(_bits(got), _bits(comp))
        plain = _label_linear(src, WARP_FRAMES[0], WARP_OUT, WARP_FRAMES[1], pad, **_warp(hip_device, deform=False))
        assert not torch.equal(_bits(got), _bits(plain))                     # the field moves labels


@pytest.mark.parametrize('dtype', ['float32', 'uint8'])
def test_zero_control_grid_equals_the_affine_entry(hip_device, dtype):
    src = torch.from_numpy(_source('random').astype(_NP[dtype])).to(hip_device)
    zero = _label_linear(src, WARP_FRAMES[0], WARP_OUT, WARP_FRAMES[1], 7.0, **_warp(hip_device, zero=True))
    affine = _label_linear(src, WARP_FRAMES[0], WARP_OUT, WARP_FRAMES[1], 7.0, **_warp(hip_device, deform=False))
    assert torch.equal(_bits(zero), _bits(affine))
    assert 0 < int((affine == 7.0).sum()) < affine.numel()


# ---------------------------------------------------------------------------------------------------------------------
# 3. properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('source, dtype', [('random', 'float32'), ('random', 'uint8'), ('signed', 'int8'), ('eight', 'int16')])
def test_properties(hip_device, source, dtype):
    from segmentation3d.utils import image_tools
    vol = _source(source)
    src = torch.from_numpy(vol.astype(_NP[dtype])).to(hip_device)
    unit = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), EYE)
    size = SRC[::-1]
    # identity returns the source bit for bit
    same = _label_linear(src, unit, size, unit, 7.0)
    assert torch.equal(_bits(same), _bits(torch.from_numpy(vol).to(hip_device)))
    # an integer translation equals 'NN', padding included
    moved = ((1.0, 1.0, 1.0), (2.0, -1.0, 3.0), EYE)
    got = _label_linear(src, unit, size, moved, 7.0)
    assert torch.equal(_bits(got), _bits(image_tools.resample_device(src, unit, size, moved, 'NN', 7.0)))
    assert 0 < int((got == 7.0).sum()) < got.numel()
    # every output value is a source label or the padding value; two runs are bit-equal
    allowed = set(np.unique(vol).tolist()) | {-9.0}
    for spatial in ({}, _warp(hip_device)):
        a = _label_linear(src, WARP_FRAMES[0], WARP_OUT, WARP_FRAMES[1], -9.0, **spatial)
        b = _label_linear(src, WARP_FRAMES[0], WARP_OUT, WARP_FRAMES[1], -9.0, **spatial)
        assert set(torch.unique(a).tolist()) <= allowed
        assert torch.equal(_bits(a), _bits(b))


def test_mc_and_crop_entries_take_the_mode(hip_device):
    """resample_device_mc with M = 1 into a given destination, and crop_image_device(_mc), are the same launch"""
    from segmentation3d.utils import image_tools
    src = torch.from_numpy(_source('random').astype(np.uint8)).to(hip_device)
    want = _label_linear(src, WARP_FRAMES[0], WARP_OUT, WARP_FRAMES[1], 0.0, **_warp(hip_device))
    out = torch.full(WARP_OUT[::-1] + (1,), 3.25, dtype=torch.float32, device=hip_device)
    got = image_tools.resample_device_mc(src.unsqueeze(3), WARP_FRAMES[0], WARP_OUT, WARP_FRAMES[1], 'LABEL_LINEAR', 0.0,
                                         out=out, **_warp(hip_device))
    assert got.data_ptr() == out.data_ptr() and torch.equal(_bits(out[..., 0]), _bits(want))
    spacing = WARP_FRAMES[1][0]
    center = [WARP_FRAMES[1][1][a] + (WARP_OUT[a] - 1) * spacing[a] / 2.0 for a in range(3)]
    crop = image_tools.crop_image_device(src, WARP_FRAMES[0], center, WARP_OUT, spacing, 'LABEL_LINEAR', **_warp(hip_device))
    origin = image_tools.crop_origin(center, WARP_OUT, spacing)
    direct = _label_linear(src, WARP_FRAMES[0], WARP_OUT, (spacing, origin, EYE), 0.0, **_warp(hip_device))
    assert torch.equal(_bits(crop), _bits(direct))
    # the Image3d wrappers: resample, resample_spacing and crop_image upload float32 and run the same launch
    from segmentation3d.utils.image3d import Image3d
    image = Image3d(_source('random'), *WARP_FRAMES[0])
    reference = Image3d(np.zeros(WARP_OUT[::-1], dtype=np.float32), *WARP_FRAMES[1])
    plain = _label_linear(src, WARP_FRAMES[0], WARP_OUT, WARP_FRAMES[1], 0.0).cpu().numpy()
    assert np.array_equal(image_tools.resample(image, reference, 'LABEL_LINEAR').array, plain)
    cropped = image_tools.crop_image(image, center, WARP_OUT, spacing, 'LABEL_LINEAR')
    want = image_tools.crop_image_device(src, WARP_FRAMES[0], center, WARP_OUT, spacing, 'LABEL_LINEAR').cpu().numpy()
    assert np.array_equal(cropped.array, want)
    spaced = image_tools.resample_spacing(image, [0.8, 0.9, 0.7], 1, 'LABEL_LINEAR')
    assert set(np.unique(spaced.array).tolist()) <= {0.0, 1.0, 2.0, 5.0, 255.0} and spaced.array.shape[0] > SRC[0]


# ---------------------------------------------------------------------------------------------------------------------
# 4. error paths
# ---------------------------------------------------------------------------------------------------------------------
def test_error_paths(hip_device):
    from segmentation3d import _engine as E
    from segmentation3d.utils import image_tools
    unit = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), EYE)
    vol = torch.from_numpy(_source('random')).to(hip_device)
    two = torch.stack([vol, vol], dim=3)
    with pytest.raises(ValueError):                                            # M = 2
        image_tools.resample_device_mc(two, unit, (4, 4, 4), unit, 'LABEL_LINEAR')
    with pytest.raises(ValueError):
        image_tools.resample_device(vol, unit, (4, 4, 4), unit, 'LABEL_LINEAR', prefiltered=True)
    with pytest.raises(ValueError):                                            # a typed source must be contiguous
        image_tools.resample_device(two.to(torch.uint8)[..., 0], unit, (4, 4, 4), unit, 'LABEL_LINEAR')
    with pytest.raises(ValueError):
        image_tools.resample_device(vol.double(), unit, (4, 4, 4), unit, 'LABEL_LINEAR')
    with pytest.raises(ValueError, match='Unsupported interpolation type.'):
        image_tools.resample_device(vol, unit, (4, 4, 4), unit, 'LABEL_NEAREST')
    # the C ABI: dtype code 3 (and an unknown code), null pointers, bad dims -- nothing is launched
    Zi, Yi, Xi = SRC
    src = torch.zeros(SRC, dtype=torch.int32, device=hip_device)
    dst = torch.full((4, 4, 4), 1.5, dtype=torch.float32, device=hip_device)
    A = np.ascontiguousarray(np.eye(3, 4), dtype=np.float64)
    a_ptr = A.ctypes.data_as(ctypes.c_void_p)
    ctrl = torch.zeros((5, 5, 5, 3), dtype=torch.float32, device=hip_device)
    L, t = np.eye(3).ravel().copy(), np.array([0.01, 0.01, 0.01])
    tail = (L.ctypes.data_as(ctypes.c_void_p), E.ptr(ctrl), 5, 5, 5, t.ctypes.data_as(ctypes.c_void_p), 0, E.stream_ptr())
    lib = E.lib()
    for code in (3, 9):
        rc = lib.seg3d_resample_label(E.ptr(src), code, E.ptr(dst), Xi, Yi, Zi, 4, 4, 4, a_ptr, 0.0, E.stream_ptr())
        assert rc == -3 and 'seg3d_resample_label' in E.last_error() and str(code) in E.last_error()
        rc = lib.seg3d_resample_label_deform(E.ptr(src), code, E.ptr(dst), Xi, Yi, Zi, 4, 4, 4, a_ptr, 0.0, *tail)
        assert rc == -3 and 'seg3d_resample_label_deform' in E.last_error()
    ok = lib.seg3d_resample_label(E.ptr(vol), 4, E.ptr(dst), Xi, Yi, Zi, 4, 4, 4, a_ptr, 0.0, E.stream_ptr())
    assert ok == 0
    torch.cuda.synchronize()
    assert torch.equal(dst, vol[:4, :4, :4])
    dst.fill_(1.5)
    for args in ((None, 4, E.ptr(dst), Xi, Yi, Zi, 4, 4, 4, a_ptr), (E.ptr(vol), 4, None, Xi, Yi, Zi, 4, 4, 4, a_ptr),
                 (E.ptr(vol), 4, E.ptr(dst), Xi, Yi, Zi, 4, 4, 4, None), (E.ptr(vol), 4, E.ptr(dst), 0, Yi, Zi, 4, 4, 4, a_ptr),
                 (E.ptr(vol), 4, E.ptr(dst), Xi, Yi, Zi, 4, -1, 4, a_ptr)):
        assert lib.seg3d_resample_label(*args, 0.0, E.stream_ptr()) not in (0, -3)
        assert lib.seg3d_resample_label_deform(*args, 0.0, *tail) not in (0, -3)
    assert lib.seg3d_resample_label_deform(E.ptr(vol), 4, E.ptr(dst), Xi, Yi, Zi, 4, 4, 4, a_ptr, 0.0, None, *tail[1:]) != 0
    assert lib.seg3d_resample_label_deform(E.ptr(vol), 4, E.ptr(dst), Xi, Yi, Zi, 4, 4, 4, a_ptr, 0.0, *tail[:6], 8,
                                           E.stream_ptr()) != 0              # mirror mask outside 0..7
    torch.cuda.synchronize()
    assert bool((dst == 1.5).all())


# ---------------------------------------------------------------------------------------------------------------------
# 5. the data set
# ---------------------------------------------------------------------------------------------------------------------
SHAPE = (18, 20, 24)                     # z, y, x: cases of 24 x 20 x 18
FRAME = ((1.0, 1.1, 0.9), (-4.0, 2.0, 7.0), EYE)
AUG = {'rotation_deg': [15.0, 10.0, 20.0], 'rotation_prob': 1.0, 'elastic_grid_mm': 8.0, 'elastic_magnitude_mm': [0.5, 1.0],
       'elastic_prob': 1.0}
ORDER = [0, 1, 1, 0, 1, 0]


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    """two cases: an int16 image, a five-label mask (blocks of 3 voxels with a fifth of the voxels re-drawn, so that
    boundaries and mixed neighbourhoods are everywhere) and its two-label version for train()"""
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.image_io import write_image
    root = tmp_path_factory.mktemp('label_interp')
    rng = np.random.RandomState(21)
    five, two = [], []
    for k in range(2):
        d = root / 'case{}'.format(k)
        d.mkdir()
        coarse = rng.randint(0, 5, size=tuple((n + 2) // 3 for n in SHAPE))
        mask = np.kron(coarse, np.ones((3, 3, 3), dtype=np.int64))[:SHAPE[0], :SHAPE[1], :SHAPE[2]]
        noise = rng.rand(*SHAPE) < 0.2
        mask = np.where(noise, rng.randint(0, 5, size=SHAPE), mask).astype(np.uint8)
        image = (rng.randint(-200, 200, size=SHAPE) + 300 * (mask % 2).astype(np.int64)).astype(np.int16)
        write_image(Image3d(image, *FRAME), str(d / 'org.mha'))
        write_image(Image3d(mask, *FRAME), str(d / 'seg5.mha'))
        write_image(Image3d((mask % 2).astype(np.uint8), *FRAME), str(d / 'seg2.mha'))
        five += [str(d / 'org.mha'), str(d / 'seg5.mha')]
        two += [str(d / 'org.mha'), str(d / 'seg2.mha')]
    (root / 'five.txt').write_text('2\n' + '\n'.join(five) + '\n')
    (root / 'two.txt').write_text('2\n' + '\n'.join(two) + '\n')
    return root


def _dataset(toy, device, **kwargs):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    interp = kwargs.pop('interp', 'LINEAR')
    return SegmentationDataset(str(toy / 'five.txt'), 5, [1.0, 1.0, 1.0], [16, 16, 16], 'MASK', [2, 2, 2], [0.9, 1.1], interp,
                               [AdaptiveNormalizer()], device=device, random_mirror_axes=('x', 'y', 'z'), augmentation=AUG,
                               **kwargs)


def _draw(ds, seed=17):
    """six seeded samples on the host + numpy's global state afterwards"""
    np.random.seed(seed)
    out = []
    for i in ORDER:
        im, seg, frame, name = ds.sample(i)
        out.append((im.contiguous().cpu(), seg.cpu(), frame, name))
    return out, np.random.get_state()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _direct_masks(ds, device, seed=17):
    """the six mask crops from crop_image_device(.., 'LABEL_LINEAR', ..) with each sample's geometry: the sample's draws are
    repeated in its order, and the mask volume is the float32 label map whatever the data set keeps"""
    from segmentation3d.utils import image_tools
    np.random.seed(seed)
    out = []
    for i in ORDER:
        case = ds.case(i)
        center, crop_spacing = ds.sample_crop_geometry(i)
        mirror = ds.sample_mirror()
        aug = ds.sample_augmentation(crop_spacing)
        ds.sample_resolution_augmentation()
        assert aug['rotation'] is not None and aug['control'] is not None
        deform = (torch.from_numpy(aug['control']).to(device), AUG['elastic_grid_mm'])
        seg = torch.from_numpy(case.seg_host.astype(np.float32)).to(device)
        out.append(image_tools.crop_image_device(seg, case.seg_frame, center, ds.crop_size, crop_spacing, 'LABEL_LINEAR',
                                                 mirror=mirror, rotation=aug['rotation'], deform=deform).cpu())
    return out


def _one_case_budget(toy_case_bytes):
    return (toy_case_bytes + 0.5) / 1e9


_VARIANTS = {
    'fp32': {},
    'compact': {'resident_storage': 'compact'},
    'budget': {'resident_storage': 'compact', 'resident_budget_gb': _one_case_budget(int(np.prod(SHAPE)) * 3)},
    'bspline': {'interp': 'BSPLINE'},
}


@pytest.mark.parametrize('variant', sorted(_VARIANTS))
def test_dataset_label_linear_against_the_nn_run(hip_device, toy, variant):
    kwargs = _VARIANTS[variant]
    nn, state_nn = _draw(_dataset(toy, hip_device, **kwargs))
    ds = _dataset(toy, hip_device, mask_interpolation='LABEL_LINEAR', **kwargs)
    assert ds.mask_interpolation == 'LABEL_LINEAR'
    got, state = _draw(ds)
    assert _same_state(state, state_nn)
    direct = _direct_masks(ds, hip_device)
    changed = 0
    for (im, seg, frame, name), (im_nn, seg_nn, frame_nn, name_nn), want in zip(got, nn, direct):
        assert torch.equal(_bits(im), _bits(im_nn)) and name == name_nn
        assert np.array_equal(frame.view(np.int32), frame_nn.view(np.int32))
        assert seg.dtype == torch.float32 and tuple(seg.shape) == (1, 16, 16, 16)
        assert torch.equal(_bits(seg[0]), _bits(want))
        assert set(torch.unique(seg).tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0}
        changed += int((seg != seg_nn).sum())
    assert changed > 0                                                        # only the mask differs, and it does
    if variant in ('compact', 'budget'):
        assert ds.case(0).seg_host.dtype == np.uint8
        assert (ds.case(1).seg_pinned if ds.case(1).staged else ds.case(1).seg).dtype == torch.uint8
    if variant == 'budget':
        assert not ds.case(0).staged and ds.case(1).staged and ds.num_staged() == 1


def test_dataset_default_is_the_nn_data_set(hip_device, toy, monkeypatch):
    from segmentation3d import _engine as E
    from segmentation3d.dataloader.dataset import SegmentationDataset
    want, state = _draw(_dataset(toy, hip_device))
    calls = []
    real = E.call
    monkeypatch.setattr(E, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    got, state_kw = _draw(_dataset(toy, hip_device, mask_interpolation='NN'))
    assert _same_state(state, state_kw)
    for (im, seg, frame, name), (im_w, seg_w, frame_w, name_w) in zip(got, want):
        assert torch.equal(_bits(im), _bits(im_w)) and torch.equal(_bits(seg), _bits(seg_w)) and name == name_w
        assert np.array_equal(frame.view(np.int32), frame_w.view(np.int32))
    assert not [c for c in calls if 'resample_label' in c]                    # the default launches what it always did
    assert [c for c in calls if 'resample' in c] == ['seg3d_resample_deform_mc', 'seg3d_resample_deform_mc'] * len(ORDER)
    with pytest.raises(ValueError):
        _dataset(toy, hip_device, mask_interpolation='LINEAR')
    assert SegmentationDataset.__init__.__defaults__[-1] == 'NN'


# ---------------------------------------------------------------------------------------------------------------------
# 6. train()
# ---------------------------------------------------------------------------------------------------------------------
_CFG = '''
from easydict import EasyDict as edict
from segmentation3d.utils.normalizer import AdaptiveNormalizer
__C = edict()
cfg = __C
__C.general = {{}}
__C.general.imseg_list = '{train}'
__C.general.save_dir = '{save}'
__C.general.model_scale = 'coarse'
__C.general.resume_epoch = -1
__C.general.num_gpus = 1
__C.general.seed = 0
__C.dataset = {{}}
__C.dataset.num_classes = 2
__C.dataset.spacing = [1.0, 1.0, 1.0]
__C.dataset.crop_size = [16, 16, 16]
__C.dataset.sampling_method = 'GLOBAL'
__C.dataset.random_translation = [2, 2, 2]
__C.dataset.random_scale = [0.9, 1.1]
__C.dataset.interpolation = 'LINEAR'
__C.dataset.mask_interpolation = 'LABEL_LINEAR'
__C.dataset.crop_normalizers = [AdaptiveNormalizer()]
__C.loss = {{}}
__C.loss.name = 'DiceCE'
__C.loss.obj_weight = [1.0, 1.0]
__C.loss.focal_gamma = 2
__C.net = {{}}
__C.net.name = 'vnet'
__C.train = {{}}
__C.train.epochs = 2
__C.train.batchsize = 2
__C.train.num_threads = 0
__C.train.lr = 1e-3
__C.train.betas = (0.9, 0.999)
__C.train.save_epochs = 100
__C.train.use_graph = False
__C.validation = {{}}
__C.validation.imseg_list = '{train}'
__C.validation.crops_per_case = 2
__C.validation.seed = 5
__C.validation.ema = 0.5
__C.validation.save_best = False
'''


def test_train_reads_the_key(hip_device, toy, monkeypatch):
    """two eager steps of vnet(1, 2) on 16^3 crops with dataset.mask_interpolation = 'LABEL_LINEAR': the run's data set and
    its validator's held-out data set carry the mode, and the held-out masks are the direct calls"""
    from segmentation3d import _engine as E
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import train
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils import image_tools
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    save = toy / 'run'
    os.makedirs(str(save), exist_ok=True)
    (save / 'cfg.py').write_text(_CFG.format(train=str(toy / 'two.txt'), save=str(save)))
    calls = []
    real = E.call
    monkeypatch.setattr(E, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    random.seed(0)
    try:
        step = train(str(save / 'cfg.py'))
    finally:
        _ops.set_activation_dtype('fp32')
    log = (save / 'coarse' / 'train_log.txt').read_text().strip().splitlines()
    assert len([l for l in log if 'train_loss' in l]) == 2 and [l for l in log if 'val_dice: ' in l]
    # 4 held-out crops + 2 batches of 2 training crops, every mask through the new entry and none through 'NN'
    assert calls.count('seg3d_resample_label') == 8
    assert calls.count('seg3d_resample_affine_mc') == 8
    masks = step.validator.masks
    assert tuple(masks.shape) == (4, 1, 16, 16, 16)
    ds = SegmentationDataset(str(toy / 'two.txt'), 2, [1.0, 1.0, 1.0], [16, 16, 16], 'GLOBAL', [0, 0, 0], [1, 1], 'LINEAR',
                             [AdaptiveNormalizer()], device=hip_device)
    state = np.random.get_state()
    np.random.seed(5)
    try:
        k = 0
        for i in range(2):
            case = ds.case(i)
            seg = torch.from_numpy(case.seg_host.astype(np.float32)).to(hip_device)
            for _ in range(2):
                center, crop_spacing = ds.sample_crop_geometry(i)
                want = image_tools.crop_image_device(seg, case.seg_frame, center, ds.crop_size, crop_spacing, 'LABEL_LINEAR')
                assert torch.equal(_bits(masks[k, 0]), _bits(want)), k
                k += 1
    finally:
        np.random.set_state(state)
