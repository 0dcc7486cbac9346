"""Compact resident training cases on the GPU.  One property throughout: the typed call on
integer data equals the float call on the same values converted to float, compared as int32 bit patterns -- no tolerance
anywhere.  Kernel shapes are those of tests/test_gpu_mc_rows.py: a (13, 19, 37) crop out of a (17, 23, 41) volume, placed so
that part of it lies outside; the data are random integers that include both ends of their type's range.

The toy data sets: all cases of a data set share one M, so the three kinds of case the feature distinguishes make two sets --
`single` (M = 1): two cases with an int16 .mha image and a uint8 mask (a) and one with a float32 image (c);
`nifti2` (M = 2): three cases, each one 4-D int16 NIfTI (b)."""
import ctypes
import functools
import os
import random
import struct

import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu

CROP = (13, 19, 37)                      # z, y, x
VOLUME = (17, 23, 41)
PAD = -3.5
_NP = {'int16': np.int16, 'uint8': np.uint8, 'int8': np.int8}
# int16 at every width; uint8 and int8 at M = 1 and M = 3
TYPED = [('int16', M) for M in (1, 2, 3, 4, 5, 8)] + [(d, M) for d in ('uint8', 'int8') for M in (1, 3)]


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _integers(dtype):
    """[Z, Y, X, 8] random integers of `dtype`, both ends of the range present in every channel"""
    info = np.iinfo(_NP[dtype])
    a = np.random.RandomState(len(dtype) + info.bits).randint(info.min, info.max + 1, size=VOLUME + (8,)).astype(_NP[dtype])
    a[0, 0, 0, :], a[-1, -1, -1, :], a[8, 11, 20, :] = info.min, info.max, info.max
    a[8, 11, 21, :] = info.min
    return a


def _at(x, shifted, device):
    """x (numpy) on the device at an aligned base, or one ELEMENT past one"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    flat = torch.empty(x.size + int(shifted), dtype=t.dtype, device=device)[int(shifted):]
    dev = flat.view(x.shape)
    dev.copy_(t)
    assert dev.data_ptr() % 16 == (x.dtype.itemsize if shifted else 0) and dev.is_contiguous()
    return dev


def _oblique(deg):
    a = np.deg2rad(deg)
    return tuple(float(v) for v in np.ravel([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]))


SRC_FRAME = ((0.7, 1.1, 2.3), (-5.0, 3.0, 1.0), _oblique(20.0))
DST_FRAME = ((0.9, 0.8, 1.7), (-2.0, 8.0, 6.0), _oblique(-35.0))
GRID_MM = 8.0


@functools.lru_cache(maxsize=None)
def _control():
    from segmentation3d.utils.image_tools import bspline_control_dims
    gx, gy, gz = bspline_control_dims(CROP[::-1], DST_FRAME[0], GRID_MM)
    return np.random.RandomState(5).uniform(-1.2, 1.2, size=(gz, gy, gx, 3)).astype(np.float32)


def _spatial(geometry, device):
    """affine: nothing; warped: rotation + elastic field + x / z mirror"""
    if geometry == 'affine':
        return {}
    return {'rotation': (0.2, -0.15, 0.3), 'mirror': (True, False, True),
            'deform': (torch.from_numpy(_control()).to(device), GRID_MM)}


def _resample(src, interp, geometry, out=None):
    from segmentation3d.utils import image_tools
    return image_tools.resample_device_mc(src, SRC_FRAME, CROP[::-1], DST_FRAME, interp, PAD, out=out,
                                          **_spatial(geometry, src.device))


@functools.lru_cache(maxsize=None)
def _float_reference(dtype, M, interp, geometry):
    """the float call on the converted values, aligned base: computed once per case and left alone"""
    src = _at(_integers(dtype)[..., :M].astype(np.float32), False, torch.device('cuda:0'))
    return _resample(src, interp, geometry)


@pytest.mark.parametrize('shifted', [False, True])
@pytest.mark.parametrize('geometry', ['affine', 'warped'])
@pytest.mark.parametrize('interp', ['LINEAR', 'NN'])
@pytest.mark.parametrize('dtype, M', TYPED)
def test_typed_resample_equals_the_float_resample(hip_device, dtype, M, interp, geometry, shifted):
    """the shifted base reaches the non-vector instantiations at M = 2 and M = 4"""
    got = _resample(_at(_integers(dtype)[..., :M], shifted, hip_device), interp, geometry)
    want = _float_reference(dtype, M, interp, geometry)
    assert got.dtype == torch.float32 and tuple(got.shape) == CROP + (M,)
    inside = int((want[..., 0] != PAD).sum())
    assert 0 < inside < want[..., 0].numel()                          # inside and padded voxels
    assert torch.equal(_bits(got), _bits(want))


def test_typed_resample_into_a_batch_slot(hip_device):
    batch = torch.full((2,) + CROP + (4,), 7.25, dtype=torch.float32, device=hip_device)
    got = _resample(_at(_integers('int16')[..., :4], False, hip_device), 'LINEAR', 'warped', out=batch[1])
    assert got.data_ptr() == batch[1].data_ptr()
    assert torch.equal(_bits(batch[1]), _bits(_float_reference('int16', 4, 'LINEAR', 'warped')))
    assert bool((batch[0] == 7.25).all())


def _rows(entry, src, code, M, stride, linear, device):
    """the C entry directly: rows of `stride` floats per destination voxel, the floats past M keep their -3"""
    from segmentation3d import _engine as E
    from segmentation3d.utils import image_tools
    Zi, Yi, Xi = VOLUME
    Zo, Yo, Xo = CROP
    A = np.ascontiguousarray(image_tools.index_affine(SRC_FRAME, DST_FRAME), dtype=np.float64)
    rows = torch.full((Zo * Yo * Xo, stride), -3.0, dtype=torch.float32, device=device)
    head = (E.ptr(src),) if code is None else (E.ptr(src), code)
    E.call(entry, *head, E.ptr(rows), M, stride, Xi, Yi, Zi, Xo, Yo, Zo, A.ctypes.data_as(ctypes.c_void_p), int(linear), PAD,
           E.stream_ptr())
    assert bool((rows[:, M:] == -3.0).all())
    return rows[:, :M]


@pytest.mark.parametrize('dtype, code, M', [('int16', 2, 2), ('int16', 2, 4), ('int16', 2, 5), ('uint8', 1, 3), ('int8', 0, 1)])
@pytest.mark.parametrize('linear', [True, False])
def test_typed_entry_with_a_padded_destination(hip_device, dtype, code, M, linear):
    """dst_stride = M + 1 through the C entry; src_dtype = 4 is the float entry"""
    x = _integers(dtype)[..., :M]
    want = _rows('seg3d_resample_affine_mc', _at(x.astype(np.float32), False, hip_device), None, M, M + 1, linear, hip_device)
    got = _rows('seg3d_resample_affine_typed_mc', _at(x, False, hip_device), code, M, M + 1, linear, hip_device)
    assert torch.equal(_bits(got), _bits(want))
    as_float = _rows('seg3d_resample_affine_typed_mc', _at(x.astype(np.float32), False, hip_device), 4, M, M + 1, linear,
                     hip_device)
    assert torch.equal(_bits(as_float), _bits(want))


@pytest.mark.parametrize('code', [3, 7])
def test_unsupported_source_codes(hip_device, code):
    from segmentation3d import _engine as E
    src = torch.zeros(VOLUME + (1,), dtype=torch.int32, device=hip_device)
    dst = torch.full(CROP + (1,), 1.5, dtype=torch.float32, device=hip_device)
    A = np.ascontiguousarray(np.eye(3, 4), dtype=np.float64)
    Zi, Yi, Xi = VOLUME
    Zo, Yo, Xo = CROP
    common = (Xi, Yi, Zi, Xo, Yo, Zo, A.ctypes.data_as(ctypes.c_void_p), 1, 0.0)
    rc = E.lib().seg3d_resample_affine_typed_mc(E.ptr(src), code, E.ptr(dst), 1, 1, *common, E.stream_ptr())
    assert rc == -3 and 'seg3d_resample_affine_typed_mc' in E.last_error() and str(code) in E.last_error()
    ctrl = torch.zeros((5, 5, 5, 3), dtype=torch.float32, device=hip_device)
    L, t = np.eye(3).ravel().copy(), np.array([0.01, 0.01, 0.01])
    rc = E.lib().seg3d_resample_deform_typed_mc(E.ptr(src), code, E.ptr(dst), 1, 1, *common,
                                                L.ctypes.data_as(ctypes.c_void_p), E.ptr(ctrl), 5, 5, 5,
                                                t.ctypes.data_as(ctypes.c_void_p), 0, E.stream_ptr())
    assert rc == -3 and 'seg3d_resample_deform_typed_mc' in E.last_error()
    torch.cuda.synchronize()
    assert bool((dst == 1.5).all())                                   # nothing was launched


def test_sources_that_are_refused(hip_device):
    from segmentation3d.utils import image_tools
    i16 = _at(_integers('int16')[..., :2], False, hip_device)
    with pytest.raises(ValueError):
        _resample(i16, 'BSPLINE', 'affine')
    with pytest.raises(ValueError):
        _resample(i16.double(), 'LINEAR', 'affine')
    with pytest.raises(ValueError):
        _resample(i16.int(), 'NN', 'affine')
    with pytest.raises(ValueError):                                   # a typed source must be contiguous
        image_tools.resample_device(i16[..., 0], SRC_FRAME, CROP[::-1], DST_FRAME, 'LINEAR')
    plane = _at(_integers('uint8')[..., 0], False, hip_device)
    got = image_tools.resample_device(plane, SRC_FRAME, CROP[::-1], DST_FRAME, 'NN', PAD)
    assert torch.equal(_bits(got), _bits(_float_reference('uint8', 1, 'NN', 'affine')[..., 0]))


# ---------------------------------------------------------------------------------------------------------------------
# the data set
# ---------------------------------------------------------------------------------------------------------------------
SHAPE = (30, 36, 40)                     # z, y, x
FRAME = ((1.0, 1.1, 0.9), (-4.0, 2.0, 7.0), tuple(np.eye(3).ravel()))
_LPS = np.diag([-1.0, -1.0, 1.0])


def _write_nifti_4d_i16(path, planes):
    """a 4-D int16 NIfTI-1 file, dim = (4, X, Y, Z, M), the sform holding FRAME"""
    planes = np.asarray(planes, dtype=np.int16)
    M, Z, Y, X = planes.shape
    spacing, origin, direction = FRAME
    rot = _LPS @ np.asarray(direction, dtype=np.float64).reshape(3, 3) * np.asarray(spacing, dtype=np.float64)
    offset = _LPS @ np.asarray(origin, dtype=np.float64)
    hdr = bytearray(352)
    struct.pack_into('<i', hdr, 0, 348)
    struct.pack_into('<8h', hdr, 40, 4, X, Y, Z, M, 1, 1, 1)
    struct.pack_into('<hh', hdr, 70, 4, 16)
    struct.pack_into('<8f', hdr, 76, 1.0, spacing[0], spacing[1], spacing[2], 1.0, 0.0, 0.0, 0.0)
    struct.pack_into('<f', hdr, 108, 352.0)
    struct.pack_into('<2f', hdr, 112, 1.0, 0.0)
    struct.pack_into('<2h', hdr, 252, 0, 1)
    for r in range(3):
        struct.pack_into('<4f', hdr, 280 + 16 * r, rot[r, 0], rot[r, 1], rot[r, 2], offset[r])
    hdr[344:348] = b'n+1\x00'
    with open(str(path), 'wb') as f:
        f.write(bytes(hdr))
        f.write(planes.astype('<i2').tobytes())


def _ct(rng):
    a = rng.randint(-1000, 3000, size=SHAPE).astype(np.int16)
    a[0, 0, 0], a[-1, -1, -1] = -32768, 32767
    return a


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.image_io import write_image
    root = tmp_path_factory.mktemp('resident')
    rng = np.random.RandomState(33)
    single, nifti2 = [], []
    for k in range(3):
        d = root / 'case{}'.format(k)
        d.mkdir()
        mask = (rng.rand(*SHAPE) > 0.6).astype(np.uint8)
        write_image(Image3d(mask, *FRAME), str(d / 'seg.mha'))
        image = _ct(rng) if k < 2 else (mask * 2.0 - 1.0 + 0.3 * rng.randn(*SHAPE)).astype(np.float32)
        if k < 2:                                  # a learnable toy: the label map shows through the noise
            image = (image // 8 + 400 * mask.astype(np.int16)).astype(np.int16)
            image[0, 0, 0], image[-1, -1, -1] = -32768, 32767
        write_image(Image3d(image, *FRAME), str(d / 'org.mha'))
        single += [str(d / 'org.mha'), str(d / 'seg.mha')]
        _write_nifti_4d_i16(d / 'two.nii', [_ct(rng), _ct(rng)])
        nifti2 += [str(d / 'two.nii'), str(d / 'seg.mha')]
    (root / 'single.txt').write_text('3\n' + '\n'.join(single) + '\n')
    (root / 'nifti2.txt').write_text('3 2\n' + '\n'.join(nifti2) + '\n')
    return root


AUG = {'rotation_deg': [15.0, 10.0, 20.0], 'rotation_prob': 1.0, 'elastic_grid_mm': 8.0, 'elastic_magnitude_mm': [0.5, 1.0],
       'elastic_prob': 1.0, 'brightness': [0.8, 1.2], 'brightness_prob': 1.0, 'contrast': [0.8, 1.2], 'contrast_prob': 1.0,
       'gamma': [0.7, 1.5], 'gamma_prob': 1.0, 'gamma_invert_prob': 0.5, 'noise_sigma': [0.01, 0.1], 'noise_prob': 1.0}
RES = {'blur_sigma_vox': [0.5, 1.5], 'blur_prob': 1.0, 'lowres_zoom': [0.5, 0.9], 'lowres_prob': 1.0}
ORDER = [0, 1, 2, 0, 2, 1]


def _dataset(toy, name, device, storage, budget=None, interp='LINEAR', volume_norm=False):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer, VolumeNormalizer
    M = 2 if name == 'nifti2' else 1
    norms = [VolumeNormalizer(clip_percentiles=(0.5, 99.5)) if volume_norm else AdaptiveNormalizer() for _ in range(M)]
    return SegmentationDataset(str(toy / (name + '.txt')), 2, [1.0, 1.0, 1.0], [16, 16, 16], 'MASK', [2, 2, 2], [0.9, 1.1],
                               interp, norms, device=device, random_mirror_axes=('x', 'y', 'z'), augmentation=AUG,
                               resolution_augmentation=RES, resident_storage=storage, resident_budget_gb=budget)


def _draw(ds, seed=17, order=ORDER):
    """six seeded samples on the host + numpy's global state afterwards"""
    np.random.seed(seed)
    out = []
    for i in order:
        im, seg, frame, name = ds.sample(i)
        out.append((im.contiguous().cpu(), seg.cpu(), frame, name))
    return out, np.random.get_state()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _same_samples(a, b):
    for (im_a, seg_a, frame_a, name_a), (im_b, seg_b, frame_b, name_b) in zip(a, b):
        if not (torch.equal(_bits(im_a), _bits(im_b)) and torch.equal(_bits(seg_a), _bits(seg_b))
                and np.array_equal(frame_a.view(np.int32), frame_b.view(np.int32)) and name_a == name_b):
            return False
    return len(a) == len(b)


@functools.lru_cache(maxsize=None)
def _fp32_run(root, name, interp, volume_norm):
    """the 'fp32' run every variant is compared with: drawn once, kept on the host"""
    import pathlib
    ds = _dataset(pathlib.Path(root), name, torch.device('cuda:0'), 'fp32', interp=interp, volume_norm=volume_norm)
    samples, state = _draw(ds)
    norms = [ds.case(i).normalizers for i in range(3)]
    return samples, state, ds.resident_bytes(), [ds.case(i).nbytes for i in range(3)], norms


def _tensor_bytes(ds):
    return sum(c.volume.numel() * c.volume.element_size() + c.seg.numel() * c.seg.element_size()
               for c in (ds.case(i) for i in range(len(ds))) if not c.staged)


@pytest.mark.parametrize('name', ['single', 'nifti2'])
def test_compact_samples_equal_the_fp32_samples(hip_device, toy, name):
    want, state, fp32_bytes, fp32_case_bytes, _ = _fp32_run(str(toy), name, 'LINEAR', False)
    assert len({tuple(s[0].flatten()[:64].tolist()) for s in want}) == len(want)       # six different crops
    ds = _dataset(toy, name, hip_device, 'compact')
    got, state_c = _draw(ds)
    assert _same_samples(got, want) and _same_state(state, state_c)
    voxels = int(np.prod(SHAPE))
    for i in range(3):
        c = ds.case(i)
        compact_image = name == 'nifti2' or i < 2
        assert c.volume.dtype == (torch.int16 if compact_image else torch.float32) and c.seg.dtype == torch.uint8
        assert not c.staged and c.volume.is_cuda and c.seg.is_cuda
        assert c.nbytes == voxels * (c.num_modality * (2 if compact_image else 4) + 1)
        assert fp32_case_bytes[i] == voxels * (c.num_modality * 4 + 4)
    assert ds.resident_bytes() == _tensor_bytes(ds) and ds.num_staged() == 0 and not ds.has_budget()
    if name == 'single':                                # an (a) case: 2 + 1 bytes per voxel against 4 + 4
        assert 8 * ds.case(0).nbytes == 3 * fp32_case_bytes[0]
    else:                                               # (b): 2 * 2 + 1 against 2 * 4 + 4
        assert 12 * ds.resident_bytes() == 5 * fp32_bytes


@pytest.mark.parametrize('name', ['single', 'nifti2'])
def test_compact_with_a_volume_normalizer(hip_device, toy, name):
    from segmentation3d.utils.image_tools import _normalizer_dict
    want, state, _, _, norms = _fp32_run(str(toy), name, 'LINEAR', True)
    ds = _dataset(toy, name, hip_device, 'compact', volume_norm=True)
    got, state_c = _draw(ds)
    assert _same_samples(got, want) and _same_state(state, state_c)
    for i in range(3):
        mine = [_normalizer_dict(n) for n in ds.case(i).normalizers]
        assert mine == [_normalizer_dict(n) for n in norms[i]] and all(d['type'] == 3 for d in mine)
        assert ds.case(i).volume.dtype == (torch.int16 if name == 'nifti2' or i < 2 else torch.float32)


def test_compact_with_bspline_keeps_the_coefficients_fp32(hip_device, toy):
    want, state, _, _, _ = _fp32_run(str(toy), 'single', 'BSPLINE', False)
    ds = _dataset(toy, 'single', hip_device, 'compact', interp='BSPLINE')
    got, state_c = _draw(ds)
    assert _same_samples(got, want) and _same_state(state, state_c)
    for i in range(3):
        assert ds.case(i).volume.dtype == torch.float32 and ds.case(i).seg.dtype == torch.uint8


# ---- the budget: it admits exactly the first case the sampler touches ----------------------------------------------------
def _one_case_budget(ds_bytes):
    return (ds_bytes + 0.5) / 1e9


@pytest.mark.parametrize('name, interp', [('single', 'LINEAR'), ('nifti2', 'LINEAR'), ('single', 'BSPLINE')])
def test_budget_stages_what_does_not_fit(hip_device, toy, name, interp):
    want, state, _, _, _ = _fp32_run(str(toy), name, interp, False)
    voxels = int(np.prod(SHAPE))
    M = 2 if name == 'nifti2' else 1
    first = voxels * (M * (4 if interp == 'BSPLINE' else 2) + 1)                 # case 0 in its storage dtypes
    ds = _dataset(toy, name, hip_device, 'compact', budget=_one_case_budget(first), interp=interp)
    assert ds.has_budget() and ds.num_staged() == 0 and ds.resident_bytes() == 0
    for i in ORDER[:3]:                                                          # first touch, in the sampler's order
        ds.case(i)
        assert ds.resident_bytes() <= first + 0.5
    assert ds.num_staged() == 2 and ds.num_resident() == 1 and ds.resident_bytes() == first == _tensor_bytes(ds)
    assert not ds.case(0).staged and ds.case(1).staged and ds.case(2).staged
    staged = ds.case(1)
    assert staged.volume is None and staged.seg is None and staged.volume_pinned.is_pinned() and staged.seg_pinned.is_pinned()
    assert not staged.volume_pinned.is_cuda and staged.seg_pinned.dtype == torch.uint8
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    got, state_b = _draw(ds)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= before + max(ds.case(i).nbytes for i in range(3))
    assert _same_samples(got, want) and _same_state(state, state_b)
    assert ds.num_staged() == 2 and ds.resident_bytes() == first
    again, _ = _draw(ds)                                                         # the staged arrays are not consumed
    assert _same_samples(again, want)


# ---- train() ------------------------------------------------------------------------------------------------------------
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
__C.dataset.random_scale = [0.95, 1.05]
__C.dataset.interpolation = 'LINEAR'
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
__C.train.use_graph = {graph}
__C.validation = {{}}
__C.validation.imseg_list = '{train}'
__C.validation.crops_per_case = 2
__C.validation.ema = 0.5
__C.validation.save_best = False
{extra}'''

_MODES = {
    'fp32': '',
    'compact': "__C.dataset.resident_storage = 'compact'\n",
    'budget': "__C.dataset.resident_storage = 'compact'\n__C.dataset.resident_budget_gb = {!r}\n".format(
        _one_case_budget(int(np.prod(SHAPE)) * 3)),
}
_RUNS = {}


def _train_run(toy, mode, graph):
    """train() on the `single` set -> (train_loss strings, val_dice strings, the residency lines); run once per variant"""
    key = (mode, graph)
    if key not in _RUNS:
        from segmentation3d import _ops
        from segmentation3d.core.seg_train import train
        save = toy / 'run_{}_{}'.format(mode, int(graph))
        os.makedirs(str(save), exist_ok=True)
        (save / 'cfg.py').write_text(_CFG.format(train=str(toy / 'single.txt'), save=str(save), graph=graph,
                                                 extra=_MODES[mode]))
        random.seed(0)
        try:
            train(str(save / 'cfg.py'))
        finally:
            _ops.set_activation_dtype('fp32')
        log = (save / 'coarse' / 'train_log.txt').read_text().strip().splitlines()
        _RUNS[key] = ([l.split('train_loss: ')[1].split(',')[0] for l in log if 'train_loss' in l],
                      [l.split('val_dice: ')[1].split(',')[0] for l in log if 'val_dice: ' in l],
                      [l for l in log if 'resident cases' in l])
    return _RUNS[key]


@pytest.mark.parametrize('graph', [False, True])
@pytest.mark.parametrize('mode', ['compact', 'budget'])
def test_train_logs_the_same_losses(hip_device, toy, mode, graph):
    losses, dices, _ = _train_run(toy, 'fp32', graph)
    assert len(losses) == 3 and len(dices) >= 1 and len(set(losses)) > 1
    got_losses, got_dices, residency = _train_run(toy, mode, graph)
    assert got_losses == losses and got_dices == dices
    if mode == 'budget':                 # one line, after the first epoch: the (a) case that came first stays, two are staged
        assert len(residency) == 1 and 'resident cases: 1, staged cases: 2, resident bytes: {}'.format(
            int(np.prod(SHAPE)) * 3) in residency[0]
    else:
        assert residency == []
