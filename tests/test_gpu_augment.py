"""GPU side of the training augmentation: seg3d_resample_deform(_mc) and
seg3d_augment_intensity against the float64 numpy oracle of tests/test_augment.py (pinned there on the CPU), the exact
contracts (zero field = the affine entries, _mc channel = planar entry, mirrored = flipped, neutral = untouched, reruns
bit-equal), the data set end to end and train() from a config file."""
import os

import numpy as np
import pytest
import torch

from gpu_util import report
from test_augment import (oracle_coords, oracle_sample, oracle_tie_distance, oracle_control_dims, oracle_rotation,
                          oracle_intensity, oracle_normal)

pytestmark = pytest.mark.gpu

# a smooth source volume at anisotropic spacing with an oblique direction matrix
_SHAPE = (40, 44, 48)                                                   # z, y, x
_SRC = ((0.8, 1.1, 1.7), (-12.0, 5.0, 30.0), tuple(oracle_rotation((0.1, -0.15, 0.2)).ravel()))
_SIZE = (32, 28, 24)                                                    # crop, x y z
_DSP = (1.0, 0.9, 1.3)
_H = 8.0
TIE = 1e-6                      # NN: voxels whose sample point is closer than this to a half-voxel tie are not compared
TIE_SHARE = 1e-3                # and they may be at most 0.1 % of the crop


def _dst_frame(src=_SRC, shape=_SHAPE, size=_SIZE, dsp=_DSP, shift=(8.0, -13.0, 22.0)):
    """crop grid with the source's direction whose centre is the source volume's centre (+ a shift in mm)"""
    sp, org, d = (np.asarray(v, dtype=np.float64) for v in src)
    D = d.reshape(3, 3)
    n_src = np.array(shape[::-1], dtype=np.float64)
    centre = org + D @ (sp * (n_src - 1) / 2) + np.asarray(shift)
    origin = centre - D @ (np.asarray(dsp) * (np.asarray(size, dtype=np.float64) - 1) / 2)
    return (tuple(dsp), tuple(origin), tuple(d))


def _smooth(M):
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in _SHAPE), indexing='ij')
    return [(np.sin(0.21 * x + 0.3 * m) * np.cos(0.17 * y - 0.1 * m) + 0.5 * np.sin(0.13 * z + 0.05 * x * (m + 1) / 4)
             ).astype(np.float32) for m in range(M)]


def _labels(seed=3):
    return np.random.RandomState(seed).randint(0, 4, size=_SHAPE).astype(np.float32)


def _control(seed, size=_SIZE, dsp=_DSP, h=_H, a=None):
    g = oracle_control_dims(size, dsp, h)
    a = h / 6.0 * 0.9 if a is None else a
    return np.random.RandomState(seed).uniform(-a, a, size=(g[2], g[1], g[0], 3)).astype(np.float32)


def _dev(planes, device):
    """list of [Z, Y, X] arrays -> planar device tensor (M = 1) or channels-last [Z, Y, X, M]"""
    if len(planes) == 1:
        return torch.from_numpy(planes[0]).to(device)
    return torch.from_numpy(np.stack(planes, -1).copy()).to(device)


def _resample(vol, method, device_ctrl=None, mirror=None, rotation=None, dst=None):
    from segmentation3d.utils import image_tools as T
    dst = dst or _dst_frame()
    deform = None if device_ctrl is None else (device_ctrl, _H)
    fn = T.resample_device if vol.dim() == 3 else T.resample_device_mc
    return fn(vol, _SRC, _SIZE, dst, method, -2.0, mirror=mirror, rotation=rotation, deform=deform)


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact contracts of the deform entries
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('method', ['LINEAR', 'NN'])
def test_zero_control_tensor_is_the_affine_entry_bit_for_bit(hip_device, method, M):
    vol = _dev(_smooth(M), hip_device)
    zero = torch.zeros(_control(0).shape, dtype=torch.float32, device=hip_device)
    for mirror in (None, (True, False, True), (True, True, True)):
        for rotation in (None, (0.2, -0.1, 0.3)):
            plain = _resample(vol, method, None, mirror, rotation)
            deformed = _resample(vol, method, zero, mirror, rotation)
            assert torch.equal(plain.view(torch.int32), deformed.view(torch.int32)), (mirror, rotation)


@pytest.mark.parametrize('M', [2, 3, 4, 5])
@pytest.mark.parametrize('method', ['LINEAR', 'NN'])
def test_mc_channel_equals_the_planar_entry_bit_for_bit(hip_device, method, M):
    planes = _smooth(M)
    ctrl = torch.from_numpy(_control(5)).to(hip_device)
    for mirror in (None, (False, True, True)):
        mc = _resample(_dev(planes, hip_device), method, ctrl, mirror, (0.1, 0.2, -0.3))
        assert tuple(mc.shape) == (_SIZE[2], _SIZE[1], _SIZE[0], M)
        for m in range(M):
            one = _resample(_dev(planes[m:m + 1], hip_device), method, ctrl, mirror, (0.1, 0.2, -0.3))
            assert torch.equal(mc[..., m].contiguous().view(torch.int32), one.view(torch.int32)), m
    assert float((mc - _resample(_dev(planes, hip_device), method, None, mirror, (0.1, 0.2, -0.3))).abs().max()) > 1e-3


def test_deform_entries_refuse_bad_arguments(hip_device):
    from segmentation3d.utils import image_tools as T
    vol = _dev(_smooth(1), hip_device)
    good = _control(0)
    with pytest.raises(ValueError, match='control'):
        T.resample_device(vol, _SRC, _SIZE, _dst_frame(), 'LINEAR', deform=(torch.zeros((3, 3, 3, 3), device=hip_device), _H))
    with pytest.raises(ValueError):
        T.resample_device(vol, _SRC, _SIZE, _dst_frame(), 'LINEAR', deform=(torch.from_numpy(good).to(hip_device), 0.0))
    with pytest.raises(ValueError):
        T.resample_device(vol, _SRC, _SIZE, _dst_frame(), 'LINEAR',
                          deform=(torch.from_numpy(good.astype(np.float64)).to(hip_device), _H))
    # the C entry checks the grid itself: too few control points / a grid finer than the voxels / an LDS image too large
    import ctypes
    from segmentation3d import _engine as E
    dst = torch.empty((4, 4, 4), dtype=torch.float32, device=hip_device)
    A = np.ascontiguousarray(np.eye(3, 4), dtype=np.float64)
    L = np.ascontiguousarray(np.eye(3), dtype=np.float64)
    ctrl = torch.zeros((4, 4, 4, 3), dtype=torch.float32, device=hip_device)

    def call(t, g=(4, 4, 4), mask=0):
        tt = np.array(t, dtype=np.float64)
        return E.call('seg3d_resample_deform', E.ptr(vol), E.ptr(dst), 48, 44, 40, 4, 4, 4, A.ctypes.data_as(ctypes.c_void_p), 1,
                      0.0, L.ctypes.data_as(ctypes.c_void_p), E.ptr(ctrl), g[0], g[1], g[2], tt.ctypes.data_as(ctypes.c_void_p),
                      mask, E.stream_ptr())
    call((0.3, 0.3, 0.3))
    for kw in ({'t': (0.5, 0.3, 0.3)}, {'t': (1.5, 0.3, 0.3)}, {'t': (0.3, 0.3, 0.3), 'g': (3, 4, 4)},
               {'t': (0.3, 0.3, 0.3), 'mask': 8}, {'t': (0.3, 0.3, 0.3), 'g': (40, 40, 40)}):
        with pytest.raises(ValueError):
            call(**kw)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 2. rotation + elastic against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [1, 4])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_rotated_deformed_linear_crop_against_the_oracle(hip_device, seed, M):
    rng = np.random.RandomState(100 + seed)
    rotation = tuple(np.deg2rad(rng.uniform(-25, 25, size=3)))
    mirror = tuple(bool(v) for v in rng.randint(0, 2, size=3))
    ctrl = _control(seed)
    planes = _smooth(M)
    got = _resample(_dev(planes, hip_device), 'LINEAR', torch.from_numpy(ctrl).to(hip_device), mirror, rotation).cpu().numpy()
    c = oracle_coords(_SRC, _dst_frame(), _SIZE, rotation, ctrl, _H, mirror)
    worst = 0.0
    for m in range(M):
        want = oracle_sample(planes[m], c, True, -2.0)
        assert 0.02 < (want == -2.0).mean() < 0.9                            # the crop leaves the volume somewhere
        worst = max(worst, float(np.abs((got if M == 1 else got[..., m]).astype(np.float64) - want).max()))
    print('deform LINEAR seed {} M {}: max |device - oracle| = {:.3e}'.format(seed, M, worst))
    report('augment_deform_linear_s{}_M{}'.format(seed, M), err=worst)
    assert worst < 2e-5


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_rotated_deformed_nn_crop_against_the_oracle_away_from_ties(hip_device, seed):
    rng = np.random.RandomState(100 + seed)
    rotation = tuple(np.deg2rad(rng.uniform(-25, 25, size=3)))
    mirror = tuple(bool(v) for v in rng.randint(0, 2, size=3))
    ctrl = _control(seed)
    lab = _labels()
    got = _resample(_dev([lab], hip_device), 'NN', torch.from_numpy(ctrl).to(hip_device), mirror, rotation).cpu().numpy()
    c = oracle_coords(_SRC, _dst_frame(), _SIZE, rotation, ctrl, _H, mirror)
    want = oracle_sample(lab, c, False, -2.0)
    near = oracle_tie_distance(c) < TIE
    share = float(near.mean())
    wrong = int(((got != want) & ~near).sum())
    print('deform NN seed {}: {} voxels near a tie (share {:.2e}), {} mismatches away from ties'.format(
        seed, int(near.sum()), share, wrong))
    report('augment_deform_nn_s{}'.format(seed), tie_share=share, mismatches=float(wrong))
    assert share <= TIE_SHARE
    assert wrong == 0


def test_quarter_turn_about_z_is_rot90_of_the_plain_crop(hip_device):
    from segmentation3d.utils import image_tools as T
    n = 24
    src = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    dst = ((1.0, 1.0, 1.0), (10.25, 8.25, 7.75), tuple(np.eye(3).ravel()))
    for method, vol in (('LINEAR', _smooth(1)[0]), ('NN', _labels())):
        v = torch.from_numpy(vol).to(hip_device)
        plain = T.resample_device(v, src, (n, n, n), dst, method, 0.0)
        turned = T.resample_device(v, src, (n, n, n), dst, method, 0.0, rotation=(0.0, 0.0, np.pi / 2))
        want = torch.rot90(plain, 1, (1, 2))
        if method == 'LINEAR':
            err = float((turned - want).abs().max())
            print('rot90 LINEAR: max |rotated - rot90(plain)| = {:.3e}'.format(err))
            assert err < 2e-5 and float(plain.abs().max()) > 0.5
        else:
            c = oracle_coords(src, dst, (n, n, n), rotation=(0.0, 0.0, np.pi / 2))
            far = torch.from_numpy(oracle_tie_distance(c) >= TIE).to(hip_device)
            assert float(far.float().mean()) >= 1 - TIE_SHARE
            assert torch.equal(turned[far], want[far])


@pytest.mark.parametrize('M', [1, 2])
def test_mirrored_deformed_crop_is_the_flip_of_the_plain_deformed_crop(hip_device, M):
    """the bars of the existing mirror test: image within 2e-5, mask exact (away from ties, asserted through the oracle)"""
    ctrl_h = _control(7)
    ctrl = torch.from_numpy(ctrl_h).to(hip_device)
    rotation = (0.15, -0.2, 0.1)
    vol, lab = _dev(_smooth(M), hip_device), _dev([_labels()], hip_device)
    plain_im, plain_lab = _resample(vol, 'LINEAR', ctrl, None, rotation), _resample(lab, 'NN', ctrl, None, rotation)
    for mirror in ((True, False, False), (False, True, True), (True, True, True)):
        dims = [2 - a for a in range(3) if mirror[a]]                       # [z, y, x(, m)]
        im = _resample(vol, 'LINEAR', ctrl, mirror, rotation)
        err = float((im - torch.flip(plain_im, dims)).abs().max())
        print('mirrored deformed crop M {} {}: max |image - flip| = {:.3e}'.format(M, mirror, err))
        assert err < 2e-5
        got = _resample(lab, 'NN', ctrl, mirror, rotation)
        c = oracle_coords(_SRC, _dst_frame(), _SIZE, rotation, ctrl_h, _H, mirror)
        far = torch.from_numpy(oracle_tie_distance(c) >= TIE).to(hip_device)
        assert float(far.float().mean()) >= 1 - TIE_SHARE
        assert torch.equal(got[far], torch.flip(plain_lab, dims)[far])


def test_image_and_mask_stay_registered(hip_device):
    """a label volume deformed as the image (NN, the _mc entry beside another channel) and as the mask (planar entry)"""
    from segmentation3d.utils import image_tools as T
    lab = _labels()
    ctrl = torch.from_numpy(_control(9)).to(hip_device)
    as_mask = T.crop_image_device(torch.from_numpy(lab).to(hip_device), _SRC, (3.0, 30.0, 60.0), _SIZE, _DSP, 'NN',
                                  mirror=(True, False, False), rotation=(0.1, 0.1, 0.1), deform=(ctrl, _H))
    as_image = T.crop_image_device_mc(_dev([lab, _smooth(1)[0]], hip_device), _SRC, (3.0, 30.0, 60.0), _SIZE, _DSP, 'NN',
                                      mirror=(True, False, False), rotation=(0.1, 0.1, 0.1), deform=(ctrl, _H))
    assert torch.equal(as_mask, as_image[..., 0]) and float(as_mask.max()) == 3.0


# ---------------------------------------------------------------------------------------------------------------------
# 3. intensity
# ---------------------------------------------------------------------------------------------------------------------
_INT_CASES = {
    'brightness': {'brightness': 1.2},
    'contrast_up': {'contrast': 1.25},
    'contrast_down': {'contrast': 0.75},
    'gamma': {'gamma': 0.7},
    'gamma_invert': {'gamma': 1.5, 'invert': True},
    'noise': {'sigma': 0.1},
    'all': {'brightness': 0.8, 'contrast': 1.2, 'gamma': 1.4, 'invert': True, 'sigma': 0.05},
}


def _crop(shape_zyx, M, seed):
    return np.clip(np.random.RandomState(seed).randn(*shape_zyx, M) * 0.5, -1.0, 1.0).astype(np.float32)


def _augment(x, params, seed, device, grid_blocks=0):
    from segmentation3d.utils.image_tools import augment_intensity_device
    t = torch.from_numpy(x.copy()).to(device)
    if x.shape[3] == 1:
        return augment_intensity_device(t[..., 0].contiguous(), params, seed, grid_blocks).unsqueeze(3)
    return augment_intensity_device(t, params, seed, grid_blocks)


@pytest.mark.parametrize('shape', [(6, 7, 9), (16, 20, 33)])
@pytest.mark.parametrize('M', [1, 2, 4, 5])
@pytest.mark.parametrize('case', sorted(_INT_CASES))
def test_intensity_against_the_oracle(hip_device, case, M, shape):
    x = _crop(shape, M, 17 + M)
    # the named transform on every modality, with per-modality values; the last modality stays neutral when M > 1
    params = []
    for m in range(M):
        p = dict(_INT_CASES[case])
        for key in ('brightness', 'contrast', 'gamma'):
            if key in p:
                p[key] = p[key] * (1.0 + 0.05 * m)
        params.append(None if (M > 1 and m == M - 1) else p)
    seed = (0x9e3779b9 << 32) | 0x1234567
    got = _augment(x, params, seed, hip_device).cpu().numpy()
    want = oracle_intensity(x, params, seed)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print('intensity {} M {} {}: max |device - oracle| = {:.3e}'.format(case, M, shape, err))
    report('augment_intensity_{}_M{}_{}'.format(case, M, shape[2]), err=err)
    assert err < 1e-4
    if M > 1:
        assert np.array_equal(got[..., M - 1].view(np.uint32), x[..., M - 1].view(np.uint32))   # neutral: untouched
    assert float(np.abs(got - x).max()) > 1e-3


@pytest.mark.parametrize('case', ['all', 'noise'])
def test_intensity_full_size_crop(hip_device, case):
    x = _crop((96, 96, 96), 4, 5)
    params = [dict(_INT_CASES[case]) for _ in range(4)]
    got = _augment(x, params, 77, hip_device)
    again = _augment(x, params, 77, hip_device)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))                         # two runs are bit-equal
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - oracle_intensity(x, params, 77)).max())
    print('intensity {} 96^3 x 4: max |device - oracle| = {:.3e}'.format(case, err))
    report('augment_intensity_{}_96'.format(case), err=err)
    assert err < 1e-4


@pytest.mark.parametrize('M', [1, 2, 3, 4, 5])
def test_neutral_parameters_return_the_input_bit_for_bit(hip_device, M):
    x = _crop((6, 7, 9), M, 3)
    x[0, 0, 0, 0] = -0.0
    for params in ([None] * M, [{'brightness': 1.0, 'contrast': 1.0, 'gamma': 1.0, 'invert': True, 'sigma': 0.0}] * M):
        got = _augment(x, params, 5, hip_device).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


def test_constant_crop_passes_through_gamma_and_contrast_unchanged(hip_device):
    x = np.full((6, 7, 9, 2), 0.25, np.float32)
    got = _augment(x, [{'gamma': 0.5, 'invert': True}, {'gamma': 2.0, 'contrast': 1.3}], 0, hip_device).cpu().numpy()
    assert np.array_equal(got, x)


def test_noise_is_standard_normal_and_a_function_of_voxel_and_modality_alone(hip_device):
    shape = (96, 96, 96)
    zeros = np.zeros(shape + (1,), np.float32)
    got = _augment(zeros, [{'sigma': 1.0}], 424242, hip_device)
    n = got.cpu().numpy()[..., 0].astype(np.float64)
    err = float(np.abs(n - oracle_normal(424242, shape, 0)).max())
    se = 1.0 / np.sqrt(n.size)
    print('noise: max |device - oracle| = {:.3e}, mean = {:.3e} ({:.2f} se), var - 1 = {:.3e} ({:.2f} se)'.format(
        err, n.mean(), n.mean() / se, n.var() - 1.0, (n.var() - 1.0) / (np.sqrt(2.0) * se)))
    report('augment_noise', err=err, mean=float(n.mean()), var=float(n.var()))
    assert err < 1e-4
    assert abs(n.mean()) < 5 * se and abs(n.var() - 1.0) < 5 * np.sqrt(2.0) * se
    # channel m does not change with M, with the vector / scalar path or with the launch's grid
    small = (10, 12, 14)
    ref = {}
    for M in (1, 2, 3, 4, 5):
        for grid in (0, 1, 7):
            out = _augment(np.zeros(small + (M,), np.float32), [{'sigma': 1.0}] * M, 99, hip_device, grid)
            for m in range(M):
                if m not in ref:
                    ref[m] = out[..., m].clone()
                assert torch.equal(out[..., m].contiguous().view(torch.int32), ref[m].contiguous().view(torch.int32)), (M, m, grid)
    assert not torch.equal(ref[0], ref[1])
    assert float((ref[0].cpu().double() - torch.from_numpy(oracle_normal(99, small, 0))).abs().max()) < 1e-4


def test_intensity_entry_refuses_bad_arguments(hip_device):
    from segmentation3d import _engine as E
    from segmentation3d.utils.image_tools import augment_intensity_device
    x = torch.zeros((4, 4, 4, 2), device=hip_device)
    with pytest.raises(ValueError):
        augment_intensity_device(x, [{'gamma': 0.0}, None])
    with pytest.raises(ValueError):
        augment_intensity_device(x.permute(3, 0, 1, 2), [None, None])
    with pytest.raises(ValueError):
        augment_intensity_device(torch.zeros((4, 4, 4, 9), device=hip_device), [None] * 9)
    bad = E.IntensityParams()                                               # all zeros: brightness 0 is refused by the C entry
    with pytest.raises(ValueError, match='brightness'):
        augment_intensity_device(x, bad)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the data set end to end
# ---------------------------------------------------------------------------------------------------------------------
_ALL_ON = {'rotation_deg': [10, 20, 30], 'rotation_prob': 1.0, 'elastic_grid_mm': 8.0, 'elastic_magnitude_mm': [0.2, 1.2],
           'elastic_prob': 1.0, 'brightness': [0.75, 1.25], 'brightness_prob': 1.0, 'contrast': [0.75, 1.25],
           'contrast_prob': 1.0, 'gamma': [0.7, 1.5], 'gamma_prob': 1.0, 'gamma_invert_prob': 0.5, 'noise_sigma': [0.0, 0.1],
           'noise_prob': 1.0}


def _datasets(tmp_path, M, device, **kw):
    from test_gpu_blend_tta import _write_case
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer, FixedNormalizer
    lst, frame = _write_case(tmp_path, M)
    norms = [AdaptiveNormalizer(), FixedNormalizer(10.0, 90.0, False)][:M]
    args = (lst, 3, [1.0, 1.0, 1.2], [32, 32, 16], 'GLOBAL', [3, 3, 3], [0.9, 1.1], 'LINEAR', norms)
    return SegmentationDataset(*args, device=device, **kw), norms, frame


@pytest.mark.parametrize('M', [1, 2])
def test_dataset_with_everything_on_equals_the_oracle_pipeline(hip_device, tmp_path, M):
    from oracle import numpy_ref
    from segmentation3d.utils.image_tools import crop_origin
    ds, norms, frame = _datasets(tmp_path, M, hip_device, augmentation=_ALL_ON, random_mirror_axes=('x', 'z'))
    case = ds.case(0)
    vols = case.image.cpu().numpy()
    vols = [vols] if M == 1 else [vols[..., m] for m in range(M)]
    worst, ties = 0.0, 0.0
    for seed in range(4):
        np.random.seed(seed)
        center, sp = ds.sample_crop_geometry(0)
        mirror = ds.sample_mirror()
        aug = ds.sample_augmentation(sp)
        assert aug['rotation'] is not None and aug['control'] is not None and aug['intensity'] is not None
        np.random.seed(seed)
        im, seg, out_frame, _ = ds.sample(0)
        assert tuple(im.shape) == (M, 16, 32, 32) and tuple(seg.shape) == (1, 16, 32, 32)
        size = [int(v) for v in ds.crop_size]
        dst = ([float(v) for v in sp], crop_origin(center, size, sp), frame[2])
        c = oracle_coords(frame, dst, size, aug['rotation'], aug['control'], _ALL_ON['elastic_grid_mm'], mirror)
        crop = np.stack([numpy_ref.apply_normalizer(oracle_sample(vols[m], c, True, 0.0),
                                                    None if norms[m] is None else norms[m].to_dict()) for m in range(M)], -1)
        want = oracle_intensity(crop, aug['intensity'], aug['seed'])
        err = float(np.abs(im.permute(1, 2, 3, 0).cpu().numpy().astype(np.float64) - want).max())
        want_seg = oracle_sample(case.seg_host.astype(np.float32), c, False, 0.0)
        near = oracle_tie_distance(c) < TIE
        wrong = int(((seg[0].cpu().numpy() != want_seg) & ~near).sum())
        print('dataset all-on M {} seed {}: max |image - oracle| = {:.3e}, ties {:.2e}, mask mismatches {}'.format(
            M, seed, err, near.mean(), wrong))
        worst, ties = max(worst, err), max(ties, float(near.mean()))
        assert near.mean() <= TIE_SHARE and wrong == 0
        # the frame is the nominal (un-rotated, un-deformed) mirrored crop frame
        plain = _datasets(tmp_path, M, hip_device, random_mirror_axes=('x', 'z'))[0]
        np.random.seed(seed)
        assert np.array_equal(plain.sample(0)[2], out_frame)
    report('augment_dataset_M{}'.format(M), err=worst, tie_share=ties)
    assert worst < 1e-4


@pytest.mark.parametrize('M', [1, 2])
def test_dataset_with_everything_off_is_bit_equal_to_no_argument(hip_device, tmp_path, M):
    off = dict(_ALL_ON, rotation_prob=0.0, elastic_prob=0.0, brightness_prob=0.0, contrast_prob=0.0, gamma_prob=0.0,
               noise_prob=0.0)
    plain = _datasets(tmp_path, M, hip_device, random_mirror_axes=('y',))[0]
    for aug in (off, {}):
        ds = _datasets(tmp_path, M, hip_device, random_mirror_axes=('y',), augmentation=aug)[0]
        for seed in range(3):
            np.random.seed(seed)
            a = plain.sample(0)
            sa = np.random.get_state()
            np.random.seed(seed)
            b = ds.sample(0)
            sb = np.random.get_state()
            assert torch.equal(a[0].contiguous().view(torch.int32), b[0].contiguous().view(torch.int32))
            assert torch.equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(sa[1], sb[1]) and sa[2] == sb[2]


_TRAIN_CFG = '''
from easydict import EasyDict as edict
from segmentation3d.utils.normalizer import AdaptiveNormalizer, FixedNormalizer
__C = edict()
cfg = __C
__C.general = {}
__C.general.imseg_list = '%s'
__C.general.save_dir = '%s'
__C.general.model_scale = 'coarse'
__C.general.resume_epoch = -1
__C.general.num_gpus = 1
__C.general.seed = 0
__C.dataset = {}
__C.dataset.num_classes = 2
__C.dataset.spacing = [1.0, 1.0, 1.0]
__C.dataset.crop_size = [32, 32, 32]
__C.dataset.sampling_method = 'GLOBAL'
__C.dataset.random_translation = [2, 2, 2]
__C.dataset.random_scale = [0.95, 1.05]
__C.dataset.random_mirror_axes = ['x']
__C.dataset.interpolation = 'LINEAR'
__C.dataset.crop_normalizers = %s
__C.dataset.augmentation = {}
__C.dataset.augmentation.rotation_deg = [15, 15, 30]
__C.dataset.augmentation.rotation_prob = 0.7
__C.dataset.augmentation.elastic_grid_mm = 12.0
__C.dataset.augmentation.elastic_magnitude_mm = [0.0, 1.9]
__C.dataset.augmentation.elastic_prob = 0.7
__C.dataset.augmentation.brightness = [0.75, 1.25]
__C.dataset.augmentation.brightness_prob = 0.5
__C.dataset.augmentation.contrast = [0.75, 1.25]
__C.dataset.augmentation.contrast_prob = 0.5
__C.dataset.augmentation.gamma = [0.7, 1.5]
__C.dataset.augmentation.gamma_prob = 0.5
__C.dataset.augmentation.gamma_invert_prob = 0.25
__C.dataset.augmentation.noise_sigma = [0.0, 0.1]
__C.dataset.augmentation.noise_prob = 0.5
__C.loss = {}
__C.loss.name = 'Dice'
__C.loss.obj_weight = [0.5, 0.5]
__C.loss.focal_gamma = 2
__C.net = {}
__C.net.name = 'vnet'
__C.train = {}
__C.train.epochs = 4
__C.train.batchsize = 2
__C.train.num_threads = 0
__C.train.lr = 1e-3
__C.train.betas = (0.9, 0.999)
__C.train.save_epochs = 2
'''


@pytest.mark.parametrize('M', [1, 2])
def test_train_engine_end_to_end_with_augmentation(hip_device, tmp_path, M):
    from oracle import detgen
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import train
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    lines = []
    for k in range(2):
        d = tmp_path / 'c{}'.format(k)
        os.makedirs(str(d), exist_ok=True)
        lab = detgen.labels(800 + k, 'aug/seg{}'.format(k), (48, 48, 48), 2)
        for m in range(M):
            img = (lab.astype(np.float32) * (m + 1) - 0.5 + 0.3 * detgen.normal(810 + 10 * k + m, 'aug/n{}{}'.format(k, m),
                                                                                (48, 48, 48))).astype(np.float32)
            write_mha(Image3d(img, *frame), str(d / 'mod{}.mha'.format(m)))
            lines.append(str(d / 'mod{}.mha'.format(m)))
        write_mha(Image3d(lab.astype(np.int8), *frame), str(d / 'seg.mha'))
        lines.append(str(d / 'seg.mha'))
    (tmp_path / 'train.txt').write_text(('2\n' if M == 1 else '2 {}\n'.format(M)) + '\n'.join(lines) + '\n')
    norms = '[AdaptiveNormalizer()]' if M == 1 else '[AdaptiveNormalizer(), FixedNormalizer(0.5, 2.0, True)]'
    cfg = tmp_path / 'cfg.py'
    cfg.write_text(_TRAIN_CFG % (str(tmp_path / 'train.txt'), str(tmp_path / 'model'), norms))
    try:
        step = train(str(cfg))
    finally:
        _ops.set_activation_dtype('fp32')
    assert step is not None
    log = (tmp_path / 'model' / 'coarse' / 'train_log.txt').read_text().strip().splitlines()
    losses = [float(l.split('train_loss: ')[1].split(',')[0]) for l in log if 'train_loss' in l]
    report('augment_train_e2e_M{}'.format(M), **{'loss_{}'.format(i): v for i, v in enumerate(losses)})
    assert len(losses) == 4 and all(np.isfinite(losses)), losses
