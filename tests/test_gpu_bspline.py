"""GPU side of the cubic B-spline interpolation: seg3d_bspline_prefilter_mc and the
seg3d_resample_bspline entries against the float64 oracle of tests/bspline_oracle.py (pinned on the CPU by
tests/test_bspline.py), their exact contracts, and the mode through image_tools, the data set and seg_infer.

Bars.  Every non-exact comparison allows 4 x the error of the fp32 run (the oracle's algorithm with fp32 storage and fp32
arithmetic) against the same float64 oracle on the same input, and at least 1e-6 x max |oracle| -- the convention of
tests/test_gpu_cldice_loss.py.  Each test prints the device error next to the fp32-run error.

Shapes are (X, Y, Z).  The x pass of the prefilter stages tiles of 63 positions (BSP_W) for 256 / M lines per workgroup and
the y / z passes load in batches of 8 after the first sample: 62 / 63 / 64 and 126 / 127 sit below, at and above one and two
tiles, (5, 20, 15) has 300 lines (two workgroups at M = 1), n = 9 / 10 / 17 are one batch, one batch + 1 and two batches;
n = 2 and n = 3 appear on every axis."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bspline_oracle as O
from gpu_util import report
from test_augment import oracle_coords, oracle_control_dims

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 5, 8)
PREFILTER_SHAPES = [(1, 1, 1), (2, 1, 1), (1, 2, 3), (3, 2, 5), (2, 3, 2), (5, 1, 7), (33, 17, 9), (130, 6, 5),
                    (62, 3, 2), (63, 2, 3), (64, 3, 2), (126, 2, 2), (127, 2, 2), (5, 20, 15), (5, 10, 8)]
IDENT = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _samples(shape_xyz, seed=0):
    """[Z, Y, X, 8] float32, uniform in [-1, 1]"""
    X, Y, Z = shape_xyz
    return np.random.RandomState(seed).uniform(-1.0, 1.0, size=(Z, Y, X, 8)).astype(np.float32)


def _step(shape_xyz):
    """a 0 / 1 step across an oblique plane: where the spline overshoots most"""
    X, Y, Z = shape_xyz
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    return (2 * x + y - z > X).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _prefilter_refs(shape_xyz):
    """(float64 oracle, fp32 run) of the 8 channels of _samples"""
    s = _samples(shape_xyz)
    return O.prefilter(s), O.prefilter_recursive(s, np.float32)


def _at(x, shifted, device):
    """x (numpy) on the device at a 16-byte aligned base, or one float past one (the scalar <4> / <2> rows)"""
    flat = torch.empty(x.size + 4, dtype=torch.float32, device=device)[int(shifted):int(shifted) + x.size]
    t = flat.view(x.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert t.data_ptr() % 16 == (4 if shifted else 0)
    return t


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(name, got, fp32_run, oracle, pad=None):
    """pad: the padding value, left out of max |oracle| (the padded voxels themselves are compared like all others)"""
    got = np.asarray(got, dtype=np.float64)
    oracle = np.asarray(oracle, dtype=np.float64)
    assert got.shape == oracle.shape, (got.shape, oracle.shape)
    err = float(np.abs(got - oracle).max())
    err32 = float(np.abs(np.asarray(fp32_run, dtype=np.float64) - oracle).max())
    bar = max(4.0 * err32, 1e-6 * float(np.abs(oracle[oracle != pad] if pad is not None else oracle).max()))
    print('{}: max |device - oracle| = {:.3e}, fp32 run {:.3e}, bar {:.3e}'.format(name, err, err32, bar))
    report('bspline_' + name, err=err, fp32_run=err32, bar=bar)
    assert err <= bar, (name, err, bar)
    return err


def _prefilter(src, dst):
    from segmentation3d import _engine as E
    Z, Y, X = (int(v) for v in src.shape[:3])
    M = int(src.shape[3]) if src.dim() == 4 else 1
    E.call('seg3d_bspline_prefilter_mc', E.ptr(src), E.ptr(dst), X, Y, Z, M, E.stream_ptr())
    return dst


def _evaluate(coef, affine, out_size, pad, dst=None, stride=None, shifted=False):
    """seg3d_resample_bspline_mc on coefficients [Z, Y, X, M] -> [Zo, Yo, Xo, stride] (the gaps keep the sentinel 7.25)"""
    from segmentation3d import _engine as E
    Zi, Yi, Xi, M = (int(v) for v in coef.shape)
    Xo, Yo, Zo = out_size
    stride = M if stride is None else stride
    if dst is None:
        dst = _at(np.full((Zo, Yo, Xo, stride), 7.25, np.float32), shifted, coef.device)
    A = np.ascontiguousarray(affine, dtype=np.float64)
    E.call('seg3d_resample_bspline_mc', E.ptr(coef), E.ptr(dst), M, stride, Xi, Yi, Zi, Xo, Yo, Zo,
           A.ctypes.data_as(ctypes.c_void_p), float(pad), E.stream_ptr())
    return dst


# ---------------------------------------------------------------------------------------------------------------------
# 1. prefilter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', PREFILTER_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_prefilter_against_the_oracle_and_its_exact_contracts(hip_device, shape):
    s = _samples(shape)
    want, run32 = _prefilter_refs(shape)
    planes = []
    for m in range(8):                                                       # the M = 1 call on every plane, once
        p = _at(s[..., m:m + 1], False, hip_device)
        planes.append(_prefilter(p, torch.empty_like(p)))
    for M in WIDTHS:
        for shifted in ((False, True) if M in (2, 4) else (False,)):
            src = _at(s[..., :M], shifted, hip_device)
            keep = src.clone()
            got = _prefilter(src, _at(np.full(src.shape, np.nan, np.float32), shifted, hip_device))
            assert torch.equal(_bits(src), _bits(keep))                      # out of place leaves the source alone
            _check('prefilter_{}_M{}{}'.format('x'.join(map(str, shape)), M, '_shifted' if shifted else ''),
                   got.cpu().numpy(), run32[..., :M], want[..., :M])
            again = _prefilter(src, torch.empty_like(got))
            assert torch.equal(_bits(got), _bits(again))                     # two runs
            inplace = _prefilter(src, src)
            assert torch.equal(_bits(got), _bits(inplace))                   # in place = out of place
            for m in range(M):
                assert torch.equal(_bits(got[..., m]), _bits(planes[m][..., 0])), (M, m)


def test_prefilter_of_a_step_volume(hip_device):
    shape = (33, 17, 9)
    s = _step(shape)
    assert 0.2 < float(s.mean()) < 0.8
    want, run32 = O.prefilter(s), O.prefilter_recursive(s, np.float32)
    assert float(want.max()) > 1.2 and float(want.min()) < -0.2             # the coefficients overshoot the samples
    src = torch.from_numpy(s).to(hip_device)
    _check('prefilter_step', _prefilter(src, torch.empty_like(src)).cpu().numpy(), run32, want)


def test_prefilter_refuses_bad_arguments(hip_device):
    from segmentation3d import _engine as E
    x = torch.zeros((2, 3, 4, 9), dtype=torch.float32, device=hip_device)
    for args in ((4, 3, 2, 9), (4, 3, 2, 0), (0, 3, 2, 1), (4, -1, 2, 1)):
        with pytest.raises(ValueError):
            E.call('seg3d_bspline_prefilter_mc', E.ptr(x), E.ptr(x), *args, E.stream_ptr())
    with pytest.raises(ValueError):
        E.call('seg3d_bspline_prefilter_mc', None, E.ptr(x), 4, 3, 2, 1, E.stream_ptr())


# ---------------------------------------------------------------------------------------------------------------------
# 2. round trip: the interpolant passes through the samples
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['uniform', 'step'])
def test_prefilter_then_identity_evaluation_returns_the_input(hip_device, kind):
    shape = (33, 17, 9)
    s = _samples(shape)[..., :3] if kind == 'uniform' else np.stack([_step(shape)] * 3, -1)
    src = torch.from_numpy(np.ascontiguousarray(s)).to(hip_device)
    coef = _prefilter(src, torch.empty_like(src))
    got = _evaluate(coef, np.eye(3, 4), shape, -3.5)
    coords = O.affine_coords(np.eye(3, 4), shape)
    run32 = O.evaluate(O.prefilter_recursive(s, np.float32), coords, -3.5, np.float32)
    oracle = O.evaluate(O.prefilter(s), coords, -3.5)
    assert float(np.abs(oracle - s).max()) <= 1e-12                          # the oracle's own round trip
    _check('round_trip_' + kind, got.cpu().numpy(), run32, oracle)


# ---------------------------------------------------------------------------------------------------------------------
# 3. evaluation against the oracle: a crop that hangs over two faces of the source
# ---------------------------------------------------------------------------------------------------------------------
SRC = (20, 13, 9)
DST = (17, 11, 7)


def _maps():
    scale = np.zeros((3, 4))
    scale[:, :3] = np.diag([1.3, 1.15, 1.25])
    scale[:, 3] = (-1.2, -0.8, 0.4)
    gx, gy, gz = 0.2, -0.15, 0.3
    Rx = np.array([[1, 0, 0], [0, np.cos(gx), -np.sin(gx)], [0, np.sin(gx), np.cos(gx)]])
    Ry = np.array([[np.cos(gy), 0, np.sin(gy)], [0, 1, 0], [-np.sin(gy), 0, np.cos(gy)]])
    Rz = np.array([[np.cos(gz), -np.sin(gz), 0], [np.sin(gz), np.cos(gz), 0], [0, 0, 1]])
    rot = np.zeros((3, 4))
    rot[:, :3] = (Rz @ Ry @ Rx) * 0.9
    rot[:, 3] = (4.5, -2.25, 1.75)
    return {'scale': scale, 'rotation': rot}


@functools.lru_cache(maxsize=None)
def _eval_refs(which):
    coef = _samples(SRC, seed=2)                                             # the coefficients are the input here
    coords = O.affine_coords(_maps()[which], DST)
    return O.evaluate(coef, coords, -3.5), O.evaluate(coef, coords, -3.5, np.float32), coords


@pytest.mark.parametrize('which', ['scale', 'rotation'])
def test_evaluation_against_the_oracle(hip_device, which):
    want, run32, coords = _eval_refs(which)
    outside = want[..., 0] == -3.5
    assert 0.05 < float(outside.mean()) < 0.8                                # padding where the crop leaves the source,
    # and samples within a voxel of a low and of a high face, where the taps are mirrored
    lows = sum(int(((c >= -0.5) & (c < 1.0)).any()) for c in coords)
    highs = sum(int(((c >= n - 2.0) & (c < n - 0.5)).any()) for c, n in zip(coords, SRC))
    assert lows >= 1 and highs >= 1
    coef = _samples(SRC, seed=2)
    for M, shifted, stride in ((1, False, 1), (3, False, 3), (4, False, 4), (4, True, 4), (8, False, 8), (3, False, 5),
                               (4, False, 8), (2, True, 2), (2, False, 4)):
        got = _evaluate(_at(coef[..., :M], shifted, hip_device), _maps()[which], DST, -3.5, stride=stride, shifted=shifted)
        got = got.cpu().numpy()
        assert np.all(got[..., M:] == 7.25)                                  # the gap floats of a batch slot are untouched
        _check('evaluate_{}_M{}_stride{}{}'.format(which, M, stride, '_shifted' if shifted else ''), got[..., :M],
               run32[..., :M], want[..., :M], pad=-3.5)                      # no voxel is left out
        assert np.array_equal(got[..., 0] == -3.5, outside)                  # the inside test is the oracle's, bitwise


def test_mc_channel_equals_the_planar_entry_bit_for_bit(hip_device):
    from segmentation3d import _engine as E
    coef = _samples(SRC, seed=2)
    A = np.ascontiguousarray(_maps()['rotation'], dtype=np.float64)
    planes = []
    for m in range(8):
        src = torch.from_numpy(np.ascontiguousarray(coef[..., m])).to(hip_device)
        dst = torch.empty((DST[2], DST[1], DST[0]), dtype=torch.float32, device=hip_device)
        E.call('seg3d_resample_bspline', E.ptr(src), E.ptr(dst), SRC[0], SRC[1], SRC[2], DST[0], DST[1], DST[2],
               A.ctypes.data_as(ctypes.c_void_p), -3.5, E.stream_ptr())
        planes.append(dst)
    for M in WIDTHS:
        for shifted in ((False, True) if M in (2, 4) else (False,)):
            got = _evaluate(_at(coef[..., :M], shifted, hip_device), A, DST, -3.5, shifted=shifted)
            again = _evaluate(_at(coef[..., :M], shifted, hip_device), A, DST, -3.5, shifted=shifted)
            assert torch.equal(_bits(got), _bits(again))
            for m in range(M):
                assert torch.equal(_bits(got[..., m]), _bits(planes[m])), (M, shifted, m)


def test_evaluation_refuses_bad_arguments(hip_device):
    coef = torch.zeros((4, 4, 4, 2), dtype=torch.float32, device=hip_device)
    with pytest.raises(ValueError):
        _evaluate(coef, np.eye(3, 4), (4, 4, 4), 0.0, stride=1)              # stride below M
    with pytest.raises(ValueError):
        _evaluate(coef, np.eye(3, 4), (4, 0, 4), 0.0, dst=coef)


# ---------------------------------------------------------------------------------------------------------------------
# 4. deformation and mirror, through image_tools
# ---------------------------------------------------------------------------------------------------------------------
_DSHAPE = (34, 32, 30)                                                       # source, x y z
_DSIZE = (14, 12, 10)
_DSP = (1.1, 0.9, 1.2)
_H = 8.0


def _deform_dst(shift=(0.4, -0.3, 0.2)):
    centre = (np.array(_DSHAPE, dtype=np.float64) - 1) / 2 + np.asarray(shift)
    origin = centre - np.asarray(_DSP) * (np.array(_DSIZE, dtype=np.float64) - 1) / 2
    return (_DSP, tuple(origin), IDENT[2])


def _control(seed, size, dsp, h, a):
    g = oracle_control_dims(size, dsp, h)
    return np.random.RandomState(seed).uniform(-a, a, size=(g[2], g[1], g[0], 3)).astype(np.float32)


@pytest.mark.parametrize('M', [1, 3, 4, 5])
def test_zero_control_grid_is_the_affine_entry_bit_for_bit(hip_device, M):
    from segmentation3d.utils import image_tools as T
    coef = torch.from_numpy(np.ascontiguousarray(_samples(_DSHAPE, seed=3)[..., :M])).to(hip_device)
    zero = torch.zeros(_control(0, _DSIZE, _DSP, _H, 1.0).shape, dtype=torch.float32, device=hip_device)
    for mirror in (None, (True, False, True)):
        for rotation in (None, (0.2, -0.1, 0.3)):
            kw = dict(mirror=mirror, rotation=rotation, prefiltered=True)
            plain = T.resample_device_mc(coef, IDENT, _DSIZE, _deform_dst((14.0, 2.0, -12.0)), 'BSPLINE', -3.5, **kw)
            bent = T.resample_device_mc(coef, IDENT, _DSIZE, _deform_dst((14.0, 2.0, -12.0)), 'BSPLINE', -3.5,
                                        deform=(zero, _H), **kw)
            assert torch.equal(_bits(plain), _bits(bent)), (mirror, rotation)
            assert 0.02 < float((plain == -3.5).float().mean()) < 0.9        # the shifted crop leaves the source


@pytest.mark.parametrize('M', [1, 4])
def test_rotated_deformed_crop_against_the_oracle(hip_device, M):
    from segmentation3d.utils import image_tools as T
    mag = 1.2                                                                # mm = source voxels here; below h / 6
    rotation, mirror = (0.1, -0.1, 0.15), (False, True, False)
    ctrl = _control(5, _DSIZE, _DSP, _H, mag)
    coef = np.ascontiguousarray(_samples(_DSHAPE, seed=3)[..., :M])
    dst = _deform_dst()
    got = T.resample_device_mc(torch.from_numpy(coef).to(hip_device), IDENT, _DSIZE, dst, 'BSPLINE', -3.5, mirror=mirror,
                               rotation=rotation, deform=(torch.from_numpy(ctrl).to(hip_device), _H), prefiltered=True)
    c = oracle_coords(IDENT, dst, _DSIZE, rotation, ctrl, _H, mirror)
    plain = oracle_coords(IDENT, dst, _DSIZE, rotation, None, None, mirror)
    assert float(np.abs(c - plain).max()) > 0.2                             # the field moves the sample points
    for r, n in enumerate(_DSHAPE):                                          # magnitude + 3 voxels inside: nothing excluded
        assert float(c[r].min()) >= mag + 3 and float(c[r].max()) <= n - 1 - (mag + 3)
    coords = (c[0], c[1], c[2])
    _check('deform_M{}'.format(M), got.cpu().numpy(), O.evaluate(coef, coords, -3.5, np.float32),
           O.evaluate(coef, coords, -3.5))


@pytest.mark.parametrize('deformed', [False, True])
def test_mirrored_crop_is_the_flip_of_the_plain_crop_bit_for_bit(hip_device, deformed):
    """dyadic spacings and origins: the mirrored index map is exact in double, so the coordinates agree bit for bit"""
    from segmentation3d.utils import image_tools as T
    size, dsp = (12, 10, 8), (0.75, 1.25, 0.5)
    dst = (dsp, (-1.625, 2.5, 3.375), IDENT[2])
    coef = torch.from_numpy(np.ascontiguousarray(_samples(SRC, seed=2)[..., :2])).to(hip_device)
    deform = None
    if deformed:
        deform = (torch.from_numpy(_control(9, size, dsp, 8.0, 1.0)).to(hip_device), 8.0)
    plain = T.resample_device_mc(coef, IDENT, size, dst, 'BSPLINE', -3.5, deform=deform, prefiltered=True)
    assert 0.02 < float((plain == -3.5).float().mean()) < 0.9
    for mask in range(1, 8):
        mirror = tuple(bool(mask >> a & 1) for a in range(3))
        got = T.resample_device_mc(coef, IDENT, size, dst, 'BSPLINE', -3.5, mirror=mirror, deform=deform, prefiltered=True)
        dims = [2 - a for a in range(3) if mirror[a]]
        assert torch.equal(_bits(got), _bits(torch.flip(plain, dims))), mirror


# ---------------------------------------------------------------------------------------------------------------------
# 5. the Python layers
# ---------------------------------------------------------------------------------------------------------------------
def test_image_tools_bspline_is_prefilter_plus_prefiltered_evaluation(hip_device):
    from segmentation3d.utils import image_tools as T
    s = torch.from_numpy(np.ascontiguousarray(_samples(SRC, seed=4)[..., :3])).to(hip_device)
    frame = ((0.8, 1.1, 1.7), (-12.0, 5.0, 30.0), IDENT[2])
    dst = ((1.0, 0.9, 1.3), (-11.0, 6.0, 31.0), IDENT[2])
    keep = s.clone()
    got = T.resample_device_mc(s, frame, DST, dst, 'BSPLINE', -1.0)
    assert torch.equal(s, keep)                                              # the samples are prefiltered into a temporary
    coef = T.bspline_prefilter_device(s)
    assert torch.equal(_bits(got), _bits(T.resample_device_mc(coef, frame, DST, dst, 'BSPLINE', -1.0, prefiltered=True)))
    assert float((got - T.resample_device_mc(s, frame, DST, dst, 'LINEAR', -1.0)).abs().max()) > 1e-2
    # planar volumes and crops are the M = 1 case
    one = T.resample_device(s[..., 1].contiguous(), frame, DST, dst, 'BSPLINE', -1.0)
    assert torch.equal(_bits(one), _bits(got[..., 1]))
    centre, spacing = (-2.0, 12.0, 37.0), (1.0, 0.9, 1.3)
    crop = T.crop_image_device_mc(coef, frame, centre, DST, spacing, 'BSPLINE', prefiltered=True)
    assert torch.equal(_bits(crop[..., 2]), _bits(T.crop_image_device(s[..., 2].contiguous(), frame, centre, DST, spacing,
                                                                     'BSPLINE')))
    # in place, 3-D input, and the checks
    x = s[..., 0].contiguous()
    assert torch.equal(_bits(T.bspline_prefilter_device(x, out=x)), _bits(coef[..., 0]))
    with pytest.raises(ValueError):
        T.bspline_prefilter_device(s, out=torch.empty((1, 2, 3), device=hip_device))
    with pytest.raises(ValueError):
        T.bspline_prefilter_device(s.double())


def _two_cases(tmp_path):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    frame = ((1.0, 1.1, 0.9), (-4.0, 2.0, 7.0), IDENT[2])
    rng = np.random.RandomState(21)
    lines = []
    for k in range(2):
        d = tmp_path / 'case{}'.format(k)
        d.mkdir()
        for m in range(2):
            write_mha(Image3d(rng.uniform(-1, 1, size=(24, 24, 24)).astype(np.float32), *frame), str(d / 'im{}.mha'.format(m)))
            lines.append(str(d / 'im{}.mha'.format(m)))
        write_mha(Image3d((rng.rand(24, 24, 24) > 0.6).astype(np.int8), *frame), str(d / 'seg.mha'))
        lines.append(str(d / 'seg.mha'))
    (tmp_path / 'train.txt').write_text('2 2\n' + '\n'.join(lines) + '\n')
    return str(tmp_path / 'train.txt')


def test_dataset_bspline_crops(hip_device, tmp_path, monkeypatch):
    from segmentation3d import _engine as E
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils import image_tools as T
    from segmentation3d.utils.normalizer import AdaptiveNormalizer, FixedNormalizer
    lst = _two_cases(tmp_path)
    aug = {'rotation_deg': [15.0, 10.0, 20.0], 'rotation_prob': 1.0, 'elastic_grid_mm': 8.0,
           'elastic_magnitude_mm': [0.5, 1.0], 'elastic_prob': 1.0}

    def dataset(interp):
        return SegmentationDataset(lst, 2, [1.0, 1.0, 1.0], [16, 16, 16], 'GLOBAL', [2, 2, 2], [0.9, 1.1], interp,
                                   [AdaptiveNormalizer(), FixedNormalizer(0.1, 0.7, False)], device=hip_device,
                                   random_mirror_axes=('x', 'y', 'z'), augmentation=aug)
    calls = []
    real = E.call
    monkeypatch.setattr(E, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    order = [0, 1, 1, 0]
    runs = {}
    for interp in ('LINEAR', 'BSPLINE'):
        ds = dataset(interp)
        np.random.seed(17)
        del calls[:]
        runs[interp] = ([ds.sample(i) for i in order], list(calls), ds)
    lin, lin_calls, ds_lin = runs['LINEAR']
    bsp, bsp_calls, ds_bsp = runs['BSPLINE']
    # the LINEAR run launches what it launched before: per sample the deform crop of the image, the normaliser, the NN
    # deform crop of the mask -- and nothing of the spline
    assert not any('bspline' in c for c in lin_calls)
    assert [c for c in lin_calls if 'resample' in c] == ['seg3d_resample_deform_mc'] * (2 * len(order))
    assert len(lin_calls) >= 3 * len(order)
    # the BSPLINE run: one prefilter per case at load, then per sample the same launches with the spline entry first
    assert bsp_calls.count('seg3d_bspline_prefilter_mc') == 2
    rest = [c for c in bsp_calls if c != 'seg3d_bspline_prefilter_mc']
    assert [c for c in rest if 'resample' in c] == ['seg3d_resample_bspline_deform_mc', 'seg3d_resample_deform_mc'] * len(order)
    assert [c for c in rest if 'resample' not in c] == [c for c in lin_calls if 'resample' not in c]
    assert len(rest) == len(lin_calls)
    mirrors = set()
    for (im_l, seg_l, frame_l, name_l), (im_b, seg_b, frame_b, name_b) in zip(lin, bsp):
        assert name_l == name_b and np.array_equal(frame_l, frame_b) and torch.equal(_bits(seg_l), _bits(seg_b))
        assert float((im_l - im_b).abs().max()) > 1e-3
    # the image crops are the image_tools composition on the raw volume: replay the draws of the seeded run
    np.random.seed(17)
    for k, i in enumerate(order):
        raw = ds_lin.case(i).volume
        assert torch.equal(_bits(T.bspline_prefilter_device(raw)), _bits(ds_bsp.case(i).volume))
        centre, spacing = ds_bsp.sample_crop_geometry(i)
        mirror = ds_bsp.sample_mirror()
        a = ds_bsp.sample_augmentation(spacing)
        assert ds_bsp.sample_resolution_augmentation() is None
        mirrors.add(mirror)
        assert a['rotation'] is not None and a['control'] is not None
        want = T.crop_image_device_mc(raw, ds_bsp.case(i).frame, centre, ds_bsp.crop_size, spacing, 'BSPLINE', mirror=mirror,
                                      rotation=a['rotation'], deform=(torch.from_numpy(a['control']).to(hip_device), 8.0))
        want = T.normalize_crop_device_mc(want, ds_bsp._norm_params, out=want).permute(3, 0, 1, 2)
        assert torch.equal(_bits(bsp[k][0]), _bits(want)), k
    assert len(mirrors) > 1
    # straight into a batch slot
    batch = torch.full((2, 16, 16, 16, 2), 7.25, dtype=torch.float32, device=hip_device)
    np.random.seed(17)
    im, _, _, _ = ds_bsp.sample(0, out=batch[1])
    assert im.data_ptr() == batch[1].data_ptr() and torch.equal(_bits(im), _bits(bsp[0][0]))
    assert bool((batch[0] == 7.25).all())


def _kaiming_vnet(seed=9):
    from segmentation3d.network import vnet
    torch.manual_seed(seed)
    net = vnet.SegmentationNet(1, 2)
    vnet.parameters_kaiming_init(net)
    return net.eval()


class _Stage(object):
    partition_type = 'SIZE'
    partition_size = [32, 32, 32]
    partition_stride = [16, 16, 16]


def test_segmentation_volume_with_a_bspline_checkpoint(hip_device, tmp_path, monkeypatch):
    from segmentation3d.core.seg_infer import load_single_model, segmentation_volume
    from segmentation3d.utils import image_tools as T
    from segmentation3d.utils.image3d import Image3d
    chk = tmp_path / 'fine' / 'checkpoints' / 'chk_5'
    chk.mkdir(parents=True)
    torch.save({'epoch': 5, 'batch': 1, 'net': 'vnet', 'max_stride': 16, 'state_dict': _kaiming_vnet().state_dict(),
                'spacing': [1.0, 1.0, 1.0], 'interpolation': 'BSPLINE', 'in_channels': 1, 'out_channels': 2,
                'crop_normalizers': [{'type': 1, 'clip_sigma': 3}]}, str(chk / 'params.pth'))
    model = load_single_model(str(tmp_path / 'fine'), 0)
    vol = np.random.RandomState(31).uniform(-1, 1, size=(40, 40, 40)).astype(np.float32)
    frame = ((0.8, 0.7, 0.75), (-20.0, 5.0, 12.5), IDENT[2])
    seen = []
    real = T.resample_device_mc

    def spy(src, src_frame, out_size, dst_frame, interp_method, *a, **kw):
        out = real(src, src_frame, out_size, dst_frame, interp_method, *a, **kw)
        seen.append((interp_method, tuple(out_size), dst_frame, out.clone()))
        return out
    monkeypatch.setattr(T, 'resample_device_mc', spy)
    probs, mask = segmentation_volume(model, _Stage, Image3d(vol, *frame), None, None, True, batch_size=4)
    assert mask.array.shape == (40, 40, 40) and mask.array.dtype == np.int8
    assert len(probs) == 2 and np.isfinite(probs[1].array).all()
    assert [s[0] for s in seen] == ['BSPLINE']
    _, size, iso, prepared = seen[0]
    assert size == (32, 32, 32)
    coords = O.affine_coords(T.index_affine(frame, iso), size)
    _check('seg_infer_prepared_volume', prepared[..., 0].cpu().numpy(),
           O.evaluate(O.prefilter_recursive(vol, np.float32), coords, 0.0, np.float32), O.evaluate(O.prefilter(vol), coords, 0.0),
           pad=0.0)


def test_train_from_a_bspline_config_then_segment(hip_device, tmp_path, monkeypatch):
    """dataset.interpolation = 'BSPLINE' in a train config trains, and the checkpoint runs through segmentation() with no
    other key changed"""
    from segmentation3d import _engine as E
    from segmentation3d import _ops
    from segmentation3d.core.seg_infer import segmentation
    from segmentation3d.core.seg_train import train
    from test_gpu_multimodal import _TRAIN_CFG, _SEG_CFG, _e2e_cases
    cases, frame = _e2e_cases(tmp_path)
    text = _TRAIN_CFG % (str(tmp_path / 'train.txt'), str(tmp_path / 'model'), '')
    assert text.count("interpolation = 'LINEAR'") == 1
    cfg = tmp_path / 'cfg.py'
    cfg.write_text(text.replace("interpolation = 'LINEAR'", "interpolation = 'BSPLINE'"))
    calls = []
    real = E.call
    monkeypatch.setattr(E, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    try:
        train(str(cfg))
    finally:
        _ops.set_activation_dtype('fp32')
    log = (tmp_path / 'model' / 'coarse' / 'train_log.txt').read_text().strip().splitlines()
    losses = [float(l.split('train_loss: ')[1].split(',')[0]) for l in log if 'train_loss' in l]
    assert len(losses) == 4 and all(np.isfinite(losses)), losses
    assert calls.count('seg3d_bspline_prefilter_mc') == 2                    # once per case, at load
    assert calls.count('seg3d_resample_bspline_mc') == 8                     # 4 batches of 2 image crops
    state = torch.load(str(tmp_path / 'model' / 'coarse' / 'checkpoints' / 'chk_2' / 'params.pth'), weights_only=True)
    assert state['interpolation'] == 'BSPLINE'
    (tmp_path / 'model' / 'infer_config.py').write_text(_SEG_CFG)
    (tmp_path / 'test.txt').write_text('1\ncase1 {}\n'.format(' '.join(cases[1][0])))
    del calls[:]
    mask = segmentation(str(tmp_path / 'test.txt'), str(tmp_path / 'model'), str(tmp_path / 'out'), 'seg.mha', 0, True, True,
                        True, True)[0]
    assert mask.array.shape == (48, 48, 48)
    assert calls.count('seg3d_bspline_prefilter_mc') == 1 and calls.count('seg3d_resample_bspline_mc') == 1
