"""Gaussian blur and low-resolution simulation of training crops on the device (DESIGN.md section 7 row f13;
csrc/augment_filter.hip) against the float64 oracles of tests/test_resolution_augment.py.

The bar of both transforms is max |gpu - f64| <= 1e-5 x max |x|, derived, not measured: a blur pass is a convex
combination of at most 13 fp32 products, about 13 x 2^-24 x max |x| = 8e-7 per pass and 2.4e-6 over the three passes (tap
rounding adds 6e-8 relative, and the oracle uses the same float32 taps); the low-resolution simulation has 4 taps per axis
with sum |w| <= 1.25, about 1.5e-6 over the three axes.  Blur followed by the low-resolution simulation stays below
2.4e-6 x 1.25^3 + 1.5e-6 = 6.2e-6, so the data set test keeps the same bar."""
import os

import numpy as np
import pytest
import torch

from gpu_util import report
from test_resolution_augment import oracle_blur, oracle_lowres, oracle_lowres_sizes

pytestmark = pytest.mark.gpu

BAR = 1e-5


def _crop(shape_zyx, M, seed):
    x = np.random.RandomState(seed).randn(*shape_zyx, M).astype(np.float32) * 1.5
    return x[..., 0].copy() if M == 1 else x


def _channels(x):
    return [x] if x.ndim == 3 else [x[..., m] for m in range(x.shape[3])]


def _shifted(x, device):
    """the crop at a base one float past an aligned allocation, and an output buffer shifted the same way"""
    n = int(np.prod(x.shape))
    src = torch.empty(n + 1, dtype=torch.float32, device=device)[1:].view(x.shape)
    dst = torch.empty(n + 1, dtype=torch.float32, device=device)[1:].view(x.shape)
    src.copy_(torch.from_numpy(x))
    assert src.data_ptr() % 8 == 4 and dst.data_ptr() % 8 == 4
    return src, dst


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check(name, fn, x, want, off, device):
    """fn(src, out) -> out on the device; want: per-modality float64 oracle; off: modalities that must come out bit-equal"""
    src = torch.from_numpy(x).to(device)
    got = fn(src, None)
    torch.cuda.synchronize()
    assert torch.equal(src.cpu(), torch.from_numpy(x))                     # the source is untouched
    g = got.cpu().numpy()
    scale = float(np.abs(x).max())
    err = max(float(np.abs(gc.astype(np.float64) - w).max()) for gc, w in zip(_channels(g), want))
    print('{}: max |gpu - f64| = {:.3e} = {:.3e} x max|x|'.format(name, err, err / scale))
    report(name, err=err, rel=err / scale)
    for m in off:
        assert np.array_equal(_channels(g)[m].view(np.int32), _channels(x)[m].view(np.int32)), m
    again = fn(src, None)
    assert torch.equal(_bits(again), _bits(got))                           # two runs
    s_src, s_dst = _shifted(x, device)
    assert torch.equal(_bits(fn(s_src, s_dst)), _bits(got))               # unaligned bases: the scalar path
    assert err <= BAR * scale, (err, scale)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# blur
# ---------------------------------------------------------------------------------------------------------------------
_SIGMAS = {'a': [2.0, 0.0, 0.5, 1.3, 0.34, 1.0, 1.7, 0.8], 'b': [0.5, 0.0, 1.3, 2.0, 1.0, 0.34, 0.8, 1.7],
           'c': [1.3, 0.0, 0.5, 1.0, 2.0, 0.8, 0.34, 1.7]}


@pytest.mark.parametrize('M', [1, 2, 3, 4, 8])
@pytest.mark.parametrize('shape,key', [((5, 7, 9), 'a'), ((1, 1, 17), 'a'), ((17, 16, 33), 'b'), ((17, 16, 33), 'c')])
def test_blur_against_the_oracle(hip_device, shape, key, M):
    from segmentation3d.utils.image_tools import blur_device
    sigmas = _SIGMAS[key][:M]                                                # M >= 2: modality 1 is off
    x = _crop(shape, M, 11)
    want = [oracle_blur(c, s) for c, s in zip(_channels(x), sigmas)]
    _check('blur_{}x{}x{}_{}_M{}'.format(*shape, key, M), lambda src, out: blur_device(src, sigmas, out=out), x, want,
           [m for m, s in enumerate(sigmas) if s == 0.0], hip_device)


def test_blur_value_does_not_depend_on_the_other_modalities(hip_device):
    """channel m of the M = 4 vector path equals the planar run of that channel bit for bit; all off is a copy"""
    from segmentation3d.utils.image_tools import blur_device
    x = _crop((17, 16, 33), 4, 12)
    sigmas = [1.3, 0.0, 0.5, 2.0]
    got = blur_device(torch.from_numpy(x).to(hip_device), sigmas)
    for m, s in enumerate(sigmas):
        one = blur_device(torch.from_numpy(np.ascontiguousarray(x[..., m])).to(hip_device), [s])
        assert torch.equal(_bits(got[..., m]), _bits(one)), m
    src = torch.from_numpy(x).to(hip_device)
    assert torch.equal(_bits(blur_device(src, [0.0, None, 0.0, 0.0])), _bits(src))


# ---------------------------------------------------------------------------------------------------------------------
# low-resolution simulation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [1, 2, 4, 5])
@pytest.mark.parametrize('rot', [0, 1, 2])
@pytest.mark.parametrize('shape', [(5, 7, 9), (16, 16, 16), (1, 8, 33)])
def test_lowres_against_the_oracle(hip_device, shape, rot, M):
    from segmentation3d.utils.image_tools import lowres_device
    z = ([0.5, 0.26, 0.99] * 2)[rot:rot + 3]
    zooms = [z[0], None, z[1], z[2], z[0]][:M]                               # M >= 2: modality 1 is off
    size = shape[::-1]
    x = _crop(shape, M, 21)
    lows = [size if zm is None else oracle_lowres_sizes(size, zm) for zm in zooms]
    want = [oracle_lowres(c, low) for c, low in zip(_channels(x), lows)]
    _check('lowres_{}x{}x{}_r{}_M{}'.format(*shape, rot, M), lambda src, out: lowres_device(src, zooms, out=out), x, want,
           [m for m, low in enumerate(lows) if tuple(low) == tuple(size)], hip_device)


def test_lowres_with_every_size_equal_to_the_crop_is_a_copy(hip_device):
    from segmentation3d.utils.image_tools import lowres_device, lowres_params
    for M in (1, 2, 4, 5):
        x = _crop((5, 7, 9), M, 22)
        src = torch.from_numpy(x).to(hip_device)
        assert torch.equal(_bits(lowres_device(src, [1.0] * M)), _bits(src))
        assert torch.equal(_bits(lowres_device(src, lowres_params([(9, 7, 5)] * M, M))), _bits(src))
    # one axis at full size reproduces that axis: the result equals the oracle with weights (0, 1, 0, 0) there
    x = _crop((5, 7, 9), 1, 23)
    got = lowres_device(torch.from_numpy(x).to(hip_device), lowres_params([(9, 3, 5)], 1)).cpu().numpy()
    assert np.abs(got - oracle_lowres(x, (9, 3, 5))).max() <= BAR * np.abs(x).max()


# ---------------------------------------------------------------------------------------------------------------------
# argument checks, capture
# ---------------------------------------------------------------------------------------------------------------------
def test_entries_refuse_bad_arguments(hip_device):
    from segmentation3d import _engine as E
    from segmentation3d.utils.image_tools import blur_device, blur_params, lowres_device, lowres_params
    x = torch.zeros((4, 5, 6, 2), dtype=torch.float32, device=hip_device)
    flat = torch.zeros(2 * x.numel(), dtype=torch.float32, device=hip_device)
    a, b = flat[:x.numel()].view(x.shape), flat[8:8 + x.numel()].view(x.shape)
    for fn, prm in ((blur_device, [1.0, 1.0]), (lowres_device, [0.5, 0.5])):
        with pytest.raises(ValueError, match='overlap'):
            fn(x, prm, out=x)
        with pytest.raises(ValueError, match='overlap'):
            fn(a, prm, out=b)
        with pytest.raises(ValueError):
            fn(x, prm, out=torch.zeros((4, 5, 6, 1), dtype=torch.float32, device=hip_device))
        with pytest.raises(ValueError):
            fn(x.permute(1, 0, 2, 3), prm)
        with pytest.raises(ValueError):
            fn(x, prm[:1])
        with pytest.raises(ValueError):
            fn(torch.zeros((2, 2, 2, 9), dtype=torch.float32, device=hip_device), prm)
    with pytest.raises(ValueError):
        blur_device(x, [2.5, 1.0])
    with pytest.raises(ValueError):
        lowres_device(x, [0.0, 0.5])
    # the C entries themselves
    out = torch.empty_like(x)
    bp, lp = blur_params([1.0, 1.0], 2), lowres_params([(3, 3, 2)] * 2, 2)
    args = (6, 5, 4, 2)
    for name, prm in (('seg3d_augment_blur', bp), ('seg3d_augment_lowres', lp)):
        with pytest.raises(ValueError, match='overlap'):
            E.call(name, E.ptr(a), E.ptr(b), *args, prm, E.stream_ptr())
        with pytest.raises(ValueError, match='overlap'):
            E.call(name, E.ptr(x), E.ptr(x), *args, prm, E.stream_ptr())
        with pytest.raises(ValueError, match='1..8'):
            E.call(name, E.ptr(x), E.ptr(out), 6, 5, 4, 9, prm, E.stream_ptr())
        with pytest.raises(ValueError):
            E.call(name, E.ptr(x), E.ptr(out), 6, 0, 4, 2, prm, E.stream_ptr())
        with pytest.raises(ValueError):
            E.call(name, None, E.ptr(out), *args, prm, E.stream_ptr())
    bad = blur_params([1.0, 1.0], 2)
    bad.radius[1] = 7
    with pytest.raises(ValueError, match='radius'):
        E.call('seg3d_augment_blur', E.ptr(x), E.ptr(out), *args, bad, E.stream_ptr())
    bad.radius[1] = -1
    with pytest.raises(ValueError, match='radius'):
        E.call('seg3d_augment_blur', E.ptr(x), E.ptr(out), *args, bad, E.stream_ptr())
    for field, m, value in (('nx', 1, 7), ('ny', 0, 6), ('nz', 1, 5), ('nz', 0, 0)):          # n' > n, n' < 1
        bad = lowres_params([(3, 3, 2)] * 2, 2)
        getattr(bad, field)[m] = value
        with pytest.raises(ValueError, match='low grid'):
            E.call('seg3d_augment_lowres', E.ptr(x), E.ptr(out), *args, bad, E.stream_ptr())
    torch.cuda.synchronize()


def test_both_entries_in_one_captured_graph(hip_device):
    from segmentation3d.utils.image_tools import blur_device, lowres_device
    x = torch.from_numpy(_crop((17, 16, 33), 4, 31)).to(hip_device)
    mid, out = torch.empty_like(x), torch.empty_like(x)
    sigmas, zooms = [1.3, 0.0, 0.5, 2.0], [0.5, 0.26, None, 0.99]

    def launches():
        blur_device(x, sigmas, out=mid)
        lowres_device(mid, zooms, out=out)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):          # warm-up on the side stream, as torch.cuda.graph expects
        launches()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    mid.zero_()
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager))


# ---------------------------------------------------------------------------------------------------------------------
# the data set and the train engine
# ---------------------------------------------------------------------------------------------------------------------
_BLUR = {'blur_sigma_vox': [0.5, 1.5], 'blur_prob': 1.0}
_LOWRES = {'lowres_zoom': [0.3, 0.8], 'lowres_prob': 1.0}
_BOTH = dict(_BLUR, **_LOWRES)


def _dataset(tmp_path, M, device, **kw):
    from test_gpu_blend_tta import _write_case
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer, FixedNormalizer
    lst, _ = _write_case(tmp_path, M)
    norms = [AdaptiveNormalizer(), FixedNormalizer(10.0, 90.0, False), None, AdaptiveNormalizer()][:M]
    args = (lst, 3, [1.0, 1.0, 1.2], [32, 24, 16], 'GLOBAL', [3, 3, 3], [0.9, 1.1], 'LINEAR', norms)
    return SegmentationDataset(*args, device=device, **kw)


def _sample(ds, seed, M, device):
    """(crop [z, y, x, M] numpy, mask, frame, the image tensor, the out slot or None, RNG end state)"""
    slot = torch.full((16, 24, 32, M), float('nan'), dtype=torch.float32, device=device) if M > 1 else None
    np.random.seed(seed)
    im, seg, frame, _ = ds.sample(0, out=slot)
    state = np.random.get_state()
    torch.cuda.synchronize()
    return im.permute(1, 2, 3, 0).contiguous().cpu().numpy(), seg.cpu().numpy(), frame, im, slot, state


@pytest.mark.parametrize('M', [1, 4])
@pytest.mark.parametrize('which', ['blur', 'lowres', 'both'])
def test_dataset_crop_equals_the_oracle_on_the_plain_crop(hip_device, tmp_path, M, which):
    section = {'blur': _BLUR, 'lowres': _LOWRES, 'both': _BOTH}[which]
    plain = _dataset(tmp_path, M, hip_device, random_mirror_axes=('y',))
    ds = _dataset(tmp_path, M, hip_device, random_mirror_axes=('y',), resolution_augmentation=section)
    worst = 0.0
    for seed in range(3):
        base, base_seg, base_frame = _sample(plain, seed, M, hip_device)[:3]
        np.random.seed(seed)                                               # the parameters, redrawn from the same seed
        _, sp = ds.sample_crop_geometry(0)
        ds.sample_mirror()
        assert ds.sample_augmentation(sp) is None
        res = ds.sample_resolution_augmentation()
        assert (res['blur'] is not None) == (which != 'lowres') and (res['lowres'] is not None) == (which != 'blur')
        got, seg, frame, im, slot, _ = _sample(ds, seed, M, hip_device)
        assert tuple(im.shape) == (M, 16, 24, 32)
        if M > 1:
            assert im.data_ptr() == slot.data_ptr()                        # the last filter wrote the caller's slot
        assert np.array_equal(seg, base_seg) and np.array_equal(frame, base_frame)
        for m in range(M):
            want = base[..., m].astype(np.float64)
            if res['blur'] is not None:
                want = oracle_blur(want, res['blur'][m])
            if res['lowres'] is not None and res['lowres'][m] is not None:
                want = oracle_lowres(want, res['lowres'][m])
            err = float(np.abs(got[..., m] - want).max()) / float(np.abs(base[..., m]).max())
            print('dataset {} M {} seed {} modality {}: max |gpu - f64| = {:.3e} x max|x|'.format(which, M, seed, m, err))
            worst = max(worst, err)
    report('resolution_dataset_{}_M{}'.format(which, M), rel=worst)
    assert worst <= BAR


@pytest.mark.parametrize('M', [1, 4])
def test_dataset_with_the_section_absent_or_off_is_bit_equal(hip_device, tmp_path, M):
    plain = _dataset(tmp_path, M, hip_device, random_mirror_axes=('y',))
    for section in (None, {}, dict(_BOTH, blur_prob=0.0, lowres_prob=0.0)):
        ds = _dataset(tmp_path, M, hip_device, random_mirror_axes=('y',), resolution_augmentation=section)
        for seed in range(2):
            a, b = _sample(plain, seed, M, hip_device), _sample(ds, seed, M, hip_device)
            assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1], b[1])
            assert np.array_equal(a[2], b[2])
            assert a[5][0] == b[5][0] and np.array_equal(a[5][1], b[5][1]) and a[5][2:] == b[5][2:]


@pytest.mark.parametrize('M', [1, 4])
def test_dataset_with_every_augmentation_on_runs_and_is_finite(hip_device, tmp_path, M):
    from test_gpu_augment import _ALL_ON
    ds = _dataset(tmp_path, M, hip_device, random_mirror_axes=('x', 'z'), augmentation=_ALL_ON, resolution_augmentation=_BOTH)
    for seed in range(2):
        got, seg, _, im, slot, _ = _sample(ds, seed, M, hip_device)
        assert np.isfinite(got).all() and np.isfinite(seg).all()
        assert M == 1 or im.data_ptr() == slot.data_ptr()


_SECTION_CFG = '''
__C.dataset.resolution_augmentation = {}
__C.dataset.resolution_augmentation.blur_sigma_vox = [0.5, 1.5]
__C.dataset.resolution_augmentation.blur_prob = 0.8
__C.dataset.resolution_augmentation.lowres_zoom = [0.5, 1.0]
__C.dataset.resolution_augmentation.lowres_prob = 0.8
'''


@pytest.mark.parametrize('M', [1, 2])
def test_train_engine_runs_with_the_section_on(hip_device, tmp_path, M):
    from oracle import detgen
    from test_gpu_augment import _TRAIN_CFG
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import train
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    lines = []
    for k in range(2):
        d = tmp_path / 'c{}'.format(k)
        os.makedirs(str(d), exist_ok=True)
        lab = detgen.labels(900 + k, 'res/seg{}'.format(k), (48, 48, 48), 2)
        for m in range(M):
            img = (lab.astype(np.float32) * (m + 1) - 0.5 + 0.3 * detgen.normal(910 + 10 * k + m, 'res/n{}{}'.format(k, m),
                                                                                (48, 48, 48))).astype(np.float32)
            write_mha(Image3d(img, *frame), str(d / 'mod{}.mha'.format(m)))
            lines.append(str(d / 'mod{}.mha'.format(m)))
        write_mha(Image3d(lab.astype(np.int8), *frame), str(d / 'seg.mha'))
        lines.append(str(d / 'seg.mha'))
    (tmp_path / 'train.txt').write_text(('2\n' if M == 1 else '2 {}\n'.format(M)) + '\n'.join(lines) + '\n')
    norms = '[AdaptiveNormalizer()]' if M == 1 else '[AdaptiveNormalizer(), FixedNormalizer(0.5, 2.0, True)]'
    text = _TRAIN_CFG.replace('__C.train.epochs = 4', '__C.train.epochs = 2') + _SECTION_CFG
    assert '__C.train.epochs = 2' in text
    cfg = tmp_path / 'cfg.py'
    cfg.write_text(text % (str(tmp_path / 'train.txt'), str(tmp_path / 'model'), norms))
    try:
        step = train(str(cfg))
    finally:
        _ops.set_activation_dtype('fp32')
    assert step is not None
    log = (tmp_path / 'model' / 'coarse' / 'train_log.txt').read_text().strip().splitlines()
    losses = [float(l.split('train_loss: ')[1].split(',')[0]) for l in log if 'train_loss' in l]
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
