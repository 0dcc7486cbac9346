"""GPU end-to-end checks of the case-level normalisers: a SegmentationDataset with VolumeNormalizer samples exactly what the
un-normalised sample gives through the type-3 kernel path with numpy's numbers for the case; inference with a type-2
checkpoint equals inference with the hand-resolved type-3 dict; the data-set fingerprint equals numpy over the pooled
foreground voxels."""
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_volume_stats import _ulps32

pytestmark = pytest.mark.gpu

IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
_SHAPES = [(24, 28, 32), (30, 26, 22)]                        # [z, y, x]
_FRAMES = [((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), IDENT), ((0.9, 1.1, 1.0), (-4.0, 2.0, 1.5), IDENT)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _case_arrays(k, M=2):
    """an MRI-like case: per modality a smooth 'head' of positive intensities in a background of exact zeros"""
    rng = np.random.RandomState(70 + k)
    shape = _SHAPES[k]
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing='ij')
    head = (x * x + y * y + z * z) < 0.8
    planes = np.stack([(rng.normal(300.0 + 150.0 * m, 60.0 + 25.0 * m, size=shape) * head) for m in range(M)])
    seg = (rng.randint(0, 3, size=shape) * head).astype(np.int8)
    return planes.astype(np.float32), seg


def _write_cases(folder, M=2):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    lines, cases = ['2 {}'.format(M)], []
    for k in range(2):
        planes, seg = _case_arrays(k, M)
        d = folder / 'case{}'.format(k)
        os.makedirs(str(d), exist_ok=True)
        for m in range(M):
            write_mha(Image3d(planes[m], *_FRAMES[k]), str(d / 'mod{}.mha'.format(m)))
            lines.append(str(d / 'mod{}.mha'.format(m)))
        write_mha(Image3d(seg, *_FRAMES[k]), str(d / 'seg.mha'))
        lines.append(str(d / 'seg.mha'))
        cases.append((planes, seg))
    lst = folder / 'train.txt'
    lst.write_text('\n'.join(lines) + '\n')
    return str(lst), cases


def _dataset(lst, norms, interp, device):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    return SegmentationDataset(lst, 3, [1.0, 1.0, 1.0], [16, 16, 16], 'GLOBAL', [2, 2, 2], [0.9, 1.1], interp, norms,
                               device=device)


def _draw(ds, seed):
    np.random.seed(seed)
    out = [ds[i] for i in (0, 1, 1, 0)]
    return out, np.random.get_state()


def _nonzero_type3(plane, pct=None):
    """numpy's numbers of one modality: float64 moments of the (clipped) non-zero voxels, nearest-rank percentiles"""
    v = np.sort(plane[plane != 0]).astype(np.float64)
    lower = upper = None
    if pct is not None:
        lower = v[int(math.floor(pct[0] / 100.0 * (v.size - 1) + 0.5))]
        upper = v[int(math.floor(pct[1] / 100.0 * (v.size - 1) + 0.5))]
        v = np.clip(v, lower, upper)
    return {'type': 3, 'mean': float(v.mean()), 'stddev': float(v.std()), 'lower': lower, 'upper': upper}


@pytest.mark.parametrize('interp', ['LINEAR', 'BSPLINE'])
def test_dataset_sample_equals_the_type3_path_with_numpy_numbers(hip_device, tmp_path, interp):
    """with 'BSPLINE' the resident tensor holds coefficients: the statistics must have been taken from the samples"""
    from segmentation3d.utils import image_tools as T
    from segmentation3d.utils.normalizer import AdaptiveNormalizer, VolumeNormalizer
    lst, cases = _write_cases(tmp_path)
    got, state_v = _draw(_dataset(lst, [VolumeNormalizer(), VolumeNormalizer()], interp, hip_device), 5)
    raw, state_n = _draw(_dataset(lst, [None, None], interp, hip_device), 5)
    ada, state_a = _draw(_dataset(lst, [AdaptiveNormalizer(), AdaptiveNormalizer()], interp, hip_device), 5)
    for k, index in enumerate((0, 1, 1, 0)):
        dicts = [_nonzero_type3(cases[index][0][m]) for m in range(2)]
        crop = raw[k][0].permute(1, 2, 3, 0).contiguous()
        want = T.normalize_crop_device_mc(crop, T.normalizer_params(dicts, 2)).permute(3, 0, 1, 2)
        assert got[k][0].shape == (2, 16, 16, 16)
        assert torch.equal(_bits(got[k][0]), _bits(want)), k
        assert not torch.equal(_bits(got[k][0]), _bits(ada[k][0])), k
        assert torch.equal(got[k][1], ada[k][1]) and np.array_equal(got[k][2], ada[k][2]) and got[k][3] == ada[k][3]
    for a, b in ((state_v, state_a), (state_v, state_n)):
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_dataset_keeps_one_struct_per_case_and_the_old_path_without_type2(hip_device, tmp_path):
    from segmentation3d.utils.normalizer import AdaptiveNormalizer, VolumeNormalizer
    lst, cases = _write_cases(tmp_path)
    mixed = _dataset(lst, [VolumeNormalizer('nonzero', (1, 99), 4), AdaptiveNormalizer()], 'LINEAR', hip_device)
    assert mixed._norm_params is None
    c0, c1 = mixed.case(0), mixed.case(1)
    assert [d['type'] if isinstance(d, dict) else d.to_dict()['type'] for d in c0.normalizers] == [3, 1]
    assert c0.norm_params.n[0].type == 0 and c0.norm_params.n[1].type == 1
    assert c0.norm_params.n[0].mean != c1.norm_params.n[0].mean
    want = _nonzero_type3(cases[0][0][0], (1, 99))
    assert c0.normalizers[0]['lower'] == max(want['lower'], c0.normalizers[0]['mean'] - 4 * c0.normalizers[0]['stddev'])
    plain = _dataset(lst, [AdaptiveNormalizer(), None], 'LINEAR', hip_device)
    assert plain._norm_params is not None and plain.case(0).norm_params is None


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


def test_segmentation_volume_with_a_type2_checkpoint(hip_device, tmp_path):
    from segmentation3d.core.seg_infer import load_single_model, segmentation_volume, sliding_window_inference
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.normalizer import VolumeNormalizer
    type2 = VolumeNormalizer('nonzero', (0.5, 99.5)).to_dict()
    chk = tmp_path / 'fine' / 'checkpoints' / 'chk_5'
    chk.mkdir(parents=True)
    torch.save({'epoch': 5, 'batch': 1, 'net': 'vnet', 'max_stride': 16, 'state_dict': _kaiming_vnet().state_dict(),
                'spacing': [1.0, 1.0, 1.0], 'interpolation': 'LINEAR', 'in_channels': 1, 'out_channels': 2,
                'crop_normalizers': [type2]}, str(chk / 'params.pth'))
    model = load_single_model(str(tmp_path / 'fine'), 0)
    assert model['crop_normalizer_dicts'] == [type2] and isinstance(model['crop_normalizers'][0], VolumeNormalizer)
    rng = np.random.RandomState(12)
    z, y, x = np.meshgrid(*[np.linspace(-1, 1, 32)] * 3, indexing='ij')
    vol = (rng.normal(400.0, 120.0, size=(32, 32, 32)) * ((x * x + y * y + z * z) < 0.9)).astype(np.float32)
    image = Image3d(vol, (1.0, 1.0, 1.0), (3.0, -2.0, 5.0), IDENT)

    def run(dicts):
        m = dict(model)
        m['crop_normalizer_dicts'] = dicts
        probs, mask = segmentation_volume(m, _Stage, image, None, None, True, batch_size=2)
        return np.stack([p.array for p in probs]), mask.array

    got, got_mask = run([type2])
    assert got.shape == (2, 32, 32, 32) and np.isfinite(got).all()
    want, want_mask = run([_nonzero_type3(vol, (0.5, 99.5))])
    assert np.array_equal(got.view(np.int32), want.view(np.int32)) and np.array_equal(got_mask, want_mask)
    adaptive, _ = run([{'type': 1, 'clip_sigma': 3}])
    assert not np.array_equal(got, adaptive)              # a silently ignored normaliser would pass the line above
    # the sliding window itself takes resolved lists only
    with pytest.raises(ValueError, match='resolve'):
        sliding_window_inference(model['net'], torch.from_numpy(vol).to(hip_device).unsqueeze(3), [[0, 0, 0]], (32, 32, 32), 2,
                                 [type2], batch_size=1, use_graph=False)


def test_intensity_fingerprint_equals_numpy_over_the_pooled_foreground(hip_device, tmp_path):
    from segmentation3d.dataloader.dataset import intensity_fingerprint
    from segmentation3d.seg_fingerprint import format_lines
    from segmentation3d.utils.normalizer import ClipZScoreNormalizer
    lst, cases = _write_cases(tmp_path)
    for resident_bytes in (8 << 30, 0):                    # resident, and re-read per pass
        stats = intensity_fingerprint(lst, (0.5, 99.5), hip_device, resident_bytes=resident_bytes)
        assert len(stats) == 2
        for m, st in enumerate(stats):
            pooled = np.sort(np.concatenate([planes[m][seg > 0] for planes, seg in cases])).astype(np.float64)
            lo = pooled[int(math.floor(0.005 * (pooled.size - 1) + 0.5))]
            hi = pooled[int(math.floor(0.995 * (pooled.size - 1) + 0.5))]
            assert st['n'] == pooled.size and st['lower'] == lo and st['upper'] == hi
            assert st['min'] == pooled[0] and st['max'] == pooled[-1]
            c = np.clip(pooled, lo, hi)
            assert _ulps32(st['mean'], c.mean()) <= 1 and _ulps32(st['std'], c.std()) <= 1
            assert st['normalizer'].to_dict() == ClipZScoreNormalizer(st['mean'], st['std'], lo, hi).to_dict()
    lines = format_lines(stats)
    assert len(lines) == 4 and lines[0].startswith('# modality 0: n = ')
    pasted = eval(lines[1], {'ClipZScoreNormalizer': ClipZScoreNormalizer})
    assert pasted.to_dict() == stats[0]['normalizer'].to_dict()


def test_intensity_fingerprint_rejects_a_mask_of_another_size(hip_device, tmp_path):
    from segmentation3d.dataloader.dataset import intensity_fingerprint
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    lst, _ = _write_cases(tmp_path)
    write_mha(Image3d(np.ones((5, 6, 7), np.int8), *_FRAMES[1]), str(tmp_path / 'case1' / 'seg.mha'))
    with pytest.raises(ValueError, match='case1'):
        intensity_fingerprint(lst, (0.5, 99.5), hip_device)
