"""On-device training augmentation on one GPU (prints one JSON line; --out FILE also writes it).  All variants of a group
are alternated in one process after a warm-up; every figure is the median with [min, max] over the repeats.
  (i)   per sample, 96^3 x 1 and 96^3 x 4, file-backed SegmentationDataset.sample(): the plain path (crop + normalise, no
        augmentation section -- the baseline, timed in the same run) against spatial only (rotation + elastic), intensity
        only (brightness, contrast, gamma, noise) and everything on; host clock around a block of samples that ends in a
        device synchronise (a sample includes its host work: RNG draws, index maps, the control tensor's upload);
  (ii)  the launches alone on a resident 96^3 x M crop, device events around a block of launches: affine against deformed
        resampling, the intensity entry with the statistics passes (contrast + gamma) and without (brightness + noise),
        and a device-to-device copy of the crop as the yardstick (apply = one read + one write = the copy's bytes, the
        statistics pass = one read = half of them);
  (iii) the vnet(M, 4) 4 x 96^3 eager train step fed by the file-backed dataset without and with full augmentation.
usage: python tools/bench_augment.py [--repeats R] [--steps K] [--skip-train] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'medical-segmentation3d-toolkit_amd'))
sys.path.insert(0, REPO)

SPATIAL = {'rotation_deg': [30, 30, 30], 'rotation_prob': 1.0, 'elastic_grid_mm': 32.0, 'elastic_magnitude_mm': [0.0, 4.0],
           'elastic_prob': 1.0}
INTENSITY = {'brightness': [0.75, 1.25], 'brightness_prob': 1.0, 'contrast': [0.75, 1.25], 'contrast_prob': 1.0,
             'gamma': [0.7, 1.5], 'gamma_prob': 1.0, 'gamma_invert_prob': 0.25, 'noise_sigma': [0.0, 0.1], 'noise_prob': 1.0}
VARIANTS = [('plain', None), ('spatial', SPATIAL), ('intensity', INTENSITY), ('all', dict(SPATIAL, **INTENSITY))]


def _stat(values):
    v = sorted(values)
    return {'median': v[len(v) // 2], 'min': v[0], 'max': v[-1]}


def _write_cases(M):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    tmp = tempfile.mkdtemp(prefix='aug_bench_')
    rng = np.random.RandomState(1)
    lines = []
    for k in range(2):
        seg = (rng.rand(128, 144, 160) > 0.7).astype(np.int8) * (1 + k)
        for m in range(M):
            p = os.path.join(tmp, 'c{}_m{}.mha'.format(k, m))
            write_mha(Image3d((rng.randn(128, 144, 160) * 50 + 10 * m).astype(np.float32)), p)
            lines.append(p)
        p = os.path.join(tmp, 'c{}_seg.mha'.format(k))
        write_mha(Image3d(seg), p)
        lines.append(p)
    lst = os.path.join(tmp, 'train.txt')
    with open(lst, 'w') as f:
        f.write(('2\n' if M == 1 else '2 {}\n'.format(M)) + '\n'.join(lines) + '\n')
    return lst


def _dataset(lst, M, dev, aug):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    return SegmentationDataset(lst, 4, [1.0, 1.0, 1.0], [96, 96, 96], 'GLOBAL', [5, 5, 5], [0.9, 1.1], 'LINEAR',
                               [AdaptiveNormalizer()] * M, device=dev, augmentation=aug)


def per_sample(lst, M, dev, repeats, block=20):
    sets = {name: _dataset(lst, M, dev, aug) for name, aug in VARIANTS}
    np.random.seed(0)
    for ds in sets.values():
        for k in range(4):
            ds.sample(k % 2)
    torch.cuda.synchronize()
    times = {name: [] for name in sets}
    for _ in range(repeats):
        for name, ds in sets.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(block):
                ds.sample(k % 2)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / block * 1e3)
    return {name: _stat(v) for name, v in times.items()}


def _events_ms(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps


def launches(M, dev, repeats, reps=50):
    from segmentation3d.utils import image_tools as T
    vol = torch.randn((128, 144, 160) + ((M,) if M > 1 else ()), device=dev)
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    size, sp, centre, h = (96, 96, 96), (1.05, 1.05, 1.05), (80.0, 72.0, 64.0), 32.0
    g = T.bspline_control_dims(size, sp, h)
    ctrl = torch.from_numpy(np.random.RandomState(0).uniform(-4, 4, size=(g[2], g[1], g[0], 3)).astype(np.float32)).to(dev)
    crop = torch.empty((96, 96, 96) + ((M,) if M > 1 else ()), dtype=torch.float32, device=dev)
    src = torch.randn_like(crop).clamp_(-1, 1)
    other = torch.empty_like(crop)
    rot = (0.3, -0.2, 0.4)
    crop_fn = T.crop_image_device if M == 1 else T.crop_image_device_mc
    with_stats = T.intensity_params([{'brightness': 1.1, 'contrast': 1.2, 'gamma': 1.3, 'sigma': 0.05}] * M, M, 7)
    no_stats = T.intensity_params([{'brightness': 1.1, 'sigma': 0.05}] * M, M, 7)
    apply_only = T.intensity_params([{'brightness': 1.1}] * M, M, 7)
    fns = {
        'resample_affine': lambda: crop_fn(vol, frame, centre, size, sp, 'LINEAR', rotation=rot),
        'resample_deform': lambda: crop_fn(vol, frame, centre, size, sp, 'LINEAR', rotation=rot, deform=(ctrl, h)),
        'intensity_all_with_stats': lambda: T.augment_intensity_device(crop, with_stats),
        'intensity_brightness_noise': lambda: T.augment_intensity_device(crop, no_stats),
        'intensity_brightness_only': lambda: T.augment_intensity_device(crop, apply_only),
        'copy_d2d': lambda: other.copy_(crop),
    }
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            crop.copy_(src)                      # the in-place transforms start from the same normalised crop
            torch.cuda.synchronize()
            times[name].append(_events_ms(fn, reps) * 1e3)
    out = {name + '_us': _stat(v) for name, v in times.items()}
    copy = out['copy_d2d_us']['median']
    out['crop_bytes'] = int(crop.numel() * 4)
    out['stats_pass_us_by_difference'] = out['intensity_all_with_stats_us']['median'] - out['intensity_brightness_noise_us']['median']
    out['apply_brightness_only_over_copy'] = out['intensity_brightness_only_us']['median'] / copy
    out['apply_brightness_noise_over_copy'] = out['intensity_brightness_noise_us']['median'] / copy
    out['all_with_stats_over_copy'] = out['intensity_all_with_stats_us']['median'] / copy
    out['deform_over_affine'] = out['resample_deform_us']['median'] / out['resample_affine_us']['median']
    return out


def train_steps(lst, M, dev, steps, repeats):
    from segmentation3d.core.seg_train import TrainStep
    from segmentation3d.dataloader.dataset import DeviceCropLoader
    step = TrainStep('vnet', M, 4, 'Dice', [0.25] * 4, device=dev, seed=0)
    sets = {'plain': _dataset(lst, M, dev, None), 'all': _dataset(lst, M, dev, dict(SPATIAL, **INTENSITY))}
    np.random.seed(0)
    total = 3 + repeats * steps
    loaders = {name: iter(DeviceCropLoader(ds, [k % 2 for k in range(4 * total)], 4)) for name, ds in sets.items()}
    for name in sets:
        for _ in range(3):
            crops, masks, _, _ = next(loaders[name])
            step(crops, masks)
    torch.cuda.synchronize()
    times = {name: [] for name in sets}
    for _ in range(repeats):
        for name in sets:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                crops, masks, _, _ = next(loaders[name])
                step(crops, masks)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    return {name: _stat(v) for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--skip-train', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from segmentation3d import _engine
    _engine.lib()
    if not torch.cuda.is_available():
        raise SystemExit('bench_augment.py needs a ROCm device')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    r = {'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'unit_per_sample': 'ms', 'unit_launches': 'us',
         'unit_train_step': 'ms'}
    for M in (1, 4):
        lst = _write_cases(M)
        r['per_sample_96^3x{}'.format(M)] = per_sample(lst, M, dev, a.repeats)
        r['launches_96^3x{}'.format(M)] = launches(M, dev, a.repeats)
        if M == 4 and not a.skip_train:
            r['train_step_vnet4x4_4x96^3_eager'] = train_steps(lst, M, dev, a.steps, min(a.repeats, 5))
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
