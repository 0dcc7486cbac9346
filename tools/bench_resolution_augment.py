"""Gaussian blur and low-resolution simulation of training crops on one GPU (prints one JSON line; --out FILE also writes
it).  One process; the variants of a group are alternated after a warm-up; every figure is the median with [min, max]
over the repeats.
  (a) the launches alone on a resident 96^3 x {1, 4} crop, device events around a block of launches: the blur at sigma 1.0
      (R = 3) and 2.0 (R = 6), the low-resolution simulation at zoom 0.5, and the device-to-device copy of the same two
      tensors as the yardstick (one read + one write of the crop = the floor of both kernels);
  (b) per sample, 96^3 x {1, 4}, file-backed SegmentationDataset.sample(): the section off (the parent's plain path) against
      blur, low resolution and both at probability 1, and -- for the reference figures of profiles/augment_bench.json, taken
      again in this run -- the parent's fully augmented sample without and with both filters; host clock around a block of
      samples that ends in a device synchronise;
  (c) the vnet(4, 4) 4 x 96^3 eager train step fed by the file-backed data set, section off against both filters on.
usage: python tools/bench_resolution_augment.py [--repeats R] [--steps K] [--skip-train] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_augment import SPATIAL, INTENSITY, _stat, _write_cases, _events_ms   # noqa: E402  (also sets up sys.path)

BLUR = {'blur_sigma_vox': [0.5, 1.5], 'blur_prob': 1.0}
LOWRES = {'lowres_zoom': [0.5, 0.9], 'lowres_prob': 1.0}
ALL = dict(SPATIAL, **INTENSITY)
VARIANTS = [('off', None, None), ('blur', None, BLUR), ('lowres', None, LOWRES), ('both', None, dict(BLUR, **LOWRES)),
            ('all_augmentation', ALL, None), ('all_augmentation_and_both', ALL, dict(BLUR, **LOWRES))]


def _dataset(lst, M, dev, aug, res):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    return SegmentationDataset(lst, 4, [1.0, 1.0, 1.0], [96, 96, 96], 'GLOBAL', [5, 5, 5], [0.9, 1.1], 'LINEAR',
                               [AdaptiveNormalizer()] * M, device=dev, augmentation=aug, resolution_augmentation=res)


def launches(M, dev, repeats, reps=50):
    from segmentation3d.utils import image_tools as T
    shape = (96, 96, 96) + ((M,) if M > 1 else ())
    src = torch.randn(shape, device=dev).clamp_(-3, 3)
    dst = torch.empty_like(src)
    blur1, blur2 = T.blur_params([1.0] * M, M), T.blur_params([2.0] * M, M)
    low = T.lowres_params([T.lowres_sizes((96, 96, 96), 0.5)] * M, M, (96, 96, 96))
    fns = {
        'blur_sigma1': lambda: T.blur_device(src, blur1, out=dst),
        'blur_sigma2': lambda: T.blur_device(src, blur2, out=dst),
        'lowres_zoom0.5': lambda: T.lowres_device(src, low, out=dst),
        'copy_d2d': lambda: dst.copy_(src),
    }
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            times[name].append(_events_ms(fn, reps) * 1e3)
    out = {name + '_us': _stat(v) for name, v in times.items()}
    copy = out['copy_d2d_us']['median']
    nbytes = int(src.numel() * 4)
    out['crop_bytes'] = nbytes
    out['copy_read_plus_write_GBps'] = 2 * nbytes / copy * 1e-3
    for name in ('blur_sigma1', 'blur_sigma2', 'lowres_zoom0.5'):
        # share of the copy rate = the one-read, one-write floor over the kernel's time
        out[name + '_share_of_copy_rate'] = copy / out[name + '_us']['median']
    return out


def per_sample(lst, M, dev, repeats, block=20):
    sets = {name: _dataset(lst, M, dev, aug, res) for name, aug, res in VARIANTS}
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


def train_steps(lst, M, dev, steps, repeats):
    from segmentation3d.core.seg_train import TrainStep
    from segmentation3d.dataloader.dataset import DeviceCropLoader
    step = TrainStep('vnet', M, 4, 'Dice', [0.25] * 4, device=dev, seed=0)
    sets = {'off': _dataset(lst, M, dev, None, None), 'both': _dataset(lst, M, dev, None, dict(BLUR, **LOWRES))}
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
    if a.repeats < 7:
        raise SystemExit('at least 7 repeats')
    from segmentation3d import _engine
    _engine.lib()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resolution_augment.py needs a ROCm device')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    r = {'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'unit_launches': 'us', 'unit_per_sample': 'ms',
         'unit_train_step': 'ms'}
    for M in (1, 4):
        lst = _write_cases(M)
        r['launches_96^3x{}'.format(M)] = launches(M, dev, a.repeats)
        r['per_sample_96^3x{}'.format(M)] = per_sample(lst, M, dev, a.repeats)
        if M == 4 and not a.skip_train:
            r['train_step_vnet4x4_4x96^3_eager'] = train_steps(lst, M, dev, a.steps, a.repeats)
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
