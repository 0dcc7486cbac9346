"""Cubic B-spline interpolation on one GPU (prints one JSON line; --out FILE also writes it, default
profiles/bspline_bench.json).  One process; the variants of a group are alternated after a warm-up; every figure is the
median with [min, max] over the repeats.
  (a) the prefilter of a 240 x 240 x 155 x 4 case and of 512 x 512 x 400 x 1, next to the device-to-device copy
      of the same bytes in the same run (one read + one write; the prefilter's three passes each read and write the
      volume twice -- s -> c+ -> c -- except an x line that fits one LDS tile), device events around a block of launches;
  (b) a 96^3 x {4, 1} crop of a resident 160 x 144 x 128 volume with 'BSPLINE' (prefiltered=True, the one evaluation
      launch) against 'LINEAR', affine and with rotation + elastic field, next to the copy of the crop's bytes;
  (c) per sample, 96^3 x 4, file-backed SegmentationDataset.sample() with each mode, plain and with rotation + elastic;
      host clock around a block of samples that ends in a device synchronise;
  (d) the vnet(4, 4) 4 x 96^3 eager train step fed by the file-backed data set with each mode.
usage: python tools/bench_bspline.py [--repeats R] [--steps K] [--skip-train] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_augment import SPATIAL, _stat, _write_cases, _events_ms   # noqa: E402  (also sets up sys.path)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('LINEAR', 'BSPLINE')


def _alternate(fns, repeats, reps):
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            times[name].append(_events_ms(fn, reps) * 1e3)
    return {name + '_us': _stat(v) for name, v in times.items()}


def prefilter(shape_xyzm, dev, repeats, reps):
    from segmentation3d.utils import image_tools as T
    X, Y, Z, M = shape_xyzm
    vol = torch.rand((Z, Y, X, M), device=dev)
    other = torch.empty_like(vol)

    # out of place (the first pass reads vol, the others run in place on `other`): repeated in place the values would grow
    out = _alternate({'prefilter': lambda: T.bspline_prefilter_device(vol, out=other),
                      'copy_d2d': lambda: other.copy_(vol)}, repeats, reps)
    nbytes = int(vol.numel() * 4)
    out['volume_bytes'] = nbytes
    out['copy_read_plus_write_GBps'] = 2 * nbytes / out['copy_d2d_us']['median'] * 1e-3
    out['prefilter_over_copy'] = out['prefilter_us']['median'] / out['copy_d2d_us']['median']
    return out


def crops(M, dev, repeats, reps=50):
    from segmentation3d.utils import image_tools as T
    vol = torch.randn((128, 144, 160, M), device=dev)
    coef = T.bspline_prefilter_device(vol)
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    size, sp, centre, h = (96, 96, 96), (1.05, 1.05, 1.05), (80.0, 72.0, 64.0), 32.0
    g = T.bspline_control_dims(size, sp, h)
    ctrl = torch.from_numpy(np.random.RandomState(0).uniform(-4, 4, size=(g[2], g[1], g[0], 3)).astype(np.float32)).to(dev)
    crop = torch.empty((96, 96, 96, M), dtype=torch.float32, device=dev)
    other = torch.empty_like(crop)
    rot = (0.3, -0.2, 0.4)
    fns = {}
    for mode, src in (('LINEAR', vol), ('BSPLINE', coef)):
        fns['affine_' + mode] = lambda mode=mode, src=src: T.crop_image_device_mc(
            src, frame, centre, size, sp, mode, out=crop, prefiltered=True)
        fns['rotation_elastic_' + mode] = lambda mode=mode, src=src: T.crop_image_device_mc(
            src, frame, centre, size, sp, mode, out=crop, rotation=rot, deform=(ctrl, h), prefiltered=True)
    fns['copy_d2d'] = lambda: other.copy_(crop)
    out = _alternate(fns, repeats, reps)
    out['crop_bytes'] = int(crop.numel() * 4)
    for kind in ('affine', 'rotation_elastic'):
        out[kind + '_BSPLINE_over_LINEAR'] = out[kind + '_BSPLINE_us']['median'] / out[kind + '_LINEAR_us']['median']
    return out


def _dataset(lst, M, dev, mode, aug):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    return SegmentationDataset(lst, 4, [1.0, 1.0, 1.0], [96, 96, 96], 'GLOBAL', [5, 5, 5], [0.9, 1.1], mode,
                               [AdaptiveNormalizer()] * M, device=dev, augmentation=aug)


def per_sample(lst, M, dev, repeats, block=20):
    sets = {'{}_{}'.format(kind, mode): _dataset(lst, M, dev, mode, aug)
            for kind, aug in (('plain', None), ('rotation_elastic', SPATIAL)) for mode in MODES}
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
    sets = {mode: _dataset(lst, M, dev, mode, None) for mode in MODES}
    np.random.seed(0)
    total = 3 + repeats * steps
    loaders = {name: iter(DeviceCropLoader(ds, [k % 2 for k in range(4 * total)], 4)) for name, ds in sets.items()}
    for name in sets:
        for _ in range(3):
            crops_, masks, _, _ = next(loaders[name])
            step(crops_, masks)
    torch.cuda.synchronize()
    times = {name: [] for name in sets}
    for _ in range(repeats):
        for name in sets:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                crops_, masks, _, _ = next(loaders[name])
                step(crops_, masks)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    return {name: _stat(v) for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--skip-train', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'bspline_bench.json'))
    a = ap.parse_args()
    if a.repeats < 7:
        raise SystemExit('at least 7 repeats')
    from segmentation3d import _engine
    _engine.lib()
    if not torch.cuda.is_available():
        raise SystemExit('bench_bspline.py needs a ROCm device')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    r = {'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'unit_launches': 'us', 'unit_per_sample': 'ms',
         'unit_train_step': 'ms'}
    r['prefilter_240x240x155x4'] = prefilter((240, 240, 155, 4), dev, a.repeats, 10)
    r['prefilter_512x512x400x1'] = prefilter((512, 512, 400, 1), dev, a.repeats, 5)
    for M in (4, 1):
        r['crop_96^3x{}'.format(M)] = crops(M, dev, a.repeats)
    lst = _write_cases(4)
    r['per_sample_96^3x4'] = per_sample(lst, 4, dev, a.repeats)
    if not a.skip_train:
        r['train_step_vnet4x4_4x96^3_eager'] = train_steps(lst, 4, dev, a.steps, a.repeats)
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
