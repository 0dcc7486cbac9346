"""'LABEL_LINEAR' mask interpolation on one GPU (prints one JSON line; --out FILE also writes it, default
profiles/label_interp_bench.json).  One process; the variants of a group are alternated after a warm-up; every figure is the
median with [min, max] over the repeats.  Everything is a 96^3 crop of a 240 x 240 x 155 five-label mask (cubes of 12 voxels
with random labels: as in a real mask almost every neighbourhood is uniform; `random` re-draws every voxel, the worst case,
in which every neighbourhood is mixed).
  (a) the mask-crop launch with 'NN' and 'LABEL_LINEAR' from float32 and uint8 sources, affine and with rotation + elastic
      field, device events around a block of launches;
  (b) the composition from existing operators -- C x resample_device of an indicator plane, stack, arg-max -- at C = 2 and
      C = 5, and a device-to-device copy of the crop's bytes, in the same group;
  (c) per sample, 96^3 x 4, file-backed SegmentationDataset.sample() with each mask mode, plain and fully augmented
      (rotation + elastic + intensity); host clock around a block of samples that ends in a device synchronise;
  (d) the vnet(4, 4) 4 x 96^3 eager train step fed by the file-backed data set with each mask mode.
usage: python tools/bench_label_interp.py [--repeats R] [--steps K] [--skip-train] [--out FILE]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o k -- python tools/bench_label_interp.py --kernel-time cubes"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_augment import SPATIAL, INTENSITY, _stat, _events_ms   # noqa: E402  (also sets up sys.path)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('NN', 'LABEL_LINEAR')
SHAPE = (155, 240, 240)                  # z, y, x
LABELS = 5


def _mask(rng, kind='cubes'):
    if kind == 'random':
        return rng.randint(0, LABELS, size=SHAPE).astype(np.uint8)
    coarse = rng.randint(0, LABELS, size=tuple((n + 11) // 12 for n in SHAPE)).astype(np.uint8)
    return np.kron(coarse, np.ones((12, 12, 12), dtype=np.uint8))[:SHAPE[0], :SHAPE[1], :SHAPE[2]]


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


def launches(dev, repeats, reps=50):
    from segmentation3d.utils import image_tools as T
    rng = np.random.RandomState(0)
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    size, sp, centre, h = (96, 96, 96), (1.05, 1.05, 1.05), (120.0, 120.0, 77.0), 32.0
    g = T.bspline_control_dims(size, sp, h)
    ctrl = torch.from_numpy(rng.uniform(-4, 4, size=(g[2], g[1], g[0], 3)).astype(np.float32)).to(dev)
    rot = (0.3, -0.2, 0.4)
    warped = {'rotation': rot, 'deform': (ctrl, h)}
    masks = {kind: torch.from_numpy(_mask(rng, kind)).to(dev) for kind in ('cubes', 'random')}
    sources = {'float32': masks['cubes'].float(), 'uint8': masks['cubes'], 'random_uint8': masks['random']}
    fns = {}
    for src_name, src in sources.items():
        for mode in MODES:
            if src_name == 'random_uint8' and mode == 'NN':
                continue
            fns['affine_{}_{}'.format(mode, src_name)] = lambda mode=mode, src=src: T.crop_image_device(
                src, frame, centre, size, sp, mode)
            fns['rotation_elastic_{}_{}'.format(mode, src_name)] = lambda mode=mode, src=src: T.crop_image_device(
                src, frame, centre, size, sp, mode, **warped)
    as_float = sources['float32']

    def composition(C, **spatial):
        planes = [T.crop_image_device((as_float == float(l)).float(), frame, centre, size, sp, 'LINEAR', **spatial)
                  for l in range(C)]
        return torch.stack(planes).argmax(0)

    for C in (2, LABELS):
        fns['affine_composition_C{}'.format(C)] = lambda C=C: composition(C)
        fns['rotation_elastic_composition_C{}'.format(C)] = lambda C=C: composition(C, **warped)
    crop = torch.empty((96, 96, 96), dtype=torch.float32, device=dev)
    other = torch.empty_like(crop)
    fns['copy_d2d'] = lambda: other.copy_(crop)
    out = _alternate(fns, repeats, reps)
    out['crop_bytes'] = int(crop.numel() * 4)
    out['share_of_voxels_where_LABEL_LINEAR_differs_from_NN_cubes'] = float(
        (T.crop_image_device(sources['uint8'], frame, centre, size, sp, 'LABEL_LINEAR')
         != T.crop_image_device(sources['uint8'], frame, centre, size, sp, 'NN')).float().mean())
    for kind in ('affine', 'rotation_elastic'):
        for src_name in ('float32', 'uint8'):
            out['{}_{}_LABEL_LINEAR_over_NN'.format(kind, src_name)] = (
                out['{}_LABEL_LINEAR_{}_us'.format(kind, src_name)]['median']
                / out['{}_NN_{}_us'.format(kind, src_name)]['median'])
        out['{}_composition_C5_over_LABEL_LINEAR'.format(kind)] = (
            out['{}_composition_C5_us'.format(kind)]['median'] / out['{}_LABEL_LINEAR_float32_us'.format(kind)]['median'])
    return out


def bare_launches(kind, dev, reps=30):
    """--kernel-time KIND: `reps` mask-crop launches per (source type, mode, geometry) and nothing else, for a run under
    `rocprofv3 --kernel-trace --stats` (the kernel's device time, which the host-side figures of (a) hide)"""
    from segmentation3d.utils import image_tools as T
    rng = np.random.RandomState(0)
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    size, sp, centre, h = (96, 96, 96), (1.05, 1.05, 1.05), (120.0, 120.0, 77.0), 32.0
    g = T.bspline_control_dims(size, sp, h)
    ctrl = torch.from_numpy(rng.uniform(-4, 4, size=(g[2], g[1], g[0], 3)).astype(np.float32)).to(dev)
    warped = {'rotation': (0.3, -0.2, 0.4), 'deform': (ctrl, h)}
    mask = torch.from_numpy(_mask(rng, kind)).to(dev)
    for src in (mask, mask.float()):
        for mode in MODES:
            for spatial in ({}, warped):
                for _ in range(reps):
                    T.crop_image_device(src, frame, centre, size, sp, mode, **spatial)
    torch.cuda.synchronize()


def _write_cases(M):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    tmp = tempfile.mkdtemp(prefix='label_interp_bench_')
    rng = np.random.RandomState(1)
    lines = []
    for k in range(2):
        for m in range(M):
            p = os.path.join(tmp, 'c{}_m{}.mha'.format(k, m))
            write_mha(Image3d((rng.standard_normal(SHAPE).astype(np.float32) * 50 + 10 * m)), p)
            lines.append(p)
        p = os.path.join(tmp, 'c{}_seg.mha'.format(k))
        write_mha(Image3d(_mask(rng).astype(np.int8)), p)
        lines.append(p)
    lst = os.path.join(tmp, 'train.txt')
    with open(lst, 'w') as f:
        f.write('2 {}\n'.format(M) + '\n'.join(lines) + '\n')
    return lst


def _dataset(lst, M, dev, mode, aug):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    return SegmentationDataset(lst, LABELS, [1.0, 1.0, 1.0], [96, 96, 96], 'GLOBAL', [5, 5, 5], [0.9, 1.1], 'LINEAR',
                               [AdaptiveNormalizer()] * M, device=dev, augmentation=aug, mask_interpolation=mode)


def per_sample(lst, M, dev, repeats, block=20):
    sets = {'{}_{}'.format(kind, mode): _dataset(lst, M, dev, mode, aug)
            for kind, aug in (('plain', None), ('all', dict(SPATIAL, **INTENSITY))) for mode in MODES}
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

    def one(name):
        crops_, masks, _, _ = next(loaders[name])
        step(crops_, masks.clamp_(max=3.0))          # vnet(4, 4): the fifth label joins the fourth, in place, both modes alike

    for name in sets:
        for _ in range(3):
            one(name)
    torch.cuda.synchronize()
    times = {name: [] for name in sets}
    for _ in range(repeats):
        for name in sets:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                one(name)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / steps * 1e3)
    return {name: _stat(v) for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--skip-train', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'label_interp_bench.json'))
    ap.add_argument('--kernel-time', choices=['cubes', 'random'], default=None,
                    help='only 30 bare launches per variant on this mask, to be run under rocprofv3 --kernel-trace --stats')
    a = ap.parse_args()
    if a.repeats < 7:
        raise SystemExit('at least 7 repeats')
    from segmentation3d import _engine
    _engine.lib()
    if not torch.cuda.is_available():
        raise SystemExit('bench_label_interp.py needs a ROCm device')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    if a.kernel_time:
        bare_launches(a.kernel_time, dev)
        return
    r = {'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'unit_launches': 'us', 'unit_per_sample': 'ms',
         'unit_train_step': 'ms'}
    r['mask_crop_96^3_of_240x240x155'] = launches(dev, a.repeats)
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
