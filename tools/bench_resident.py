"""Compact resident training cases on one GPU (prints one JSON line; --out FILE also writes it, default
profiles/resident_bench.json).  One process; the variants of a group are alternated after a warm-up; every figure is the
median with [min, max] over the repeats.
  (a) the crop launch alone, 96^3 x {1, 4} 'LINEAR' out of a resident 240 x 240 x 155 x M volume, affine and with rotation +
      elastic field, from an fp32 and from an int16 source (the same values), device events around a block of launches;
  (b) the 96^3 'NN' mask crop out of a 240 x 240 x 155 volume from fp32 and from uint8;
  (c) per sample, 96^3 x 4, file-backed SegmentationDataset.sample() on int16 images + uint8 masks of 240 x 240 x 155 x 4:
      resident_storage 'fp32', 'compact', and 'compact' with a budget that stages every case (each sample uploads its case
      from pinned host memory); host clock around a block of samples that ends in a device synchronise;
  (d) torch.cuda.memory_allocated() after loading the same cases with 'fp32' and with 'compact'.
usage: python tools/bench_resident.py [--repeats R] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_augment import SPATIAL, _stat, _events_ms   # noqa: E402  (also sets up sys.path)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = (155, 240, 240)                   # z, y, x
FRAME = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
SIZE, SPACING, CENTRE, GRID_MM = (96, 96, 96), (1.05, 1.05, 1.05), (120.0, 120.0, 77.0), 32.0


def _alternate(fns, repeats, reps):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            times[name].append(_events_ms(fn, reps) * 1e3)
    return {name + '_us': _stat(v) for name, v in times.items()}


def crops(M, dev, repeats, reps=50):
    from segmentation3d.utils import image_tools as T
    i16 = torch.randint(-1000, 3000, CASE + (M,), dtype=torch.int16, device=dev)
    sources = {'fp32': i16.float(), 'int16': i16}
    g = T.bspline_control_dims(SIZE, SPACING, GRID_MM)
    ctrl = torch.from_numpy(np.random.RandomState(0).uniform(-4, 4, size=(g[2], g[1], g[0], 3)).astype(np.float32)).to(dev)
    crop = torch.empty((96, 96, 96, M), dtype=torch.float32, device=dev)
    other = torch.empty_like(crop)
    rot = (0.3, -0.2, 0.4)
    fns = {}
    for name, src in sources.items():
        fns['affine_' + name] = lambda src=src: T.crop_image_device_mc(src, FRAME, CENTRE, SIZE, SPACING, 'LINEAR', out=crop)
        fns['rotation_elastic_' + name] = lambda src=src: T.crop_image_device_mc(
            src, FRAME, CENTRE, SIZE, SPACING, 'LINEAR', out=crop, rotation=rot, deform=(ctrl, GRID_MM))
    fns['copy_d2d'] = lambda: other.copy_(crop)
    out = _alternate(fns, repeats, reps)
    out['crop_bytes'] = int(crop.numel() * 4)
    for kind in ('affine', 'rotation_elastic'):
        out[kind + '_int16_over_fp32'] = out[kind + '_int16_us']['median'] / out[kind + '_fp32_us']['median']
    return out


def mask_crops(dev, repeats, reps=50):
    from segmentation3d.utils import image_tools as T
    u8 = torch.randint(0, 4, CASE, dtype=torch.uint8, device=dev)
    fns = {name: (lambda src=src: T.crop_image_device(src, FRAME, CENTRE, SIZE, SPACING, 'NN'))
           for name, src in (('fp32', u8.float()), ('uint8', u8))}
    out = _alternate(fns, repeats, reps)
    out['uint8_over_fp32'] = out['uint8_us']['median'] / out['fp32_us']['median']
    return out


def _write_cases(M, count=2):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    tmp = tempfile.mkdtemp(prefix='resident_bench_')
    rng = np.random.RandomState(1)
    lines = []
    for k in range(count):
        for m in range(M):
            p = os.path.join(tmp, 'c{}_m{}.mha'.format(k, m))
            write_mha(Image3d(rng.randint(-1000, 3000, size=CASE).astype(np.int16)), p)
            lines.append(p)
        p = os.path.join(tmp, 'c{}_seg.mha'.format(k))
        write_mha(Image3d((rng.rand(*CASE) > 0.7).astype(np.uint8) * (1 + k)), p)
        lines.append(p)
    lst = os.path.join(tmp, 'train.txt')
    with open(lst, 'w') as f:
        f.write('{} {}\n'.format(count, M) + '\n'.join(lines) + '\n')
    return lst


def _dataset(lst, M, dev, storage, budget=None, aug=None):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    return SegmentationDataset(lst, 4, [1.0, 1.0, 1.0], [96, 96, 96], 'GLOBAL', [5, 5, 5], [0.9, 1.1], 'LINEAR',
                               [AdaptiveNormalizer()] * M, device=dev, augmentation=aug, resident_storage=storage,
                               resident_budget_gb=budget)


def per_sample(lst, M, dev, repeats, block=20):
    variants = (('fp32', 'fp32', None), ('compact', 'compact', None), ('compact_staged', 'compact', 1e-9))
    sets, footprint = {}, {}
    for kind, aug in (('plain', None), ('rotation_elastic', SPATIAL)):
        for name, storage, budget in variants:
            torch.cuda.synchronize()
            before = torch.cuda.memory_allocated()
            ds = _dataset(lst, M, dev, storage, budget, aug)
            for k in range(2):
                ds.case(k)
            torch.cuda.synchronize()
            if kind == 'plain':
                footprint[name] = {'memory_allocated_bytes': int(torch.cuda.memory_allocated() - before),
                                   'resident_bytes': int(ds.resident_bytes()), 'staged_cases': int(ds.num_staged())}
            sets['{}_{}'.format(kind, name)] = ds
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
    out = {name: _stat(v) for name, v in times.items()}
    case = sets['plain_compact_staged'].case(0)
    out['staged_upload_bytes_per_sample'] = int(case.nbytes)
    return out, footprint


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'resident_bench.json'))
    a = ap.parse_args()
    if a.repeats < 7:
        raise SystemExit('at least 7 repeats')
    from segmentation3d import _engine
    _engine.lib()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resident.py needs a ROCm device')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    r = {'device': torch.cuda.get_device_name(0), 'repeats': a.repeats, 'unit_launches': 'us', 'unit_per_sample': 'ms',
         'case_zyx': list(CASE)}
    for M in (1, 4):
        r['crop_96^3x{}'.format(M)] = crops(M, dev, a.repeats)
    r['mask_crop_96^3'] = mask_crops(dev, a.repeats)
    lst = _write_cases(4)
    r['per_sample_96^3x4'], r['footprint_2_cases_x4'] = per_sample(lst, 4, dev, a.repeats)
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
