"""Device timing of the whole-volume statistics: every pass of seg3d_volume_stats next to a
device-to-device copy that moves the bytes the pass reads, the one-volume entry in total, the torch composition on a size
where torch.sort still runs, and the data-set sample time with VolumeNormalizer against AdaptiveNormalizer.

  python tools/bench_volume_stats.py [--repeats 7] [--inner 3] [--out profiles/volume_stats_bench.json]

Cases: 240 x 240 x 155 x 4 (a BraTS case, 143 MB), non-zero selection, ranks 0.005 / 0.995 with the clamp; and
512 x 512 x 400 x 1 (419 MB), every voxel, the same ranks.  Data: uniform in [-1, 1), and CT-like integers in
[-1000, 3000] with 60 % of the voxels at -1000.
  hist level 0 / 1 / 2   read the volume (4 M bytes per voxel); levels 1 and 2 run one workgroup row per modality, each
                         reading whole rows, so they read M times that from cache / HBM
  moments                reads the volume once
Every launch figure is `inner` back-to-back calls captured in one hipGraph (the method of tools/bench_topk_loss.py), one
process, the variants alternate inside every repeat, median [min, max] over the repeats.  A copy of b bytes moves 2 b, so
the copy beside a pass that reads b bytes copies b / 2.
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'medical-segmentation3d-toolkit_amd'))
sys.path.insert(0, os.path.join(REPO, 'tools'))
sys.path.insert(0, REPO)

from bench_topk_loss import summary, timed_capture                    # noqa: E402
from segmentation3d import _engine as E                                # noqa: E402
from segmentation3d.utils import image_tools as T                      # noqa: E402

QUANTILES = (0.005, 0.995)


def make_volume(shape, kind, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    if kind == 'uniform':
        return torch.rand(shape, generator=gen, device=dev) * 2.0 - 1.0
    v = torch.randint(-1000, 3001, shape, generator=gen, device=dev).float()
    v[torch.rand(shape[:3], generator=gen, device=dev) < 0.6] = -1000.0          # whole rows: a CT background
    return v


def bench_passes(vol, mode, dev, repeats, inner):
    Z, Y, X, M = vol.shape
    nv, nbytes = Z * Y * X, vol.numel() * 4
    acc = T.VolumeStatsAccumulator(M, mode, QUANTILES, True, dev)
    for level in acc.levels():               # a resolved state, so that every pass can be timed on its own
        acc.add_hist(vol, None, level)
        acc.resolve(level)
    acc.add_moments(vol, None)
    out = torch.empty((M, 9), dtype=torch.float64, device=dev)
    state2 = torch.empty_like(acc.state)
    q = (ctypes.c_double * 4)(*QUANTILES, 0.0, 0.0)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    runs = {
        'hist level 0': lambda: acc.add_hist(vol, None, 0),
        'hist level 1': lambda: acc.add_hist(vol, None, 1),
        'hist level 2': lambda: acc.add_hist(vol, None, 2),
        'moments': lambda: acc.add_moments(vol, None),
        'total (seg3d_volume_stats)': lambda: E.call('seg3d_volume_stats', E.ptr(vol), None, nv, M, acc.mode, 2, q, 1,
                                                    E.ptr(state2), E.ptr(out), E.stream_ptr()),
        'copy': lambda: dst.copy_(src),
    }
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            times[k].append(timed_capture(fn, inner))
    res = {k: summary(v) for k, v in times.items()}
    copy_us = res['copy']['median']
    rows = {}
    for k in runs:
        if k == 'copy':
            continue
        passes = 4 if k.startswith('total') else 1
        rows[k] = {'us': res[k], 'reads_bytes': passes * nbytes, 'GBps_of_bytes_read': passes * nbytes / res[k]['median'] * 1e-3,
                   'fraction_of_copy_rate': passes * copy_us / res[k]['median']}
    return {'shape_zyxm': [Z, Y, X, M], 'mode': mode, 'copy_us': res['copy'], 'passes': rows}


def torch_composition(vol, mode):
    """the same numbers from stock torch ops on one modality (sort-based; boolean indexing synchronises)"""
    x = vol.reshape(-1)
    if mode == 'nonzero':
        x = x[x != 0]
    s, _ = torch.sort(x)
    n = s.numel()
    lo, hi = (s[int(np.floor(qq * (n - 1) + 0.5))] for qq in QUANTILES)
    c = torch.clamp(s.double(), float(lo), float(hi))
    return n, float(s[0]), float(s[-1]), float(c.mean()), float(c.std(unbiased=False)), float(lo), float(hi)


def bench_torch(dev, repeats):
    out = {}
    for kind in ('uniform', 'ct'):
        vol = make_volume((128, 256, 256, 1), kind, dev, 3)
        t = {'seg3d_volume_stats (with the read-back)': [], 'torch sort composition': []}
        for _ in range(repeats + 1):
            for name, fn in (('seg3d_volume_stats (with the read-back)',
                              lambda: T.volume_stats_device(vol, 'nonzero', quantiles=QUANTILES, clip=True)),
                             ('torch sort composition', lambda: torch_composition(vol, 'nonzero'))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = fn()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) * 1e6)
            del r
        res = {k: summary(v[1:]) for k, v in t.items()}       # the first round warms both up
        res['torch_over_device'] = res['torch sort composition']['median'] / res['seg3d_volume_stats (with the read-back)']['median']
        out[kind] = res
    return {'shape_zyxm': [128, 256, 256, 1], 'wall_clock_us': out}


def bench_sample(dev, repeats, inner):
    """SegmentationDataset.sample of a four-modality case at the flagship crop (96^3), VolumeNormalizer against
    AdaptiveNormalizer: the adaptive path runs a per-crop statistics pass that the case-level path drops"""
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    from segmentation3d.utils.normalizer import AdaptiveNormalizer, VolumeNormalizer
    rng = np.random.RandomState(0)
    shape, frame = (128, 160, 160), ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0))
    with tempfile.TemporaryDirectory() as tmp:
        lines = ['1 4']
        for m in range(4):
            p = os.path.join(tmp, 'mod{}.mha'.format(m))
            write_mha(Image3d(rng.normal(300.0, 80.0, size=shape).astype(np.float32), *frame), p)
            lines.append(p)
        write_mha(Image3d(rng.randint(0, 4, size=shape).astype(np.int8), *frame), os.path.join(tmp, 'seg.mha'))
        lines.append(os.path.join(tmp, 'seg.mha'))
        lst = os.path.join(tmp, 'train.txt')
        with open(lst, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        sets = {name: SegmentationDataset(lst, 4, [1.0, 1.0, 1.0], [96, 96, 96], 'GLOBAL', [5, 5, 5], [0.9, 1.1], 'LINEAR',
                                          [cls() for _ in range(4)], device=dev)
                for name, cls in (('AdaptiveNormalizer', AdaptiveNormalizer), ('VolumeNormalizer', VolumeNormalizer))}
        buf = torch.empty((96, 96, 96, 4), dtype=torch.float32, device=dev)
        times = {k: [] for k in sets}
        for rep in range(repeats + 1):
            for name, ds in sets.items():
                np.random.seed(rep)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    ds.sample(0, out=buf)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e6 / inner)
    res = {k: summary(v[1:]) for k, v in times.items()}           # the first round loads the case
    res['volume_over_adaptive'] = res['VolumeNormalizer']['median'] / res['AdaptiveNormalizer']['median']
    return {'crop': [96, 96, 96], 'modalities': 4, 'samples_per_timing': inner, 'wall_clock_us_per_sample': res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=3)
    ap.add_argument('--sample-inner', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'volume_stats_bench.json'))
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    result = {'method': 'one process, variants alternated inside every repeat, median [min, max] of {}'.format(args.repeats),
              'quantiles': list(QUANTILES), 'clamp': True, 'cases': {}}
    for name, shape, mode in (('brats 240x240x155x4 nonzero', (155, 240, 240, 4), 'nonzero'),
                              ('ct 512x512x400x1 all', (400, 512, 512, 1), 'all')):
        for kind in ('uniform', 'ct'):
            vol = make_volume(shape, kind, dev, 1)
            r = bench_passes(vol, mode, dev, args.repeats, args.inner)
            result['cases']['{}, {} data'.format(name, kind)] = r
            del vol
            torch.cuda.empty_cache()
            print('--- {}, {} data: us per launch, median [min, max] of {}; copy {:.0f} us'.format(
                name, kind, args.repeats, r['copy_us']['median']))
            for k, v in r['passes'].items():
                print('  {:28s} {:9.1f} [{:9.1f}, {:9.1f}]  {:7.1f} GB/s read  {:.2f} of the copy rate'.format(
                    k, v['us']['median'], v['us']['min'], v['us']['max'], v['GBps_of_bytes_read'], v['fraction_of_copy_rate']))
    result['torch_composition'] = bench_torch(dev, args.repeats)
    for kind, v in result['torch_composition']['wall_clock_us'].items():
        print('--- 128x256x256x1 {}: device {:.0f} us, torch sort {:.0f} us ({:.1f} x)'.format(
            kind, v['seg3d_volume_stats (with the read-back)']['median'], v['torch sort composition']['median'],
            v['torch_over_device']))
    result['dataset_sample'] = bench_sample(dev, args.repeats, args.sample_inner)
    s = result['dataset_sample']['wall_clock_us_per_sample']
    print('--- sample 96^3 x 4: Adaptive {:.0f} us, Volume {:.0f} us (ratio {:.3f})'.format(
        s['AdaptiveNormalizer']['median'], s['VolumeNormalizer']['median'], s['volume_over_adaptive']))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
