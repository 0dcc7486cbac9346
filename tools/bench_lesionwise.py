"""Device timing of the lesion-wise evaluation: every new launch next to a device-to-device
copy of the bytes it must move, and `cal_lesionwise` end to end next to the SciPy pipeline of tests/lesion_oracle.py on
the same input and the same host.

  python tools/bench_lesionwise.py [--repeats 7] [--scipy-repeats 7] [--inner 5] [--out profiles/lesionwise_bench.json]

The case: one 240 x 240 x 155 volume (int16 labels) with about 30 ground-truth ellipsoids of mixed size and a perturbed
copy as prediction (blobs shifted by a voxel or two, some dropped, a few spurious ones added), spacing 1 mm.
  label_set_mask    reads 2 bytes, writes 1 byte per voxel
  dilate18 x1 / x3  reads and writes 1 byte per voxel and iteration (halo from cache)
  ccl26_label       must read the mask and write the id map, 5 bytes per voxel; its seven passes move more
  lesion_pairs      reads Dmap, A, Pmap: 9 bytes per voxel; with and without the in-wave collapse of equal keys
  lesion_select     reads 9, writes 2 bytes per voxel
Every launch figure is `inner` back-to-back calls captured in one hipGraph (the method of tools/bench_topk_loss.py), the
variants alternate inside every repeat, median [min, max] over the repeats.  The end-to-end figures are wall-clock seconds
from host arrays to the result dict, device and SciPy alternating.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'medical-segmentation3d-toolkit_amd'))
sys.path.insert(0, os.path.join(REPO, 'tools'))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)

from bench_topk_loss import summary, timed_capture                    # noqa: E402
from segmentation3d import _engine as E                                # noqa: E402
from segmentation3d.utils import metrics as M                          # noqa: E402

SHAPE = (155, 240, 240)     # [z, y, x]


def synthetic_case(seed=0, blobs=30):
    rng = np.random.RandomState(seed)
    gt, seg = np.zeros(SHAPE, np.int16), np.zeros(SHAPE, np.int16)
    zz, yy, xx = np.ogrid[:SHAPE[0], :SHAPE[1], :SHAPE[2]]

    def ellipsoid(c, r):
        return ((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1.0

    for k in range(blobs):
        big = k < 3
        r = rng.uniform(12, 22, 3) if big else rng.uniform(1.5, 7, 3)
        c = [rng.uniform(rk + 2, s - rk - 2) for rk, s in zip(r, SHAPE)]
        gt[ellipsoid(c, r)] = 1
        if k % 6 == 5:
            continue                                                        # dropped by the prediction
        shift = rng.randint(-2, 3, 3)
        seg[ellipsoid([ck + sk for ck, sk in zip(c, shift)], r * rng.uniform(0.85, 1.1))] = 1
    for _ in range(4):                                                      # spurious components
        r = rng.uniform(1.5, 4, 3)
        seg[ellipsoid([rng.uniform(rk + 2, s - rk - 2) for rk, s in zip(r, SHAPE)], r)] = 1
    return gt, seg


def bench_launches(gt, seg, dev, repeats, inner):
    Z, Y, X = SHAPE
    n = gt.size
    g, s = torch.from_numpy(gt).to(dev), torch.from_numpy(seg).to(dev)
    a, b = M._set_mask(g, [1]), M._set_mask(s, [1])
    grown = M._dilate18(a, SHAPE, 3)
    dmap, dcount, _ = M._ccl26(grown, SHAPE, 0)
    pmap, pcount, _ = M._ccl26(b, SHAPE, 4096)
    kg, kp = int(dcount[0]), int(pcount[0])
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    out, work = torch.empty_like(mask), torch.empty_like(mask)
    ids = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(2, dtype=torch.int32, device=dev)
    sizes = torch.empty(4096, dtype=torch.int32, device=dev)
    ccl_work = torch.empty(E.query('seg3d_ccl26_label_workspace_ints', n), dtype=torch.int32, device=dev)
    words = torch.zeros(2 * (kg + 1) + 16384, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    flag = torch.ones(kp + 1, dtype=torch.uint8, device=dev)
    flag[0] = 0
    sp = E.stream_ptr
    variants = {
        'label_set_mask': (3, lambda: E.call('seg3d_label_set_mask', E.ptr(g), 2, n, M._label_set([1]), E.ptr(mask), sp())),
        'dilate18 x1': (2, lambda: E.call('seg3d_binary_dilate18', E.ptr(a), E.ptr(out), E.ptr(work), X, Y, Z, 1, sp())),
        'dilate18 x3': (6, lambda: E.call('seg3d_binary_dilate18', E.ptr(a), E.ptr(out), E.ptr(work), X, Y, Z, 3, sp())),
        'ccl26_label': (5, lambda: E.call('seg3d_ccl26_label', E.ptr(grown), X, Y, Z, E.ptr(ids), E.ptr(count), E.ptr(sizes),
                                          4096, E.ptr(ccl_work), sp())),
        'lesion_pairs': (9, lambda: E.call('seg3d_lesion_pairs', E.ptr(dmap), E.ptr(a), E.ptr(pmap), n, kg, E.ptr(words),
                                           E.ptr(words[kg + 1:]), E.ptr(words[2 * (kg + 1):]), 16384, 1, E.ptr(status), sp())),
        'lesion_pairs, no collapse': (9, lambda: E.call('seg3d_lesion_pairs', E.ptr(dmap), E.ptr(a), E.ptr(pmap), n, kg,
                                                        E.ptr(words), E.ptr(words[kg + 1:]), E.ptr(words[2 * (kg + 1):]), 16384, 0,
                                                        E.ptr(status), sp())),
        'lesion_select': (11, lambda: E.call('seg3d_lesion_select', E.ptr(dmap), E.ptr(a), E.ptr(pmap), E.ptr(flag), kp, 1, n,
                                             E.ptr(mask), E.ptr(out), sp())),
    }
    runs = {}
    for name, (bytes_per_voxel, fn) in variants.items():
        src = torch.empty(bytes_per_voxel * n // 2, dtype=torch.uint8, device=dev)      # a copy of b bytes moves 2 b
        dst = torch.empty_like(src)
        runs[name] = fn
        runs['copy ' + name] = lambda src=src, dst=dst: dst.copy_(src)
    times = {k: [] for k in runs}
    for _ in range(repeats):
        for k, fn in runs.items():
            times[k].append(timed_capture(fn, inner))
    res = {k: summary(v) for k, v in times.items()}
    rows = {}
    for name, (bytes_per_voxel, _) in variants.items():
        us, copy_us = res[name]['median'], res['copy ' + name]['median']
        rows[name] = {'us': res[name], 'copy_us': res['copy ' + name], 'must_move_bytes': bytes_per_voxel * n,
                      'GBps_of_must_move': bytes_per_voxel * n / us * 1e-3, 'times_the_copy': us / copy_us}
    return {'lesions': kg, 'predicted_components': kp, 'launches': rows}


def bench_end_to_end(gt, seg, repeats, scipy_repeats):
    import lesion_oracle as O
    M.cal_lesionwise(gt, seg, [1])                                            # warm-up: library load, allocator
    torch.cuda.synchronize()
    device, scipy_s, got, want = [], [], None, None
    for k in range(max(repeats, scipy_repeats)):
        if k < repeats:
            t0 = time.perf_counter()
            got, = M.cal_lesionwise(gt, seg, [1])
            device.append(time.perf_counter() - t0)
            print('  run {}: cal_lesionwise {:.3f} s'.format(k, device[-1]), flush=True)
        if k < scipy_repeats:
            t0 = time.perf_counter()
            want = O.lesionwise(gt, seg, [1])
            scipy_s.append(time.perf_counter() - t0)
            print('  run {}: scipy {:.3f} s'.format(k, scipy_s[-1]), flush=True)
    agree = None
    if want is not None:
        agree = (all(got[k] == want[k] for k in ('n_gt', 'n_tp', 'n_fn', 'n_fp')) and abs(got['lw_dice'] - want['lw_dice']) <= 1e-12
                 and got['lw_hd95'] == want['lw_hd95'])
    out = {'cal_lesionwise_s': summary(device), 'device_repeats': repeats, 'scipy_repeats': scipy_repeats,
           'result': {k: got[k] for k in ('lw_dice', 'lw_hd95', 'n_gt', 'n_tp', 'n_fn', 'n_fp', 'lesion_f1')},
           'agrees_with_scipy': agree}
    if scipy_s:
        out['scipy_s'] = summary(scipy_s)
        out['scipy_over_device'] = out['scipy_s']['median'] / out['cal_lesionwise_s']['median']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--scipy-repeats', type=int, default=7, help='runs of the SciPy pipeline (each takes about a minute)')
    ap.add_argument('--inner', type=int, default=5, help='calls per captured graph')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'lesionwise_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_lesionwise.py needs a ROCm device: timings are taken on the GPU only')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    gt, seg = synthetic_case()
    result = {'device': torch.cuda.get_device_name(dev), 'shape_zyx': list(SHAPE), 'repeats': args.repeats, 'inner': args.inner}
    result.update(bench_launches(gt, seg, dev, args.repeats, args.inner))
    print('--- {} x {} x {} (x, y, z), {} lesions, {} predicted components: us per launch, median [min, max] of {}'.format(
        SHAPE[2], SHAPE[1], SHAPE[0], result['lesions'], result['predicted_components'], args.repeats))
    for k, v in result['launches'].items():
        print('  {:26s} {:9.1f} [{:9.1f}, {:9.1f}]  copy {:8.1f}  {:7.1f} GB/s of the bytes it must move, {:5.2f} x the copy'.format(
            k, v['us']['median'], v['us']['min'], v['us']['max'], v['copy_us']['median'], v['GBps_of_must_move'],
            v['times_the_copy']))
    result['end_to_end'] = e = bench_end_to_end(gt, seg, args.repeats, args.scipy_repeats)
    print('  cal_lesionwise {:.3f} [{:.3f}, {:.3f}] s'.format(*(e['cal_lesionwise_s'][k] for k in ('median', 'min', 'max'))))
    if 'scipy_s' in e:
        print('  scipy          {:.3f} [{:.3f}, {:.3f}] s   ({:.1f} x), results agree: {}'.format(
            *(e['scipy_s'][k] for k in ('median', 'min', 'max')), e['scipy_over_device'], e['agrees_with_scipy']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
