"""Device timing of the boundary loss and its signed distance map next to DiceCE and a
device-to-device copy.

  python tools/bench_boundary_loss.py [--repeats 7] [--inner 10] [--steps 30] [--step-repeats 5] [--no-steps]
                                      [--out profiles/boundary_loss_bench.json]

On 4 x 2 x 96^3 (probabilities) / 4 x 96^3 (target), in ONE process, the method of tools/bench_topk_loss.py:
  signed_distance K=1 / K=2  seg3d_signed_distance alone for one and for two classes (pass x, pass y, pass z)
  DiceBoundary fwd / fwd+bwd the loss: the distance map of both classes + one streaming pass + finalize; backward
  DiceCE fwd / fwd+bwd       the compound loss with gamma = 0
  copy K=1 / K=2             a device-to-device copy of the bytes the distance pass must move: the target in and K phi
                             volumes out, (1 + K) * N * S * 4 bytes -- the floor of the distance map
Every figure is `inner` back-to-back calls captured in one hipGraph, one warm-up replay, one replay between two device
events, event time / inner.  ONE captured graph is alive at a time; the variants alternate inside every repeat.  Medians
with [min, max] over the repeats.

Then TrainStep('vnet', 1, 2) on 4 x 1 x 96^3 with DiceBoundary and with DiceCE (whole step in a hipGraph), alternated in
blocks of `steps` steps -- one TrainStep alive at a time -- and their difference per pair of blocks.
"""
import argparse
import gc
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'medical-segmentation3d-toolkit_amd'))
sys.path.insert(0, os.path.join(REPO, 'tools'))
sys.path.insert(0, REPO)

from bench_topk_loss import summary, timed_capture                    # noqa: E402
from segmentation3d import _ops                                        # noqa: E402
from segmentation3d.core.seg_train import TrainStep, build_loss       # noqa: E402

N, EDGE, C = 4, 96, 2
SPACING = (0.7, 1.3, 2.5)


def bench_kernels(dev, repeats, inner):
    gen = torch.Generator().manual_seed(C)
    p = torch.softmax(2.0 * torch.randn((N, C, EDGE, EDGE, EDGE), generator=gen), dim=1).to(dev)
    # blobs, not noise: the cost of the distance map does not depend on the labels, but the step below should see a mask
    t = (torch.randn((N, 1, EDGE, EDGE, EDGE), generator=gen).to(dev))
    t = (torch.nn.functional.avg_pool3d(t, 9, stride=1, padding=4) > 0).float().contiguous()
    pg = p.clone().requires_grad_(True)
    nvox = N * EDGE ** 3
    losses = {'DiceBoundary': build_loss('DiceBoundary', C, None, 2, spacing=SPACING), 'DiceCE': build_loss('DiceCE', C, None, 2)}
    losses['DiceBoundary'](p, t)    # the device scalar exists before any capture
    variants = {}
    for k in (1, 2):
        ids = list(range(k))
        src = torch.empty((1 + k) * nvox, device=dev)
        dst = torch.empty_like(src)
        variants['signed_distance K={}'.format(k)] = lambda ids=ids: _ops.signed_distance(t, ids, SPACING, None, num_class=C)
        variants['copy K={}'.format(k)] = lambda src=src, dst=dst: dst.copy_(src)
    for name, loss_fn in losses.items():
        def fwd(loss_fn=loss_fn):
            with torch.no_grad():
                loss_fn(p, t)

        def both(loss_fn=loss_fn):
            pg.grad = None
            loss_fn(pg, t).backward()
        variants[name + ' fwd'] = fwd
        variants[name + ' fwd+bwd'] = both
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():          # alternated: every repeat visits every variant once, one graph at a time
            times[k].append(timed_capture(fn, inner))
    res = {k: summary(v) for k, v in times.items()}
    out = {'shape': [N, C, EDGE, EDGE, EDGE], 'spacing': list(SPACING), 'us_per_call': res, 'signed_distance': {}}
    for k in (1, 2):
        moved = 2 * (1 + k) * nvox * 4          # the copy reads and writes (1 + K) * N * S * 4 bytes
        ts, tc = res['signed_distance K={}'.format(k)]['median'], res['copy K={}'.format(k)]['median']
        # min / FMA pairs of the brute-force transform: 2 fields x (X + Y + Z) candidates per voxel and class (pass x
        # updates one of its two fields per candidate)
        pairs = k * nvox * (EDGE + 2 * EDGE + 2 * EDGE)
        out['signed_distance']['K{}'.format(k)] = {'us': ts, 'copy_floor_us': tc, 'copy_bytes': moved,
                                                   'times_the_copy_floor': ts / tc, 'min_plus_candidates': pairs,
                                                   'candidates_per_s': pairs / (ts * 1e-6)}
    return out


def bench_steps(dev, repeats, steps):
    """A B A B ...: every block builds its own TrainStep, warms it up (two eager steps, the capture, two replays), times
    `steps` replays and drops it again: one captured TrainStep alive at a time"""
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((N, 1, EDGE, EDGE, EDGE), generator=gen).to(dev)
    t = torch.randint(0, 2, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    options = {'DiceBoundary': {'spacing': SPACING}, 'DiceCE': None}
    times = {k: [] for k in options}
    for _ in range(repeats):
        for name, opts in options.items():
            step = TrainStep('vnet', 1, 2, loss_name=name, device=dev, seed=0, use_graph=True, loss_options=opts)
            for _ in range(5):
                step(x, t)
            torch.cuda.synchronize()
            assert step._graph is not None, 'the train step was not captured'
            t0 = time.perf_counter()
            for _ in range(steps):
                step(x, t)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / steps)
            del step
            gc.collect()
            torch.cuda.synchronize()
            _ops.PACK_CACHE.clear()
    diff = [a - b for a, b in zip(times['DiceBoundary'], times['DiceCE'])]
    return {'shape': [N, 1, EDGE, EDGE, EDGE], 'net': 'vnet(1, 2)', 'steps_per_block': steps,
            'ms_per_step': {k: summary(v) for k, v in times.items()}, 'DiceBoundary_minus_DiceCE_ms': summary(diff)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10, help='calls per captured graph')
    ap.add_argument('--steps', type=int, default=30, help='train steps per timed block')
    ap.add_argument('--step-repeats', type=int, default=5, help='timed blocks per loss')
    ap.add_argument('--no-steps', action='store_true', help='kernels only')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'boundary_loss_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_boundary_loss.py needs a ROCm device: timings are taken on the GPU only')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    result = {'device': torch.cuda.get_device_name(dev), 'repeats': args.repeats, 'inner': args.inner}
    r = bench_kernels(dev, args.repeats, args.inner)
    result['kernels'] = r
    print('--- 4 x {} x 96^3: us per call, median [min, max] over {} repeats'.format(C, args.repeats))
    for k, v in r['us_per_call'].items():
        print('  {:22s} {:9.1f} [{:9.1f}, {:9.1f}]'.format(k, v['median'], v['min'], v['max']))
    for k, v in r['signed_distance'].items():
        print('  signed_distance {}: {:.1f} x the copy floor, {:.3e} min-plus candidates / s'.format(
            k, v['times_the_copy_floor'], v['candidates_per_s']))
    if not args.no_steps:
        result['train_step'] = bench_steps(dev, args.step_repeats, args.steps)
        for k, v in result['train_step']['ms_per_step'].items():
            print('  TrainStep {:13s} {:8.3f} [{:8.3f}, {:8.3f}] ms / step'.format(k, v['median'], v['min'], v['max']))
        d = result['train_step']['DiceBoundary_minus_DiceCE_ms']
        print('  DiceBoundary - DiceCE    {:8.3f} [{:8.3f}, {:8.3f}] ms / step'.format(d['median'], d['min'], d['max']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
