"""Device timing of the region loss, the region confusion counts and the train step of a region-based model (DESIGN.md
section 7 row f23).

  python tools/bench_region_loss.py [--repeats 7] [--inner 20] [--steps 30] [--out profiles/region_loss_bench.json]

On sigmoid probabilities 4 x 3 x 96^3 with BraTS's regions, in ONE process:
  RegionDiceBCE      the fused loss, forward alone and forward + backward
  torch              the same loss composed from stock torch device ops (table gather, masked sums, clamp, log)
  copy               a device-to-device copy that moves the loss's algorithmic bytes (reads half of them, writes half)
  DiceCE             the compound loss at C = 3 on soft-max probabilities of the same shape
  region counts      seg3d_region_confusion_counts (R = 3) next to seg3d_confusion_counts (C = 3)
Every variant is `inner` back-to-back calls captured in one hipGraph, one warm-up replay, one timed replay between two device
events; the figure is event time / inner.  Unlike tools/bench_loss.py a block captures, times and DROPS its graph before the
next block captures its own: at most one captured graph is alive at any time.  The blocks alternate
A B .. A B ..: every repeat visits every variant once.  The buffers (14 MB per plane set) are re-read by every launch and fit
the last-level cache, for the copy just as for the losses, so rates are fractions of the copy's, not of the HBM peak.

Then TrainStep('vnet', 1, .) on 4 x 1 x 96^3 with RegionDiceBCE (R = 3) and with DiceCE (C = 3), whole step in a hipGraph,
alternated in blocks of `steps` steps; every block builds its own TrainStep, warms it up, times it and drops it, followed by
gc.collect() and PACK_CACHE.clear(): no two TrainSteps exist side by side.
Medians with min / max over the repeats.  Not measured: other R or shapes, the scalar path, bf16 activation mode, HBM-cold
buffers, several GPUs.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'medical-segmentation3d-toolkit_amd'))
sys.path.insert(0, REPO)

from segmentation3d import _ops                                           # noqa: E402
from segmentation3d.core.seg_train import TrainStep, build_loss           # noqa: E402
from segmentation3d.loss.region_loss import region_lut                    # noqa: E402

N, EDGE, R = 4, 96, 3
REGIONS, ORDER = [[1, 2, 3], [1, 3], [3]], [2, 1, 3]


def summary(values):
    return {'median': statistics.median(values), 'min': min(values), 'max': max(values)}


def timed_block(fn, inner):
    """capture `inner` calls of fn, replay once to warm up, time one replay, drop the graph: us per call"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / inner
    del g
    gc.collect()
    return us


def torch_region_loss(p, t, member):
    """RegionDiceBCE with unit weights from stock torch ops; member: bool [256, R] on the device"""
    n, r = p.shape[0], p.shape[1]
    T = t.reshape(n, -1)
    label = (T >= 0) & (T < 256) & (T == T.floor())
    z = member[torch.where(label, T, torch.zeros_like(T)).long()].permute(0, 2, 1) & label.unsqueeze(1)
    m, zf, P = label.unsqueeze(1).float(), z.float(), p.reshape(n, r, -1)
    d = (2.0 * (P * zf).sum(2) + 1e-5) / ((P * m).sum(2) + zf.sum(2) + 1e-5)
    q = torch.where(z, P, 1.0 - P).clamp_min(1e-12)
    return (1.0 - d.mean(0)).mean() + (-torch.log(q) * m).sum() / (m.sum() * r).clamp_min(1.0)


def bench_kernels(dev, repeats, inner):
    gen = torch.Generator().manual_seed(3)
    shape = (N, R, EDGE, EDGE, EDGE)
    nvox = N * EDGE ** 3
    p = torch.sigmoid(2.0 * torch.randn(shape, generator=gen)).to(dev)
    ps = torch.softmax(2.0 * torch.randn(shape, generator=gen), dim=1).to(dev)
    t = torch.randint(0, 4, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    tc = torch.randint(0, R, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    pg, psg = p.clone().requires_grad_(True), ps.clone().requires_grad_(True)
    lut = region_lut(REGIONS)
    member = torch.tensor([[(w >> r) & 1 for r in range(R)] for w in lut], dtype=torch.bool, device=dev)
    region, dicece = build_loss('RegionDiceBCE', 4, None, 2, regions=REGIONS), build_loss('DiceCE', R, None, 2)
    fwd_bytes, bwd_bytes = 4 * nvox * (R + 1), 4 * nvox * (2 * R + 1)
    src_f, src_b = (torch.empty(nb // 8, device=dev) for nb in (fwd_bytes, fwd_bytes + bwd_bytes))   # floats: half the bytes
    dst_f, dst_b = torch.empty_like(src_f), torch.empty_like(src_b)
    counts_r, counts_c = (torch.zeros((R, 3), dtype=torch.int64, device=dev) for _ in range(2))

    def no_grad(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    def both(loss, x, target):
        def run():
            x.grad = None
            loss(x, target).backward()
        return run

    variants = {
        'RegionDiceBCE fwd': no_grad(lambda: region(p, t)),
        'RegionDiceBCE fwd+bwd': both(region, pg, t),
        'torch fwd': no_grad(lambda: torch_region_loss(p, t, member)),
        'torch fwd+bwd': both(lambda x, y: torch_region_loss(x, y, member), pg, t),
        'copy fwd bytes': lambda: dst_f.copy_(src_f),
        'copy fwd+bwd bytes': lambda: dst_b.copy_(src_b),
        'DiceCE fwd': no_grad(lambda: dicece(ps, tc)),
        'DiceCE fwd+bwd': both(dicece, psg, tc),
        'region_confusion_counts': lambda: _ops.region_confusion_counts(p, t, lut, out=counts_r),
        'confusion_counts': lambda: _ops.confusion_counts(ps, tc, out=counts_c),
    }
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():            # alternated: every repeat visits every variant once, one graph at a time
            times[k].append(timed_block(fn, inner))
    res = {k: summary(v) for k, v in times.items()}
    rate_f = fwd_bytes / (res['copy fwd bytes']['median'] * 1e-6)
    rate_b = (fwd_bytes + bwd_bytes) / (res['copy fwd+bwd bytes']['median'] * 1e-6)
    fused_f, fused_b = res['RegionDiceBCE fwd']['median'], res['RegionDiceBCE fwd+bwd']['median']
    return {'shape': list(shape), 'regions': REGIONS, 'us_per_call': res,
            'algorithmic_bytes': {'fwd': fwd_bytes, 'bwd': bwd_bytes, 'counts': fwd_bytes},
            'copy_bytes_per_s': {'fwd': rate_f, 'fwd+bwd': rate_b},
            'fraction_of_copy_rate': {'fwd': fwd_bytes / (fused_f * 1e-6) / rate_f,
                                      'fwd+bwd': (fwd_bytes + bwd_bytes) / (fused_b * 1e-6) / rate_b,
                                      'region_confusion_counts': fwd_bytes / (res['region_confusion_counts']['median'] * 1e-6) / rate_f,
                                      'confusion_counts': fwd_bytes / (res['confusion_counts']['median'] * 1e-6) / rate_f},
            'torch_over_fused': {'fwd': res['torch fwd']['median'] / fused_f, 'fwd+bwd': res['torch fwd+bwd']['median'] / fused_b},
            'DiceCE_over_fused': {'fwd': res['DiceCE fwd']['median'] / fused_f, 'fwd+bwd': res['DiceCE fwd+bwd']['median'] / fused_b}}


def bench_steps(dev, repeats, steps):
    """A B A B ...: every block builds its own TrainStep, warms it up (two eager steps, the capture, two replays), times
    `steps` replays and drops it again (tools/bench_loss.py bench_steps)"""
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((N, 1, EDGE, EDGE, EDGE), generator=gen).to(dev)
    targets = {'RegionDiceBCE': torch.randint(0, 4, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev),
               'DiceCE': torch.randint(0, R, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)}
    kwargs = {'RegionDiceBCE': dict(regions=REGIONS, region_class_order=ORDER), 'DiceCE': {}}
    times = {k: [] for k in targets}
    for _ in range(repeats):
        for name, t in targets.items():
            step = TrainStep('vnet', 1, 4 if name == 'RegionDiceBCE' else R, loss_name=name, device=dev, seed=0, use_graph=True,
                             **kwargs[name])
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
            _ops.PACK_CACHE.clear()
    return {'shape': [N, 1, EDGE, EDGE, EDGE], 'net': 'vnet(1, 3 outputs)', 'steps_per_block': steps,
            'ms_per_step': {k: summary(v) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20, help='calls per captured graph')
    ap.add_argument('--steps', type=int, default=30, help='train steps per timed block')
    ap.add_argument('--no-steps', action='store_true', help='kernels only')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'region_loss_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_region_loss.py needs a ROCm device: timings are taken on the GPU only')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    result = {'device': torch.cuda.get_device_name(dev), 'repeats': args.repeats, 'inner': args.inner,
              'not_measured': ['other R or shapes', 'the scalar path', 'bf16 activation mode', 'HBM-cold buffers', 'several GPUs'],
              'kernels': bench_kernels(dev, args.repeats, args.inner)}
    print('--- 4 x 3 x 96^3: us per call, median [min, max] over {} repeats'.format(args.repeats))
    for k, v in result['kernels']['us_per_call'].items():
        print('  {:26s} {:9.1f} [{:9.1f}, {:9.1f}]'.format(k, v['median'], v['min'], v['max']))
    for key in ('fraction_of_copy_rate', 'torch_over_fused', 'DiceCE_over_fused'):
        print('  {}: {}'.format(key, {k: round(v, 3) for k, v in result['kernels'][key].items()}))
    if not args.no_steps:
        result['train_step'] = bench_steps(dev, args.repeats, args.steps)
        for k, v in result['train_step']['ms_per_step'].items():
            print('  TrainStep {:14s} {:8.3f} [{:8.3f}, {:8.3f}] ms / step'.format(k, v['median'], v['min'], v['max']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
