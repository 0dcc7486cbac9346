"""Device timing of the loss kernels and of the train step with the compound loss.

  python tools/bench_loss.py [--repeats 7] [--inner 20] [--steps 30] [--step-repeats 5] [--out profiles/loss_bench.json]

On probabilities 4 x C x 96^3 (C = 2 and 5), in ONE process, the variants alternated inside every repeat:
  Dice, Focal          the existing losses (MultiDiceLoss, FocalLoss gamma = 2)
  DiceCE, DiceFocal    the compound loss with gamma = 0 / gamma = 2
  copy                 a device-to-device copy of the probabilities tensor (reads and writes N*C*S*4 bytes each)
Every variant is `inner` back-to-back launches captured in one hipGraph (no host work between the kernels), one warm-up
replay, then per repeat one replay between two device events; the figure is event time / inner.  "fwd" is the forward
alone (partial + finalize kernels), "fwd+bwd" both passes; the backward kernel's time is their difference.
The buffers (28 MB at C = 2, 71 MB at C = 5) are re-read by every launch and fit the 256 MB last-level cache, for the copy
just as for the losses -- inside a train step the probabilities were likewise written just before the loss reads them.
Rates are therefore given as a fraction of the copy rate of the same run, not of the HBM peak.

Then TrainStep('vnet', 1, 2) on 4 x 1 x 96^3 with Dice and with DiceCE (whole step in a hipGraph, as bench.py runs it),
alternated in blocks of `steps` steps (a fresh TrainStep per block, warmed up before its window), a device synchronise
around each block.
Medians with min / max over the repeats; algorithmic bytes per launch are computed from the shapes.
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

from segmentation3d.core.seg_train import TrainStep, build_loss       # noqa: E402

N, EDGE = 4, 96


def algorithmic_bytes(name, C, nvox):
    """(forward, backward) bytes a launch has to move: target + planes read, planes written (fp32)"""
    t, planes = 4 * nvox, 4 * nvox * C
    if name == 'Focal':                       # reads the target and the one probability it selects
        return t + 4 * nvox, t + 4 * nvox + planes
    if name == 'Dice':
        return t + planes, t + planes + planes
    # compound: the forward reads everything once; the backward reads the target and p_t (C <= 5: all planes with
    # 16-byte loads) and writes C planes
    return t + planes, t + (planes if C <= 5 else 4 * nvox) + planes


def summary(values):
    return {'median': statistics.median(values), 'min': min(values), 'max': max(values)}


def capture(fn, inner):
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
    return g


def time_graph(g, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / inner     # us per launch


def bench_losses(dev, C, repeats, inner):
    gen = torch.Generator().manual_seed(C)
    p = torch.softmax(2.0 * torch.randn((N, C, EDGE, EDGE, EDGE), generator=gen), dim=1).to(dev)
    t = torch.randint(0, C, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    pg = p.clone().requires_grad_(True)
    dst = torch.empty_like(p)
    nvox = N * EDGE ** 3
    graphs = {}
    for name in ('Dice', 'Focal', 'DiceCE', 'DiceFocal'):
        loss_fn = build_loss(name, C, None, 2)

        def fwd(loss_fn=loss_fn):
            with torch.no_grad():
                loss_fn(p, t)

        def both(loss_fn=loss_fn):
            pg.grad = None
            loss_fn(pg, t).backward()
        graphs[name + ' fwd'] = capture(fwd, inner)
        graphs[name + ' fwd+bwd'] = capture(both, inner)
    graphs['copy'] = capture(lambda: dst.copy_(p), inner)
    times = {k: [] for k in graphs}
    for _ in range(repeats):
        for k, g in graphs.items():            # alternated: every repeat visits every variant once
            times[k].append(time_graph(g, inner))
    res = {k: summary(v) for k, v in times.items()}
    copy_rate = 2 * 4 * nvox * C / (res['copy']['median'] * 1e-6)
    out = {'shape': [N, C, EDGE, EDGE, EDGE], 'us_per_launch': res, 'copy_bytes_per_s': copy_rate, 'kernels': {}}
    for name in ('Dice', 'Focal', 'DiceCE', 'DiceFocal'):
        bf, bb = algorithmic_bytes(name, C, nvox)
        tf = res[name + ' fwd']['median']
        tb = res[name + ' fwd+bwd']['median'] - tf
        out['kernels'][name] = {
            'fwd_bytes': bf, 'bwd_bytes': bb, 'fwd_us': tf, 'bwd_us_by_difference': tb,
            'fwd_bytes_per_s': bf / (tf * 1e-6), 'bwd_bytes_per_s': bb / (tb * 1e-6),
            'fwd_fraction_of_copy_rate': bf / (tf * 1e-6) / copy_rate, 'bwd_fraction_of_copy_rate': bb / (tb * 1e-6) / copy_rate}
    pair = [a + b for a, b in zip(times['Dice fwd+bwd'], times['Focal fwd+bwd'])]
    out['unfused_Dice_plus_Focal_us'] = summary(pair)
    out['DiceFocal_us'] = res['DiceFocal fwd+bwd']
    return out


def bench_steps(dev, repeats, steps):
    """A B A B ...: every block builds its own TrainStep, warms it up (two eager steps, the capture, two replays), times
    `steps` replays and drops it again.  Two captured TrainSteps cannot be kept side by side in one process: the
    packed-weight cache (and the job table a captured step points at) is process-wide, so the second step's first
    re-pack replaces the table under the first one's graph."""
    from segmentation3d import _ops
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((N, 1, EDGE, EDGE, EDGE), generator=gen).to(dev)
    t = torch.randint(0, 2, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    times = {'Dice': [], 'DiceCE': []}
    for _ in range(repeats):
        for name in times:
            step = TrainStep('vnet', 1, 2, loss_name=name, obj_weight=[0.5, 0.5], device=dev, seed=0, use_graph=True)
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
    return {'shape': [N, 1, EDGE, EDGE, EDGE], 'net': 'vnet(1, 2)', 'steps_per_block': steps,
            'ms_per_step': {k: summary(v) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20, help='launches per captured graph')
    ap.add_argument('--steps', type=int, default=30, help='train steps per timed block')
    ap.add_argument('--step-repeats', type=int, default=5, help='timed blocks per loss')
    ap.add_argument('--no-steps', action='store_true', help='loss kernels only')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'loss_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_loss.py needs a ROCm device: timings are taken on the GPU only')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    result = {'device': torch.cuda.get_device_name(dev), 'repeats': args.repeats, 'inner': args.inner, 'losses': {}}
    for C in (2, 5):
        r = bench_losses(dev, C, args.repeats, args.inner)
        result['losses']['C{}'.format(C)] = r
        print('--- 4 x {} x 96^3: us per launch, median [min, max] over {} repeats'.format(C, args.repeats))
        for k, v in r['us_per_launch'].items():
            print('  {:18s} {:9.1f} [{:9.1f}, {:9.1f}]'.format(k, v['median'], v['min'], v['max']))
        print('  copy rate {:.3e} B/s'.format(r['copy_bytes_per_s']))
        for k, v in r['kernels'].items():
            print('  {:10s} fwd {:>11d} B {:6.2f} of copy rate | bwd {:>11d} B {:6.2f} of copy rate'.format(
                k, v['fwd_bytes'], v['fwd_fraction_of_copy_rate'], v['bwd_bytes'], v['bwd_fraction_of_copy_rate']))
        u, f = r['unfused_Dice_plus_Focal_us'], r['DiceFocal_us']
        print('  Dice + Focal (two launches of each pass) {:.1f} [{:.1f}, {:.1f}] us  vs  DiceFocal {:.1f} [{:.1f}, {:.1f}] us'
              .format(u['median'], u['min'], u['max'], f['median'], f['min'], f['max']))
    if not args.no_steps:
        result['train_step'] = bench_steps(dev, args.step_repeats, args.steps)
        for k, v in result['train_step']['ms_per_step'].items():
            print('  TrainStep {:7s} {:8.3f} [{:8.3f}, {:8.3f}] ms / step'.format(k, v['median'], v['min'], v['max']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
