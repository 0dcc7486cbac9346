"""Device timing of the Dice + top-k loss next to DiceCE and a device-to-device copy.

  python tools/bench_topk_loss.py [--repeats 7] [--inner 20] [--steps 30] [--step-repeats 5] [--no-steps]
                                  [--out profiles/topk_loss_bench.json]

On probabilities 4 x C x 96^3 (C = 2 and 5), in ONE process:
  DiceTopK fwd / fwd+bwd   the top-k loss (k_percent = 10): zero + pass A + 3 x (histogram, scan) + sum + finalize; backward
  DiceCE fwd / fwd+bwd     the compound loss with gamma = 0 (one fused reduction + finalize; backward)
  copy                     a device-to-device copy of the probabilities tensor (reads and writes N*C*S*4 bytes each)
Every figure is `inner` back-to-back calls captured in one hipGraph, one warm-up replay, one replay between two device
events, event time / inner.  ONE captured graph is alive at a time: per repeat and variant the graph is captured, timed,
dropped, and the device synchronised; the variants alternate inside every repeat.  Medians with [min, max] over the repeats.
The buffers fit the 256 MB last-level cache, for the copy as for the losses, so rates are given as a fraction of the copy
rate of the same run on the ALGORITHMIC bytes: pass A (C + 2) * 4 per voxel, each refine pass (3 histograms) and the sum
pass 4 per voxel, backward (2C + 2) * 4 per voxel.  The split of the forward into its launches comes from a kernel trace
of this tool (profiles/topk_loss_kernel_stats.csv), not from here.

Then TrainStep('vnet', 1, 2) on 4 x 1 x 96^3 with DiceTopK and with DiceCE (whole step in a hipGraph), alternated in
blocks of `steps` steps -- one TrainStep alive at a time, as tools/bench_loss.py's bench_steps does it.
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
K_PERCENT = 10.0


def summary(values):
    return {'median': statistics.median(values), 'min': min(values), 'max': max(values)}


def timed_capture(fn, inner):
    """capture `inner` calls of fn, replay once to warm up, time one replay, drop the graph, synchronise: us per call"""
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
    torch.cuda.synchronize()
    return us


def bench_losses(dev, C, repeats, inner):
    gen = torch.Generator().manual_seed(C)
    p = torch.softmax(2.0 * torch.randn((N, C, EDGE, EDGE, EDGE), generator=gen), dim=1).to(dev)
    t = torch.randint(0, C, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    pg = p.clone().requires_grad_(True)
    dst = torch.empty_like(p)
    nvox = N * EDGE ** 3
    losses = {'DiceTopK': build_loss('DiceTopK', C, None, 2, topk_percent=K_PERCENT), 'DiceCE': build_loss('DiceCE', C, None, 2)}
    variants = {}
    for name, loss_fn in losses.items():
        def fwd(loss_fn=loss_fn):
            with torch.no_grad():
                loss_fn(p, t)

        def both(loss_fn=loss_fn):
            pg.grad = None
            loss_fn(pg, t).backward()
        variants[name + ' fwd'] = fwd
        variants[name + ' fwd+bwd'] = both
    variants['copy'] = lambda: dst.copy_(p)
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():          # alternated: every repeat visits every variant once, one graph at a time
            times[k].append(timed_capture(fn, inner))
    res = {k: summary(v) for k, v in times.items()}
    copy_rate = 2 * 4 * nvox * C / (res['copy']['median'] * 1e-6)
    selection = [int(v) for v in losses['DiceTopK'].last_selection.cpu()]
    passes = {'pass_A': (C + 2) * 4 * nvox, 'refine_x3': 3 * 4 * nvox, 'sum': 4 * nvox}
    fwd_bytes = {'DiceTopK': sum(passes.values()), 'DiceCE': (C + 1) * 4 * nvox}
    bwd_bytes = {'DiceTopK': (2 * C + 2) * 4 * nvox, 'DiceCE': (2 * C + 1) * 4 * nvox}
    out = {'shape': [N, C, EDGE, EDGE, EDGE], 'k_percent': K_PERCENT, 'selection_n_k_m_neq_r': selection,
           'us_per_call': res, 'copy_bytes_per_s': copy_rate, 'topk_forward_algorithmic_bytes': passes, 'losses': {}}
    for name in losses:
        tf = res[name + ' fwd']['median']
        tb = res[name + ' fwd+bwd']['median'] - tf
        out['losses'][name] = {
            'fwd_bytes': fwd_bytes[name], 'bwd_bytes': bwd_bytes[name], 'fwd_us': tf, 'bwd_us_by_difference': tb,
            'fwd_fraction_of_copy_rate': fwd_bytes[name] / (tf * 1e-6) / copy_rate,
            'bwd_fraction_of_copy_rate': bwd_bytes[name] / (tb * 1e-6) / copy_rate}
    return out


def bench_steps(dev, repeats, steps):
    """A B A B ...: every block builds its own TrainStep, warms it up (two eager steps, the capture, two replays), times
    `steps` replays and drops it again: one captured TrainStep alive at a time"""
    from segmentation3d import _ops
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((N, 1, EDGE, EDGE, EDGE), generator=gen).to(dev)
    t = torch.randint(0, 2, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    options = {'DiceTopK': {'topk_percent': K_PERCENT}, 'DiceCE': None}
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
    diff = [a - b for a, b in zip(times['DiceTopK'], times['DiceCE'])]
    return {'shape': [N, 1, EDGE, EDGE, EDGE], 'net': 'vnet(1, 2)', 'steps_per_block': steps,
            'ms_per_step': {k: summary(v) for k, v in times.items()}, 'DiceTopK_minus_DiceCE_ms': summary(diff)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20, help='calls per captured graph')
    ap.add_argument('--steps', type=int, default=30, help='train steps per timed block')
    ap.add_argument('--step-repeats', type=int, default=5, help='timed blocks per loss')
    ap.add_argument('--no-steps', action='store_true', help='loss kernels only')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'topk_loss_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_topk_loss.py needs a ROCm device: timings are taken on the GPU only')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    result = {'device': torch.cuda.get_device_name(dev), 'repeats': args.repeats, 'inner': args.inner, 'sizes': {}}
    for C in (2, 5):
        r = bench_losses(dev, C, args.repeats, args.inner)
        result['sizes']['C{}'.format(C)] = r
        print('--- 4 x {} x 96^3: us per call, median [min, max] over {} repeats; (n, k, m, n_eq, r) = {}'.format(
            C, args.repeats, r['selection_n_k_m_neq_r']))
        for k, v in r['us_per_call'].items():
            print('  {:18s} {:9.1f} [{:9.1f}, {:9.1f}]'.format(k, v['median'], v['min'], v['max']))
        print('  copy rate {:.3e} B/s'.format(r['copy_bytes_per_s']))
        for k, v in r['losses'].items():
            print('  {:10s} fwd {:>11d} B {:6.2f} of copy rate | bwd {:>11d} B {:6.2f} of copy rate'.format(
                k, v['fwd_bytes'], v['fwd_fraction_of_copy_rate'], v['bwd_bytes'], v['bwd_fraction_of_copy_rate']))
    if not args.no_steps:
        result['train_step'] = bench_steps(dev, args.step_repeats, args.steps)
        for k, v in result['train_step']['ms_per_step'].items():
            print('  TrainStep {:9s} {:8.3f} [{:8.3f}, {:8.3f}] ms / step'.format(k, v['median'], v['min'], v['max']))
        d = result['train_step']['DiceTopK_minus_DiceCE_ms']
        print('  DiceTopK - DiceCE    {:8.3f} [{:8.3f}, {:8.3f}] ms / step'.format(d['median'], d['min'], d['max']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
