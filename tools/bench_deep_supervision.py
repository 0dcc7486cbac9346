"""Device timing of the fused deep-supervision head and of the train step with deep supervision.

  python tools/bench_deep_supervision.py [--repeats 7] [--inner 20] [--steps 30] [--step-repeats 5]
                                         [--out profiles/deep_supervision_bench.json]

Head kernels, at the three shapes the heads see in the 4 x 96^3 train step (4 x 48^3 x 64, 4 x 24^3 x 128, 4 x 12^3 x 256,
C = 2), forward + backward, in ONE process, the variants alternated inside every repeat:
  fused      _ops.ds_head: seg3d_ds_head_fwd, then seg3d_ds_head_bwd + seg3d_ds_head_bwd_finalize
  baseline   what the package offered for the same arithmetic before: _ops.conv(x, w, b, 'k1') + _ops.softmax_channels and
             their autograd backward (tap-major direct conv, softmax, softmax backward, direct data- and weight-gradient)
  copy       a device-to-device copy of the feature tensor (reads and writes N*S*Cin*4 bytes each)
Every variant is `inner` back-to-back forward + backward passes captured in one hipGraph, one warm-up replay, then per repeat
one replay between two device events; the figure is event time / inner.  The feature tensors (113 / 28 / 7 MB) are re-read by
every pass and fit the 256 MB last-level cache, for the copy just as for the heads -- inside a train step the decoder wrote the
feature shortly before the head reads it.  Rates are therefore given as a fraction of the copy rate of the same run.
Algorithmic bytes of forward + backward: x read twice, dx written once, probabilities written once and read once, dprobs read
once (weights and partial slabs are noise): (3 Cin + 3 C) * 4 bytes per voxel.

Then TrainStep('vnet', 1, 2, 'DiceCE') on 4 x 1 x 96^3 with deep_supervision = 0 and 3 (whole step in a hipGraph, as bench.py
runs it), alternated in blocks of `steps` steps (a fresh TrainStep per block, warmed up before its window), a device
synchronise around each block.  Medians with min / max over the repeats.
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

from segmentation3d import _ops                                        # noqa: E402
from segmentation3d.core.seg_train import TrainStep                   # noqa: E402

N, EDGE, C = 4, 96, 2
HEAD_SHAPES = ((48, 64), (24, 128), (12, 256))     # (edge, Cin) of up_64 / up_128 / up_256 in the 4 x 96^3 step


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
    return a.elapsed_time(b) * 1e3 / inner     # us per pass


def bench_head(dev, edge, cin, repeats, inner):
    gen = torch.Generator().manual_seed(cin)
    xn = torch.randn((N, edge, edge, edge, cin), generator=gen).to(dev)
    x = xn.permute(0, 4, 1, 2, 3).requires_grad_(True)              # logical NCDHW, NDHWC memory: what the decoder hands over
    w = (torch.randn((C, cin, 1, 1, 1), generator=gen) / cin ** 0.5).to(dev).requires_grad_(True)
    b = torch.zeros(C).to(dev).requires_grad_(True)
    r = torch.randn((N, C, edge, edge, edge), generator=gen).to(dev)
    dst = torch.empty_like(xn)

    def run(head):
        x.grad = w.grad = b.grad = None
        head(x, w, b).backward(r)

    def fused(x_, w_, b_):
        return _ops.ds_head(x_, w_, b_)

    def baseline(x_, w_, b_):
        return _ops.softmax_channels(_ops.conv(x_, w_, b_, 'k1'))

    # the two variants compute the same thing: checked at the timed size before anything is timed
    run(fused)
    pf, gf = fused(x, w, b).detach(), (x.grad.clone(), w.grad.clone(), b.grad.clone())
    run(baseline)
    pb, gb = baseline(x, w, b).detach(), (x.grad.clone(), w.grad.clone(), b.grad.clone())
    diff = {'probs_max_abs': float((pf - pb).abs().max()),
            'grads_max_rel': max(float((a - c).abs().max() / (c.abs().max() + 1e-30)) for a, c in zip(gf, gb))}
    graphs = {'fused': capture(lambda: run(fused), inner), 'baseline': capture(lambda: run(baseline), inner),
              'copy': capture(lambda: dst.copy_(xn), inner)}
    times = {k: [] for k in graphs}
    for _ in range(repeats):
        for k, g in graphs.items():            # alternated: every repeat visits every variant once
            times[k].append(time_graph(g, inner))
    res = {k: summary(v) for k, v in times.items()}
    nvox = N * edge ** 3
    copy_rate = 2 * 4 * nvox * cin / (res['copy']['median'] * 1e-6)
    nbytes = (3 * cin + 3 * C) * 4 * nvox
    out = {'shape': [N, edge, edge, edge, cin], 'classes': C, 'us_per_pass_fwd_bwd': res, 'copy_bytes_per_s': copy_rate,
           'algorithmic_bytes_fwd_bwd': nbytes, 'fused_vs_baseline_difference': diff,
           'speedup_median': res['baseline']['median'] / res['fused']['median']}
    for k in ('fused', 'baseline'):
        out[k + '_fraction_of_copy_rate'] = nbytes / (res[k]['median'] * 1e-6) / copy_rate
    return out


def bench_steps(dev, repeats, steps):
    """A B A B ...: every block builds its own TrainStep, warms it up (two eager steps, the capture, two replays), times
    `steps` replays and drops it again (two captured TrainSteps cannot be kept side by side: the packed-weight cache is
    process-wide)."""
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((N, 1, EDGE, EDGE, EDGE), generator=gen).to(dev)
    t = torch.randint(0, 2, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    times = {0: [], 3: []}
    for _ in range(repeats):
        for levels in times:
            step = TrainStep('vnet', 1, 2, loss_name='DiceCE', device=dev, seed=0, use_graph=True, deep_supervision=levels)
            for _ in range(5):
                step(x, t)
            torch.cuda.synchronize()
            assert step._graph is not None, 'the train step was not captured'
            t0 = time.perf_counter()
            for _ in range(steps):
                step(x, t)
            torch.cuda.synchronize()
            times[levels].append((time.perf_counter() - t0) * 1e3 / steps)
            del step
            gc.collect()
            _ops.PACK_CACHE.clear()
    return {'shape': [N, 1, EDGE, EDGE, EDGE], 'net': 'vnet(1, 2)', 'loss': 'DiceCE', 'steps_per_block': steps,
            'ms_per_step': {'deep_supervision_{}'.format(k): summary(v) for k, v in times.items()},
            'extra_ms_median': statistics.median(times[3]) - statistics.median(times[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20, help='forward + backward passes per captured graph')
    ap.add_argument('--steps', type=int, default=30, help='train steps per timed block')
    ap.add_argument('--step-repeats', type=int, default=5, help='timed blocks per setting')
    ap.add_argument('--no-steps', action='store_true', help='head kernels only')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'deep_supervision_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_deep_supervision.py needs a ROCm device: timings are taken on the GPU only')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    result = {'device': torch.cuda.get_device_name(dev), 'repeats': args.repeats, 'inner': args.inner, 'heads': {}}
    for edge, cin in HEAD_SHAPES:
        r = bench_head(dev, edge, cin, args.repeats, args.inner)
        result['heads']['4x{}^3x{}'.format(edge, cin)] = r
        print('--- head 4 x {}^3 x {} -> {}: us per forward + backward, median [min, max] over {} repeats'.format(
            edge, cin, C, args.repeats))
        for k, v in r['us_per_pass_fwd_bwd'].items():
            print('  {:9s} {:9.1f} [{:9.1f}, {:9.1f}]'.format(k, v['median'], v['min'], v['max']))
        print('  fused {:.2f} / baseline {:.2f} of the copy rate ({:.3e} B/s) on {} algorithmic bytes; fused is {:.2f}x the '
              'baseline; difference {}'.format(r['fused_fraction_of_copy_rate'], r['baseline_fraction_of_copy_rate'],
                                               r['copy_bytes_per_s'], r['algorithmic_bytes_fwd_bwd'], r['speedup_median'],
                                               r['fused_vs_baseline_difference']))
    if not args.no_steps:
        result['train_step'] = bench_steps(dev, args.step_repeats, args.steps)
        for k, v in result['train_step']['ms_per_step'].items():
            print('  TrainStep {:20s} {:8.3f} [{:8.3f}, {:8.3f}] ms / step'.format(k, v['median'], v['min'], v['max']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
