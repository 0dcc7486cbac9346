"""Device timing of the optimizer kernels and of the train step with clipping / SGD.

  python tools/bench_optim.py [--repeats 7] [--inner 20] [--steps 30] [--step-repeats 5] [--out profiles/optim_bench.json]

On flat buffers of the size of vnet(1, 2)'s (14.56 M floats, every parameter padded to 64), in ONE process, the variants
alternated inside every repeat:
  adam            seg3d_adam_step          (host-side scalars: the eager default)   28 B / parameter
  adam_ctl        seg3d_adam_step_ctl      (scalars from the control block)         28 B / parameter
  sgd_ctl         seg3d_sgd_step_ctl       (Nesterov 0.99, weight decay 3e-5)       20 B / parameter
  sumsq           seg3d_grad_sumsq_partial (the norm pass of a clipping step)        4 B / parameter
  prepare         seg3d_optim_prepare      (one workgroup, reads the sumsq slots)
Every variant is `inner` back-to-back launches captured in one hipGraph, one warm-up replay, then per repeat one replay
between two device events; the figure is event time / inner.  The buffers are 58 MB each: the three or four of an update
(175 - 233 MB) can largely stay in the 256 MB last-level cache between back-to-back launches, so the rates are cache-warm
figures, not HBM rates.

Then TrainStep('vnet', 1, 2, 'DiceCE') on 4 x 1 x 96^3 (whole step in a hipGraph, as bench.py runs it) with
  Adam            as today          Adam+clip   max_grad_norm 12          SGD+clip+poly   the nnU-Net-family recipe
alternated in blocks of `steps` steps (a fresh TrainStep per block, warmed up before its window).  "Clipping costs X" is
the difference to the unclipped step OF THE SAME RUN.  Medians with min / max over the repeats.
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

from segmentation3d import _engine as E                               # noqa: E402
from segmentation3d.core.seg_train import TrainStep                   # noqa: E402

N, EDGE = 4, 96
BYTES_PER_PARAM = {'adam': 28, 'adam_ctl': 28, 'sgd_ctl': 20, 'sumsq': 4}
STEP_VARIANTS = {
    'Adam': ('Adam', None),
    'Adam+clip': ('Adam', {'max_grad_norm': 12.0}),
    'SGD+clip+poly': ('SGD', {'momentum': 0.99, 'nesterov': True, 'weight_decay': 3e-5, 'max_grad_norm': 12.0,
                              'lr_schedule': {'name': 'poly', 'total_steps': 1000}}),
}


def summary(values):
    return {'median': statistics.median(values), 'min': min(values), 'max': max(values)}


def capture(fn, inner):
    fn()
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


def flat_size():
    from segmentation3d.network import vnet
    return sum((p.numel() + 63) // 64 * 64 for p in vnet.SegmentationNet(1, 2).parameters())


def bench_kernels(dev, repeats, inner):
    n = flat_size()
    gen = torch.Generator().manual_seed(3)
    p = (0.05 * torch.randn(n, generator=gen)).to(dev)
    g = (1e-3 * torch.randn(n, generator=gen)).to(dev)
    m, v, buf = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    nparts = E.query('seg3d_grad_sumsq_part_count', n)
    part = torch.zeros(nparts, dtype=torch.float64, device=dev)
    step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    ctl = torch.zeros(8, dtype=torch.float32, device=dev)

    def prepare():
        E.call('seg3d_optim_prepare', E.ptr(step_dev), E.ptr(ctl), E.ptr(part), nparts, 1.0, 12.0, 1, 1e-2, 100000, 0, 0.9,
               0.9, 0.999, E.stream_ptr())

    def sumsq():
        E.call('seg3d_grad_sumsq_partial', E.ptr(g), n, E.ptr(part), E.stream_ptr())
    sumsq()
    prepare()            # the *_ctl variants read a valid control block
    fns = {
        'adam': lambda: E.call('seg3d_adam_step', E.ptr(p), E.ptr(g), E.ptr(m), E.ptr(v), n, 10, 1e-4, 0.9, 0.999, 1e-8,
                               0.0, 1.0, E.stream_ptr()),
        'adam_ctl': lambda: E.call('seg3d_adam_step_ctl', E.ptr(p), E.ptr(g), E.ptr(m), E.ptr(v), n, E.ptr(ctl), 0.9, 0.999,
                                   1e-8, 0.0, E.stream_ptr()),
        'sgd_ctl': lambda: E.call('seg3d_sgd_step_ctl', E.ptr(p), E.ptr(g), E.ptr(buf), n, E.ptr(ctl), 0.99, 3e-5, 1,
                                  E.stream_ptr()),
        'sumsq': sumsq,
        'prepare': prepare,
    }
    graphs = {k: capture(fn, inner) for k, fn in fns.items()}
    times = {k: [] for k in graphs}
    for _ in range(repeats):
        for k, gr in graphs.items():            # alternated: every repeat visits every variant once
            times[k].append(time_graph(gr, inner))
    res = {k: summary(t) for k, t in times.items()}
    out = {'floats': n, 'sumsq_slots': nparts, 'us_per_launch': res, 'bytes_per_launch': {}, 'bytes_per_s': {}}
    for k, b in BYTES_PER_PARAM.items():
        out['bytes_per_launch'][k] = b * n
        out['bytes_per_s'][k] = b * n / (res[k]['median'] * 1e-6)
    return out


def bench_steps(dev, repeats, steps):
    """A B C A B C ...: every block builds its own TrainStep (two captured TrainSteps cannot be kept side by side: the
    packed-weight cache is process-wide), warms it up, times `steps` replays and drops it again"""
    from segmentation3d import _ops
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((N, 1, EDGE, EDGE, EDGE), generator=gen).to(dev)
    t = torch.randint(0, 2, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    times = {k: [] for k in STEP_VARIANTS}
    coef = {}
    for _ in range(repeats):
        for name, (optimizer, options) in STEP_VARIANTS.items():
            step = TrainStep('vnet', 1, 2, loss_name='DiceCE', obj_weight=[0.5, 0.5], device=dev, seed=0, use_graph=True,
                             optimizer=optimizer, optim_options=options)
            for _ in range(5):
                step(x, t)
            torch.cuda.synchronize()
            assert step._graph is not None, 'the train step was not captured'
            t0 = time.perf_counter()
            for _ in range(steps):
                step(x, t)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / steps)
            if step.opt.last_clip_coef is not None:
                coef[name] = float(step.opt.last_clip_coef)
            del step
            gc.collect()
            _ops.PACK_CACHE.clear()
    res = {k: summary(v) for k, v in times.items()}
    return {'shape': [N, 1, EDGE, EDGE, EDGE], 'net': 'vnet(1, 2)', 'loss': 'DiceCE', 'steps_per_block': steps,
            'ms_per_step': res, 'last_clip_coef': coef,
            'clip_cost_ms_vs_same_run_adam': res['Adam+clip']['median'] - res['Adam']['median'],
            'sgd_recipe_ms_vs_same_run_adam': res['SGD+clip+poly']['median'] - res['Adam']['median']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20, help='launches per captured graph')
    ap.add_argument('--steps', type=int, default=30, help='train steps per timed block')
    ap.add_argument('--step-repeats', type=int, default=5, help='timed blocks per variant')
    ap.add_argument('--no-steps', action='store_true', help='kernels only')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'optim_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_optim.py needs a ROCm device: timings are taken on the GPU only')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    result = {'device': torch.cuda.get_device_name(dev), 'repeats': args.repeats, 'inner': args.inner}
    r = result['kernels'] = bench_kernels(dev, args.repeats, args.inner)
    print('--- {} floats: us per launch, median [min, max] over {} repeats'.format(r['floats'], args.repeats))
    for k, v in r['us_per_launch'].items():
        rate = '  {:.3e} B/s'.format(r['bytes_per_s'][k]) if k in r['bytes_per_s'] else ''
        print('  {:10s} {:9.1f} [{:9.1f}, {:9.1f}]{}'.format(k, v['median'], v['min'], v['max'], rate))
    if not args.no_steps:
        s = result['train_step'] = bench_steps(dev, args.step_repeats, args.steps)
        for k, v in s['ms_per_step'].items():
            print('  TrainStep {:14s} {:8.3f} [{:8.3f}, {:8.3f}] ms / step'.format(k, v['median'], v['min'], v['max']))
        print('  clipping costs {:+.3f} ms, the SGD recipe {:+.3f} ms against the Adam step of this run'.format(
            s['clip_cost_ms_vs_same_run_adam'], s['sgd_recipe_ms_vs_same_run_adam']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
