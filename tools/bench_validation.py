"""Device timing of the confusion-count kernel and of a validation pass.

  python tools/bench_validation.py [--repeats 7] [--inner 20] [--pass-repeats 7] [--steps 10] [--out profiles/validation_bench.json]

(a) On probabilities 4 x C x 96^3 (C = 2 and 5), in ONE process, the variants alternated inside every repeat:
  kernel   _ops.confusion_counts (seg3d_confusion_counts): arg-max + per-class (tp, fp, fn) in one pass
  torch    the stock-torch chain it replaces: probs.argmax(1), then the 3 C masked sums
  copy     a device-to-device copy of the probabilities tensor (reads and writes N*C*S*4 bytes each)
Every variant is `inner` back-to-back calls captured in one hipGraph (no host work between the kernels), one warm-up replay,
then per repeat one replay between two device events; the figure is event time / inner.  As in tools/bench_loss.py the
buffers (28 MB at C = 2, 71 MB at C = 5) fit the last-level cache for every variant alike, so the kernel's rate on its
algorithmic bytes, (C + 1) * 4 per voxel, is given as a fraction of the copy rate of the same run, not of the HBM peak.

(b) ms per validation pass (core/seg_validate.Validator.run: 16 crops of 96^3, 4 per forward, vnet(1, 2), DiceCE; eager,
read-back included) next to the ms per train step of the TrainStep whose network it scores -- ONE TrainStep with its one
captured graph for the whole part, the two alternated inside every repeat, a device synchronise around each.
Medians with min / max over the repeats.
"""
import argparse
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
from segmentation3d.core.seg_train import TrainStep, build_loss       # noqa: E402
from segmentation3d.core.seg_validate import Validator                # noqa: E402

N, EDGE, CROPS = 4, 96, 16


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
    return a.elapsed_time(b) * 1e3 / inner     # us per call


def bench_counts(dev, C, repeats, inner):
    gen = torch.Generator().manual_seed(C)
    p = torch.softmax(2.0 * torch.randn((N, C, EDGE, EDGE, EDGE), generator=gen), dim=1).to(dev)
    t = torch.randint(0, C, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    dst = torch.empty_like(p)
    out_k = torch.zeros((C, 3), dtype=torch.int64, device=dev)
    out_t = torch.zeros((C, 3), dtype=torch.int64, device=dev)
    nvox = N * EDGE ** 3

    def kernel():
        out_k.zero_()
        _ops.confusion_counts(p, t, out=out_k)

    def chain():
        pred, tt = p.argmax(1), t[:, 0]
        for c in range(C):
            pc, tc = pred == c, tt == c
            out_t[c, 0] = (pc & tc).sum()
            out_t[c, 1] = (pc & ~tc).sum()
            out_t[c, 2] = (~pc & tc).sum()
    graphs = {'kernel': capture(kernel, inner), 'torch': capture(chain, inner), 'copy': capture(lambda: dst.copy_(p), inner)}
    assert torch.equal(out_k, out_t), 'the kernel and the torch chain disagree'
    times = {k: [] for k in graphs}
    for _ in range(repeats):
        for k, g in graphs.items():            # alternated: every repeat visits every variant once
            times[k].append(time_graph(g, inner))
    res = {k: summary(v) for k, v in times.items()}
    copy_rate = 2 * 4 * nvox * C / (res['copy']['median'] * 1e-6)
    nbytes = (C + 1) * 4 * nvox
    rate = nbytes / (res['kernel']['median'] * 1e-6)
    return {'shape': [N, C, EDGE, EDGE, EDGE], 'us_per_call': res, 'copy_bytes_per_s': copy_rate,
            'kernel_algorithmic_bytes': nbytes, 'kernel_bytes_per_s': rate, 'kernel_fraction_of_copy_rate': rate / copy_rate,
            'torch_over_kernel': res['torch']['median'] / res['kernel']['median'],
            'spreads_do_not_overlap': res['kernel']['max'] < res['torch']['min']}


def bench_pass(dev, repeats, steps):
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((N, 1, EDGE, EDGE, EDGE), generator=gen).to(dev)
    t = torch.randint(0, 2, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    crops = torch.randn((CROPS, 1, EDGE, EDGE, EDGE), generator=gen).to(dev)
    masks = torch.randint(0, 2, (CROPS, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    step = TrainStep('vnet', 1, 2, loss_name='DiceCE', obj_weight=[1.0, 1.0], device=dev, seed=0, use_graph=True)
    for _ in range(5):
        step(x, t)
    torch.cuda.synchronize()
    assert step._graph is not None, 'the train step was not captured'
    validator = Validator(step.net, build_loss('DiceCE', 2, [1.0, 1.0]), crops, masks, N)
    validator.run(0)                                                   # warm-up: allocator, plans of the no-grad forward
    times = {'train_step': [], 'validation_pass': []}
    for k in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step(x, t)
        torch.cuda.synchronize()
        times['train_step'].append((time.perf_counter() - t0) * 1e3 / steps)
        t0 = time.perf_counter()
        validator.run(k + 1)                                           # ends in its read-back: a synchronisation
        times['validation_pass'].append((time.perf_counter() - t0) * 1e3)
    res = {k: summary(v) for k, v in times.items()}
    return {'net': 'vnet(1, 2)', 'loss': 'DiceCE', 'crops': [CROPS, 1, EDGE, EDGE, EDGE], 'crops_per_forward': N,
            'train_shape': [N, 1, EDGE, EDGE, EDGE], 'steps_per_block': steps, 'ms': res,
            'pass_in_train_steps': res['validation_pass']['median'] / res['train_step']['median']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20, help='calls per captured graph')
    ap.add_argument('--pass-repeats', type=int, default=7, help='timed validation passes')
    ap.add_argument('--steps', type=int, default=10, help='train steps per timed block')
    ap.add_argument('--no-pass', action='store_true', help='kernel timings only')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'validation_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_validation.py needs a ROCm device: timings are taken on the GPU only')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    result = {'device': torch.cuda.get_device_name(dev), 'repeats': args.repeats, 'inner': args.inner, 'counts': {}}
    for C in (2, 5):
        r = bench_counts(dev, C, args.repeats, args.inner)
        result['counts']['C{}'.format(C)] = r
        print('--- 4 x {} x 96^3: us per call, median [min, max] over {} repeats'.format(C, args.repeats))
        for k, v in r['us_per_call'].items():
            print('  {:8s} {:9.1f} [{:9.1f}, {:9.1f}]'.format(k, v['median'], v['min'], v['max']))
        print('  kernel: {} B at {:.2f} of the copy rate ({:.3e} B/s); torch chain / kernel = {:.1f}; spreads apart: {}'.format(
            r['kernel_algorithmic_bytes'], r['kernel_fraction_of_copy_rate'], r['copy_bytes_per_s'], r['torch_over_kernel'],
            r['spreads_do_not_overlap']))
    if not args.no_pass:
        result['validation_pass'] = r = bench_pass(dev, args.pass_repeats, args.steps)
        for k, v in r['ms'].items():
            print('  {:16s} {:8.3f} [{:8.3f}, {:8.3f}] ms'.format(k, v['median'], v['min'], v['max']))
        print('  one pass of {} crops = {:.2f} train steps'.format(CROPS, r['pass_in_train_steps']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
