"""Device timing of the Dice + clDice loss and its soft skeleton next to DiceCE, a
device-to-device copy of the bytes the kernels must move, and the same loss composed from stock torch device ops.

  python tools/bench_cldice_loss.py [--repeats 7] [--inner 10] [--steps 30] [--step-repeats 5] [--no-steps]
                                    [--out profiles/cldice_loss_bench.json]

On 4 x 2 x 96^3 (probabilities) / 4 x 96^3 (target) with iters = 3, in ONE process, the method of tools/bench_topk_loss.py:
  soft_skeleton              seg3d_soft_skeleton alone on the N foreground probability planes (iters + 1 stage launches)
  DiceClDice fwd / fwd+bwd   the loss: Dice partial sums, both skeletons, the four sums, finalize; backward: iters + 1 gather
                             passes and the pass that writes dprobs
  DiceCE fwd / fwd+bwd       the compound loss with gamma = 0
  copy fwd / copy fwd+bwd    a device-to-device copy moving the bytes the kernels must move if every tile read its halo
                             from cache (moved_bytes below) -- the floor of the staged design
  stock fwd / fwd+bwd        the same loss from max_pool3d / relu / sums with autograd, fp32 on the device
Every figure is `inner` back-to-back calls captured in one hipGraph, one warm-up replay, one replay between two device
events, event time / inner.  ONE captured graph is alive at a time; the variants alternate inside every repeat.  Medians
with [min, max] over the repeats.

Then TrainStep('vnet', 1, 2) on 4 x 1 x 96^3 with DiceClDice and with DiceCE (whole step in a hipGraph), alternated in
blocks of `steps` steps -- one TrainStep alive at a time -- and their difference per pair of blocks.
"""
import argparse
import gc
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'medical-segmentation3d-toolkit_amd'))
sys.path.insert(0, os.path.join(REPO, 'tools'))
sys.path.insert(0, REPO)

from bench_topk_loss import summary, timed_capture                    # noqa: E402
from segmentation3d import _ops                                        # noqa: E402
from segmentation3d.core.seg_train import TrainStep, build_loss       # noqa: E402

N, EDGE, C, ITERS, K = 4, 96, 2, 3, 1


def moved_bytes(n, c, k, s, iters):
    """bytes the kernels read and write per call when a tile's halo comes from cache: (forward, backward)"""
    plane = n * k * s
    # target skeleton: stage 0 reads the target, writes x_1 and s; a middle stage reads and writes x and s; the last
    # stage writes no x.  The prediction's stage 0 also reads the probability; every stage keeps 9 bytes per voxel.
    target_skel = 12 + 16 * (iters - 1) + 12
    pred_skel = 16 + 16 * (iters - 1) + 12 + 9 * (iters + 1)
    fwd = plane * (target_skel + pred_skel + 16) + n * s * 4 * (c + 1)      # + the four sums, + the Dice partial sums
    # stage k reads the target and its 9 bytes, writes dL/ds and dL/dx; a middle stage also reads those two; stage 0 reads
    # no b and writes no dL/ds; the last pass reads the target, dL/dP and ST per listed class and writes C planes
    bwd = plane * (21 + 25 * (iters - 1) + 17 + 8) + n * s * 4 * (1 + c)
    return fwd, bwd


def stock_loss(p, t, iters):
    """Dice + clDice for C = 2, class list [1], no ignore label, from stock torch ops (fp32, autograd)"""
    def erode(x):
        return torch.min(torch.min(-F.max_pool3d(-x, (3, 1, 1), 1, (1, 0, 0)), -F.max_pool3d(-x, (1, 3, 1), 1, (0, 1, 0))),
                         -F.max_pool3d(-x, (1, 1, 3), 1, (0, 0, 1)))

    def skeleton(x):
        s = torch.relu(x - F.max_pool3d(erode(x), 3, 1, 1))
        for _ in range(iters):
            x = erode(x)
            d = torch.relu(x - F.max_pool3d(erode(x), 3, 1, 1))
            s = s + torch.relu(d - s * d)
        return s
    onehot = torch.cat([1.0 - t, t], dim=1)
    inter = (p * onehot).flatten(2).sum(-1)
    union = p.flatten(2).sum(-1) + onehot.flatten(2).sum(-1)
    l_dice = (1.0 - (2.0 * inter + 1e-5) / (union + 1e-5)).mean()
    sp, st = skeleton(p[:, 1:2]), skeleton(t)
    tprec = ((sp * t).flatten(1).sum(-1) + 1.0) / (sp.flatten(1).sum(-1) + 1.0)
    tsens = ((st * p[:, 1:2]).flatten(1).sum(-1) + 1.0) / (st.flatten(1).sum(-1) + 1.0)
    return l_dice + (1.0 - 2.0 * tprec * tsens / (tprec + tsens)).mean()


def bench_kernels(dev, repeats, inner):
    gen = torch.Generator().manual_seed(C)
    p = torch.softmax(2.0 * torch.randn((N, C, EDGE, EDGE, EDGE), generator=gen), dim=1).to(dev)
    p = torch.softmax(4.0 * F.avg_pool3d(torch.log(p), 5, stride=1, padding=2), dim=1).contiguous()   # blobs, not noise
    t = torch.randn((N, 1, EDGE, EDGE, EDGE), generator=gen).to(dev)
    t = (F.avg_pool3d(t, 9, stride=1, padding=4) > 0).float().contiguous()
    pg = p.clone().requires_grad_(True)
    S = EDGE ** 3
    losses = {'DiceClDice': build_loss('DiceClDice', C, None, 2, cldice_iters=ITERS), 'DiceCE': build_loss('DiceCE', C, None, 2)}
    ours = float(losses['DiceClDice'](p, t))
    stock = float(stock_loss(p, t, ITERS))
    fwd_bytes, bwd_bytes = moved_bytes(N, C, K, S, ITERS)
    fg = p[:, 1].contiguous()
    variants = {'soft_skeleton': lambda: _ops.soft_skeleton(fg, ITERS)}
    for name, nbytes in (('copy fwd', fwd_bytes), ('copy fwd+bwd', fwd_bytes + bwd_bytes)):
        src = torch.empty(nbytes // 8, device=dev)      # a copy of b bytes moves 2 b
        dst = torch.empty_like(src)
        variants[name] = lambda src=src, dst=dst: dst.copy_(src)
    for name, loss_fn in list(losses.items()) + [('stock', lambda a, b: stock_loss(a, b, ITERS))]:
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
    med = {k: v['median'] for k, v in res.items()}
    return {'shape': [N, C, EDGE, EDGE, EDGE], 'iters': ITERS, 'classes': [1], 'us_per_call': res,
            'loss_ours': ours, 'loss_stock': stock, 'moved_bytes': {'fwd': fwd_bytes, 'bwd': bwd_bytes},
            'times_the_copy_floor': {'fwd': med['DiceClDice fwd'] / med['copy fwd'],
                                     'fwd+bwd': med['DiceClDice fwd+bwd'] / med['copy fwd+bwd']},
            'stock_over_ours': {'fwd': med['stock fwd'] / med['DiceClDice fwd'],
                                'fwd+bwd': med['stock fwd+bwd'] / med['DiceClDice fwd+bwd']}}


def bench_steps(dev, repeats, steps):
    """A B A B ...: every block builds its own TrainStep, warms it up (two eager steps, the capture, two replays), times
    `steps` replays and drops it again: one captured TrainStep alive at a time"""
    gen = torch.Generator().manual_seed(7)
    x = torch.randn((N, 1, EDGE, EDGE, EDGE), generator=gen).to(dev)
    t = torch.randint(0, 2, (N, 1, EDGE, EDGE, EDGE), generator=gen).float().to(dev)
    options = {'DiceClDice': {'cldice_iters': ITERS}, 'DiceCE': None}
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
    diff = [a - b for a, b in zip(times['DiceClDice'], times['DiceCE'])]
    return {'shape': [N, 1, EDGE, EDGE, EDGE], 'net': 'vnet(1, 2)', 'steps_per_block': steps,
            'ms_per_step': {k: summary(v) for k, v in times.items()}, 'DiceClDice_minus_DiceCE_ms': summary(diff)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--inner', type=int, default=10, help='calls per captured graph')
    ap.add_argument('--steps', type=int, default=30, help='train steps per timed block')
    ap.add_argument('--step-repeats', type=int, default=5, help='timed blocks per loss')
    ap.add_argument('--no-steps', action='store_true', help='kernels only')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'cldice_loss_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_cldice_loss.py needs a ROCm device: timings are taken on the GPU only')
    dev = torch.device('cuda:0')
    torch.cuda.set_device(dev)
    result = {'device': torch.cuda.get_device_name(dev), 'repeats': args.repeats, 'inner': args.inner}
    r = bench_kernels(dev, args.repeats, args.inner)
    result['kernels'] = r
    print('--- 4 x {} x 96^3, iters = {}: us per call, median [min, max] over {} repeats'.format(C, ITERS, args.repeats))
    for k, v in r['us_per_call'].items():
        print('  {:22s} {:9.1f} [{:9.1f}, {:9.1f}]'.format(k, v['median'], v['min'], v['max']))
    print('  loss: fused {:.7f}, stock {:.7f}'.format(r['loss_ours'], r['loss_stock']))
    for k in ('fwd', 'fwd+bwd'):
        print('  {}: {:.1f} x the copy floor, stock / fused = {:.2f}'.format(k, r['times_the_copy_floor'][k],
                                                                         r['stock_over_ours'][k]))
    if not args.no_steps:
        result['train_step'] = bench_steps(dev, args.step_repeats, args.steps)
        for k, v in result['train_step']['ms_per_step'].items():
            print('  TrainStep {:13s} {:8.3f} [{:8.3f}, {:8.3f}] ms / step'.format(k, v['median'], v['min'], v['max']))
        d = result['train_step']['DiceClDice_minus_DiceCE_ms']
        print('  DiceClDice - DiceCE      {:8.3f} [{:8.3f}, {:8.3f}] ms / step'.format(d['median'], d['min'], d['max']))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
