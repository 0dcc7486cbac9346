"""Whole-volume timing of Gaussian patch blending and mirror test-time augmentation.

  python tools/bench_blend_tta.py [--volume 512,512,400] [--batch 16] [--repeats 5] [--out profiles/blend_tta_bench.json]
      vnet(1, 2), fp32, box 96, stride 48.  Variants, alternated inside one process (one warm-up job each, then `repeats`
      rounds over all of them, device synchronise around every job):
        constant            the default path
        gaussian            Gaussian weights, no mirrors
        gaussian+x/xy/xyz   mirror TTA inside the gather / scatter kernels (one graph replay per batch)
        flip:x/xy/xyz       the same job with the mirrors done by torch.flip around the plain gather and the un-mirrored
                            blend scatter (captured in one graph per volume like the fused path)
  python tools/bench_blend_tta.py --trace-jobs
      one job each of constant, gaussian and gaussian+x on ONE stream, for a kernel trace taken from outside
      (rocprofv3 --kernel-trace --stats -- python tools/bench_blend_tta.py --trace-jobs); prints the algorithmic bytes
      per launch of the gather and scatter kernels so that the traced times turn into bytes / s.
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
sys.path.insert(0, REPO)

from segmentation3d.core import seg_infer as SI                        # noqa: E402
from segmentation3d.network import vnet                                # noqa: E402
from segmentation3d.utils.image_tools import image_partition_by_fixed_size   # noqa: E402

NORM = {'type': 1, 'clip_sigma': 3}
BOX, STRIDE, C = 96, 48, 2


def fused_job(net, vol, starts, batch, blend, axes, two_streams=True):
    return SI.sliding_window_inference(net, vol, starts, (BOX,) * 3, C, NORM, batch_size=batch, use_graph=True,
                                       two_streams=two_streams, blend=blend, mirror_axes=axes)


def torch_flip_job(net, vol, starts, batch, axes):
    """the sliding window of core/seg_infer.py with the mirrors done by torch.flip copies of the [P, 1, 96^3] input and the
    [P, C, 96^3] output around the plain gather and the un-mirrored Gaussian scatter"""
    from segmentation3d import _ops
    flips = SI.mirror_flip_masks(axes)
    dims = {f: [4 - b for b in range(3) if f >> b & 1] for f in flips}
    with torch.cuda.device(vol.device), torch.no_grad():
        batcher = SI.SlidingWindowBatcher(vol, starts, (BOX,) * 3, C, NORM, max_batch=batch, blend='gaussian')
        batches = [list(range(i, min(i + batch, len(starts)))) for i in range(0, len(starts), batch)]
        batcher.plan(batches)
        side = SI._job_stream(vol.device, 'side')
        cache_was_on = _ops.weight_cache(True)

        def run_batch(buf=None):
            buf = batcher.gather_current(out=buf)
            for f in flips:
                x = torch.flip(buf, dims[f]) if f else buf
                y = SI._forward_two_streams(net, x, side)
                batcher.scatter_current(torch.flip(y, dims[f]) if f else y)
            return buf
        try:
            stream = SI._job_stream(vol.device, 'warmup')
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                batcher.select(0)
                static_in = run_batch()
            torch.cuda.current_stream().wait_stream(stream)
            batcher._ctl.zero_()
            torch.cuda.synchronize()
            graph = SI._capture_in_shared_pool(lambda: run_batch(static_in), vol.device)
            for b in range(1, len(batches)):
                batcher.select(b)
                graph.replay()
            probs, mask = batcher.finalize()
        finally:
            if not cache_was_on:
                torch.cuda.synchronize()
                _ops.weight_cache(False)
    return probs, mask, batcher


def algorithmic_bytes(starts, batch, shape_zyx):
    """per launch: gather reads + writes P * box floats; scatter reads P * C * box floats and reads + writes the C + 1
    accumulator planes of the batch's bounding box (mean over the batches of the job)"""
    nv = BOX ** 3
    sel = np.array(starts)
    boxes = []
    for i in range(0, len(starts), batch):
        s = sel[i:i + batch]
        ext = s.max(0) + BOX - s.min(0)
        boxes.append(int(np.prod(ext)))
    P = batch
    return {'gather_bytes': 2 * 4 * P * nv, 'scatter_bytes_mean': int(4 * P * C * nv + 2 * 4 * (C + 1) * np.mean(boxes)),
            'batches': len(boxes), 'bounding_box_voxels_mean': float(np.mean(boxes))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--volume', default='512,512,400')
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace-jobs', action='store_true')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = vnet.SegmentationNet(1, C)
    vnet.parameters_kaiming_init(net)
    net = net.to(dev).eval()
    X, Y, Z = (int(v) for v in args.volume.split(','))
    vol = torch.randn((Z, Y, X), generator=torch.Generator().manual_seed(7)).to(dev)
    starts, _ = image_partition_by_fixed_size(((X, Y, Z), (1.0, 1.0, 1.0)), [0, 0, 0], [X, Y, Z], [BOX] * 3, [STRIDE] * 3, 16)
    info = {'volume_xyz': [X, Y, Z], 'box': BOX, 'stride': STRIDE, 'batch': args.batch, 'patches': len(starts), 'net': 'vnet(1,2)',
            'dtype': 'fp32'}
    info.update(algorithmic_bytes(starts, args.batch, (Z, Y, X)))
    if args.trace_jobs:
        for blend, axes in (('constant', ()), ('gaussian', ()), ('gaussian', ('x',))):
            for _ in range(2):                         # the first job of a variant loads code objects / fills the pool
                out = fused_job(net, vol, starts, args.batch, blend, axes, two_streams=False)
                torch.cuda.synchronize()
                del out
        print(json.dumps(info))
        return
    variants = [('constant', lambda: fused_job(net, vol, starts, args.batch, 'constant', ())),
                ('gaussian', lambda: fused_job(net, vol, starts, args.batch, 'gaussian', ()))]
    for axes in ('x', 'xy', 'xyz'):
        variants.append(('gaussian+' + axes, lambda a=axes: fused_job(net, vol, starts, args.batch, 'gaussian', tuple(a))))
        variants.append(('flip:' + axes, lambda a=axes: torch_flip_job(net, vol, starts, args.batch, tuple(a))))
    times = {name: [] for name, _ in variants}
    agree, kept = {}, None
    for rnd in range(args.repeats + 1):                # round 0 = warm-up of every variant
        for name, job in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = job()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rnd:
                times[name].append(dt)
            elif name.startswith('gaussian+'):
                kept = out[0].clone()
            elif name.startswith('flip:'):       # same result as the fused job before it (up to the forward's last bits)
                agree[name[5:]] = float((out[0] - kept).abs().max())
                del kept
            del out
        print('round {} done'.format(rnd), flush=True)
    res = dict(info)
    res['seconds'] = {k: {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'all': v}
                      for k, v in times.items()}
    plain = res['seconds']['gaussian']['median']
    res['tta_ratio'] = {a: res['seconds']['gaussian+' + a]['median'] / (2 ** len(a) * plain) for a in ('x', 'xy', 'xyz')}
    res['fused_over_torch_flip'] = {a: res['seconds']['gaussian+' + a]['median'] / res['seconds']['flip:' + a]['median']
                                    for a in ('x', 'xy', 'xyz')}
    res['max_abs_fused_minus_torch_flip'] = agree
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
