"""Two ranks share the one test GPU (gloo): the sharded sliding window with Gaussian blending and mirror TTA against the
single-process run.  acc and count are still plain sums, so SlabShardPlan / merge_slabs need nothing new; only the order
in which the halo sums are added differs between the two runs."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

_BOX, _STRIDE, _SHAPE, _C = (32, 32, 32), 16, (96, 64, 64), 2
_AXES = ('x', 'z')
_NORM = {'type': 1, 'clip_sigma': 3.0}


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _setup():
    from segmentation3d.utils.image_tools import image_partition_by_fixed_size
    Z, Y, X = _SHAPE
    rng = np.random.RandomState(71)
    vol = (rng.randn(Z, Y, X) * 200 - 100).astype(np.float32)
    starts, _ = image_partition_by_fixed_size(((X, Y, Z), (1.0, 1.0, 1.0)), [0, 0, 0], [X, Y, Z], [32] * 3, [16] * 3, 16)
    return vol, starts


def _net(device):
    from segmentation3d.network import vnet
    torch.manual_seed(5)
    net = vnet.SegmentationNet(1, _C)
    vnet.parameters_kaiming_init(net)
    return net.to(device).eval()


def _worker(rank, world, port, out):
    from conftest import PKG  # noqa: F401  (sys.path)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from segmentation3d.core.seg_infer import sliding_window_inference
    net = _net('cuda:0')
    vol, starts = _setup()
    probs, mask, batcher = sliding_window_inference(net, torch.from_numpy(vol).cuda(), starts, _BOX, _C, _NORM, batch_size=4,
                                                    shard=True, gather='none', blend='gaussian', mirror_axes=_AXES)
    torch.cuda.synchronize()
    torch.save({'probs': probs.cpu(), 'mask': mask.cpu(), 'owned': list(batcher.shard_plan.owned(rank)),
                'mine': len(batcher.shard_plan.patches[rank])}, out.format(rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharded_gaussian_mirror_matches_single_rank(hip_device, tmp_path):
    from segmentation3d.core.seg_infer import mirror_flip_masks, sliding_window_inference
    world, port, out = 2, _free_port(), str(tmp_path / 'bt{}.pt')
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    vol, starts = _setup()
    probs, _, _ = sliding_window_inference(_net(hip_device), torch.from_numpy(vol).to(hip_device), starts, _BOX, _C, _NORM,
                                           batch_size=4, blend='gaussian', mirror_axes=_AXES)
    probs = probs.cpu()
    # tolerance: a probability is a ratio of two sums of n terms each; the two runs add the same terms in another order,
    # n_max = (largest overlap count) x (flips) terms at the most, each addition rounding by at most 2^-24 relative
    hits = np.zeros(_SHAPE, np.int32)
    for s in starts:
        hits[s[2]:s[2] + 32, s[1]:s[1] + 32, s[0]:s[0] + 32] += 1
    n_max = int(hits.max()) * len(mirror_flip_masks(_AXES))
    assert hits.max() == 8 and n_max == 32
    tol = n_max * 2.0 ** -23
    r = [torch.load(out.format(k), weights_only=True) for k in range(world)]
    assert r[0]['mine'] + r[1]['mine'] == len(starts)
    assert r[0]['owned'][0] == 0 and r[0]['owned'][1] == r[1]['owned'][0] and r[1]['owned'][1] == _SHAPE[0]
    for k in range(world):
        z0, z1 = r[k]['owned']
        assert z1 > z0
        err = float((r[k]['probs'][:, z0:z1] - probs[:, z0:z1]).abs().max())
        print('rank {} slab [{}, {}): max |sharded - single| = {} (tolerance {})'.format(k, z0, z1, err, tol))
        assert err <= tol
        # every voxel of the owned slab: the mask is the arg-max of the rank's own probabilities
        assert torch.equal(r[k]['mask'][z0:z1], r[k]['probs'][:, z0:z1].argmax(0).to(torch.int8))
