"""The validation pass under data parallelism, in the pattern of tests/test_gpu_ddp.py: two ranks share the one test GPU (gloo
backend), rank r scores crops r::2, the counts and loss sums are all-reduced -- both ranks return the same dict, and the reduced
counts equal those of one process over the whole crop set bit for bit."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

V, BATCH, NCLS = 3, 1, 3      # three crops, rank 0 takes two and rank 1 one; one crop per forward in every process, so that
                              # each crop meets the same kernels and plans wherever it is scored


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _validator(dev):
    from oracle import detgen
    from segmentation3d.core.seg_train import build_loss
    from segmentation3d.core.seg_validate import Validator
    from segmentation3d.network import vnet
    torch.manual_seed(11)
    net = vnet.SegmentationNet(1, NCLS)
    vnet.parameters_kaiming_init(net)
    net = net.to(dev)
    crops = torch.from_numpy(detgen.normal(911, 'valddp/x', (V, 1, 32, 32, 32))).to(dev)
    masks = torch.from_numpy(detgen.labels(912, 'valddp/t', (V, 1, 32, 32, 32), NCLS)).to(dev)
    return Validator(net, build_loss('DiceCE', NCLS), crops, masks, BATCH, ema=0.5)


def _worker(rank, world, port, out):
    from conftest import PKG  # noqa: F401  (sys.path)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    v = _validator(torch.device('cuda:0'))
    result = v.run(1)
    torch.cuda.synchronize()
    torch.save({'result': result, 'counts': v.counts.cpu(), 'mine': int(v.crops.shape[0]), 'state': v.state_dict()},
               out.format(rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_validation_equals_one_process(hip_device, tmp_path):
    world, port, out = 2, _free_port(), str(tmp_path / 'rank{}.pt')
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    r0 = torch.load(out.format(0), weights_only=True)
    r1 = torch.load(out.format(1), weights_only=True)
    assert (r0['mine'], r1['mine']) == (2, 1)
    assert r0['result'] == r1['result'] and r0['state'] == r1['state']      # every rank returns identical numbers
    assert torch.equal(r0['counts'], r1['counts'])
    single = _validator(hip_device)
    ref = single.run(1)
    assert torch.equal(r0['counts'], single.counts.cpu())                    # integer sums: bit for bit
    assert int(r0['counts'][:, [0, 2]].sum()) == V * 32 ** 3                 # every voxel is some class's tp or fn
    assert r0['result']['dice'] == ref['dice'] and r0['result']['mean_dice'] == ref['mean_dice']
    assert r0['result']['ema_dice'] == ref['ema_dice'] and r0['result']['improved'] is True
    # the same three per-crop losses (fp32) summed in doubles in another order: (l0 + l2) + l1 against (l0 + l1) + l2
    assert abs(r0['result']['val_loss'] - ref['val_loss']) < 1e-12
