"""Deep supervision under data parallelism: two gloo ranks share the one test GPU (as tests/test_gpu_ddp.py does), each with
its own sample; the auxiliary heads' parameters are ordinary entries of the flat buffers, so their gradient-ready hooks fire
during backward, every bucket is reduced from a hook, and both ranks end every step with identical parameters."""
import datetime
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

STEPS = 2


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out):
    from conftest import PKG  # noqa: F401  (sys.path)
    from oracle import detgen
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    # a rank that never arrives ends the test after two minutes instead of gloo's default half hour
    dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.cuda.set_device(0)
    from segmentation3d.core.seg_train import TrainStep
    step = TrainStep('vnet', 1, 2, 'DiceCE', device=torch.device('cuda:0'), seed=rank, deep_supervision=2)  # different init per rank
    x = torch.from_numpy(detgen.normal(81, 'dsddp/x', (2, 1, 32, 32, 32)))
    t = torch.from_numpy(detgen.labels(82, 'dsddp/t', (2, 1, 32, 32, 32), 2)).float()
    dev = step.device
    losses, launched = [], []
    for _ in range(STEPS):
        losses.append(float(step(x[rank:rank + 1].to(dev), t[rank:rank + 1].to(dev))))
        launched.append(step.reducer.launched_in_backward)
    torch.cuda.synchronize()
    names = [k for k, _ in step.net.named_parameters()]
    torch.save({'params': [f['params'].cpu() for f in step.opt._flat if f is not None],
                'heads': {k: p.detach().cpu() for k, p in step.net.named_parameters() if k.startswith('ds_out_')},
                'names': names, 'losses': losses, 'launched': launched, 'buckets': len(step.reducer.bucket_sizes())},
               out.format(rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_deeply_supervised_steps_keep_ranks_identical(hip_device, tmp_path):
    world, port, out = 2, _free_port(), str(tmp_path / 'rank{}.pt')
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    r0 = torch.load(out.format(0), weights_only=True)
    r1 = torch.load(out.format(1), weights_only=True)
    assert r0['names'] == r1['names'] and r0['names'][-4:] == ['ds_out_64.conv.weight', 'ds_out_64.conv.bias',
                                                                'ds_out_128.conv.weight', 'ds_out_128.conv.bias']
    assert len(r0['params']) == len(r1['params']) >= 1
    for a, b in zip(r0['params'], r1['params']):                   # broadcast at start + identical reduced gradients
        assert torch.equal(a, b)
    assert sorted(r0['heads']) == sorted(r0['names'][-4:])
    for k in r0['heads']:
        assert torch.equal(r0['heads'][k], r1['heads'][k]), k
        assert bool(torch.isfinite(r0['heads'][k]).all())
    # every bucket's all-reduce was enqueued from a gradient-ready hook during backward, in every step: the heads' hooks fired
    assert r0['buckets'] >= 4
    assert r0['launched'] == [r0['buckets']] * STEPS and r1['launched'] == [r1['buckets']] * STEPS
    assert all(l == l and abs(l) < 1e3 for l in r0['losses'] + r1['losses'])
