"""GPU checks of the optimizer side of the training recipe: the fp64 sum-of-squares pass, FusedSGD against
torch.optim.SGD, global-norm clipping against torch.nn.utils.clip_grad_norm_, the device-side learning-rate schedules,
graph capture, two data-parallel ranks, and train() with the new config keys.

References are torch's optimizers in float32 on the CPU.  The 1e-6 bar on parameters is the one of
test_fused_adam_matches_torch_adam (a few float32 roundings of O(1) values over five steps); norms and learning rates
are float32 roundings of fp64 results (2^-24 = 6e-8 relative), held to relative 1e-6."""
import copy
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gpu_util import report, max_err
from oracle import detgen

pytestmark = pytest.mark.gpu

SHAPES = [(16, 1, 3, 3, 3), (16,), (33,), (5, 7), (1,)]
STEPS = 5


def _t(seed, name, shape):
    return torch.from_numpy(detgen.normal(seed, name, shape))


def _params(hip_device, seed=51):
    ps_ref = [_t(seed, 'op{}'.format(i), s).requires_grad_(True) for i, s in enumerate(SHAPES)]
    ps_dev = [torch.nn.Parameter(p.detach().clone().to(hip_device)) for p in ps_ref]
    return ps_ref, ps_dev


def _grads(step, scale=1.0):
    return [_t(60 + step, 'og{}'.format(i), s) * scale for i, s in enumerate(SHAPES)]


def _set_grads(ps_ref, ps_dev, grads, hip_device):
    for a, b, g in zip(ps_ref, ps_dev, grads):
        a.grad = g.clone()
        b.grad.copy_(g.to(hip_device))


def _norm64(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


# ---------------------------------------------------------------------------------------------------------------------
# 1. sum of squares through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
def _sumsq(g):
    from segmentation3d import _engine as E
    n = g.numel()
    nparts = E.query('seg3d_grad_sumsq_part_count', n)
    assert 1 <= nparts <= 8192
    part = torch.full((nparts + 1,), -1.0, dtype=torch.float64, device=g.device)     # one guard slot behind the last
    E.call('seg3d_grad_sumsq_partial', E.ptr(g), n, E.ptr(part), E.stream_ptr())
    torch.cuda.synchronize()
    assert float(part[nparts]) == -1.0
    return part[:nparts].cpu()


@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 256, 257, 4099, 2 ** 23 + 5])
def test_grad_sumsq_matches_float64(hip_device, n):
    """tail only, one vector, vector + tail, several workgroups, and more than one sweep of the capped grid
    (8192 workgroups x 256 threads x 4 floats = 2^23)"""
    gen = torch.Generator().manual_seed(1000 + n % 997)
    g_host = torch.randn(n, generator=gen, dtype=torch.float32)
    g = g_host.to(hip_device)
    p1, p2 = _sumsq(g), _sumsq(g)
    assert torch.equal(p1, p2)                                   # the summation order depends on n only
    want = float(np.sum(g_host.numpy().astype(np.float64) ** 2))
    got = math.fsum(p1.tolist())
    rel = abs(got - want) / want
    report('grad_sumsq_n{}'.format(n), rel=rel, slots=float(p1.numel()))
    assert rel < 1e-10, (n, got, want)


def test_grad_sumsq_does_not_overflow_float32(hip_device):
    g_host = torch.from_numpy(detgen.normal(7, 'sumsq/big', (4099,)))
    g_host[7] = 1e30                                             # its square overflows an fp32 accumulator
    g_host[4098] = -1e30                                         # and one in the scalar tail
    part = _sumsq(g_host.to(hip_device))
    got = math.fsum(part.tolist())
    want = float(np.sum(g_host.numpy().astype(np.float64) ** 2))
    assert math.isfinite(got) and abs(got - want) / want < 1e-10, (got, want)


# ---------------------------------------------------------------------------------------------------------------------
# 2. FusedSGD against torch.optim.SGD
# ---------------------------------------------------------------------------------------------------------------------
SGD_CONFIGS = [dict(momentum=0.0), dict(momentum=0.9), dict(momentum=0.99, nesterov=True, weight_decay=3e-5)]


@pytest.mark.parametrize('cfg', SGD_CONFIGS, ids=['plain', 'momentum', 'nesterov_wd'])
def test_fused_sgd_matches_torch_sgd(hip_device, cfg):
    from segmentation3d.optim.fused_sgd import FusedSGD
    ps_ref, ps_dev = _params(hip_device)
    ref = torch.optim.SGD(ps_ref, lr=1e-2, **cfg)
    opt = FusedSGD(ps_dev, lr=1e-2, **cfg)
    saved = None
    for step in range(STEPS):
        ref.zero_grad()
        opt.zero_grad()
        _set_grads(ps_ref, ps_dev, _grads(step), hip_device)
        ref.step()
        opt.step()
        if step == 1:        # after step 2: torch's state, to be continued by a fresh FusedSGD below
            saved = (copy.deepcopy(ref.state_dict()), [p.detach().clone() for p in ps_ref])
    err = max(max_err(b, a) for a, b in zip(ps_ref, ps_dev))
    report('fused_sgd_' + '_'.join('{}{}'.format(k[0], v) for k, v in cfg.items()), err=err)
    assert err < 1e-6
    sd = opt.state_dict()
    want_keys = ['momentum_buffer', 'step'] if cfg['momentum'] > 0 else ['step']
    for i in range(len(SHAPES)):
        assert sorted(sd['state'][i].keys()) == want_keys
        assert float(sd['state'][i]['step']) == STEPS
    if cfg['momentum'] > 0:
        # the buffer sums five O(1) gradients (|buf| up to ~10, ulp 1e-6): a few roundings of that size
        assert max_err(sd['state'][0]['momentum_buffer'], ref.state_dict()['state'][0]['momentum_buffer']) < 1e-5
    # a torch.optim.SGD state dict, loaded after step 2, continues to the same parameters
    ps2 = [torch.nn.Parameter(p.clone().to(hip_device)) for p in saved[1]]
    opt2 = FusedSGD(ps2, lr=1e-2, **cfg)
    opt2.load_state_dict(saved[0])
    for step in range(2, STEPS):
        opt2.zero_grad()
        for b, g in zip(ps2, _grads(step)):
            b.grad.copy_(g.to(hip_device))
        opt2.step()
    err2 = max(max_err(b, a) for a, b in zip(ps_ref, ps2))
    report('fused_sgd_resumed_from_torch', err=err2)
    assert err2 < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 3. clipping
# ---------------------------------------------------------------------------------------------------------------------
MAX_NORM = 5.0      # the unscaled gradients have a norm of ~sqrt(517) = 23: x3 is clipped, x0.01 is not


def _make(kind, ps, **kw):
    from segmentation3d.optim.fused_adam import FusedAdam
    from segmentation3d.optim.fused_sgd import FusedSGD
    if kind == 'SGD':
        return FusedSGD(ps, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=3e-5, **kw)
    return FusedAdam(ps, lr=1e-3, betas=(0.9, 0.999), **kw)


def _make_ref(kind, ps):
    if kind == 'SGD':
        return torch.optim.SGD(ps, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=3e-5)
    return torch.optim.Adam(ps, lr=1e-3, betas=(0.9, 0.999))


@pytest.mark.parametrize('kind', ['SGD', 'Adam'])
def test_clipping_matches_clip_grad_norm(hip_device, kind):
    """the gradient scale alternates so that the clip toggles: Adam divides a constant gradient scale out, so a clip
    that never toggles would pass even if it did nothing"""
    ps_ref, ps_dev = _params(hip_device)
    ref, opt = _make_ref(kind, ps_ref), _make(kind, ps_dev, max_grad_norm=MAX_NORM)
    clipped = []
    for step in range(STEPS):
        grads = _grads(step, 3.0 if (step + 1) % 2 == 1 else 0.01)          # steps count from 1: odd steps x3
        norm = _norm64(grads)
        clipped.append(norm > MAX_NORM)
        ref.zero_grad()
        opt.zero_grad()
        _set_grads(ps_ref, ps_dev, grads, hip_device)
        torch.nn.utils.clip_grad_norm_(ps_ref, MAX_NORM)
        ref.step()
        opt.step()
        got = float(opt.last_grad_norm)
        assert abs(got - norm) / norm < 1e-6, (step, got, norm)
        coef = float(opt.last_clip_coef)
        assert (coef < 1.0) == clipped[-1] and abs(coef - min(1.0, MAX_NORM / (norm + 1e-6))) < 1e-6
    assert clipped == [True, False, True, False, True]
    err = max(max_err(b, a) for a, b in zip(ps_ref, ps_dev))
    report('clip_' + kind, err=err)
    assert err < 1e-6
    if kind == 'Adam':
        sd, rsd = opt.state_dict(), ref.state_dict()
        assert sorted(sd['state'][0].keys()) == ['exp_avg', 'exp_avg_sq', 'step']
        err_m = max(max_err(sd['state'][i]['exp_avg'], rsd['state'][i]['exp_avg']) for i in range(len(SHAPES)))
        report('clip_Adam_exp_avg', err=err_m)
        assert err_m < 1e-6


@pytest.mark.parametrize('kind', ['SGD', 'Adam'])
def test_inert_clip_is_bit_equal_to_no_clip(hip_device, kind):
    runs = []
    for kw in (dict(max_grad_norm=1e9), dict()):
        _, ps_dev = _params(hip_device)
        opt = _make(kind, ps_dev, **kw)
        for step in range(STEPS):
            opt.zero_grad()
            for b, g in zip(ps_dev, _grads(step, 3.0 if step % 2 == 0 else 0.01)):
                b.grad.copy_(g.to(hip_device))
            opt.step()
        runs.append(opt._flat[0]['params'].cpu())
        if kw:
            assert float(opt.last_clip_coef) == 1.0 and float(opt.last_grad_norm) > 0.0
    assert torch.equal(runs[0], runs[1])


# ---------------------------------------------------------------------------------------------------------------------
# 4. schedules
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,steps', [('poly', 10), ('cosine', 8)])
def test_schedule_on_device_matches_lr_at(hip_device, name, steps):
    from segmentation3d.optim.fused_sgd import FusedSGD
    from segmentation3d.optim.lr_schedule import lr_at
    sched = {'name': name, 'total_steps': 8, 'warmup_steps': 2, 'power': 0.9}
    ps_ref, ps_dev = _params(hip_device)
    ref = torch.optim.SGD(ps_ref, lr=1e-2, momentum=0.9)
    opt = FusedSGD(ps_dev, lr=1e-2, momentum=0.9, lr_schedule=sched)
    saved = None
    for t in range(1, steps + 1):
        want = lr_at(t, 1e-2, **sched)
        for g in ref.param_groups:
            g['lr'] = want
        before = opt._flat[0]['params'].clone()
        ref.zero_grad()
        opt.zero_grad()
        _set_grads(ps_ref, ps_dev, _grads(t), hip_device)
        ref.step()
        opt.step()
        got = float(opt.last_lr)
        assert abs(got - want) <= 1e-6 * want, (t, got, want)          # want == 0 asks for an exact 0
        assert opt.param_groups[0]['lr'] == want and opt.param_groups[0]['initial_lr'] == 1e-2
        if name == 'poly' and t > 8:
            assert want == 0.0 and torch.equal(before, opt._flat[0]['params'])     # lr == 0: parameters bit-unchanged
        else:
            assert want > 0.0 and not torch.equal(before, opt._flat[0]['params'])
        if t == 4:
            saved = copy.deepcopy(opt.state_dict())
    err = max(max_err(b, a) for a, b in zip(ps_ref, ps_dev))
    report('schedule_' + name, err=err)
    assert err < 1e-6
    # a fresh optimizer that loads the state of step 4 continues the schedule with step 5
    _, ps2 = _params(hip_device)
    opt2 = FusedSGD(ps2, lr=1e-2, momentum=0.9, lr_schedule=sched)
    opt2.load_state_dict(saved)
    assert opt2.param_groups[0]['lr'] == lr_at(4, 1e-2, **sched)
    opt2.zero_grad()
    opt2.step()
    want5 = lr_at(5, 1e-2, **sched)
    assert abs(float(opt2.last_lr) - want5) <= 1e-6 * want5 and opt2.param_groups[0]['lr'] == want5
    assert int(opt2._flat[0]['step_dev'].item()) == 5 and float(opt2.state_dict()['state'][0]['step']) == 5


# ---------------------------------------------------------------------------------------------------------------------
# 5. graph capture against eager
# ---------------------------------------------------------------------------------------------------------------------
# The gradient is linear in the two weights of the compound loss.  With unit weights the global gradient norm of
# vnet(1, 2) on these inputs is below 1 on every step (0.60 on the first, measured on an MI355X and equal to the float64
# norm of the flat buffer), so a clip at 1.0 would never bite; with both weights at 4 the first step's norm is 2.4.
GRAPH_LOSS_OPTIONS = {'dice_weight': 4.0, 'ce_weight': 4.0}


@pytest.mark.parametrize('optimizer,options', [
    ('SGD', {'max_grad_norm': 1.0, 'lr_schedule': {'name': 'poly', 'total_steps': 8}, 'momentum': 0.99, 'nesterov': True}),
    ('Adam', {'max_grad_norm': 1.0})], ids=['SGD', 'Adam'])
def test_graph_captured_step_with_control_block_equals_eager(hip_device, optimizer, options):
    """TrainStep(use_graph=True) with the control-block optimizers walks the eager loss curve, counts its steps on the
    device and follows the schedule; the clip at 1.0 has to be active on at least one step, and the norm the device
    reports is the float64 norm of the flat gradient buffer"""
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import TrainStep
    from segmentation3d.optim.lr_schedule import lr_at
    curves, coefs, norms = {}, {}, {}
    for use_graph in (False, True):
        step = TrainStep('vnet', 1, 2, 'DiceCE', [0.5, 0.5], lr=1e-3, device=hip_device, seed=3, use_graph=use_graph,
                         loss_options=GRAPH_LOSS_OPTIONS, optimizer=optimizer, optim_options=options)
        losses, cs, ns = [], [], []
        for i in range(6):
            x = torch.from_numpy(detgen.normal(90 + i % 2, 'gs/x', (2, 1, 32, 32, 32))).to(hip_device)
            t = torch.from_numpy(detgen.labels(95 + i % 2, 'gs/t', (2, 1, 32, 32, 32), 2)).to(hip_device)
            losses.append(float(step(x, t)))
            cs.append(float(step.opt.last_clip_coef))
            ns.append(float(step.opt.last_grad_norm))
            # the gradients of the step are still in the flat buffer: the norm the device measured is theirs
            want = math.sqrt(float((step.opt._flat[0]['grads'].double() ** 2).sum()))
            assert abs(ns[-1] - want) <= 1e-6 * want, (i, ns[-1], want)
        curves[use_graph], coefs[use_graph], norms[use_graph] = losses, cs, ns
        assert (step._graph is not None) == use_graph
        assert [int(f['step']) for f in step.opt._flat if f is not None] == [6]
        assert int(step.opt._flat[0]['step_dev'].item()) == 6
        if optimizer == 'SGD':
            assert step.opt.param_groups[0]['lr'] == lr_at(6, 1e-3, 'poly', total_steps=8)
            assert abs(float(step.opt.last_lr) - lr_at(6, 1e-3, 'poly', total_steps=8)) < 1e-9
        else:
            assert step.opt.param_groups[0]['lr'] == 1e-3
    _ops.PACK_CACHE.clear()
    report('graph_step_ctl_' + optimizer, **{'eager_{}'.format(i): v for i, v in enumerate(curves[False])},
           **{'graph_{}'.format(i): v for i, v in enumerate(curves[True])},
           **{'coef_{}'.format(i): v for i, v in enumerate(coefs[True])},
           **{'norm_{}'.format(i): v for i, v in enumerate(norms[True])})
    assert curves[False] == curves[True], curves
    assert coefs[False] == coefs[True], coefs
    assert min(coefs[True]) < 1.0, coefs            # the clip at 1.0 is active on these inputs


# ---------------------------------------------------------------------------------------------------------------------
# 6. two data-parallel ranks (gloo) on the one GPU
# ---------------------------------------------------------------------------------------------------------------------
DDP_MAX_NORM = 0.05


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out):
    from conftest import PKG  # noqa: F401  (sys.path)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from segmentation3d.core.seg_train import TrainStep
    step = TrainStep('vnet', 1, 2, 'Dice', [0.5, 0.5], lr=1e-2, device=torch.device('cuda:0'), seed=rank,
                     optimizer='SGD', optim_options={'max_grad_norm': DDP_MAX_NORM, 'momentum': 0.99, 'nesterov': True})
    x = torch.from_numpy(detgen.normal(81, 'ddp/x', (2, 1, 32, 32, 32)))
    t = torch.from_numpy(detgen.labels(82, 'ddp/t', (2, 1, 32, 32, 32), 2))
    dev = step.device
    step(x[rank:rank + 1].to(dev), t[rank:rank + 1].to(dev))
    torch.cuda.synchronize()
    flat = step.opt._flat[0]
    torch.save({'grads': flat['grads'].cpu(), 'params': flat['params'].cpu(), 'norm': step.opt.last_grad_norm.cpu(),
                'coef': step.opt.last_clip_coef.cpu()}, out.format(rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_clipped_sgd_step(hip_device, tmp_path):
    world, port, out = 2, _free_port(), str(tmp_path / 'rank{}.pt')
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    r0 = torch.load(out.format(0), weights_only=True)
    r1 = torch.load(out.format(1), weights_only=True)
    assert torch.equal(r0['params'], r1['params'])
    assert torch.equal(r0['norm'], r1['norm']) and torch.equal(r0['coef'], r1['coef'])
    for r in (r0, r1):
        want = math.sqrt(float((r['grads'].double() ** 2).sum())) / 2.0     # the buffer holds the SUM over the ranks
        got = float(r['norm'])
        report('ddp_clip_norm', norm=got, want=want, coef=float(r['coef']))
        assert abs(got - want) / want < 1e-6, (got, want)
        assert float(r['coef']) < 1.0                                       # the clip is active
        assert abs(float(r['coef']) - DDP_MAX_NORM / (want + 1e-6)) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 7. train() with the new config keys
# ---------------------------------------------------------------------------------------------------------------------
_CFG = '''
from easydict import EasyDict as edict
from segmentation3d.utils.normalizer import AdaptiveNormalizer
__C = edict()
cfg = __C
__C.general = {}
__C.general.imseg_list = ''
__C.general.save_dir = '%(save_dir)s'
__C.general.model_scale = 'coarse'
__C.general.resume_epoch = %(resume)d
__C.general.num_gpus = 1
__C.general.seed = 0
__C.dataset = {}
__C.dataset.num_classes = 2
__C.dataset.num_samples = 2
__C.dataset.spacing = [1.0, 1.0, 1.0]
__C.dataset.crop_size = [32, 32, 32]
__C.dataset.interpolation = 'LINEAR'
__C.dataset.crop_normalizers = [AdaptiveNormalizer()]
__C.loss = {}
__C.loss.name = 'DiceCE'
__C.loss.obj_weight = [0.5, 0.5]
__C.loss.focal_gamma = 2
__C.net = {}
__C.net.name = 'vnet'
__C.train = {}
__C.train.epochs = 8
__C.train.batchsize = 2
__C.train.num_threads = 0
__C.train.lr = 1e-2
__C.train.betas = (0.9, 0.999)
__C.train.save_epochs = 2
__C.train.optimizer = 'SGD'
__C.train.momentum = 0.99
__C.train.nesterov = True
__C.train.weight_decay = 3e-5
__C.train.clip_grad_norm = 12
__C.train.lr_schedule = 'poly'
__C.train.lr_power = 0.9
'''


def _batches(n):
    def factory(cfg):
        for i in range(n):
            yield (torch.from_numpy(detgen.normal(90 + i % 2, 'gs/x', (2, 1, 32, 32, 32))),
                   torch.from_numpy(detgen.labels(95 + i % 2, 'gs/t', (2, 1, 32, 32, 32), 2)))
    return factory


def _logged_lrs(path):
    return [float(l.split('lr: ')[1]) for l in open(path).read().splitlines() if 'train_loss' in l]


def test_train_with_sgd_poly_config_and_resume(hip_device, tmp_path):
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import train
    from segmentation3d.optim.fused_sgd import FusedSGD
    from segmentation3d.optim.lr_schedule import lr_at
    sched = dict(name='poly', total_steps=8, power=0.9)        # total_steps: ceil(epochs * num_samples / batchsize)
    save_dir = str(tmp_path / 'model')
    log = os.path.join(save_dir, 'coarse', 'train_log.txt')
    try:
        first = tmp_path / 'optim_cfg_first.py'
        first.write_text(_CFG % dict(save_dir=save_dir, resume=-1))
        step = train(str(first), data_iter_factory=_batches(4))
        assert isinstance(step.opt, FusedSGD) and step.opt.max_grad_norm == 12.0
        assert step.opt.lr_schedule == {'name': 'poly', 'total_steps': 8, 'warmup_steps': 0, 'power': 0.9}
        assert step.opt._flat[0]['step'] == 4 and int(step.opt._flat[0]['step_dev'].item()) == 4
        assert _logged_lrs(log) == [float('{:.6e}'.format(lr_at(t, 1e-2, **sched))) for t in (1, 2, 3, 4)]
        # epoch 2 is reached after three steps (one two-sample batch per epoch): the checkpoint holds step 3
        sd = torch.load(os.path.join(save_dir, 'coarse', 'checkpoints', 'chk_2', 'optimizer.pth'), map_location='cpu',
                        weights_only=True)
        assert sorted(sd['state'][0].keys()) == ['momentum_buffer', 'step'] and float(sd['state'][0]['step']) == 3
        assert sd['param_groups'][0]['lr'] == lr_at(3, 1e-2, **sched) and sd['param_groups'][0]['initial_lr'] == 1e-2
        second = tmp_path / 'optim_cfg_resume.py'
        second.write_text(_CFG % dict(save_dir=save_dir, resume=2))
        step = train(str(second), data_iter_factory=_batches(2))
        assert step.opt._flat[0]['step'] == 5 and int(step.opt._flat[0]['step_dev'].item()) == 5
        assert step.opt.param_groups[0]['lr'] == lr_at(5, 1e-2, **sched)
        assert abs(float(step.opt.last_lr) - lr_at(5, 1e-2, **sched)) <= 1e-6 * lr_at(5, 1e-2, **sched)
        assert _logged_lrs(log)[4:] == [float('{:.6e}'.format(lr_at(t, 1e-2, **sched))) for t in (4, 5)]
    finally:
        _ops.set_activation_dtype('fp32')
        _ops.PACK_CACHE.clear()


# ---------------------------------------------------------------------------------------------------------------------
# 8. the device-resident step count: prepare -> update, against the host-argument step seg3d_adam_step
# ---------------------------------------------------------------------------------------------------------------------
ADAM_LR, ADAM_EPS = 1e-3, 1e-8
ADAM_KW = dict(lr=ADAM_LR, betas=(0.9, 0.999), weight_decay=0.01)


def _prepare_constant(step_dev, ctl, grad_scale, lr, beta1, beta2):
    """seg3d_optim_prepare with no clipping (max_norm 0, no slots) and the constant schedule"""
    from segmentation3d import _engine as E
    E.call('seg3d_optim_prepare', E.ptr(step_dev), E.ptr(ctl), None, 0, grad_scale, 0.0, 0, lr, 1, 0, 0.9, beta1, beta2,
           E.stream_ptr())


def _step_with_grads(opt, ps, t, hip_device):
    opt.zero_grad()
    for b, g in zip(ps, _grads(t)):
        b.grad.copy_(g.to(hip_device))
    opt.step()


def test_device_step_adam_equals_host_step_adam(hip_device):
    """the default FusedAdam (host-side scalars) against one that counts its steps on the device, stepped eagerly:
    parameters, both moments and the counters are bit-equal after every step"""
    from segmentation3d.optim.fused_adam import FusedAdam
    _, ps_a = _params(hip_device)
    _, ps_b = _params(hip_device)
    a, b = FusedAdam(ps_a, **ADAM_KW), FusedAdam(ps_b, **ADAM_KW)
    a.grad_scale = b.grad_scale = 0.5
    b.use_device_step()
    fa, fb = a._flat[0], b._flat[0]
    for t in range(1, 9):
        _step_with_grads(a, ps_a, t, hip_device)
        _step_with_grads(b, ps_b, t, hip_device)
        for k in ('params', 'exp_avg', 'exp_avg_sq'):
            assert torch.equal(fa[k], fb[k]), (t, k)
        assert fa['step'] == fb['step'] == t and int(fb['step_dev'].item()) == t
        assert all(float(a.state[x]['step']) == float(b.state[y]['step']) == t for x, y in zip(ps_a, ps_b))
    assert float(fa['exp_avg'].abs().max()) > 0.0


def _adam_float64(p, g, m, v, t, lr, beta1, beta2, eps, wd, grad_scale):
    """torch.optim.Adam's single-tensor rule in float64, on the float32-rounded hyper-parameters the kernels receive"""
    lr, beta1, beta2, eps, wd = (float(np.float32(x)) for x in (lr, beta1, beta2, eps, wd))
    gg = g * grad_scale + wd * p
    m = m + (gg - m) * (1.0 - beta1)
    v = v * beta2 + (1.0 - beta2) * gg * gg
    p = p - (lr / (1.0 - beta1 ** t)) * (m / (np.sqrt(v) / math.sqrt(1.0 - beta2 ** t) + eps))
    return p, m, v


@pytest.mark.parametrize('n', [1, 3, 4, 5, 255, 256, 257, 4099])
def test_adam_entries_tail_and_alignment(hip_device, n):
    """the sizes at which the float4 body and the scalar tail meet.  prepare -> seg3d_adam_step_ctl is bit-equal to
    seg3d_adam_step with the same scalars, and both follow the float64 rule: the reference is evaluated on the same
    float32 hyper-parameters, so what is left is the kernel's own roundings -- under ten per element and step, each
    2^-24 = 6e-8 of a value no larger than the buffer's maximum, over three steps: held to 1e-6 of the buffer's maximum.
    Four guard floats behind every buffer stay untouched."""
    from segmentation3d import _engine as E
    beta1, beta2, wd, scale = 0.9, 0.999, 0.01, 0.25
    host = {k: detgen.normal(300 + n % 97, 'tail/' + k, (n,)) for k in ('p', 'g1', 'g2', 'g3')}

    def buf(values):
        t = torch.full((n + 4,), 7.0, dtype=torch.float32)
        t[:n] = torch.from_numpy(values)
        return t.to(hip_device)

    zeros = np.zeros(n, dtype=np.float32)
    A = {k: buf(x) for k, x in (('p', host['p']), ('m', zeros), ('v', zeros))}
    B = {k: t.clone() for k, t in A.items()}
    step_dev = torch.zeros(1, dtype=torch.int32, device=hip_device)
    ctl = torch.zeros(8, dtype=torch.float32, device=hip_device)
    p64, m64, v64 = host['p'].astype(np.float64), zeros.astype(np.float64), zeros.astype(np.float64)
    for t in (1, 2, 3):
        g = buf(host['g{}'.format(t)])
        _prepare_constant(step_dev, ctl, scale, ADAM_LR, beta1, beta2)
        E.call('seg3d_adam_step_ctl', E.ptr(A['p']), E.ptr(g), E.ptr(A['m']), E.ptr(A['v']), n, E.ptr(ctl), beta1, beta2,
               ADAM_EPS, wd, E.stream_ptr())
        E.call('seg3d_adam_step', E.ptr(B['p']), E.ptr(g), E.ptr(B['m']), E.ptr(B['v']), n, t, ADAM_LR, beta1, beta2,
               ADAM_EPS, wd, scale, E.stream_ptr())
        p64, m64, v64 = _adam_float64(p64, host['g{}'.format(t)].astype(np.float64), m64, v64, t, ADAM_LR, beta1, beta2,
                                      ADAM_EPS, wd, scale)
        assert int(step_dev.item()) == t
        for k, want in (('p', p64), ('m', m64), ('v', v64)):
            assert torch.equal(A[k], B[k]), (n, t, k)
            assert torch.equal(A[k][n:].cpu(), torch.full((4,), 7.0)), (n, t, k)
            rel = float(np.abs(A[k][:n].cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
            report('adam_tail_n{}_t{}_{}'.format(n, t, k), rel=rel)
            assert rel < 1e-6, (n, t, k, rel)


def test_adam_entries_tail_and_alignment_refusal(hip_device):
    """a pointer 4 bytes past a 16-byte boundary is SEG3D_ERR_INVALID (ValueError) at every entry, with its message"""
    from segmentation3d import _engine as E
    n = 64
    p, g, m, v = (torch.zeros(n + 4, dtype=torch.float32, device=hip_device) for _ in range(4))
    ctl = torch.zeros(8, dtype=torch.float32, device=hip_device)
    part = torch.zeros(4, dtype=torch.float64, device=hip_device)
    s = E.stream_ptr()

    def entries(bufs):
        a, b, c, d = (E.ptr(x) for x in bufs)
        return {
            'seg3d_adam_step': (a, b, c, d, n, 1, ADAM_LR, 0.9, 0.999, ADAM_EPS, 0.0, 1.0, s),
            'seg3d_adam_step_ctl': (a, b, c, d, n, E.ptr(ctl), 0.9, 0.999, ADAM_EPS, 0.0, s),
            'seg3d_sgd_step_ctl': (a, b, c, n, E.ptr(ctl), 0.9, 0.0, 0, s),
        }

    for i in range(4):
        bufs = [p, g, m, v]
        bufs[i] = bufs[i][1:]
        for name, args in entries(bufs).items():
            if name == 'seg3d_sgd_step_ctl' and i == 3:
                continue                                          # SGD has three buffers
            with pytest.raises(ValueError) as err:
                E.call(name, *args)
            assert str(err.value) == name + ': buffers must be 16-byte aligned', (name, i)
    with pytest.raises(ValueError) as err:
        E.call('seg3d_grad_sumsq_partial', E.ptr(g[1:]), n, E.ptr(part), s)
    assert str(err.value) == 'seg3d_grad_sumsq_partial: grads must be 16-byte aligned, part 8-byte aligned'
    torch.cuda.synchronize()
    assert all(float(x.abs().max()) == 0.0 for x in (p, g, m, v))     # a refused call launches nothing


@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.5, 0.9), (0.0, 0.99)])
def test_prepare_bias_corrections_equal_host_pow(hip_device, betas):
    """seg3d_adam_step takes 1 - beta1^t and sqrt(1 - beta2^t) from the host's pow, seg3d_optim_prepare from the
    device's: for t = 1 .. 4096 the two float32 values are the same bits, so a run that moves its step count to the
    device part-way (TrainStep captures after two eager steps) continues the curve it would have walked on the host"""
    beta1, beta2 = (float(np.float32(b)) for b in betas)           # the entries take float arguments
    T = 4096
    step_dev = torch.zeros(1, dtype=torch.int32, device=hip_device)
    ctl = torch.zeros(8, dtype=torch.float32, device=hip_device)
    rows = torch.zeros((T, 8), dtype=torch.float32, device=hip_device)
    for t in range(1, T + 1):
        _prepare_constant(step_dev, ctl, 1.0, ADAM_LR, beta1, beta2)
        rows[t - 1].copy_(ctl)
    got = rows.cpu().numpy()
    assert int(step_dev.item()) == T
    want1 = np.array([np.float32(1.0 - math.pow(beta1, t)) for t in range(1, T + 1)], dtype=np.float32)
    want2 = np.array([np.float32(math.sqrt(1.0 - math.pow(beta2, t))) for t in range(1, T + 1)], dtype=np.float32)
    for name, g, w in (('bc1', got[:, 2].copy(), want1), ('bc2_sqrt', got[:, 3].copy(), want2)):
        off = np.nonzero(g.view(np.uint32) != w.view(np.uint32))[0]
        report('prepare_{}_b{}_{}'.format(name, betas[0], betas[1]), mismatches=float(off.size))
        assert off.size == 0, (name, betas, [(int(i) + 1, float(g[i]), float(w[i])) for i in off[:8]])
    assert np.array_equal(got[:, 0], np.full(T, np.float32(ADAM_LR))) and np.array_equal(got[:, 1], np.ones(T, np.float32))


@pytest.mark.parametrize('on_device', [True, False], ids=['device_count', 'host_count'])
def test_capture_failure_rewinds_both_counters(hip_device, on_device):
    """what TrainStep does around a graph capture, around an eager step instead: the counters saved before the step
    are back after restore_step_counts(), and the optimizer goes on exactly like a fresh one loaded from its state"""
    from segmentation3d.optim.fused_adam import FusedAdam

    def make(ps):
        opt = FusedAdam(ps, **ADAM_KW)
        if on_device:
            opt.use_device_step()
        return opt

    def counts(opt):
        f = opt._flat[0]
        steps = {float(opt.state[q]['step']) for q in f['list']}
        return (f['step'], int(f['step_dev'].item()) if on_device else None, steps)

    _, ps_dev = _params(hip_device)
    opt = make(ps_dev)
    for t in (1, 2, 3):
        _step_with_grads(opt, ps_dev, t, hip_device)
    saved = opt.step_counts()
    assert saved == [3]
    _step_with_grads(opt, ps_dev, 4, hip_device)
    assert counts(opt) == (4, 4 if on_device else None, {4.0})
    opt.restore_step_counts(saved)
    assert counts(opt) == (3, 3 if on_device else None, {3.0})
    ps2 = [torch.nn.Parameter(q.detach().clone()) for q in ps_dev]
    opt2 = make(ps2)
    opt2.load_state_dict(copy.deepcopy(opt.state_dict()))
    _step_with_grads(opt, ps_dev, 5, hip_device)
    _step_with_grads(opt2, ps2, 5, hip_device)
    assert counts(opt) == counts(opt2) == (4, 4 if on_device else None, {4.0})
    for k in ('params', 'exp_avg', 'exp_avg_sq'):
        assert torch.equal(opt._flat[0][k], opt2._flat[0][k]), k
