"""Host-side checks of the optimizer options (no GPU): the learning-rate rule `lr_at` against closed forms and against
torch's schedulers, the config helper's defaults, and the argument validation of FusedSGD / FusedAdam."""
import math
import types

import pytest
import torch

from conftest import PKG  # noqa: F401  (sys.path)

BASE = 1e-2


def _lr_at(*args, **kw):
    from segmentation3d.optim.lr_schedule import lr_at
    return lr_at(*args, **kw)


def test_lr_at_closed_forms():
    # steps count from 1; step t has s = t - 1 completed steps behind it
    assert _lr_at(1, BASE) == BASE and _lr_at(1000, BASE, 'constant', total_steps=3) == BASE
    assert _lr_at(1, BASE, 'poly', total_steps=10, power=0.9) == BASE
    assert _lr_at(6, BASE, 'poly', total_steps=10, power=2.0) == pytest.approx(BASE * 0.25, rel=1e-15)
    assert _lr_at(6, BASE, 'poly', total_steps=10, power=0.9) == pytest.approx(BASE * 0.5 ** 0.9, rel=1e-15)
    assert _lr_at(1, BASE, 'cosine', total_steps=10) == BASE
    assert _lr_at(6, BASE, 'cosine', total_steps=10) == pytest.approx(BASE * 0.5, rel=1e-15)
    assert _lr_at(11, BASE, 'cosine', total_steps=10) == pytest.approx(0.0, abs=1e-18)
    assert _lr_at(500, BASE, 'cosine', total_steps=10) == _lr_at(11, BASE, 'cosine', total_steps=10)   # min(s, T)
    with pytest.raises(ValueError):
        _lr_at(0, BASE)
    with pytest.raises(ValueError):
        _lr_at(1, BASE, 'linear')


def test_lr_at_poly_is_zero_at_and_past_total_steps():
    T = 8
    for power in (0.9, 1.0, 2.0):
        assert _lr_at(T, BASE, 'poly', total_steps=T, power=power) > 0.0          # s = T - 1: the last live step
        for t in (T + 1, T + 2, T + 100):                                          # s >= T
            assert _lr_at(t, BASE, 'poly', total_steps=T, power=power) == 0.0
        assert _lr_at(T + 1, BASE, 'poly', total_steps=T, warmup_steps=3, power=power) == 0.0


def test_lr_at_warmup_ramp():
    W = 4
    for t in range(1, 12):
        want = BASE * min(1.0, t / float(W))
        assert _lr_at(t, BASE, 'constant', warmup_steps=W) == pytest.approx(want, rel=1e-15)
    assert _lr_at(1, BASE, 'constant', warmup_steps=1) == BASE
    # the ramp multiplies the decay
    got = _lr_at(2, BASE, 'poly', total_steps=8, warmup_steps=4, power=0.9)
    assert got == pytest.approx(BASE * 0.5 * (1 - 1 / 8.0) ** 0.9, rel=1e-15)


def _torch_lrs(make_scheduler, steps):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE)
    sched = make_scheduler(opt)
    out = []
    for _ in range(steps):
        out.append(opt.param_groups[0]['lr'])      # the rate the coming opt.step() uses
        opt.step()
        sched.step()
    return out


@pytest.mark.parametrize('power', [0.9, 1.0, 2.0])
def test_lr_at_matches_torch_polynomial_lr(power):
    T = 12
    ref = _torch_lrs(lambda o: torch.optim.lr_scheduler.PolynomialLR(o, total_iters=T, power=power), T + 3)
    for t, want in enumerate(ref, start=1):
        got = _lr_at(t, BASE, 'poly', total_steps=T, power=power)
        assert got == pytest.approx(want, rel=1e-12, abs=0.0), (t, got, want)      # exact zeros at and past T


@pytest.mark.parametrize('name,warmup', [('cosine', 0), ('cosine', 3), ('poly', 3), ('constant', 5)])
def test_lr_at_matches_torch_lambda_lr(name, warmup):
    T, power = 10, 0.9

    def factor(s):       # LambdaLR hands over the number of completed steps
        w = min(1.0, (s + 1.0) / warmup) if warmup else 1.0
        if name == 'poly':
            return w * max(0.0, 1.0 - s / float(T)) ** power
        if name == 'cosine':
            return w * 0.5 * (1.0 + math.cos(math.pi * min(s, T) / float(T)))
        return w

    ref = _torch_lrs(lambda o: torch.optim.lr_scheduler.LambdaLR(o, factor), T + 3)
    for t, want in enumerate(ref, start=1):
        got = _lr_at(t, BASE, name, total_steps=T, warmup_steps=warmup, power=power)
        assert got == pytest.approx(want, rel=1e-12, abs=0.0), (t, got, want)


def test_lr_at_cosine_matches_torch_cosine_annealing():
    T = 9
    ref = _torch_lrs(lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=T), T + 1)
    for t, want in enumerate(ref, start=1):
        # CosineAnnealingLR steps recursively: its own rounding grows with the step count, hence the absolute bar
        assert abs(_lr_at(t, BASE, 'cosine', total_steps=T) - want) <= 1e-12 * BASE, t


def test_optim_options_from_config_defaults_reproduce_todays_run():
    from segmentation3d.core.seg_train import optim_options_from_config
    train_cfg = types.SimpleNamespace(epochs=6, batchsize=2, lr=1e-4, betas=(0.9, 0.999), save_epochs=2, num_threads=0)
    assert optim_options_from_config(train_cfg) == {
        'optimizer': 'Adam', 'momentum': 0.99, 'nesterov': True, 'weight_decay': 0.0, 'max_grad_norm': None,
        'lr_schedule': None}
    # the shipped config keeps the reference's keys
    from segmentation3d.utils.file_io import load_config
    import os
    shipped = load_config(os.path.join(PKG, 'segmentation3d', 'config', 'train_config.py'))
    got = optim_options_from_config(shipped.train, num_samples=10)
    assert got['optimizer'] == 'Adam' and got['max_grad_norm'] is None and got['lr_schedule'] is None
    assert got['weight_decay'] == 0.0


def test_optim_options_from_config_reads_the_new_keys():
    from segmentation3d.core.seg_train import optim_options_from_config
    train_cfg = types.SimpleNamespace(epochs=5, batchsize=2, optimizer='SGD', momentum=0.9, nesterov=False,
                                      weight_decay=3e-5, clip_grad_norm=12, lr_schedule='poly', lr_power=0.8,
                                      warmup_steps=2)
    got = optim_options_from_config(train_cfg, num_samples=7, world_size=2)
    assert got == {'optimizer': 'SGD', 'momentum': 0.9, 'nesterov': False, 'weight_decay': 3e-5, 'max_grad_norm': 12,
                   'lr_schedule': {'name': 'poly', 'total_steps': 9, 'warmup_steps': 2, 'power': 0.8}}   # ceil(35 / 4)
    train_cfg.total_steps = 100
    assert optim_options_from_config(train_cfg)['lr_schedule']['total_steps'] == 100
    train_cfg.optimizer = 'LAMB'
    with pytest.raises(ValueError):
        optim_options_from_config(train_cfg, num_samples=7)


def _param():
    return [torch.nn.Parameter(torch.zeros(3))]        # on the CPU: validation comes before any device work


@pytest.mark.parametrize('kw', [
    dict(lr=1e-2, nesterov=True),                                   # Nesterov without momentum
    dict(lr=1e-2, momentum=0.0, nesterov=True),
    dict(lr=-1e-2),
    dict(lr=1e-2, momentum=-0.1),
    dict(lr=1e-2, weight_decay=-1e-5),
    dict(lr=1e-2, max_grad_norm=-1.0),
    dict(lr=1e-2, lr_schedule={'name': 'linear', 'total_steps': 5}),
    dict(lr=1e-2, lr_schedule={'name': 'poly', 'total_steps': 0}),
    dict(lr=1e-2, lr_schedule={'name': 'poly'}),                    # a decaying schedule needs its horizon
    dict(lr=1e-2, lr_schedule={'name': 'poly', 'total_steps': 5, 'warmup_steps': -1}),
    dict(lr=1e-2, lr_schedule={'name': 'poly', 'total_steps': 5, 'power': -0.5}),
])
def test_fused_sgd_rejects_bad_values(kw):
    from segmentation3d.optim.fused_sgd import FusedSGD
    with pytest.raises(ValueError):
        FusedSGD(_param(), **kw)


@pytest.mark.parametrize('kw', [
    dict(max_grad_norm=-12.0),
    dict(lr_schedule={'name': 'exp', 'total_steps': 5}),
    dict(lr_schedule={'name': 'cosine', 'total_steps': 0}),
    dict(lr_schedule={'name': 'cosine', 'total_steps': 5, 'warmup_steps': -2}),
])
def test_fused_adam_rejects_bad_values(kw):
    from segmentation3d.optim.fused_adam import FusedAdam
    with pytest.raises(ValueError):
        FusedAdam(_param(), lr=1e-3, **kw)


def test_train_step_rejects_unknown_optimizer_options():
    from segmentation3d.core.seg_train import build_optimizer
    with pytest.raises(ValueError):
        build_optimizer('RMSprop', _param(), 1e-3)
    with pytest.raises(ValueError):
        build_optimizer('SGD', _param(), 1e-3, optim_options={'dampening': 0.1})
