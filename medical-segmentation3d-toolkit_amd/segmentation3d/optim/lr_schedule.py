"""Learning-rate schedules of the fused optimizers -- host restatement of the rule that `seg3d_optim_prepare`
(csrc/adam.hip) evaluates on the device, for logging, for `param_groups[i]['lr']` and for the tests.

With s = step - 1 completed steps and T = total_steps:   lr = base_lr * w(s) * d(s)
    warm-up  w = min(1, (s + 1) / warmup_steps), or 1 when warmup_steps == 0
    decay    d = 1                                    'constant'
             d = max(0, 1 - s / T) ** power           'poly'    (0 for every s >= T)
             d = 0.5 * (1 + cos(pi * min(s, T) / T))  'cosine'
"""
import math

SCHEDULE_CODES = {'constant': 0, 'poly': 1, 'cosine': 2}      # SEG3D_SCHEDULE_* of include/seg3d_hip.h


def normalize_schedule(lr_schedule):
    """None, or a checked copy {'name', 'total_steps', 'warmup_steps', 'power'} of the `lr_schedule` dict"""
    if lr_schedule is None:
        return None
    if not isinstance(lr_schedule, dict):
        raise ValueError('lr_schedule must be None or a dict, got {!r}'.format(lr_schedule))
    unknown = set(lr_schedule) - {'name', 'total_steps', 'warmup_steps', 'power'}
    if unknown:
        raise ValueError('unknown lr_schedule keys: {}'.format(sorted(unknown)))
    name = lr_schedule.get('name', 'constant')
    if name not in SCHEDULE_CODES:
        raise ValueError('unknown lr_schedule name {!r} (one of {})'.format(name, sorted(SCHEDULE_CODES)))
    total_steps = lr_schedule.get('total_steps', 1 if name == 'constant' else None)
    if total_steps is None or int(total_steps) != total_steps or int(total_steps) < 1:
        raise ValueError('lr_schedule total_steps must be an integer >= 1, got {!r}'.format(total_steps))
    warmup_steps = lr_schedule.get('warmup_steps', 0)
    if int(warmup_steps) != warmup_steps or int(warmup_steps) < 0:
        raise ValueError('lr_schedule warmup_steps must be an integer >= 0, got {!r}'.format(warmup_steps))
    power = float(lr_schedule.get('power', 0.9))
    if not power >= 0.0:
        raise ValueError('lr_schedule power must be >= 0, got {!r}'.format(power))
    return {'name': name, 'total_steps': int(total_steps), 'warmup_steps': int(warmup_steps), 'power': power}


def lr_at(step, base_lr, name='constant', total_steps=1, warmup_steps=0, power=0.9):
    """learning rate that optimisation step `step` (1-based: the first step is 1) uses"""
    if step < 1:
        raise ValueError('lr_at: steps count from 1, got {}'.format(step))
    if name not in SCHEDULE_CODES:
        raise ValueError('unknown lr_schedule name {!r}'.format(name))
    s = float(step - 1)
    T = float(total_steps)
    w = min(1.0, (s + 1.0) / float(warmup_steps)) if warmup_steps > 0 else 1.0
    if name == 'poly':
        d = max(0.0, 1.0 - s / T) ** power
    elif name == 'cosine':
        d = 0.5 * (1.0 + math.cos(math.pi * min(s, T) / T))
    else:
        d = 1.0
    return base_lr * w * d
