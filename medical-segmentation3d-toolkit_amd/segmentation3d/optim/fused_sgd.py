"""FusedSGD -- `torch.optim.SGD` semantics (momentum, Nesterov, L2 weight decay; dampening 0) executed as ONE HIP
kernel over a flat parameter buffer: the optimizer of the nnU-Net-family recipe the DiceCE loss comes from (Nesterov
momentum 0.99, weight decay 3e-5, global-norm clipping at 12, polynomial decay of the learning rate).

Flat buffers, gradient sinks and the device control block are optim/flat_optimizer.py's, shared with FusedAdam.  Every
step goes through the control block (`seg3d_optim_prepare` -> `seg3d_sgd_step_ctl`, preceded by the sum-of-squares pass
when `max_grad_norm` is set): 20 B/param of HBM traffic against Adam's 28, no host read-back, capturable.
`state_dict()` has torch's `momentum_buffer` per parameter (when momentum > 0) plus `step`, which torch.optim.SGD
ignores; a torch.optim.SGD state dict loads (its step count is unknown: the schedule restarts at step 0).
"""
from segmentation3d import _engine as E
from segmentation3d.optim.flat_optimizer import FlatBufferOptimizer


class FusedSGD(FlatBufferOptimizer):
    _ALWAYS_CONTROL = True
    _ZERO_MISSING_STATE = True

    def __init__(self, params, lr, momentum=0.0, nesterov=False, weight_decay=0.0, max_grad_norm=None, lr_schedule=None,
                 direct_grads=True):
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError('invalid SGD hyper-parameters: lr, momentum and weight_decay must be >= 0')
        if nesterov and not momentum > 0.0:
            raise ValueError('Nesterov momentum needs momentum > 0')
        defaults = dict(lr=lr, momentum=momentum, nesterov=bool(nesterov), weight_decay=weight_decay)
        super(FusedSGD, self).__init__(params, defaults, direct_grads=direct_grads, max_grad_norm=max_grad_norm,
                                       lr_schedule=lr_schedule)

    def _state_buffer_names(self, group):
        return ('momentum_buffer',) if group['momentum'] > 0.0 else ()

    def _launch_control(self, group, f):
        E.call('seg3d_sgd_step_ctl', E.ptr(f['params']), E.ptr(f['grads']), E.ptr(f.get('momentum_buffer', None)),
               f['total'], E.ptr(f['ctl']), float(group['momentum']), float(group['weight_decay']),
               int(bool(group['nesterov'])), E.stream_ptr())
