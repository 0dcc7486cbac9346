"""FusedAdam -- `torch.optim.Adam` semantics (core/seg_train.py:83,127 of the reference: Adam(lr, betas), eps 1e-8,
no weight decay, no amsgrad) executed as ONE HIP kernel over a flat parameter buffer.

MI355X-first layout: all parameters of a group live in one contiguous fp32 buffer (likewise gradients, exp_avg,
exp_avg_sq); `p.data` / `p.grad` are views into it.  One launch updates 14.56 M parameters (28 B/param of HBM traffic)
and the data-parallel gradient all-reduce works on contiguous slices of the same buffer (core/ddp.py).
With `direct_grads` (default) every parameter's slice of the gradient buffer is registered as a gradient sink
(`_grad_sink.py`): the backward kernels accumulate into it themselves instead of autograd adding a temporary.
`state_dict()` / `load_state_dict()` keep torch.optim.Adam's structure (`step`, `exp_avg`, `exp_avg_sq` per
parameter), so `optimizer.pth` files are interchangeable with the reference's.
The flat-buffer machinery is optim/flat_optimizer.py's, shared with FusedSGD.  With `max_grad_norm` and `lr_schedule`
both None (default) an eager step is one `seg3d_adam_step` with host-side scalars.  Everything else -- either option
set, or the step count moved to the device for a captured train step (use_device_step) -- goes through the device
control block: `seg3d_optim_prepare` -> `seg3d_adam_step_ctl`, the same update with the same bits.
"""
from segmentation3d import _engine as E
from segmentation3d.optim.flat_optimizer import FlatBufferOptimizer


class FusedAdam(FlatBufferOptimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, direct_grads=True,
                 max_grad_norm=None, lr_schedule=None):
        if lr < 0.0 or eps < 0.0 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError('invalid Adam hyper-parameters')
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super(FusedAdam, self).__init__(params, defaults, direct_grads=direct_grads, max_grad_norm=max_grad_norm,
                                        lr_schedule=lr_schedule)

    def _state_buffer_names(self, group):
        return ('exp_avg', 'exp_avg_sq')

    def _launch(self, group, f):
        beta1, beta2 = group['betas']
        E.call('seg3d_adam_step', E.ptr(f['params']), E.ptr(f['grads']), E.ptr(f['exp_avg']), E.ptr(f['exp_avg_sq']),
               f['total'], f['step'], float(group['lr']), float(beta1), float(beta2), float(group['eps']),
               float(group['weight_decay']), float(self.grad_scale), E.stream_ptr())

    def _launch_control(self, group, f):
        beta1, beta2 = group['betas']
        E.call('seg3d_adam_step_ctl', E.ptr(f['params']), E.ptr(f['grads']), E.ptr(f['exp_avg']), E.ptr(f['exp_avg_sq']),
               f['total'], E.ptr(f['ctl']), float(beta1), float(beta2), float(group['eps']),
               float(group['weight_decay']), E.stream_ptr())
