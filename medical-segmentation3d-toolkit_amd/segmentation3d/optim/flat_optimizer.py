"""Flat-buffer machinery shared by FusedAdam and FusedSGD.

MI355X-first layout: all parameters of a group live in one contiguous fp32 buffer (likewise gradients and every
per-parameter state buffer); `p.data` / `p.grad` are views into it.  One launch updates the whole group and the
data-parallel gradient all-reduce works on contiguous slices of the same buffer (core/ddp.py).
With `direct_grads` (default) every parameter's slice of the gradient buffer is registered as a gradient sink
(`_grad_sink.py`): the backward kernels accumulate into it themselves instead of autograd adding a temporary.

A step is one of two things.  Without a control block (FusedAdam with neither `max_grad_norm` nor `lr_schedule`, stepping
eagerly) it is one launch with host-side scalars, `seg3d_adam_step`.  With one -- `max_grad_norm` and / or `lr_schedule`
given, always for FusedSGD, and for every optimizer after use_device_step(), which TrainStep calls before it captures a
hipGraph -- the step count, the learning rate, the clip coefficient and the gradient norm live on the device (SEG3D_CTL_*
of include/seg3d_hip.h), so that the same launches serve an eager step and a captured one, and nothing is read back:
    [seg3d_grad_sumsq_partial per group, only when clipping] -> per group: seg3d_optim_prepare -> the update kernel
The host keeps its own count beside the device's (`step` and `step_dev` of a group) for `state_dict()` and the schedule's
`group['lr']`; a graph replay advances the device's alone and the host follows in note_replayed_step().
The norm is that of ALL groups together, times `grad_scale` (the mean gradient under data parallelism: every rank
computes the same coefficient from the same reduced buffer).  As in torch.nn.utils.clip_grad_norm_, a step whose norm
is not finite is not skipped.
"""
import ctypes

import torch

from segmentation3d import _engine as E
from segmentation3d import _grad_sink as G
from segmentation3d.optim.lr_schedule import SCHEDULE_CODES, lr_at, normalize_schedule

_ALIGN = 64  # floats; keeps every parameter view 256-byte aligned (kernels read gamma/beta/weights with 16-byte loads)
_CTL_FLOATS, _CTL_LR, _CTL_NORM, _CTL_COEF = 8, 0, 4, 5    # SEG3D_CTL_* of include/seg3d_hip.h
_CONSTANT = {'name': 'constant', 'total_steps': 1, 'warmup_steps': 0, 'power': 0.9}


class FlatBufferOptimizer(torch.optim.Optimizer):
    _ALWAYS_CONTROL = False        # FusedSGD has no host-argument kernel: it always steps through the control block
    _ZERO_MISSING_STATE = False    # load_state_dict of a state without the buffers: zero them (torch.optim.SGD dicts)

    def __init__(self, params, defaults, direct_grads=True, max_grad_norm=None, lr_schedule=None):
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError('max_grad_norm must be None or > 0, got {!r}'.format(max_grad_norm))
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.lr_schedule = normalize_schedule(lr_schedule)
        super(FlatBufferOptimizer, self).__init__(params, defaults)
        self._flat = []  # per group: dict(list, offsets, params, grads, <state buffers>, step, total)
        self.grad_scale = 1.0  # set to 1/world_size by the data-parallel wrapper after a sum all-reduce
        self.direct_grads = bool(direct_grads)
        # _control: every group has a control block (step_dev, ctl) and the kernels count the steps on the device, so that
        # a whole train step can be captured in a hipGraph and replayed; the host count follows in note_replayed_step()
        self._control = False
        self._part, self._nparts = None, 0
        for group in self.param_groups:
            if self.lr_schedule is not None:
                group.setdefault('initial_lr', group['lr'])     # torch's scheduler convention: the base rate
            self._flat.append(self._flatten_group(group))
        if self._ALWAYS_CONTROL or self.max_grad_norm is not None or self.lr_schedule is not None:
            self._alloc_control()

    def _state_buffer_names(self, group):
        """names of the per-parameter state tensors kept flat, in allocation order"""
        raise NotImplementedError

    def _launch(self, group, f):
        """the update with host-side scalars, step count f['step'] included"""
        raise NotImplementedError

    def _launch_control(self, group, f):
        """the update that reads lr / gradient multiplier / bias corrections from f['ctl']"""
        raise NotImplementedError

    # ---- flat buffers ------------------------------------------------------------------------------------------
    def _flatten_group(self, group):
        ps = [p for p in group['params'] if p.requires_grad]
        if not ps:
            return None
        dev = ps[0].device
        for p in ps:
            if p.device != dev or p.dtype != torch.float32:
                raise ValueError('{} needs all parameters in float32 on one device'.format(type(self).__name__))
        E.require_device(ps[0])
        offsets, total = [], 0
        for p in ps:
            offsets.append(total)
            total += (p.numel() + _ALIGN - 1) // _ALIGN * _ALIGN
        names = tuple(self._state_buffer_names(group))
        flat_p = torch.zeros(total, dtype=torch.float32, device=dev)
        flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        bufs = {k: torch.zeros(total, dtype=torch.float32, device=dev) for k in names}
        for p, off in zip(ps, offsets):
            n = p.numel()
            flat_p[off:off + n].copy_(p.data.reshape(-1))
            p.data = flat_p[off:off + n].view(p.shape)
            if p.grad is not None:
                flat_g[off:off + n].copy_(p.grad.reshape(-1))
            p.grad = flat_g[off:off + n].view(p.shape)
            if self.direct_grads:
                G.register(p, p.grad)
            st = {'step': torch.tensor(0.0)}
            for k in names:
                st[k] = bufs[k][off:off + n].view(p.shape)
            self.state[p] = st
        f = {'list': ps, 'offsets': offsets, 'params': flat_p, 'grads': flat_g, 'step': 0, 'total': total, 'names': names}
        f.update(bufs)
        return f

    def _alloc_control(self):
        live = [f for f in self._flat if f is not None]
        if not live:
            return
        off = 0
        for f in live:
            dev = f['params'].device
            f['step_dev'] = torch.full((1,), int(f['step']), dtype=torch.int32, device=dev)
            f['ctl'] = torch.zeros(_CTL_FLOATS, dtype=torch.float32, device=dev)
            f['part_off'] = off
            off += E.query('seg3d_grad_sumsq_part_count', f['total'])
        if self.max_grad_norm is not None:
            # one fp64 slot per workgroup of the sum-of-squares pass, the groups laid end to end
            self._part = torch.zeros(off, dtype=torch.float64, device=live[0]['params'].device)
            self._nparts = off
        self._control = True

    def use_device_step(self):
        """count the steps on the device (before capturing a train step in a hipGraph): an optimizer on host-side scalars
        gets its control block, and the device counters start from the host counts; idempotent"""
        if not self._control:
            self._alloc_control()
        for f in self._flat:
            if f is not None:
                f['step_dev'].fill_(int(f['step']))

    def _note_host_step(self, group, f):
        step_t = torch.tensor(float(f['step']))     # one host tensor shared by the group's per-parameter states
        for p in f['list']:
            self.state[p]['step'] = step_t
        if self.lr_schedule is not None and f['step'] >= 1:
            group['lr'] = lr_at(f['step'], group['initial_lr'], **self.lr_schedule)   # the rate that step used

    def note_replayed_step(self):
        """a captured step was replayed: the device advanced its counter, bring the host-side bookkeeping along"""
        for group, f in zip(self.param_groups, self._flat):
            if f is None:
                continue
            f['step'] += 1
            self._note_host_step(group, f)

    def step_counts(self):
        """the per-group host step counts (None for a group without parameters), for restore_step_counts()"""
        return [None if f is None else f['step'] for f in self._flat]

    def restore_step_counts(self, counts):
        """rewind the host counts, the per-parameter `state['step']` and the device counters to `counts`: after a graph
        capture, which ran step()'s host side without its kernels, or after one that failed"""
        for group, f, count in zip(self.param_groups, self._flat, counts):
            if f is None:
                continue
            f['step'] = count
            if self._control:
                f['step_dev'].fill_(int(count))
            self._note_host_step(group, f)

    def flat_grads(self):
        """list of flat gradient buffers (one per parameter group) -- what the data-parallel reducer all-reduces"""
        return [f['grads'] for f in self._flat if f is not None]

    def flat_layout(self):
        """[(parameter, group index, offset, numel)] in buffer order"""
        out = []
        for gi, f in enumerate(self._flat):
            if f is None:
                continue
            for p, off in zip(f['list'], f['offsets']):
                out.append((p, gi, off, p.numel()))
        return out

    def _control_view(self, slot):
        for f in self._flat:
            if f is not None and self._control:
                return f['ctl'][slot]
        return None

    @property
    def last_grad_norm(self):
        """0-dim DEVICE tensor, a view of the control block: the global gradient norm (times grad_scale) that the last
        step measured -- reading it is the caller's sync, not the optimizer's.  0 without max_grad_norm (the norm pass
        runs only when clipping); None off the control-block path."""
        return self._control_view(_CTL_NORM)

    @property
    def last_clip_coef(self):
        """0-dim device view: min(1, max_grad_norm / (norm + 1e-6)) of the last step (1 without max_grad_norm)"""
        return self._control_view(_CTL_COEF)

    @property
    def last_lr(self):
        """0-dim device view: the learning rate the first group's last step used"""
        return self._control_view(_CTL_LR)

    # ---- optimizer API -------------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=False):
        """zero the flat gradient buffer (one memset) and keep `p.grad` pointing into it"""
        for f in self._flat:
            if f is None:
                continue
            f['grads'].zero_()
            for p, off in zip(f['list'], f['offsets']):
                n = p.numel()
                if p.grad is None or p.grad.data_ptr() != f['grads'].data_ptr() + 4 * off:
                    p.grad = f['grads'][off:off + n].view(p.shape)
                    if self.direct_grads:
                        G.register(p, p.grad)

    def _gather_stray_grads(self, f):
        for p, off in zip(f['list'], f['offsets']):
            n = p.numel()
            view = f['grads'][off:off + n]
            if p.grad is None:
                if not self.direct_grads:
                    view.zero_()          # with sinks the kernels wrote here even though autograd never set .grad
                p.grad = view.view(p.shape)
            elif p.grad.data_ptr() != view.data_ptr():
                # a stray tensor (someone assigned p.grad): what autograd put there joins what the sinks wrote
                if self.direct_grads:
                    view.add_(p.grad.reshape(-1))
                else:
                    view.copy_(p.grad.reshape(-1))
                p.grad = view.view(p.shape)
            if p.data.data_ptr() != f['params'].data_ptr() + 4 * off:
                # someone re-assigned p.data (e.g. load_state_dict keeps storage, .to() does not): re-adopt it
                f['params'][off:off + n].copy_(p.data.reshape(-1))
                p.data = f['params'][off:off + n].view(p.shape)
                from segmentation3d import _ops
                _ops.PACK_CACHE.invalidate()

    def _step_control(self, live):
        stream = E.stream_ptr()
        clip = self.max_grad_norm is not None
        if clip:
            for _, f in live:
                E.call('seg3d_grad_sumsq_partial', E.ptr(f['grads']), f['total'],
                       ctypes.c_void_p(self._part.data_ptr() + 8 * f['part_off']), stream)
        sched = self.lr_schedule if self.lr_schedule is not None else _CONSTANT
        for group, f in live:
            base_lr = group['initial_lr'] if self.lr_schedule is not None else group['lr']
            beta1, beta2 = group.get('betas', (0.0, 0.0))
            E.call('seg3d_optim_prepare', E.ptr(f['step_dev']), E.ptr(f['ctl']), E.ptr(self._part), self._nparts,
                   float(self.grad_scale), self.max_grad_norm if clip else 0.0, SCHEDULE_CODES[sched['name']],
                   float(base_lr), sched['total_steps'], sched['warmup_steps'], sched['power'], float(beta1),
                   float(beta2), stream)
            self._launch_control(group, f)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        live = [(group, f) for group, f in zip(self.param_groups, self._flat) if f is not None]
        for group, f in live:
            self._gather_stray_grads(f)
            f['step'] += 1
        if self._control:
            self._step_control(live)
        else:
            for group, f in live:
                self._launch(group, f)
        for group, f in live:
            self._note_host_step(group, f)
        if live:
            # the kernel rewrote the parameters without touching their version counters: refresh (one launch) or
            # invalidate the packed conv-weight images
            from segmentation3d import _ops
            if _ops.PACK_CACHE.enabled:
                _ops.PACK_CACHE.repack_all()
            else:
                _ops.PACK_CACHE.invalidate()
        return loss

    def release_grad_sinks(self):
        """stop routing gradients into the flat buffer (e.g. before using torch.autograd.grad on these parameters)"""
        self.direct_grads = False
        for f in self._flat:
            if f is not None:
                G.unregister(f['list'])

    def load_state_dict(self, state_dict):
        super(FlatBufferOptimizer, self).load_state_dict(state_dict)
        for group in self.param_groups:              # a foreign dict (torch.optim.*) lacks the keys it does not know
            for k, v in self.defaults.items():
                group.setdefault(k, v)
            if self.lr_schedule is not None:
                group.setdefault('initial_lr', group['lr'])
        # torch replaced the state tensors with loaded copies: move them back into the flat buffers
        for group, f in zip(self.param_groups, self._flat):
            if f is None:
                continue
            step = 0
            for p, off in zip(f['list'], f['offsets']):
                n = p.numel()
                st = self.state.get(p, None)
                missing = st is None or any(st.get(k, None) is None for k in f['names'])
                if missing and not self._ZERO_MISSING_STATE:
                    continue
                if st is None:
                    st = self.state[p]
                for k in f['names']:
                    if missing:
                        f[k][off:off + n].zero_()
                    else:
                        f[k][off:off + n].copy_(st[k].reshape(-1).to(f[k].device))
                    st[k] = f[k][off:off + n].view(p.shape)
                step = max(step, int(float(st.get('step', 0.0))))
                st['step'] = torch.tensor(float(step))
            f['step'] = step
            if self._control:
                f['step_dev'].fill_(int(step))        # a step through the control block reads its count from the device
            if self.lr_schedule is not None and step >= 1:
                group['lr'] = lr_at(step, group['initial_lr'], **self.lr_schedule)
