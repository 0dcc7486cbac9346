"""The compound loss family and what shares its code, driven through the C ABI against the plain float64 references of
tests/compound_cases.py: seg3d_softmax_fwd/bwd, seg3d_sigmoid_fwd/bwd, seg3d_compound_loss_fwd/bwd, seg3d_topk_loss_fwd/bwd,
seg3d_boundary_loss_fwd/bwd (phi a given input of noise with a distance map's signs) and seg3d_confusion_counts.  The cases are
those of tests/compound_cases.py; tests/test_compound_cases.py shows on the host that each reaches the <CT, VEC> instantiation,
block count, finalize round, lane step and grid-stride trip it is named for.

Operands (compound_cases.loss_inputs, head_inputs, confusion_inputs): soft-max probabilities with selected p_t of 0, 1e-30, 1e-12,
1.0 and 0.5; targets that are integer ids, ids outside [0, C) (-1, C, C + 3, 1000), the ignore label inside and outside [0, C),
in-contract non-integers (0.5, 1.7, C - 0.25, 0.3), -0.5 and -0.0; a class absent from a sample, a sample and a whole case with
nothing counted; a zero class weight, unnormalised alpha, a zero region weight, either term weight 0, gout != 1.  Every output and
workspace is a buffer of exactly the documented size (elements or bytes) filled with NaN -- integers with a fixed pattern -- inside
guard bands: afterwards every guard is bit-identical, every element the header says is written is finite (not the pattern), and
every input is bit-identical to what it was.  A case on the 16-byte path is launched a second time with probs, target, ell and the
gradient one float past a 16-byte boundary (the scalar path) and held to the same reference under the same bars.

Bars: nothing is pinned to what the kernels give.  Each case evaluates the same reference function in float32 on the CPU: the
yardstick.  err <= 4 * yardstick + floor * scale, floor = 1e-5 for loss figures and coef, 2e-6 for per-voxel outputs, under the
caps of the existing tests: loss 1e-4 of max(1, |ref|), gradient relative L2 1e-4, tau within 4 ulp, the selection integers and the
confusion counts exact.  dprobs, ell and the head's din on a one-plane gradient are compared PER ELEMENT relative to |ref| (to 1e-30
below it), the yardstick taken the same way; the head's din on a dense gradient, p_c (d_c - sum p d), cancels and is compared to
the scale.  Exact: zeros on every plane of a voxel that does not count, on planes c != (int)t when the region term is off, no
distribution gradient where p_t < 1e-12 (an element whose reference is 0.0 must be 0.0); a negative ell exactly on the voxels that do
not count; loss[1] of top-k and of boundary bit-equal to the compound loss's on the same inputs and path.

Figures, MI355X, the largest over the cases of a family, the scalar relaunches included (a run appends every figure to the parity
report that gpu_util.report writes).  Scaled figures (loss, coef, probs, din) are absolute beside their scale; per-element figures
(dprobs, ell, one-plane din) are relative:
    compound  loss    err 6.8e-7  yardstick 7.1e-7  bar 9.7e-5  (scale 9.6)                              err / bar 0.013
              coef    err 9.3e-4  yardstick 2.2e-3  bar 2.8e-1  (scale 2.8e4: a sample with nothing counted) err / bar 0.014
              dprobs  per element: err 3.6e-7  yardstick 4.6e-7  bar 3.9e-6; relative L2 2.2e-7 (cap 1e-4) err / bar 0.11
    top-k     loss    err 3.1e-6  yardstick 3.1e-6  bar 5.1e-4  (scale 49)                               err / bar 0.014
              coef    err 4.7e-4  yardstick 1.3e-3  bar 2.8e-1  (scale 2.8e4)                           err / bar 0.013
              ell     per element: err 2.0e-7  yardstick 1.3e-7  bar 2.5e-6                              err / bar 0.081
              dprobs  per element: err 2.3e-7  yardstick 3.2e-7  bar 3.3e-6; relative L2 1.2e-7          err / bar 0.077
              tau     1.6 ulp at most (cap 4); n, k, m, n_eq, r exact in every case
    boundary  loss    err 7.9e-8  yardstick 1.2e-7  bar 1.3e-5  (scale 1.2)                              err / bar 0.006
              coef    err 9.7e-4  yardstick 1.3e-3  bar 3.0e-1  (scale 2.9e4)                           err / bar 0.008
              dprobs  per element: err 3.2e-7  yardstick 4.8e-7  bar 3.9e-6; relative L2 9.5e-8          err / bar 0.087
    softmax   probs   err 3.0e-7  yardstick 2.5e-7  bar 3.0e-6                                           err / bar 0.10
              din     dense: err 5.0e-7  yardstick 5.0e-7  bar 4.5e-6 (scale 1.6), relative L2 3.9e-6    err / bar 0.23
                      one plane, per element: err 1.4e-7  yardstick 1.4e-7  bar 2.6e-6                   err / bar 0.054
    sigmoid   probs   err 8.9e-8  yardstick 8.9e-8  bar 2.4e-6                                           err / bar 0.038
              din     per element: err 1.7e-7  yardstick 1.7e-7  bar 2.7e-6 (dense and one plane)        err / bar 0.064
    confusion every count exact
Every exact comparison holds, every guard is intact, loss[1] of top-k and of boundary is bit-equal to the compound loss's in every
case and on both paths.  With the parent's register path in compound_bwd_body (p_t picked by `t == (float)c`) the 16-byte launch
of the compound and top-k cases with C <= 5 and the distribution term on misses the per-element bar by 100 % on exactly the
counted non-integer targets (the gradient's distribution part is dropped there) while their scalar relaunch passes; the path now
takes the class of the counting rule.  The slowest case is the 4 211 716-voxel top-k one (1.0 s, references and the scalar relaunch
included; compound 0.4 s, boundary 0.4 s, the 2 097 230-voxel head cases 0.6 s and 0.8 s); the file takes 7 s: 25 compound, 28
top-k, 25 boundary, 14 head and 23 confusion cases and the refusals.
"""
import time

import pytest
import torch

import compound_cases as K
from float64_util import FLOOR_EW, FLOOR_RED, Figures, Guarded, _engine

pytestmark = pytest.mark.gpu

GUARD = 1024
CAP_LOSS, CAP_GRAD_L2, TAU_ULPS = 1e-4, 1e-4, 4          # tests/test_gpu_compound_loss.py, test_gpu_topk_loss.py, test_gpu_boundary_loss.py
F64, F32 = torch.float64, torch.float32


# ---- buffers -------------------------------------------------------------------------------------------------------------------------
class Inputs:
    """device copies of the inputs, `shift` floats past a 16-byte boundary where asked; afterwards compared bit for bit"""

    def __init__(self, dev):
        self.dev, self.kept = dev, []

    def put(self, name, t, shift=0):
        flat = t.contiguous().reshape(-1)
        buf = torch.empty(flat.numel() + 8, dtype=flat.dtype, device=self.dev)
        view = buf[shift:shift + flat.numel()]
        view.copy_(flat)
        assert view.data_ptr() % 16 == (shift * flat.element_size()) % 16
        self.kept.append((name, view, flat.clone()))
        return view

    def unchanged(self, fig):
        for name, view, orig in self.kept:
            bits = torch.int32 if orig.dtype == F32 else orig.dtype
            fig.require(bool(torch.equal(view.cpu().view(bits), orig.view(bits))), '{}: the input was written'.format(name))


def _outputs(dev, shift=0, shifted=(), **sizes):
    out = {}
    for k, n in sizes.items():
        dtype = {'workspace': torch.uint8, 'selection': torch.int64, 'counts': torch.int64}.get(k, F32)
        out[k] = Guarded(n, GUARD, dev, dtype=dtype, shift=shift if k in shifted else 0)
    return out


def _written(fig, bufs, skip=('workspace',)):
    for k, g in bufs.items():
        fig.require(g.guards_untouched(), '{}: the guard bands were written'.format(k))
        if k not in skip:
            fig.require(g.written(), '{}: an element was not written (or is not finite)'.format(k))


def _untouched(bufs):
    return all(g.all_nan() and g.guards_untouched() for g in bufs.values())


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------
def _rel_l2(fig, key, dev, ref, cap=CAP_GRAD_L2):
    norm = float(ref.norm())
    fig.figs[key + '_rel_l2'] = float((dev.double().reshape(ref.shape) - ref).norm()) / norm if norm > 0.0 else 0.0
    fig.require(fig.figs[key + '_rel_l2'] <= cap, '{}: relative L2 {:.3e} > {:.0e}'.format(key, fig.figs[key + '_rel_l2'], cap))


def _per_element(fig, key, dev, ref, yard, floor=FLOOR_EW, cap=CAP_GRAD_L2):
    """|dev - ref| <= bar * max(|ref|, 1e-30) for every element, bar = min(4 * yardstick + floor, cap), the yardstick the largest such
    ratio of the fp32 evaluation; an element whose reference is 0.0 must be 0.0"""
    dev = dev.double().reshape(ref.shape)
    if not bool(torch.isfinite(dev).all()):
        fig.fails.append('{}: {} elements are not finite'.format(key, int((~torch.isfinite(dev)).sum())))
        return
    zero = ref == 0.0
    fig.require(bool((dev[zero] == 0.0).all()), '{}: {} elements are not 0.0 where the reference is'.format(key, int((dev[zero] != 0.0).sum())))
    if bool(zero.all()):
        return
    ye, e = float(K.per_element(yard, ref).max()), K.per_element(dev, ref)
    err, bar = float(e.max()), min(4.0 * ye + floor, cap)
    fig.figs.update({key + '_relerr': err, key + '_relyard': ye, key + '_relbar': bar})
    fig.require(ye <= 1e-4, '{}: the fp32 yardstick is {:.3e} (relative) away from the float64 reference'.format(key, ye))
    if not err <= bar:
        at = int(e.reshape(-1).argmax())
        fig.fails.append('{}: per-element relative err {:.3e} > bar {:.3e} (yardstick {:.3e}) at flat index {}: {:.9e} against {:.9e}; '
                         '{} elements above the bar'.format(key, err, bar, ye, at, float(dev.reshape(-1)[at]), float(ref.reshape(-1)[at]),
                                                          int((e > bar).sum())))


def _loss_cap(ref):
    return CAP_LOSS * max(1.0, float(ref.abs().max()))


def _finish(fig, t0):
    torch.cuda.synchronize()
    fig.figs['seconds'] = time.perf_counter() - t0
    fig.done()


def _launches(c):
    """the case's own launch and, for a case on the 16-byte path, the scalar launch of the same inputs"""
    return [('', c.shift)] + ([('scalar_', 1)] if K.vec(c) else [])


def _gradient_checks(fig, key, c, d, ref, yard):
    N, C, S = c.N, c.C, c.S
    _per_element(fig, key, d, ref['dprobs'], yard['dprobs'])
    _rel_l2(fig, key, d, ref['dprobs'])
    d = d.reshape(N, C, S)
    off = ~ref['valid'].unsqueeze(1).expand(N, C, S)
    fig.require(bool((d[off] == 0.0).all()), '{}: not 0.0 on a voxel that does not count'.format(key))
    if c.dice_weight == 0.0 and not isinstance(c, K.Boundary):      # (the boundary term itself sits on every plane)
        fig.require(bool((d[ref['onehot'] == 0.0] == 0.0).all()), '{}: the region term is off, a plane c != (int)t is not 0.0'.format(key))


def _region_bits(E, dev, c, pd, td, wd, ad, got_lr, fig):
    """loss[1] of the compound loss on the same inputs and path, bit for bit"""
    o = _outputs(dev, part=K.part_floats(c.N, c.C, c.S), coef=2 * K.coef_rows(c) * c.C + 1, loss=3)
    E.call('seg3d_compound_loss_fwd', E.ptr(pd), E.ptr(td), E.ptr(wd), E.ptr(ad), E.ptr(o['part'].t), E.ptr(o['coef'].t), E.ptr(o['loss'].t),
           c.N, c.C, c.S, 0.0, 1.0, 1.0, c.batch_dice, c.ignore, E.stream_ptr())
    torch.cuda.synchronize()
    mine = o['loss'].t.cpu()[1:2]
    fig.require(bool(torch.equal(mine.view(torch.int32), got_lr.reshape(1).view(torch.int32))),
                'loss[1] {:.9e} is not bit-equal to the compound loss\'s {:.9e}'.format(float(got_lr), float(mine)))


# ---- compound loss -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.COMPOUND_CASES, ids=K.case_id)
def test_compound(hip_device, case):
    E, dev, c, t0 = _engine(), hip_device, case, time.perf_counter()
    N, C, S, R = c.N, c.C, c.S, K.coef_rows(c)
    fig = Figures('compound/' + K.case_id(c))
    p, t, wdice, alpha, gout = K.loss_inputs(c)
    ref, yard = [K.compound_ref(p, t, wdice, alpha, c, gout, dt) for dt in (F64, F32)]
    for tag, shift in _launches(c):
        i = Inputs(dev)
        pd, td, wd, ad, gd = i.put('probs', p, shift), i.put('target', t, shift), i.put('wdice', wdice), i.put('alpha', alpha), \
            i.put('gout', torch.tensor([gout]))
        assert E.query('seg3d_compound_loss_part_floats', N, C, S) == K.part_floats(N, C, S)
        o = _outputs(dev, shift, ('dprobs',), part=K.part_floats(N, C, S), coef=2 * R * C + 1, loss=3, dprobs=N * C * S)
        E.call('seg3d_compound_loss_fwd', E.ptr(pd), E.ptr(td), E.ptr(wd), E.ptr(ad), E.ptr(o['part'].t), E.ptr(o['coef'].t),
               E.ptr(o['loss'].t), N, C, S, c.gamma, c.dice_weight, c.ce_weight, c.batch_dice, c.ignore, E.stream_ptr())
        E.call('seg3d_compound_loss_bwd', E.ptr(pd), E.ptr(td), E.ptr(o['coef'].t), E.ptr(ad), E.ptr(gd), E.ptr(o['dprobs'].t), N, C, S,
               c.gamma, c.batch_dice, c.ignore, E.stream_ptr())
        torch.cuda.synchronize()
        _written(fig, o)
        i.unchanged(fig)
        fig.check(tag + 'loss', o['loss'].t.cpu(), ref['loss'], yard['loss'], FLOOR_RED, cap=_loss_cap(ref['loss']))
        fig.check(tag + 'coef', o['coef'].t.cpu(), ref['coef'], yard['coef'], FLOOR_RED)
        _gradient_checks(fig, tag + 'dprobs', c, o['dprobs'].t.cpu(), ref, yard)
    _finish(fig, t0)


# ---- Dice + top-k --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.TOPK_CASES + [K.TIE_CASE], ids=K.case_id)
def test_topk(hip_device, case):
    E, dev, c, t0 = _engine(), hip_device, case, time.perf_counter()
    N, C, S, R = c.N, c.C, c.S, K.coef_rows(c)
    fig = Figures('compound/' + K.case_id(c))
    p, t, wdice, alpha, gout = K.loss_inputs(c)
    ref, yard = [K.topk_ref(p, t, wdice, alpha, c, gout, dt) for dt in (F64, F32)]
    valid = ref['valid']
    for tag, shift in _launches(c):
        i = Inputs(dev)
        pd, td, wd, ad, gd = i.put('probs', p, shift), i.put('target', t, shift), i.put('wdice', wdice), i.put('alpha', alpha), \
            i.put('gout', torch.tensor([gout]))
        nbytes = E.query('seg3d_topk_loss_workspace_bytes', N, C, S)
        assert nbytes == K.topk_workspace_bytes(N, C, S)
        o = _outputs(dev, shift, ('ell', 'dprobs'), workspace=nbytes, ell=N * S, coef=2 * R * C + 3, loss=3, selection=5, threshold=1,
                     dprobs=N * C * S)
        E.call('seg3d_topk_loss_fwd', E.ptr(pd), E.ptr(td), E.ptr(wd), E.ptr(ad), E.ptr(o['workspace'].t), E.ptr(o['ell'].t),
               E.ptr(o['coef'].t), E.ptr(o['loss'].t), E.ptr(o['selection'].t), E.ptr(o['threshold'].t), N, C, S, c.k_percent,
               c.dice_weight, c.ce_weight, c.batch_dice, c.ignore, E.stream_ptr())
        torch.cuda.synchronize()
        ell_bits = o['ell'].t.clone()
        E.call('seg3d_topk_loss_bwd', E.ptr(pd), E.ptr(td), E.ptr(o['ell'].t), E.ptr(o['coef'].t), E.ptr(ad), E.ptr(gd),
               E.ptr(o['dprobs'].t), N, C, S, c.batch_dice, c.ignore, E.stream_ptr())
        torch.cuda.synchronize()
        _written(fig, o)
        i.unchanged(fig)
        fig.require(bool(torch.equal(ell_bits.view(torch.int32), o['ell'].t.view(torch.int32))), tag + 'ell: the backward wrote it')
        sel, ell = tuple(o['selection'].t.cpu().tolist()), o['ell'].t.cpu().reshape(N, S)
        fig.require(sel == ref['selection'], '{}selection {} != {}'.format(tag, sel, ref['selection']))
        tau, tau_ref = o['threshold'].t.cpu(), ref['tau'].float().reshape(1)
        ulp = float(torch.nextafter(tau_ref.abs(), torch.tensor([float('inf')])) - tau_ref.abs())
        fig.figs[tag + 'tau_ulps'] = abs(float(tau) - float(ref['tau'])) / ulp
        fig.require(fig.figs[tag + 'tau_ulps'] <= TAU_ULPS, '{}tau {:.9e} against {:.9e}'.format(tag, float(tau), float(ref['tau'])))
        fig.require(float(tau) == float(o['coef'].t[2 * R * C]), tag + 'threshold and coef disagree on tau')
        fig.require(bool((ell[~valid] < 0.0).all()) and bool((ell[valid] >= 0.0).all()) and not bool(torch.signbit(ell[valid]).any()),
                    tag + 'ell: the sentinel is not exactly on the voxels that do not count')
        if bool(valid.any()):
            _per_element(fig, tag + 'ell', ell[valid], ref['ell'][valid], yard['ell'][valid])
        fig.check(tag + 'loss', o['loss'].t.cpu(), ref['loss'], yard['loss'], FLOOR_RED, cap=_loss_cap(ref['loss']))
        fig.check(tag + 'coef', o['coef'].t.cpu(), ref['coef'], yard['coef'], FLOOR_RED)
        _gradient_checks(fig, tag + 'dprobs', c, o['dprobs'].t.cpu(), ref, yard)
        _region_bits(E, dev, c, pd, td, wd, ad, o['loss'].t.cpu()[1], fig)
    _finish(fig, t0)


# ---- Dice + boundary -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.BOUNDARY_CASES, ids=K.case_id)
def test_boundary(hip_device, case):
    E, dev, c, t0 = _engine(), hip_device, case, time.perf_counter()
    N, C, S, R = c.N, c.C, c.S, K.coef_rows(c)
    fig = Figures('compound/' + K.case_id(c))
    p, t, wdice, alpha, gout = K.loss_inputs(c)
    phi = K.phi_input(c, t)
    ref, yard = [K.boundary_ref(p, t, phi, wdice, c, gout, dt) for dt in (F64, F32)]
    for tag, shift in _launches(c):
        i = Inputs(dev)
        pd, td, hd, wd, ad = i.put('probs', p, shift), i.put('target', t, shift), i.put('phi', phi), i.put('wdice', wdice), i.put('alpha', alpha)
        bd, gd = i.put('boundary_weight', torch.tensor([K.BOUNDARY_WEIGHT])), i.put('gout', torch.tensor([gout]))
        nbytes = E.query('seg3d_boundary_loss_workspace_bytes', N, C, S)
        assert nbytes == K.boundary_workspace_bytes(N, C, S)
        o = _outputs(dev, shift, ('dprobs',), workspace=nbytes, coef=2 * R * C + C, loss=3, dprobs=N * C * S)
        E.call('seg3d_boundary_loss_fwd', E.ptr(pd), E.ptr(td), E.ptr(hd), E.ptr(wd), E.ptr(bd), E.ptr(o['workspace'].t), E.ptr(o['coef'].t),
               E.ptr(o['loss'].t), N, C, S, c.dice_weight, c.include_background, c.batch_dice, c.ignore, E.stream_ptr())
        E.call('seg3d_boundary_loss_bwd', E.ptr(td), E.ptr(hd), E.ptr(o['coef'].t), E.ptr(gd), E.ptr(o['dprobs'].t), N, C, S,
               c.include_background, c.batch_dice, c.ignore, E.stream_ptr())
        torch.cuda.synchronize()
        _written(fig, o)
        i.unchanged(fig)
        fig.check(tag + 'loss', o['loss'].t.cpu(), ref['loss'], yard['loss'], FLOOR_RED, cap=_loss_cap(ref['loss']))
        fig.check(tag + 'coef', o['coef'].t.cpu(), ref['coef'], yard['coef'], FLOOR_RED)
        _gradient_checks(fig, tag + 'dprobs', c, o['dprobs'].t.cpu(), ref, yard)
        _region_bits(E, dev, c, pd, td, wd, ad, o['loss'].t.cpu()[1], fig)
    _finish(fig, t0)


# ---- head activations ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.HEAD_CASES, ids=K.case_id)
def test_head(hip_device, case):
    E, dev, c, t0 = _engine(), hip_device, case, time.perf_counter()
    N, C, S = c.N, c.C, c.S
    fig = Figures('compound/' + K.case_id(c))
    x, d = K.head_inputs(c)
    p, py = [K.head_fwd_ref(c.kind, x, dt) for dt in (F64, F32)]
    i = Inputs(dev)
    xd = i.put('in', x)
    o = _outputs(dev, probs=N * C * S)
    E.call('seg3d_{}_fwd'.format(c.kind), E.ptr(xd), E.ptr(o['probs'].t), N, C, S, E.stream_ptr())
    torch.cuda.synchronize()
    _written(fig, o)
    got = o['probs'].t.cpu()
    fig.check('probs', got, p, py, FLOOR_EW)
    fig.require(float(got.min()) >= 0.0 and float(got.max()) <= 1.0, 'probs: outside [0, 1]')
    # the backward on the reference's probabilities (rounded to float32), so that its reference does not depend on the forward kernel
    p32 = p.float()
    pd = i.put('probs', p32)
    for key, dd in (('din', d), ('din_sparse', K.sparse_dprobs(p32, d))):
        g, gy = [K.head_bwd_ref(c.kind, p32, dd, dt) for dt in (F64, F32)]
        dpd = i.put('dprobs', dd)
        ob = _outputs(dev, din=N * S * C)
        E.call('seg3d_{}_bwd'.format(c.kind), E.ptr(pd), E.ptr(dpd), E.ptr(ob['din'].t), N, C, S, E.stream_ptr())
        torch.cuda.synchronize()
        _written(fig, ob)
        fig.check(key, ob['din'].t.cpu(), g, gy, FLOOR_EW)
        _rel_l2(fig, key, ob['din'].t.cpu(), g)
        if key == 'din_sparse' or c.kind == 'sigmoid':
            _per_element(fig, key, ob['din'].t.cpu(), g, gy)
    i.unchanged(fig)
    _finish(fig, t0)


# ---- confusion counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', K.CONFUSION_CASES, ids=K.case_id)
def test_confusion(hip_device, case):
    E, dev, c, t0 = _engine(), hip_device, case, time.perf_counter()
    fig = Figures('compound/' + K.case_id(c))
    p, t, counts0 = K.confusion_inputs(c)
    want = counts0 + K.confusion_ref(p, t, c.ignore).reshape(-1)
    i = Inputs(dev)
    pd, td = i.put('probs', p, c.shift), i.put('target', t, c.shift)
    o = {'counts': Guarded(3 * c.C, 16, dev, dtype=torch.int64, fill=counts0.to(dev))}
    E.call('seg3d_confusion_counts', E.ptr(pd), E.ptr(td), E.ptr(o['counts'].t), c.N, c.C, c.S, c.ignore, E.stream_ptr())
    torch.cuda.synchronize()
    _written(fig, o)
    i.unchanged(fig)
    got = o['counts'].t.cpu()
    fig.require(bool(torch.equal(got, want)), 'counts {} != {}'.format(got.tolist(), want.tolist()))
    fig.figs['wrong_counts'] = float((got != want).sum())
    _finish(fig, t0)


# ---- one refusal per entry: every output is still untouched ------------------------------------------------------------------------------
def test_refusals(hip_device):
    E, dev = _engine(), hip_device
    N, C, S, BAD = 1, 2, 8, K.MAXC + 1
    ones, st = torch.ones(BAD * S, device=dev), E.stream_ptr
    o = _outputs(dev, probs=BAD * S, din=BAD * S, part=K.part_floats(N, BAD, S), coef=2 * BAD + BAD, loss=3, dprobs=BAD * S, ell=S,
                 workspace=K.topk_workspace_bytes(N, BAD, S), selection=5, threshold=1)
    o['counts'] = Guarded(3 * BAD, 16, dev, dtype=torch.int64)
    P, q = E.ptr(ones), {k: E.ptr(g.t) for k, g in o.items()}
    calls = {
        'seg3d_softmax_fwd': (P, q['probs'], N, BAD, S, st()), 'seg3d_softmax_bwd': (P, P, q['din'], N, BAD, S, st()),
        'seg3d_sigmoid_fwd': (P, q['probs'], N, BAD, S, st()), 'seg3d_sigmoid_bwd': (P, P, q['din'], N, BAD, S, st()),
        'seg3d_compound_loss_fwd': (P, P, P, P, q['part'], q['coef'], q['loss'], N, C, S, 0.0, 0.0, 0.0, 0, -1.0, st()),
        'seg3d_compound_loss_bwd': (P, P, P, P, P, q['dprobs'], N, C, S, -1.0, 0, -1.0, st()),
        'seg3d_topk_loss_fwd': (P, P, P, P, q['workspace'], q['ell'], q['coef'], q['loss'], q['selection'], q['threshold'], N, C, S, 0.0,
                                1.0, 1.0, 0, -1.0, st()),
        'seg3d_topk_loss_bwd': (P, P, P, P, P, P, q['dprobs'], N, BAD, S, 0, -1.0, st()),
        'seg3d_boundary_loss_fwd': (P, P, P, P, P, q['workspace'], q['coef'], q['loss'], N, 1, S, 1.0, 0, 0, -1.0, st()),
        'seg3d_boundary_loss_bwd': (P, P, P, P, q['dprobs'], N, 1, S, 0, 0, -1.0, st()),
        'seg3d_confusion_counts': (P, P, q['counts'], N, BAD, S, -1.0, st()),
    }
    assert sorted(calls) == sorted(K.REFUSALS)
    for name, args in calls.items():
        with pytest.raises(ValueError) as info:
            E.call(name, *args)
        assert str(info.value).startswith(name + ':'), (name, K.REFUSALS[name], str(info.value))
    torch.cuda.synchronize()
    assert _untouched(o)
