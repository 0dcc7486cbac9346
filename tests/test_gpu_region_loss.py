"""The region loss (seg3d_region_loss_fwd / _bwd, csrc/region_loss.hip) on the GPU, through the C ABI and through
RegionDiceBCELoss, against the float64 oracle of tests/test_region_loss.py evaluated on the same float32 probabilities; the
Dice term against DiceCELoss's region term; run-to-run bits; TrainStep with a region loss, eager and in a hipGraph.

Shapes: S = 5x7x9 (scalar path with a tail), 4x4x8 (16-byte path), 1, 33x32x32 (nine workgroups per sample at DICE_VPB = 4096),
N in {1, 3}, R in {1, 2, 3, 5, 6, 16} (1..5: exact instantiations, 6 and 16: the generic one), BraTS's overlapping regions among
them; a 16-byte case is launched a second time one float past a 16-byte boundary (the scalar path at S % 4 == 0).
Values: labels of every region, background 0, a label in no region, and -1, 1.5, 256, 300, 255; probabilities with exact 0, 1,
0.5 and 1e-13 (below the clamp).  Every output sits in a NaN-filled buffer of the documented size between guard bands.

Bars (nothing is pinned to what the kernels give): each case evaluates the same oracle in float32 on the CPU -- the yardstick.
A term's bar is max(4 * |yardstick - oracle|, 1e-6), absolute (the terms are O(1): the few clamped voxels of a case add at most
27.6 / n_counted each).  The gradient's error and yardstick are max |g - oracle| / max |oracle|, the bar max(4 * yardstick, 1e-6).
Exact: zeros on every plane of a voxel that does not count, an all-zero gradient and L_bce = 0 when nothing counts, no BCE
gradient below the clamp, a term whose weight is 0 absent from L.

Only one captured graph is alive at any time and no two TrainSteps exist side by side: each is built, used, dropped,
followed by gc.collect() and PACK_CACHE.clear() before the next.

Figures on the MI355X: see DESIGN.md section 7, row f23."""
import gc

import pytest
import torch

from conftest import REPO  # noqa: F401
from float64_util import Guarded, _engine
from gpu_util import report
from test_region_loss import BRATS, oracle, region_targets

pytestmark = pytest.mark.gpu

GUARD = 1024
FLOOR = 1e-6
F64, F32 = torch.float64, torch.float32
SHAPES = {'5x7x9': (5, 7, 9), '4x4x8': (4, 4, 8), '1': (1,), '33x32x32': (33, 32, 32)}
NOWHERE = 30          # a label that no region lists: background for every region
REGIONS = {
    1: [[1]],
    2: [[1, 2], [2]],
    3: BRATS,
    5: [[1, 2, 3, 4, 5], [2, 3], [3], [4, 5], [5]],
    6: [[1], [2], [3], [4], [5], [6, 1]],
    16: [[k + 1, 17 + k % 3] for k in range(15)] + [[16, 200]],
}


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _inputs(seed, N, R, shape, stray=True):
    """sigmoid(2 randn) probabilities, labels drawn from {0, every listed label, NOWHERE}; from 16 voxels up a few targets are
    -1, 1.5, 256, 300 and 255 and a few probabilities exactly 0, 1, 0.5 and 1e-13"""
    g = torch.Generator().manual_seed(seed)
    S = _numel(shape)
    p = torch.sigmoid(2.0 * torch.randn((N, R, S), generator=g)).float()
    labels = torch.tensor([0, NOWHERE] + sorted({l for region in REGIONS[R] for l in region}), dtype=torch.float32)
    t = labels[torch.randint(0, labels.numel(), (N, S), generator=g)]
    if stray and S >= 16:
        for k, v in enumerate((-1.0, 1.5, 256.0, 300.0, 255.0)):
            t[(k % N), (3 * k + 1) % S] = v
        for k, v in enumerate((0.0, 1.0, 0.5, 1e-13, 1.0, 0.0)):
            p[(k % N), (k % R), (5 * k + 2) % S] = v          # (on a target of either kind: the draw decides)
    return p.reshape((N, R) + shape), t.reshape((N, 1) + shape)


def _put(dev, t, shift):
    flat = t.contiguous().reshape(-1)
    buf = torch.empty(flat.numel() + 8, dtype=flat.dtype, device=dev)
    view = buf[shift:shift + flat.numel()]
    view.copy_(flat)
    assert view.data_ptr() % 16 == (4 * shift) % 16
    return view


def _abi(dev, p, t, regions, weights=None, dice_weight=1.0, bce_weight=1.0, gamma=0.0, batch_dice=False, ignore_label=None,
         gout=1.0, shift=0):
    """forward + backward through the C ABI; returns (terms [3], dprobs like p), both on the host"""
    from segmentation3d import _ops
    from segmentation3d.loss.region_loss import region_lut
    E = _engine()
    N, R, S = p.shape[0], p.shape[1], _numel(p.shape[2:])
    w = torch.ones(R, dtype=F64) if weights is None else torch.tensor(weights, dtype=F64)
    wd, ad = (w / w.sum()).float().to(dev), w.float().to(dev)
    pd, td, gd = _put(dev, p, shift), _put(dev, t, shift), torch.tensor([gout], dtype=F32, device=dev)
    table = _ops._region_table(region_lut(regions))
    nblk = (S + 4095) // 4096
    rows = 1 if batch_dice else N
    assert E.query('seg3d_region_loss_part_floats', N, R, S) == N * nblk * (3 * R + 2)
    part, coef, loss = Guarded(N * nblk * (3 * R + 2), GUARD, dev), Guarded(2 * rows * R + 1, GUARD, dev), Guarded(3, GUARD, dev)
    dprobs = Guarded(N * R * S, GUARD, dev, shift=shift)
    ignore = -1.0 if ignore_label is None else float(ignore_label)
    E.call('seg3d_region_loss_fwd', E.ptr(pd), E.ptr(td), table, E.ptr(wd), E.ptr(ad), E.ptr(part.t), E.ptr(coef.t),
           E.ptr(loss.t), N, R, S, float(gamma), float(dice_weight), float(bce_weight), int(batch_dice), ignore, E.stream_ptr())
    E.call('seg3d_region_loss_bwd', E.ptr(pd), E.ptr(td), table, E.ptr(coef.t), E.ptr(ad), E.ptr(gd), E.ptr(dprobs.t), N, R, S,
           float(gamma), int(batch_dice), ignore, E.stream_ptr())
    torch.cuda.synchronize()
    for name, buf in (('part', part), ('coef', coef), ('loss', loss), ('dprobs', dprobs)):
        assert buf.guards_untouched(), name + ': the guard bands were written'
        assert buf.written(), name + ': an element was not written (or is not finite)'
    assert torch.equal(pd.cpu(), p.reshape(-1)) and torch.equal(td.cpu(), t.reshape(-1))      # the inputs are read only
    return loss.t.cpu(), dprobs.t.cpu().reshape(p.shape)


def _references(p, t, regions, gout=1.0, **opts):
    """[(terms, gradient)] of the oracle in float64 and in float32 (the yardstick)"""
    out = []
    for dtype in (F64, F32):
        pr = p.clone().requires_grad_(True)
        terms = oracle(pr, t, regions, dtype=dtype, **opts)
        (g,) = torch.autograd.grad(terms[0] * gout, pr)
        out.append((torch.stack([x.detach().double() for x in terms]), g.double()))
    return out


def _compare(name, terms, grad, p, t, regions, gout=1.0, **opts):
    (ref_terms, ref_grad), (yard_terms, yard_grad) = _references(p, t, regions, gout, **opts)
    figs, fails = {}, []
    for k, key in enumerate(('L', 'L_dice', 'L_bce')):
        err, yard = abs(float(terms[k]) - float(ref_terms[k])), abs(float(yard_terms[k]) - float(ref_terms[k]))
        bar = max(4.0 * yard, FLOOR)
        figs.update({key + '_err': err, key + '_yard': yard, key + '_bar': bar})
        if not err <= bar:
            fails.append('{}: err {:.3e} > bar {:.3e}'.format(key, err, bar))
    scale = float(ref_grad.abs().max())
    if scale == 0.0:
        if float(grad.abs().max()) != 0.0:
            fails.append('the gradient is not 0.0 where the oracle\'s is')
    else:
        err, yard = float((grad.double() - ref_grad).abs().max()) / scale, float((yard_grad - ref_grad).abs().max()) / scale
        bar = max(4.0 * yard, FLOOR)
        figs.update(grad_err=err, grad_yard=yard, grad_bar=bar, grad_scale=scale)
        if not err <= bar:
            fails.append('gradient: err {:.3e} > bar {:.3e} (relative to {:.3e})'.format(err, bar, scale))
    # exact zeros on every plane of a voxel that does not count
    _, counted = region_targets(t, regions, opts.get('ignore_label'))
    dead = (~counted).reshape((t.shape[0], 1) + tuple(t.shape[2:])).expand_as(grad)
    if bool(dead.any()) and float(grad[dead].abs().max()) != 0.0:
        fails.append('a voxel that does not count has a gradient')
    report('region_loss/' + name, **figs)
    print('region_loss/' + name, figs)
    assert not fails, '{}: {}'.format(name, '; '.join(fails))
    return figs


# ---- every shape class with every instantiation, through the C ABI ----------------------------------------------------------------
@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('R', sorted(REGIONS))
def test_abi_equals_the_oracle(hip_device, R, N, shape):
    p, t = _inputs(1000 + 10 * R + N, N, R, SHAPES[shape])
    opts = dict(ignore_label=255)
    S = _numel(SHAPES[shape])
    for tag, shift in [('', 0)] + ([('scalar_', 1)] if S % 4 == 0 else []):
        terms, grad = _abi(hip_device, p, t, REGIONS[R], shift=shift, **opts)
        _compare('{}R{}_N{}_{}'.format(tag, R, N, shape), terms, grad, p, t, REGIONS[R], **opts)


OPTIONS = {
    'batch_dice': dict(batch_dice=True),
    'no_batch_dice_weights': dict(weights=[0.2, 1.0, 3.0]),
    'dice_weight0': dict(dice_weight=0.0),
    'bce_weight0': dict(bce_weight=0.0),
    'gamma0': dict(gamma=0.0),
    'gamma1': dict(gamma=1.0),
    'gamma2': dict(gamma=2.0),
    'gamma1.5': dict(gamma=1.5),
    'ignore255': dict(ignore_label=255),
    'ignore_unlisted_id': dict(ignore_label=NOWHERE),
    'no_ignore': dict(),
    'gout': dict(gout=-2.5),
    'combined': dict(weights=[0.2, 1.0, 3.0], batch_dice=True, ignore_label=NOWHERE, gamma=1.5, dice_weight=0.7, bce_weight=1.3,
                     gout=0.3),
}


@pytest.mark.parametrize('shape', ['5x7x9', '33x32x32'])
@pytest.mark.parametrize('option', list(OPTIONS))
def test_options_equal_the_oracle(hip_device, option, shape):
    """each option alone and one combination on BraTS's regions, N = 3, on the scalar and on the 16-byte path"""
    opts = dict(OPTIONS[option])
    gout = opts.pop('gout', 1.0)
    p, t = _inputs(2000, 3, 3, SHAPES[shape])
    terms, grad = _abi(hip_device, p, t, BRATS, gout=gout, **opts)
    _compare('{}_{}'.format(option, shape), terms, grad, p, t, BRATS, gout=gout, **opts)
    if opts.get('dice_weight', 1.0) == 0.0:
        assert float(terms[0]) == float(terms[2])              # (the BCE weight of this case is 1)
        # without the Dice term nothing is left below the clamp: the planted 1e-13 / 0 / 1 probabilities on their own side
        z, _ = region_targets(t, BRATS, opts.get('ignore_label'))
        q = torch.where(z.reshape(p.shape), p, 1.0 - p)
        assert float(grad[q < 1e-12].abs().max() if bool((q < 1e-12).any()) else 0.0) == 0.0
    if opts.get('bce_weight', 1.0) == 0.0:
        assert float(terms[0]) == float(terms[1])


def test_nothing_counts(hip_device):
    """a batch whose every voxel is the ignore label or no label: L_bce = 0, L_dice = its empty value, gradient all zero"""
    p, t = _inputs(3000, 3, 3, SHAPES['5x7x9'], stray=False)
    t[:] = 255.0
    t[0, 0, 0, 0, :3] = torch.tensor([-1.0, 1.5, 300.0])
    for opts in (dict(ignore_label=255), dict(ignore_label=255, batch_dice=True, gamma=2.0)):
        terms, grad = _abi(hip_device, p, t, BRATS, **opts)
        _compare('nothing_counts', terms, grad, p, t, BRATS, **opts)
        assert float(terms[2]) == 0.0 and float(grad.abs().max()) == 0.0 and bool(torch.isfinite(terms).all())


def test_refusals(hip_device):
    E, dev = _engine(), hip_device
    from segmentation3d import _ops
    x = torch.ones(17 * 8, device=dev)
    out = {k: Guarded(n, GUARD, dev) for k, n in (('part', 64), ('coef', 64), ('loss', 3), ('dprobs', 17 * 8))}
    P, table, st = E.ptr(x), _ops._region_table([0] * 256), E.stream_ptr
    q = {k: E.ptr(g.t) for k, g in out.items()}
    for name, args in (
            ('seg3d_region_loss_fwd', (P, P, table, P, P, q['part'], q['coef'], q['loss'], 1, 17, 8, 0.0, 1.0, 1.0, 0, -1.0, st())),
            ('seg3d_region_loss_fwd', (P, P, table, P, P, q['part'], q['coef'], q['loss'], 1, 2, 8, 0.0, 0.0, 0.0, 0, -1.0, st())),
            ('seg3d_region_loss_fwd', (P, P, None, P, P, q['part'], q['coef'], q['loss'], 1, 2, 8, 0.0, 1.0, 1.0, 0, -1.0, st())),
            ('seg3d_region_loss_bwd', (P, P, table, P, P, P, q['dprobs'], 1, 0, 8, 0.0, 0, -1.0, st())),
            ('seg3d_region_loss_bwd', (P, P, table, P, P, P, q['dprobs'], 1, 2, 8, -1.0, 0, -1.0, st()))):
        with pytest.raises(ValueError) as info:
            E.call(name, *args)
        assert str(info.value).startswith(name + ':')
    torch.cuda.synchronize()
    assert all(g.all_nan() and g.guards_untouched() for g in out.values())
    with pytest.raises(ValueError):
        _ops._region_table([0] * 255)


# ---- through Python -----------------------------------------------------------------------------------------------------------
def _module(dev, p, t, regions, gout=None, **opts):
    from segmentation3d.loss.region_loss import RegionDiceBCELoss
    loss_fn = RegionDiceBCELoss(regions, **opts)
    pg = p.to(dev).requires_grad_(True)
    loss = loss_fn(pg, t.to(dev))
    (loss if gout is None else loss * gout).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), loss_fn.last_terms.detach().cpu(), pg.grad.detach().cpu()


def test_module_equals_the_abi_and_two_runs_are_bit_equal(hip_device):
    from segmentation3d.core.seg_train import build_loss
    opts = dict(weights=[0.2, 1.0, 3.0], ignore_label=255, gamma=2.0, batch_dice=True, dice_weight=0.7, bce_weight=1.3)
    p, t = _inputs(4000, 3, 3, SHAPES['33x32x32'])
    a = _module(hip_device, p, t, BRATS, gout=0.5, **opts)
    b = _module(hip_device, p, t, BRATS, gout=0.5, **opts)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and float(a[0]) == float(a[1][0])
    terms, grad = _abi(hip_device, p, t, BRATS, gout=0.5, **opts)
    assert torch.equal(terms, a[1]) and torch.equal(grad, a[2])
    _compare('module', a[1], a[2], p, t, BRATS, gout=0.5, **opts)
    # build_loss reaches the same object: focal_gamma is gamma, ce_weight the BCE weight
    loss_fn = build_loss('RegionDiceFocal', 4, [0.2, 1.0, 3.0], 2.0, regions=BRATS, ignore_label=255, batch_dice=True,
                         dice_weight=0.7, ce_weight=1.3)
    pg = p.to(hip_device).requires_grad_(True)
    (loss_fn(pg, t.to(hip_device)) * 0.5).backward()
    assert torch.equal(loss_fn.last_terms.cpu(), a[1]) and torch.equal(pg.grad.cpu(), a[2])
    # no gradient is asked for: the forward alone
    with torch.no_grad():
        assert float(loss_fn(p.to(hip_device), t.to(hip_device))) == float(a[0])


@pytest.mark.parametrize('C,shape', [(2, '5x7x9'), (4, '33x32x32'), (6, '4x4x8'), (8, '5x7x9')])
@pytest.mark.parametrize('batch_dice', [False, True])
def test_dice_term_is_the_compound_family_s(hip_device, C, shape, batch_dice):
    """regions [[1], .., [C-1]] on targets 0..C-1: L_dice on the planes 1..C-1 is the region term of
    DiceCELoss(include_background=False) on all C planes -- the same device code with one class fewer"""
    from segmentation3d.loss.compound_loss import DiceCELoss
    g = torch.Generator().manual_seed(5000 + C)
    sp = SHAPES[shape]
    p = torch.softmax(2.0 * torch.randn((3, C) + sp, generator=g), dim=1).float()
    t = torch.randint(0, C, (3, 1) + sp, generator=g).float()
    regions = [[c] for c in range(1, C)]
    sub = p[:, 1:].contiguous()
    _, terms, _ = _module(hip_device, sub, t, regions, batch_dice=batch_dice)
    ce = DiceCELoss(C, include_background=False, batch_dice=batch_dice)
    ce(p.to(hip_device), t.to(hip_device))
    family = float(ce.last_terms[1])
    ref = float(oracle(sub, t, regions, batch_dice=batch_dice)[1])
    yard = abs(float(oracle(sub, t, regions, batch_dice=batch_dice, dtype=F32)[1]) - ref)
    bar = max(4.0 * yard, FLOOR)
    figs = dict(region_err=abs(float(terms[1]) - ref), family_err=abs(family - ref), between=abs(float(terms[1]) - family),
                bar=bar, bit_equal=float(float(terms[1]) == family))
    report('region_loss/dice_vs_DiceCE_C{}_{}_{}'.format(C, shape, int(batch_dice)), **figs)
    print(figs)
    assert figs['region_err'] <= bar and figs['family_err'] <= bar and figs['between'] <= bar, figs


# ---- TrainStep ------------------------------------------------------------------------------------------------------------------
def _clear():
    """after `del step`: nothing of a TrainStep is left when the next one is built"""
    from segmentation3d import _ops
    gc.collect()
    _ops.PACK_CACHE.clear()


def _batch(dev, edge):
    g = torch.Generator().manual_seed(6000)
    t = torch.randint(0, 4, (2, 1, edge, edge, edge), generator=g).float()
    x = (t / 3.0 * 2.0 - 1.0 + 0.3 * torch.randn(t.shape, generator=g)).float()
    return x.to(dev), t.to(dev)


def _entries(monkeypatch):
    """the names of the C-ABI entries called from here on"""
    E, seen = _engine(), []
    call = E.call

    def spy(name, *args):
        seen.append(name)
        return call(name, *args)
    monkeypatch.setattr(E, 'call', spy)
    return seen


def test_train_step_eager_and_graph_print_the_same_losses(hip_device, monkeypatch):
    """vnet at the smallest crop its max_stride allows, four steps with RegionDiceBCE on BraTS's regions: the step built
    eagerly and the step captured in a hipGraph (one after the other, the cache cleared between them) print identical
    train_loss strings, and the region step launches the sigmoid head and the region loss"""
    from segmentation3d.core.seg_train import TrainStep
    from segmentation3d.loss.region_loss import RegionDiceBCELoss
    lines = {}
    for use_graph in (False, True):
        step = TrainStep('vnet', 1, 4, loss_name='RegionDiceBCE', lr=1e-3, device=hip_device, seed=3, use_graph=use_graph,
                         regions=BRATS, region_class_order=[2, 1, 3], loss_options=dict(ignore_label=255))
        assert isinstance(step.loss_func, RegionDiceBCELoss) and step.net.output_activation == 'sigmoid'
        assert step.regions == BRATS and step.region_class_order == [2, 1, 3]
        x, t = _batch(hip_device, step.max_stride)
        seen = _entries(monkeypatch) if not use_graph else []
        out = []
        for _ in range(4):
            loss = step(x, t).detach()
            terms = step.loss_func.last_terms
            assert float(terms[0]) == float(loss) and abs(float(terms[1] + terms[2]) - float(loss)) < 1e-6
            out.append('{:.4f}'.format(float(loss)))
        monkeypatch.undo()
        assert step.use_graph == use_graph and (step._graph is not None) == use_graph
        if not use_graph:
            assert {'seg3d_sigmoid_fwd', 'seg3d_sigmoid_bwd', 'seg3d_region_loss_fwd', 'seg3d_region_loss_bwd'} <= set(seen)
            assert not any('softmax' in n or 'compound' in n for n in seen)
            assert tuple(step.net(x).shape) == (2, 3, step.max_stride, step.max_stride, step.max_stride)
        lines[use_graph] = out
        del step, loss, terms
        _clear()
    report('region_loss/train_step', **{'loss_{}'.format(i): float(v) for i, v in enumerate(lines[True])})
    assert lines[False] == lines[True], lines
    assert all(0.0 < float(v) < 10.0 for v in lines[True]), lines


def test_soft_max_step_launches_what_it_launched(hip_device, monkeypatch):
    """a TrainStep without regions: the soft-max head and the compound loss, no entry of the region path"""
    from segmentation3d.core.seg_train import TrainStep
    from segmentation3d.loss.compound_loss import DiceCELoss
    step = TrainStep('vnet', 1, 4, loss_name='DiceCE', lr=1e-3, device=hip_device, seed=3)
    assert isinstance(step.loss_func, DiceCELoss) and step.net.output_activation == 'softmax' and step.regions is None
    x, t = _batch(hip_device, step.max_stride)
    seen = _entries(monkeypatch)
    step(x, t)
    monkeypatch.undo()
    assert {'seg3d_softmax_fwd', 'seg3d_softmax_bwd', 'seg3d_compound_loss_fwd', 'seg3d_compound_loss_bwd'} <= set(seen)
    assert not any('region' in n or 'sigmoid' in n for n in seen)
    del step
    _clear()


def test_train_step_refusals(hip_device):
    from segmentation3d.core.seg_train import REGION_LOSSES, TrainStep
    order = [2, 1, 3]
    for name in REGION_LOSSES:
        with pytest.raises(ValueError, match='deep supervision'):
            TrainStep('vnet', 1, 4, loss_name=name, device=hip_device, regions=BRATS, region_class_order=order, deep_supervision=2)
        with pytest.raises(ValueError, match='needs regions'):
            TrainStep('vnet', 1, 4, loss_name=name, device=hip_device)
    for name in ('Dice', 'Focal', 'CE', 'DiceCE', 'DiceFocal', 'DiceTopK', 'DiceBoundary', 'DiceClDice', 'DiceBCE'):
        with pytest.raises(ValueError, match='takes no regions'):
            TrainStep('vnet', 1, 4, loss_name=name, device=hip_device, regions=BRATS, region_class_order=order)
    with pytest.raises(ValueError, match='Unknown loss function'):
        TrainStep('vnet', 1, 4, loss_name='DiceBCE', device=hip_device)
    _clear()
