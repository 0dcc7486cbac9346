"""The soft-skeleton and Dice + clDice kernels (seg3d_soft_skeleton, seg3d_cldice_loss_fwd / _bwd) on the GPU against the
float64 oracle of tests/cldice_oracle.py; ties, run-to-run and hipGraph behaviour; training and deep supervision.

Bars.  Nothing is fixed in advance: every comparison also evaluates the oracle in stock fp32 on the CPU on the same inputs,
and the device's error against float64 may be at most 4 x that fp32 error (the margin is for the different order of the
sums), but never has to be below 1e-6, the project's usual bar.  This holds for the absolute error of the three loss terms
and for gpu_util.rel_err of the gradient.  A 0 / 1 volume must give the oracle's skeleton exactly: every stage is a
selection or an exact operation on 0 and 1.
Gradient comparisons use planes whose values are pairwise distinct (a smoothed random field, rank-transformed to
(rank + 1) / (S + 1)): then the gradient does not depend on which of several equal positions a min or max picks.  Ties are
checked on values only.
The kernels' tile is 32 x 8 x 8 (x, y, z): the spatial shape (10, 11, 37) spans two tiles with a remainder on every axis.
Measured on the MI355X over this file's cases: skeleton within 7.1e-8 of float64 (the fp32 oracle: 7.1e-8), 0 / 1 masks exact;
loss terms within 7.4e-8 (fp32 oracle: up to 1.6e-7); rel_err(dprobs) <= 2.8e-7 (fp32 oracle: up to 3.4e-7); eager and captured
train steps bit-equal.  DESIGN.md section 7, row f17."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO  # noqa: F401
from cldice_oracle import cldice_oracle, soft_skeleton_oracle
from gpu_util import max_err, rel_err, report
from oracle import detgen

pytestmark = pytest.mark.gpu

FLOOR = 1e-6
MARGIN = 4.0
TWO_TILES = (10, 11, 37)
SKEL_SHAPES = [(1, 1, 1), (1, 1, 5), (3, 3, 3), (7, 9, 13), TWO_TILES]   # (Z, Y, X)


def _bar(fp32_err):
    return max(MARGIN * fp32_err, FLOOR)


def _ranked_planes(seed, planes, spatial):
    """[planes, Z, Y, X] float32: per plane a smoothed random field, rank-transformed to (rank + 1) / (S + 1) -- pairwise
    distinct, blob-like, no denormal differences"""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((planes, 1) + tuple(spatial), generator=g, dtype=torch.float64)
    for _ in range(2):
        f = F.avg_pool3d(F.pad(f, (1, 1, 1, 1, 1, 1), mode='replicate'), 3, 1)
    f = f.reshape(planes, -1) + 1e-9 * torch.randn((planes, f[0].numel()), generator=g, dtype=torch.float64)
    S = f.shape[1]
    rank = f.argsort(dim=1).argsort(dim=1).double()
    x = ((rank + 1.0) / (S + 1.0)).float()
    for k in range(planes):
        assert len(np.unique(x[k].numpy())) == S                     # pairwise distinct in fp32
    return x.reshape((planes,) + tuple(spatial))


def _blob_labels(seed, N, C, spatial):
    """[N, 1, Z, Y, X] float class ids: the arg-max of C smoothed random fields"""
    f = _ranked_planes(seed, N * C, spatial).reshape((N, C) + tuple(spatial))
    return f.argmax(dim=1, keepdim=True).float()


# ---- the skeleton -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _skeleton_case(shape, iters):
    x = _ranked_planes(11 + iters, 2, shape)
    mask = (_ranked_planes(29 + iters, 2, shape) > 0.45).float()
    with torch.no_grad():
        return (x, soft_skeleton_oracle(x.double(), iters), soft_skeleton_oracle(x, iters), mask,
                soft_skeleton_oracle(mask.double(), iters))


@pytest.mark.parametrize('iters', [1, 3, 16])
@pytest.mark.parametrize('shape', SKEL_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_soft_skeleton_equals_the_oracle(hip_device, shape, iters):
    """two pairwise-distinct planes and two binary masks per shape.
    Measured on the MI355X: largest error 7.1e-8 (k = 16 at 10 x 11 x 37), the fp32 oracle's own 7.1e-8; masks exact."""
    from segmentation3d.utils import image_tools
    x, ref, ref32, mask, mask_ref = _skeleton_case(shape, iters)
    got = image_tools.soft_skeleton_device(x.to(hip_device), iters)
    got_mask = image_tools.soft_skeleton_device(mask.to(hip_device), iters)
    torch.cuda.synchronize()
    assert got.shape == x.shape and got.dtype == torch.float32
    fp32 = max_err(ref32, ref)
    err = max_err(got, ref)
    name = 'skel_{}_k{}'.format('x'.join(str(v) for v in shape), iters)
    report(name, err=err, fp32=fp32)
    print(name, err, fp32)
    assert err <= _bar(fp32), (err, fp32)
    assert torch.equal(got_mask.cpu().double(), mask_ref)            # exact on 0 / 1
    if min(shape) >= 7 and iters >= 3:
        assert float((ref > 0).double().mean()) >= 0.10              # a kernel returning zeros cannot pass


def test_soft_skeleton_wrapper_shapes_and_refusals(hip_device):
    from segmentation3d import _ops
    from segmentation3d.utils import image_tools
    x, ref, _, _, _ = _skeleton_case((7, 9, 13), 3)
    one = image_tools.soft_skeleton_device(x[0].to(hip_device), 3)                       # [Z, Y, X]
    batch = image_tools.soft_skeleton_device(x.reshape(1, 2, 7, 9, 13).to(hip_device), 3)  # [N, K, Z, Y, X]
    torch.cuda.synchronize()
    assert one.shape == (7, 9, 13) and batch.shape == (1, 2, 7, 9, 13)
    assert torch.equal(one.cpu(), batch[0, 0].cpu()) and max_err(batch[0], ref) <= FLOOR
    for bad in (0, 17):
        with pytest.raises(ValueError):
            _ops.soft_skeleton(x.to(hip_device), bad)
    with pytest.raises(ValueError):
        _ops.soft_skeleton(torch.zeros(1, 1, 257, device=hip_device), 1)
    with pytest.raises(ValueError):
        _ops.soft_skeleton(torch.zeros(4, 4, device=hip_device), 1)


# ---- loss and gradient ------------------------------------------------------------------------------------------------
def _inputs(seed, N, C, spatial, slab=False, out_of_range=False):
    """p [N, C, Z, Y, X] pairwise distinct per plane, blob labels t [N, 1, Z, Y, X]; slab: an ignored slab of label 255
    across z; out_of_range: ids C, -1 and 1000 sprinkled in"""
    p = _ranked_planes(seed, N * C, spatial).reshape((N, C) + tuple(spatial))
    t = _blob_labels(seed + 1, N, C, spatial)
    if slab:
        z = spatial[0]
        t[:, :, z // 2:z // 2 + max(1, z // 5)] = 255.0
    if out_of_range:
        r = torch.rand(t.shape, generator=torch.Generator().manual_seed(seed + 2))
        t[r < 0.05] = float(C)
        t[(r >= 0.05) & (r < 0.10)] = -1.0
        t[(r >= 0.10) & (r < 0.13)] = 1000.0
    return p, t


def _gpu(dev, p, t, C, **opts):
    from segmentation3d.loss.cldice_loss import DiceClDiceLoss
    loss_fn = DiceClDiceLoss(C, **opts)
    pg = p.to(dev).requires_grad_(True)
    loss = loss_fn(pg, t.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), loss_fn.last_terms.detach().cpu(), pg.grad.detach().cpu()


def _oracle(p, t, dtype, want_grad, **opts):
    pr = p.clone().to(dtype).requires_grad_(want_grad)
    ref = cldice_oracle(pr, t, dtype=dtype, skeletons=True, **opts)
    grad = torch.autograd.grad(ref[0], pr)[0].double() if want_grad else None
    return [float(r.detach()) for r in ref[:3]], grad, ref[3].detach()


def _dead(t, C, ignore):
    valid = (t >= 0) & (t < C)
    if ignore is not None:
        valid = valid & (t != float(ignore))
    return (~valid).expand(-1, C, -1, -1, -1)


def _check(name, dev, p, t, C, gradient=True, skeleton_share=0.10, **opts):
    """the device against float64, under 4 x the error of the same arithmetic in stock fp32 (at least 1e-6)"""
    loss, terms, grad = _gpu(dev, p, t, C, **opts)
    ref, ref_grad, sp = _oracle(p, t, torch.float64, gradient, **opts)
    ref32, ref32_grad, _ = _oracle(p, t, torch.float32, gradient, **opts)
    if skeleton_share:
        assert float((sp > 0).double().mean()) >= skeleton_share     # a kernel returning zeros cannot pass
    errs, bars = {}, {}
    for i, key in enumerate(('loss', 'dice', 'cl')):
        errs[key] = abs(float(terms[i]) - ref[i])
        bars[key] = _bar(abs(ref32[i] - ref[i]))
    if gradient:
        errs['dprobs_rel'] = rel_err(grad, ref_grad)
        bars['dprobs_rel'] = _bar(rel_err(ref32_grad, ref_grad))
    report('cldice_' + name, **errs, **{'fp32_' + k: (v / MARGIN if v > FLOOR else 0.0) for k, v in bars.items()})
    print('cldice_' + name, errs, bars)
    assert float(loss) == float(terms[0])
    assert torch.isfinite(terms).all() and torch.isfinite(grad).all()
    for key in errs:
        assert errs[key] <= bars[key], (key, errs, bars)
    dead = _dead(t, C, opts.get('ignore_label'))
    if bool(dead.any()):
        assert float(grad[dead].abs().max()) == 0.0                  # exact zeros on voxels that do not count
    return loss, terms, grad


WEIGHTS = [0.2, 1.0, 3.0, 0.5, 2.0]
SUBSET = {2: [1], 3: [2], 5: [3, 1]}
OPTIONS = {
    'default': dict(),
    'weights': dict(weights=WEIGHTS),
    'batch_dice': dict(batch_dice=True),
    'no_background': dict(include_background=False),
    'ignore255': dict(ignore_label=255),
    'out_of_range': dict(),
    'subset': dict(),
    'cl_only': dict(dice_weight=0.0, cldice_weight=1.0),
    'iters1': dict(iters=1),
    'combined': dict(weights=WEIGHTS, include_background=False, batch_dice=True, ignore_label=255, dice_weight=0.7,
                     cldice_weight=0.3, iters=5),
}


@pytest.mark.parametrize('C', [2, 3, 5])
@pytest.mark.parametrize('option', list(OPTIONS))
def test_loss_and_gradient_equal_the_oracle(hip_device, option, C):
    """2 x C x 10 x 11 x 37 (two tiles with a remainder on every axis), each option alone and one combination.
    Measured on the MI355X: terms within 7.4e-8 of float64, rel_err(dprobs) <= 2.8e-7 (bars 1.0e-6 to 1.4e-6)."""
    opts = dict(OPTIONS[option])
    if 'weights' in opts:
        opts['weights'] = opts['weights'][:C]
    if option in ('subset', 'combined'):
        opts['cldice_classes'] = SUBSET[C]
    p, t = _inputs(100 + C, 2, C, TWO_TILES, slab=opts.get('ignore_label') is not None,
                   out_of_range=option in ('out_of_range', 'combined'))
    _, _, grad = _check('{}_C{}'.format(option, C), hip_device, p, t, C, **opts)
    if opts.get('dice_weight', 1.0) == 0.0:
        assert float(grad[:, 0].abs().max()) == 0.0                  # the background is in no clDice class list
        assert float(grad[:, 1:].abs().max()) > 0.0


def test_generic_class_count(hip_device):
    """C = 7 takes the kernels' generic (16-class) instantiation; classes 6 and 2 of it"""
    p, t = _inputs(160, 1, 7, (7, 9, 13))
    _check('generic_C7', hip_device, p, t, 7, cldice_classes=[6, 2], iters=2)


@pytest.mark.parametrize('shape', [(5, 7, 9), (16, 20, 24)], ids=['scalar', 'vec'])
def test_without_the_cldice_term_it_is_dicece_without_the_ce_term(hip_device, shape):
    """cldice_weight = 0 against DiceCELoss(ce_weight=0): the same bits in the loss and in the gradient"""
    from segmentation3d.loss.compound_loss import DiceCELoss
    C = 3
    p, t = _inputs(200, 2, C, shape, slab=True)
    opts = dict(weights=[0.2, 1.0, 3.0], ignore_label=255, dice_weight=0.8)
    loss, terms, grad = _gpu(hip_device, p, t, C, cldice_weight=0.0, **opts)
    ce = DiceCELoss(C, ce_weight=0.0, **opts)
    pg = p.to(hip_device).requires_grad_(True)
    ce_loss = ce(pg, t.to(hip_device))
    ce_loss.backward()
    torch.cuda.synchronize()
    assert np.float32(float(loss)).tobytes() == np.float32(float(ce_loss.detach())).tobytes()
    assert np.float32(float(terms[1])).tobytes() == np.float32(float(ce.last_terms[1])).tobytes()
    assert torch.equal(grad.view(torch.int32), pg.grad.cpu().view(torch.int32))
    ref, _, _ = _oracle(p, t, torch.float64, False, cldice_weight=0.0, **opts)
    assert abs(float(terms[2]) - ref[2]) <= FLOOR                    # the term is still reported


# ---- ties: values only --------------------------------------------------------------------------------------------------
def _tie_cases(C, spatial):
    t = _blob_labels(300, 2, C, spatial)
    other = _blob_labels(301, 2, C, spatial)
    onehot = lambda lab: torch.cat([(lab == c).float() for c in range(C)], dim=1)   # noqa: E731
    return {'saturated': (onehot(other), t), 'constant': (torch.full((2, C) + tuple(spatial), 1.0 / C), t),
            'one_hot_of_t': (onehot(t), t)}


@pytest.mark.parametrize('case', ['saturated', 'constant', 'one_hot_of_t'])
def test_ties_give_the_oracles_values_and_a_finite_gradient(hip_device, case):
    """saturated 0 / 1 probabilities, constant planes, p == one-hot(t): the three terms within the bar, the gradient
    finite (its value depends on the selection rule), L_cl within the bar of 0 for p == one-hot(t)"""
    C = 3
    p, t = _tie_cases(C, TWO_TILES)[case]
    for opts in (dict(), dict(batch_dice=True, iters=2)):
        _, terms, _ = _check('ties_' + case, hip_device, p, t, C, gradient=False, skeleton_share=0.0, **opts)
        if case == 'one_hot_of_t':
            assert abs(float(terms[2])) <= FLOOR


def test_nothing_counted(hip_device):
    """a sample with nothing counted inside a batch, then a batch with nothing counted: L_cl = 0, zero gradient, no NaN"""
    C = 3
    p, t = _inputs(400, 2, C, (7, 9, 13))
    t[1] = 255.0
    for opts in (dict(ignore_label=255), dict(ignore_label=255, batch_dice=True)):
        _, _, grad = _check('one_sample_ignored', hip_device, p, t, C, skeleton_share=0.0, **opts)
        assert float(grad[1].abs().max()) == 0.0
    t[:] = 255.0
    for opts in (dict(ignore_label=255), dict(ignore_label=255, batch_dice=True, include_background=False)):
        loss, terms, grad = _gpu(hip_device, p, t, C, **opts)
        assert torch.isfinite(terms).all() and torch.isfinite(grad).all()
        assert float(terms[2]) == 0.0 and abs(float(terms[1])) < 1e-6 and abs(float(loss)) < 1e-6
        assert float(grad.abs().max()) == 0.0


# ---- contracts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('opts', [dict(), dict(weights=[0.2, 1.0, 3.0], include_background=False, batch_dice=True,
                                               ignore_label=255)], ids=['default', 'options'])
@pytest.mark.parametrize('shape', [(5, 7, 9), (16, 20, 24)], ids=['scalar', 'vec'])
def test_dice_term_is_bit_equal_to_dicece(hip_device, shape, opts):
    """last_terms[1] comes from the compound loss's device code in the compound loss's order of additions (scalar path,
    and the 16-byte path over more than one workgroup per sample)"""
    from segmentation3d.loss.compound_loss import DiceCELoss
    C = 3
    p, t = _inputs(600, 2, C, shape, slab='ignore_label' in opts)
    _, terms, _ = _gpu(hip_device, p, t, C, **opts)
    ce = DiceCELoss(C, **opts)
    ce(p.to(hip_device), t.to(hip_device))
    torch.cuda.synchronize()
    assert np.float32(float(terms[1])).tobytes() == np.float32(float(ce.last_terms[1])).tobytes()


def test_two_runs_and_graph_replay_are_bit_equal(hip_device):
    """two eager runs agree bit for bit; ONE captured graph replayed on new contents gives the bits of an eager call on the
    same contents"""
    from segmentation3d.loss.cldice_loss import DiceClDiceLoss
    C = 3
    opts = dict(weights=[0.2, 1.0, 3.0], ignore_label=255)
    first = _inputs(700, 2, C, TWO_TILES, slab=True)
    second = _inputs(710, 2, C, TWO_TILES, slab=True, out_of_range=True)
    a = _gpu(hip_device, first[0], first[1], C, **opts)
    b = _gpu(hip_device, first[0], first[1], C, **opts)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
    want = _gpu(hip_device, second[0], second[1], C, **opts)

    loss_fn = DiceClDiceLoss(C, **opts)
    pg = first[0].to(hip_device).requires_grad_(True)
    tg = first[1].to(hip_device)

    def step():
        pg.grad = None
        loss = loss_fn(pg, tg)
        loss.backward()
        return loss

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):          # warm-up on the side stream, as torch.cuda.graph expects
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    terms, grad = loss_fn.last_terms, pg.grad
    for contents, ref in ((first, a), (second, want), (first, a)):
        with torch.no_grad():
            pg.copy_(contents[0])
            tg.copy_(contents[1])
            grad.zero_()
            terms.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(terms.cpu(), ref[1]) and torch.equal(grad.cpu().view(torch.int32), ref[2].view(torch.int32))
        assert float(loss.detach()) == float(ref[0])


# ---- training -----------------------------------------------------------------------------------------------------------
def test_train_step_eager_and_graph_agree(hip_device):
    """TrainStep('vnet', 1, 2, loss_name='DiceClDice') on 2 x 32^3 for three steps, eager and with the whole step in one
    hipGraph: finite losses, terms[0] == loss, equal losses and the same parameters afterwards (the DiceCE train-step
    test's tolerance, 1e-6)."""
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import TrainStep
    from segmentation3d.loss.cldice_loss import DiceClDiceLoss
    t = detgen.labels(700, 'cl/t', (2, 1, 32, 32, 32), 2).astype(np.float32)
    x = (t * 2.0 - 1.0 + 0.3 * detgen.normal(701, 'cl/x', (2, 1, 32, 32, 32))).astype(np.float32)
    x, t = torch.from_numpy(x).to(hip_device), torch.from_numpy(t).to(hip_device)
    params, runs = {}, {}
    for use_graph in (False, True):
        step = TrainStep('vnet', 1, 2, loss_name='DiceClDice', lr=1e-3, device=hip_device, seed=3, use_graph=use_graph,
                         loss_options={'cldice_weight': 0.5, 'cldice_iters': 2})
        assert isinstance(step.loss_func, DiceClDiceLoss) and step.loss_func.iters == 2
        losses = []
        for _ in range(3):
            loss = step(x, t)
            terms = step.loss_func.last_terms
            losses.append(float(loss))
            assert float(terms[0]) == float(loss)
        torch.cuda.synchronize()
        assert step.use_graph == use_graph and (step._graph is not None) == use_graph
        assert all(np.isfinite(losses)), losses
        runs[use_graph] = losses
        params[use_graph] = [q.detach().cpu().clone() for q in step.net.parameters()]
        report('cldice_train_{}'.format('graph' if use_graph else 'eager'), **{'loss_{}'.format(i): v for i, v in enumerate(losses)})
        _ops.PACK_CACHE.clear()
    diff = max(float((a - b).abs().max()) for a, b in zip(params[False], params[True]))
    ldiff = max(abs(a - b) for a, b in zip(runs[False], runs[True]))
    report('cldice_train_eager_vs_graph', max_param_diff=diff, max_loss_diff=ldiff)
    print('cldice_train_eager_vs_graph', diff, ldiff)
    assert diff < 1e-6 and ldiff < 1e-6, (diff, ldiff)


def test_deep_supervision_calls_one_object_at_two_resolutions(hip_device):
    """DeepSupervisionLoss(DiceClDiceLoss, levels=1): both levels' forwards run before any backward; the combined loss and
    both gradients against the oracle applied per level"""
    from segmentation3d.loss.cldice_loss import DiceClDiceLoss
    from segmentation3d.loss.deep_supervision_loss import DeepSupervisionLoss
    C, N = 3, 2
    opts = dict(ignore_label=255, iters=2)
    p0, t = _inputs(900, N, C, (12, 16, 40), slab=True)
    p1, _ = _inputs(905, N, C, (6, 8, 20))
    levels_t = [t, t[:, :, ::2, ::2, ::2].contiguous()]
    w = [2.0 / 3.0, 1.0 / 3.0]
    loss_fn = DeepSupervisionLoss(DiceClDiceLoss(C, **opts), 1)
    g0, g1 = p0.to(hip_device).requires_grad_(True), p1.to(hip_device).requires_grad_(True)
    loss = loss_fn([g0, g1], t.to(hip_device))
    loss.backward()
    torch.cuda.synchronize()
    total, total32 = 0.0, 0.0
    for k, (p, tk, g) in enumerate(zip((p0, p1), levels_t, (g0, g1))):
        ref, ref_grad, _ = _oracle(p, tk, torch.float64, True, **opts)
        ref32, ref32_grad, _ = _oracle(p, tk, torch.float32, True, **opts)
        total, total32 = total + w[k] * ref[0], total32 + w[k] * ref32[0]
        assert abs(float(loss_fn.last_levels[k]) - ref[0]) <= _bar(abs(ref32[0] - ref[0]))
        err, bar = rel_err(g.grad.cpu() / w[k], ref_grad), _bar(rel_err(ref32_grad, ref_grad))
        report('cldice_deep_level{}'.format(k), dprobs_rel=err, fp32=bar / MARGIN if bar > FLOOR else 0.0)
        assert err <= bar, (k, err, bar)
    assert abs(float(loss) - total) <= _bar(abs(total32 - total))


def test_validator_with_a_second_loss_object_next_to_a_captured_step(hip_device):
    """a captured TrainStep('DiceClDice') and a Validator whose loss is a second object built from the same options: the
    validation loss is that loss on the network's own output, the train step's `.last_terms` stays the train step's, and
    the captured step goes on afterwards"""
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import TrainStep, build_loss
    from segmentation3d.core.seg_validate import Validator
    t = detgen.labels(720, 'clv/t', (2, 1, 32, 32, 32), 2).astype(np.float32)
    x = (t * 2.0 - 1.0 + 0.3 * detgen.normal(721, 'clv/x', (2, 1, 32, 32, 32))).astype(np.float32)
    x, t = torch.from_numpy(x).to(hip_device), torch.from_numpy(t).to(hip_device)
    options = {'cldice_weight': 0.5, 'cldice_iters': 2}
    step = TrainStep('vnet', 1, 2, loss_name='DiceClDice', lr=1e-3, device=hip_device, seed=3, use_graph=True,
                     loss_options=options)
    for _ in range(3):
        step(x, t)
    torch.cuda.synchronize()
    assert step._graph is not None
    kept = step.loss_func.last_terms.clone()
    validator = Validator(step.net, build_loss('DiceClDice', 2, None, 2, **options), x, t, batchsize=2)
    result = validator.run(epoch=0)
    with torch.no_grad():
        direct = build_loss('DiceClDice', 2, None, 2, **options)(step.net(x), t)
    torch.cuda.synchronize()
    assert np.isfinite(result['val_loss']) and abs(result['val_loss'] - float(direct)) < 1e-6
    assert validator.loss_func is not step.loss_func and torch.equal(step.loss_func.last_terms, kept)
    loss = step(x, t)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and float(step.loss_func.last_terms[0]) == float(loss)
    _ops.PACK_CACHE.clear()
