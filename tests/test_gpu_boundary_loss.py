"""The signed-distance and boundary-loss kernels (seg3d_signed_distance, seg3d_boundary_loss_fwd / _bwd) on the GPU
against the float64 oracle of tests/boundary_oracle.py; run-to-run and hipGraph behaviour; the weight schedule; training.

Bars.  Distance map, unit spacing: the squared distances are integers below 2^24, so round(phi^2) must be the exact integer,
|phi| within 1 ulp (fp32) of its root, signs and zeros exact.  Anisotropic spacing: relative error at most 1e-6 -- three
products and two sums in fp32 bound the error of d^2 by about 2e-7, the root halves it and adds one rounding (about 5x
margin).  Loss: the terms within 1e-4 (the bar of tests/test_gpu_compound_loss.py), scaled by max(1, mean |phi|) for L and
L_boundary, which are not O(1); the gradient within gpu_util.rel_err < 1e-4; exact zeros where the definition says zero.
Measured on the MI355X: see each test's docstring and DESIGN.md section 7, row f16."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
from boundary_oracle import boundary_oracle, signed_distance_oracle
from gpu_util import rel_err, report
from oracle import detgen

pytestmark = pytest.mark.gpu

# (X, Y, Z); the last one has the longest y line there is (the largest LDS tile of the strided pass)
MAP_SHAPES = [(1, 1, 1), (9, 7, 5), (65, 3, 2), (4, 5, 130), (256, 2, 1), (3, 256, 2)]
SPACINGS = [(1.0, 1.0, 1.0), (0.7, 1.3, 2.5)]
# class list -> (ids, number of label values)
CLASS_LISTS = {1: ([1], 3), 3: ([2, 0, 5], 6), 16: (list(range(16)), 16)}
MAP_CASES = ['random', 'single_voxel', 'empty', 'everything', 'ignore_wall', 'out_of_range']


def _labels(case, shape, ids, nlab, seed):
    """t [2, Z, Y, X] float32, ignore label (or None)"""
    X, Y, Z = shape
    rng = np.random.RandomState(seed)
    c = ids[0]
    other = [v for v in range(nlab) if v != c]
    ignore = None
    if case == 'random':
        t = rng.randint(0, nlab, size=(2, Z, Y, X))
    elif case == 'single_voxel':
        t = np.full((2, Z, Y, X), other[0])
        t[0, Z // 2, Y // 2, X // 3] = c
        t[1, Z - 1, 0, X - 1] = c
    elif case == 'empty':
        t = np.asarray(other)[rng.randint(0, len(other), size=(2, Z, Y, X))]
    elif case == 'everything':
        t = np.full((2, Z, Y, X), c)
        t[1] = rng.randint(0, nlab, size=(Z, Y, X))                 # the second sample keeps the batch index honest
    elif case == 'ignore_wall':
        # G on one side, H on the other, a wall of the ignore label between them along the longest axis
        t = np.full((2, Z, Y, X), other[0])
        ax = int(np.argmax((Z, Y, X)))
        n = (Z, Y, X)[ax]
        sl = [slice(None)] * 3
        sl[ax] = slice(0, n // 3)
        t[(slice(None),) + tuple(sl)] = c
        sl[ax] = slice(n // 3, max(n // 3 + 1, n // 2))
        t[(slice(None),) + tuple(sl)] = 255
        ignore = 255
    else:
        t = rng.randint(0, nlab, size=(2, Z, Y, X))
        r = rng.rand(2, Z, Y, X)
        t[r < 0.1] = nlab
        t[(r >= 0.1) & (r < 0.2)] = -1
        t[(r >= 0.2) & (r < 0.25)] = 1000
    return t.astype(np.float32), ignore


@functools.lru_cache(maxsize=None)
def _map_case(case, shape, nids, spacing):
    """labels and the float64 oracle, computed once per case"""
    ids, nlab = CLASS_LISTS[nids]
    t, ignore = _labels(case, shape, ids, nlab, 1000 + 7 * MAP_CASES.index(case) + nids)
    phi, d2 = signed_distance_oracle(t, ids, spacing, num_class=nlab, ignore_label=ignore, squared=True)
    return t, ignore, phi, d2


@pytest.mark.parametrize('nids', list(CLASS_LISTS))
@pytest.mark.parametrize('spacing', SPACINGS, ids=['unit', 'aniso'])
@pytest.mark.parametrize('shape', MAP_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_signed_distance_equals_the_oracle(hip_device, shape, spacing, nids):
    """every case (random labels, one voxel of G, G empty, G everything, an ignored wall, out-of-range ids), N = 2.
    Measured on the MI355X: unit spacing exact (round(phi^2) the integer, |phi| 0 ulp off the rounded root); anisotropic
    spacing: largest relative error 9.5e-8."""
    from segmentation3d import _ops
    ids, nlab = CLASS_LISTS[nids]
    worst = 0.0
    for case in MAP_CASES:
        t, ignore, ref, d2 = _map_case(case, shape, nids, spacing)
        phi = _ops.signed_distance(torch.from_numpy(t).to(hip_device), ids, spacing, ignore, num_class=nlab)
        torch.cuda.synchronize()
        assert phi.shape == ref.shape and phi.dtype == torch.float32
        got = phi.cpu().numpy()
        assert np.isfinite(got).all(), case
        assert np.array_equal(np.sign(got), np.sign(ref)), case            # signs and zeros are exact
        g64 = got.astype(np.float64)
        if spacing == (1.0, 1.0, 1.0):
            assert np.array_equal(np.rint(g64 * g64), d2), case
            root = np.sqrt(d2).astype(np.float32)
            ulps = np.abs(np.abs(got) - root) / np.spacing(np.maximum(root, np.float32(1e-30)))
            assert float(ulps.max()) <= 1.0, (case, float(ulps.max()))
            worst = max(worst, float(ulps.max()))
        else:
            nz = ref != 0
            err = float((np.abs(g64 - ref)[nz] / np.abs(ref)[nz]).max()) if nz.any() else 0.0
            assert err <= 1e-6, (case, err)
            worst = max(worst, err)
    name = 'sdf_{}_{}_K{}'.format('x'.join(str(v) for v in shape), 'unit' if spacing[0] == 1.0 else 'aniso', nids)
    report(name, worst=worst)
    print(name, worst)


def test_signed_distance_wrapper_and_refusals(hip_device):
    """image_tools.signed_distance_device on an unbatched integer volume; bad arguments raise"""
    from segmentation3d import _ops
    from segmentation3d.utils import image_tools
    t, _, ref, _ = _map_case('random', (9, 7, 5), 3, (0.7, 1.3, 2.5))
    lab = torch.from_numpy(t[0]).to(torch.int16).to(hip_device)
    phi = image_tools.signed_distance_device(lab, [2, 0, 5], (0.7, 1.3, 2.5))
    assert phi.shape == (3, 5, 7, 9)
    assert rel_err(phi, ref[0]) < 1e-6
    dev_t = torch.from_numpy(t).to(hip_device)
    with pytest.raises(ValueError):
        _ops.signed_distance(dev_t, [], (1, 1, 1), None)
    with pytest.raises(ValueError):
        _ops.signed_distance(dev_t, list(range(17)), (1, 1, 1), None)
    with pytest.raises(ValueError):
        _ops.signed_distance(dev_t, [1], (1, 0, 1), None)
    with pytest.raises(ValueError):
        _ops.signed_distance(torch.zeros(1, 1, 1, 257, device=hip_device), [1], (1, 1, 1), None)


# ---- loss and gradient ------------------------------------------------------------------------------------------------
def _inputs(seed, shape, C, ignore_frac=0.0):
    g = torch.Generator().manual_seed(seed)
    N, sp = shape[0], tuple(shape[1:])
    p = torch.softmax(2.0 * torch.randn((N, C) + sp, generator=g), dim=1).float()
    t = torch.randint(0, C, (N, 1) + sp, generator=g).float()
    if ignore_frac > 0.0:
        t[torch.rand(t.shape, generator=g) < ignore_frac] = 255.0
    return p, t


def _gpu(dev, p, t, C, **opts):
    from segmentation3d.loss.boundary_loss import DiceBoundaryLoss
    loss_fn = DiceBoundaryLoss(C, **opts)
    pg = p.to(dev).requires_grad_(True)
    loss = loss_fn(pg, t.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), loss_fn.last_terms.detach().cpu(), pg.grad.detach().cpu()


def _kernel_phi(dev, t, C, opts):
    from segmentation3d import _ops
    ids = list(range(C)) if opts.get('include_background', True) else list(range(1, C))
    phi = _ops.signed_distance(t.to(dev), ids, opts.get('spacing', (1, 1, 1)), opts.get('ignore_label'), num_class=C)
    torch.cuda.synchronize()
    return phi.cpu()


def _check(name, dev, p, t, C, **opts):
    loss, terms, grad = _gpu(dev, p, t, C, **opts)
    phi = _kernel_phi(dev, t, C, opts)                  # the kernel's own fp32 map: the reduction is judged on its own
    oopts = {k: v for k, v in opts.items() if k != 'spacing'}
    pr = p.clone().requires_grad_(True)
    ref = boundary_oracle(pr, t, phi.numpy(), **oopts)
    (ref_grad,) = torch.autograd.grad(ref[0], pr)
    ref = [r.detach() for r in ref]
    scale = max(1.0, float(phi.abs().mean()))
    errs = {'loss': abs(float(terms[0]) - float(ref[0])) / scale, 'region': abs(float(terms[1]) - float(ref[1])),
            'boundary': abs(float(terms[2]) - float(ref[2])) / scale, 'dprobs_rel': rel_err(grad, ref_grad)}
    report('boundary_' + name, **errs)
    print('boundary_' + name, errs)
    assert float(loss) == float(terms[0])
    assert torch.isfinite(terms).all() and torch.isfinite(grad).all()
    assert errs['loss'] < 1e-4 and errs['region'] < 1e-4 and errs['boundary'] < 1e-4, errs
    assert errs['dprobs_rel'] < 1e-4, errs
    ign = opts.get('ignore_label')
    valid = (t >= 0) & (t < C)
    if ign is not None:
        valid = valid & (t != float(ign))
    dead = (~valid).expand(-1, C, *([-1] * (t.dim() - 2)))
    if bool(dead.any()):
        assert float(grad[dead].abs().max()) == 0.0     # exact zeros on voxels that do not count
    return loss, terms, grad


OPTIONS = {
    'default': dict(),
    'aniso': dict(spacing=(0.7, 1.3, 2.5)),
    'no_background': dict(include_background=False, spacing=(0.7, 1.3, 2.5)),
    'batch_dice': dict(batch_dice=True),
    'weights': dict(weights=[0.2, 1.0, 3.0, 0.5, 2.0]),
    'ignore255': dict(ignore_label=255, spacing=(0.7, 1.3, 2.5)),
    'boundary_only': dict(dice_weight=0.0, boundary_weight=1.0, spacing=(0.7, 1.3, 2.5)),
    'combined': dict(weights=[0.2, 1.0, 3.0, 0.5, 2.0], include_background=False, batch_dice=True, ignore_label=255,
                     dice_weight=0.7, boundary_weight=0.3, spacing=(0.7, 1.3, 2.5)),
}


@pytest.mark.parametrize('C', [2, 3, 5])
@pytest.mark.parametrize('option', list(OPTIONS))
def test_loss_and_gradient_equal_the_oracle(hip_device, option, C):
    """2 x C x 5 x 7 x 9, each option alone and one combination.
    Measured on the MI355X over this file's cases: terms within 4.6e-8 of the oracle (scaled), rel_err(dprobs) <= 1.1e-7."""
    opts = dict(OPTIONS[option])
    if 'weights' in opts:
        opts['weights'] = opts['weights'][:C]
    p, t = _inputs(100 + C, (2, 5, 7, 9), C, ignore_frac=0.15 if opts.get('ignore_label') is not None else 0.0)
    _, _, grad = _check('{}_C{}'.format(option, C), hip_device, p, t, C, **opts)
    if opts.get('dice_weight', 1.0) == 0.0 and not opts.get('include_background', True):
        assert float(grad[:, 0].abs().max()) == 0.0


def test_boundary_only_without_background_leaves_plane_zero_untouched(hip_device):
    p, t = _inputs(150, (2, 5, 7, 9), 3)
    _, _, grad = _check('boundary_only_nobg', hip_device, p, t, 3, dice_weight=0.0, boundary_weight=1.0,
                        include_background=False)
    assert float(grad[:, 0].abs().max()) == 0.0 and float(grad[:, 1:].abs().max()) > 0.0


def test_one_voxel(hip_device):
    """1 x 2 x 1 x 1 x 1: H is empty for the voxel's class and G for the other: phi = 0, L_boundary = 0"""
    p = torch.tensor([0.3, 0.7]).reshape(1, 2, 1, 1, 1)
    t = torch.ones(1, 1, 1, 1, 1)
    _, terms, _ = _check('one_voxel', hip_device, p, t, 2)
    assert float(terms[2]) == 0.0


def test_pass_cases_give_no_nan(hip_device):
    """a sample with nothing counted inside a batch, and a batch with nothing counted: finite, L_boundary == 0 where the
    definition says so, zero gradient on everything that does not count"""
    C = 3
    p, t = _inputs(500, (2, 5, 7, 9), C)
    t[1] = 255.0
    for opts in (dict(ignore_label=255), dict(ignore_label=255, batch_dice=True, spacing=(0.7, 1.3, 2.5))):
        _, _, grad = _check('one_sample_ignored', hip_device, p, t, C, **opts)
        assert float(grad[1].abs().max()) == 0.0
    t[:] = 255.0
    for opts in (dict(ignore_label=255), dict(ignore_label=255, batch_dice=True, include_background=False)):
        loss, terms, grad = _gpu(hip_device, p, t, C, **opts)
        assert torch.isfinite(terms).all() and torch.isfinite(grad).all()
        assert float(terms[2]) == 0.0 and abs(float(terms[1])) < 1e-6 and abs(float(loss)) < 1e-6
        assert float(grad.abs().max()) == 0.0
    # one class everywhere: G or H is empty for every class, so the boundary term vanishes and sends no gradient
    t[:] = 1.0
    loss, terms, grad = _gpu(hip_device, p, t, C, dice_weight=0.0, boundary_weight=1.0)
    assert float(terms[2]) == 0.0 and float(loss) == 0.0 and float(grad.abs().max()) == 0.0


@pytest.mark.parametrize('opts', [dict(), dict(weights=[0.2, 1.0, 3.0], include_background=False, batch_dice=True,
                                               ignore_label=255)], ids=['default', 'options'])
@pytest.mark.parametrize('shape', [(2, 5, 7, 9), (2, 16, 20, 24)], ids=['scalar', 'vec'])
def test_region_term_is_bit_equal_to_dicece(hip_device, shape, opts):
    """last_terms[1] comes from the compound loss's device code in the compound loss's order of additions (scalar path,
    and the 16-byte path over more than one workgroup per sample)"""
    from segmentation3d.loss.compound_loss import DiceCELoss
    C = 3
    p, t = _inputs(600, shape, C, ignore_frac=0.1 if 'ignore_label' in opts else 0.0)
    _, terms, _ = _gpu(hip_device, p, t, C, spacing=(0.7, 1.3, 2.5), **opts)
    ce = DiceCELoss(C, **opts)
    ce(p.to(hip_device), t.to(hip_device))
    torch.cuda.synchronize()
    assert float(terms[1]) == float(ce.last_terms[1])
    assert np.float32(float(terms[1])).tobytes() == np.float32(float(ce.last_terms[1])).tobytes()


def test_set_boundary_weight_two_runs_and_graph_replay(hip_device):
    """two eager runs agree bit for bit; the loss after set_boundary_weight equals the oracle at the new weight; ONE graph
    captured at the old weight and replayed after the change gives the bits of an eager call at the new weight"""
    from segmentation3d.loss.boundary_loss import DiceBoundaryLoss
    C = 3
    p, t = _inputs(700, (2, 16, 20, 24), C, ignore_frac=0.1)
    opts = dict(weights=[0.2, 1.0, 3.0], ignore_label=255, spacing=(0.7, 1.3, 2.5))
    a = _gpu(hip_device, p, t, C, boundary_weight=0.01, **opts)
    b = _gpu(hip_device, p, t, C, boundary_weight=0.01, **opts)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    new = _check('new_weight_eager_reference', hip_device, p, t, C, boundary_weight=0.4, **opts)

    loss_fn = DiceBoundaryLoss(C, boundary_weight=0.01, **opts)
    pg = p.to(hip_device).requires_grad_(True)
    tg = t.to(hip_device)

    def step():
        pg.grad = None
        loss = loss_fn(pg, tg)
        loss.backward()
        return loss

    step()
    torch.cuda.synchronize()
    assert torch.equal(loss_fn.last_terms.cpu(), a[1]) and torch.equal(pg.grad.cpu(), a[2])
    loss_fn.set_boundary_weight(0.4)
    assert loss_fn.boundary_weight == 0.4
    step()
    torch.cuda.synchronize()
    assert torch.equal(loss_fn.last_terms.cpu(), new[1]) and torch.equal(pg.grad.cpu(), new[2])   # eager, after the change
    phi = _kernel_phi(hip_device, t, C, opts)
    ref = boundary_oracle(p, t, phi.numpy(), boundary_weight=0.4, **{k: v for k, v in opts.items() if k != 'spacing'})
    assert abs(float(loss_fn.last_terms[0]) - float(ref[0])) < 1e-4 * max(1.0, float(phi.abs().mean()))

    loss_fn.set_boundary_weight(0.01)
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
    for weight, want in ((0.01, a), (0.4, new)):
        loss_fn.set_boundary_weight(weight)      # a plain fill outside the captured region
        with torch.no_grad():
            grad.zero_()
            terms.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(terms.cpu(), want[1]) and torch.equal(grad.cpu(), want[2]), weight
        assert float(loss) == float(want[0])


# ---- training -----------------------------------------------------------------------------------------------------------
def test_train_step_eager_and_graph_agree(hip_device):
    """TrainStep('vnet', 1, 2, loss_name='DiceBoundary') on 2 x 32^3 for three steps, eager and with the whole step in one
    hipGraph: finite losses, terms[0] == loss, and the same parameters afterwards.  The DiceCE train-step test's tolerance
    is 1e-6; measured on the MI355X: the two modes agree bit for bit (0.0)."""
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import TrainStep
    from segmentation3d.loss.boundary_loss import DiceBoundaryLoss
    t = detgen.labels(700, 'cl/t', (2, 1, 32, 32, 32), 2).astype(np.float32)
    x = (t * 2.0 - 1.0 + 0.3 * detgen.normal(701, 'cl/x', (2, 1, 32, 32, 32))).astype(np.float32)
    x, t = torch.from_numpy(x).to(hip_device), torch.from_numpy(t).to(hip_device)
    params = {}
    for use_graph in (False, True):
        step = TrainStep('vnet', 1, 2, loss_name='DiceBoundary', lr=1e-3, device=hip_device, seed=3, use_graph=use_graph,
                         loss_options={'boundary_weight': 0.05, 'spacing': (0.7, 1.3, 2.5)})
        assert isinstance(step.loss_func, DiceBoundaryLoss) and step.loss_func.spacing == (0.7, 1.3, 2.5)
        losses = []
        for _ in range(3):
            loss = step(x, t)
            terms = step.loss_func.last_terms
            losses.append(float(loss))
            assert float(terms[0]) == float(loss)
        torch.cuda.synchronize()
        assert step.use_graph == use_graph and (step._graph is not None) == use_graph
        assert all(np.isfinite(losses)), losses
        params[use_graph] = [q.detach().cpu().clone() for q in step.net.parameters()]
        report('boundary_train_{}'.format('graph' if use_graph else 'eager'), **{'loss_{}'.format(i): v for i, v in enumerate(losses)})
        _ops.PACK_CACHE.clear()
    diff = max(float((a - b).abs().max()) for a, b in zip(params[False], params[True]))
    report('boundary_train_eager_vs_graph', max_param_diff=diff)
    print('boundary_train_eager_vs_graph', diff)
    assert diff < 1e-6, diff


def test_train_engine_follows_the_weight_schedule(hip_device, tmp_path):
    """core/seg_train.train() from a config file with loss.name = 'DiceBoundary', the three schedule keys and a
    `validation` section: the logged boundary_weight is min(max, w0 + step * epoch) and both loss objects end on it"""
    from segmentation3d.core.seg_train import train
    from segmentation3d.loss.boundary_loss import DiceBoundaryLoss
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    lists = {}
    for name, first in (('train', 0), ('val', 2)):
        paths = []
        for k in range(first, first + 2):
            os.makedirs(str(tmp_path / 'c{}'.format(k)), exist_ok=True)
            lab = detgen.labels(800 + k, 'bde2e/seg{}'.format(k), (48, 48, 48), 2)
            img = (lab.astype(np.float32) * 2.0 - 1.0 + 0.3 * detgen.normal(810 + k, 'bde2e/n{}'.format(k), (48, 48, 48))).astype(np.float32)
            ip, sp = str(tmp_path / 'c{}'.format(k) / 'org.mha'), str(tmp_path / 'c{}'.format(k) / 'seg.mha')
            write_mha(Image3d(img, *frame), ip)
            write_mha(Image3d(lab.astype(np.int8), *frame), sp)
            paths += [ip, sp]
        (tmp_path / (name + '.txt')).write_text('2\n' + '\n'.join(paths) + '\n')
        lists[name] = str(tmp_path / (name + '.txt'))
    cfg = tmp_path / 'cfg.py'
    cfg.write_text('''
from easydict import EasyDict as edict
from segmentation3d.utils.normalizer import AdaptiveNormalizer
__C = edict()
cfg = __C
__C.general = {}
__C.general.imseg_list = '%s'
__C.general.save_dir = '%s'
__C.general.model_scale = 'coarse'
__C.general.resume_epoch = -1
__C.general.num_gpus = 1
__C.general.seed = 0
__C.dataset = {}
__C.dataset.num_classes = 2
__C.dataset.spacing = [1.0, 1.0, 1.0]
__C.dataset.crop_size = [32, 32, 32]
__C.dataset.sampling_method = 'GLOBAL'
__C.dataset.random_translation = [2, 2, 2]
__C.dataset.random_scale = [0.95, 1.05]
__C.dataset.interpolation = 'LINEAR'
__C.dataset.crop_normalizers = [AdaptiveNormalizer()]
__C.loss = {}
__C.loss.name = 'DiceBoundary'
__C.loss.obj_weight = [1.0, 1.0]
__C.loss.focal_gamma = 2
__C.loss.boundary_weight = 0.01
__C.loss.boundary_weight_step = 0.02
__C.loss.boundary_weight_max = 0.05
__C.net = {}
__C.net.name = 'vnet'
__C.train = {}
__C.train.epochs = 4
__C.train.batchsize = 2
__C.train.num_threads = 0
__C.train.lr = 1e-3
__C.train.betas = (0.9, 0.999)
__C.train.save_epochs = 2
__C.validation = {}
__C.validation.imseg_list = '%s'
__C.validation.crops_per_case = 2
__C.validation.ema = 0.5
''' % (lists['train'], str(tmp_path / 'model'), lists['val']))
    from segmentation3d import _ops
    try:
        step = train(str(cfg))
    finally:
        _ops.set_activation_dtype('fp32')
    assert isinstance(step.loss_func, DiceBoundaryLoss) and step.loss_func.spacing == (1.0, 1.0, 1.0)
    log = (tmp_path / 'model' / 'coarse' / 'train_log.txt').read_text().strip().splitlines()
    lines = [l for l in log if 'train_loss' in l]
    losses = [float(l.split('train_loss: ')[1].split(',')[0]) for l in lines]
    epochs = [int(l.split('epoch: ')[1].split(',')[0]) for l in lines]
    weights = [float(l.split('boundary_weight: ')[1].split(',')[0]) for l in lines]
    val = [float(l.split('val_loss: ')[1].split(',')[0]) for l in log if 'val_loss' in l]
    assert len(losses) == 4 and all(np.isfinite(losses)), losses
    assert epochs == [0, 1, 2, 3]
    assert weights == pytest.approx([min(0.05, 0.01 + 0.02 * e) for e in epochs], rel=1e-5)
    assert len(val) >= 1 and all(np.isfinite(val)), val
    assert step.loss_func.boundary_weight == pytest.approx(0.05)
    assert isinstance(step.validator.loss_func, DiceBoundaryLoss)
    assert step.validator.loss_func.boundary_weight == step.loss_func.boundary_weight
