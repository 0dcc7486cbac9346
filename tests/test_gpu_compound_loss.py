"""The compound loss kernels (seg3d_compound_loss_fwd / _bwd) on the GPU against the float64 oracle of
tests/test_compound_loss.py, evaluated on the same float32 probabilities; run-to-run and hipGraph behaviour; training.

Bars are the project's parity bars: the loss and its two terms within 1e-4 of the oracle (they are O(1)), the gradient
within gpu_util.rel_err < 1e-4, and exact zeros where the definition says zero."""
import os

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
from gpu_util import rel_err, report
from oracle import detgen
from test_compound_loss import oracle

pytestmark = pytest.mark.gpu

SHAPES = {'5x7x9': (2, 5, 7, 9), '17^3': (3, 17, 17, 17), '32^3': (2, 32, 32, 32), '4x96^3': (4, 96, 96, 96)}


def _inputs(seed, shape, C, ignore_frac=0.0, out_of_range=False):
    """probabilities = soft-max of 2 * randn logits (p_t stays far above the 1e-12 clamp), random class ids"""
    g = torch.Generator().manual_seed(seed)
    N, sp = shape[0], tuple(shape[1:])
    p = torch.softmax(2.0 * torch.randn((N, C) + sp, generator=g), dim=1).float()
    t = torch.randint(0, C, (N, 1) + sp, generator=g).float()
    if ignore_frac > 0.0:
        t[torch.rand(t.shape, generator=g) < ignore_frac] = 255.0
    if out_of_range:
        r = torch.rand(t.shape, generator=g)
        t[r < 0.03] = float(C)
        t[(r >= 0.03) & (r < 0.06)] = -1.0
        t[(r >= 0.06) & (r < 0.08)] = 1000.0
    return p, t


def _gpu(dev, p, t, C, **opts):
    from segmentation3d.loss.compound_loss import DiceCELoss
    loss_fn = DiceCELoss(C, **opts)
    pg = p.to(dev).requires_grad_(True)
    loss = loss_fn(pg, t.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), loss_fn.last_terms.detach().cpu(), pg.grad.detach().cpu()


def _check(name, dev, p, t, C, check_floor=True, **opts):
    if check_floor:
        assert float(p.min()) > 1e-9      # the comparison never sits on the clamp's kink: checked, not assumed
    loss, terms, grad = _gpu(dev, p, t, C, **opts)
    pr = p.clone().requires_grad_(True)
    ref = oracle(pr, t, **opts)
    (ref_grad,) = torch.autograd.grad(ref[0], pr)
    errs = {'loss': abs(float(terms[0]) - float(ref[0])), 'region': abs(float(terms[1]) - float(ref[1])),
            'dist': abs(float(terms[2]) - float(ref[2])), 'dprobs_rel': rel_err(grad, ref_grad)}
    report('compound_' + name, **errs)
    print('compound_' + name, errs)
    assert float(loss) == float(terms[0])
    assert torch.isfinite(terms).all() and torch.isfinite(grad).all()
    assert errs['loss'] < 1e-4 and errs['region'] < 1e-4 and errs['dist'] < 1e-4, errs
    assert errs['dprobs_rel'] < 1e-4, errs
    # exact zeros: every plane of a voxel that does not count ...
    ign = opts.get('ignore_label')
    valid = (t >= 0) & (t < C)
    if ign is not None:
        valid = valid & (t != float(ign))
    dead = (~valid).expand(-1, C, *([-1] * (t.dim() - 2)))
    if bool(dead.any()):
        assert float(grad[dead].abs().max()) == 0.0
    # ... the region part of an excluded background plane (what is left there is the distribution part on t == 0) ...
    if not opts.get('include_background', True):
        off = (t != 0)
        assert float(grad[:, :1][off].abs().max()) == 0.0
    # ... and, without the region term, every plane but the target's
    if opts.get('dice_weight', 1.0) == 0.0:
        for c in range(C):
            if bool((t != c).any()):
                assert float(grad[:, c:c + 1][t != c].abs().max()) == 0.0
    return errs


@pytest.mark.parametrize('C', [1, 2, 5, 16])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_forward_backward_equal_the_oracle(hip_device, shape, C):
    """every shape class (S % 4 != 0: scalar path; odd S above one workgroup's share; 16-byte path; full size) with every
    class-count specialisation (1, 2, 5 exact; 16 generic), default options.
    Measured on the MI355X over this file's cases: loss and terms within 3.3e-7 of the oracle, rel_err(dprobs) <= 2.0e-7
    (DESIGN.md section 7, row f7)."""
    p, t = _inputs(100 + C, SHAPES[shape], C)
    _check('{}_C{}'.format(shape, C), hip_device, p, t, C)


OPTIONS = {
    'weights': dict(weights=[0.2, 1.0, 3.0, 0.5, 2.0]),
    'no_background': dict(include_background=False),
    'batch_dice': dict(batch_dice=True),
    'ignore255': dict(ignore_label=255),
    'out_of_range': dict(),
    'gamma0': dict(gamma=0.0),
    'gamma1': dict(gamma=1.0),
    'gamma2': dict(gamma=2.0),
    'gamma1.5': dict(gamma=1.5),
    'dice_weight0': dict(dice_weight=0.0),
    'ce_weight0': dict(ce_weight=0.0),
    'combined_a': dict(weights=[0.2, 1.0, 3.0, 0.5, 2.0], include_background=False, batch_dice=True, ignore_label=255,
                       gamma=2.0, dice_weight=0.7, ce_weight=1.3),
    'combined_b': dict(weights=[0.2, 1.0, 3.0, 0.5, 2.0], ignore_label=255, gamma=1.5, dice_weight=2.0, ce_weight=0.5),
}


@pytest.mark.parametrize('shape', ['17^3', '32^3'])
@pytest.mark.parametrize('option', list(OPTIONS))
def test_options_equal_the_oracle(hip_device, option, shape):
    """each option alone and two combinations, C = 5, on the scalar (17^3) and the 16-byte (32^3) path"""
    opts = OPTIONS[option]
    ignore_frac = 0.1 if opts.get('ignore_label') is not None else 0.0
    p, t = _inputs(200, SHAPES[shape], 5, ignore_frac=ignore_frac,
                   out_of_range=option in ('out_of_range', 'combined_b'))
    _check('{}_{}'.format(option, shape), hip_device, p, t, 5, **opts)


@pytest.mark.parametrize('C,opts', [(2, dict(ignore_label=255, gamma=2.0)), (16, dict(ignore_label=255, batch_dice=True,
                                                                                    include_background=False, gamma=1.5))])
def test_options_at_full_size(hip_device, C, opts):
    p, t = _inputs(300 + C, SHAPES['4x96^3'], C, ignore_frac=0.1, out_of_range=True)
    _check('full_C{}'.format(C), hip_device, p, t, C, **opts)


@pytest.mark.parametrize('gamma', [0.0, 2.0])
def test_clamp_case(hip_device, gamma):
    """a handful of voxels with p_t = 0 exactly: each contributes -log(1e-12) (times (1 - 1e-12)^gamma) to the loss, and
    the distribution term sends no gradient there (the clamp's gradient, as autograd gives for clamp_min)"""
    C = 3
    p, t = _inputs(400, SHAPES['32^3'], C)
    flat_t = t.reshape(2, -1)
    P = p.reshape(2, C, -1)
    where = [(0, 0), (0, 5), (0, 4099), (1, 17), (1, 32767)]
    for n, s in where:
        c = int(flat_t[n, s])
        P[n, (c + 1) % C, s] += P[n, c, s]
        P[n, c, s] = 0.0
    # both terms against the oracle (value and gradient) ...
    _check('clamp_gamma{}'.format(gamma), hip_device, p, t, C, check_floor=False, gamma=gamma)
    # ... and the distribution term alone: finite and exactly zero gradients on all planes of those voxels
    _check('clamp_dist_gamma{}'.format(gamma), hip_device, p, t, C, check_floor=False, gamma=gamma, dice_weight=0.0)
    _, terms, grad = _gpu(hip_device, p, t, C, gamma=gamma, dice_weight=0.0)
    G = grad.reshape(2, C, -1)
    for n, s in where:
        assert float(G[n, :, s].abs().max()) == 0.0
    assert float(terms[2]) > 5 * (-np.log(1e-12)) / flat_t.numel()


def test_ignored_samples_give_no_nan(hip_device):
    """an all-ignored sample inside a batch and an all-ignored batch: finite everywhere, zero where nothing counts"""
    C = 3
    p, t = _inputs(500, SHAPES['17^3'], C)
    t[1] = 255.0
    for opts in (dict(ignore_label=255), dict(ignore_label=255, batch_dice=True, gamma=2.0)):
        _check('one_sample_ignored', hip_device, p, t, C, **opts)
    t[:] = 255.0
    for opts in (dict(ignore_label=255), dict(ignore_label=255, batch_dice=True, gamma=2.0, include_background=False)):
        loss, terms, grad = _gpu(hip_device, p, t, C, **opts)
        assert torch.isfinite(terms).all() and torch.isfinite(grad).all()
        assert float(terms[2]) == 0.0 and abs(float(terms[1])) < 1e-6 and abs(float(loss)) < 1e-6
        assert float(grad.abs().max()) == 0.0


def test_two_runs_bit_equal_and_graph_replay_equals_eager(hip_device):
    """no atomics, fixed summation order: two eager runs agree bit for bit, and forward + backward captured in a hipGraph
    and replayed twice gives the eager bits (one replay series, nothing is provoked)"""
    from segmentation3d.loss.compound_loss import DiceCELoss
    C = 5
    p, t = _inputs(600, SHAPES['32^3'], C, ignore_frac=0.1)
    opts = dict(weights=[0.2, 1.0, 3.0, 0.5, 2.0], ignore_label=255, gamma=2.0)
    a = _gpu(hip_device, p, t, C, **opts)
    b = _gpu(hip_device, p, t, C, **opts)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])

    loss_fn = DiceCELoss(C, **opts)
    pg = p.to(hip_device).requires_grad_(True)
    tg = t.to(hip_device)

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
    for _ in range(2):
        with torch.no_grad():
            grad.zero_()
            terms.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(terms.cpu(), a[1]) and torch.equal(grad.cpu(), a[2])
        assert float(loss) == float(a[0])


@pytest.mark.parametrize('mode,use_graph', [('fp32', False), ('fp32', True), ('bf16', False), ('bf16', True)])
def test_train_step_with_dicece(hip_device, mode, use_graph):
    """TrainStep('vnet', 1, 2, loss_name='DiceCE'): 6 steps on a fixed 2 x 32^3 batch, eager / whole step in a hipGraph,
    fp32 / bf16 mode"""
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import TrainStep
    from segmentation3d.loss.compound_loss import DiceCELoss
    t = detgen.labels(700, 'cl/t', (2, 1, 32, 32, 32), 2).astype(np.float32)
    x = (t * 2.0 - 1.0 + 0.3 * detgen.normal(701, 'cl/x', (2, 1, 32, 32, 32))).astype(np.float32)
    x, t = torch.from_numpy(x).to(hip_device), torch.from_numpy(t).to(hip_device)
    with _ops.activation_dtype(mode):
        step = TrainStep('vnet', 1, 2, loss_name='DiceCE', lr=1e-3, device=hip_device, seed=3, use_graph=use_graph)
        assert isinstance(step.loss_func, DiceCELoss)
        losses = []
        for _ in range(6):
            loss = step(x, t)
            terms = step.loss_func.last_terms
            losses.append(float(loss))
            assert abs(float(terms[1] + terms[2]) - float(loss)) < 1e-6 and float(terms[0]) == float(loss)
        _ops.PACK_CACHE.clear()
    report('compound_train_{}_{}'.format(mode, 'graph' if use_graph else 'eager'),
           **{'loss_{}'.format(i): v for i, v in enumerate(losses)})
    assert step.use_graph == use_graph and (step._graph is not None) == use_graph
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_train_engine_end_to_end_with_dicece_and_ignore_label(hip_device, tmp_path):
    """core/seg_train.train() from a config file with loss.name = 'DiceCE' and loss.ignore_label = 255 on a toy data set
    whose uint8 masks carry a slab of 255 ("not annotated"; the mask crop is resampled with NN, so the value survives)"""
    from segmentation3d.core.seg_train import train
    from segmentation3d.loss.compound_loss import DiceCELoss
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    paths = []
    for k in range(2):
        os.makedirs(str(tmp_path / 'c{}'.format(k)), exist_ok=True)
        lab = detgen.labels(800 + k, 'cle2e/seg{}'.format(k), (48, 48, 48), 2)
        img = (lab.astype(np.float32) * 2.0 - 1.0 + 0.3 * detgen.normal(810 + k, 'cle2e/n{}'.format(k), (48, 48, 48))).astype(np.float32)
        seg = lab.astype(np.uint8)
        seg[:, 20:28, :] = 255
        ip, sp = str(tmp_path / 'c{}'.format(k) / 'org.mha'), str(tmp_path / 'c{}'.format(k) / 'seg.mha')
        write_mha(Image3d(img, *frame), ip)
        write_mha(Image3d(seg, *frame), sp)
        paths += [ip, sp]
    (tmp_path / 'train.txt').write_text('2\n' + '\n'.join(paths) + '\n')
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
__C.loss.name = 'DiceCE'
__C.loss.obj_weight = [0.5, 0.5]
__C.loss.focal_gamma = 2
__C.loss.ignore_label = 255
__C.net = {}
__C.net.name = 'vnet'
__C.train = {}
__C.train.epochs = 6
__C.train.batchsize = 2
__C.train.num_threads = 0
__C.train.lr = 1e-3
__C.train.betas = (0.9, 0.999)
__C.train.save_epochs = 2
''' % (str(tmp_path / 'train.txt'), str(tmp_path / 'model')))
    from segmentation3d import _ops
    try:
        step = train(str(cfg))
    finally:
        _ops.set_activation_dtype('fp32')
    assert isinstance(step.loss_func, DiceCELoss) and step.loss_func.ignore_label == 255.0
    log = (tmp_path / 'model' / 'coarse' / 'train_log.txt').read_text().strip().splitlines()
    losses = [float(l.split('train_loss: ')[1].split(',')[0]) for l in log if 'train_loss' in l]
    report('compound_train_e2e', **{'loss_{}'.format(i): v for i, v in enumerate(losses)})
    assert len(losses) == 6 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
