"""The compound loss (soft Dice + cross-entropy / focal, ignore label) without a GPU: the float64 oracle that the GPU tests
compare the kernels with, pinned against independent answers, and the module / build_loss / config behaviour.

The oracle is a stock-torch restatement of the definitions in DESIGN.md section 7 (row f7), written from the formulas;
it is differentiable, so autograd supplies the reference gradient."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

import conftest  # noqa: F401  (puts the package on sys.path)
from segmentation3d.core.seg_train import build_loss, loss_options_from_config
from segmentation3d.loss.compound_loss import DiceCELoss
from segmentation3d.loss.cross_entropy_loss import CrossEntropyLoss
from segmentation3d.loss.focal_loss import FocalLoss
from segmentation3d.loss.multi_dice_loss import MultiDiceLoss

EPS = 1e-5
PMIN = 1e-12


def oracle(p, t, weights=None, dice_weight=1.0, ce_weight=1.0, gamma=0.0, include_background=True, batch_dice=False,
           ignore_label=None):
    """(L, L_region, L_dist) as float64 0-dim tensors; p [N, C, *spatial] (any float dtype, evaluated in float64),
    t [N, 1, *spatial] float class ids"""
    N, C = p.shape[0], p.shape[1]
    P = p.double().reshape(N, C, -1)
    T = t.reshape(N, -1).double()
    valid = (T >= 0) & (T < C)
    if ignore_label is not None:
        valid = valid & (T != float(ignore_label))
    v = valid.double()
    w = torch.ones(C, dtype=torch.float64) if weights is None else torch.tensor([float(x) for x in weights], dtype=torch.float64)
    K = list(range(C)) if include_background else list(range(1, C))
    if not K:
        raise ValueError('no class left')
    onehot = torch.stack([((T == c) & valid).double() for c in range(C)], dim=1)          # [N, C, S]
    I = (P * onehot).sum(-1)                                                               # onehot carries v
    U = (P * v[:, None, :]).sum(-1) + onehot.sum(-1)
    if batch_dice:
        I, U = I.sum(0, keepdim=True), U.sum(0, keepdim=True)
    d = (2.0 * I + EPS) / (U + EPS)
    wsum = sum(w[c] for c in K)
    l_region = sum((w[c] / wsum) * (1.0 - d[:, c].mean()) for c in K)
    idx = torch.where(valid, T, torch.zeros_like(T)).long()
    pt = P.gather(1, idx[:, None, :]).squeeze(1).clamp_min(PMIN)
    a = w[idx] * v
    f = a * (-torch.log(pt))
    if gamma != 0.0:
        f = f * (1.0 - pt) ** gamma
    den = a.sum()
    l_dist = f.sum() / den if float(den) > 0.0 else f.sum() * 0.0
    total = torch.zeros((), dtype=torch.float64)
    if dice_weight > 0.0:
        total = total + dice_weight * l_region
    if ce_weight > 0.0:
        total = total + ce_weight * l_dist
    return total, l_region, l_dist


def _case(seed, shape, C, ignore_frac=0.0, ignore_label=255):
    g = torch.Generator().manual_seed(seed)
    N = shape[0]
    p = torch.softmax(2.0 * torch.randn((N, C) + tuple(shape[1:]), generator=g, dtype=torch.float64), dim=1)
    t = torch.randint(0, C, (N, 1) + tuple(shape[1:]), generator=g).double()
    if ignore_frac > 0.0:
        t[torch.rand(t.shape, generator=g) < ignore_frac] = float(ignore_label)
    return p, t


# ---- the oracle against independent answers -------------------------------------------------------------------------
@pytest.mark.parametrize('weights', [None, [0.2, 1.0, 3.0]])
@pytest.mark.parametrize('ignore', [None, 255])
def test_oracle_gamma0_is_nll_loss(weights, ignore):
    p, t = _case(1, (2, 5, 6, 7), 3, ignore_frac=0.2 if ignore is not None else 0.0)
    p.requires_grad_(True)
    total, _, l_dist = oracle(p, t, weights=weights, dice_weight=0.0, ignore_label=ignore)
    q = p.detach().clone().requires_grad_(True)
    ref = F.nll_loss(torch.log(q.clamp_min(PMIN)), t[:, 0].long(), weight=None if weights is None else torch.tensor(weights, dtype=torch.float64),
                     ignore_index=ignore if ignore is not None else -100, reduction='mean')
    assert abs(total.item() - ref.item()) < 1e-12 and total.item() == l_dist.item()
    total.backward()
    ref.backward()
    assert float((p.grad - q.grad).abs().max()) < 1e-12


def test_oracle_perfect_prediction_is_zero():
    _, t = _case(2, (2, 4, 5, 6), 4)
    p = torch.stack([(t[:, 0] == c).double() for c in range(4)], dim=1)
    total, l_region, l_dist = oracle(p, t)
    assert abs(float(l_region)) < 1e-12 and float(l_dist) == 0.0 and abs(float(total)) < 1e-12


@pytest.mark.parametrize('C', [2, 5])
def test_oracle_uniform_prediction_closed_forms(C):
    _, t = _case(3, (1, 6, 6, 6), C)
    S = t.numel()
    p = torch.full((1, C, 6, 6, 6), 1.0 / C, dtype=torch.float64)
    _, l_region, l_dist = oracle(p, t)
    assert abs(float(l_dist) - math.log(C)) < 1e-12
    expect = 0.0
    for c in range(C):
        Sc = float((t == c).sum())
        expect += (1.0 / C) * (1.0 - (2.0 * Sc / C + EPS) / (S / C + Sc + EPS))
    assert abs(float(l_region) - expect) < 1e-12


def test_oracle_everything_ignored_is_zero_with_zero_gradient():
    p, t = _case(4, (2, 3, 4, 5), 3)
    t[:] = 255.0
    p.requires_grad_(True)
    for gamma in (0.0, 2.0):
        total, l_region, l_dist = oracle(p, t, gamma=gamma, ignore_label=255)
        assert total.item() == 0.0 and l_region.item() == 0.0 and l_dist.item() == 0.0
        (g,) = torch.autograd.grad(total, p)
        assert torch.isfinite(g).all() and float(g.abs().max()) == 0.0


def test_oracle_batch_dice_equals_per_sample_for_one_sample():
    p, t = _case(5, (1, 5, 5, 5), 3, ignore_frac=0.1)
    a = oracle(p, t, weights=[1.0, 2.0, 3.0], ignore_label=255, batch_dice=False)
    b = oracle(p, t, weights=[1.0, 2.0, 3.0], ignore_label=255, batch_dice=True)
    assert all(abs(float(x) - float(y)) < 1e-15 for x, y in zip(a, b))


def test_oracle_out_of_range_labels_and_background_exclusion():
    p, t = _case(6, (2, 4, 4, 4), 3)
    t2 = t.clone()
    t2[0, 0, 0] = 7.0
    t2[1, 0, 1] = -3.0
    keep = ((t2 >= 0) & (t2 < 3)).expand(-1, 3, -1, -1, -1)
    p.requires_grad_(True)
    total, _, _ = oracle(p, t2, include_background=False, gamma=1.0)
    (g,) = torch.autograd.grad(total, p)
    assert float(g[~keep].abs().max()) == 0.0 and float(g[keep].abs().max()) > 0.0
    # without the background, plane 0 receives the distribution part only: zero wherever the target is not 0
    not_bg = (t2 != 0).expand(-1, 1, -1, -1, -1)
    assert float(g[:, :1][not_bg].abs().max()) == 0.0
    with pytest.raises(ValueError):
        oracle(p[:, :1], t, include_background=False)


# ---- module, build_loss and config behaviour -------------------------------------------------------------------------
def test_build_loss_names():
    ce = build_loss('DiceCE', 3, None, 2)
    fo = build_loss('DiceFocal', 3, [1.0, 2.0, 3.0], 1.5, ignore_label=255, batch_dice=True, include_background=False,
                    dice_weight=0.5, ce_weight=2.0)
    assert isinstance(ce, DiceCELoss) and ce.gamma == 0.0 and ce.ignore_label is None and ce.include_background
    assert not ce.batch_dice and ce.dice_weight == 1.0 and ce.ce_weight == 1.0 and ce.num_class == 3
    assert isinstance(fo, DiceCELoss) and fo.gamma == 1.5 and fo.ignore_label == 255.0 and fo.batch_dice
    assert not fo.include_background and fo.dice_weight == 0.5 and fo.ce_weight == 2.0
    assert torch.allclose(ce.region_weights, torch.full((3,), 1.0 / 3.0)) and torch.equal(ce.class_weights, torch.ones(3))
    assert torch.allclose(fo.region_weights, torch.tensor([0.0, 0.4, 0.6])) and torch.equal(fo.class_weights, torch.tensor([1.0, 2.0, 3.0]))
    # the three existing names are untouched
    assert type(build_loss('Dice', 2, [0.5, 0.5])) is MultiDiceLoss
    assert type(build_loss('Dice', 2)) is MultiDiceLoss
    assert type(build_loss('Focal', 2, None, 2)) is FocalLoss
    assert type(build_loss('CE', 2)) is CrossEntropyLoss
    with pytest.raises(ValueError, match='Unknown loss function'):
        build_loss('DiceBCE', 2)


@pytest.mark.parametrize('kwargs', [
    dict(dice_weight=-1.0), dict(ce_weight=-0.5), dict(dice_weight=0.0, ce_weight=0.0), dict(gamma=-1.0),
    dict(weights=[1.0, 2.0]), dict(weights=[1.0, 0.0, 1.0]), dict(weights=[1.0, -2.0, 1.0])])
def test_constructor_rejects(kwargs):
    with pytest.raises(ValueError):
        DiceCELoss(3, **kwargs)


def test_single_class_needs_the_background():
    DiceCELoss(1)
    with pytest.raises(ValueError):
        DiceCELoss(1, include_background=False)


def test_forward_rejects_mismatched_shapes():
    loss = DiceCELoss(3)
    with pytest.raises(ValueError):
        loss(torch.rand(2, 4, 4, 4, 4), torch.zeros(2, 1, 4, 4, 4))      # channels != num_class
    with pytest.raises(ValueError):
        loss(torch.rand(2, 3, 4, 4, 4), torch.zeros(2, 1, 4, 4, 5))      # target size
    with pytest.raises(ValueError):
        loss(torch.rand(2, 3, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))


def test_no_cpu_fallback():
    """a missing device is an error, never a quiet eager computation"""
    with pytest.raises(Exception):
        DiceCELoss(2)(torch.rand(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))


def test_config_without_the_new_keys_gives_the_defaults():
    old = types.SimpleNamespace(name='Dice', obj_weight=[0.5, 0.5], focal_gamma=2)
    assert loss_options_from_config(old) == {'dice_weight': 1.0, 'ce_weight': 1.0, 'include_background': True,
                                            'batch_dice': False, 'ignore_label': None}
    new = types.SimpleNamespace(name='DiceCE', obj_weight=None, focal_gamma=2, dice_weight=0.5, ce_weight=2.0,
                                include_background=False, batch_dice=True, ignore_label=255)
    opts = loss_options_from_config(new)
    assert opts == {'dice_weight': 0.5, 'ce_weight': 2.0, 'include_background': False, 'batch_dice': True, 'ignore_label': 255}
    loss = build_loss(new.name, 2, new.obj_weight, new.focal_gamma, **opts)
    assert loss.ignore_label == 255.0 and loss.batch_dice and not loss.include_background


def test_shipped_train_config_keeps_its_keys_and_loads():
    import os
    from segmentation3d.utils.file_io import load_config
    cfg = load_config(os.path.join(conftest.PKG, 'segmentation3d', 'config', 'train_config.py'))
    assert sorted(cfg.loss.keys()) == ['focal_gamma', 'name', 'obj_weight']
    assert loss_options_from_config(cfg.loss) == loss_options_from_config(types.SimpleNamespace())
