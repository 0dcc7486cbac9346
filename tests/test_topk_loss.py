"""The Dice + top-k cross-entropy loss without a GPU: the float64 oracle that tests/test_gpu_topk_loss.py compares the
kernels with, pinned against closed forms, the compound oracle and torch.topk; and the module / build_loss / config
behaviour.

The oracle restates the definitions of DESIGN.md section 7 (row f15) in stock torch, in float64 on the given (float32)
probabilities.  Ties are decided on the float64 values: equal float32 inputs give equal float64 values.  The top-k term is
written as sum_v w_v ell_v / k with the constant weights w_v = 1 / (r / n_eq) / 0, so autograd supplies the reference
gradient, tie rule included."""
import math
import types

import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from segmentation3d.core.seg_train import build_loss, loss_options_from_config
from segmentation3d.loss.compound_loss import DiceCELoss
from segmentation3d.loss.topk_loss import DiceTopKLoss, topk_count
from test_compound_loss import oracle, _case

PMIN = 1e-12


def device_count(n, k_percent):
    """the device's expression, spelled out: max(1, (long long)((double)n * k_percent / 100.0)); 0 for n == 0"""
    if n == 0:
        return 0
    return max(1, int(math.trunc((float(n) * float(k_percent)) / 100.0)))


def topk_oracle(p, t, weights=None, dice_weight=1.0, ce_weight=1.0, k_percent=10.0, include_background=True,
                batch_dice=False, ignore_label=None):
    """dict with the float64 0-dim tensors 'total', 'region', 'topk' (differentiable w.r.t. p), 'selection' =
    (n, k, m, n_eq, r), 'tau' (float, 0.0 when nothing counts), 'ell' / 'w' [N, S] (per-voxel loss and top-k weight; 0 on
    voxels that do not count), 'valid' [N, S] and 'margin': the relative gap between the k-th and the (k+1)-th largest
    ell (inf when k == n or nothing counts)"""
    N, C = p.shape[0], p.shape[1]
    P = p.double().reshape(N, C, -1)
    T = t.reshape(N, -1).double()
    valid = (T >= 0) & (T < C)
    if ignore_label is not None:
        valid = valid & (T != float(ignore_label))
    a = torch.ones(C, dtype=torch.float64) if weights is None else torch.tensor([float(x) for x in weights], dtype=torch.float64)
    _, l_region, _ = oracle(p, t, weights=weights, dice_weight=dice_weight, ce_weight=ce_weight, gamma=0.0,
                            include_background=include_background, batch_dice=batch_dice, ignore_label=ignore_label)
    idx = torch.where(valid, T, torch.zeros_like(T)).long()
    pt = P.gather(1, idx[:, None, :]).squeeze(1).clamp_min(PMIN)
    ell = a[idx] * (-torch.log(pt))
    ell = ell + 0.0                                                     # -0.0 -> +0.0, the gradient stays
    ell = torch.where(valid, ell, torch.zeros_like(ell))
    vals = ell.detach()[valid]
    n = int(vals.numel())
    k = device_count(n, k_percent)
    w = torch.zeros_like(vals)
    tau, m, n_eq, r, margin = 0.0, 0, 0, 0, float('inf')
    if n > 0:
        srt = torch.sort(vals, descending=True).values
        tau = float(srt[k - 1])
        m = int((vals > tau).sum())
        n_eq = int((vals == tau).sum())
        r = k - m
        assert 1 <= r <= n_eq
        w = (vals > tau).double() + (vals == tau).double() * (float(r) / float(n_eq))
        if k < n:
            margin = (tau - float(srt[k])) / tau if tau > 0.0 else 0.0
    W = torch.zeros_like(ell.detach())
    W[valid] = w
    l_topk = (W * ell).sum() / k if k > 0 else ell.sum() * 0.0
    total = torch.zeros((), dtype=torch.float64)
    if dice_weight > 0.0:
        total = total + dice_weight * l_region
    if ce_weight > 0.0:
        total = total + ce_weight * l_topk
    return {'total': total, 'region': l_region, 'topk': l_topk, 'selection': (n, k, m, n_eq, r), 'tau': tau,
            'ell': ell.detach(), 'w': W, 'valid': valid, 'margin': margin}


def tie_fixture(seed=0):
    """C = 2, one sample 5 x 5 x 8, target 1 everywhere; p_1 = 1/8 on 30 voxels, 1/4 on 50, 1/2 on 120, shuffled"""
    g = torch.Generator().manual_seed(seed)
    p1 = torch.cat([torch.full((30,), 0.125), torch.full((50,), 0.25), torch.full((120,), 0.5)])
    p1 = p1[torch.randperm(200, generator=g)].reshape(1, 1, 5, 5, 8)
    p = torch.cat([1.0 - p1, p1], dim=1).float()
    t = torch.ones(1, 1, 5, 5, 8)
    return p, t


TIE_CASES = {20.0: (200, 40, 30, 50, 10), 15.0: (200, 30, 0, 30, 30), 0.1: (200, 1, 0, 30, 1), 100.0: (200, 200, 80, 120, 120)}


# ---- the oracle against independent answers -------------------------------------------------------------------------
@pytest.mark.parametrize('k_percent', list(TIE_CASES))
def test_oracle_tie_fixture_closed_forms(k_percent):
    p, t = tie_fixture()
    o = topk_oracle(p, t, k_percent=k_percent, dice_weight=0.0)
    n, k, m, n_eq, r = o['selection']
    assert o['selection'] == TIE_CASES[k_percent]
    assert abs(float(o['w'].sum()) - k) < 1e-9                       # sum w_v == k
    if k_percent == 20.0:
        assert abs(o['topk'].item() - 1.9061547465398494) < 1e-12
        assert abs(o['topk'].item() - (30 * math.log(8) + 10 * math.log(4)) / 40) < 1e-12
        assert abs(o['tau'] - math.log(4)) < 1e-15
    if k_percent == 100.0:
        assert abs(o['topk'].item() - (30 * math.log(8) + 50 * math.log(4) + 120 * math.log(2)) / 200) < 1e-12


def test_oracle_tie_gradient_is_shared_equally():
    p, t = tie_fixture()
    p.requires_grad_(True)
    o = topk_oracle(p, t, k_percent=20.0, dice_weight=0.0)
    (g,) = torch.autograd.grad(o['total'], p)
    n, k, m, n_eq, r = o['selection']
    g1, p1 = g[0, 1].reshape(-1).double(), p.detach()[0, 1].reshape(-1).double()
    assert float(g[0, 0].abs().max()) == 0.0
    assert torch.allclose(g1[p1 == 0.125], torch.full((30,), -1.0 / (k * 0.125), dtype=torch.float64), rtol=1e-6)
    assert torch.allclose(g1[p1 == 0.25], torch.full((50,), -(r / n_eq) / (k * 0.25), dtype=torch.float64), rtol=1e-6)
    assert float(g1[p1 == 0.5].abs().max()) == 0.0


@pytest.mark.parametrize('ignore', [None, 255])
def test_oracle_k100_is_the_compound_cross_entropy(ignore):
    """k_percent = 100 with unit weights: every counted voxel is selected, the top-k term is the plain mean"""
    p, t = _case(11, (2, 5, 6, 7), 3, ignore_frac=0.2 if ignore is not None else 0.0)
    o = topk_oracle(p, t, k_percent=100.0, ignore_label=ignore)
    ref = oracle(p, t, gamma=0.0, ignore_label=ignore)
    assert abs(o['topk'].item() - float(ref[2])) < 1e-12
    assert abs(o['region'].item() - float(ref[1])) < 1e-12 and abs(o['total'].item() - float(ref[0])) < 1e-12
    n, k, m, n_eq, r = o['selection']
    assert k == n and m + r == k


@pytest.mark.parametrize('weights', [None, [0.2, 1.0, 3.0]])
def test_oracle_equals_torch_topk_without_ties(weights):
    p, t = _case(12, (2, 5, 6, 7), 3, ignore_frac=0.2)
    p.requires_grad_(True)
    o = topk_oracle(p, t, weights=weights, k_percent=10.0, dice_weight=0.0, ignore_label=255)
    n, k, m, n_eq, r = o['selection']
    assert n_eq == 1 and r == 1 and m == k - 1 and o['margin'] > 0.0
    q = p.detach().clone().requires_grad_(True)
    a = torch.ones(3, dtype=torch.float64) if weights is None else torch.tensor(weights, dtype=torch.float64)
    T = t.reshape(2, -1)
    valid = T != 255.0
    idx = torch.where(valid, T, torch.zeros_like(T)).long()
    ell = a[idx] * (-torch.log(q.reshape(2, 3, -1).gather(1, idx[:, None, :]).squeeze(1).clamp_min(PMIN)))
    ref = torch.topk(ell[valid], k).values.sum() / k
    assert abs(o['total'].item() - ref.item()) < 1e-12
    (g,) = torch.autograd.grad(o['total'], p)
    (gr,) = torch.autograd.grad(ref, q)
    assert float((g - gr).abs().max()) < 1e-12


def test_oracle_everything_ignored_is_zero_with_zero_gradient():
    p, t = _case(13, (2, 3, 4, 5), 3)
    t[:] = 255.0
    p.requires_grad_(True)
    o = topk_oracle(p, t, ignore_label=255)
    assert o['selection'] == (0, 0, 0, 0, 0) and o['topk'].item() == 0.0 and o['total'].item() == 0.0
    (g,) = torch.autograd.grad(o['total'], p)
    assert float(g.abs().max()) == 0.0


@pytest.mark.parametrize('n', [0, 1, 9, 10, 630, 2 ** 31])
@pytest.mark.parametrize('k_percent', [0.01, 10.0, 15.0, 33.3, 100.0])
def test_topk_count_is_the_device_expression(n, k_percent):
    assert topk_count(n, k_percent) == device_count(n, k_percent)
    if n == 0:
        assert topk_count(n, k_percent) == 0
    else:
        assert 1 <= topk_count(n, k_percent) <= n
    if k_percent == 10.0:
        assert topk_count(n, k_percent) == {0: 0, 1: 1, 9: 1, 10: 1, 630: 63, 2 ** 31: 214748364}[n]


# ---- module, build_loss and config behaviour -------------------------------------------------------------------------
def test_build_loss_dicetopk():
    d = build_loss('DiceTopK', 3, None, 2)
    assert isinstance(d, DiceTopKLoss) and d.k_percent == 10.0 and d.num_class == 3 and d.ignore_label is None
    assert d.dice_weight == 1.0 and d.ce_weight == 1.0 and d.include_background and not d.batch_dice
    assert torch.allclose(d.region_weights, torch.full((3,), 1.0 / 3.0)) and torch.equal(d.class_weights, torch.ones(3))
    f = build_loss('DiceTopK', 3, [1.0, 2.0, 3.0], 1.5, ignore_label=255, batch_dice=True, include_background=False,
                   dice_weight=0.5, ce_weight=2.0, topk_percent=25)
    assert isinstance(f, DiceTopKLoss) and f.k_percent == 25.0 and f.ignore_label == 255.0 and f.batch_dice
    assert not f.include_background and f.dice_weight == 0.5 and f.ce_weight == 2.0
    assert torch.allclose(f.region_weights, torch.tensor([0.0, 0.4, 0.6])) and torch.equal(f.class_weights, torch.tensor([1.0, 2.0, 3.0]))
    assert f.last_terms is None and f.last_selection is None and f.last_threshold is None
    # the other names are untouched
    assert type(build_loss('DiceCE', 3, None, 2)) is DiceCELoss
    with pytest.raises(ValueError, match='Unknown loss function'):
        build_loss('DiceBCE', 2)


@pytest.mark.parametrize('kwargs', [
    dict(dice_weight=-1.0), dict(ce_weight=-0.5), dict(dice_weight=0.0, ce_weight=0.0),
    dict(weights=[1.0, 2.0]), dict(weights=[1.0, 0.0, 1.0]), dict(weights=[1.0, -2.0, 1.0]),
    dict(k_percent=0.0), dict(k_percent=-1.0), dict(k_percent=100.5), dict(k_percent=float('nan')), dict(k_percent=float('inf'))])
def test_constructor_rejects(kwargs):
    with pytest.raises(ValueError):
        DiceTopKLoss(3, **kwargs)


def test_constructor_rejects_num_class_and_background():
    DiceTopKLoss(1, k_percent=100.0)
    with pytest.raises(ValueError):
        DiceTopKLoss(0)
    with pytest.raises(ValueError):
        DiceTopKLoss(1, include_background=False)


def test_forward_rejects_mismatched_shapes():
    loss = DiceTopKLoss(3)
    with pytest.raises(ValueError):
        loss(torch.rand(2, 4, 4, 4, 4), torch.zeros(2, 1, 4, 4, 4))      # channels != num_class
    with pytest.raises(ValueError):
        loss(torch.rand(2, 3, 4, 4, 4), torch.zeros(2, 1, 4, 4, 5))      # target size


def test_no_cpu_fallback():
    """a missing device is an error, never a quiet eager computation"""
    with pytest.raises(Exception):
        DiceTopKLoss(2)(torch.rand(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))


def test_config_key_is_passed_on_only_when_present():
    old = types.SimpleNamespace(name='DiceTopK', obj_weight=None, focal_gamma=2)
    assert 'topk_percent' not in loss_options_from_config(old)
    assert build_loss(old.name, 2, old.obj_weight, old.focal_gamma, **loss_options_from_config(old)).k_percent == 10.0
    new = types.SimpleNamespace(name='DiceTopK', obj_weight=None, focal_gamma=2, topk_percent=20, ignore_label=255)
    opts = loss_options_from_config(new)
    assert opts == {'dice_weight': 1.0, 'ce_weight': 1.0, 'include_background': True, 'batch_dice': False,
                    'ignore_label': 255, 'topk_percent': 20}
    loss = build_loss(new.name, 2, new.obj_weight, new.focal_gamma, **opts)
    assert isinstance(loss, DiceTopKLoss) and loss.k_percent == 20.0 and loss.ignore_label == 255.0


def test_shipped_train_config_has_no_topk_percent():
    import os
    from segmentation3d.utils.file_io import load_config
    cfg = load_config(os.path.join(conftest.PKG, 'segmentation3d', 'config', 'train_config.py'))
    assert 'topk_percent' not in cfg.loss
    assert 'topk_percent' not in loss_options_from_config(cfg.loss)
