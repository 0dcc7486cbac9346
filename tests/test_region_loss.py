"""Region training on the host: the options RegionDiceBCELoss, build_loss, the config keys, TrainStep and the Validator
refuse, and the oracle of the region loss that tests/test_gpu_region_loss.py holds the
kernels against -- plain torch with autograd, in float64 (or, as the yardstick of the device test, in float32), checked
here against a 2-voxel example worked by hand and against F.binary_cross_entropy."""
import math
import os
import types

import pytest
import torch
import torch.nn.functional as F

import conftest  # noqa: F401  (puts the package on sys.path)
from conftest import PKG
from segmentation3d.core.seg_train import (REGION_LOSSES, TrainStep, build_loss, loss_options_from_config,
                                           regions_from_config)
from segmentation3d.core.seg_validate import Validator, validate_validation
from segmentation3d.loss.region_loss import RegionDiceBCELoss, region_lut

BRATS = [[1, 2, 3], [1, 3], [3]]


def region_targets(t, regions, ignore_label=None):
    """(z [N, R, S] bool, counted [N, S] bool) of float label ids t [N, ...]: a voxel counts iff t is an integer in
    [0, 256) and not the ignore label; z is False wherever the voxel does not count"""
    N = t.shape[0]
    T = t.reshape(N, -1).double()
    label = (T >= 0) & (T < 256) & (T == T.floor())
    counted = label if ignore_label is None else label & (T != float(ignore_label))
    member = torch.zeros((256, len(regions)), dtype=torch.bool)
    for r, region in enumerate(regions):
        member[list(region), r] = True
    z = member[torch.where(label, T, torch.zeros_like(T)).long()].permute(0, 2, 1)
    return z & counted.unsqueeze(1), counted


def oracle(p, t, regions, weights=None, dice_weight=1.0, bce_weight=1.0, gamma=0.0, batch_dice=False, ignore_label=None,
           dtype=torch.float64):
    """(L, L_dice, L_bce) of the definitions in include/seg3d_hip.h, differentiable w.r.t. p"""
    N, R = p.shape[0], p.shape[1]
    P = p.to(dtype).reshape(N, R, -1)
    zb, counted = region_targets(t, regions, ignore_label)
    z, m = zb.to(dtype), counted.unsqueeze(1).to(dtype)
    w = torch.ones(R, dtype=dtype) if weights is None else torch.tensor([float(v) for v in weights], dtype=dtype)
    I, Ps, Ts = (P * z).sum(2), (P * m).sum(2), z.sum(2)
    if batch_dice:
        I, Ps, Ts = I.sum(0, keepdim=True), Ps.sum(0, keepdim=True), Ts.sum(0, keepdim=True)
    d = (2.0 * I + 1e-5) / (Ps + Ts + 1e-5)
    l_dice = ((w / w.sum()) * (1.0 - d.mean(0))).sum()
    qc = torch.where(zb, P, 1.0 - P).clamp_min(1e-12)
    ell = -torch.log(qc)
    if gamma > 0.0:
        ell = (1.0 - qc).clamp_min(0.0) ** gamma * ell
    n_counted = int(counted.sum())
    l_bce = (w.view(1, R, 1) * ell * m).sum() / (n_counted * w.sum()) if n_counted > 0 else torch.zeros((), dtype=dtype)
    total = torch.zeros((), dtype=dtype)
    if dice_weight > 0.0:
        total = total + dice_weight * l_dice
    if bce_weight > 0.0:
        total = total + bce_weight * l_bce
    return total, l_dice, l_bce


# ---- the oracle itself ------------------------------------------------------------------------------------------------------
def test_oracle_on_a_hand_worked_example():
    """regions {1, 2} and {2}; voxel 0 has label 1 (in region 0 only), voxel 1 label 2 (in both)"""
    p = torch.tensor([[[0.8, 0.6], [0.3, 0.9]]], dtype=torch.float32)
    t = torch.tensor([[[1.0, 2.0]]])
    p64 = [[float(v) for v in row] for row in p[0]]          # the float32 values, as doubles
    d0 = (2 * (p64[0][0] + p64[0][1]) + 1e-5) / ((p64[0][0] + p64[0][1]) + 2 + 1e-5)
    d1 = (2 * p64[1][1] + 1e-5) / ((p64[1][0] + p64[1][1]) + 1 + 1e-5)
    dice = 0.5 * (1 - d0) + 0.5 * (1 - d1)
    bce = -(math.log(p64[0][0]) + math.log(p64[0][1]) + math.log(1 - p64[1][0]) + math.log(p64[1][1])) / 4
    got = oracle(p, t, [[1, 2], [2]])
    assert abs(float(got[1]) - dice) < 1e-15 and abs(float(got[2]) - bce) < 1e-15
    assert abs(float(got[0]) - (dice + bce)) < 1e-15
    # weights 1 : 3, focal gamma 2, term weights: the same sums by hand
    q = [p64[0][0], p64[0][1], 1 - p64[1][0], p64[1][1]]
    a = [1.0, 1.0, 3.0, 3.0]
    focal = sum(ai * (1 - qi) ** 2 * -math.log(qi) for ai, qi in zip(a, q)) / (2 * 4.0)
    got = oracle(p, t, [[1, 2], [2]], weights=[1, 3], gamma=2.0, dice_weight=0.5, bce_weight=2.0)
    assert abs(float(got[2]) - focal) < 1e-15
    assert abs(float(got[1]) - (0.25 * (1 - d0) + 0.75 * (1 - d1))) < 1e-15
    assert abs(float(got[0]) - (0.5 * float(got[1]) + 2.0 * focal)) < 1e-15
    # a voxel that does not count leaves every sum: the result is that of the one-voxel problem
    t2 = torch.tensor([[[1.0, 7.5]]])
    one = oracle(p[:, :, :1], t2[:, :, :1], [[1, 2], [2]])
    for a_, b_ in zip(oracle(p, t2, [[1, 2], [2]]), one):
        assert float(a_) == float(b_)


def test_oracle_bce_is_binary_cross_entropy_and_labels_in_no_region_are_background():
    g = torch.Generator().manual_seed(1)
    p = torch.rand((2, 3, 4, 5, 6), generator=g).clamp(0.01, 0.99)
    t = torch.randint(0, 6, (2, 1, 4, 5, 6), generator=g).float()     # labels 4 and 5 are in no region, 0 is background
    z, counted = region_targets(t, BRATS)
    assert bool(counted.all()) and not bool(z[:, :, (t.reshape(2, -1) >= 4)[0]][0].any())
    ref = F.binary_cross_entropy(p.double().reshape(2, 3, -1), z.double())
    assert abs(float(oracle(p, t, BRATS)[2]) - float(ref)) < 1e-14
    # ignore label, stray values: the mean runs over the counted voxels only
    t[0, 0, 0, 0, :3] = torch.tensor([255.0, 1.5, -1.0])
    t[1, 0, 1, 1, :2] = torch.tensor([256.0, 300.0])
    z, counted = region_targets(t, BRATS, ignore_label=255)
    assert int((~counted).sum()) == 5
    keep = counted.unsqueeze(1).expand(-1, 3, -1)
    ref = F.binary_cross_entropy(p.double().reshape(2, 3, -1)[keep], z.double()[keep])
    assert abs(float(oracle(p, t, BRATS, ignore_label=255)[2]) - float(ref)) < 1e-14
    nothing = oracle(p, torch.full_like(t, 255.0), BRATS, ignore_label=255)
    assert float(nothing[2]) == 0.0 and abs(float(nothing[1])) < 1e-12


def test_oracle_clamp_sends_no_gradient():
    p = torch.tensor([[[0.0, 1.0, 1e-13, 0.5]]], requires_grad=True)
    t = torch.tensor([[[1.0, 0.0, 1.0, 1.0]]])
    loss = oracle(p, t, [[1]], dice_weight=0.0)[0]
    (g,) = torch.autograd.grad(loss, p)
    assert torch.isfinite(g).all() and float(g[0, 0, 0]) == 0.0 and float(g[0, 0, 1]) == 0.0 and float(g[0, 0, 2]) == 0.0
    assert abs(float(g[0, 0, 3]) + 2.0 / 4) < 1e-15


# ---- RegionDiceBCELoss / build_loss -------------------------------------------------------------------------------------------
def test_loss_options_are_checked():
    loss = RegionDiceBCELoss(BRATS, weights=[1, 2, 3], dice_weight=0.5, bce_weight=2, gamma=1.5, batch_dice=True,
                             ignore_label=255)
    assert loss.regions == BRATS and loss.num_regions == 3 and loss.lut == region_lut(BRATS)
    assert (loss.dice_weight, loss.bce_weight, loss.gamma, loss.batch_dice, loss.ignore_label) == (0.5, 2.0, 1.5, True, 255.0)
    assert torch.allclose(loss.dice_weights, torch.tensor([1 / 6, 2 / 6, 3 / 6])) and loss.bce_weights.tolist() == [1, 2, 3]
    assert loss.last_terms is None
    for bad in (dict(weights=[1, 2]), dict(weights=[1, 0, 1]), dict(weights=[1, -1, 1]), dict(weights=[1, float('inf'), 1]),
                dict(dice_weight=-1), dict(bce_weight=-0.5), dict(dice_weight=0, bce_weight=0), dict(gamma=-1),
                dict(gamma=float('nan')), dict(ignore_label=3), dict(ignore_label=1.0)):
        with pytest.raises(ValueError):
            RegionDiceBCELoss(BRATS, **bad)
    for bad in (None, [], [[0, 1]], [[1, 1]], [[256]], [[1]] * 17, 'abc'):
        with pytest.raises(ValueError):
            RegionDiceBCELoss(bad)
    RegionDiceBCELoss(BRATS, ignore_label=4)        # an ordinary id that no region lists
    RegionDiceBCELoss(BRATS, ignore_label=0)
    with pytest.raises(ValueError):                 # channels
        RegionDiceBCELoss(BRATS)(torch.zeros((1, 2, 2, 2, 2)), torch.zeros((1, 1, 2, 2, 2)))
    with pytest.raises(ValueError):                 # target size
        RegionDiceBCELoss(BRATS)(torch.zeros((1, 3, 2, 2, 2)), torch.zeros((1, 1, 2, 2, 3)))


def test_build_loss_names_and_keywords():
    assert REGION_LOSSES == ('RegionDiceBCE', 'RegionDiceFocal')
    a = build_loss('RegionDiceBCE', 4, None, 2, regions=BRATS, dice_weight=0.7, ce_weight=1.3, batch_dice=True,
                   ignore_label=255, include_background=False)
    assert type(a) is RegionDiceBCELoss and (a.gamma, a.dice_weight, a.bce_weight, a.batch_dice, a.ignore_label) == \
        (0.0, 0.7, 1.3, True, 255.0)
    b = build_loss('RegionDiceFocal', 4, [1, 2, 3], 1.5, regions=BRATS)
    assert type(b) is RegionDiceBCELoss and b.gamma == 1.5 and b.bce_weights.tolist() == [1, 2, 3]
    for name in REGION_LOSSES:
        with pytest.raises(ValueError, match='needs regions'):
            build_loss(name, 4)
    for name in ('Dice', 'Focal', 'CE', 'DiceCE', 'DiceFocal', 'DiceTopK', 'DiceBoundary', 'DiceClDice'):
        with pytest.raises(ValueError, match='takes no regions'):
            build_loss(name, 4, regions=BRATS)
    with pytest.raises(ValueError, match='Unknown loss function'):
        build_loss('DiceBCE', 4)


def test_config_keys():
    plain = types.SimpleNamespace(name='DiceCE', dice_weight=0.5)
    assert regions_from_config(plain) == (None, None)
    assert loss_options_from_config(plain) == {'dice_weight': 0.5, 'ce_weight': 1.0, 'include_background': True,
                                               'batch_dice': False, 'ignore_label': None}
    both = types.SimpleNamespace(name='RegionDiceBCE', regions=[(3, 1, 2), (3, 1), (3,)], region_class_order=[2, 1, 3],
                                 ce_weight=0.5)
    assert regions_from_config(both) == (BRATS, [2, 1, 3])
    opts = loss_options_from_config(both)
    assert opts['regions'] == BRATS and 'region_class_order' not in opts
    loss = build_loss(both.name, 4, None, 2, **opts)
    assert type(loss) is RegionDiceBCELoss and loss.bce_weight == 0.5
    for bad in (dict(regions=BRATS), dict(region_class_order=[1, 2, 3]), dict(regions=BRATS, region_class_order=[1, 2]),
                dict(regions=[[0]], region_class_order=[1]), dict(regions=BRATS, region_class_order=[1, 2, 200])):
        with pytest.raises(ValueError):
            regions_from_config(types.SimpleNamespace(name='RegionDiceBCE', **bad))
        with pytest.raises(ValueError):
            loss_options_from_config(types.SimpleNamespace(name='RegionDiceBCE', **bad))


def test_shipped_configs_load_unchanged():
    from segmentation3d.utils.file_io import load_config
    folder = os.path.join(PKG, 'segmentation3d', 'config')
    cfg = load_config(os.path.join(folder, 'train_config.py'))
    assert 'regions' not in dict(cfg.loss) and 'region_class_order' not in dict(cfg.loss)
    assert regions_from_config(cfg.loss) == (None, None)
    assert sorted(loss_options_from_config(cfg.loss)) == ['batch_dice', 'ce_weight', 'dice_weight', 'ignore_label',
                                                          'include_background']
    load_config(os.path.join(folder, 'infer_config.py'))


def test_train_step_refuses_mismatched_names_and_deep_supervision():
    """every refusal comes before anything is built, so no device is needed"""
    for name in ('Dice', 'Focal', 'CE', 'DiceCE', 'DiceFocal', 'DiceTopK', 'DiceBoundary', 'DiceClDice'):
        with pytest.raises(ValueError, match='takes no regions'):
            TrainStep('vnet', 1, 4, loss_name=name, regions=BRATS, region_class_order=[2, 1, 3])
    for name in REGION_LOSSES:
        with pytest.raises(ValueError, match='needs regions'):
            TrainStep('vnet', 1, 4, loss_name=name)
        with pytest.raises(ValueError, match='deep supervision'):
            TrainStep('vnet', 1, 4, loss_name=name, regions=BRATS, region_class_order=[2, 1, 3], deep_supervision=1)
        with pytest.raises(ValueError):       # the order is required with the regions
            TrainStep('vnet', 1, 4, loss_name=name, regions=BRATS)
        with pytest.raises(ValueError):
            TrainStep('vnet', 1, 4, loss_name=name, regions=BRATS, region_class_order=[1, 2])
        with pytest.raises(ValueError):
            TrainStep('vnet', 1, 4, loss_name=name, regions=[[0]], region_class_order=[1])
    with pytest.raises(ValueError, match='without regions'):
        TrainStep('vnet', 1, 4, loss_name='DiceCE', region_class_order=[1, 2, 3])


# ---- validation ----------------------------------------------------------------------------------------------------------------
def test_validator_argument_checks():
    crops, masks = torch.zeros((2, 1, 4, 4, 4)), torch.zeros((2, 1, 4, 4, 4))
    v = Validator(None, None, crops, masks, 2, regions=[(3, 1, 2), (1, 3), (3,)])
    assert v.regions == BRATS and v._lut == region_lut(BRATS)
    assert Validator(None, None, crops, masks, 2).regions is None
    for bad in ([], [[0]], [[1, 1]], 'x', [[1]] * 17):
        with pytest.raises(ValueError):
            Validator(None, None, crops, masks, 2, regions=bad)
    assert validate_validation({'imseg_list': 'val.txt'}, 4)['ema'] == 0.9


def test_mean_region_dice_runs_over_all_regions():
    from segmentation3d.utils.metrics import dice_from_counts, mean_foreground_dice, mean_region_dice
    counts = [[2, 1, 1], [0, 0, 0], [3, 0, 1]]
    d = dice_from_counts(counts)
    assert d[0] == 4 / 6 and math.isnan(d[1]) and d[2] == 6 / 7
    assert mean_region_dice(counts) == (4 / 6 + 6 / 7) / 2          # row 0 is a region, not a background class
    assert mean_foreground_dice(counts) == 6 / 7
    assert math.isnan(mean_region_dice([[0, 0, 0]]))
