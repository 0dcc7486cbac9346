"""CPU-side checks of the Dice + clDice loss: closed forms of the float64 oracle that the GPU
tests compare against, the module's argument checks, build_loss and the optional config keys."""
import os
import types

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from cldice_oracle import cldice_oracle, soft_skeleton_oracle
from segmentation3d.core.seg_train import build_loss, loss_options_from_config
from segmentation3d.loss.cldice_loss import DiceClDiceLoss, cldice_class_list
from segmentation3d.loss.compound_loss import DiceCELoss


# ---- the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('iters', [1, 3, 16])
def test_a_one_voxel_wide_line_is_its_own_skeleton(iters):
    x = torch.zeros(9, 9, 11, dtype=torch.float64)
    x[4, 4, 2:9] = 1.0
    assert torch.equal(soft_skeleton_oracle(x, iters), x)


def test_ball_of_radius_4():
    """empty for k = 1 and 3 (the erosions have not reached the centre), exactly the centre voxel for k = 8"""
    zz, yy, xx = np.meshgrid(np.arange(15), np.arange(15), np.arange(15), indexing='ij')
    ball = torch.from_numpy((((zz - 7) ** 2 + (yy - 7) ** 2 + (xx - 7) ** 2) <= 16).astype(np.float64))
    assert float(soft_skeleton_oracle(ball, 1).abs().max()) == 0.0
    assert float(soft_skeleton_oracle(ball, 3).abs().max()) == 0.0
    centre = torch.zeros_like(ball)
    centre[7, 7, 7] = 1.0
    assert torch.equal(soft_skeleton_oracle(ball, 8), centre)


def test_a_constant_plane_has_no_skeleton():
    x = torch.full((2, 5, 6, 7), 0.37, dtype=torch.float64)
    assert float(soft_skeleton_oracle(x, 3).abs().max()) == 0.0


def test_prediction_equal_to_a_binary_target_has_no_cldice_loss():
    g = torch.Generator().manual_seed(3)
    t = (torch.rand((2, 1, 6, 8, 9), generator=g) < 0.4).float()
    p = torch.cat([1.0 - t, t], dim=1)
    total, l_dice, l_cl = cldice_oracle(p, t, iters=3)
    assert float(l_cl) == 0.0
    assert abs(float(l_dice)) < 1e-9 and float(total) == float(l_dice)


def test_uncounted_voxels_get_no_gradient_from_the_oracle():
    g = torch.Generator().manual_seed(4)
    p = torch.rand((1, 3, 5, 6, 7), generator=g, dtype=torch.float64).requires_grad_(True)
    t = torch.randint(0, 3, (1, 1, 5, 6, 7), generator=g).float()
    t[:, :, 2] = 255.0
    total, _, _ = cldice_oracle(p, t, ignore_label=255, iters=2)
    (grad,) = torch.autograd.grad(total, p)
    assert float(grad[:, :, 2].abs().max()) == 0.0 and float(grad.abs().max()) > 0.0


# ---- the module ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kwargs', [
    dict(weights=[1.0, -1.0, 1.0]), dict(weights=[1.0, 0.0, 1.0]), dict(weights=[1.0, 1.0]),
    dict(weights=[1.0, float('inf'), 1.0]),
    dict(iters=0), dict(iters=17), dict(iters=2.5),
    dict(dice_weight=0.0, cldice_weight=0.0), dict(dice_weight=-1.0), dict(cldice_weight=float('nan')),
    dict(cldice_classes=[]), dict(cldice_classes=[1, 1]), dict(cldice_classes=[0, 1]), dict(cldice_classes=[3]),
    dict(cldice_classes=[-1]),
], ids=lambda k: '-'.join('{}={}'.format(a, b) for a, b in k.items()))
def test_constructor_refuses(kwargs):
    with pytest.raises(ValueError):
        DiceClDiceLoss(3, **kwargs)


def test_constructor_refuses_class_counts():
    for c in (1, 17):
        with pytest.raises(ValueError):
            DiceClDiceLoss(c)


def test_defaults_and_class_list():
    loss = DiceClDiceLoss(4)
    assert (loss.dice_weight, loss.cldice_weight, loss.iters) == (1.0, 1.0, 3)
    assert loss.cldice_classes == [1, 2, 3] and loss.last_terms is None
    assert torch.allclose(loss.cldice_weights, torch.full((3,), 1.0 / 3.0))
    loss = DiceClDiceLoss(4, weights=[5.0, 1.0, 2.0, 3.0], cldice_classes=(3, 1), include_background=False)
    assert loss.cldice_classes == [3, 1]
    assert torch.allclose(loss.cldice_weights, torch.tensor([0.75, 0.25]))          # normalised over K, in K's order
    assert torch.allclose(loss.region_weights, torch.tensor([0.0, 1.0, 2.0, 3.0]) / 6.0)
    assert cldice_class_list(2, None) == [1]


def test_forward_refuses_bad_shapes_before_it_needs_a_device():
    loss = DiceClDiceLoss(2)
    with pytest.raises(ValueError):
        loss(torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(ValueError):
        loss(torch.zeros(1, 2, 4, 4), torch.zeros(1, 1, 4, 4))
    with pytest.raises(ValueError):
        loss(torch.zeros(1, 2, 4, 4, 4), torch.zeros(1, 1, 4, 4, 5))
    with pytest.raises(ValueError):
        loss(torch.zeros(1, 2, 1, 1, 257), torch.zeros(1, 1, 1, 1, 257))


def test_build_loss_selects_it():
    loss = build_loss('DiceClDice', 3, [1.0, 2.0, 3.0], dice_weight=0.5, include_background=False, batch_dice=True,
                      ignore_label=255, cldice_weight=0.2, cldice_iters=5, cldice_classes=[2])
    assert isinstance(loss, DiceClDiceLoss)
    assert (loss.dice_weight, loss.cldice_weight, loss.iters, loss.cldice_classes) == (0.5, 0.2, 5, [2])
    assert (loss.include_background, loss.batch_dice, loss.ignore_label) == (False, True, 255.0)
    assert isinstance(build_loss('DiceClDice', 2), DiceClDiceLoss)
    # the new keywords are ignored by the other losses
    other = build_loss('DiceCE', 2, cldice_weight=0.2, cldice_iters=5, cldice_classes=[1])
    assert type(other) is DiceCELoss
    with pytest.raises(ValueError):
        build_loss('DiceClDice', 2, cldice_iters=0)
    with pytest.raises(ValueError):
        build_loss('DiceClDice', 2, cldice_classes=[2])


def test_config_keys_are_optional():
    plain = types.SimpleNamespace(name='DiceClDice')
    opts = loss_options_from_config(plain)
    assert not any(k.startswith('cldice') for k in opts)
    loss = build_loss('DiceClDice', 3, **opts)
    assert (loss.cldice_weight, loss.iters, loss.cldice_classes) == (1.0, 3, [1, 2])
    with_keys = types.SimpleNamespace(name='DiceClDice', cldice_weight=0.3, cldice_iters=7, cldice_classes=[2],
                                      ignore_label=255)
    opts = loss_options_from_config(with_keys)
    assert (opts['cldice_weight'], opts['cldice_iters'], opts['cldice_classes'], opts['ignore_label']) == (0.3, 7, [2], 255)
    loss = build_loss('DiceClDice', 3, **opts)
    assert (loss.cldice_weight, loss.iters, loss.cldice_classes, loss.ignore_label) == (0.3, 7, [2], 255.0)
    one_key = loss_options_from_config(types.SimpleNamespace(name='DiceClDice', cldice_iters=2))
    assert one_key['cldice_iters'] == 2 and 'cldice_weight' not in one_key and 'cldice_classes' not in one_key


def test_a_config_without_the_keys_builds_what_it_built_before():
    """the options of a section without the new keys are exactly the five the compound losses had, and the shipped
    training config has none of the new keys"""
    opts = loss_options_from_config(types.SimpleNamespace(name='DiceCE', dice_weight=0.5))
    assert opts == {'dice_weight': 0.5, 'ce_weight': 1.0, 'include_background': True, 'batch_dice': False,
                    'ignore_label': None}
    assert type(build_loss('DiceCE', 2, **opts)) is DiceCELoss
    import segmentation3d
    from segmentation3d.utils.file_io import load_config
    shipped = load_config(os.path.join(os.path.dirname(segmentation3d.__file__), 'config', 'train_config.py'))
    assert 'name' in dict(shipped.loss) and not any(k.startswith('cldice') for k in dict(shipped.loss))
