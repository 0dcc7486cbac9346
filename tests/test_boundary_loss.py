"""The Dice + boundary loss without a GPU: the float64 oracle (tests/boundary_oracle.py) pinned against hand-computed
maps and an independent transform, the module's argument checks, build_loss, the config keys and the weight schedule."""
import math
import types

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (puts the package on sys.path)
from boundary_oracle import boundary_oracle, signed_distance_oracle
from segmentation3d.core.seg_train import (TrainStep, boundary_schedule_from_config, build_loss,
                                           loss_options_from_config)
from segmentation3d.loss.boundary_loss import DiceBoundaryLoss
from segmentation3d.loss.compound_loss import DiceCELoss


# ---- the oracle against hand-computed maps ------------------------------------------------------------------------------
def test_oracle_on_a_line():
    """1 x 5 line, spacing 2 mm along x: G = {2, 3} for class 1"""
    t = np.array([0, 0, 1, 1, 0], dtype=np.float64).reshape(1, 1, 1, 5)
    phi = signed_distance_oracle(t, [1, 0], (2.0, 1.0, 1.0))
    assert phi.shape == (1, 2, 1, 1, 5)
    assert phi[0, 0].ravel().tolist() == [4.0, 2.0, -2.0, -2.0, 2.0]
    assert phi[0, 1].ravel().tolist() == [-4.0, -2.0, 2.0, 2.0, -2.0]      # the complement has the opposite sign
    # an ignored voxel is neither G nor H: no query, no feature, no boundary
    t[0, 0, 0, 1] = 255
    phi = signed_distance_oracle(t, [1], (2.0, 1.0, 1.0), num_class=2, ignore_label=255)
    assert phi[0, 0].ravel().tolist() == [4.0, 0.0, -4.0, -2.0, 2.0]
    # out-of-range ids do not count either; a class that is absent, or is everything, gives zeros
    t2 = np.array([0, 2, 1, -1, 0], dtype=np.float64).reshape(1, 1, 1, 5)
    assert signed_distance_oracle(t2, [1], (1, 1, 1), num_class=2)[0, 0].ravel().tolist() == [2.0, 0.0, -2.0, 0.0, 2.0]
    assert not signed_distance_oracle(t2, [3], (1, 1, 1), num_class=5).any()
    assert not signed_distance_oracle(np.ones((1, 1, 1, 5)), [1], (1, 1, 1)).any()


@pytest.mark.parametrize('spacing', [(1.0, 1.0, 1.0), (1.0, 2.0, 3.0)])
def test_oracle_on_a_cube(spacing):
    """3 x 3 x 3 with the centre voxel as the object: -(smallest spacing) inside, the centre distance outside"""
    t = np.zeros((1, 3, 3, 3))
    t[0, 1, 1, 1] = 1
    phi, d2 = signed_distance_oracle(t, [1], spacing, squared=True)
    sx, sy, sz = spacing
    for z in range(3):
        for y in range(3):
            for x in range(3):
                want = math.sqrt((sx * (x - 1)) ** 2 + (sy * (y - 1)) ** 2 + (sz * (z - 1)) ** 2)
                if (z, y, x) == (1, 1, 1):
                    want = -min(spacing)
                assert phi[0, 0, z, y, x] == pytest.approx(want, rel=1e-15)
                assert d2[0, 0, z, y, x] == pytest.approx(want * want, rel=1e-15)


def test_oracle_against_scipy():
    ndi = pytest.importorskip('scipy.ndimage')
    rng = np.random.RandomState(3)
    t = rng.randint(0, 3, size=(2, 5, 7, 9)).astype(np.float64)
    spacing = (0.7, 1.3, 2.5)
    phi = signed_distance_oracle(t, [0, 1, 2], spacing)
    for n in range(2):
        for c in range(3):
            m = t[n] == c
            want = ndi.distance_transform_edt(~m, sampling=spacing[::-1]) - ndi.distance_transform_edt(m, sampling=spacing[::-1])
            assert np.abs(phi[n, c] - want).max() < 1e-12


def test_loss_oracle_by_hand():
    """one sample, two voxels: t = (0, 1), unit spacing: phi_0 = (-1, +1), phi_1 = (+1, -1)"""
    p = torch.tensor([0.8, 0.3, 0.2, 0.7], dtype=torch.float64).reshape(1, 2, 1, 1, 2).requires_grad_(True)
    t = torch.tensor([0.0, 1.0]).reshape(1, 1, 1, 1, 2)
    phi = signed_distance_oracle(t[:, 0].numpy(), [0, 1], (1, 1, 1), num_class=2)
    total, region, boundary = boundary_oracle(p, t, phi, dice_weight=1.0, boundary_weight=0.5)
    want = 0.5 * ((-0.8 + 0.3) + (0.2 - 0.7)) / 2.0
    (g,) = torch.autograd.grad(boundary, p)
    assert float(boundary.detach()) == pytest.approx(want, rel=1e-15)
    assert float(total.detach()) == pytest.approx(float(region.detach()) + 0.5 * want, rel=1e-15)
    assert g.reshape(-1).tolist() == pytest.approx([-0.25, 0.25, 0.25, -0.25])
    # without the background only class 1's map enters, with weight 1
    _, _, b1 = boundary_oracle(p, t, phi[:, 1:], include_background=False)
    assert float(b1.detach()) == pytest.approx((0.2 - 0.7) / 2.0, rel=1e-15)


# ---- the module -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kwargs', [
    dict(num_class=0), dict(num_class=17), dict(weights=[1.0]), dict(weights=[1.0, 0.0]), dict(weights=[1.0, -2.0]),
    dict(weights=[1.0, float('nan')]), dict(dice_weight=-1.0), dict(dice_weight=float('inf')),
    dict(boundary_weight=-0.1), dict(boundary_weight=float('nan')), dict(boundary_weight=float('inf')),
    dict(spacing=(1, 1)), dict(spacing=(1, 1, 1, 1)), dict(spacing=(1, 0, 1)), dict(spacing=(1, -1, 1)),
    dict(spacing=(1, float('inf'), 1)), dict(spacing=(1, float('nan'), 1)), dict(spacing=1.0), dict(spacing=(1, 1, 1e9)),
    dict(num_class=1, include_background=False),
])
def test_constructor_refuses(kwargs):
    args = dict(num_class=2)
    args.update(kwargs)
    with pytest.raises(ValueError):
        DiceBoundaryLoss(**args)


def test_forward_refuses_bad_shapes_before_it_needs_a_device():
    loss = DiceBoundaryLoss(2)
    with pytest.raises(ValueError):
        loss(torch.zeros(1, 3, 2, 2, 2), torch.zeros(1, 1, 2, 2, 2))       # wrong channel count
    with pytest.raises(ValueError):
        loss(torch.zeros(1, 2, 2, 2, 2), torch.zeros(1, 1, 2, 2, 3))       # target does not match
    with pytest.raises(ValueError):
        loss(torch.zeros(1, 2, 1, 1, 257), torch.zeros(1, 1, 1, 1, 257))   # an axis above 256
    with pytest.raises(ValueError):
        loss(torch.zeros(2, 2, 8), torch.zeros(2, 1, 8))                   # not a volume


def test_weight_setter_and_defaults():
    loss = DiceBoundaryLoss(3, weights=[1.0, 2.0, 1.0], include_background=False, spacing=[0.5, 1, 2])
    assert loss.boundary_weight == 0.01 and loss.dice_weight == 1.0 and loss.spacing == (0.5, 1.0, 2.0)
    assert loss.region_weights.tolist() == pytest.approx([0.0, 2.0 / 3.0, 1.0 / 3.0])
    assert loss.last_terms is None
    loss.set_boundary_weight(0.25)
    assert loss.boundary_weight == 0.25
    loss.set_boundary_weight(0)
    assert loss.boundary_weight == 0.0
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            loss.set_boundary_weight(bad)
    assert loss.boundary_weight == 0.0


def test_build_loss_selects_it():
    loss = build_loss('DiceBoundary', 3, [1.0, 2.0, 3.0], dice_weight=0.5, include_background=False, batch_dice=True,
                      ignore_label=255, boundary_weight=0.2, spacing=(0.7, 1.3, 2.5))
    assert isinstance(loss, DiceBoundaryLoss)
    assert (loss.dice_weight, loss.boundary_weight, loss.spacing) == (0.5, 0.2, (0.7, 1.3, 2.5))
    assert (loss.include_background, loss.batch_dice, loss.ignore_label) == (False, True, 255.0)
    assert isinstance(build_loss('DiceBoundary', 2), DiceBoundaryLoss)
    # the new keywords are ignored by the other losses
    other = build_loss('DiceCE', 2, boundary_weight=0.2, spacing=(2, 2, 2))
    assert type(other) is DiceCELoss
    with pytest.raises(ValueError):
        build_loss('DiceBoundary', 2, spacing=(1, 1, 0))


def test_config_keys_are_optional():
    plain = types.SimpleNamespace(name='DiceBoundary')
    opts = loss_options_from_config(plain)
    assert 'boundary_weight' not in opts and 'spacing' not in opts
    assert build_loss('DiceBoundary', 2, **opts).boundary_weight == 0.01
    with_key = types.SimpleNamespace(name='DiceBoundary', boundary_weight=0.05, ignore_label=255)
    opts = loss_options_from_config(with_key)
    assert opts['boundary_weight'] == 0.05 and opts['ignore_label'] == 255
    assert build_loss('DiceBoundary', 2, **opts).boundary_weight == 0.05


def test_schedule_values_clamp_and_bad_keys():
    w = boundary_schedule_from_config(types.SimpleNamespace())
    assert [w(e) for e in (0, 1, 100)] == [0.01, 0.01, 0.01]                # defaults: a constant weight
    w = boundary_schedule_from_config(types.SimpleNamespace(boundary_weight=0.01, boundary_weight_step=0.01,
                                                            boundary_weight_max=0.05))
    assert [w(e) for e in range(7)] == pytest.approx([0.01, 0.02, 0.03, 0.04, 0.05, 0.05, 0.05])
    assert w(4) == 0.05 and w(1000) == 0.05                                  # the clamp is exact
    assert w(3) == w(3)                                                      # no state: a resumed run continues it
    w = boundary_schedule_from_config(types.SimpleNamespace(boundary_weight=0.0, boundary_weight_step=0.5))
    assert [w(e) for e in range(4)] == [0.0, 0.5, 1.0, 1.0]                  # default maximum 1.0
    for bad in (dict(boundary_weight=-0.01), dict(boundary_weight=float('nan')), dict(boundary_weight_step=-1.0),
                dict(boundary_weight_step=float('inf')), dict(boundary_weight_max=-1.0),
                dict(boundary_weight_max=float('nan')), dict(boundary_weight=2.0),
                dict(boundary_weight=0.5, boundary_weight_max=0.1)):
        with pytest.raises(ValueError):
            boundary_schedule_from_config(types.SimpleNamespace(**bad))


def test_train_step_refuses_deep_supervision():
    """raised before a device or a network is needed"""
    with pytest.raises(ValueError, match='deep supervision'):
        TrainStep('vnet', 1, 2, loss_name='DiceBoundary', deep_supervision=1)
