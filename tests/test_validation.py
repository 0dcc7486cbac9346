"""Host side of the online validation: Dice from confusion counts, the moving average and its
state, the `validation` section's checks, checkpoint selection next to a `best` folder.  No GPU."""
import math
import os

import pytest
import torch

from conftest import PKG  # noqa: F401  (sys.path)


def test_dice_from_counts_hand_worked():
    from segmentation3d.utils.metrics import dice_from_counts, mean_foreground_dice
    counts = [[90, 5, 5], [3, 1, 2], [0, 4, 0], [0, 0, 0]]          # (tp, fp, fn)
    dice = dice_from_counts(counts)
    assert dice[0] == 180.0 / 190.0 and dice[1] == 6.0 / 9.0 and dice[2] == 0.0
    assert math.isnan(dice[3])                                        # neither labels nor prediction hold class 3
    assert all(isinstance(d, float) for d in dice)
    assert mean_foreground_dice(counts) == (6.0 / 9.0 + 0.0) / 2.0    # nan-mean over classes 1 .. C-1
    assert dice_from_counts(torch.tensor(counts))[:3] == dice[:3]                 # tensors, arrays and lists alike
    # every foreground class empty -> nan, whatever the background holds
    assert math.isnan(mean_foreground_dice([[10, 0, 0], [0, 0, 0], [0, 0, 0]]))
    # doubles on the host: counts beyond float32's integers stay exact
    big = 3 * 2 ** 40 + 1
    assert dice_from_counts([[0, 0, 0], [big, 1, 0]])[1] == (2.0 * big) / (2.0 * big + 1.0)
    with pytest.raises(ValueError):
        dice_from_counts([[1, 2]])


def test_ema_rule():
    from segmentation3d.core.seg_validate import DiceEma
    e = DiceEma(0.9)
    assert e.ema_dice is None and e.best_ema_dice is None
    assert e.update(float('nan'), 1) is False and e.ema_dice is None          # nothing to initialise from yet
    assert e.update(0.5, 2) is True and e.ema_dice == 0.5                     # the first finite value initialises
    assert e.update(0.7, 3) is True and e.ema_dice == 0.9 * 0.5 + 0.1 * 0.7   # then a * ema + (1 - a) * mean
    before = e.ema_dice
    assert e.update(float('nan'), 4) is False and e.ema_dice == before        # nan leaves it unchanged
    assert e.update(0.1, 5) is False and e.ema_dice == 0.9 * before + 0.1 * 0.1   # a fall is no gain
    assert e.update(0.0, 6) is False and e.best_epoch == 3 and e.best_ema_dice == before
    flat = DiceEma(0.0)                                                       # a = 0: the average is the last value
    assert flat.update(0.4, 1) is True and flat.update(0.4, 2) is False       # equal is not a strict gain
    assert flat.update(0.41, 3) is True and flat.best_epoch == 3
    for bad in (1.0, -0.1, 1.5, 'x', None, True):
        with pytest.raises(ValueError):
            DiceEma(bad)


def test_validator_state_dict_round_trip():
    from segmentation3d.core.seg_validate import Validator
    crops, masks = torch.zeros(2, 1, 4, 4, 4), torch.zeros(2, 1, 4, 4, 4)
    a = Validator(None, None, crops, masks, 1, ema=0.5)
    assert a.state_dict() == {'ema_dice': None, 'best_ema_dice': None, 'best_epoch': None}
    a.tracker.update(0.6, 4)
    a.tracker.update(0.2, 5)
    state = a.state_dict()
    assert state == {'ema_dice': 0.4, 'best_ema_dice': 0.6, 'best_epoch': 4}
    b = Validator(None, None, crops, masks, 1, ema=0.5)
    b.load_state_dict(state)
    assert b.state_dict() == state
    assert b.tracker.update(0.7, 6) is False and b.tracker.ema_dice == 0.5 * 0.4 + 0.5 * 0.7   # continues, best stays 0.6
    assert b.tracker.update(0.9, 7) is True and b.tracker.best_epoch == 7
    with pytest.raises(ValueError):
        Validator(None, None, crops, masks[:1], 1)
    with pytest.raises(ValueError):
        Validator(None, None, crops, masks, 0)


def test_validate_validation():
    from segmentation3d.core.seg_validate import VALIDATION_DEFAULTS, validate_validation
    assert validate_validation(None) is None
    assert validate_validation({}) is None and validate_validation({'imseg_list': None, 'epochs': 2}) is None
    v = validate_validation({'imseg_list': '/data/val.txt'})
    assert v == dict(VALIDATION_DEFAULTS, imseg_list='/data/val.txt')
    assert v['epochs'] == 1 and v['crops_per_case'] == 4 and v['batchsize'] is None and v['seed'] == 0
    assert v['ema'] == 0.9 and v['save_best'] is True
    full = {'imseg_list': 'v.txt', 'epochs': 3, 'crops_per_case': 1, 'batchsize': 2, 'seed': 7, 'ema': 0.0,
            'save_best': False}
    assert validate_validation(full, num_classes=5) == full
    bad = [{'epoch': 1}, {'epochs': 0}, {'epochs': 1.5}, {'crops_per_case': 0}, {'crops_per_case': -3}, {'ema': 1.0},
           {'ema': -0.01}, {'ema': 'high'}, {'batchsize': 0}, {'seed': -1}, {'save_best': 1}, {'imseg_list': 5}]
    for extra in bad:
        with pytest.raises(ValueError):
            validate_validation(dict({'imseg_list': 'v.txt'}, **extra))
    with pytest.raises(ValueError):
        validate_validation({'epochs': 0})                 # a bad value raises even while validation is off
    with pytest.raises(ValueError):
        validate_validation({'imseg_list': 'v.txt'}, num_classes=1)
    with pytest.raises(ValueError):
        validate_validation(['imseg_list'])


def test_checkpoint_selection_next_to_best(tmp_path):
    from segmentation3d.utils.model_io import get_checkpoint_folder, select_checkpoint_folder
    root = tmp_path / 'checkpoints'
    for name in ('chk_2', 'chk_10', 'best'):
        os.makedirs(str(root / name))
    assert get_checkpoint_folder(str(root), -1) == str(root / 'chk_10')      # "latest" does not see `best`
    assert select_checkpoint_folder(str(root)) == str(root / 'chk_10')
    assert select_checkpoint_folder(str(root), 'latest') == str(root / 'chk_10')
    assert select_checkpoint_folder(str(root), 'best') == str(root / 'best')
    assert select_checkpoint_folder(str(root), 2) == str(root / 'chk_2')
    with pytest.raises(FileNotFoundError) as err:
        select_checkpoint_folder(str(root), 3)
    assert str(root / 'chk_3') in str(err.value)
    os.rmdir(str(root / 'best'))
    with pytest.raises(FileNotFoundError) as err:
        select_checkpoint_folder(str(root), 'best')
    assert str(root / 'best') in str(err.value)
    for bad in ('newest', -1, 1.0, True):
        with pytest.raises(ValueError):
            select_checkpoint_folder(str(root), bad)


def test_checkpoint_state_validation_key():
    from types import SimpleNamespace as ns
    from segmentation3d.utils.model_io import checkpoint_state
    cfg = ns(dataset=ns(spacing=[1, 1, 1], interpolation='LINEAR', num_classes=2, crop_normalizers=[None]),
             net=ns(name='vnet'))
    net = torch.nn.Linear(2, 2)
    plain = checkpoint_state(net, 3, 7, cfg, 16, 1)
    assert 'validation' not in plain
    state = {'ema_dice': 0.5, 'best_ema_dice': 0.6, 'best_epoch': 2}
    with_val = checkpoint_state(net, 3, 7, cfg, 16, 1, validation=state)
    assert with_val['validation'] == state and set(with_val) == set(plain) | {'validation'}


def test_shipped_configs_have_no_validation():
    folder = os.path.join(PKG, 'segmentation3d', 'config')
    assert 'validation' not in open(os.path.join(folder, 'train_config.py')).read()
    from segmentation3d.utils.file_io import load_config
    ic = load_config(os.path.join(folder, 'infer_config.py'))
    assert 'checkpoint' not in ic.coarse and 'checkpoint' not in ic.fine     # optional: named in a comment only
    assert 'checkpoint' in open(os.path.join(folder, 'infer_config.py')).read()
