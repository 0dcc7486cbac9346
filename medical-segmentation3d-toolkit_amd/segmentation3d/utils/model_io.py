"""Checkpoint layout of the reference (utils/model_io.py:7-92): `<model>/checkpoints/chk_<epoch>/{params.pth,
optimizer.pth}`; `params.pth` holds epoch, batch, net name, max_stride, state_dict, spacing, interpolation,
in/out channels and the crop normaliser dictionaries.  The format is the compatibility contract, so parameters stay in
the reference layouts inside `state_dict`; packed / NDHWC weights are derived on the device at run time.
"""
import glob
import os
import shutil
from collections import OrderedDict

import torch


def get_checkpoint_folder(chk_root, epoch):
    """folder of the checkpoint with the given epoch; epoch < 0 selects the latest `chk_<n>`"""
    assert os.path.isdir(chk_root), 'The folder does not exist: {}'.format(chk_root)
    if epoch < 0:
        epochs = [int(os.path.basename(p).split('_')[-1]) for p in glob.glob(os.path.join(chk_root, 'chk_*'))]
        epoch = max(epochs) if epochs else -1
    return os.path.join(chk_root, 'chk_{}'.format(epoch))


BEST_FOLDER = 'best'   # checkpoint of the best validation score (core/seg_validate.py); not `chk_*`: "latest" globs that


def select_checkpoint_folder(chk_root, selection='latest'):
    """folder named by the `checkpoint` key of an inference stage: 'latest' (or None; the largest `chk_<n>`), 'best'
    (`<chk_root>/best`, written by a run with validation) or an integer epoch; a folder that is not there raises with its path"""
    if selection is None or selection == 'latest':
        folder = get_checkpoint_folder(chk_root, -1)
    elif selection == BEST_FOLDER:
        folder = os.path.join(chk_root, BEST_FOLDER)
    elif isinstance(selection, int) and not isinstance(selection, bool) and selection >= 0:
        folder = get_checkpoint_folder(chk_root, selection)
    else:
        raise ValueError("checkpoint must be 'latest', 'best' or an epoch >= 0, got {!r}".format(selection))
    if not os.path.isdir(folder):
        raise FileNotFoundError('checkpoint folder not found: {}'.format(folder))
    return folder


def strip_module_prefix(state_dict):
    """DataParallel-trained checkpoints prefix every key with 'module.' (core/seg_infer.py:130-142)"""
    if not any(k.startswith('module.') for k in state_dict):
        return state_dict
    return OrderedDict((k[len('module.'):] if k.startswith('module.') else k, v) for k, v in state_dict.items())


DEEP_SUPERVISION_PREFIX = 'ds_out_'   # the auxiliary heads of network/_vnet_base.py: training only


def strip_deep_supervision(state_dict):
    """a copy of `state_dict` without the deep-supervision heads' entries: inference runs the main output only, so a
    deeply supervised checkpoint loads into a plain network"""
    if not any(k.startswith(DEEP_SUPERVISION_PREFIX) for k in state_dict):
        return state_dict
    return OrderedDict((k, v) for k, v in state_dict.items() if not k.startswith(DEEP_SUPERVISION_PREFIX))


def inference_state_dict(state_dict):
    """what an inference network loads from a checkpoint's `state_dict`: no 'module.' prefix, no auxiliary heads"""
    return strip_deep_supervision(strip_module_prefix(state_dict))


def _chk_dir(model_folder, epoch_idx):
    return os.path.join(model_folder, 'checkpoints', 'chk_{}'.format(epoch_idx))


def _read(path, what):
    assert os.path.isfile(path), '{} file not found: {}'.format(what, path)
    return torch.load(path, map_location='cpu', weights_only=True)   # plain tensors / containers only


def load_checkpoint(epoch_idx, net, opt, save_dir):
    """restore network + optimizer from `<save_dir>/checkpoints/chk_<epoch_idx>`; returns (epoch, batch).  opt = None loads the
    network alone (inference): the auxiliary heads of a deeply supervised checkpoint are then dropped for a network without
    them.  With an optimizer (a training resume) the network must have the checkpoint's `deep_supervision`: the optimizer
    state covers exactly those parameters."""
    folder = _chk_dir(save_dir, epoch_idx)
    state = _read(os.path.join(folder, 'params.pth'), 'checkpoint')
    target = getattr(net, 'module', net)
    weights = strip_module_prefix(state['state_dict'])
    trained, built = int(state.get('deep_supervision', 0)), int(getattr(target, 'deep_supervision', 0))
    if opt is None and built == 0:
        weights = strip_deep_supervision(weights)     # inference: a network without the auxiliary heads takes the main path only
    elif trained != built:
        raise ValueError('the checkpoint was trained with deep_supervision = {} but the network was built with {}'.format(
            trained, built))
    trained_act, built_act = state.get('output_activation', 'softmax'), getattr(target, 'output_activation', 'softmax')
    if trained_act != built_act:
        raise ValueError('the checkpoint was trained with output_activation = {!r} but the network was built with {!r}'.format(
            trained_act, built_act))
    target.load_state_dict(weights)
    if opt is not None:
        opt.load_state_dict(_read(os.path.join(folder, 'optimizer.pth'), 'optimizer'))
    return state['epoch'], state['batch']


def checkpoint_deep_supervision(epoch_idx, save_dir):
    """the `deep_supervision` a checkpoint was trained with (0 for checkpoints written before the key existed)"""
    state = _read(os.path.join(_chk_dir(save_dir, epoch_idx), 'params.pth'), 'checkpoint')
    return int(state.get('deep_supervision', 0))


def region_keys(state):
    """(regions, region_class_order, output_activation) of a `params.pth` dictionary; a checkpoint written before the keys
    existed is an exclusive-class one: (None, None, 'softmax')"""
    return state.get('regions'), state.get('region_class_order'), state.get('output_activation', 'softmax')


def checkpoint_regions(epoch_idx, save_dir):
    """region_keys of the checkpoint `<save_dir>/checkpoints/chk_<epoch_idx>`"""
    return region_keys(_read(os.path.join(_chk_dir(save_dir, epoch_idx), 'params.pth'), 'checkpoint'))


def checkpoint_state(net, epoch_idx, batch_idx, cfg, max_stride, num_modality, regions=None, region_class_order=None,
                     validation=None):
    """the `params.pth` dictionary (fields of utils/model_io.py:75-84; tensors moved to the host); `regions` /
    `region_class_order` of a region-based run are stored next to the channel counts (out_channels is then the number of
    regions) with the head's activation;
    `validation` (a Validator's state dict) adds the key of that name, a run without validation keeps the key set"""
    weights = OrderedDict((key, value.detach().cpu()) for key, value in net.state_dict().items())
    geometry = {'spacing': cfg.dataset.spacing, 'interpolation': cfg.dataset.interpolation, 'max_stride': max_stride}
    channels = {'in_channels': num_modality,   # a region-based network has one output per region
                'out_channels': cfg.dataset.num_classes if regions is None else len(regions),
                'deep_supervision': int(getattr(getattr(net, 'module', net), 'deep_supervision', 0))}
    state = {'epoch': epoch_idx, 'batch': batch_idx, 'net': cfg.net.name, 'state_dict': weights,
             'crop_normalizers': [None if n is None else n.to_dict() for n in cfg.dataset.crop_normalizers]}
    state.update(geometry)
    state.update(channels)
    state['regions'] = None if regions is None else [[int(l) for l in r] for r in regions]
    state['region_class_order'] = None if region_class_order is None else [int(l) for l in region_class_order]
    state['output_activation'] = str(getattr(getattr(net, 'module', net), 'output_activation', 'softmax'))
    if validation is not None:
        state['validation'] = dict(validation)
    return state


def save_checkpoint(net, opt, epoch_idx, batch_idx, cfg, max_stride, num_modality, regions=None, region_class_order=None,
                    validation=None, folder_name=None):
    """write params.pth / optimizer.pth (+ a copy of train_config.py) for `epoch_idx` into `chk_<epoch_idx>`, or into
    `checkpoints/<folder_name>` (the best-validation checkpoint); returns the folder"""
    model_folder = os.path.join(cfg.general.save_dir, cfg.general.model_scale)
    folder = _chk_dir(model_folder, epoch_idx) if folder_name is None else os.path.join(model_folder, 'checkpoints',
                                                                                        folder_name)
    os.makedirs(folder, exist_ok=True)
    torch.save(checkpoint_state(net, epoch_idx, batch_idx, cfg, max_stride, num_modality, regions, region_class_order,
                                validation), os.path.join(folder, 'params.pth'))
    torch.save(opt.state_dict(), os.path.join(folder, 'optimizer.pth'))
    config_copy = os.path.join(model_folder, 'train_config.py')
    if os.path.isfile(config_copy):
        shutil.copy(config_copy, os.path.join(folder, 'train_config.py'))
    return folder


def checkpoint_validation(epoch_idx, save_dir):
    """the Validator state dict stored in `chk_<epoch_idx>/params.pth`, None for a run without validation"""
    return _read(os.path.join(_chk_dir(save_dir, epoch_idx), 'params.pth'), 'checkpoint').get('validation')
