"""Training engine -- MI355X-native replacement of the hot loop of the reference's core/seg_train.py:110-127
(zero_grad -> net(crops) -> loss(outputs, masks) -> backward -> Adam step) and of its `nn.DataParallel` wrap (:76-78).

`TrainStep` is the unit both `train()` and bench.py drive: one process per GPU, the network's 3-D conv / GroupNorm /
loss / Adam arithmetic in HIP kernels, gradients exchanged with a bucketed RCCL all-reduce overlapped with backward
(core/ddp.py) when torch.distributed is initialised.
"""
import importlib
import gc
import json
import math
import os
import shutil
import time

import numpy as np
import torch
import torch.distributed as dist

from segmentation3d import _ops
from segmentation3d.core.ddp import GradientReducer
from segmentation3d.loss.boundary_loss import DiceBoundaryLoss
from segmentation3d.loss.cldice_loss import DiceClDiceLoss
from segmentation3d.loss.compound_loss import DiceCELoss
from segmentation3d.loss.cross_entropy_loss import CrossEntropyLoss
from segmentation3d.loss.deep_supervision_loss import DeepSupervisionLoss, normalise_level_weights
from segmentation3d.loss.focal_loss import FocalLoss
from segmentation3d.loss.multi_dice_loss import MultiDiceLoss
from segmentation3d.loss.region_loss import RegionDiceBCELoss, check_region_class_order, check_regions
from segmentation3d.loss.topk_loss import DiceTopKLoss
from segmentation3d.optim.fused_adam import FusedAdam
from segmentation3d.optim.fused_sgd import FusedSGD


REGION_LOSSES = ('RegionDiceBCE', 'RegionDiceFocal')


def build_loss(name, num_classes, obj_weight=None, focal_gamma=2, use_gpu=True, dice_weight=1.0, ce_weight=1.0,
               include_background=True, batch_dice=False, ignore_label=None, topk_percent=10.0, boundary_weight=0.01,
               spacing=(1, 1, 1), cldice_weight=1.0, cldice_iters=3, cldice_classes=None, regions=None):
    """loss selection of core/seg_train.py:91-102, plus the compound losses 'DiceCE' (soft Dice + cross-entropy),
    'DiceFocal' (soft Dice + focal with focal_gamma), 'DiceTopK' (soft Dice + cross-entropy over the hardest
    topk_percent of the batch's voxels) and 'DiceBoundary' (soft Dice + boundary loss on signed distance maps in units of
    `spacing`, weighted by boundary_weight; ce_weight is not read) and 'DiceClDice' (soft Dice + soft-clDice topology
    loss on soft skeletons of cldice_iters iterations for the classes cldice_classes, weighted by cldice_weight; ce_weight
    is not read); the keyword options after use_gpu apply to those five only, topk_percent to 'DiceTopK' only,
    boundary_weight and spacing to 'DiceBoundary' only, the cldice_ options to 'DiceClDice' only.
    'RegionDiceBCE' and 'RegionDiceFocal' (focal_gamma) are the losses of a region-based model (loss/region_loss.py): they
    need `regions`, obj_weight then has one weight per region, ce_weight is the weight of the BCE term, and num_classes and
    include_background are not read (a region-based model has no background channel); no other loss takes `regions`"""
    if name in REGION_LOSSES:
        if regions is None:
            raise ValueError('loss {!r} needs regions'.format(name))
        return RegionDiceBCELoss(regions, weights=obj_weight, dice_weight=dice_weight, bce_weight=ce_weight,
                                 gamma=focal_gamma if name == 'RegionDiceFocal' else 0.0, batch_dice=batch_dice,
                                 ignore_label=ignore_label)
    if regions is not None:
        raise ValueError('loss {!r} takes no regions (RegionDiceBCE and RegionDiceFocal do)'.format(name))
    if name == 'DiceClDice':
        return DiceClDiceLoss(num_classes, weights=obj_weight, dice_weight=dice_weight, cldice_weight=cldice_weight,
                              iters=cldice_iters, cldice_classes=cldice_classes, include_background=include_background,
                              batch_dice=batch_dice, ignore_label=ignore_label, use_gpu=use_gpu)
    if name == 'DiceBoundary':
        return DiceBoundaryLoss(num_classes, weights=obj_weight, dice_weight=dice_weight, boundary_weight=boundary_weight,
                                spacing=spacing, include_background=include_background, batch_dice=batch_dice,
                                ignore_label=ignore_label, use_gpu=use_gpu)
    if name == 'DiceTopK':
        return DiceTopKLoss(num_classes, weights=obj_weight, dice_weight=dice_weight, ce_weight=ce_weight,
                            k_percent=topk_percent, include_background=include_background, batch_dice=batch_dice,
                            ignore_label=ignore_label, use_gpu=use_gpu)
    if name in ('DiceCE', 'DiceFocal'):
        return DiceCELoss(num_classes, weights=obj_weight, dice_weight=dice_weight, ce_weight=ce_weight,
                          gamma=focal_gamma if name == 'DiceFocal' else 0.0, include_background=include_background,
                          batch_dice=batch_dice, ignore_label=ignore_label, use_gpu=use_gpu)
    if name == 'Focal':
        return FocalLoss(class_num=num_classes, alpha=obj_weight, gamma=focal_gamma, use_gpu=use_gpu)
    if name == 'Dice':
        weights = obj_weight if obj_weight is not None else [1.0 / num_classes] * num_classes
        return MultiDiceLoss(weights=weights, num_class=num_classes, use_gpu=use_gpu)
    if name == 'CE':
        return CrossEntropyLoss()
    raise ValueError('Unknown loss function')


def loss_options_from_config(loss_cfg):
    """the optional keys of the config's `loss` section that the compound losses read, with their defaults (a config
    without them -- every reference config -- loads unchanged); `topk_percent` ('DiceTopK'), `boundary_weight`
    ('DiceBoundary') and `cldice_weight`, `cldice_iters`, `cldice_classes` ('DiceClDice'; defaults 1.0, 3, None = every
    foreground class) are passed on only when the section has them, and so is `regions` (regions_from_config: checked,
    and only together with `region_class_order`)"""
    opts = {'dice_weight': getattr(loss_cfg, 'dice_weight', 1.0), 'ce_weight': getattr(loss_cfg, 'ce_weight', 1.0),
            'include_background': getattr(loss_cfg, 'include_background', True),
            'batch_dice': getattr(loss_cfg, 'batch_dice', False), 'ignore_label': getattr(loss_cfg, 'ignore_label', None)}
    if hasattr(loss_cfg, 'topk_percent'):
        opts['topk_percent'] = loss_cfg.topk_percent
    if hasattr(loss_cfg, 'boundary_weight'):
        opts['boundary_weight'] = loss_cfg.boundary_weight
    for key in ('cldice_weight', 'cldice_iters', 'cldice_classes'):
        if hasattr(loss_cfg, key):
            opts[key] = getattr(loss_cfg, key)
    regions, _ = regions_from_config(loss_cfg)
    if regions is not None:
        opts['regions'] = regions
    return opts


def regions_from_config(loss_cfg):
    """(regions, region_class_order) of the config's `loss` section -- the label-id sets a region-based model is trained on
    and the label inference writes for each of them -- or (None, None) when the section has neither key.  One key without
    the other and anything check_regions / check_region_class_order refuse raise ValueError."""
    regions, order = getattr(loss_cfg, 'regions', None), getattr(loss_cfg, 'region_class_order', None)
    if regions is None and order is None:
        return None, None
    if regions is None or order is None:
        raise ValueError('loss.regions and loss.region_class_order are required together')
    regions = check_regions(regions)
    return regions, check_region_class_order(order, len(regions))


def boundary_schedule_from_config(loss_cfg):
    """the weight of the boundary term of 'DiceBoundary' as a function of the epoch index, from three optional keys of the
    config's `loss` section: boundary_weight (w0, default 0.01), boundary_weight_step (default 0.0) and
    boundary_weight_max (default 1.0):  w(epoch) = min(max, w0 + step * epoch) -- Kervadec's "increase" strategy.  It keeps
    no state, so a resumed run continues it.  Bad values raise ValueError."""
    w0 = float(getattr(loss_cfg, 'boundary_weight', 0.01))
    step = float(getattr(loss_cfg, 'boundary_weight_step', 0.0))
    top = float(getattr(loss_cfg, 'boundary_weight_max', 1.0))
    for key, v in (('boundary_weight', w0), ('boundary_weight_step', step), ('boundary_weight_max', top)):
        if not (math.isfinite(v) and v >= 0.0):
            raise ValueError('loss.{} must be finite and >= 0, got {}'.format(key, v))
    if w0 > top:
        raise ValueError('loss.boundary_weight = {} is above loss.boundary_weight_max = {}'.format(w0, top))

    def weight(epoch):
        return min(top, w0 + step * max(0, int(epoch)))
    return weight


def optim_options_from_config(train_cfg, num_samples=None, world_size=1):
    """the optional keys of the config's `train` section that select and configure the optimizer, with defaults that
    reproduce the reference's run (Adam at one constant rate, no clipping: a config without them loads unchanged).
    Returns {'optimizer': 'Adam' | 'SGD', + TrainStep's `optim_options`}; `momentum` / `nesterov` are read by SGD only.
    `total_steps = None` means the whole run: ceil(epochs * num_samples / (batchsize * world_size))."""
    name = getattr(train_cfg, 'optimizer', 'Adam')
    if name not in ('Adam', 'SGD'):
        raise ValueError('Unknown optimizer {!r} (Adam or SGD)'.format(name))
    schedule = getattr(train_cfg, 'lr_schedule', 'constant')
    warmup_steps = int(getattr(train_cfg, 'warmup_steps', 0))
    lr_schedule = None
    if schedule != 'constant' or warmup_steps > 0:
        total_steps = getattr(train_cfg, 'total_steps', None)
        if total_steps is None:
            if num_samples is None:
                raise ValueError('train.total_steps is not set and the number of samples is unknown')
            total_steps = max(1, int(math.ceil(float(train_cfg.epochs) * num_samples /
                                               (train_cfg.batchsize * max(1, int(world_size))))))
        lr_schedule = {'name': schedule, 'total_steps': total_steps, 'warmup_steps': warmup_steps,
                       'power': getattr(train_cfg, 'lr_power', 0.9)}
    return {'optimizer': name, 'momentum': getattr(train_cfg, 'momentum', 0.99),
            'nesterov': getattr(train_cfg, 'nesterov', True), 'weight_decay': getattr(train_cfg, 'weight_decay', 0.0),
            'max_grad_norm': getattr(train_cfg, 'clip_grad_norm', None), 'lr_schedule': lr_schedule}


def deep_supervision_from_config(train_cfg):
    """the optional keys `train.deep_supervision` (number of auxiliary decoder levels, 0..3; default 0 = the reference's
    single full-resolution loss) and `train.deep_supervision_weights` (per-level weights, default None = halving per level)
    as TrainStep's keyword arguments"""
    weights = getattr(train_cfg, 'deep_supervision_weights', None)
    return {'deep_supervision': int(getattr(train_cfg, 'deep_supervision', 0)),
            'deep_supervision_weights': None if weights is None else list(weights)}


def build_validator(cfg, val_cfg, step, num_modality):
    """the Validator of a run whose config has a `validation` section (`val_cfg`: validate_validation's dict): the held-out
    cases go through a SegmentationDataset with the run's geometry and normalisers but no random translation, scale, mirror
    or augmentation; `validation.crops_per_case` crops of each are drawn once with `validation.seed` and stay on the device"""
    from segmentation3d.core.seg_validate import Validator
    from segmentation3d.dataloader.dataset import SegmentationDataset, collect_fixed_crops
    held_out = SegmentationDataset(
        imlist_file=val_cfg['imseg_list'], num_classes=cfg.dataset.num_classes, spacing=cfg.dataset.spacing,
        crop_size=cfg.dataset.crop_size, sampling_method=cfg.dataset.sampling_method, random_translation=[0, 0, 0],
        random_scale=[1, 1], interpolation=cfg.dataset.interpolation, crop_normalizers=cfg.dataset.crop_normalizers,
        device=step.device, resident_storage=getattr(cfg.dataset, 'resident_storage', 'fp32'),
        resident_budget_gb=getattr(cfg.dataset, 'resident_budget_gb', None),   # a budget of its own, of the same size
        mask_interpolation=getattr(cfg.dataset, 'mask_interpolation', 'NN'))
    if held_out.num_modality() != num_modality:
        raise ValueError('the validation cases of {} have {} modalities, the training set has {}'.format(
            val_cfg['imseg_list'], held_out.num_modality(), num_modality))
    crops, masks = collect_fixed_crops(held_out, val_cfg['crops_per_case'], val_cfg['seed'])
    loss_options = loss_options_from_config(cfg.loss)
    if cfg.loss.name == 'DiceBoundary':
        loss_options['spacing'] = tuple(cfg.dataset.spacing)
    loss_func = build_loss(cfg.loss.name, cfg.dataset.num_classes, cfg.loss.obj_weight, cfg.loss.focal_gamma, use_gpu=True,
                           **loss_options)   # a second object: the training loss's .last_terms stays the train step's
    batchsize = val_cfg['batchsize'] if val_cfg['batchsize'] is not None else cfg.train.batchsize
    return Validator(step.net, loss_func, crops, masks, batchsize, ignore_label=loss_options['ignore_label'],
                     ema=val_cfg['ema'], regions=loss_options.get('regions'))


def validation_log_line(epoch_idx, result):
    """'epoch: 3, val_loss: 0.2134, val_dice: 0.8123, val_dice_ema: 0.7990, val_dice_per_class: [0.9912, 0.8123]'"""
    ema = float('nan') if result['ema_dice'] is None else result['ema_dice']
    return 'epoch: {}, val_loss: {:.4f}, val_dice: {:.4f}, val_dice_ema: {:.4f}, val_dice_per_class: [{}]'.format(
        epoch_idx, result['val_loss'], result['mean_dice'], ema, ', '.join('{:.4f}'.format(d) for d in result['dice']))


def build_optimizer(name, params, lr, betas=(0.9, 0.999), optim_options=None):
    """'Adam' -> FusedAdam(lr, betas), 'SGD' -> FusedSGD(lr); `optim_options`: weight_decay, max_grad_norm,
    lr_schedule, and for SGD momentum, nesterov"""
    opts = dict(optim_options or {})
    opts.pop('optimizer', None)
    unknown = set(opts) - {'momentum', 'nesterov', 'weight_decay', 'max_grad_norm', 'lr_schedule'}
    if unknown:
        raise ValueError('unknown optim_options: {}'.format(sorted(unknown)))
    if name == 'Adam':
        opts.pop('momentum', None)
        opts.pop('nesterov', None)
        return FusedAdam(params, lr=lr, betas=betas, **opts)
    if name == 'SGD':
        return FusedSGD(params, lr=lr, **opts)
    raise ValueError('Unknown optimizer {!r} (Adam or SGD)'.format(name))


class TrainStep(object):
    """network + loss + FusedAdam or FusedSGD (+ gradient reducer when distributed) on one device; `loss_options` is a
    dict of build_loss's keyword options for the compound losses (dice_weight, ce_weight, include_background, batch_dice,
    ignore_label, topk_percent for loss_name='DiceTopK', boundary_weight and spacing for loss_name='DiceBoundary', which
    serves one resolution and is refused together with deep supervision, cldice_weight, cldice_iters and cldice_classes
    for loss_name='DiceClDice'); `optimizer` / `optim_options` are
    build_optimizer's (gradient-norm clipping, lr schedule, SGD);
    `deep_supervision` = L in 1..3 builds the network with L auxiliary heads and trains on the weighted per-level losses
    (loss/deep_supervision_loss.py; `deep_supervision_weights`: L + 1 weights, None = halving per level);
    `regions` (R label-id sets) with `region_class_order` makes it a region-based model: the network gets R sigmoid outputs
    in place of num_classes soft-max ones and loss_name must be one of REGION_LOSSES -- either without the other raises,
    and so does the combination with deep supervision (the fused auxiliary heads end in a soft-max)"""

    def __init__(self, net_name, in_channels, num_classes, loss_name='Dice', obj_weight=None, focal_gamma=2, lr=1e-4,
                 betas=(0.9, 0.999), device=None, seed=0, distributed=None, num_buckets=4, use_graph=False,
                 loss_options=None, optimizer='Adam', optim_options=None, deep_supervision=0, deep_supervision_weights=None,
                 regions=None, region_class_order=None):
        if loss_name == 'DiceBoundary' and int(deep_supervision) > 0:
            # one loss object would be called at levels whose spacing is 2^k times the nominal one
            raise ValueError("loss_name='DiceBoundary' is not combined with deep supervision")
        loss_options = dict(loss_options or {})
        if regions is None:
            regions = loss_options.get('regions')
        if (loss_name in REGION_LOSSES) != (regions is not None):
            raise ValueError('loss_name={!r} {} regions: a region-based model is trained with one of {}'.format(
                loss_name, 'needs' if regions is None else 'takes no', REGION_LOSSES))
        if regions is None and region_class_order is not None:
            raise ValueError('region_class_order given without regions')
        self.regions, self.region_class_order = None, None
        if regions is not None:
            self.regions = check_regions(regions)
            self.region_class_order = check_region_class_order(region_class_order, len(self.regions))
            if int(deep_supervision) > 0:
                raise ValueError('a region-based model is not combined with deep supervision')
            loss_options['regions'] = self.regions
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if self.device.type == 'cuda' and self.device.index is not None:
            torch.cuda.set_device(self.device)   # the engine launches on the current device's stream (_engine.stream_ptr)
        net_module = importlib.import_module('segmentation3d.network.' + net_name)      # core/seg_train.py:72
        self.deep_supervision = int(deep_supervision)
        if self.deep_supervision:
            normalise_level_weights(self.deep_supervision, deep_supervision_weights)   # bad levels / weights raise before anything is built
            if _ops.activation_dtype_name() != 'fp32':
                raise ValueError('deep supervision runs in fp32 activation mode only')
        elif deep_supervision_weights is not None:
            raise ValueError('deep_supervision_weights given but deep_supervision is 0')
        torch.manual_seed(seed)
        if self.regions is not None:
            self.net = net_module.SegmentationNet(in_channels, len(self.regions), output_activation='sigmoid')
        elif self.deep_supervision:
            self.net = net_module.SegmentationNet(in_channels, num_classes, deep_supervision=self.deep_supervision)
        else:
            self.net = net_module.SegmentationNet(in_channels, num_classes)
        self.max_stride = self.net.max_stride()
        net_module.parameters_kaiming_init(self.net)                                    # core/seg_train.py:75
        self.net = self.net.to(self.device)
        self.opt = build_optimizer(optimizer, self.net.parameters(), lr, betas, optim_options)   # core/seg_train.py:83
        _ops.weight_cache(True)   # packed conv weights are refreshed by the optimizer's step() with one launch per step
        self.loss_func = build_loss(loss_name, num_classes, obj_weight, focal_gamma, use_gpu=True, **loss_options)
        if self.deep_supervision:
            self.loss_func = DeepSupervisionLoss(self.loss_func, self.deep_supervision, deep_supervision_weights)
        if distributed is None:
            distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        self.reducer = None
        if distributed:
            self.reducer = GradientReducer(self.opt.flat_grads(), self.opt.flat_layout(), num_buckets=num_buckets)
            self.reducer.broadcast_parameters([f['params'] for f in self.opt._flat if f is not None], src=0)
            self.opt.grad_scale = 1.0 / self.reducer.world_size
            _ops.PACK_CACHE.invalidate()   # the broadcast rewrote the parameters
        # use_graph (single process only): after two eager steps the whole step -- zero_grad, forward, loss, backward,
        # Adam, weight re-pack: ~420 launches -- is captured ONCE in a hipGraph and replayed; the host then costs one
        # replay per step instead of ~10 ms of launch work (what bounds the bf16 mode, whose kernels take about as long).
        # Inputs are copied into static buffers; a new input shape re-captures.  Not combined with the gradient reducer:
        # its collectives stay outside hipGraphs.
        self.use_graph = bool(use_graph) and self.reducer is None
        self._graph, self._gx, self._gt, self._gloss, self._eager_calls = None, None, None, None, 0
        if self.device.type == 'cuda':
            # the weight-gradient side stream is chosen by a probe that synchronises the device: here, not inside the first backward
            _ops.prepare_side_stream(self.device)

    def __call__(self, crops, masks):
        """one optimisation step; returns the (device) loss tensor of this rank's batch"""
        if self.use_graph:
            return self._graphed(crops, masks)
        return self._eager(crops, masks)

    def _graphed(self, crops, masks):
        if self._graph is not None and (self._gx.shape != crops.shape or self._gt.shape != masks.shape or
                                        self._gx.dtype != crops.dtype or self._gt.dtype != masks.dtype):
            self._graph, self._eager_calls = None, 0          # new geometry: warm up and capture again
        if self._graph is None:
            if self._eager_calls < 2:                         # allocator, packed-weight images, plans warm up eagerly
                self._eager_calls += 1
                return self._eager(crops, masks)
            self.opt.use_device_step()
            self._gx, self._gt = crops.clone(), masks.clone()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            step_counts = self.opt.step_counts()
            try:
                with torch.cuda.graph(graph):
                    self._gloss = self._eager(self._gx, self._gt)
            except Exception as exc:                           # capture refused (driver / allocator state): stay eager
                import warnings
                warnings.warn('TrainStep: hipGraph capture of the train step failed ({}); continuing eagerly'.format(exc))
                torch.cuda.synchronize()
                self.opt.restore_step_counts(step_counts)
                self.use_graph = False
                return self._eager(crops, masks)
            self.opt.restore_step_counts(step_counts)         # capture ran the host side of opt.step() once, no kernels
            self._graph = graph
        self._gx.copy_(crops)
        self._gt.copy_(masks)
        self._graph.replay()
        self.opt.note_replayed_step()
        return self._gloss

    def _eager(self, crops, masks):
        self.opt.zero_grad()
        if self.reducer is not None:
            self.reducer.begin_step()
        outputs = self.net.forward_deep(crops) if self.deep_supervision else self.net(crops)
        loss = self.loss_func(outputs, masks)
        loss.backward()
        if self.reducer is not None:
            self.reducer.finish_step()   # the norm a clipping optimizer measures is that of the REDUCED buffer
        self.opt.step()
        return loss


def epoch_of_batch(batch_idx, batchsize, num_samples, world_size=1):
    """epoch index after `batch_idx` steps (core/seg_train.py:135: batch_idx * batchsize // len(dataset)).  Under data
    parallelism every step consumes world_size * batchsize samples -- each rank draws its 1/world shard of a pass
    (EpochConcateDistributedSampler) -- so the GLOBAL batch is what advances the epoch; with world_size = 1 this is the
    reference's formula."""
    return int(batch_idx) * int(batchsize) * int(world_size) // int(num_samples)


def train(train_config_file, data_iter_factory=None):
    """training engine with the reference's config schema (config/train_config.py) and checkpoint layout.

    Data: by default the GPU-resident `SegmentationDataset` (dataloader/dataset.py: cases read once, crops resampled
    and normalised on the device) driven by `EpochConcateSampler` -- or its distributed variant, one shard per rank --
    exactly as core/seg_train.py:56-70 wires the reference's dataset; alternatively pass
    `data_iter_factory(cfg) -> iterator of (crops, masks[, frames, names])`.  Model folder, config copies, seeding,
    loss selection, logging format and checkpoint cadence follow core/seg_train.py:22-152.

    An optional `validation` section (core/seg_validate.py; not in the reference) scores the network on fixed held-out crops
    whenever the epoch index reaches a new multiple of `validation.epochs`: one `val_` log line, the checkpoint with the
    best moving-average Dice in `checkpoints/best`, and the average's state in every `chk_<epoch>/params.pth`.
    """
    from segmentation3d.utils.file_io import load_config, setup_logger
    from segmentation3d.utils.model_io import BEST_FOLDER, checkpoint_validation, load_checkpoint, save_checkpoint
    from segmentation3d.core.seg_validate import validate_validation
    assert os.path.isfile(train_config_file), 'Config not found: {}'.format(train_config_file)
    cfg = load_config(train_config_file)
    # optional `validation` section (None: off, and then nothing below differs from a run without it); bad keys / values
    # raise before anything is built
    val_cfg = validate_validation(getattr(cfg, 'validation', None), cfg.dataset.num_classes)
    boundary_schedule = boundary_schedule_from_config(cfg.loss) if cfg.loss.name == 'DiceBoundary' else None   # likewise
    regions, region_class_order = regions_from_config(cfg.loss)   # likewise; (None, None): an exclusive-class run
    model_folder = os.path.join(cfg.general.save_dir, cfg.general.model_scale)
    distributed = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank() if distributed else 0
    world_size = dist.get_world_size() if distributed else 1
    if rank == 0:
        if os.path.isdir(model_folder) and cfg.general.resume_epoch < 0:
            shutil.rmtree(model_folder)
        os.makedirs(model_folder, exist_ok=True)
        shutil.copy(train_config_file, os.path.join(model_folder, 'train_config.py'))
        infer_cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'config', 'infer_config.py')
        if os.path.isfile(infer_cfg):
            shutil.copy(infer_cfg, os.path.join(cfg.general.save_dir, 'infer_config.py'))
    logger = setup_logger(os.path.join(model_folder, 'train_log.txt'), 'seg3d') if rank == 0 else None
    np.random.seed(cfg.general.seed)
    if cfg.general.num_gpus <= 0:
        raise RuntimeError('segmentation3d HIP engine needs general.num_gpus > 0 (no CPU training path)')
    dataset = None
    if data_iter_factory is None:
        # the built-in dataset decides the number of input channels (core/seg_train.py:73: dataset.num_modality()); it
        # reads only the list and the file headers here, the volumes are loaded on first use
        from segmentation3d.dataloader.dataset import SegmentationDataset
        dataset = SegmentationDataset(
            imlist_file=cfg.general.imseg_list, num_classes=cfg.dataset.num_classes, spacing=cfg.dataset.spacing,
            crop_size=cfg.dataset.crop_size, sampling_method=cfg.dataset.sampling_method,
            random_translation=cfg.dataset.random_translation, random_scale=cfg.dataset.random_scale,
            interpolation=cfg.dataset.interpolation, crop_normalizers=cfg.dataset.crop_normalizers, device=None,
            random_mirror_axes=getattr(cfg.dataset, 'random_mirror_axes', None) or (),
            augmentation=getattr(cfg.dataset, 'augmentation', None),
            resolution_augmentation=getattr(cfg.dataset, 'resolution_augmentation', None),
            resident_storage=getattr(cfg.dataset, 'resident_storage', 'fp32'),
            resident_budget_gb=getattr(cfg.dataset, 'resident_budget_gb', None),
            mask_interpolation=getattr(cfg.dataset, 'mask_interpolation', 'NN'))
        num_modality = dataset.num_modality()
        configured = getattr(cfg.dataset, 'num_modality', None)
        if configured is not None and int(configured) != num_modality:
            raise ValueError('cfg.dataset.num_modality = {} but the cases of {} have {} modalities'.format(
                configured, cfg.general.imseg_list, num_modality))
    else:
        num_modality = int(getattr(cfg.dataset, 'num_modality', 1))
    _ops.set_activation_dtype(str(getattr(cfg.train, 'compute_dtype', 'fp32')))
    num_samples = len(dataset) if dataset is not None else int(getattr(cfg.dataset, 'num_samples', cfg.train.batchsize))
    optim_options = optim_options_from_config(cfg.train, num_samples, world_size)
    show_lr = optim_options['lr_schedule'] is not None and optim_options['lr_schedule']['name'] != 'constant'
    deep = deep_supervision_from_config(cfg.train)
    loss_options = loss_options_from_config(cfg.loss)
    if boundary_schedule is not None:
        loss_options['spacing'] = tuple(cfg.dataset.spacing)
    if cfg.general.resume_epoch >= 0 and not hasattr(cfg.train, 'deep_supervision'):
        from segmentation3d.utils.model_io import checkpoint_deep_supervision
        deep['deep_supervision'] = checkpoint_deep_supervision(cfg.general.resume_epoch, model_folder)   # rebuild the same net
    step = TrainStep(cfg.net.name, num_modality, cfg.dataset.num_classes, cfg.loss.name, cfg.loss.obj_weight,
                     cfg.loss.focal_gamma, cfg.train.lr, tuple(cfg.train.betas), seed=cfg.general.seed,
                     use_graph=bool(getattr(cfg.train, 'use_graph', False)),
                     loss_options=loss_options, optimizer=optim_options.pop('optimizer'),
                     optim_options=optim_options, regions=regions, region_class_order=region_class_order, **deep)
    assert np.all(np.array(cfg.dataset.crop_size) % step.max_stride == 0), 'crop size not divisible by max stride'
    last_save_epoch, batch_idx = 0, 0
    if cfg.general.resume_epoch >= 0:
        last_save_epoch, batch_idx = load_checkpoint(cfg.general.resume_epoch, step.net, step.opt, model_folder)
    if dataset is not None:
        from segmentation3d.dataloader.dataset import DeviceCropLoader
        from segmentation3d.dataloader.sampler import EpochConcateSampler, EpochConcateDistributedSampler
        dataset.device = step.device
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            sampler = EpochConcateDistributedSampler(dataset, cfg.train.epochs, max(0, cfg.general.resume_epoch))
        else:
            sampler = EpochConcateSampler(dataset, cfg.train.epochs)
        batches = DeviceCropLoader(dataset, sampler, cfg.train.batchsize)
    else:
        batches = data_iter_factory(cfg)
    validator, last_val_epoch = None, last_save_epoch
    if val_cfg is not None:
        validator = build_validator(cfg, val_cfg, step, num_modality)
        if cfg.general.resume_epoch >= 0:
            stored = checkpoint_validation(cfg.general.resume_epoch, model_folder)
            if stored is not None:
                validator.load_state_dict(stored)   # the moving average and the best value continue
        step.validator = validator
    steps_this_run = 0
    residency_pending = dataset is not None
    boundary_epoch = None
    for batch in batches:
        crops, masks = batch[0], batch[1]
        begin_t = time.time()
        crops, masks = crops.to(step.device, non_blocking=True), masks.to(step.device, non_blocking=True)
        if boundary_schedule is not None:
            epoch_now = epoch_of_batch(batch_idx, cfg.train.batchsize, num_samples, world_size)
            if epoch_now != boundary_epoch:   # a plain fill of the device scalar, outside the captured step
                boundary_epoch = epoch_now
                step.loss_func.set_boundary_weight(boundary_schedule(epoch_now))
                if validator is not None:
                    validator.loss_func.set_boundary_weight(boundary_schedule(epoch_now))
        loss = step(crops, masks)
        epoch_idx = epoch_of_batch(batch_idx, cfg.train.batchsize, num_samples, world_size)
        batch_idx += 1
        steps_this_run += 1
        if steps_this_run == 3 and bool(getattr(cfg.train, 'gc_freeze', True)):   # (also after a resume: counted per run)
            # everything that lives for the whole run (modules, packed-weight cache, dataset) leaves the collector's young
            # generations: the collections that a step's short-lived autograd objects trigger were the largest single
            # host cost of an eager step (bf16 mode: 10.6 -> 6.5 ms per step)
            gc.collect()
            gc.freeze()
        value = loss.item()
        sample_duration = (time.time() - begin_t) / cfg.train.batchsize
        if logger is not None:
            line = 'epoch: {}, batch: {}, train_loss: {:.4f}, time: {:.4f} s/vol'.format(epoch_idx, batch_idx, value,
                                                                                        sample_duration)
            if show_lr:   # the reference's log format unless a schedule moves the rate
                line += ', lr: {:.6e}'.format(step.opt.param_groups[0]['lr'])
            if boundary_schedule is not None:
                line += ', boundary_weight: {:.6g}'.format(step.loss_func.boundary_weight)
            logger.info(line)
            if (residency_pending and dataset.has_budget()
                    and epoch_of_batch(batch_idx, cfg.train.batchsize, num_samples, world_size) >= 1):
                # a run with dataset.resident_budget_gb: what the first pass over the cases left where
                residency_pending = False
                logger.info('resident cases: {}, staged cases: {}, resident bytes: {}'.format(
                    dataset.num_resident(), dataset.num_staged(), dataset.resident_bytes()))
        if validator is not None and epoch_idx != 0 and epoch_idx % val_cfg['epochs'] == 0 and last_val_epoch != epoch_idx:
            result = validator.run(epoch_idx)     # every rank: the counts are all-reduced
            last_val_epoch = epoch_idx
            if logger is not None:
                logger.info(validation_log_line(epoch_idx, result))
            if rank == 0 and result['improved'] and val_cfg['save_best']:
                folder = save_checkpoint(step.net, step.opt, epoch_idx, batch_idx, cfg, step.max_stride, num_modality,
                                         regions, region_class_order, validation=validator.state_dict(),
                                         folder_name=BEST_FOLDER)
                with open(os.path.join(folder, 'validation.json'), 'w') as f:
                    json.dump(dict(result, epoch=epoch_idx, batch=batch_idx), f, indent=1)
        if rank == 0 and epoch_idx != 0 and epoch_idx % cfg.train.save_epochs == 0 and last_save_epoch != epoch_idx:
            save_checkpoint(step.net, step.opt, epoch_idx, batch_idx, cfg, step.max_stride, num_modality, regions,
                            region_class_order, validation=None if validator is None else validator.state_dict())
            last_save_epoch = epoch_idx
    return step
