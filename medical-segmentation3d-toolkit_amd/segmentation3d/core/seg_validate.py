"""Online validation for core/seg_train.train() -- the reference trains blind (its core/seg_train.py has no validation), so
the definitions are this project's.

Between epochs the network is run, without autograd, over a FIXED set of held-out crops that stays resident on the device
(dataloader.dataset.collect_fixed_crops).  Per batch: `net(x)`, the run's loss, and ONE pass that takes the arg-max and adds
the per-class (tp, fp, fn) into a device buffer (_ops.confusion_counts, seg3d_confusion_counts).  Counts and the loss sum
stay on the device for the whole pass and are read back once.

  dice[c]    = 2 tp / (2 tp + fp + fn)          nan for a class that neither labels nor prediction contain
  mean_dice  = nan-mean of dice over the foreground classes 1 .. C-1
               (region-based model: dice has one value per region and the mean runs over all R of them)
  ema_dice   = the first finite mean_dice, then a * ema + (1 - a) * mean_dice; a nan mean leaves it unchanged
  improved   = ema_dice is strictly above every earlier value (the run keeps that checkpoint in `checkpoints/best`)
  val_loss   = mean over the crops of the batch losses (each batch weighted by its size)

The pass runs eagerly: it is never captured into a hipGraph of its own next to a captured train step (two captured steps of one
process share the packed-weight tables, tools/bench_loss.py).  A region-based model (`regions`; row f23) goes through the
same pass with seg3d_region_confusion_counts in place of the arg-max counts: region r is predicted where p_r > 0.5.
Whole-volume sliding-window validation, thresholds other than 0.5 and surface metrics on regions are out of scope.
"""
import math

import torch
import torch.distributed as dist

from segmentation3d import _ops
from segmentation3d.loss.region_loss import check_regions, region_lut
from segmentation3d.utils.metrics import dice_from_counts, mean_foreground_dice, mean_region_dice

# keys and defaults of the optional `validation` section of a training config
VALIDATION_DEFAULTS = {
    'imseg_list': None,       # list file of the held-out cases; None (or no section): validation off
    'epochs': 1,              # validate when the epoch index first reaches a multiple of this
    'crops_per_case': 4,
    'batchsize': None,        # None: train.batchsize
    'seed': 0,                # seed of the fixed crops
    'ema': 0.9,               # in [0, 1)
    'save_best': True,
}


def _integer(name, value, lowest):
    if isinstance(value, bool) or not isinstance(value, int) or value < lowest:
        raise ValueError('validation.{} must be an integer >= {}, got {!r}'.format(name, lowest, value))
    return value


def check_ema(ema):
    try:
        a = float(ema)
    except (TypeError, ValueError):
        raise ValueError('validation.ema must be a number in [0, 1), got {!r}'.format(ema))
    if isinstance(ema, bool) or not 0.0 <= a < 1.0:
        raise ValueError('validation.ema must be in [0, 1), got {!r}'.format(ema))
    return a


def validate_validation(section, num_classes=2):
    """the `validation` section (dict / EasyDict / None) -> a plain dict with every key of VALIDATION_DEFAULTS, or None when
    the section is absent or names no `imseg_list` (validation off).  Unknown keys and bad values -- `epochs` or
    `crops_per_case` below 1, `ema` outside [0, 1), fewer than 2 classes -- raise ValueError."""
    if section is None:
        return None
    if not hasattr(section, 'keys'):
        raise ValueError('validation must be a dict, got {!r}'.format(type(section)))
    unknown = sorted(set(section.keys()) - set(VALIDATION_DEFAULTS))
    if unknown:
        raise ValueError('unknown validation option(s) {}; known: {}'.format(unknown, sorted(VALIDATION_DEFAULTS)))
    v = {k: section[k] if k in section else d for k, d in VALIDATION_DEFAULTS.items()}
    v['epochs'] = _integer('epochs', v['epochs'], 1)
    v['crops_per_case'] = _integer('crops_per_case', v['crops_per_case'], 1)
    if v['batchsize'] is not None:
        v['batchsize'] = _integer('batchsize', v['batchsize'], 1)
    v['seed'] = _integer('seed', v['seed'], 0)
    v['ema'] = check_ema(v['ema'])
    if not isinstance(v['save_best'], bool):
        raise ValueError('validation.save_best must be True or False, got {!r}'.format(v['save_best']))
    if v['imseg_list'] is None:
        return None
    if not isinstance(v['imseg_list'], str):
        raise ValueError('validation.imseg_list must be a path, got {!r}'.format(v['imseg_list']))
    if int(num_classes) < 2:
        raise ValueError('validation needs dataset.num_classes >= 2 (a foreground class), got {}'.format(num_classes))
    return v


class DiceEma(object):
    """the moving average of the mean validation Dice and its best value (host arithmetic in doubles)"""

    def __init__(self, ema=0.9):
        self.alpha = check_ema(ema)
        self.ema_dice = None
        self.best_ema_dice = None
        self.best_epoch = None

    def update(self, mean_dice, epoch=None):
        """take one validation result; returns `improved`: the average is strictly above every earlier value"""
        mean_dice = float(mean_dice)
        if math.isnan(mean_dice):
            return False                      # nothing to score: the average stays
        if self.ema_dice is None:
            self.ema_dice = mean_dice
        else:
            self.ema_dice = self.alpha * self.ema_dice + (1.0 - self.alpha) * mean_dice
        if self.best_ema_dice is None or self.ema_dice > self.best_ema_dice:
            self.best_ema_dice, self.best_epoch = self.ema_dice, epoch
            return True
        return False

    def state_dict(self):
        return {'ema_dice': self.ema_dice, 'best_ema_dice': self.best_ema_dice, 'best_epoch': self.best_epoch}

    def load_state_dict(self, state):
        for key in ('ema_dice', 'best_ema_dice'):
            value = state[key]
            setattr(self, key, None if value is None else float(value))
        self.best_epoch = None if state['best_epoch'] is None else int(state['best_epoch'])


class Validator(object):
    """the validation pass over fixed device-resident crops.

    :param net: the network being trained; called as net(x) under torch.no_grad() -- with deep supervision that is the
                full-resolution output alone
    :param loss_func: a loss object of its OWN (build_loss with the run's options; with deep supervision the plain base
                loss), so that the training loss's `.last_terms` is never overwritten
    :param crops, masks: [V, M, z, y, x] / [V, 1, z, y, x] device tensors (collect_fixed_crops)
    :param batchsize: crops per forward
    :param ignore_label: the loss's ignore label: such voxels enter no count
    :param ema: the moving average's coefficient in [0, 1)
    :param regions: the R label-id sets of a region-based model (None: exclusive classes); the network then has R sigmoid
                outputs, the counts are per region and the mean Dice runs over all of them
    Under data parallelism rank r takes crops r::world_size and the counts and loss sums are all-reduced, so every rank
    returns identical numbers (and every rank must call run()).
    """

    def __init__(self, net, loss_func, crops, masks, batchsize, ignore_label=None, ema=0.9, regions=None):
        if crops.dim() != 5 or masks.dim() != 5 or crops.shape[0] != masks.shape[0] or crops.shape[0] < 1:
            raise ValueError('crops / masks must be [V, M, z, y, x] / [V, 1, z, y, x] with V >= 1, got {} and {}'.format(
                tuple(crops.shape), tuple(masks.shape)))
        self.batchsize = _integer('batchsize', int(batchsize), 1)
        self.net, self.loss_func = net, loss_func
        self.ignore_label = None if ignore_label is None else float(ignore_label)
        self.tracker = DiceEma(ema)
        self.regions = None if regions is None else check_regions(regions)
        self._lut = None if regions is None else region_lut(self.regions)
        self.distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        rank, world = (dist.get_rank(), dist.get_world_size()) if self.distributed else (0, 1)
        if crops.shape[0] < world:
            raise ValueError('validation has {} crops for {} ranks: every rank needs one'.format(crops.shape[0], world))
        self.crops, self.masks = crops[rank::world].contiguous(), masks[rank::world].contiguous()
        self.counts = None        # int64 [C, 3], made at the first batch (C is the network's; with regions it is R)
        self._loss = torch.zeros(2, dtype=torch.float64, device=crops.device)   # (sum of batch loss * batch size, crops)

    def accumulate(self):
        """the device side of one pass: zero the accumulators, then per batch forward, loss and confusion counts.  Nothing
        is synchronised or read back (the whole call can be captured into a hipGraph).
        The packed-weight cache is frozen for the pass.  A batch of another size than the train step's can select another
        conv plan and with it a packed image the train step never registered; registering it would drop the job table
        that a captured train step reads on every replay.  Frozen, the forward uses the images that are current (the
        optimizer's step or the replay refreshed them) and packs any other into a buffer of its own."""
        self._loss.zero_()
        if self.counts is not None:
            self.counts.zero_()
        with torch.no_grad(), _ops.PACK_CACHE.frozen():
            for b in range(0, int(self.crops.shape[0]), self.batchsize):
                x, t = self.crops[b:b + self.batchsize], self.masks[b:b + self.batchsize]
                probs = self.net(x)
                if self.counts is None:
                    self.counts = torch.zeros((int(probs.shape[1]), 3), dtype=torch.int64, device=probs.device)
                loss = self.loss_func(probs, t)
                if self.regions is None:
                    _ops.confusion_counts(probs, t, self.ignore_label, out=self.counts)
                else:
                    if int(probs.shape[1]) != len(self.regions):
                        raise ValueError('the network has {} outputs for {} regions'.format(int(probs.shape[1]),
                                                                                           len(self.regions)))
                    _ops.region_confusion_counts(probs, t, self._lut, self.ignore_label, out=self.counts)
                n = int(x.shape[0])
                self._loss[0] += loss.detach().double() * n
                self._loss[1] += n

    def finish(self, epoch=None):
        """reduce over the ranks, read back once, update the moving average; returns the result dict"""
        if self.distributed:
            dist.all_reduce(self.counts, op=dist.ReduceOp.SUM)
            dist.all_reduce(self._loss, op=dist.ReduceOp.SUM)
        # one read-back: counts are far below 2^53, so their doubles are exact
        host = torch.cat([self.counts.reshape(-1).double(), self._loss]).cpu().tolist()
        counts = [[int(v) for v in host[3 * c:3 * c + 3]] for c in range(int(self.counts.shape[0]))]
        loss_sum, ncrops = host[-2], host[-1]
        mean = mean_foreground_dice(counts) if self.regions is None else mean_region_dice(counts)
        improved = self.tracker.update(mean, epoch)
        return {'val_loss': loss_sum / ncrops if ncrops > 0 else float('nan'), 'dice': dice_from_counts(counts),
                'mean_dice': mean, 'ema_dice': self.tracker.ema_dice, 'improved': improved}

    def run(self, epoch=None):
        """one validation pass -> {'val_loss', 'dice' (list of C), 'mean_dice', 'ema_dice', 'improved'}"""
        self.accumulate()
        return self.finish(epoch)

    def state_dict(self):
        return self.tracker.state_dict()

    def load_state_dict(self, state):
        self.tracker.load_state_dict(state)
