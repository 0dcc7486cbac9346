"""DiceCELoss -- soft Dice + cross-entropy / focal on the network's probabilities, with an ignore label.  The reference
has no such loss; the definitions are this project's.

Input `p` [N, C, *spatial] float32 probabilities (the head's soft-max output), target `t` [N, 1, *spatial] float class ids.
A voxel counts iff 0 <= t < C and t != ignore_label; every other voxel enters no sum and gets a zero gradient.

  region term:        d[n,c] = (2 sum_s p_c t_c + 1e-5) / (sum_s p_c + sum_s t_c + 1e-5)       (t_c = [t == c]; no arg-max
                      L_region = sum_{c in K} w'_c (1 - mean_n d[n,c])                           gate, non-squared denominator)
                      K = all classes, or 1 .. C-1 without the background; w' = weights normalised over K.
                      batch_dice: the sums run over the batch as well, one ratio per class.  Under data parallelism the
                      batch is this rank's own batch -- there is no collective.
  distribution term:  pt = max(p_t, 1e-12);  L_dist = sum a_t (1 - pt)^gamma (-log pt) / sum a_t  (0 when no voxel counts)
                      a = weights, not normalised (the weighted mean does not depend on their scale); gamma = 0 is the
                      weighted cross-entropy F.nll_loss(log(p.clamp_min(1e-12)), t, weight=a, ignore_index=...).
  loss:               L = dice_weight * L_region + ce_weight * L_dist; a term whose weight is 0 never enters L.

All sums come from ONE pass over the probabilities (seg3d_compound_loss_fwd) and the backward is one elementwise kernel.
"""
import math

import torch
import torch.nn as nn

from segmentation3d import _ops


def class_weight_tensors(num_class, weights, include_background, require_finite=False):
    """validate the per-class weights (None = all ones; positive, and finite if asked) and return (region, classes): the
    float32 region weights normalised over the included classes (0 for an excluded background) and the weights as given"""
    if weights is None:
        weights = [1.0] * num_class
    weights = [float(w) for w in weights]
    if len(weights) != num_class:
        raise ValueError('weights has {} entries but num_class is {}'.format(len(weights), num_class))
    if not all(w > 0.0 and (math.isfinite(w) or not require_finite) for w in weights):
        raise ValueError('class weights must be positive, got {}'.format(weights))
    if not include_background and num_class == 1:
        raise ValueError('include_background=False leaves no class with num_class = 1')
    region = torch.tensor(weights, dtype=torch.float64)
    if not include_background:
        region[0] = 0.0
    return (region / region.sum()).float(), torch.tensor(weights, dtype=torch.float32)


class DiceCELoss(nn.Module):
    """ soft Dice + cross-entropy (gamma = 0) or focal (gamma > 0) compound loss """

    def __init__(self, num_class, weights=None, dice_weight=1.0, ce_weight=1.0, gamma=0.0, include_background=True,
                 batch_dice=False, ignore_label=None, use_gpu=True):
        """
        :param num_class: the number of classes C (channels of the input)
        :param weights: positive weight per class (region term: normalised over the included classes; distribution
                        term: the class weights of the weighted mean), None = all ones
        :param dice_weight, ce_weight: weights of the two terms, >= 0 and not both 0
        :param gamma: focal exponent of the distribution term, >= 0 (0: cross-entropy)
        :param include_background: False leaves class 0 out of the region term
        :param batch_dice: sum the region term's numerators and denominators over the batch before the ratio
        :param ignore_label: target value whose voxels are left out of the loss (None: only out-of-range ids are)
        :param use_gpu: kept for signature compatibility; the weights follow the input's device
        """
        super(DiceCELoss, self).__init__()
        num_class = int(num_class)
        if num_class < 1:
            raise ValueError('num_class must be >= 1, got {}'.format(num_class))
        region_weights, class_weights = class_weight_tensors(num_class, weights, include_background)
        dice_weight, ce_weight, gamma = float(dice_weight), float(ce_weight), float(gamma)
        if dice_weight < 0.0 or ce_weight < 0.0 or (dice_weight == 0.0 and ce_weight == 0.0):
            raise ValueError('dice_weight and ce_weight must be >= 0 and not both 0, got {} and {}'.format(dice_weight,
                                                                                                         ce_weight))
        if not gamma >= 0.0:
            raise ValueError('gamma must be >= 0, got {}'.format(gamma))
        self.num_class = num_class
        self.dice_weight, self.ce_weight, self.gamma = dice_weight, ce_weight, gamma
        self.include_background = bool(include_background)
        self.batch_dice = bool(batch_dice)
        self.ignore_label = None if ignore_label is None else float(ignore_label)
        self.region_weights, self.class_weights = region_weights, class_weights
        self.use_gpu = use_gpu
        self.last_terms = None

    def _check_shapes(self, input_tensor, target):
        if input_tensor.dim() < 3 or input_tensor.shape[1] != self.num_class:
            raise ValueError('input of shape {} does not have num_class = {} channels'.format(tuple(input_tensor.shape),
                                                                                              self.num_class))
        if target.numel() * self.num_class != input_tensor.numel():
            raise ValueError('target shape {} does not match input {}'.format(tuple(target.shape),
                                                                              tuple(input_tensor.shape)))

    def _weights_on(self, device):
        if self.region_weights.device != device:
            self.region_weights = self.region_weights.to(device)
            self.class_weights = self.class_weights.to(device)

    def _ignore_value(self):
        """any value outside [0, C) stands for "no ignore label": such voxels are left out by the range rule anyway"""
        return -1.0 if self.ignore_label is None else self.ignore_label

    def forward(self, input_tensor, target):
        """
        :param input_tensor: network output probabilities [N, C, D, H, W] (any trailing spatial shape), float32
        :param target: ground truth class ids, float, [N, 1, D, H, W]
        :return: the loss (0-dim tensor, differentiable w.r.t. input_tensor); `.last_terms` then holds the device tensor
                 (L, L_region, L_dist) of this call, written without a synchronisation
        """
        self._check_shapes(input_tensor, target)
        self._weights_on(input_tensor.device)
        loss, self.last_terms = _ops.CompoundLossFunction.apply(
            input_tensor, target, self.region_weights, self.class_weights, self.gamma, self.dice_weight, self.ce_weight,
            self.batch_dice, self._ignore_value())
        return loss
