"""Regions for region-based models: validation, the label -> region lookup table and the
training loss RegionDiceBCELoss (row f23).  The reference knows exclusive classes only.

`regions` is a list of R label-id sets (1 <= R <= 16, ids 1..255, background 0 in none), e.g. BraTS: whole tumour {1, 2, 3},
tumour core {1, 3}, enhancing tumour {3}.  Regions may overlap, so a region-based network has one sigmoid output per region
instead of a soft-max over exclusive classes.  Bit r of `lut[l]` says whether label l belongs to region r; the device code
(evaluation counts, the training loss, the validation counts) looks memberships up in that 256-word table.  `region_class_order` is the label inference writes for each
region when it composes the thresholded region probabilities back into a label map.

RegionDiceBCELoss: input `p` [N, R, *spatial] float32 sigmoid probabilities, target `t` [N, 1, *spatial] float label ids.
A voxel counts iff t is an integer in [0, 256) and t != ignore_label; every other voxel enters no sum and gets a zero
gradient.  The target of region r is z_r = [t in region r]; a label in no region is background for every region.

  Dice term:  d[n,r] = (2 sum_s p_r z_r + 1e-5) / (sum_s p_r + sum_s z_r + 1e-5),  L_dice = sum_r w'_r (1 - mean_n d[n,r]),
              w' = weights normalised over the R regions; batch_dice as in DiceCELoss.  It is the compound loss's region
              term with planes as classes, from the same device code.
  BCE term:   q = z ? p : 1 - p,  qc = max(q, 1e-12),  L_bce = sum_v sum_r a_r (1 - qc)^gamma (-log qc) / (n_counted sum_r a_r)
              (0 when no voxel counts); a = weights as given.  With unit weights and gamma = 0 it is
              F.binary_cross_entropy(p, z) (mean) over the counted voxels.
  loss:       L = dice_weight * L_dice + bce_weight * L_bce; a term whose weight is 0 never enters L.

All sums come from ONE pass over the probabilities (seg3d_region_loss_fwd) and the backward is one elementwise kernel.
"""
import math

import torch
import torch.nn as nn

MAX_REGIONS = 16


def check_regions(regions):
    """-> list of R sorted label-id lists; ValueError unless 1 <= R <= 16 and every region is a non-empty set of distinct
    integer ids in 1..255"""
    if regions is None or isinstance(regions, (str, bytes)) or not hasattr(regions, '__len__'):
        raise ValueError('regions must be a list of label-id lists, got {!r}'.format(regions))
    if not 1 <= len(regions) <= MAX_REGIONS:
        raise ValueError('between 1 and {} regions are supported, got {}'.format(MAX_REGIONS, len(regions)))
    out = []
    for k, region in enumerate(regions):
        if isinstance(region, (str, bytes)) or not hasattr(region, '__iter__'):
            raise ValueError('region {} must be a list of label ids, got {!r}'.format(k, region))
        ids = list(region)
        if not ids:
            raise ValueError('region {} is empty'.format(k))
        for l in ids:
            if isinstance(l, bool) or int(l) != l or not 1 <= int(l) <= 255:
                raise ValueError('region {}: label id {!r} is not an integer in 1..255'.format(k, l))
        ids = [int(l) for l in ids]
        if len(set(ids)) != len(ids):
            raise ValueError('region {} lists a label id twice: {}'.format(k, ids))
        out.append(sorted(ids))
    return out


def check_region_class_order(region_class_order, num_regions):
    """-> list of R ints in 1..127 (the label written for region r at inference; the mask is int8)"""
    if region_class_order is None or isinstance(region_class_order, (str, bytes)) or not hasattr(region_class_order, '__len__'):
        raise ValueError('region_class_order must be a list of {} label ids, got {!r}'.format(num_regions, region_class_order))
    order = list(region_class_order)
    if len(order) != num_regions:
        raise ValueError('region_class_order has {} entries for {} regions'.format(len(order), num_regions))
    for l in order:
        if isinstance(l, bool) or int(l) != l or not 1 <= int(l) <= 127:
            raise ValueError('region_class_order entry {!r} is not an integer in 1..127'.format(l))
    return [int(l) for l in order]


def region_lut(regions):
    """the 256-word table of the kernels: bit r of lut[l] is set iff label l is in region r (a list of Python ints)"""
    lut = [0] * 256
    for r, region in enumerate(check_regions(regions)):
        for l in region:
            lut[l] |= 1 << r
    return lut


class RegionDiceBCELoss(nn.Module):
    """ soft Dice + binary cross-entropy (gamma = 0) or focal (gamma > 0) on the sigmoid outputs of a region-based model """

    def __init__(self, regions, weights=None, dice_weight=1.0, bce_weight=1.0, gamma=0.0, batch_dice=False,
                 ignore_label=None):
        """
        :param regions: list of R label-id lists (check_regions); the network has one sigmoid output per region
        :param weights: positive finite weight per region (Dice term: normalised over the regions; BCE term: the weights
                        of the weighted mean), None = all ones
        :param dice_weight, bce_weight: weights of the two terms, >= 0 and not both 0
        :param gamma: focal exponent of the BCE term, >= 0 (0: binary cross-entropy)
        :param batch_dice: sum the Dice term's numerators and denominators over the batch before the ratio
        :param ignore_label: label id whose voxels are left out of the loss (None: only values that are no label are);
                        it may not sit in a region
        """
        super(RegionDiceBCELoss, self).__init__()
        self.regions = check_regions(regions)
        num = len(self.regions)
        weights = [1.0] * num if weights is None else [float(w) for w in weights]
        if len(weights) != num:
            raise ValueError('weights has {} entries for {} regions'.format(len(weights), num))
        if not all(w > 0.0 and math.isfinite(w) for w in weights):
            raise ValueError('region weights must be positive and finite, got {}'.format(weights))
        dice_weight, bce_weight, gamma = float(dice_weight), float(bce_weight), float(gamma)
        if not (dice_weight >= 0.0 and bce_weight >= 0.0) or (dice_weight == 0.0 and bce_weight == 0.0):
            raise ValueError('dice_weight and bce_weight must be >= 0 and not both 0, got {} and {}'.format(dice_weight,
                                                                                                          bce_weight))
        if not (gamma >= 0.0 and math.isfinite(gamma)):
            raise ValueError('gamma must be finite and >= 0, got {}'.format(gamma))
        if ignore_label is not None:
            ignore_label = float(ignore_label)
            if any(ignore_label == l for region in self.regions for l in region):
                raise ValueError('ignore_label {:g} is a label of a region'.format(ignore_label))
        self.num_regions = num
        self.lut = region_lut(self.regions)
        self.dice_weight, self.bce_weight, self.gamma = dice_weight, bce_weight, gamma
        self.batch_dice = bool(batch_dice)
        self.ignore_label = ignore_label
        total = math.fsum(weights)
        self.dice_weights = torch.tensor([w / total for w in weights], dtype=torch.float64).float()
        self.bce_weights = torch.tensor(weights, dtype=torch.float32)
        self.last_terms = None

    def forward(self, input_tensor, target):
        """
        :param input_tensor: sigmoid probabilities [N, R, D, H, W] (any trailing spatial shape), float32
        :param target: ground truth label ids, float, [N, 1, D, H, W]
        :return: the loss (0-dim tensor, differentiable w.r.t. input_tensor); `.last_terms` then holds the device tensor
                 (L, L_dice, L_bce) of this call, written without a synchronisation
        """
        from segmentation3d import _ops
        if input_tensor.dim() < 3 or input_tensor.shape[1] != self.num_regions:
            raise ValueError('input of shape {} does not have {} region channels'.format(tuple(input_tensor.shape),
                                                                                       self.num_regions))
        if target.numel() * self.num_regions != input_tensor.numel():
            raise ValueError('target shape {} does not match input {}'.format(tuple(target.shape),
                                                                              tuple(input_tensor.shape)))
        if self.dice_weights.device != input_tensor.device:
            self.dice_weights = self.dice_weights.to(input_tensor.device)
            self.bce_weights = self.bce_weights.to(input_tensor.device)
        ignore = -1.0 if self.ignore_label is None else self.ignore_label   # outside [0, 256): no ignore label
        loss, self.last_terms = _ops.RegionLossFunction.apply(
            input_tensor, target, self.lut, self.dice_weights, self.bce_weights, self.gamma, self.dice_weight,
            self.bce_weight, self.batch_dice, ignore)
        return loss
