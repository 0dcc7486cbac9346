"""DiceClDiceLoss -- soft Dice + soft-clDice topology loss (Shit et al., CVPR 2021, "clDice -- a Novel Topology-Preserving
Loss Function for Tubular Structure Segmentation") on the network's probabilities, with the differentiable soft skeletons
of the prediction and of the target computed on the device every call.  The reference has no such loss; the definitions
are this project's.

Input `p` [N, C, Z, Y, X] float32 probabilities, target `t` [N, 1, Z, Y, X] float class ids.  A voxel counts iff
0 <= t < C and t != ignore_label (the rule of DiceCELoss); m(v) is 1 on counted voxels and 0 elsewhere.  For a class c:
P_c = m p_c and T_c = m [t == c] -- a voxel that does not count is background for both skeletons, enters no sum and gets a
zero gradient (an un-annotated slab ends a vessel).

  morphology:     nothing exists outside the volume.  E(x)(v) = min of x over v and its 6 face neighbours inside the volume;
                  D(x)(v) = max of x over the 3x3x3 neighbourhood inside the volume;  O(x) = D(E(x)).
  soft skeleton:  x_0 = x, s_0 = relu(x_0 - O(x_0));  for j = 1..k:  x_j = E(x_{j-1}),  d_j = relu(x_j - O(x_j)),
                  s_j = s_{j-1} + relu(d_j - s_{j-1} d_j);  skel_k(x) = s_k  (the published soft_skel, k = `iters`).
  clDice term:    per sample n and class c of the class list K (default: the foreground classes 1 .. C-1):
                  SP = skel_k(P_c), ST = skel_k(T_c),  Tprec = (sum SP T_c + 1) / (sum SP + 1),
                  Tsens = (sum ST P_c + 1) / (sum ST + 1),  cl = 2 Tprec Tsens / (Tprec + Tsens);
                  L_cl = sum_{c in K} w'_c (1 - mean_n cl[n,c]),  w' = the class weights normalised over K.
                  batch_dice sums the four sums over n before the ratios, as the Dice term does.
  region term:    L_dice of DiceCELoss, unchanged and computed by the same device code (bit-equal); include_background
                  applies to this term only.
  loss:           L = dice_weight * L_dice + cldice_weight * L_cl.
  gradient:       relu' is 1 for a positive argument and 0 otherwise; a min or max sends its gradient to one position that
                  attains it -- among several, the one with the lowest linear index (z, then y, then x).  For planes whose
                  values are pairwise distinct the gradient does not depend on that choice.

Nothing in the loss depends on the voxel spacing, so one object serves every level of a DeepSupervisionLoss, with the same
iteration count at every level.  Every axis of the crop is at most 256 voxels.
"""
import math

import torch.nn as nn
import torch

from segmentation3d import _ops
from segmentation3d.loss.compound_loss import class_weight_tensors

MAX_AXIS = 256
MAX_ITERS = 16


def cldice_class_list(num_class, cldice_classes):
    """the validated class list K of the clDice term: None = the foreground classes 1 .. C-1; otherwise 1..16 distinct
    ids in 1 .. C-1.  ValueError for an empty list, duplicates, the background or an id out of range."""
    if cldice_classes is None:
        ids = list(range(1, num_class))
    else:
        try:
            ids = [int(c) for c in cldice_classes]
        except TypeError:
            raise ValueError('cldice_classes must be a list of class ids, got {!r}'.format(cldice_classes))
        if any(float(c) != float(i) for c, i in zip(cldice_classes, ids)):
            raise ValueError('cldice_classes must hold integer class ids, got {!r}'.format(cldice_classes))
    if not ids:
        raise ValueError('cldice_classes is empty (num_class = {} has no foreground class)'.format(num_class)
                         if cldice_classes is None else 'cldice_classes is empty')
    if len(set(ids)) != len(ids):
        raise ValueError('cldice_classes has duplicates: {}'.format(ids))
    if any(c == 0 for c in ids):
        raise ValueError('cldice_classes must not contain the background class 0')
    if any(not 1 <= c < num_class for c in ids):
        raise ValueError('cldice_classes {} out of range 1..{}'.format(ids, num_class - 1))
    return ids


class DiceClDiceLoss(nn.Module):
    """ soft Dice + soft-clDice on soft skeletons computed on the device """

    def __init__(self, num_class, weights=None, dice_weight=1.0, cldice_weight=1.0, iters=3, cldice_classes=None,
                 include_background=True, batch_dice=False, ignore_label=None, use_gpu=True):
        """
        :param num_class: the number of classes C (channels of the input), 2..16
        :param weights: positive finite weight per class; the Dice term normalises them over its included classes, the
                        clDice term over its class list; None = all ones
        :param dice_weight, cldice_weight: weights of the two terms, finite, >= 0 and not both 0
        :param iters: iterations k of the soft skeleton, 1..16 (about the largest radius of the structures in voxels)
        :param cldice_classes: class ids of the clDice term, distinct, in 1 .. C-1; None = every foreground class
        :param include_background: False leaves class 0 out of the Dice term
        :param batch_dice: sum both terms' numerators and denominators over the batch before the ratios
        :param ignore_label: target value whose voxels are left out of the loss (None: only out-of-range ids are)
        :param use_gpu: kept for signature compatibility; the buffers follow the input's device
        """
        super(DiceClDiceLoss, self).__init__()
        num_class = int(num_class)
        if not 2 <= num_class <= 16:
            raise ValueError('num_class must be in 2..16, got {}'.format(num_class))
        self.region_weights, class_weights = class_weight_tensors(num_class, weights, include_background,
                                                                  require_finite=True)
        dice_weight, cldice_weight = float(dice_weight), float(cldice_weight)
        for name, w in (('dice_weight', dice_weight), ('cldice_weight', cldice_weight)):
            if not (math.isfinite(w) and w >= 0.0):
                raise ValueError('{} must be finite and >= 0, got {}'.format(name, w))
        if dice_weight == 0.0 and cldice_weight == 0.0:
            raise ValueError('dice_weight and cldice_weight must not both be 0')
        if isinstance(iters, bool) or int(iters) != iters or not 1 <= int(iters) <= MAX_ITERS:
            raise ValueError('iters must be an integer in 1..{}, got {!r}'.format(MAX_ITERS, iters))
        self.cldice_classes = cldice_class_list(num_class, cldice_classes)
        picked = class_weights.double()[self.cldice_classes]
        self.cldice_weights = (picked / picked.sum()).float()
        self.num_class = num_class
        self.dice_weight = dice_weight
        self.cldice_weight = cldice_weight
        self.iters = int(iters)
        self.include_background = bool(include_background)
        self.batch_dice = bool(batch_dice)
        self.ignore_label = None if ignore_label is None else float(ignore_label)
        self.use_gpu = use_gpu
        self.last_terms = None

    def forward(self, input_tensor, target):
        """
        :param input_tensor: network output probabilities [N, C, Z, Y, X], float32
        :param target: ground truth class ids, float, [N, 1, Z, Y, X]
        :return: the loss (0-dim tensor, differentiable w.r.t. input_tensor); `.last_terms` then holds the device tensor
                 (L, L_dice, L_cl) of this call, written without a synchronisation
        """
        if input_tensor.dim() != 5 or input_tensor.shape[1] != self.num_class:
            raise ValueError('input of shape {} is not [N, {}, Z, Y, X]'.format(tuple(input_tensor.shape), self.num_class))
        if target.numel() * self.num_class != input_tensor.numel():
            raise ValueError('target shape {} does not match input {}'.format(tuple(target.shape),
                                                                              tuple(input_tensor.shape)))
        if max(input_tensor.shape[2:]) > MAX_AXIS:
            raise ValueError('every axis of the crop must be at most {} voxels, got {}'.format(
                MAX_AXIS, tuple(input_tensor.shape[2:])))
        if self.region_weights.device != input_tensor.device:
            self.region_weights = self.region_weights.to(input_tensor.device)
            self.cldice_weights = self.cldice_weights.to(input_tensor.device)
        ignore = -1.0 if self.ignore_label is None else self.ignore_label
        loss, self.last_terms = _ops.ClDiceLossFunction.apply(
            input_tensor, target, self.region_weights, self.cldice_weights, self.cldice_classes, self.iters,
            self.dice_weight, self.cldice_weight, self.batch_dice, ignore)
        return loss
