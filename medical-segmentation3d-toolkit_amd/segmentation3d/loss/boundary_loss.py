"""DiceBoundaryLoss -- soft Dice + boundary (signed-distance) loss of Kervadec et al. (MIDL 2019) on the network's
probabilities, with the distance maps computed on the device every call.  The reference has no such loss; the definitions
are this project's.

Input `p` [N, C, Z, Y, X] float32 probabilities, target `t` [N, 1, Z, Y, X] float class ids, voxel spacing (sx, sy, sz) in
mm.  A voxel counts iff 0 <= t < C and t != ignore_label (the rule of DiceCELoss); every other voxel is a feature of no
distance transform, enters no sum and gets a zero gradient.

  distance map:   for sample n and class c in K (all classes, or 1 .. C-1 without the background):
                  G = counted voxels of class c, H = counted voxels of the other classes;
                  phi[n,c](v) = +d(v, G) on H, -d(v, H) on G, d = sqrt(sx^2 dx^2 + sy^2 dy^2 + sz^2 dz^2) between voxel
                  centres.  This is the plain signed map edt(~m) - edt(m), WITHOUT the "- 1" offset of Kervadec's reference
                  code.  G or H empty in a sample: phi[n,c] = 0.  Nothing exists outside the crop.
  boundary term:  L_boundary = sum_{c in K} w'_c (sum_{n, counted v} phi[n,c](v) p[n,c](v)) / max(1, n_counted); it may be
                  negative.  w' = weights normalised over K, n_counted = counted voxels of this rank's batch.
  region term:    L_region of DiceCELoss, unchanged and computed by the same device code (bit-equal).
  loss:           L = dice_weight * L_region + boundary_weight * L_boundary.
  gradient:       dL/dp[n,c,v] = (A t_c + B) + boundary_weight w'_c phi[n,c](v) / max(1, n_counted) on counted voxels.

`boundary_weight` lives in a one-element device tensor that the kernels read: `set_boundary_weight` changes it with a plain
fill between steps, so a train step captured into a hipGraph follows a schedule (`boundary_schedule_from_config` in
core/seg_train.py is Kervadec's "increase" strategy).  Every axis of the crop is at most 256 voxels.  One loss object serves
one resolution: deep supervision would call it at levels whose spacing is 2^k times the nominal one, which TrainStep
refuses.  Under data parallelism n_counted is this rank's own -- there is no collective.
"""
import math

import torch
import torch.nn as nn

from segmentation3d import _ops
from segmentation3d.loss.compound_loss import class_weight_tensors

MAX_AXIS = 256


def _check_boundary_weight(w):
    w = float(w)
    if not (math.isfinite(w) and w >= 0.0):
        raise ValueError('boundary_weight must be finite and >= 0, got {}'.format(w))
    return w


class DiceBoundaryLoss(nn.Module):
    """ soft Dice + boundary loss on signed distance maps computed on the device """

    def __init__(self, num_class, weights=None, dice_weight=1.0, boundary_weight=0.01, spacing=(1, 1, 1),
                 include_background=True, batch_dice=False, ignore_label=None, use_gpu=True):
        """
        :param num_class: the number of classes C (channels of the input)
        :param weights: positive weight per class, normalised over the included classes; None = all ones
        :param dice_weight: weight of the soft-Dice term, >= 0
        :param boundary_weight: initial weight of the boundary term, finite and >= 0 (see set_boundary_weight)
        :param spacing: voxel spacing (sx, sy, sz) of the crops in mm, three positive finite numbers
        :param include_background: False leaves class 0 out of both terms
        :param batch_dice: sum the region term's numerators and denominators over the batch before the ratio
        :param ignore_label: target value whose voxels are left out of the loss (None: only out-of-range ids are)
        :param use_gpu: kept for signature compatibility; the buffers follow the input's device
        """
        super(DiceBoundaryLoss, self).__init__()
        num_class = int(num_class)
        if not 1 <= num_class <= 16:
            raise ValueError('num_class must be in 1..16, got {}'.format(num_class))
        self.region_weights, _ = class_weight_tensors(num_class, weights, include_background, require_finite=True)
        dice_weight = float(dice_weight)
        if not (math.isfinite(dice_weight) and dice_weight >= 0.0):
            raise ValueError('dice_weight must be finite and >= 0, got {}'.format(dice_weight))
        self.num_class = num_class
        self.dice_weight = dice_weight
        self.spacing = _ops._spacing3(spacing)
        self.include_background = bool(include_background)
        self.batch_dice = bool(batch_dice)
        self.ignore_label = None if ignore_label is None else float(ignore_label)
        self._boundary_weight = _check_boundary_weight(boundary_weight)
        self._weight_dev = None   # the device scalar, created on the first call's device
        self.use_gpu = use_gpu
        self.last_terms = None

    @property
    def boundary_weight(self):
        """the host copy of the boundary term's weight"""
        return self._boundary_weight

    def set_boundary_weight(self, w):
        """new weight of the boundary term, finite and >= 0: one fill of the device scalar, to be called between steps
        (outside any graph capture); a captured step replayed afterwards uses the new value"""
        self._boundary_weight = _check_boundary_weight(w)
        if self._weight_dev is not None:
            self._weight_dev.fill_(self._boundary_weight)

    def forward(self, input_tensor, target):
        """
        :param input_tensor: network output probabilities [N, C, Z, Y, X], float32
        :param target: ground truth class ids, float, [N, 1, Z, Y, X]
        :return: the loss (0-dim tensor, differentiable w.r.t. input_tensor); `.last_terms` then holds the device tensor
                 (L, L_region, L_boundary) of this call, written without a synchronisation
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
        if self._weight_dev is None or self._weight_dev.device != input_tensor.device:
            if input_tensor.is_cuda and torch.cuda.is_current_stream_capturing():
                # a fill captured here would put the weight back at every replay
                raise RuntimeError('DiceBoundaryLoss: call the loss once on this device before capturing it into a graph')
            self._weight_dev = torch.full((1,), self._boundary_weight, dtype=torch.float32, device=input_tensor.device)
        ignore = -1.0 if self.ignore_label is None else self.ignore_label
        loss, self.last_terms = _ops.BoundaryLossFunction.apply(
            input_tensor, target, self.region_weights, self._weight_dev, self.spacing, self.dice_weight,
            self.include_background, self.batch_dice, ignore)
        return loss
