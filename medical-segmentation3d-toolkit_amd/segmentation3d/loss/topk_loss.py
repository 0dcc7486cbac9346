"""DiceTopKLoss -- soft Dice + top-k cross-entropy on the network's probabilities, with an ignore label (nnU-Net's
DC_and_topk_loss).  The reference has no such loss; the definitions are this project's.

Input `p` [N, C, *spatial] float32 probabilities, target `t` [N, 1, *spatial] float class ids.  A voxel counts iff
0 <= t < C and t != ignore_label (the rule of DiceCELoss); every other voxel enters no sum and gets a zero gradient.

  region term:   L_region of DiceCELoss, unchanged (weights normalised over the included classes, include_background,
                 batch_dice, eps = 1e-5) and computed by the same device code.
  per voxel:     ell_v = a_t * (-log(max(p_t, 1e-12))) in float32; a = weights, positive, NOT normalised (unit weights give
                 nnU-Net's loss); -0.0 (p_t == 1) counts as +0.0.
  count and k:   n = counted voxels of this rank's whole batch; k = max(1, int(n * k_percent / 100.0)) evaluated in double
                 (`topk_count`); n == 0: L_topk = 0, zero gradient, k = 0.
  selection:     tau = the k-th largest ell, m = #{ell > tau}, n_eq = #{ell == tau}, r = k - m.
  top-k term:    L_topk = (sum_{ell > tau} ell + r * tau) / k.
  loss:          L = dice_weight * L_region + ce_weight * L_topk; a term whose weight is 0 never enters L.
  gradient:      the top-k term sends ce_weight * w_v / k * (-a_t / p_t) (0 where p_t < 1e-12) to plane c == t, with w_v = 1
                 above tau, r / n_eq at tau -- ties share the remaining r places equally, whatever their order -- and 0 below.

tau comes from a radix select on the device (seg3d_topk_loss_fwd): nothing is read back, k follows the data (ignore
label) inside a captured hipGraph, and integer atomics only make every result bit-reproducible.  Under data parallelism n,
k and tau are this rank's own -- there is no collective.
"""
import math

from segmentation3d import _ops
from segmentation3d.loss.compound_loss import DiceCELoss


def topk_count(n, k_percent):
    """k of n counted voxels: the device's expression max(1, (long long)((double)n * k_percent / 100.0)), 0 for n == 0"""
    n = int(n)
    if n <= 0:
        return 0
    return max(1, int(float(n) * float(k_percent) / 100.0))


class DiceTopKLoss(DiceCELoss):
    """ soft Dice + cross-entropy over the hardest k_percent of the batch's counted voxels """

    def __init__(self, num_class, weights=None, dice_weight=1.0, ce_weight=1.0, k_percent=10.0, include_background=True,
                 batch_dice=False, ignore_label=None, use_gpu=True):
        """
        :param k_percent: the share of the counted voxels the cross-entropy term averages, in (0, 100]
        every other parameter: as for DiceCELoss (the distribution term's gamma is 0: there is no focal factor)
        """
        super(DiceTopKLoss, self).__init__(num_class, weights=weights, dice_weight=dice_weight, ce_weight=ce_weight,
                                           gamma=0.0, include_background=include_background, batch_dice=batch_dice,
                                           ignore_label=ignore_label, use_gpu=use_gpu)
        k_percent = float(k_percent)
        if not (math.isfinite(k_percent) and 0.0 < k_percent <= 100.0):
            raise ValueError('k_percent must be in (0, 100], got {}'.format(k_percent))
        self.k_percent = k_percent
        self.last_selection = None
        self.last_threshold = None

    def forward(self, input_tensor, target):
        """
        :return: the loss (0-dim tensor, differentiable w.r.t. input_tensor); afterwards `.last_terms` holds the device
                 tensor (L, L_region, L_topk), `.last_selection` int64 (n, k, m, n_eq, r) and `.last_threshold` the
                 float32 tau of this call, all written without a synchronisation
        """
        self._check_shapes(input_tensor, target)
        self._weights_on(input_tensor.device)
        loss, self.last_terms, self.last_selection, threshold = _ops.TopKLossFunction.apply(
            input_tensor, target, self.region_weights, self.class_weights, self.k_percent, self.dice_weight, self.ce_weight,
            self.batch_dice, self._ignore_value())
        self.last_threshold = threshold.reshape(())
        return loss
