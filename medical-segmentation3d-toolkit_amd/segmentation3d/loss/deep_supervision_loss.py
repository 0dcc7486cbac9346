"""DeepSupervisionLoss -- the weighted sum of one loss per decoder resolution.  The reference trains on the full-resolution
output only; the definitions are this project's.

Input: the list [p_0, p_1, .., p_L] that `net.forward_deep` returns (p_k: probabilities at 1 / 2^k resolution) and the
full-resolution target [N, 1, D, H, W] of float class ids.  Level k is scored against the nearest-neighbour label map
t_k = t[:, :, ::2^k, ::2^k, ::2^k] (one launch writes all L of them, _ops.label_pyramid; values are copied, so an ignore
label or an out-of-range id keeps its meaning at every level) with the SAME base loss:

    L = sum_k w_k base(p_k, t_k),      default w_k = 2^-k / sum_j 2^-j,  k = 0..L

Explicit weights are normalised to sum 1.  The coarse levels reach the decoder early in backward; level 0 alone trains the
layers above 1/2 resolution.
"""
import torch
import torch.nn as nn

from segmentation3d import _ops

MAX_LEVELS = 3


def normalise_level_weights(levels, weights=None):
    """the normalised per-level weights (w_0, .., w_L) as a list of floats"""
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= MAX_LEVELS:
        raise ValueError('levels must be an integer in 1..{}, got {!r}'.format(MAX_LEVELS, levels))
    if weights is None:
        weights = [2.0 ** -k for k in range(levels + 1)]
    try:
        weights = [float(w) for w in weights]
    except (TypeError, ValueError):
        raise ValueError('weights must be a sequence of {} numbers, got {!r}'.format(levels + 1, weights))
    if len(weights) != levels + 1:
        raise ValueError('weights has {} entries for {} levels (one per level, the full resolution included)'.format(
            len(weights), levels))
    if not all(w >= 0.0 and w == w and w != float('inf') for w in weights) or not weights[0] > 0.0:
        raise ValueError('weights must be finite and >= 0 with weights[0] > 0, got {}'.format(weights))
    total = sum(weights)
    return [w / total for w in weights]


class DeepSupervisionLoss(nn.Module):
    """ sum_k w_k base_loss(p_k, target down-sampled by 2^k) over the outputs of net.forward_deep """

    def __init__(self, base_loss, levels, weights=None):
        """
        :param base_loss: the per-level loss, called as base_loss(probabilities, target) (any loss of build_loss)
        :param levels: the number L of auxiliary levels, 1..3 (the network's `deep_supervision`)
        :param weights: L + 1 non-negative weights, weights[0] > 0, normalised to sum 1; None = halving per level
        """
        super(DeepSupervisionLoss, self).__init__()
        self.weights = normalise_level_weights(levels, weights)
        self.levels = levels
        self.base_loss = base_loss
        self.last_terms = None
        self.last_levels = None

    def forward(self, outputs, target):
        """
        :param outputs: [p_0, .., p_L], p_k [N, C, D / 2^k, H / 2^k, W / 2^k]
        :param target: ground truth class ids, float, [N, 1, D, H, W]
        :return: the combined loss (0-dim tensor); `.last_levels` then holds the device tensor of the L + 1 per-level
                 losses and, for a compound base loss, `.last_terms` that loss's terms at level 0 (no synchronisation)
        """
        if not isinstance(outputs, (list, tuple)) or len(outputs) != self.levels + 1:
            raise ValueError('expected the {} outputs of forward_deep, got {}'.format(
                self.levels + 1, len(outputs) if isinstance(outputs, (list, tuple)) else type(outputs).__name__))
        targets = [target] + _ops.label_pyramid(target, self.levels)
        total, per_level, terms0 = None, [], None
        for k, (p, t, w) in enumerate(zip(outputs, targets, self.weights)):
            if tuple(p.shape[2:]) != tuple(t.shape[-3:]):
                raise ValueError('output {} has spatial shape {} but its label map has {}'.format(k, tuple(p.shape[2:]),
                                                                                                tuple(t.shape[-3:])))
            level = self.base_loss(p, t)
            if k == 0:
                terms0 = getattr(self.base_loss, 'last_terms', None)
            per_level.append(level.detach().reshape(()))
            if w == 0.0:
                continue          # the level is reported but trains nothing
            total = level * w if total is None else total + level * w
        if hasattr(self.base_loss, 'last_terms'):
            self.base_loss.last_terms = terms0
        self.last_terms = terms0
        self.last_levels = torch.stack(per_level)
        return total
