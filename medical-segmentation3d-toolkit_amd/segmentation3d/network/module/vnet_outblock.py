"""OutputBlock: the V-Net head (reference: network/module/vnet_outblock.py:4-24).

features -> 3x3x3 conv to `out_channels` classes -> GroupNorm -> ReLU -> 1x1x1 conv -> GroupNorm -> Softmax over the
class axis; returns contiguous [N, classes, D, H, W] probabilities.  Reference attribute names: `conv1`, `gn1`, `act1`,
`conv2`, `gn2`, `softmax`.

`activation='sigmoid'` (region-based training, not in the reference) ends in an element-wise `sigmoid` instead: one
probability per region.  Neither activation has parameters, so the state_dict keys are the same.
"""
import torch.nn as nn

from segmentation3d.network.module.layers import Sigmoid, Softmax, attach_unit, run_unit

_FIRST, _SECOND = ('conv1', 'gn1', 'act1'), ('conv2', 'gn2', None)
ACTIVATIONS = ('softmax', 'sigmoid')


def check_activation(activation):
    if activation not in ACTIVATIONS:
        raise ValueError("unknown output activation {!r}: 'softmax' or 'sigmoid'".format(activation))
    return activation


class OutputBlock(nn.Module):

    def __init__(self, in_channels, out_channels, activation='softmax'):
        super(OutputBlock, self).__init__()
        self.activation = check_activation(activation)
        attach_unit(self, _FIRST, 'k3', in_channels, out_channels)
        attach_unit(self, _SECOND, 'k1', out_channels, out_channels, act=False)
        if self.activation == 'sigmoid':
            self.sigmoid = Sigmoid()
        else:
            self.softmax = Softmax(dim=1)

    def forward(self, input):
        hidden = run_unit(self, _FIRST, input, relu=True)
        logits = run_unit(self, _SECOND, hidden, relu=False)
        return self.sigmoid(logits) if self.activation == 'sigmoid' else self.softmax(logits)
