"""Oracle of the Dice + clDice loss, shared by tests/test_cldice_loss.py and
tests/test_gpu_cldice_loss.py: stock torch on the CPU with autograd, in float64 by default (`dtype=torch.float32` is the
"same arithmetic in stock fp32" run the GPU bars are derived from).  Written from the definitions:

  E(x) = min over the voxel and its 6 face neighbours = the min of three line pools -max_pool3d(-x) along z, y and x;
  D(x) = max_pool3d(x, 3, 1, 1);  max_pool3d pads with -inf, which is the "nothing exists outside the volume" rule;
  x_0 = x, s_0 = relu(x_0 - D(E(x_0)));  x_j = E(x_{j-1}), d_j = relu(x_j - D(E(x_j))), s_j = s_{j-1} + relu(d_j - s_{j-1} d_j).
"""
import torch
import torch.nn.functional as F

EPS = 1e-5   # the compound loss's Dice smoothing


def erode(x):
    """E on [B, 1, Z, Y, X]"""
    a = -F.max_pool3d(-x, (3, 1, 1), 1, (1, 0, 0))
    b = -F.max_pool3d(-x, (1, 3, 1), 1, (0, 1, 0))
    c = -F.max_pool3d(-x, (1, 1, 3), 1, (0, 0, 1))
    return torch.min(torch.min(a, b), c)


def dilate(x):
    """D on [B, 1, Z, Y, X]"""
    return F.max_pool3d(x, 3, 1, 1)


def soft_skeleton_oracle(x, iters):
    """skel_iters of every volume of x [..., Z, Y, X]; same shape and dtype, differentiable"""
    shape = x.shape
    x = x.reshape((-1, 1) + tuple(shape[-3:]))
    s = torch.relu(x - dilate(erode(x)))
    for _ in range(int(iters)):
        x = erode(x)
        d = torch.relu(x - dilate(erode(x)))
        s = s + torch.relu(d - s * d)
    return s.reshape(shape)


def cldice_oracle(p, t, weights=None, dice_weight=1.0, cldice_weight=1.0, iters=3, cldice_classes=None,
                  include_background=True, batch_dice=False, ignore_label=None, dtype=torch.float64, skeletons=False):
    """(L, L_dice, L_cl) as 0-dim tensors of `dtype`; p [N, C, Z, Y, X], t [N, 1, Z, Y, X] float class ids.
    skeletons=True also returns SP [N, |K|, Z, Y, X]."""
    N, C = p.shape[0], p.shape[1]
    P = p.to(dtype)
    T = t.reshape((N,) + tuple(p.shape[2:])).double()
    valid = (T >= 0) & (T < C)
    if ignore_label is not None:
        valid = valid & (T != float(ignore_label))
    m = valid.to(dtype)
    w = torch.ones(C, dtype=dtype) if weights is None else torch.tensor([float(x) for x in weights], dtype=dtype)
    onehot = torch.stack([((T == c) & valid).to(dtype) for c in range(C)], dim=1)          # T_c, [N, C, Z, Y, X]
    Pm = P * m[:, None]                                                                    # P_c
    # the compound loss's soft-Dice term
    KD = list(range(C)) if include_background else list(range(1, C))
    I = (Pm * onehot).flatten(2).sum(-1)
    U = Pm.flatten(2).sum(-1) + onehot.flatten(2).sum(-1)
    if batch_dice:
        I, U = I.sum(0, keepdim=True), U.sum(0, keepdim=True)
    d = (2.0 * I + EPS) / (U + EPS)
    wsum = sum(w[c] for c in KD)
    l_dice = sum((w[c] / wsum) * (1.0 - d[:, c].mean()) for c in KD)
    # the clDice term
    K = list(range(1, C)) if cldice_classes is None else [int(c) for c in cldice_classes]
    SP = soft_skeleton_oracle(Pm[:, K], iters)
    ST = soft_skeleton_oracle(onehot[:, K], iters)
    s0 = (SP * onehot[:, K]).flatten(2).sum(-1)
    s1 = SP.flatten(2).sum(-1)
    s2 = (ST * Pm[:, K]).flatten(2).sum(-1)
    s3 = ST.flatten(2).sum(-1)
    if batch_dice:
        s0, s1, s2, s3 = (v.sum(0, keepdim=True) for v in (s0, s1, s2, s3))
    tprec = (s0 + 1.0) / (s1 + 1.0)
    tsens = (s2 + 1.0) / (s3 + 1.0)
    cl = 2.0 * tprec * tsens / (tprec + tsens)                                             # [N or 1, |K|]
    wk = sum(w[c] for c in K)
    l_cl = sum((w[c] / wk) * (1.0 - cl[:, i].mean()) for i, c in enumerate(K))
    total = torch.zeros((), dtype=dtype)
    if dice_weight > 0.0:
        total = total + dice_weight * l_dice
    if cldice_weight > 0.0:
        total = total + cldice_weight * l_cl
    if skeletons:
        return total, l_dice, l_cl, SP
    return total, l_dice, l_cl
