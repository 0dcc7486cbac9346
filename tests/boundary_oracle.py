"""Float64 oracle of the boundary loss, shared by tests/test_boundary_loss.py and
tests/test_gpu_boundary_loss.py: the signed distance map by brute force over all voxel pairs in numpy float64, and the loss
restated in float64 torch (differentiable, so autograd supplies the reference gradient).  No scipy here."""
import numpy as np
import torch

from test_compound_loss import oracle as compound_oracle


def counted_mask(t, num_class=None, ignore_label=None):
    """the counting rule: 0 <= t < C and t != ignore_label (num_class None: every non-negative id)"""
    t = np.asarray(t, dtype=np.float64)
    valid = t >= 0
    if num_class is not None:
        valid &= t < num_class
    if ignore_label is not None:
        valid &= t != float(ignore_label)
    return valid


def signed_distance_oracle(t, class_ids, spacing, num_class=None, ignore_label=None, squared=False):
    """phi [N, K, Z, Y, X] float64 for the class-id volume t [N, Z, Y, X]; spacing = (sx, sy, sz), x the last axis.
    phi = +d(v, G) on H, -d(v, H) on G, 0 on voxels that do not count and where G or H is empty.  Every pair (query,
    feature) is evaluated; with squared=True also returns the non-negative squared distances (exact integers in float64 for
    unit spacing)."""
    t = np.asarray(t, dtype=np.float64)
    N, Z, Y, X = t.shape
    sx, sy, sz = (float(s) for s in spacing)
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    pos = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1).astype(np.float64)
    w = np.array([sx * sx, sy * sy, sz * sz])
    valid = counted_mask(t, num_class, ignore_label).reshape(N, -1)
    cls = np.trunc(t).reshape(N, -1)
    phi = np.zeros((N, len(class_ids), Z * Y * X))
    d2 = np.zeros_like(phi)
    for n in range(N):
        for k, c in enumerate(class_ids):
            G = np.flatnonzero(valid[n] & (cls[n] == c))
            H = np.flatnonzero(valid[n] & (cls[n] != c))
            if len(G) == 0 or len(H) == 0:
                continue
            diff = pos[H][:, None, :] - pos[G][None, :, :]                 # [|H|, |G|, 3]
            D = (diff * diff * w).sum(-1)
            d2[n, k, H] = D.min(1)
            d2[n, k, G] = D.min(0)
            phi[n, k, H] = np.sqrt(d2[n, k, H])
            phi[n, k, G] = -np.sqrt(d2[n, k, G])
    shape = (N, len(class_ids), Z, Y, X)
    if squared:
        return phi.reshape(shape), d2.reshape(shape)
    return phi.reshape(shape)


def boundary_oracle(p, t, phi, weights=None, dice_weight=1.0, boundary_weight=0.01, include_background=True,
                    batch_dice=False, ignore_label=None):
    """(L, L_region, L_boundary) as float64 0-dim tensors.  p [N, C, Z, Y, X], t [N, 1, Z, Y, X] float class ids, phi
    [N, |K|, Z, Y, X] the signed distance maps of the classes K (all, or 1 .. C-1 without the background) -- the oracle's
    own or the kernel's, so that the reduction can be judged on its own."""
    N, C = p.shape[0], p.shape[1]
    P = p.double().reshape(N, C, -1)
    T = t.reshape(N, -1).double()
    valid = (T >= 0) & (T < C)
    if ignore_label is not None:
        valid = valid & (T != float(ignore_label))
    v = valid.double()
    w = torch.ones(C, dtype=torch.float64) if weights is None else torch.tensor([float(x) for x in weights], dtype=torch.float64)
    K = list(range(C)) if include_background else list(range(1, C))
    PHI = torch.as_tensor(np.asarray(phi), dtype=torch.float64).reshape(N, len(K), -1)
    wsum = sum(w[c] for c in K)
    n_counted = max(1.0, float(v.sum()))
    l_boundary = sum((w[c] / wsum) * (PHI[:, i] * P[:, c] * v).sum() for i, c in enumerate(K)) / n_counted
    _, l_region, _ = compound_oracle(p, t, weights=weights, dice_weight=1.0, ce_weight=0.0,
                                     include_background=include_background, batch_dice=batch_dice, ignore_label=ignore_label)
    total = dice_weight * l_region + boundary_weight * l_boundary
    return total, l_region, l_boundary
