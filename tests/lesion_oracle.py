"""SciPy / numpy restatement of the lesion-wise evaluation and of the normalized surface Dice, for the tests only.

A target is a set of label ids.  A = ground-truth voxels in the target, B = segmentation voxels in the target.
  1. A' = A dilated dilation_iters times by scipy's generate_binary_structure(3, 2) (the 18-neighbourhood, nothing outside
     the volume); 0 iterations: A' = A.
  2. lesions D_i = 26-connected components of A' (ndimage.label with the full 3 x 3 x 3 structure), RE-NUMBERED here by
     the lowest linear voxel index of each component; G_i = A n D_i.
  3. predicted components P_j = 26-connected components of B, numbered the same way.
  4. M_i = {j : P_j n D_i != {}}, U_i = union of the P_j in M_i.
  5. M_i empty: false negative, dice 0, hd95 = penalty; else dice_i = 2 |G_i n U_i| / (|G_i| + |U_i|), hd95_i = the float64
     surface oracle's HD95 between G_i and U_i.
  6. |G_i| < min_lesion_voxels: dropped after matching.   7. a P_j in no M_i (dropped lesions' included): false positive.
  8. n = kept + FP; lw_dice = sum dice / n; lw_hd95 = (sum hd95 + penalty FP) / n; (1, 0) when n = 0;
     lesion_f1 = 2 TP / (2 TP + FN + FP), 1 when the denominator is 0.
"""
import numpy as np
from scipy import ndimage

from test_gpu_surface_metrics import _ref_surface, _ref_surface_distances

_S18 = ndimage.generate_binary_structure(3, 2)
_S26 = np.ones((3, 3, 3), bool)


def target_mask(vol, target):
    ids = [target] if np.isscalar(target) else list(target)
    return np.isin(np.asarray(vol), ids)


def dilate18(mask, iters):
    mask = np.asarray(mask, bool)
    if iters == 0:          # scipy reads iterations < 1 as "until nothing changes"
        return mask.copy()
    return ndimage.binary_dilation(mask, _S18, iterations=iters, border_value=0)


def components26(mask):
    """(int32 id map, K, sizes): ids 1..K in the order of each component's lowest linear index (z * Y + y) * X + x"""
    lab, k = ndimage.label(np.asarray(mask, bool), _S26)
    flat = lab.ravel()
    values, first = np.unique(flat, return_index=True)
    keep = values > 0
    values, first = values[keep], first[keep]
    remap = np.zeros(k + 1, np.int32)
    remap[values[np.argsort(first, kind='stable')]] = np.arange(1, k + 1, dtype=np.int32)
    ids = remap[lab].astype(np.int32)
    sizes = np.bincount(ids.ravel(), minlength=k + 1)[1:].tolist()
    return ids, int(k), sizes


def pair_table(gt, seg, target, dilation_iters):
    """everything the device reports as integers: (Dmap, Kg, Pmap, Kp, psizes, |G_i|, |G_i n B|, sorted pairs)"""
    a, b = target_mask(gt, target), target_mask(seg, target)
    dmap, kg, _ = components26(dilate18(a, dilation_iters))
    pmap, kp, psizes = components26(b)
    gsize = np.bincount(dmap[a], minlength=kg + 1)[1:].tolist()
    inter = np.bincount(dmap[a & b], minlength=kg + 1)[1:].tolist()
    both = (dmap > 0) & (pmap > 0)
    pairs = sorted(set(zip(dmap[both].tolist(), pmap[both].tolist())))
    return dmap, kg, pmap, kp, psizes, gsize, inter, pairs


def lesionwise(gt, seg, target, spacing=(1.0, 1.0, 1.0), dilation_iters=3, min_lesion_voxels=1, hd95_penalty=374.0):
    a = target_mask(gt, target)
    dmap, kg, pmap, kp, psizes, gsize, inter, pairs = pair_table(gt, seg, target, dilation_iters)
    used, lesions = set(), []
    n_tp = n_fn = 0
    for i in range(1, kg + 1):
        ids = tuple(sorted(j for (l, j) in pairs if l == i))
        used.update(ids)
        g = a & (dmap == i)
        voxels = int(g.sum())
        assert voxels > 0
        if voxels < min_lesion_voxels:
            continue
        if ids:
            u = np.isin(pmap, ids)
            dice = 2.0 * int((g & u).sum()) / float(voxels + int(u.sum()))
            hd95 = _ref_surface_distances(g.astype(np.uint8), u.astype(np.uint8), 1, spacing)['hd95']
            n_tp += 1
        else:
            dice, hd95 = 0.0, float(hd95_penalty)
            n_fn += 1
        lesions.append((i, voxels, dice, hd95, ids))
    n_fp = kp - len(used)
    n = len(lesions) + n_fp
    den = 2 * n_tp + n_fn + n_fp
    return {'lw_dice': sum(l[2] for l in lesions) / n if n else 1.0,
            'lw_hd95': (sum(l[3] for l in lesions) + float(hd95_penalty) * n_fp) / n if n else 0.0,
            'n_gt': len(lesions), 'n_tp': n_tp, 'n_fn': n_fn, 'n_fp': n_fp,
            'lesion_f1': 2.0 * n_tp / den if den else 1.0, 'lesions': lesions}


def nsd(gt, seg, label, spacing=(1.0, 1.0, 1.0), tau=1.0):
    """normalized surface Dice at tolerance tau: squared float64 distances against tau * tau; NaN when a mask is empty"""
    a, b = np.asarray(gt) == label, np.asarray(seg) == label
    if not a.any() or not b.any():
        return float('nan')
    sx, sy, sz = spacing
    sa, sb = _ref_surface(a), _ref_surface(b)
    within = 0
    for query, feature in ((sa, sb), (sb, sa)):
        if spacing == (1.0, 1.0, 1.0):      # exact integers
            d2 = np.round(ndimage.distance_transform_edt(~feature)[query] ** 2)
        else:
            d2 = ndimage.distance_transform_edt(~feature, sampling=(sz, sy, sx))[query] ** 2
        within += int((d2 <= tau * tau).sum())
    return within / float(int(sa.sum()) + int(sb.sum()))
