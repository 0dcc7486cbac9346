"""Dice evaluation metric with the reference's name and return convention (utils/metrics.py:5-37 `cal_dsc`):
(dsc, seg_type) with seg_type in {'TN', 'FP', 'FN', 'TP'} decided by the voxel-count threshold; and the surface-distance
metrics HD / HD95 / ASSD / NSD (`cal_surface_distances`) and the lesion-wise Dice / HD95 with lesion detection counts
(`cal_lesionwise`), which the reference does not have.

The counting runs on the GPU: ONE pass over the two label volumes (libseg3d_hip.so: seg3d_label_overlap_counts)
yields area_gt / area_seg / intersection for every requested label; the reference makes three numpy passes per label.
Inputs may be Image3d, numpy arrays or torch tensors (host data is uploaded; device tensors are used in place).
"""
import ctypes
import math

import numpy as np
import torch

from segmentation3d import _engine as E
from segmentation3d.utils.image3d import Image3d

_DTYPE_CODES = {torch.int8: 0, torch.uint8: 1, torch.int16: 2, torch.int32: 3, torch.float32: 4}
MAX_LABELS_PER_PASS = 16


def _as_device_labels(vol, device):
    if isinstance(vol, Image3d):
        vol = vol.array
    if isinstance(vol, np.ndarray):
        if vol.dtype == np.float64:
            vol = vol.astype(np.float32)
        elif vol.dtype in (np.int64, np.uint16, np.uint32, np.uint64):
            vol = vol.astype(np.int32)
        elif vol.dtype == np.bool_:
            vol = vol.astype(np.uint8)
        vol = torch.from_numpy(np.array(vol, order='C'))   # private writable copy (file readers return read-only views)
    if not isinstance(vol, torch.Tensor):
        raise TypeError('label volume must be an Image3d, a numpy array or a torch tensor')
    if vol.dtype == torch.float64:
        vol = vol.float()
    elif vol.dtype == torch.int64:
        vol = vol.int()
    elif vol.dtype == torch.bool:
        vol = vol.to(torch.uint8)
    if vol.dtype not in _DTYPE_CODES:
        raise ValueError('unsupported label dtype {}'.format(vol.dtype))
    return vol.to(device).contiguous()


def _default_device(x):
    return x.device if isinstance(x, torch.Tensor) and x.is_cuda else torch.device('cuda', torch.cuda.current_device())


def _device_pair(gt, seg, device, grid3d=False):
    """(gt, seg, device) as contiguous device tensors of one dtype; grid3d: both must be one 3-D [z, y, x] grid"""
    if device is None:
        device = _default_device(gt)
    g, s = _as_device_labels(gt, device), _as_device_labels(seg, device)
    if g.dtype != s.dtype:                      # compare in a common type, like numpy's == does
        common = torch.float32 if torch.float32 in (g.dtype, s.dtype) else torch.int32
        g, s = g.to(common), s.to(common)
    if grid3d and (g.dim() != 3 or g.shape != s.shape):
        raise ValueError('ground truth shape {} and segmentation shape {} must be one 3-D [z, y, x] grid'.format(
            tuple(g.shape), tuple(s.shape)))
    if g.numel() != s.numel():
        raise ValueError('ground truth and segmentation differ in size: {} vs {}'.format(tuple(g.shape), tuple(s.shape)))
    E.require_device(g, s)
    return g, s, device


def _overlap_counts(entry, pair, sets, table):
    """[(area_gt, area_seg, intersection)] per set, as Python ints, from one pass of `entry` over the device pair per 16
    sets; table(chunk) is the entry's host argument for a chunk of sets"""
    g, s, device = pair
    out = []
    for k0 in range(0, len(sets), MAX_LABELS_PER_PASS):
        chunk = list(sets[k0:k0 + MAX_LABELS_PER_PASS])
        counts = torch.zeros(3 * len(chunk), dtype=torch.int64, device=device)
        E.call(entry, E.ptr(g), E.ptr(s), _DTYPE_CODES[g.dtype], g.numel(), table(chunk), len(chunk), E.ptr(counts),
               E.stream_ptr())
        c = counts.cpu().tolist()
        out.extend((c[3 * k], c[3 * k + 1], c[3 * k + 2]) for k in range(len(chunk)))
    return out


def label_overlap_counts(gt, seg, labels, device=None):
    """[(area_gt, area_seg, intersection)] per label, as Python ints, from one device pass per 16 labels"""
    pair = _device_pair(gt, seg, device)
    return _overlap_counts('seg3d_label_overlap_counts', pair, [int(l) for l in labels],
                           lambda chunk: (ctypes.c_int * len(chunk))(*chunk))


def _classify(area_gt, area_seg, intersection, threshold):
    """utils/metrics.py:24-35"""
    if area_gt < threshold and area_seg < threshold:
        return 1.0, 'TN'
    if area_gt < threshold and area_seg >= threshold:
        return 0.0, 'FP'
    if area_gt >= threshold and area_seg < threshold:
        return 0.0, 'FN'
    return 2 * intersection / (area_gt + area_seg), 'TP'


def cal_dsc(gt_npy, seg_npy, label, threshold):
    """Dice ratio of one label.
    :return: (dsc, seg_type) exactly as the reference's cal_dsc"""
    (a_gt, a_seg, inter), = label_overlap_counts(gt_npy, seg_npy, [label])
    return _classify(a_gt, a_seg, inter, threshold)


def cal_dsc_labels(gt, seg, labels, threshold):
    """[(dsc, seg_type)] for several labels from a single pass over the volumes"""
    return [_classify(a, b, c, threshold) for a, b, c in label_overlap_counts(gt, seg, labels)]


def region_overlap_counts(gt, seg, regions, device=None):
    """[(area_gt, area_seg, intersection)] per region (a set of label ids: a voxel is in the region when its label is in the
    set), as Python ints, from one device pass per 16 regions (seg3d_region_overlap_counts)"""
    from segmentation3d.loss.region_loss import region_lut
    pair = _device_pair(gt, seg, device)
    return _overlap_counts('seg3d_region_overlap_counts', pair, regions,
                           lambda chunk: (ctypes.c_uint * 256)(*region_lut(chunk)))


def cal_region_dsc(gt, seg, regions, threshold):
    """[(dsc, seg_type)] per region -- cal_dsc with set membership (BraTS-style overlapping regions), one pass"""
    return [_classify(a, b, c, threshold) for a, b, c in region_overlap_counts(gt, seg, regions)]


# ---- surface-distance metrics (csrc/surface.hip) -------------------------------------------
_NAN_SURFACE = {'hd': float('nan'), 'hd95': float('nan'), 'assd': float('nan')}
_BOX_INIT = (2 ** 31 - 1,) * 3 + (-1,) * 3 + (0, 0)   # empty box, then the two surface-voxel counts


def percentile_ranks(n, q=95):
    """(lo, hi, gamma) of numpy.percentile(., q) with its default linear interpolation over n sorted values: the result
    is interpolated between the order statistics lo and hi (0-based) with weight gamma"""
    virtual = (q / 100.0) * (n - 1)
    lo = int(math.floor(virtual))
    return lo, min(lo + 1, n - 1), virtual - lo


def percentile_from_order_stats(a, b, gamma):
    """numpy's linear interpolation between the order statistics a <= b (numpy.lib._function_base_impl._lerp)"""
    diff = b - a
    return b - diff * (1.0 - gamma) if gamma >= 0.5 else a + diff * gamma


def combine_directed(ab, ba):
    """{'hd', 'hd95', 'assd'} from the two directed distance sets D_AB = {d(p, dB) : p in dA} and D_BA, each given as
    (count, max, sum, p95), or None when a label is absent (then every value is NaN)"""
    if ab is None or ba is None or ab[0] == 0 or ba[0] == 0:
        return dict(_NAN_SURFACE)
    return {'hd': float(max(ab[1], ba[1])), 'hd95': float(max(ab[3], ba[3])),
            'assd': float((ab[2] + ba[2]) / (ab[0] + ba[0]))}


def _frame(gt, seg, spacing):
    """the spacing (sx, sy, sz) to use; Image3d inputs must agree in size and spacing (relative 1e-6)"""
    images = [v for v in (gt, seg) if isinstance(v, Image3d)]
    if len(images) == 2:
        a, b = images
        if a.GetSize() != b.GetSize():
            raise ValueError('ground truth size {} and segmentation size {} differ'.format(a.GetSize(), b.GetSize()))
        if any(abs(p - q) > 1e-6 * max(abs(p), abs(q)) for p, q in zip(a.spacing, b.spacing)):
            raise ValueError('ground truth spacing {} and segmentation spacing {} differ'.format(a.spacing, b.spacing))
    if spacing is None:
        spacing = images[0].spacing if images else (1.0, 1.0, 1.0)
    spacing = tuple(float(v) for v in spacing)
    if len(spacing) != 3 or not all(v > 0 and math.isfinite(v) for v in spacing):
        raise ValueError('spacing must be three positive numbers (sx, sy, sz), got {}'.format(spacing))
    return spacing


class _SurfacePlan(object):
    """device buffers of one (gt, seg) pair: label volumes, both surface masks, box + counts, EDT workspace"""

    def __init__(self, gt, seg, spacing, device=None):
        self.spacing = _frame(gt, seg, spacing)
        g, s, device = _device_pair(gt, seg, device, grid3d=True)
        self.g, self.s, self.code = g, s, _DTYPE_CODES[g.dtype]
        self.Z, self.Y, self.X = (int(v) for v in g.shape)
        nbytes = E.query('seg3d_surface_distance_workspace_bytes', self.X, self.Y, self.Z)
        if nbytes < 0:
            raise ValueError('volume of {} voxels is too large (limit 2^31 - 1)'.format(g.numel()))
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.surf = torch.empty((2, g.numel()), dtype=torch.uint8, device=device)
        self.box = torch.empty(8, dtype=torch.int32, device=device)
        self.box_init = torch.tensor(_BOX_INIT, dtype=torch.int32, device=device)
        self.stats = torch.empty(6, dtype=torch.float64, device=device)

    def _launch_surfaces(self, volumes, code, label):
        self.box.copy_(self.box_init)
        for k, vol in enumerate(volumes):
            E.call('seg3d_label_surface', E.ptr(vol), code, self.X, self.Y, self.Z, int(label), E.ptr(self.surf[k]),
                   E.ptr(self.box), E.ptr(self.box[6 + k:7 + k]), E.stream_ptr())

    def surfaces(self, label):
        """launch: both surface masks of `label`, their common box and their voxel counts (box[6], box[7])"""
        self._launch_surfaces((self.g, self.s), self.code, label)

    def mask_surfaces(self, a, b):
        """surfaces() for two ready-made 0/1 uint8 device masks of the plan's grid (their label 1) in place of the two
        label volumes -- the per-lesion masks of cal_lesionwise"""
        self._launch_surfaces((a, b), _DTYPE_CODES[torch.uint8], 1)

    def distances(self, direction, dist2, index=None):
        """launch: squared distances of the query surface to the feature surface into dist2 (+ voxel index), and
        (count, max, sum) into stats[3 * direction ...].  direction 0: D_AB (query dA, feature dB); 1: D_BA"""
        feat, query = self.surf[1 - direction], self.surf[direction]
        sx, sy, sz = self.spacing
        E.call('seg3d_surface_distance', E.ptr(feat), E.ptr(query), self.X, self.Y, self.Z, E.ptr(self.box), sx, sy, sz,
               E.ptr(self.workspace), E.ptr(dist2), E.ptr(index), dist2.numel(), E.ptr(self.stats[3 * direction:]),
               E.stream_ptr())


def directed_surface_distances(gt, seg, label, spacing=None):
    """(voxel index, squared distance) of D_AB and of D_BA as int64 / float64 numpy arrays, sorted by voxel index
    (index = (z * Y + y) * X + x); for tests and inspection"""
    plan = _SurfacePlan(gt, seg, spacing)
    plan.surfaces(label)
    counts = plan.box[6:8].tolist()
    out = []
    for direction in (0, 1):
        n = counts[direction]
        dist2 = torch.empty(n, dtype=torch.float64, device=plan.g.device)
        index = torch.empty(n, dtype=torch.int32, device=plan.g.device)
        if n and counts[1 - direction]:
            plan.distances(direction, dist2, index)
        idx, d2 = index.cpu().numpy().astype(np.int64), dist2.cpu().numpy()
        order = np.argsort(idx, kind='stable')
        out.append((idx[order], d2[order]))
    return out


def check_nsd_tolerance(tau):
    """None, or the tolerance in millimetres as a float; ValueError unless it is finite and >= 0"""
    if tau is None:
        return None
    try:
        value = float(tau)
    except (TypeError, ValueError):
        raise ValueError('nsd_tolerance must be a number of millimetres, got {!r}'.format(tau))
    if isinstance(tau, bool) or not math.isfinite(value) or value < 0.0:
        raise ValueError('nsd_tolerance must be finite and >= 0, got {!r}'.format(tau))
    return value


def _plan_metrics(plan, nsd_tolerance=None):
    """{'hd', 'hd95', 'assd'} (+ 'nsd' with a tolerance) of the two surfaces that plan.surfaces / plan.mask_surfaces
    launched last; every value NaN when one of them is empty.  One readback of the counts, one of the statistics."""
    dev = plan.g.device
    na, nb = plan.box[6:8].tolist()
    if na == 0 or nb == 0:
        out = dict(_NAN_SURFACE)
        if nsd_tolerance is not None:
            out['nsd'] = float('nan')
        return out
    picks, ranks, within = [plan.stats], [], []
    for direction, n in enumerate((na, nb)):
        dist2 = torch.empty(n, dtype=torch.float64, device=dev)
        plan.distances(direction, dist2)
        lo, hi, gamma = percentile_ranks(n)
        ranks.append(gamma)
        # order statistics of the squared distances are those of the distances (sqrt is monotone)
        picks.append(torch.stack([torch.kthvalue(dist2, lo + 1).values, torch.kthvalue(dist2, hi + 1).values]))
        if nsd_tolerance is not None:   # fp64 squared distances against tau * tau in double, counted on the device
            within.append((dist2 <= nsd_tolerance * nsd_tolerance).sum().to(torch.float64).reshape(1))
    v = torch.cat(picks + within).tolist()
    directed = []
    for direction in (0, 1):
        count, mx, total = v[3 * direction:3 * direction + 3]
        a, b = math.sqrt(v[6 + 2 * direction]), math.sqrt(v[7 + 2 * direction])
        directed.append((int(count), mx, total, percentile_from_order_stats(a, b, ranks[direction])))
    out = combine_directed(directed[0], directed[1])
    if nsd_tolerance is not None:
        out['nsd'] = (int(v[10]) + int(v[11])) / float(na + nb)
    return out


def cal_surface_distances(gt, seg, labels, spacing=None, nsd_tolerance=None):
    """Surface-distance metrics of every label: [{'hd', 'hd95', 'assd'}] as Python floats, in physical units.

    For label l: A = (gt == l), B = (seg == l).  The surface dA is the set of voxels of A with at least one of their 6
    face neighbours outside A (voxels outside the volume count as outside A, so an object touching the border has a
    surface there).  d(p, dB) is the Euclidean distance from the centre of voxel p to the nearest centre of a dB voxel;
    only the spacing enters.  With D_AB = {d(p, dB) : p in dA} and D_BA = {d(q, dA) : q in dB}:
      HD   = max(max D_AB, max D_BA)
      HD95 = max(P95(D_AB), P95(D_BA)), P95 = numpy.percentile(., 95) with linear interpolation
      ASSD = (sum D_AB + sum D_BA) / (|D_AB| + |D_BA|), summed in fp64
      NSD  = (|{d in D_AB : d^2 <= tau^2}| + |{d in D_BA : d^2 <= tau^2}|) / (|D_AB| + |D_BA|)   (normalized surface Dice
             at tolerance tau = nsd_tolerance; key 'nsd', present only when a tolerance is given)
    If A or B is empty, all values are NaN.

    :param gt, seg: Image3d, numpy arrays or torch tensors, [z, y, x] on one grid
    :param labels: any number of labels
    :param spacing: (sx, sy, sz); default: the Image3d spacing (gt and seg must agree to a relative 1e-6), else 1, 1, 1
    :param nsd_tolerance: tau in physical units, finite and >= 0; None: no 'nsd' key
    The surfaces, the exact EDT (restricted to the box that encloses both surfaces) and the gather of the distances at
    the surface voxels run in csrc/surface.hip; HD95 takes two order statistics of the gathered distances on the device,
    NSD a count over them.
    """
    nsd_tolerance = check_nsd_tolerance(nsd_tolerance)
    plan = _SurfacePlan(gt, seg, spacing)
    results = []
    for label in labels:
        plan.surfaces(label)
        results.append(_plan_metrics(plan, nsd_tolerance))
    return results


# ---- lesion-wise evaluation (csrc/lesion.hip, csrc/postproc.hip) ---------------------------
_CCL_CAPACITY = 4096          # components whose sizes one labelling returns without a second launch
_MIN_PAIR_TABLE = 1024


def check_target(target):
    """a target of the lesion-wise path -> sorted list of distinct label ids in 1..255 (one label l is the set {l})"""
    if isinstance(target, (int, np.integer)) and not isinstance(target, bool):
        target = [target]
    if isinstance(target, (str, bytes)) or not hasattr(target, '__iter__'):
        raise ValueError('a lesion-wise target is a label id or a set of label ids in 1..255, got {!r}'.format(target))
    ids = list(target)
    if not ids:
        raise ValueError('a lesion-wise target must hold at least one label id')
    for l in ids:
        if isinstance(l, bool) or not isinstance(l, (int, float, np.integer, np.floating)) or int(l) != l \
                or not 1 <= int(l) <= 255:
            raise ValueError('lesion-wise target {!r}: label id {!r} is not an integer in 1..255'.format(target, l))
    return sorted(set(int(l) for l in ids))


def check_lesion_options(dilation_iters=3, min_lesion_voxels=1, hd95_penalty=374.0):
    """(dilation_iters, min_lesion_voxels, hd95_penalty) checked: 0..16, >= 1, finite and >= 0 (defaults: BraTS-GLI)"""
    for name, v in (('dilation_iters', dilation_iters), ('min_lesion_voxels', min_lesion_voxels)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError('{} must be an integer, got {!r}'.format(name, v))
    if not 0 <= dilation_iters <= 16:
        raise ValueError('dilation_iters must be in 0..16, got {}'.format(dilation_iters))
    if min_lesion_voxels < 1:
        raise ValueError('min_lesion_voxels must be at least 1, got {}'.format(min_lesion_voxels))
    try:
        penalty = float(hd95_penalty)
    except (TypeError, ValueError):
        raise ValueError('hd95_penalty must be a number, got {!r}'.format(hd95_penalty))
    if isinstance(hd95_penalty, bool) or not math.isfinite(penalty) or penalty < 0.0:
        raise ValueError('hd95_penalty must be finite and >= 0, got {!r}'.format(hd95_penalty))
    return int(dilation_iters), int(min_lesion_voxels), penalty


def lesionwise_from_table(gt_sizes, inter, pred_sizes, pairs, hd95_of, min_lesion_voxels=1, hd95_penalty=374.0):
    """The host half of the lesion-wise score, from exact integers, in doubles.

    :param gt_sizes: |G_i| for the lesions i = 1..Kg (gt_sizes[i - 1])
    :param inter: |G_i n B| likewise
    :param pred_sizes: |P_j| for the predicted components j = 1..Kp
    :param pairs: the (i, j) with P_j touching the dilated lesion D_i
    :param hd95_of: callable (i, matched ids) -> HD95 between G_i and the union U_i of its matched components
    A lesion without a match is a false negative (dice 0, hd95 = hd95_penalty); a lesion below min_lesion_voxels is
    dropped after matching (neither scored nor FN, its matches are no false positives); a component in no M_i is a
    false positive.  With n = kept + FP: lw_dice = sum dice / n, lw_hd95 = (sum hd95 + penalty * FP) / n (1 and 0 when
    n = 0), lesion_f1 = 2 TP / (2 TP + FN + FP) (1 when the denominator is 0).
    :return: {'lw_dice', 'lw_hd95', 'n_gt', 'n_tp', 'n_fn', 'n_fp', 'lesion_f1', 'lesions'}; 'lesions' lists
             (id, voxels, dice, hd95, matched ids) of every kept lesion"""
    _, min_lesion_voxels, hd95_penalty = check_lesion_options(0, min_lesion_voxels, hd95_penalty)
    gt_sizes, inter, pred_sizes = [int(v) for v in gt_sizes], [int(v) for v in inter], [int(v) for v in pred_sizes]
    if len(inter) != len(gt_sizes):
        raise ValueError('gt_sizes and inter differ in length: {} vs {}'.format(len(gt_sizes), len(inter)))
    matched = {}
    for i, j in pairs:
        i, j = int(i), int(j)
        if not (1 <= i <= len(gt_sizes) and 1 <= j <= len(pred_sizes)):
            raise ValueError('pair ({}, {}) outside 1..{} x 1..{}'.format(i, j, len(gt_sizes), len(pred_sizes)))
        matched.setdefault(i, set()).add(j)
    used, lesions = set(), []
    sum_dice = sum_hd95 = 0.0
    n_tp = n_fn = 0
    for i, voxels in enumerate(gt_sizes, 1):
        ids = tuple(sorted(matched.get(i, ())))
        used.update(ids)
        if voxels < min_lesion_voxels:
            continue
        if ids:
            union = sum(pred_sizes[j - 1] for j in ids)
            dice = 2.0 * inter[i - 1] / float(voxels + union)
            hd95 = float(hd95_of(i, ids))
            n_tp += 1
        else:
            dice, hd95 = 0.0, hd95_penalty
            n_fn += 1
        sum_dice += dice
        sum_hd95 += hd95
        lesions.append((i, voxels, dice, hd95, ids))
    n_fp = len(pred_sizes) - len(used)
    n = len(lesions) + n_fp
    f1_den = 2 * n_tp + n_fn + n_fp
    return {'lw_dice': sum_dice / n if n else 1.0,
            'lw_hd95': (sum_hd95 + hd95_penalty * n_fp) / n if n else 0.0,
            'n_gt': len(lesions), 'n_tp': n_tp, 'n_fn': n_fn, 'n_fp': n_fp,
            'lesion_f1': 2.0 * n_tp / f1_den if f1_den else 1.0,
            'lesions': lesions}


def _label_set(ids):
    bits = [0] * 8
    for l in ids:
        bits[l >> 5] |= 1 << (l & 31)
    return E.LabelSet((ctypes.c_uint * 8)(*bits))


def _set_mask(vol, ids):
    """launch: flat uint8 0/1 mask of the voxels of the device label volume whose value is in ids"""
    mask = torch.empty(vol.numel(), dtype=torch.uint8, device=vol.device)
    E.call('seg3d_label_set_mask', E.ptr(vol), _DTYPE_CODES[vol.dtype], vol.numel(), _label_set(ids), E.ptr(mask),
           E.stream_ptr())
    return mask


def _dilate18(mask, shape, iters):
    """launch: the flat mask dilated iters times by the 18-neighbourhood (iters = 0: the mask itself)"""
    if iters == 0:
        return mask
    Z, Y, X = shape
    out = torch.empty_like(mask)
    work = torch.empty_like(mask) if iters >= 2 else None
    E.call('seg3d_binary_dilate18', E.ptr(mask), E.ptr(out), E.ptr(work), X, Y, Z, iters, E.stream_ptr())
    return out


def _ccl26(mask, shape, capacity):
    """launch: (flat int32 id map, int32 (K, K > capacity), int32 sizes[capacity]) of the mask's 26-connected components"""
    Z, Y, X = shape
    n = mask.numel()
    words = E.query('seg3d_ccl26_label_workspace_ints', n)
    if words < 0:
        raise ValueError('volume of {} voxels is too large (limit 2^31 - 1)'.format(n))
    ids = torch.empty(n, dtype=torch.int32, device=mask.device)
    count = torch.empty(2, dtype=torch.int32, device=mask.device)
    sizes = torch.empty(capacity, dtype=torch.int32, device=mask.device) if capacity else None
    work = torch.empty(words, dtype=torch.int32, device=mask.device)
    E.call('seg3d_ccl26_label', E.ptr(mask), X, Y, Z, E.ptr(ids), E.ptr(count), E.ptr(sizes), capacity, E.ptr(work),
           E.stream_ptr())
    return ids, count, sizes


def _volume3d(vol, device):
    v = _as_device_labels(vol, _default_device(vol) if device is None else device)
    if v.dim() != 3:
        raise ValueError('expected one 3-D [z, y, x] grid, got shape {}'.format(tuple(v.shape)))
    E.require_device(v)
    return v


def lesion_components(vol, target, dilation_iters=0, device=None):
    """26-connected components of the voxels of `vol` whose label is in `target`, after dilation_iters dilations by the
    18-neighbourhood: (id map as a device int32 tensor [z, y, x], K, sizes).  Ids 1..K follow each component's lowest
    linear voxel index (z * Y + y) * X + x; sizes[k - 1] is the voxel count of component k (of the dilated mask)."""
    ids = check_target(target)
    iters = check_lesion_options(dilation_iters)[0]
    v = _volume3d(vol, device)
    shape = tuple(int(d) for d in v.shape)
    mask = _dilate18(_set_mask(v, ids), shape, iters)
    capacity = _CCL_CAPACITY
    while True:
        idmap, count, sizes = _ccl26(mask, shape, capacity)
        host = torch.cat([count, sizes]).tolist()
        if not host[1]:
            return idmap.view(shape), host[0], host[2:2 + host[0]]
        capacity = host[0]


def lesion_pair_table(dmap, a, pmap, kg, capacity=None, extra=()):
    """|G_i|, |G_i n B| for i = 1..kg and the sorted distinct (i, j) pairs with dmap = i > 0 and pmap = j > 0, from one
    pass over the three device arrays (seg3d_lesion_pairs).  The pair set is a device hash table of `capacity` words
    (a power of two; default 4 * kg, at least 1024); when it overflows the table is doubled and the launch repeated.
    `extra`: small device integer tensors read back in the same transfer.
    :return: (gsize list, inter list, pairs list, [extra as lists])"""
    if capacity is None:
        capacity = _MIN_PAIR_TABLE
        while capacity < 4 * kg:
            capacity *= 2
    if capacity < 1 or capacity & (capacity - 1):
        raise ValueError('pair table capacity must be a power of two, got {}'.format(capacity))
    dmap, pmap, a = dmap.reshape(-1), pmap.reshape(-1), a.reshape(-1)
    E.require_device(dmap, a, pmap)
    n = dmap.numel()
    while True:
        words = torch.zeros(2 * (kg + 1) + capacity, dtype=torch.int64, device=dmap.device)
        status = torch.zeros(1, dtype=torch.int32, device=dmap.device)
        gsize, inter, table = words[:kg + 1], words[kg + 1:2 * (kg + 1)], words[2 * (kg + 1):]
        E.call('seg3d_lesion_pairs', E.ptr(dmap), E.ptr(a), E.ptr(pmap), n, kg, E.ptr(gsize), E.ptr(inter), E.ptr(table),
               capacity, 1, E.ptr(status), E.stream_ptr())
        parts = [status.to(torch.int64), words] + [t.reshape(-1).to(torch.int64) for t in extra]
        host = torch.cat(parts).cpu().numpy()
        if not host[0]:
            break
        capacity *= 2
    body = host[1:1 + words.numel()]
    keys = np.sort(body[2 * (kg + 1):][body[2 * (kg + 1):] != 0])
    pairs = [(int(k >> 32), int(k & 0xffffffff)) for k in keys]
    extras, at = [], 1 + words.numel()
    for t in extra:
        extras.append(host[at:at + t.numel()].tolist())
        at += t.numel()
    return body[1:kg + 1].tolist(), body[kg + 2:2 * (kg + 1)].tolist(), pairs, extras


def cal_lesionwise(gt, seg, targets, spacing=None, dilation_iters=3, min_lesion_voxels=1, hd95_penalty=374.0):
    """Lesion-wise Dice / HD95 and lesion detection counts of every target (BraTS 2023 lesion-wise ranking rule).

    A target is a label id or a set of label ids in 1..255.  A = ground-truth voxels in the target, B = segmentation
    voxels in the target.  A is dilated dilation_iters times by the 18-neighbourhood; the 26-connected components D_i of
    the result are the lesions, G_i = A n D_i; P_j are the 26-connected components of B.  Component ids follow the lowest
    linear voxel index.  M_i = {j : P_j touches D_i}, U_i its union (a component may count in several lesions);
    dice_i = 2 |G_i n U_i| / (|G_i| + |U_i|) and hd95_i = HD95(G_i, U_i) as cal_surface_distances defines it, or 0 and
    hd95_penalty for an unmatched lesion.  Aggregation: lesionwise_from_table.

    :param gt, seg, spacing: as cal_surface_distances
    :return: one dict per target: 'lw_dice', 'lw_hd95', 'n_gt', 'n_tp', 'n_fn', 'n_fp', 'lesion_f1', 'lesions'
    Masks, dilation, labelling, pair table and the per-lesion masks and distances run on the device; the pair list, the
    counts and the sizes come back in one transfer per target, distance arrays never leave the device."""
    iters, min_lesion_voxels, hd95_penalty = check_lesion_options(dilation_iters, min_lesion_voxels, hd95_penalty)
    targets = [check_target(t) for t in targets]
    plan = _SurfacePlan(gt, seg, spacing)
    dev, n, shape = plan.g.device, plan.g.numel(), (plan.Z, plan.Y, plan.X)
    g_mask = torch.empty(n, dtype=torch.uint8, device=dev)
    u_mask = torch.empty(n, dtype=torch.uint8, device=dev)
    results = []
    for ids in targets:
        a, b = _set_mask(plan.g, ids), _set_mask(plan.s, ids)
        grown = _dilate18(a, shape, iters)
        capacity = _CCL_CAPACITY
        while True:
            dmap, dcount, _ = _ccl26(grown, shape, 0)
            pmap, pcount, psizes = _ccl26(b, shape, capacity)
            gsize, inter, pairs, (dc, pc, ps) = lesion_pair_table(dmap, a, pmap, capacity, extra=(dcount, pcount, psizes))
            kg, kp = dc[0], pc[0]
            if max(kg, kp) <= capacity:
                break
            capacity = max(kg, kp)

        def hd95_of(i, matched, dmap=dmap, a=a, pmap=pmap, kp=kp):
            flag = np.zeros(kp + 1, np.uint8)
            flag[list(matched)] = 1
            E.call('seg3d_lesion_select', E.ptr(dmap), E.ptr(a), E.ptr(pmap), E.ptr(torch.from_numpy(flag).to(dev)), kp,
                   i, n, E.ptr(g_mask), E.ptr(u_mask), E.stream_ptr())
            plan.mask_surfaces(g_mask, u_mask)
            return _plan_metrics(plan)['hd95']

        results.append(lesionwise_from_table(gsize[:kg], inter[:kg], ps[:kp], pairs, hd95_of, min_lesion_voxels,
                                             hd95_penalty))
    return results


def _counts_rows(counts):
    """[C, 3] confusion counts (device / host tensor, numpy array or nested list) -> list of (tp, fp, fn) Python ints"""
    if isinstance(counts, torch.Tensor):
        counts = counts.detach().cpu().tolist()
    elif isinstance(counts, np.ndarray):
        counts = counts.tolist()
    rows = [tuple(int(v) for v in row) for row in counts]
    if not rows or any(len(r) != 3 for r in rows):
        raise ValueError('confusion counts must be [C, 3] = (tp, fp, fn) per class')
    return rows


def dice_from_counts(counts):
    """per-class Dice 2 tp / (2 tp + fp + fn) from [C, 3] confusion counts (_ops.confusion_counts) as Python floats, in
    doubles on the host; a class that neither the labels nor the prediction contain (denominator 0) gives nan"""
    dice = []
    for tp, fp, fn in _counts_rows(counts):
        den = 2 * tp + fp + fn
        dice.append(float('nan') if den == 0 else (2.0 * tp) / float(den))
    return dice


def mean_foreground_dice(counts):
    """nan-mean of dice_from_counts over the foreground classes 1 .. C-1; nan when every foreground class is empty"""
    fg = [d for d in dice_from_counts(counts)[1:] if not math.isnan(d)]
    return sum(fg) / len(fg) if fg else float('nan')


def mean_region_dice(counts):
    """nan-mean of dice_from_counts over all R rows of [R, 3] region counts (_ops.region_confusion_counts): a region-based
    model has no background channel, so no row is excluded; nan when every region is empty"""
    rows = [d for d in dice_from_counts(counts) if not math.isnan(d)]
    return sum(rows) / len(rows) if rows else float('nan')
