"""Dice evaluation metric with the reference's name and return convention (utils/metrics.py:5-37 `cal_dsc`):
(dsc, seg_type) with seg_type in {'TN', 'FP', 'FN', 'TP'} decided by the voxel-count threshold; and the surface-distance
metrics HD / HD95 / ASSD (`cal_surface_distances`, which the reference does not have).

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


def _device_pair(gt, seg, device):
    if device is None:
        device = gt.device if isinstance(gt, torch.Tensor) and gt.is_cuda else torch.device('cuda', torch.cuda.current_device())
    g, s = _as_device_labels(gt, device), _as_device_labels(seg, device)
    if g.dtype != s.dtype:                      # compare in a common type, like numpy's == does
        common = torch.float32 if torch.float32 in (g.dtype, s.dtype) else torch.int32
        g, s = g.to(common), s.to(common)
    if g.numel() != s.numel():
        raise ValueError('ground truth and segmentation differ in size: {} vs {}'.format(tuple(g.shape), tuple(s.shape)))
    E.require_device(g, s)
    return g, s, device


def label_overlap_counts(gt, seg, labels, device=None):
    """[(area_gt, area_seg, intersection)] per label, as Python ints, from one device pass per 16 labels"""
    g, s, device = _device_pair(gt, seg, device)
    labels = [int(l) for l in labels]
    out = []
    for k0 in range(0, len(labels), MAX_LABELS_PER_PASS):
        chunk = labels[k0:k0 + MAX_LABELS_PER_PASS]
        counts = torch.zeros(3 * len(chunk), dtype=torch.int64, device=device)
        arr = (ctypes.c_int * len(chunk))(*chunk)
        E.call('seg3d_label_overlap_counts', E.ptr(g), E.ptr(s), _DTYPE_CODES[g.dtype], g.numel(), arr, len(chunk),
               E.ptr(counts), E.stream_ptr())
        c = counts.cpu().tolist()
        out.extend((c[3 * k], c[3 * k + 1], c[3 * k + 2]) for k in range(len(chunk)))
    return out


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
    g, s, device = _device_pair(gt, seg, device)
    out = []
    for k0 in range(0, len(regions), MAX_LABELS_PER_PASS):
        chunk = list(regions[k0:k0 + MAX_LABELS_PER_PASS])
        counts = torch.zeros(3 * len(chunk), dtype=torch.int64, device=device)
        lut = (ctypes.c_uint * 256)(*region_lut(chunk))
        E.call('seg3d_region_overlap_counts', E.ptr(g), E.ptr(s), _DTYPE_CODES[g.dtype], g.numel(), lut, len(chunk),
               E.ptr(counts), E.stream_ptr())
        c = counts.cpu().tolist()
        out.extend((c[3 * k], c[3 * k + 1], c[3 * k + 2]) for k in range(len(chunk)))
    return out


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
        if device is None:
            device = gt.device if isinstance(gt, torch.Tensor) and gt.is_cuda else torch.device(
                'cuda', torch.cuda.current_device())
        g, s = _as_device_labels(gt, device), _as_device_labels(seg, device)
        if g.dtype != s.dtype:
            common = torch.float32 if torch.float32 in (g.dtype, s.dtype) else torch.int32
            g, s = g.to(common), s.to(common)
        if g.dim() != 3 or g.shape != s.shape:
            raise ValueError('ground truth shape {} and segmentation shape {} must be one 3-D [z, y, x] grid'.format(
                tuple(g.shape), tuple(s.shape)))
        E.require_device(g, s)
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

    def surfaces(self, label):
        """launch: both surface masks of `label`, their common box and their voxel counts (box[6], box[7])"""
        self.box.copy_(self.box_init)
        for k, vol in enumerate((self.g, self.s)):
            E.call('seg3d_label_surface', E.ptr(vol), self.code, self.X, self.Y, self.Z, int(label), E.ptr(self.surf[k]),
                   E.ptr(self.box), E.ptr(self.box[6 + k:7 + k]), E.stream_ptr())

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


def cal_surface_distances(gt, seg, labels, spacing=None):
    """Surface-distance metrics of every label: [{'hd', 'hd95', 'assd'}] as Python floats, in physical units.

    For label l: A = (gt == l), B = (seg == l).  The surface dA is the set of voxels of A with at least one of their 6
    face neighbours outside A (voxels outside the volume count as outside A, so an object touching the border has a
    surface there).  d(p, dB) is the Euclidean distance from the centre of voxel p to the nearest centre of a dB voxel;
    only the spacing enters.  With D_AB = {d(p, dB) : p in dA} and D_BA = {d(q, dA) : q in dB}:
      HD   = max(max D_AB, max D_BA)
      HD95 = max(P95(D_AB), P95(D_BA)), P95 = numpy.percentile(., 95) with linear interpolation
      ASSD = (sum D_AB + sum D_BA) / (|D_AB| + |D_BA|), summed in fp64
    If A or B is empty, all three values are NaN.

    :param gt, seg: Image3d, numpy arrays or torch tensors, [z, y, x] on one grid
    :param labels: any number of labels
    :param spacing: (sx, sy, sz); default: the Image3d spacing (gt and seg must agree to a relative 1e-6), else 1, 1, 1
    The surfaces, the exact EDT (restricted to the box that encloses both surfaces) and the gather of the distances at
    the surface voxels run in csrc/surface.hip; HD95 takes two order statistics of the gathered distances on the device.
    """
    plan = _SurfacePlan(gt, seg, spacing)
    dev = plan.g.device
    results = []
    for label in labels:
        plan.surfaces(label)
        na, nb = plan.box[6:8].tolist()
        if na == 0 or nb == 0:
            results.append(dict(_NAN_SURFACE))
            continue
        picks, ranks = [plan.stats], []
        for direction, n in enumerate((na, nb)):
            dist2 = torch.empty(n, dtype=torch.float64, device=dev)
            plan.distances(direction, dist2)
            lo, hi, gamma = percentile_ranks(n)
            ranks.append(gamma)
            # order statistics of the squared distances are those of the distances (sqrt is monotone)
            picks.append(torch.stack([torch.kthvalue(dist2, lo + 1).values, torch.kthvalue(dist2, hi + 1).values]))
        v = torch.cat(picks).tolist()
        directed = []
        for direction in (0, 1):
            count, mx, total = v[3 * direction:3 * direction + 3]
            a, b = math.sqrt(v[6 + 2 * direction]), math.sqrt(v[7 + 2 * direction])
            directed.append((int(count), mx, total, percentile_from_order_stats(a, b, ranks[direction])))
        results.append(combine_directed(directed[0], directed[1]))
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
