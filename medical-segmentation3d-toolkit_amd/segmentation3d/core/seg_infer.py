"""Sliding-window whole-volume inference -- MI355X-native replacement of the patch path of the reference's
core/seg_infer.py (segmentation_voi :208-246, segmentation_volume :249-350, load_single_model :99-164,
load_models :167-205).

Reference behaviour: for every partition box, slice the ROI on the host, normalise it, run the net TWICE on a batch
of one, copy every class map back to the host and `+=` it into a SimpleITK volume through full-volume numpy round
trips (utils/image_tools.py:446-450); finally multiply by 1/count and arg-max.

Here the volume stays resident in HBM.  `SlidingWindowBatcher` crops + normalises P patches per launch
(seg3d_patch_gather_normalize_mc_flip; one modality is its M = 1 case), the net runs ONCE per patch (the reference's two
forwards are identical in eval mode, so their mean is the single result bit for bit), and the class maps are accumulated
on the device in list order (seg3d_patch_scatter_blend, no atomics => the same float summation order as the reference's
sequential loop).
gather -> net -> scatter is captured once into a hipGraph (torch.cuda.CUDAGraph drives hipStreamBeginCapture) and
replayed per batch; only a 4*(3P+7)-byte control block changes between replays.
"""
import importlib
import os
import threading
import time

import numpy as np
import torch

from segmentation3d import _engine as E
from segmentation3d import _ops
from segmentation3d.utils.image3d import Image3d
from segmentation3d.utils import image_tools
from segmentation3d.utils.image_tools import image_partition_by_fixed_size
from segmentation3d.loss.region_loss import check_region_class_order
from segmentation3d.utils.model_io import inference_state_dict, region_keys, select_checkpoint_folder
from segmentation3d.utils.normalizer import normalizer_from_dict


# ---------------------------------------------------------------------------------------------------------------------
# Gaussian patch blending and mirror test-time augmentation (not in the reference)
# ---------------------------------------------------------------------------------------------------------------------
BLEND_MODES = ('constant', 'gaussian')
_AXIS_BITS = {'x': 1, 'y': 2, 'z': 4}
_MIN_CORNER_WEIGHT = 1e-30


def check_blend_mode(blend):
    if blend not in BLEND_MODES:
        raise ValueError("unknown blend mode {!r}: 'constant' or 'gaussian'".format(blend))
    return blend


def check_mirror_axes(mirror_axes):
    """-> tuple of distinct axis letters in the given order; accepts a list / tuple of letters or a string such as 'xy'"""
    if mirror_axes is None:
        return ()
    out = []
    for a in mirror_axes:
        if not isinstance(a, str) or a not in _AXIS_BITS:
            raise ValueError("unknown mirror axis {!r}: 'x', 'y' or 'z'".format(a))
        if a not in out:
            out.append(a)
    return tuple(out)


def mirror_flip_masks(mirror_axes):
    """the flip set of mirror TTA: every subset of `mirror_axes` as a bit mask (bit 0 = x, 1 = y, 2 = z), ascending, 0 first"""
    bits = 0
    for a in check_mirror_axes(mirror_axes):
        bits |= _AXIS_BITS[a]
    return [m for m in range(8) if m & ~bits == 0]


def blend_weight_tables(box, sigma_scale=0.125):
    """the three 1-D float32 Gaussian tables (x, y, z) of a (bx, by, bz) box:
    g[i] = exp(-0.5 * ((i - (n - 1) / 2) / (sigma_scale * n))^2) in float64, rounded to float32.  Centred at (n - 1) / 2,
    so g[i] == g[n - 1 - i] exactly.  The weight of local voxel (lx, ly, lz) is (g_z[lz] * g_y[ly]) * g_x[lx].
    ValueError for a sigma_scale that is not positive and finite or whose smallest (corner) weight is below 1e-30: 1 / count
    must stay a finite normal float32."""
    s = float(sigma_scale)
    if not (np.isfinite(s) and s > 0.0):
        raise ValueError('sigma_scale must be positive and finite, got {!r}'.format(sigma_scale))
    tables = []
    for n in box:
        n = int(n)
        if n <= 0:
            raise ValueError('box {} must be positive'.format(tuple(box)))
        i = np.arange(n, dtype=np.float64)
        tables.append(np.exp(-0.5 * ((i - (n - 1) / 2.0) / (s * n)) ** 2).astype(np.float32))
    corner = float(tables[0].min()) * float(tables[1].min()) * float(tables[2].min())
    if not corner >= _MIN_CORNER_WEIGHT:
        raise ValueError('sigma_scale = {!r} gives a corner weight of {:.3g} on box {} (below 1e-30)'.format(
            sigma_scale, corner, tuple(int(b) for b in box)))
    return tuple(tables)


def blend_options(cfg):
    """(blend mode, sigma scale, mirror axes) of a stage section of infer_config.py.  The three keys are optional -- a
    config written by the reference has none of them -- and default to ('constant', 0.125, ())."""
    blend = check_blend_mode(getattr(cfg, 'blend_mode', None) or 'constant')
    sigma = getattr(cfg, 'blend_sigma_scale', None)
    sigma = 0.125 if sigma is None else float(sigma)
    axes = check_mirror_axes(getattr(cfg, 'tta_mirror_axes', None))
    return blend, sigma, axes


# ---------------------------------------------------------------------------------------------------------------------
# model ensembling (not in the reference)
# ---------------------------------------------------------------------------------------------------------------------
ENSEMBLE_MEMBER_KEYS = ('in_channels', 'out_channels', 'output_activation', 'region_class_order')


def ensemble_weights(weights, K):
    """-> K Python floats that sum to 1: the members' weights, normalised in double.  None = equal weights; K = 1 gives
    exactly 1.0.  ValueError for a wrong length or an entry that is not a positive finite number."""
    K = int(K)
    if K < 1:
        raise ValueError('an ensemble needs at least one member, got {}'.format(K))
    if weights is None:
        weights = [1.0] * K
    if isinstance(weights, (str, bytes)) or not hasattr(weights, '__len__'):
        raise ValueError('ensemble weights must be a list of {} numbers, got {!r}'.format(K, weights))
    if len(weights) != K:
        raise ValueError('{} ensemble weights for {} members'.format(len(weights), K))
    w = []
    for v in weights:
        if isinstance(v, (bool, str, bytes)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError('ensemble weight {!r} is not a number'.format(v))
        v = float(v)
        if not (np.isfinite(v) and v > 0.0):
            raise ValueError('ensemble weight {!r} is not positive and finite'.format(v))
        w.append(v)
    if K == 1:
        return [1.0]
    total = float(np.sum(np.asarray(w, dtype=np.float64)))
    if not np.isfinite(total):
        raise ValueError('ensemble weights {} do not have a finite sum'.format(w))
    return [v / total for v in w]


def check_ensemble_members(members):
    """the members of an ensemble are averaged plane by plane, so they must agree in in_channels, out_channels,
    output_activation and region_class_order (ValueError naming the key and the member); network type, spacing,
    max_stride, interpolation and normalisers may differ.  -> the list of members"""
    members = list(members)
    if not members:
        raise ValueError('an ensemble needs at least one member')

    def value(m, key):
        v = m.get(key)
        if key == 'output_activation':
            return v or 'softmax'
        if key == 'region_class_order':
            return None if v is None else [int(l) for l in v]
        return None if v is None else int(v)
    for key in ENSEMBLE_MEMBER_KEYS:
        want = value(members[0], key)
        for k, m in enumerate(members[1:], 1):
            if value(m, key) != want:
                raise ValueError('ensemble member {} has {} = {!r}, member 0 has {!r}'.format(k, key, value(m, key), want))
    return members


def ensemble_options(stage_cfg):
    """(names, weights, checkpoints) of a stage section of infer_config.py, from its optional keys
      ensemble = ['fold_0', 'fold_1', ...]   model folders under the model folder
      ensemble_weights = None                K positive numbers; None = equal
      checkpoint = 'latest'                  as for a single model, or a list of K
    names: the K folder names, weights: ensemble_weights(.., K), checkpoints: K selections.  Without the `ensemble` key (or
    with None) the stage is the single model `model_name`, as before: (None, None, None).  ValueError for an empty list, a
    non-list, duplicate or non-string names and for a `checkpoint` list whose length is not K (or one without `ensemble`)."""
    names = getattr(stage_cfg, 'ensemble', None)
    checkpoint = getattr(stage_cfg, 'checkpoint', 'latest')
    if names is None:
        if isinstance(checkpoint, (list, tuple)):
            raise ValueError('checkpoint = {!r} is a list but the stage has no ensemble'.format(checkpoint))
        if getattr(stage_cfg, 'ensemble_weights', None) is not None:
            raise ValueError('ensemble_weights without ensemble')
        return None, None, None
    if not isinstance(names, (list, tuple)):
        raise ValueError('ensemble must be a list of model folder names, got {!r}'.format(names))
    names = list(names)
    if not names:
        raise ValueError('ensemble is empty: list at least one model folder')
    for n in names:
        if not isinstance(n, str) or not n:
            raise ValueError('ensemble entry {!r} is not a model folder name'.format(n))
    if len(set(names)) != len(names):
        raise ValueError('ensemble lists a model twice: {}'.format(names))
    K = len(names)
    weights = ensemble_weights(getattr(stage_cfg, 'ensemble_weights', None), K)
    if isinstance(checkpoint, (list, tuple)):
        if len(checkpoint) != K:
            raise ValueError('{} checkpoint selections for {} ensemble members'.format(len(checkpoint), K))
        checkpoints = list(checkpoint)
    else:
        checkpoints = [checkpoint] * K
    return names, weights, checkpoints


class SlidingWindowBatcher(object):
    """device-side crop/normalise + accumulate for one resident volume.

    :param volume: float32 device tensor [Z, Y, X], or [Z, Y, X, M] for M co-registered modalities (channels-last)
    :param starts: list of [x, y, z] patch start voxels (all patches share `box`)
    :param box: (bx, by, bz) patch size in voxels
    :param num_classes: C
    :param normalizer: checkpoint-style dict {'type': 0|1, ...} or None (utils/normalizer.py:36-39,78-81); for a
           [Z, Y, X, M] volume a list of M of them, one per modality
    :param blend: 'constant' (every patch counts 1, the reference) or 'gaussian' (blend_weight_tables, uploaded once)
    :param sigma_scale: Gaussian sigma as a fraction of the box edge
    """

    def __init__(self, volume, starts, box, num_classes, normalizer, max_batch=16, blend='constant', sigma_scale=0.125):
        E.require_device(volume)
        if volume.dim() not in (3, 4) or volume.dtype != torch.float32:
            raise ValueError('volume must be a float32 [Z, Y, X] or [Z, Y, X, M] tensor')
        # a [Z, Y, X] volume is the same memory as [Z, Y, X, 1]: one modality is the M = 1 case, with a list of one normaliser
        single = volume.dim() == 3
        self.volume = (volume.unsqueeze(3) if single else volume).contiguous()
        self.Z, self.Y, self.X, self.M = (int(s) for s in self.volume.shape)
        self.box = tuple(int(b) for b in box)
        self.C = int(num_classes)
        self.starts = [[int(v) for v in s] for s in starts]
        bx, by, bz = self.box
        for s in self.starts:
            if s[0] < 0 or s[1] < 0 or s[2] < 0 or s[0] + bx > self.X or s[1] + by > self.Y or s[2] + bz > self.Z:
                raise ValueError('patch {} with box {} leaves the volume {}'.format(s, self.box, (self.X, self.Y, self.Z)))
        self.normalizer = normalizer
        self._norm_params = image_tools.normalizer_params([normalizer] if single else list(normalizer), self.M)
        dev = volume.device
        self.acc = torch.zeros((self.C, self.Z, self.Y, self.X), dtype=torch.float32, device=dev)
        self.count = torch.zeros((self.Z, self.Y, self.X), dtype=torch.float32, device=dev)
        self.max_batch = int(max_batch)
        nws = E.query('seg3d_patch_stats_mc_doubles', bx, by, bz, self.max_batch, self.M)
        self._stat_ws = torch.empty((nws,), dtype=torch.float64, device=dev)
        self._mean_std = torch.empty((self.max_batch, self.M, 2), dtype=torch.float32, device=dev)
        # control block on the device: [P][3] starts then {lo xyz, extent xyz, n_valid}
        self._ctl = torch.zeros((3 * self.max_batch + 7,), dtype=torch.int32, device=dev)
        self._plan = None
        self.blend = check_blend_mode(blend)
        self._wtab = None
        if self.blend == 'gaussian':
            self._wtab = torch.from_numpy(np.concatenate(blend_weight_tables(self.box, sigma_scale))).to(dev)

    # ---- control block ---------------------------------------------------------------------------------------------
    def _control_words(self, idx):
        P = self.max_batch
        if not 0 < len(idx) <= P:
            raise ValueError('batch of {} patches exceeds max_batch={}'.format(len(idx), P))
        bx, by, bz = self.box
        sel = np.array([self.starts[k] for k in idx], dtype=np.int32)
        lo = sel.min(0)
        hi = sel.max(0) + np.array([bx, by, bz], dtype=np.int32)
        host = np.zeros((3 * P + 7,), dtype=np.int32)
        host[:3 * len(idx)] = sel.reshape(-1)
        host[3 * len(idx):3 * P] = np.tile(sel[0], P - len(idx))  # padding patches: gathered, never scattered
        host[3 * P:3 * P + 3] = lo
        host[3 * P + 3:3 * P + 6] = hi - lo
        host[3 * P + 6] = len(idx)
        return host

    def set_batch(self, idx):
        """upload starts / bounding box / valid count of the patches `idx` (synchronous 4*(3P+7)-byte copy)"""
        self._ctl.copy_(torch.from_numpy(self._control_words(idx)))

    def plan(self, batches):
        """upload the control blocks of ALL batches in one copy; `select(b)` then switches batch with a stream-ordered
        device-to-device copy, so the host never has to wait for the GPU between batches"""
        words = np.stack([self._control_words(idx) for idx in batches])
        self._plan = torch.from_numpy(words).to(self._ctl.device)

    def select(self, b):
        self._ctl.copy_(self._plan[b], non_blocking=True)

    def _starts_ptr(self):
        return E.ptr(self._ctl)

    def _ctl_ptr(self):
        import ctypes
        return ctypes.c_void_p(self._ctl.data_ptr() + 4 * 3 * self.max_batch)

    # ---- kernels -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _flip_mask(flip):
        flip = int(flip)
        if not 0 <= flip <= 7:
            raise ValueError('flip mask {} outside 0..7'.format(flip))
        return flip

    def gather_current(self, out=None, flip=0):
        """crop + normalise the max_batch patches described by the control block -> [P, M, bz, by, bx] view of NDHWC
        memory (for one modality that is a contiguous [P, 1, bz, by, bx] tensor).  flip: mirror mask (bit 0 = x, 1 = y,
        2 = z; 0 = the plain gather); the result equals torch.flip of the plain gather along those axes, bit for bit"""
        flip = self._flip_mask(flip)
        bx, by, bz = self.box
        P = self.max_batch
        if out is None:
            out = torch.empty((P, bz, by, bx, self.M), dtype=torch.float32,
                              device=self.volume.device).permute(0, 4, 1, 2, 3)
        elif tuple(out.shape) != (P, self.M, bz, by, bx) or not out.permute(0, 2, 3, 4, 1).is_contiguous():
            raise ValueError('out must be the [P, M, bz, by, bx] view of a contiguous [P, bz, by, bx, M] batch')
        E.call('seg3d_patch_gather_normalize_mc_flip', E.ptr(self.volume), self._starts_ptr(), E.ptr(out),
               E.ptr(self._stat_ws), E.ptr(self._mean_std), self.Z, self.Y, self.X, bx, by, bz, P, self.M,
               self._norm_params, flip, E.stream_ptr())
        return out

    def scatter_current(self, probs, flip=0):
        """accumulate probs [P, C, bz, by, bx] of the control block's valid patches into acc / count, each voxel with the
        batcher's blend weight.  flip: the probabilities are stored mirrored by that mask (the net saw gather_current(flip=
        flip)) and are accumulated un-mirrored"""
        flip = self._flip_mask(flip)
        bx, by, bz = self.box
        P = self.max_batch
        if tuple(probs.shape) != (P, self.C, bz, by, bx) or not probs.is_contiguous():
            raise ValueError('probs must be contiguous [{}, {}, {}, {}, {}], got {}'.format(P, self.C, bz, by, bx,
                                                                                            tuple(probs.shape)))
        max_box = min(self.X * self.Y * self.Z, min(self.X, bx * P) * min(self.Y, by * P) * min(self.Z, bz * P))
        E.call('seg3d_patch_scatter_blend', E.ptr(probs), self._starts_ptr(), self._ctl_ptr(), E.ptr(self._wtab),
               E.ptr(self.acc), E.ptr(self.count), self.Z, self.Y, self.X, bx, by, bz, self.C, flip, max_box,
               E.stream_ptr())

    # convenience (eager) forms used by tests and the non-graph path
    def gather(self, idx, flip=0):
        self.set_batch(idx)
        return self.gather_current(flip=flip)[:len(idx)]

    def scatter(self, idx, probs, flip=0):
        self.set_batch(idx)
        P = self.max_batch
        if probs.shape[0] != P:
            pad = torch.zeros((P - probs.shape[0],) + tuple(probs.shape[1:]), dtype=probs.dtype, device=probs.device)
            probs = torch.cat((probs, pad), 0)
        self.scatter_current(probs.contiguous(), flip=flip)

    def finalize(self, z_range=None, regions_order=None):
        """acc *= 1/count (in place) and arg-max -> (probs [C,Z,Y,X], mask int8 [Z,Y,X]).
        z_range = (z0, z1): only that slab of planes (a rank of the sharded sliding window finalizes the slab it owns);
        the mask is zero outside it.
        regions_order (C labels in 1..127, region-based models): the C planes are region probabilities and the mask is
        composed by the sequential overwrite rule instead -- 0, then for r = 0 .. C-1 in order p_r > 0.5 writes
        regions_order[r] (seg3d_finalize_regions)"""
        import ctypes
        if regions_order is not None:
            regions_order = check_region_class_order(regions_order, self.C)
        plane = self.Y * self.X
        if z_range is None:
            mask = torch.empty((self.Z, self.Y, self.X), dtype=torch.int8, device=self.volume.device)
            z0, z1 = 0, self.Z
        else:
            mask = torch.zeros((self.Z, self.Y, self.X), dtype=torch.int8, device=self.volume.device)
            z0, z1 = int(z_range[0]), int(z_range[1])
            if not 0 <= z0 <= z1 <= self.Z:
                raise ValueError('z range {} outside the volume'.format(z_range))
        if z1 > z0 and regions_order is not None:
            E.call('seg3d_finalize_regions', ctypes.c_void_p(self.acc.data_ptr() + 4 * z0 * plane),
                   ctypes.c_void_p(self.count.data_ptr() + 4 * z0 * plane), ctypes.c_void_p(mask.data_ptr() + z0 * plane),
                   self.C, (ctypes.c_int * self.C)(*regions_order), (z1 - z0) * plane, self.Z * plane, E.stream_ptr())
        elif z1 > z0:
            E.call('seg3d_finalize_argmax', ctypes.c_void_p(self.acc.data_ptr() + 4 * z0 * plane),
                   ctypes.c_void_p(self.count.data_ptr() + 4 * z0 * plane), ctypes.c_void_p(mask.data_ptr() + z0 * plane),
                   self.C, (z1 - z0) * plane, self.Z * plane, E.stream_ptr())
        return self.acc, mask


def shard_batches(batches, rank, world_size):
    """round-robin deal of patch batches (kept for callers that merge with a full all-reduce; the sliding window itself
    uses SlabShardPlan below)"""
    return [b for i, b in enumerate(batches) if i % world_size == rank]


class SlabShardPlan(object):
    """Patch inference over several GPUs: patches are independent, so the patch list is cut into `world`
    chunks that are CONTIGUOUS IN Z (sorted by z start, ties in list order; equal patch counts).  Rank r then only ever
    touches the planes [touch_lo[r], touch_hi[r]) of its accumulators, and the volume is cut into disjoint OWNED slabs
    [bounds[r], bounds[r + 1]) with bounds[r] = the smallest z start of rank r.  A lower rank's patches reach at most
    box_z - stride_z planes into the slabs above it, so the merge moves only those halo planes (rank q -> owner r,
    q < r) instead of all-reducing (C + 1) full volumes; every rank finalizes (divide + arg-max) its own slab.
    Pure host index arithmetic: the same plan is computed by every rank."""

    def __init__(self, starts, box, volume_zyx, world_size):
        self.world = int(world_size)
        self.Z = int(volume_zyx[0])
        bz = int(box[2])
        n = len(starts)
        order = sorted(range(n), key=lambda k: (int(starts[k][2]), k))
        cuts = [(n * r) // self.world for r in range(self.world + 1)]
        self.patches = [sorted(order[cuts[r]:cuts[r + 1]]) for r in range(self.world)]   # list order within a rank
        self.touch_lo, self.touch_hi, self.bounds = [], [], []
        prev = 0
        for r in range(self.world):
            zs = [int(starts[k][2]) for k in self.patches[r]]
            lo = min(zs) if zs else prev
            hi = max(zs) + bz if zs else prev
            self.touch_lo.append(lo)
            self.touch_hi.append(hi)
            self.bounds.append(0 if r == 0 else max(lo, prev))
            prev = self.bounds[-1]
        self.bounds.append(self.Z)

    def owned(self, rank):
        return self.bounds[rank], self.bounds[rank + 1]

    def transfers(self):
        """[(src rank, dst rank, z0, z1)]: planes of src's accumulators that belong to dst's slab, in a fixed global order"""
        out = []
        for r in range(self.world):
            o0, o1 = self.owned(r)
            for q in range(self.world):
                if q == r or not self.patches[q]:
                    continue
                z0, z1 = max(o0, self.touch_lo[q]), min(o1, self.touch_hi[q])
                if z1 > z0:
                    out.append((q, r, z0, z1))
        return out


def _stage_on_host(t, group):
    """gloo (the CPU rehearsal backend; also used when several test ranks share one GPU) moves host memory only: device
    buffers are staged through the host there.  RCCL ("nccl") takes device pointers directly."""
    import torch.distributed as dist
    return t.is_cuda and dist.get_backend(group) == 'gloo'


def merge_slabs(acc, count, plan, rank, group=None):
    """exchange the halo planes of a SlabShardPlan: afterwards acc [C,Z,Y,X] / count [Z,Y,X] of rank r are complete
    inside plan.owned(r) (point-to-point sends over RCCL / xGMI; nothing is exchanged for planes only one rank touched).
    The owner adds the incoming partial sums in ascending source-rank order (fixed => reproducible)."""
    import torch.distributed as dist
    C = acc.shape[0]
    stage = _stage_on_host(acc, group)
    ops, recvs, keep = [], [], []
    for q, r, z0, z1 in plan.transfers():
        if rank == q:
            buf = torch.cat((acc[:, z0:z1], count[z0:z1].unsqueeze(0)), 0).contiguous()
            if stage:
                buf = buf.cpu()
            keep.append(buf)
            peer = r if group is None else dist.get_global_rank(group, r)
            ops.append(dist.P2POp(dist.isend, buf, peer, group))
        elif rank == r:
            buf = torch.empty((C + 1, z1 - z0) + tuple(acc.shape[2:]), dtype=acc.dtype,
                              device='cpu' if stage else acc.device)
            peer = q if group is None else dist.get_global_rank(group, q)
            ops.append(dist.P2POp(dist.irecv, buf, peer, group))
            recvs.append((z0, z1, buf))
    if ops:
        for w in dist.batch_isend_irecv(ops):
            w.wait()
    for z0, z1, buf in recvs:
        buf = buf.to(acc.device)
        acc[:, z0:z1] += buf[:C]
        count[z0:z1] += buf[C]


def gather_slabs(probs, mask, plan, group=None, with_probs=True):
    """replicate the finalized slabs on every rank: each owner broadcasts its slab of every class map (contiguous planes,
    no staging) and of the mask -- the output's own size, once"""
    import torch.distributed as dist
    stage = _stage_on_host(mask, group)

    def bcast(view, src):
        if not stage:
            dist.broadcast(view, src=src, group=group)
            return
        host = view.cpu()
        dist.broadcast(host, src=src, group=group)
        view.copy_(host)
    for r in range(plan.world):
        z0, z1 = plan.owned(r)
        if z1 <= z0:
            continue
        src = r if group is None else dist.get_global_rank(group, r)
        bcast(mask[z0:z1], src)
        if with_probs:
            for c in range(probs.shape[0]):
                bcast(probs[c, z0:z1], src)


def _forward_two_streams(net, batch, side):
    """forward of one patch batch as two half batches on two HIP streams: while one half runs an MFMA-bound conv, the
    other half's HBM-bound GroupNorm / stride-2 / head kernels share the chip (patches are independent; GroupNorm(1, C)
    is per sample, so the result is identical).  Works eagerly and under hipGraph capture (fork / join by events)."""
    P = batch.shape[0]
    if side is None or P < 2:
        return net(batch).contiguous()
    h = P // 2
    cur = torch.cuda.current_stream()
    side.wait_stream(cur)
    with _ops.two_forwards():
        with torch.cuda.stream(side):
            out_b = net(batch[h:])
        out_a = net(batch[:h])
    cur.wait_stream(side)
    out_b.record_stream(cur)
    return torch.cat([out_a, out_b], 0)


def sliding_window_inference(net, volume, starts, box, num_classes, normalizer, batch_size=8, use_graph=True,
                             process_group=None, shard=False, two_streams=True, gather='all', blend='constant',
                             sigma_scale=0.125, mirror_axes=(), regions_order=None):
    """run `net` over all patches of a device-resident volume; returns (probs [C,Z,Y,X], mask int8 [Z,Y,X], batcher).
    blend = 'gaussian' weights every patch voxel with blend_weight_tables(box, sigma_scale); mirror_axes (a subset of
    'x', 'y', 'z') adds mirror test-time augmentation: every batch is gathered, predicted and accumulated once per mask of
    mirror_flip_masks(mirror_axes), and the result is the weighted mean over patches and flips.  The flip sequence of a
    batch is part of the captured graph: one replay per batch whatever the number of flips.
    With shard=True under an initialised torch.distributed group the patch list is cut into z-contiguous chunks, one per
    rank (SlabShardPlan); after the patch loop only the halo planes are exchanged (merge_slabs), every rank divides and
    arg-maxes the slab it owns, and the slabs are replicated (gather='all': probabilities and mask, 'mask': mask only,
    'none': each rank keeps just its slab; batcher.shard_plan tells which).  Float summation order inside a halo then
    differs from the sequential reference loop by rounding only.
    regions_order (num_classes labels in 1..127): `net` is a region-based (sigmoid) network; the accumulated planes are
    region probabilities and the mask is composed from them by SlidingWindowBatcher.finalize's overwrite rule.  Nothing
    else changes: gather, scatter, blending, mirror TTA and the slab merge are sums of num_classes planes either way."""
    with torch.cuda.device(volume.device):
        return _sliding_window_inference(net, volume, starts, box, num_classes, normalizer, batch_size, use_graph,
                                         process_group, shard, two_streams, gather, blend, sigma_scale, mirror_axes,
                                         regions_order)


# hipGraph capture for the per-volume graphs.  `with torch.cuda.graph(g)` empties the caching allocator before every capture
# and gives every graph a private pool that is handed back to the driver when the graph dies: one volume = ~50 hipMalloc +
# ~50 hipFree calls (measured: torch.cuda.memory_stats num_device_alloc / num_device_free grow by 51-54 per job), which
# cost 30-60 ms on a healthy box and far more on a box where the driver is slow at it (whole jobs read 1.4-1.8 s instead
# of 0.96 s; with 50 patches per replay the calls alone made every job after the first take 2.8 s).  All volume graphs of a
# device therefore capture into ONE pool that a tiny keep-alive graph holds for the life of the process: the segments a
# dead graph leaves behind are reused by the next capture, and nothing is emptied.
# The caching allocator keeps free blocks per (pool, stream): the warm-up stream, the capture stream and the second forward
# stream are therefore created once per device as well -- with fresh streams per volume no block was ever reused (reserved
# memory grew by 20 GB per job).
# Retained footprint: the pool keeps every segment a volume graph of this device ever needed (the peak intermediates of the
# largest box / batch seen, ~20 GB for 16 patches of 96^3) reserved until release_graph_pool(device) is called --
# torch.cuda.empty_cache() cannot return memory of a live graph pool.
_GRAPH_POOLS = {}
_JOB_STREAMS = {}
_GRAPH_POOL_LOCK = threading.Lock()


def _job_stream(device, which):
    key = (device.index if device.index is not None else torch.cuda.current_device(), which)
    st = _JOB_STREAMS.get(key)
    if st is None:
        st = _JOB_STREAMS[key] = torch.cuda.Stream(device=device)
    return st


def _capture_in_shared_pool(fn, device):
    """capture fn() into a CUDAGraph whose memory comes from the device's shared volume-graph pool.  Graphs that share a pool
    must not be alive at the same time unless they replay in capture order (the pool hands a dead temporary's block to the
    next capture): the shared pool therefore serves ONE live volume graph per device; a second concurrent job (another
    thread, a nested call) captures into a private pool of its own, as torch.cuda.graph would."""
    import weakref
    key = device.index if device.index is not None else torch.cuda.current_device()
    cur = torch.cuda.current_stream()
    # the check of `live`, the claim of the shared pool and the creation of the pool itself are one critical section: two
    # threads that both saw live == 0 would capture into the same pool while both graphs are alive
    with _GRAPH_POOL_LOCK:
        entry = _GRAPH_POOLS.get(key)
        if entry is None:
            stream = _job_stream(device, 'capture')
            pool = torch.cuda.graph_pool_handle()
            keep = torch.cuda.CUDAGraph()
            anchor = torch.zeros(1, device=device)
            stream.wait_stream(cur)
            with torch.cuda.stream(stream):
                keep.capture_begin(pool=pool)
                anchor.add_(1.0)
                keep.capture_end()
            cur.wait_stream(stream)
            entry = _GRAPH_POOLS[key] = {'pool': pool, 'keep': keep, 'anchor': anchor, 'live': 0}
        shared = entry['live'] == 0
        if shared:
            entry['live'] += 1
    stream = _job_stream(device, 'capture') if shared else torch.cuda.Stream(device=device)
    graph = torch.cuda.CUDAGraph()
    try:
        stream.wait_stream(cur)
        with torch.cuda.stream(stream):
            graph.capture_begin(pool=entry['pool'] if shared else torch.cuda.graph_pool_handle())
            try:
                fn()
            finally:
                graph.capture_end()
        cur.wait_stream(stream)
    except BaseException:
        if shared:
            with _GRAPH_POOL_LOCK:
                entry['live'] -= 1
        raise
    if shared:
        def _released(e=entry):
            with _GRAPH_POOL_LOCK:
                e['live'] -= 1
        weakref.finalize(graph, _released)
    return graph


def release_graph_pool(device=None):
    """hand the shared volume-graph pool of `device` (default: the current one) back to the caching allocator -- for a process
    that ran inference and now wants the memory for training, or shares the GPU.  Refuses (returns False) while a volume
    graph of that device is alive; the next sliding-window job simply builds a new pool."""
    if device is None:
        key = torch.cuda.current_device()
    else:
        device = torch.device(device)
        key = device.index if device.index is not None else torch.cuda.current_device()
    with _GRAPH_POOL_LOCK:
        entry = _GRAPH_POOLS.get(key)
        if entry is None:
            return True
        if entry['live'] != 0:
            return False
        del _GRAPH_POOLS[key]
    entry.clear()                 # drops the keep-alive graph: the pool's segments become ordinary cached blocks
    torch.cuda.synchronize(key)
    torch.cuda.empty_cache()
    return True


def _sliding_window_inference(net, volume, starts, box, num_classes, normalizer, batch_size, use_graph, process_group,
                              shard, two_streams, gather, blend='constant', sigma_scale=0.125, mirror_axes=(),
                              regions_order=None):
    if gather not in ('all', 'mask', 'none'):
        raise ValueError("gather must be 'all', 'mask' or 'none'")
    if regions_order is not None:
        regions_order = check_region_class_order(regions_order, int(num_classes))
    flips = mirror_flip_masks(mirror_axes)
    batcher = SlidingWindowBatcher(volume, starts, box, num_classes, normalizer, max_batch=batch_size, blend=blend,
                                   sigma_scale=sigma_scale)
    P = batcher.max_batch
    sharded = shard and torch.distributed.is_available() and torch.distributed.is_initialized() and \
        torch.distributed.get_world_size(process_group) > 1
    plan, rank = None, 0
    if sharded:
        rank = torch.distributed.get_rank(process_group)
        plan = SlabShardPlan(batcher.starts, batcher.box, (batcher.Z, batcher.Y, batcher.X),
                             torch.distributed.get_world_size(process_group))
        mine = plan.patches[rank]
    else:
        mine = list(range(len(starts)))
    batcher.shard_plan = plan
    batches = [mine[i:i + P] for i in range(0, len(mine), P)]
    if batches:
        batcher.plan(batches)
    graph, first = None, 0
    # the weights do not change during a volume: keep their packed (MFMA-layout) images across batches, so neither
    # the eager batches nor the captured graph re-pack 26 tensors per forward
    cache_was_on = _ops.weight_cache(True)
    side = _job_stream(volume.device, 'side') if (two_streams and P >= 2) else None

    def run_batch(buf=None):
        """the current batch once per flip, in flip-set order: mirrored gather -> net -> un-mirroring scatter; returns the
        gather buffer (reused by every flip, and by every replay when captured)"""
        for f in flips:
            buf = batcher.gather_current(out=buf, flip=f)
            batcher.scatter_current(_forward_two_streams(net, buf, side), flip=f)
        return buf
    try:
        with torch.no_grad():
            if use_graph and len(batches) > 2:
                # warm-up on a side stream (allocator, lazy code-object loading, packed weights), then capture
                # gather -> net -> scatter once.  The warm-up batch is accumulated for real: it simply is the first
                # batch of the job.
                stream = _job_stream(volume.device, 'warmup')
                stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(stream):
                    batcher.select(0)
                    static_in = run_batch()
                torch.cuda.current_stream().wait_stream(stream)
                first = 1
                # capture with n_valid = 0 in the control block so the captured launch itself accumulates nothing
                batcher._ctl.zero_()
                torch.cuda.synchronize()
                graph = _capture_in_shared_pool(lambda: run_batch(static_in), volume.device)
            for b in range(first, len(batches)):
                batcher.select(b)
                if graph is not None:
                    graph.replay()
                else:
                    run_batch()
            if sharded:
                merge_slabs(batcher.acc, batcher.count, plan, rank, process_group)
                probs, mask = batcher.finalize(plan.owned(rank), regions_order=regions_order)
                if gather != 'none':
                    gather_slabs(probs, mask, plan, process_group, with_probs=(gather == 'all'))
            else:
                probs, mask = batcher.finalize(regions_order=regions_order)
    finally:
        if not cache_was_on:
            torch.cuda.synchronize()   # the images were allocated on the warm-up stream: nothing may still read them
            _ops.weight_cache(False)
    return probs, mask, batcher


# ---------------------------------------------------------------------------------------------------------------------
# reference-shaped API
# ---------------------------------------------------------------------------------------------------------------------
class _Model(dict):
    """attribute dict (the reference uses easydict here, core/seg_infer.py:107)"""
    __getattr__ = dict.get
    __setattr__ = dict.__setitem__


def load_single_model(model_folder, gpu_id=0, checkpoint='latest'):
    """load one model folder `<folder>/checkpoints/chk_<latest>/params.pth` (reference: seg_infer.py:99-164); `checkpoint`
    = 'best' loads `checkpoints/best` (written by a training run with validation), an integer that epoch's `chk_<n>`.
    gpu_id must be >= 0: this engine has no CPU path (the reference's gpu_id = -1 branch is served by stock torch)."""
    assert os.path.isdir(model_folder), 'Model folder does not exist: {}'.format(model_folder)
    if gpu_id is None or int(gpu_id) < 0:
        raise E.Seg3dEngineError('segmentation3d HIP engine needs gpu_id >= 0 (no CPU inference path)')
    device = torch.device('cuda:{}'.format(int(gpu_id)))
    # the reference pins the GPU with CUDA_VISIBLE_DEVICES (seg_infer.py:104-105); here the chosen device becomes the
    # CURRENT device: every kernel of this engine is launched on the current device's stream
    torch.cuda.set_device(device)
    chk_dir = select_checkpoint_folder(os.path.join(model_folder, 'checkpoints'), checkpoint)
    state = torch.load(os.path.join(chk_dir, 'params.pth'), map_location='cpu', weights_only=True)
    net_module = importlib.import_module('segmentation3d.network.' + state['net'])
    # region-based checkpoints carry their regions and the head's activation; one without
    # the keys is an exclusive-class (soft-max) model
    regions, region_class_order, activation = region_keys(state)
    if activation == 'sigmoid':
        if region_class_order is None:
            raise ValueError('region-based checkpoint {} has no region_class_order'.format(chk_dir))
        region_class_order = check_region_class_order(region_class_order, int(state['out_channels']))
        net = net_module.SegmentationNet(state['in_channels'], state['out_channels'], output_activation='sigmoid')
    else:
        net = net_module.SegmentationNet(state['in_channels'], state['out_channels'])
    net.load_state_dict(inference_state_dict(state['state_dict']))   # (the auxiliary heads of a deeply supervised run stay behind)
    net.eval()
    net = net.to(device)
    model = _Model()
    model.net = net
    model.device = device
    model.spacing, model.max_stride, model.interpolation = state['spacing'], state['max_stride'], state['interpolation']
    model.in_channels, model.out_channels = state['in_channels'], state['out_channels']
    model.output_activation, model.regions = activation, regions
    model.region_class_order = region_class_order if activation == 'sigmoid' else None
    model.crop_normalizers = [None if d is None else normalizer_from_dict(d) for d in state['crop_normalizers']]
    model.crop_normalizer_dicts = list(state['crop_normalizers'])
    return model


def load_models(model_folder, gpu_id=0):
    """load `infer_config.py` plus the coarse / fine models it names (reference: seg_infer.py:167-205)"""
    from segmentation3d.utils.file_io import load_config
    assert os.path.isdir(model_folder), 'Model folder does not exist: {}'.format(model_folder)
    infer_cfg = load_config(os.path.join(model_folder, 'infer_config.py'))
    models = _Model()
    models.infer_cfg = infer_cfg
    scale = infer_cfg.general.single_scale
    if scale not in ('coarse', 'fine', 'DISABLE'):
        raise ValueError('Unsupported single scale type!')
    models.coarse_model = models.fine_model = None
    for stage in ('coarse', 'fine'):
        if scale not in (stage, 'DISABLE'):
            continue
        stage_cfg = getattr(infer_cfg, stage)
        names, weights, checkpoints = ensemble_options(stage_cfg)
        if names is None:       # a single model is the ensemble of one member with weight 1.0
            names, weights, checkpoints = [stage_cfg.model_name], [1.0], [getattr(stage_cfg, 'checkpoint', 'latest')]
        # every member is a model folder of its own; <stage>_model stays member 0 for callers that read it
        members = check_ensemble_members([load_single_model(os.path.join(model_folder, n), gpu_id, c)
                                          for n, c in zip(names, checkpoints)])
        models[stage + '_model'] = members[0]
        models[stage + '_members'] = members
        models[stage + '_weights'] = weights
    return models


def _segment_stage(models, stage, image, bbox_start_voxel, bbox_end_voxel, tta):
    """one stage of segmentation(): its members (one for a stage without an `ensemble` key) with their weights"""
    return segmentation_volume_ensemble(models[stage + '_members'], getattr(models['infer_cfg'], stage), image,
                                        bbox_start_voxel, bbox_end_voxel, weights=models[stage + '_weights'], **tta)


def _case_images(model, image, case=None):
    """an Image3d, or a list of M co-registered Image3d -> (list of images, M); checks the frames and that the model
    takes M input channels (ValueError naming the case)"""
    images = list(image) if isinstance(image, (list, tuple)) else [image]
    if not images or not all(isinstance(im, Image3d) for im in images):
        raise ValueError('image must be an Image3d or a non-empty list of Image3d')
    case = case if case is not None else 'with {} modalities'.format(len(images))
    from segmentation3d.utils.image_io import check_modalities
    check_modalities(images, case)
    in_channels = model.get('in_channels') if hasattr(model, 'get') else None
    if in_channels is not None and int(in_channels) != len(images):
        raise ValueError('case {}: {} modalities but the model takes in_channels = {}'.format(case, len(images),
                                                                                             in_channels))
    return images, len(images)


def _model_normalizers(model, M):
    dicts = list(model['crop_normalizer_dicts'] or [])
    if M == 1:                  # the reference applies crop_normalizers[0] (core/seg_infer.py:221-224); none = no normalisation
        return dicts[:1] or [None]
    if len(dicts) != M:
        raise ValueError('model has {} crop normalizers for {} modalities'.format(len(dicts), M))
    return dicts


def segmentation_voi(model, iso_image, start_voxel, end_voxel, use_gpu=True):
    """segment one volume of interest (reference: seg_infer.py:208-246); returns the list of per-class Image3d maps.
    iso_image: an Image3d or a list of M co-registered Image3d (one per modality).
    Kept for API parity; whole volumes should go through segmentation_volume, which batches patches on the device."""
    images, M = _case_images(model, iso_image)
    iso_image = images[0]
    with torch.cuda.device(model['device']):
        vol = image_tools.images_to_device(images, model['device'])
        norm = image_tools.resolve_normalizers(_model_normalizers(model, M), vol)
    box = [int(end_voxel[d] - start_voxel[d]) for d in range(3)]
    probs, _, _ = sliding_window_inference(model['net'], vol, [list(start_voxel)], box, model['out_channels'], norm,
                                           batch_size=1, use_graph=False)
    z0, y0, x0 = start_voxel[2], start_voxel[1], start_voxel[0]
    maps = []
    for c in range(model['out_channels']):
        roi = probs[c, z0:z0 + box[2], y0:y0 + box[1], x0:x0 + box[0]].cpu().numpy()
        maps.append(Image3d(roi, iso_image.GetSpacing(), iso_image.GetOrigin(), iso_image.GetDirection()))
    return maps


def _physical_to_index(frame, point):
    """sitk TransformPhysicalPointToIndex: nearest index (round half up per axis)"""
    spacing, origin, direction = (np.asarray(v, dtype=np.float64) for v in frame)
    c = np.diag(1.0 / spacing) @ np.linalg.inv(direction.reshape(3, 3)) @ (np.asarray(point, dtype=np.float64) - origin)
    return [int(np.floor(v + 0.5)) for v in c]


def _index_to_physical(frame, index):
    spacing, origin, direction = (np.asarray(v, dtype=np.float64) for v in frame)
    return origin + direction.reshape(3, 3) @ (spacing * np.asarray(index, dtype=np.float64))


def segmentation_volume(model, cfg, image, bbox_start_voxel, bbox_end_voxel, use_gpu=True, batch_size=8, blend=None,
                        mirror_axes=None):
    """segment a whole volume (reference: seg_infer.py:249-350), everything between the upload of the image and the
    download of the probability maps / mask on the device:
      resample to the model spacing, size up to a multiple of max_stride (image_tools.py:348-377)  -> seg3d_resample_affine_mc
      partition (host index arithmetic), one batched gather -> net -> scatter per hipGraph replay, divide by overlap
      the class probabilities back onto the image grid, padding 1.0 for class 0 and 0.0 otherwise (:330-333), and the
      arg-max -> int8 mask (:336-339) in one launch -> seg3d_ensemble_accumulate (a single model is the K = 1, weight 1.0
      case of segmentation_volume_ensemble; that launch takes 1..16 planes, so a model with more out_channels whose grid is
      not the image grid raises ValueError); largest component / small-component removal (:342-348)
    `use_gpu` is kept for signature compatibility (the reference shrinks spacing / partitions on the CPU path only).
    image: an Image3d, or a list of M co-registered Image3d (one per modality; the model must take in_channels = M):
    the M modalities are resampled to the model grid in one launch (seg3d_resample_affine_mc) and every patch is
    normalised with its modality's normaliser (seg3d_patch_gather_normalize_mc).
    Patch blending and mirror TTA come from the optional stage keys cfg.blend_mode ('constant' | 'gaussian'),
    cfg.blend_sigma_scale and cfg.tta_mirror_axes (blend_options: defaults 'constant', 0.125, []); `blend` / `mirror_axes`,
    when not None, override the config.
    Returns (mean_probs: list of Image3d, mask: Image3d int8).
    """
    images, _ = _case_images(model, image)
    return _image_grid_result([model], [1.0], cfg, images, bbox_start_voxel, bbox_end_voxel, batch_size, blend, mirror_axes)


def _member_probabilities(model, cfg, images, bbox_start_voxel, bbox_end_voxel, batch_size, blend, sigma_scale, mirror_axes,
                          src=None):
    """the front half of a volume job, once per member (a single model is the ensemble of one): resample the
    image to the model's grid, partition (the bounding box mapped into that grid), run the sliding window.
    src: the resident [Z, Y, X, M] image when the caller already uploaded it.
    Returns (probs [C, Zp, Yp, Xp], net_mask int8 [Zp, Yp, Xp], iso_frame, (Xp, Yp, Zp)) on the model's grid; the batcher
    and the volume graph are gone when this returns (graphs that share the device pool must not be alive together)."""
    image = images[0]
    dev = model['device']
    ms = int(model['max_stride'])
    num_classes = int(model['out_channels'])
    spacing = [float(s) for s in model['spacing']]
    img_frame = (image.GetSpacing(), image.GetOrigin(), image.GetDirection())
    iso_frame = (spacing, image.GetOrigin(), image.GetDirection())
    X, Y, Z = image.GetSize()
    Xp, Yp, Zp = image_tools.resampled_size((X, Y, Z), image.GetSpacing(), spacing, ms)
    interp = model.get('interpolation', 'LINEAR') or 'LINEAR'
    # all modalities to the model grid in one launch: [Zp, Yp, Xp, M].  A model trained with 'BSPLINE' gets the spline: the
    # uploaded tensor is prefiltered into a temporary (src may be shared by the members of an ensemble, so not in place)
    # and evaluated onto the model grid
    if src is None:
        src = image_tools.images_to_device(images, dev)
    # a VolumeNormalizer takes its numbers from the image as uploaded -- the samples on the image grid, before any
    # resampling or prefilter -- once per member (and so once per cascade stage); without one this is the list itself
    norm = image_tools.resolve_normalizers(_model_normalizers(model, len(images)), src)
    vol = image_tools.resample_device_mc(src, img_frame, (Xp, Yp, Zp), iso_frame, interp, 0.0)
    del src
    if cfg.partition_type == 'DISABLE':
        starts, box = [[0, 0, 0]], (Xp, Yp, Zp)
    elif cfg.partition_type == 'SIZE':
        if bbox_start_voxel is not None and bbox_end_voxel is not None:
            # bounding box given in image voxels -> iso grid (seg_infer.py:292-303)
            s0 = _physical_to_index(iso_frame, _index_to_physical(img_frame, [float(v) for v in bbox_start_voxel]))
            e0 = _physical_to_index(iso_frame, _index_to_physical(img_frame, [float(v) for v in bbox_end_voxel]))
            s0 = [max(0, v) for v in s0]
            e0 = [min(v, lim) for v, lim in zip(e0, (Xp, Yp, Zp))]
        else:
            s0, e0 = [0, 0, 0], [Xp, Yp, Zp]
        starts, ends = image_partition_by_fixed_size(((Xp, Yp, Zp), spacing), s0, e0, list(cfg.partition_size),
                                                     list(cfg.partition_stride), ms)
        box = tuple(ends[0][d] - starts[0][d] for d in range(3))
    else:
        raise ValueError('Unsupported partition type!')
    order = model.get('region_class_order')    # region-based model: one sigmoid plane per region, composed label map
    probs, net_mask, _ = sliding_window_inference(model['net'], vol, starts, box, num_classes, norm,
                                                  batch_size=min(batch_size, max(1, len(starts))), blend=blend,
                                                  sigma_scale=sigma_scale, mirror_axes=mirror_axes, regions_order=order)
    return probs, net_mask, iso_frame, (Xp, Yp, Zp)


def _on_image_grid(model, image):
    """the model's grid IS the image grid: the size a stride multiple already, the spacings equal within 1e-9 relative"""
    spacing = [float(s) for s in model['spacing']]
    size = image_tools.resampled_size(image.GetSize(), image.GetSpacing(), spacing, int(model['max_stride']))
    return tuple(size) == tuple(image.GetSize()) and all(abs(a - b) <= 1e-9 * max(abs(a), abs(b), 1.0)
                                                         for a, b in zip(image.GetSpacing(), spacing))


def _image_grid_result(members, weights, cfg, images, bbox_start_voxel, bbox_end_voxel, batch_size, blend, mirror_axes):
    """the back half of a volume job, for one model (members = [model], weights = [1.0]) and for an ensemble alike: every
    member's finalized probabilities to the image grid and into the weighted sum, the label map, the connected-component
    options, the download.  blend / mirror_axes: None = what cfg says.
    One case stays off the kernel: a single member whose grid IS the image grid.  Its finalized probabilities are the
    result as they stand: index_affine is an exact identity only for an identity direction matrix and bitwise equal
    spacings, and a tap weight of 1e-16 changes a probability of 1e-30."""
    cfg_blend, sigma_scale, cfg_axes = blend_options(cfg)
    blend = cfg_blend if blend is None else check_blend_mode(blend)
    mirror_axes = cfg_axes if mirror_axes is None else check_mirror_axes(mirror_axes)
    front = (cfg, images, bbox_start_voxel, bbox_end_voxel, batch_size, blend, sigma_scale, mirror_axes)
    dev = members[0]['device']
    K = len(members)
    with torch.cuda.device(dev):
        image = images[0]
        num_classes = int(members[0]['out_channels'])
        order = members[0].get('region_class_order')
        img_frame = (image.GetSpacing(), image.GetOrigin(), image.GetDirection())
        X, Y, Z = image.GetSize()
        if K == 1 and _on_image_grid(members[0], image):
            out_probs, mask, _, _ = _member_probabilities(members[0], *front)
            if order is None:       # first maximum wins, like tensor.max(0) in the reference
                mask = out_probs.argmax(0).to(torch.int8)
        else:
            if not 1 <= num_classes <= 16:
                raise ValueError('out_channels = {}: bringing probabilities to an image grid that is not the model\'s grid '
                                 'takes 1..16 planes (seg3d_ensemble_accumulate)'.format(num_classes))
            src = image_tools.images_to_device(images, dev) if K > 1 else None     # (one member uploads, and frees, its own)
            out_probs = torch.empty((num_classes, Z, Y, X), dtype=torch.float32, device=dev)    # the first member overwrites it
            mask = torch.empty((Z, Y, X), dtype=torch.int8, device=dev)
            for k, model in enumerate(members):
                probs, _, iso_frame, _ = _member_probabilities(model, *front, src=src)
                # (outside a member's grid: class 0 with probability 1; region planes are all foreground and 0 there)
                image_tools.ensemble_accumulate_device(probs, iso_frame, out_probs, img_frame, weights[k], k == 0,
                                                       pad0=1.0 if order is None else 0.0,
                                                       mask=mask if k == K - 1 else None, regions_order=order)
                del probs       # stream-ordered: the next member may reuse the block after the launch above
            del src
        labels = list(range(1, num_classes)) if order is None else sorted(set(order))
        if getattr(cfg, 'pick_largest_cc', False) and labels:
            mask = image_tools.connected_component_filter_device(mask, labels, 'largest')
        if getattr(cfg, 'remove_small_cc', 0) and cfg.remove_small_cc > 0 and labels:
            mask = image_tools.connected_component_filter_device(mask, labels, 'min_size', int(cfg.remove_small_cc))
        mean_probs = [Image3d(out_probs[c].cpu().numpy(), *img_frame) for c in range(num_classes)]
        return mean_probs, Image3d(mask.cpu().numpy(), *img_frame)


def segmentation_volume_ensemble(members, cfg, image, bbox_start_voxel, bbox_end_voxel, weights=None, batch_size=8, blend=None,
                                 mirror_axes=None):
    """segment a whole volume with an ensemble: the weighted mean of the members' probabilities on the image grid, then the
    label map.  members: loaded models (load_single_model) that agree in
    check_ensemble_members' keys -- one per cross-validation fold, or several configurations; their network, spacing,
    max_stride and normalisers may differ.  weights: K positive numbers (ensemble_weights; None = equal).
    The members run one after another, each up to its finalized probabilities on its own grid (_member_probabilities:
    resample, partition with the bounding box mapped into that grid, sliding window with the stage's blending and mirror
    TTA); one seg3d_ensemble_accumulate launch then interpolates all its planes onto the image grid and adds them with the
    member's weight, and the launch of the last member writes the label map in the same pass (arg-max, or the region
    overwrite rule for sigmoid members).  With K > 1 also when a member's grid is the image grid.  Only one member's
    probabilities and volume graph exist at a time.
    Returns (mean_probs: list of Image3d, mask: Image3d int8), like segmentation_volume."""
    members = check_ensemble_members(members)
    weights = ensemble_weights(weights, len(members))
    images, _ = _case_images(members[0], image)
    dev = members[0]['device']
    for k, m in enumerate(members):
        if m['device'] != dev:
            raise ValueError('ensemble member {} is on {}, member 0 on {}'.format(k, m['device'], dev))
    return _image_grid_result(members, weights, cfg, images, bbox_start_voxel, bbox_end_voxel, batch_size, blend, mirror_axes)


_IMAGE_SUFFIXES = ('.mhd', '.nii', '.hdr', '.nii.gz', '.mha', '.image3d')     # core/seg_infer.py:80, 375-376
_READABLE_SUFFIXES = ('.mha', '.mhd', '.nii', '.nii.gz')


def read_test_txt(txt_file):
    """list file: first line = number of cases, then `<case name> <image path> [<path_1> ...]` per line (reference:
    seg_infer.py:23-45 reads one path).  A case's entry is its path, or the list of its M paths when M files hold its
    modalities (a single 4-D NIfTI path holds all of them)."""
    from segmentation3d.utils.file_io import readlines
    lines = readlines(txt_file)
    case_num = int(lines[0])
    if len(lines) - 1 != case_num:
        raise ValueError('case num do not equal path num!')
    names, paths = [], []
    for line in lines[1:1 + case_num]:
        parts = line.strip().split()
        if len(parts) < 2:
            raise ValueError('expected "<case name> <image path>", got: {}'.format(line))
        for path in parts[1:]:
            if not os.path.isfile(path):
                raise ValueError('image not exist: {}'.format(path))
        names.append(parts[0])
        paths.append(parts[1] if len(parts) == 2 else parts[1:])
    return names, paths


def read_case_images(entry, case):
    """the images of one inference case: a 3-D file -> one Image3d (as the reference reads it); a 4-D NIfTI file or
    several files -> the list of its M co-registered modalities (checked to share one grid)"""
    from segmentation3d.utils.image_io import read_image, read_image_modalities, check_modalities
    paths = [entry] if isinstance(entry, str) else list(entry)
    images = []
    for path in paths:
        images += read_image_modalities(path) if len(paths) == 1 else [read_image(path)]
    if len(images) == 1:
        return images[0]
    check_modalities(images, case)
    return images


def read_test_folder(folder_path):
    """every image file of a folder, case name = file name up to the image suffix (reference: seg_infer.py:68-96; DICOM
    series folders are out of scope here)"""
    import glob
    files = []
    for suf in _IMAGE_SUFFIXES:
        files += glob.glob(os.path.join(folder_path, '*' + suf))
    names, paths = [], []
    for path in sorted(set(files)):
        name = os.path.basename(path)
        for suf in _IMAGE_SUFFIXES:
            idx = name.find(suf)
            if idx != -1:
                name = name[:idx]
                break
        names.append(name)
        paths.append(path)
    return names, paths


def segmentation(input_path, model_folder, output_folder, seg_name, gpu_id, return_mask, save_mask, save_image,
                 save_prob, blend=None, mirror_axes=None):
    """volumetric image segmentation engine for image files (reference: seg_infer.py:353-493): single-scale
    ('coarse' / 'fine') or the coarse -> fine cascade ('DISABLE') through the coarse mask's bounding box.
    input_path: a list file (.txt, one or several co-registered modality paths per case), one image file, or a folder of
    image files; a 4-D NIfTI file is one case of M modalities.  Results go to `<output_folder>/<case name>/` with the
    reference's file names (seg_name, org.mha -- org_<m>.mha per modality when M > 1 --, mean_prob_<c>.mha).
    blend ('constant' | 'gaussian') and mirror_axes (e.g. ('x', 'y') or 'xy'): patch blending and mirror TTA of every
    stage; None = what the stage's section of infer_config.py says."""
    from segmentation3d.utils.image_io import write_image
    if blend is not None:
        check_blend_mode(blend)
    if mirror_axes is not None:
        mirror_axes = check_mirror_axes(mirror_axes)
    tta = dict(blend=blend, mirror_axes=mirror_axes)
    begin = time.time()
    models = load_models(model_folder, gpu_id)
    load_model_time = time.time() - begin
    if os.path.isfile(input_path):
        if input_path.endswith('.txt'):
            names, paths = read_test_txt(input_path)
        elif input_path.endswith(_IMAGE_SUFFIXES):
            names, paths = [os.path.basename(input_path)], [input_path]        # seg_infer.py:377-379: name = file name
        else:
            raise ValueError('Unsupported input path.')
    elif os.path.isdir(input_path):
        names, paths = read_test_folder(input_path)
        if len(names) == 0:
            raise ValueError('Empty test folder!')
    else:
        raise ValueError('The file {} does not exist.'.format(input_path))
    for entry in paths:
        for path in ([entry] if isinstance(entry, str) else entry):
            if not path.endswith(_READABLE_SUFFIXES):
                raise ValueError('Unsupported image format (MetaImage and NIfTI are read here): {}'.format(path))
    scale = models['infer_cfg'].general.single_scale
    if scale not in ('coarse', 'fine', 'DISABLE'):
        raise ValueError('Unsupported scale type!')
    masks, total = [], 0.0
    for i, path in enumerate(paths):
        print('{}: {}'.format(i, path))
        begin = time.time()
        image = read_case_images(path, names[i])
        modalities = image if isinstance(image, list) else [image]
        for m, im in enumerate(modalities):
            if im.array.dtype != np.float32:                                    # sitk.ReadImage(path, sitk.sitkFloat32)
                modalities[m] = im.like(im.array.astype(np.float32))
        image = modalities if len(modalities) > 1 else modalities[0]
        read_image_time = time.time() - begin
        begin = time.time()
        if scale == 'coarse':
            mean_probs, mask = _segment_stage(models, 'coarse', image, None, None, tta)
        elif scale == 'fine':
            mean_probs, mask = _segment_stage(models, 'fine', image, None, None, tta)
        else:
            # coarse -> fine cascade (seg_infer.py:428-444): the coarse mask's bounding box restricts the fine pass
            from segmentation3d.utils.image_tools import get_bounding_box
            print('Coarse segmentation: ')
            _, mask = _segment_stage(models, 'coarse', image, None, None, tta)
            start_voxel, end_voxel = get_bounding_box(mask, None)
            if start_voxel is None:
                start_voxel, end_voxel = [0, 0, 0], list(mask.GetSize())
            bbox_ratio = 100
            for idx in range(3):
                bbox_ratio *= (end_voxel[idx] - start_voxel[idx]) / mask.GetSize()[idx]
            print('Fine segmentation (bbox ratio: {:.2f}%): '.format(bbox_ratio))
            mean_probs, mask = _segment_stage(models, 'fine', image, start_voxel, end_voxel, tta)
        torch.cuda.synchronize()
        inference_time = time.time() - begin
        total += inference_time
        if return_mask:
            masks.append(mask)
        begin = time.time()
        case = names[i]
        if save_mask or save_image or save_prob:
            os.makedirs(os.path.join(output_folder, case), exist_ok=True)
        if save_mask:
            write_image(mask, os.path.join(output_folder, case, seg_name))
        if save_image:
            if len(modalities) == 1:
                write_image(image, os.path.join(output_folder, case, 'org.mha'))
            else:
                for m, im in enumerate(modalities):
                    write_image(im, os.path.join(output_folder, case, 'org_{}.mha'.format(m)))
        if save_prob:
            for c, p in enumerate(mean_probs):
                write_image(p, os.path.join(output_folder, case, 'mean_prob_{}.mha'.format(c)))
        save_time = time.time() - begin
        print('total test time: {:.2f}, average inference time: {:.2f}'.format(
            load_model_time + read_image_time + inference_time + save_time, total / (i + 1)))
    return masks
