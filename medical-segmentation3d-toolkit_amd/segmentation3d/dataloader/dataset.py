"""Training data path: `SegmentationDataset` with the reference's constructor, sampling
methods and RNG call order (dataloader/dataset.py:55-209), but the crop itself runs on the GPU.

The reference reads both volumes from disk, resamples a crop with SimpleITK and normalises it in a DataLoader worker
for every sample; at >150 patches/s per GPU four such workers cannot feed eight GPUs.  Here every case is read ONCE
(MetaImage, utils/mha_io.py), kept resident in HBM, and a sample costs two launches of the resampling kernel
(csrc/postproc.hip: image LINEAR / NN / BSPLINE -- the resident volume then holds the spline
coefficients, prefiltered once at load, csrc/bspline.hip --, mask NN or, with `mask_interpolation = 'LABEL_LINEAR'`,
the per-label trilinear vote of row f22) plus the on-device normaliser (csrc/patch.hip) -- no worker
processes, no host copies.  The random decisions (crop centre, translation, scale) stay on the host with numpy's
global RNG in exactly the reference's order, so a seeded run draws the same crops.
`DeviceCropLoader` batches the samples of a sampler into device tensors for core/seg_train.train().
Optional augmentation beyond the reference (off by default): axis mirrors, rotation and
elastic deformation inside the resampling launches, intensity transforms in one fused pass over the normalised crop
(csrc/augment.hip); its random decisions are drawn after the reference's, and none is drawn while it is off.
A second optional section, `resolution_augmentation` (row f13): Gaussian blur and low-resolution simulation of the
normalised crop (csrc/augment_filter.hip), drawn after every other decision of the sample and before the intensity pass.
How the cases are kept (row f21, two optional keys, defaults = everything above): `resident_storage = 'compact'` keeps integer
images as int16 and masks as uint8 -- the resampling kernels convert on load, the crops are bit-identical -- and
`resident_budget_gb` stages the cases that do not fit in pinned host memory and uploads them per sample.
"""
import os

import numpy as np
import pandas as pd
import torch
from torch.utils.data import Dataset

from segmentation3d import _engine as E
from segmentation3d.utils.file_io import readlines
from segmentation3d.utils.image3d import Image3d
from segmentation3d.utils import image_tools
from segmentation3d.utils.image_io import read_image, read_image_modalities, num_modalities, check_modalities


def _is_4d_nifti(path):
    return (path.endswith('.nii') or path.endswith('.nii.gz')) and os.path.isfile(path) and num_modalities(path) > 1


def read_train_txt(imlist_file):
    """txt list (dataset.py:12-32): first line = `<number of cases>` or `<number of cases> <M>`, then per case M image
    paths (one per line) and the mask path.  One 4-D NIfTI path may stand in for the M image paths.  A case's image entry
    is a path, or the list of its M paths when M > 1 files hold its modalities; single-modality files give exactly the
    reference's lists."""
    lines = readlines(imlist_file)
    head = lines[0].split()
    num_cases = int(head[0])
    num_mod = int(head[1]) if len(head) > 1 else 1
    if num_mod < 1:
        raise ValueError('{}: number of modalities must be positive, got {}'.format(imlist_file, num_mod))
    if len(head) == 1 and len(lines) - 1 < num_cases * 2:
        raise ValueError('too few lines in imlist file')
    im_list, seg_list = [], []
    pos = 1
    for i in range(num_cases):
        if pos >= len(lines):
            raise ValueError('too few lines in imlist file')
        first = lines[pos]
        if num_mod == 1 or _is_4d_nifti(first):
            paths = [first]
            if len(head) > 1 and case_modalities(first) != num_mod:
                raise ValueError('case {}: {} holds {} modalities, the list declares {}'.format(
                    i, first, case_modalities(first), num_mod))
        else:
            paths = lines[pos:pos + num_mod]
        pos += len(paths)
        if pos >= len(lines):
            raise ValueError('too few lines in imlist file')
        seg_path = lines[pos]
        pos += 1
        for im_path in paths:
            assert os.path.isfile(im_path), 'image not exist: {}'.format(im_path)
        assert os.path.isfile(seg_path), 'mask not exist: {}'.format(seg_path)
        im_list.append(paths[0] if len(paths) == 1 else paths)
        seg_list.append(seg_path)
    return im_list, seg_list


def _modality_columns(columns):
    """image_path, image_path_1, ... image_path_{M-1} in modality order"""
    cols = ['image_path']
    while 'image_path_{}'.format(len(cols)) in columns:
        cols.append('image_path_{}'.format(len(cols)))
    return cols


def read_train_csv(imlist_file, mode='train'):
    """csv list with columns image_name, image_path (, image_path_1 ... image_path_{M-1}) (, mask_path)
    (dataset.py:35-52); with more than one image column a case's image entry is the list of its M paths"""
    images_df = pd.read_csv(imlist_file)
    cols = _modality_columns(images_df.columns)
    if len(cols) == 1:
        image_paths = images_df['image_path'].tolist()
    else:
        image_paths = [list(row) for row in images_df[cols].itertuples(index=False, name=None)]
    if mode == 'test':
        return images_df['image_name'].tolist(), image_paths
    if mode in ('train', 'validation'):
        return image_paths, images_df['mask_path'].tolist()
    raise ValueError('Unsupported mode type.')


def case_modalities(entry):
    """number of modalities of a case's image entry (a path or a list of paths) from the file headers alone"""
    paths = [entry] if isinstance(entry, str) else list(entry)
    if len(paths) == 1:
        return num_modalities(paths[0])
    for path in paths:
        if num_modalities(path) != 1:
            raise ValueError('{}: a 4-D file stands in for all modalities of a case, not one of several'.format(path))
    return len(paths)


def read_case_modalities(entry, case, dtype=np.float32):
    """list of M Image3d of one case (one 4-D NIfTI or M 3-D files), checked to share one grid; dtype=None keeps the
    stored element types"""
    paths = [entry] if isinstance(entry, str) else list(entry)
    images = []
    for path in paths:
        images += read_image_modalities(path, dtype)
    check_modalities(images, case)
    return images


# how the cases are kept for the run (not in the reference): the two optional keys
# dataset.resident_storage / dataset.resident_budget_gb
RESIDENT_STORAGE = ('fp32', 'compact')
RESIDENT_GB = 10 ** 9       # bytes of one GB of resident_budget_gb


def validate_resident_options(storage, budget):
    """(dataset.resident_storage, dataset.resident_budget_gb) -> (storage, budget in bytes or None).  ValueError for a
    storage that is not 'fp32' or 'compact' and for a budget that is neither None nor a finite positive number."""
    if not isinstance(storage, str) or storage not in RESIDENT_STORAGE:
        raise ValueError('dataset.resident_storage = {!r}: one of {}'.format(storage, RESIDENT_STORAGE))
    if budget is None:
        return storage, None
    if isinstance(budget, bool) or not isinstance(budget, (int, float, np.integer, np.floating)):
        raise ValueError('dataset.resident_budget_gb = {!r}: None or a positive number of GB'.format(budget))
    if not (np.isfinite(budget) and budget > 0):
        raise ValueError('dataset.resident_budget_gb = {!r} must be finite and positive'.format(budget))
    return storage, float(budget) * RESIDENT_GB


# how the mask crop is interpolated (not in the reference): the optional key
# dataset.mask_interpolation.  'NN' is the reference's nearest-neighbour lookup, 'LABEL_LINEAR' the per-label trilinear vote
MASK_INTERPOLATION = ('NN', 'LABEL_LINEAR')


def validate_mask_interpolation(value):
    """dataset.mask_interpolation -> the value; ValueError for anything that is not 'NN' or 'LABEL_LINEAR'"""
    if not isinstance(value, str) or value not in MASK_INTERPOLATION:
        raise ValueError('dataset.mask_interpolation = {!r}: one of {}'.format(value, MASK_INTERPOLATION))
    return value


def _pinned_copy(tensor):
    """a device tensor downloaded into pinned host memory (a blocking copy)"""
    host = torch.empty(tensor.shape, dtype=tensor.dtype, pin_memory=True)
    host.copy_(tensor)
    return host


class _Case(object):
    """one case resident on the device, plus the host-side per-slice label histogram that lets MASK sampling pick the k-th
    voxel of a label (in np.argwhere order) without scanning the volume.  `image` is one modality or a list of M
    co-registered modalities, kept as ONE channels-last [Z, Y, X, M] fp32 tensor `volume` (a BraTS case of
    240 x 240 x 155 x 4 is 143 MB resident); the attribute `image` is that tensor, or its [Z, Y, X] view for one
    modality.  The mask and the histogram are the same for any M.
    bspline: `volume` is prefiltered in place once, here, and holds the cubic B-spline COEFFICIENTS of the image from then
    on (same footprint; image_tools.bspline_prefilter_device), which is what a 'BSPLINE' crop evaluates.
    compact: `volume` / `seg` are int16 / uint8 (or int16) tensors where the values allow it, 3 bytes per voxel and modality
    instead of 8; the resampling kernels convert on load, so every crop is the fp32 case's bit for bit.
    staged (a data set with a budget that these bytes no longer fit): `volume` / `seg` / `image` are None, the arrays wait
    in pinned host memory (`volume_pinned`, `seg_pinned`) and tensors() uploads them per sample."""

    def __init__(self, image, seg, device, bspline=False, volume_normalizers=None, compact=False, admit=None):
        images = image if isinstance(image, (list, tuple)) else [image]
        image = images[0]
        self.num_modality = len(images)
        self.frame = (image.GetSpacing(), image.GetOrigin(), image.GetDirection())
        self.seg_frame = (seg.GetSpacing(), seg.GetOrigin(), seg.GetDirection())
        self.size = image.GetSize()
        self.seg_size = seg.GetSize()
        self.seg_host = np.array(seg.array, order='C')                       # [z, y, x], label values as stored
        # compact: image and mask stay in the integer type that holds them exactly
        # (image_tools.storage_dtype); the B-spline coefficients of an image are no integers, so that image stays fp32
        image_dtype = image_tools.case_storage_dtype(images) if compact and not bspline else np.dtype(np.float32)
        seg_dtype = image_tools.storage_dtype(self.seg_host, 'mask') if compact else np.dtype(np.float32)
        # the fp32 samples on the device: the resident tensor itself, or -- a compact image that needs its statistics -- a
        # temporary that is freed once the numbers are known
        volume = None
        if image_dtype == np.float32 or volume_normalizers is not None:
            volume = image_tools.images_to_device(images, device)           # [Z, Y, X, M]
        # a data set with a VolumeNormalizer: this case's own numbers, from the SAMPLES (before the prefilter below)
        self.normalizers = self.norm_params = None
        if volume_normalizers is not None:
            with torch.cuda.device(volume.device):
                self.normalizers = image_tools.resolve_normalizers(volume_normalizers, volume)
            self.norm_params = image_tools.normalizer_params(self.normalizers, self.num_modality)
        if image_dtype != np.float32:
            volume = image_tools.images_to_device(images, device, image_dtype)
        elif bspline:
            image_tools.bspline_prefilter_device(volume, out=volume)
        seg_volume = torch.from_numpy(self.seg_host.astype(seg_dtype)).to(device)
        self.nbytes = volume.numel() * volume.element_size() + seg_volume.numel() * seg_volume.element_size()
        # a data set with a budget asks `admit` whether these bytes still fit; if not the case is STAGED: its two arrays
        # wait in pinned host memory and tensors() uploads them for every sample
        self.staged = admit is not None and not admit(self.nbytes)
        self._device = volume.device
        self.volume_pinned = self.seg_pinned = None
        if self.staged:
            self.volume_pinned, self.seg_pinned = _pinned_copy(volume), _pinned_copy(seg_volume)
            volume = seg_volume = None
        self.volume, self.seg = volume, seg_volume
        self.image = None if self.staged else (volume[..., 0] if self.num_modality == 1 else volume)
        self._slice_counts = {}

    def tensors(self):
        """(volume, seg) on the device.  A resident case hands out its tensors; a staged one uploads its pinned arrays
        on the current stream (two asynchronous copies), and the caller drops the result once the sample's launches are
        queued: the caching allocator is stream-ordered, so the memory is reused only after those launches have run."""
        if not self.staged:
            return self.volume, self.seg
        return (self.volume_pinned.to(self._device, non_blocking=True),
                self.seg_pinned.to(self._device, non_blocking=True))

    def label_voxel(self, label, draw):
        """`draw(n)` -> index in [0, n) of the voxel to take among the n voxels equal to `label`, enumerated like
        np.argwhere (z, then y, then x); returns (x, y, z) or None when the label is absent (draw is not called)"""
        cum = self._slice_counts.get(label)
        if cum is None:
            per_slice = (self.seg_host == label).reshape(self.seg_host.shape[0], -1).sum(1)
            cum = np.concatenate([[0], np.cumsum(per_slice)])
            self._slice_counts[label] = cum
        total = int(cum[-1])
        if total == 0:
            return None
        k = int(draw(total))
        z = int(np.searchsorted(cum, k, side='right') - 1)
        yx = np.argwhere(self.seg_host[z] == label)[k - int(cum[z])]
        return [int(yx[1]), int(yx[0]), z]


# training augmentation (not in the reference): keys and defaults of the `augmentation`
# section -- everything off
AUGMENTATION_DEFAULTS = {
    'rotation_deg': [0.0, 0.0, 0.0],        # per-axis max angle (x, y, z), uniform in [-a, a]
    'rotation_prob': 1.0,
    'elastic_grid_mm': 32.0,                # control-point spacing h of the cubic B-spline displacement field
    'elastic_magnitude_mm': [0.0, 0.0],     # a ~ uniform in [lo, hi]; control displacements uniform in [-a, a] mm
    'elastic_prob': 0.0,
    'brightness': [1.0, 1.0],               # multiplicative, uniform in [lo, hi]
    'brightness_prob': 0.0,
    'contrast': [1.0, 1.0],
    'contrast_prob': 0.0,
    'gamma': [1.0, 1.0],
    'gamma_prob': 0.0,
    'gamma_invert_prob': 0.0,
    'noise_sigma': [0.0, 0.0],
    'noise_prob': 0.0,
}


def _range2(name, value, lowest, strict):
    try:
        lo, hi = (float(v) for v in value)
    except (TypeError, ValueError):
        raise ValueError('augmentation.{} must be a [lo, hi] pair, got {!r}'.format(name, value))
    ok = np.isfinite(lo) and np.isfinite(hi) and lo <= hi and (lo > lowest if strict else lo >= lowest)
    if not ok:
        raise ValueError('augmentation.{} = {!r}: need {} {} lo <= hi'.format(name, value, lowest, '<' if strict else '<='))
    return [lo, hi]


def validate_augmentation(augmentation):
    """the `augmentation` section (dict / EasyDict / None) -> a plain dict with every key of AUGMENTATION_DEFAULTS, or None
    when the section is absent or switches nothing on.  Unknown keys, bad ranges, probabilities outside [0, 1] and an
    elastic magnitude that does not satisfy the folding bound raise ValueError.
    Folding: a partial derivative of a cubic B-spline field is a convex combination of differences of neighbouring
    control values, so with control displacements in [-a, a] every entry of the Jacobian of u is at most 2a / h, its
    Frobenius norm at most 6a / h, and id + u is injective when a < h / 6.  The bound is sufficient, not necessary."""
    if augmentation is None:
        return None
    if not hasattr(augmentation, 'keys'):
        raise ValueError('augmentation must be a dict, got {!r}'.format(type(augmentation)))
    unknown = sorted(set(augmentation.keys()) - set(AUGMENTATION_DEFAULTS))
    if unknown:
        raise ValueError('unknown augmentation option(s) {}; known: {}'.format(unknown, sorted(AUGMENTATION_DEFAULTS)))
    a = {k: augmentation[k] if k in augmentation else v for k, v in AUGMENTATION_DEFAULTS.items()}
    for key in a:
        if key.endswith('_prob'):
            try:
                pr = float(a[key])
            except (TypeError, ValueError):
                raise ValueError('augmentation.{} must be a number, got {!r}'.format(key, a[key]))
            if not 0.0 <= pr <= 1.0:
                raise ValueError('augmentation.{} = {!r} outside [0, 1]'.format(key, a[key]))
            a[key] = pr
    try:
        rot = [float(v) for v in a['rotation_deg']]
    except (TypeError, ValueError):
        raise ValueError('augmentation.rotation_deg must be three angles, got {!r}'.format(a['rotation_deg']))
    if len(rot) != 3 or not all(np.isfinite(v) and 0.0 <= v <= 180.0 for v in rot):
        raise ValueError('augmentation.rotation_deg = {!r}: three angles in [0, 180]'.format(a['rotation_deg']))
    a['rotation_deg'] = rot
    try:
        h = float(a['elastic_grid_mm'])
    except (TypeError, ValueError):
        raise ValueError('augmentation.elastic_grid_mm must be a number, got {!r}'.format(a['elastic_grid_mm']))
    if not (np.isfinite(h) and h > 0.0):
        raise ValueError('augmentation.elastic_grid_mm = {!r} must be positive'.format(a['elastic_grid_mm']))
    a['elastic_grid_mm'] = h
    a['elastic_magnitude_mm'] = _range2('elastic_magnitude_mm', a['elastic_magnitude_mm'], 0.0, False)
    if not a['elastic_magnitude_mm'][1] < h / 6.0:
        raise ValueError('augmentation.elastic_magnitude_mm = {!r}: the largest magnitude must be below elastic_grid_mm / 6 '
                         '= {:g} mm, which keeps the deformation free of folds'.format(a['elastic_magnitude_mm'], h / 6.0))
    for key in ('brightness', 'contrast', 'gamma'):
        a[key] = _range2(key, a[key], 0.0, True)
    a['noise_sigma'] = _range2('noise_sigma', a['noise_sigma'], 0.0, False)
    on = {
        'rotation': a['rotation_prob'] > 0.0 and any(v > 0.0 for v in rot),
        'elastic': a['elastic_prob'] > 0.0 and a['elastic_magnitude_mm'][1] > 0.0,
        'brightness': a['brightness_prob'] > 0.0 and a['brightness'] != [1.0, 1.0],
        'contrast': a['contrast_prob'] > 0.0 and a['contrast'] != [1.0, 1.0],
        'gamma': a['gamma_prob'] > 0.0 and a['gamma'] != [1.0, 1.0],
        'noise': a['noise_prob'] > 0.0 and a['noise_sigma'][1] > 0.0,
    }
    if not any(on.values()):
        return None
    a['enabled'] = on
    return a


# blur / low-resolution simulation (not in the reference): keys and defaults of the
# `resolution_augmentation` section -- everything off.  A section of its own: AUGMENTATION_DEFAULTS stays as it is.
RESOLUTION_AUGMENTATION_DEFAULTS = {
    'blur_sigma_vox': [0.0, 0.0],           # sigma in voxels of the crop grid, uniform in [lo, hi], hi <= 2
    'blur_prob': 0.0,                       # per modality
    'lowres_zoom': [1.0, 1.0],              # zoom of the low grid, uniform in [lo, hi], 0 < lo <= hi <= 1
    'lowres_prob': 0.0,                     # per modality
}


def validate_resolution_augmentation(section):
    """the `resolution_augmentation` section (dict / EasyDict / None) -> a plain dict with every key of
    RESOLUTION_AUGMENTATION_DEFAULTS plus `enabled` = {'blur', 'lowres'}, or None when the section is absent or switches
    nothing on.  Raises ValueError for a section that is not a dict, unknown keys, a probability outside [0, 1], a
    blur_sigma_vox pair that breaks 0 <= lo <= hi <= 2 and a lowres_zoom pair that breaks 0 < lo <= hi <= 1.
    Blur is on iff blur_prob > 0 and hi > 0 (then lo > 0 is required: a drawn sigma of 0 has no taps); the low-resolution
    simulation is on iff lowres_prob > 0 and lo < 1."""
    if section is None:
        return None
    if not hasattr(section, 'keys'):
        raise ValueError('resolution_augmentation must be a dict, got {!r}'.format(type(section)))
    unknown = sorted(set(section.keys()) - set(RESOLUTION_AUGMENTATION_DEFAULTS))
    if unknown:
        raise ValueError('unknown resolution_augmentation option(s) {}; known: {}'.format(
            unknown, sorted(RESOLUTION_AUGMENTATION_DEFAULTS)))
    a = {k: section[k] if k in section else v for k, v in RESOLUTION_AUGMENTATION_DEFAULTS.items()}
    for key in ('blur_prob', 'lowres_prob'):
        try:
            pr = float(a[key])
        except (TypeError, ValueError):
            raise ValueError('resolution_augmentation.{} must be a number, got {!r}'.format(key, a[key]))
        if not 0.0 <= pr <= 1.0:
            raise ValueError('resolution_augmentation.{} = {!r} outside [0, 1]'.format(key, a[key]))
        a[key] = pr
    pairs = {}
    for key in ('blur_sigma_vox', 'lowres_zoom'):
        try:
            lo, hi = (float(v) for v in a[key])
        except (TypeError, ValueError):
            raise ValueError('resolution_augmentation.{} must be a [lo, hi] pair, got {!r}'.format(key, a[key]))
        pairs[key] = [lo, hi]
    lo, hi = pairs['blur_sigma_vox']
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 <= lo <= hi <= image_tools.BLUR_MAX_SIGMA):
        raise ValueError('resolution_augmentation.blur_sigma_vox = {!r}: need 0 <= lo <= hi <= {:g}'.format(
            a['blur_sigma_vox'], image_tools.BLUR_MAX_SIGMA))
    lo, hi = pairs['lowres_zoom']
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= hi <= 1.0):
        raise ValueError('resolution_augmentation.lowres_zoom = {!r}: need 0 < lo <= hi <= 1'.format(a['lowres_zoom']))
    a.update(pairs)
    on = {
        'blur': a['blur_prob'] > 0.0 and a['blur_sigma_vox'][1] > 0.0,
        'lowres': a['lowres_prob'] > 0.0 and a['lowres_zoom'][0] < 1.0,
    }
    if on['blur'] and not a['blur_sigma_vox'][0] > 0.0:
        raise ValueError('resolution_augmentation.blur_sigma_vox = {!r}: an enabled blur needs lo > 0'.format(
            a['blur_sigma_vox']))
    if not any(on.values()):
        return None
    a['enabled'] = on
    return a


class SegmentationDataset(Dataset):
    """training data set for volumetric segmentation (constructor as dataloader/dataset.py:58-100)"""

    def __init__(self, imlist_file, num_classes, spacing, crop_size, sampling_method, random_translation, random_scale,
                 interpolation, crop_normalizers, device=None, random_mirror_axes=(), augmentation=None,
                 resolution_augmentation=None, resident_storage='fp32', resident_budget_gb=None, mask_interpolation='NN'):
        # how the cases are kept: 'compact' stores integer data in its integer type, a budget (GB of 1e9 bytes) stages the
        # cases that no longer fit in pinned host memory.  The defaults are the data set of always: fp32, everything resident
        self.resident_storage, self._budget_bytes = validate_resident_options(resident_storage, resident_budget_gb)
        # how the mask crop is cut: 'NN' (the reference, the default) or the per-label trilinear vote 'LABEL_LINEAR'
        self.mask_interpolation = validate_mask_interpolation(mask_interpolation)
        if imlist_file.endswith('txt'):
            self.im_list, self.seg_list = read_train_txt(imlist_file)
        elif imlist_file.endswith('csv'):
            self.im_list, self.seg_list = read_train_csv(imlist_file)
        else:
            raise ValueError('imseg_list must be a txt file')
        self.num_classes = num_classes
        self.spacing = np.array(spacing, dtype=np.double)
        assert self.spacing.size == 3, 'only 3-element of spacing is supported'
        self.crop_size = np.array(crop_size, dtype=np.int32)
        assert self.crop_size.size == 3, 'only 3-element of crop size is supported'
        self.sampling_method = sampling_method
        assert self.sampling_method in ('CENTER', 'GLOBAL', 'MASK', 'HYBRID'), \
            'sampling_method must be CENTER, GLOBAL, MASK or HYBRID'
        self.random_translation = np.array(random_translation, dtype=np.double)
        assert self.random_translation.size == 3, 'Only 3-element of random translation is supported'
        self.random_scale = np.array(random_scale, dtype=np.double)
        assert self.random_scale.size == 2, 'Only 2-element of random scale is supported'
        self.interpolation = interpolation
        assert self.interpolation in ('LINEAR', 'NN', 'BSPLINE'), 'interpolation must be LINEAR, NN or BSPLINE'
        self.crop_normalizers = crop_normalizers
        assert isinstance(self.crop_normalizers, list), 'crop normalizers must be a list'
        # mirror augmentation (not in the reference): every listed axis is mirrored with probability 1/2 per sample
        self.random_mirror_axes = []
        for a in (random_mirror_axes or ()):
            if a not in ('x', 'y', 'z'):
                raise ValueError("unknown mirror axis {!r}: 'x', 'y' or 'z'".format(a))
            if a not in self.random_mirror_axes:
                self.random_mirror_axes.append(a)
        # rotation / elastic / intensity augmentation (not in the reference): None when the section is absent or all off,
        # and then a sample takes the code path and draws the RNG stream it always did
        self.augmentation = validate_augmentation(augmentation)
        if self.augmentation is not None and self.augmentation['enabled']['elastic']:
            # the kernel's per-axis factor sp / h must be <= 1, and its weight tables + control grid live in 64 KB of LDS
            coarsest = self.spacing * self.random_scale[1]
            if self.augmentation['elastic_grid_mm'] < float(np.max(coarsest)):
                raise ValueError('augmentation.elastic_grid_mm = {:g} is below the coarsest crop spacing {:g} mm'.format(
                    self.augmentation['elastic_grid_mm'], float(np.max(coarsest))))
            dims = image_tools.bspline_control_dims(self.crop_size, coarsest, self.augmentation['elastic_grid_mm'])
            if int(np.sum(self.crop_size)) * 36 + int(np.prod(dims)) * 12 > 65536:
                raise ValueError('augmentation.elastic_grid_mm = {:g}: a control grid of {} points does not fit the 64 KB '
                                 'of on-chip memory the resampling kernel keeps it in'.format(
                                     self.augmentation['elastic_grid_mm'], dims))
        # blur / low-resolution simulation (not in the reference): None when the section is absent or off -- no draw, no
        # launch, the same tensors
        self.resolution_augmentation = validate_resolution_augmentation(resolution_augmentation)
        # modalities per case from the list and the file headers (no volume is read here): every case must have the same M,
        # and there is one normaliser per modality (None: no normalisation, dataset.py:202)
        self._num_modality = 1
        for k, entry in enumerate(self.im_list):
            m = case_modalities(entry)
            if k == 0:
                self._num_modality = m
            elif m != self._num_modality:
                raise ValueError('case {}: {} modalities, case {} has {}'.format(self.case_name(k), m, self.case_name(0),
                                                                                 self._num_modality))
        if not 1 <= self._num_modality <= 8:
            raise ValueError('case {}: {} modalities, 1..8 are supported'.format(self.case_name(0), self._num_modality))
        # (a single-modality case takes crop_normalizers[0], as dataset.py:199-203 does)
        norms = self.crop_normalizers[:1] if self._num_modality == 1 else self.crop_normalizers
        if len(norms) != self._num_modality:
            raise ValueError('case {}: {} modalities but {} crop normalizers (one per modality, None for none)'.format(
                self.case_name(0), self._num_modality, len(self.crop_normalizers)))
        # a VolumeNormalizer (type 2) has no numbers until it meets a volume: every case resolves the list against its own
        # volume at load and keeps its own struct (_Case.norm_params); without one the struct is the data set's, as ever
        self._volume_normalizers = list(norms) if image_tools.has_volume_normalizer(norms) else None
        self._norm_params = None if self._volume_normalizers is not None else \
            image_tools.normalizer_params(norms, self._num_modality)
        self.device = device if device is not None else torch.device('cuda', torch.cuda.current_device())
        self._cases = {}

    def __len__(self):
        return len(self.im_list)

    def num_modality(self):
        return self._num_modality

    def case_name(self, index):
        entry = self.im_list[index]
        image_path = entry if isinstance(entry, str) else entry[0]
        return os.path.basename(os.path.dirname(image_path)) + '_' + os.path.basename(image_path)

    # ---- resident volumes --------------------------------------------------------------------------------------------
    def case(self, index):
        """the case, loaded at first touch.  With a budget it becomes resident if the bytes already resident plus its own
        (image + mask tensor in their storage dtype) fit, and is staged otherwise; nothing is ever evicted -- first come,
        first resident -- so a seeded sampler gives the same split every run.  (The first touch of a staged case still
        passes through the device once: that is where its layout, statistics and B-spline coefficients are made.)"""
        c = self._cases.get(index)
        if c is None:
            compact = self.resident_storage == 'compact'
            image = read_case_modalities(self.im_list[index], self.case_name(index), None if compact else np.float32)
            c = _Case(image, read_image(self.seg_list[index], dtype=None), self.device,
                      bspline=self.interpolation == 'BSPLINE', volume_normalizers=self._volume_normalizers,
                      compact=compact, admit=None if self._budget_bytes is None else self._admit)
            self._cases[index] = c
        return c

    def has_budget(self):
        return self._budget_bytes is not None

    def _admit(self, nbytes):
        return self.resident_bytes() + nbytes <= self._budget_bytes

    def resident_bytes(self):
        """bytes of the image and mask tensors of the cases resident on the device"""
        return sum(c.nbytes for c in self._cases.values() if not c.staged)

    def num_resident(self):
        return sum(1 for c in self._cases.values() if not c.staged)

    def num_staged(self):
        """cases touched so far that did not fit the budget and are uploaded per sample"""
        return sum(1 for c in self._cases.values() if c.staged)

    # ---- crop centres (host, numpy global RNG, reference call order) ------------------------------------------------------
    def global_sample(self, case):
        """uniform position such that the crop lies inside the image where it fits (dataset.py:110-127)"""
        origin = case.seg_frame[1]
        im_size_mm = [case.seg_size[idx] * case.seg_frame[0][idx] for idx in range(3)]
        crop_size_mm = self.crop_size * self.spacing
        sp = np.array(origin, dtype=np.double)
        for i in range(3):
            if im_size_mm[i] > crop_size_mm[i]:
                sp[i] = origin[i] + np.random.uniform(0, im_size_mm[i] - crop_size_mm[i])
        return sp + crop_size_mm / 2

    def center_sample(self, case):
        """world coordinate of the image centre (dataset.py:129-142)"""
        spacing, origin, direction = (np.asarray(v, dtype=np.double) for v in case.seg_frame)
        end_voxel = np.array([case.seg_size[idx] - 1 for idx in range(3)], dtype=np.double)
        end_world = origin + direction.reshape(3, 3) @ (spacing * end_voxel)
        return np.array([(origin[idx] + end_world[idx]) / 2.0 for idx in range(3)], dtype=np.double)

    def _mask_sample(self, case):
        label = np.random.randint(1, self.num_classes)
        voxel = case.label_voxel(label, lambda n: np.random.randint(0, n))
        if voxel is None:                      # if no segmentation
            return self.global_sample(case)
        spacing, origin, direction = (np.asarray(v, dtype=np.double) for v in case.seg_frame)
        return origin + direction.reshape(3, 3) @ (spacing * np.array(voxel, dtype=np.double))

    def sample_crop_geometry(self, index):
        """(centre, crop spacing) of the next sample of case `index` -- consumes the RNG like dataset.py:166-200"""
        case = self.case(index)
        if self.sampling_method == 'CENTER':
            center = self.center_sample(case)
        elif self.sampling_method == 'GLOBAL':
            center = self.global_sample(case)
        elif self.sampling_method == 'MASK':
            center = self._mask_sample(case)
        else:  # HYBRID
            center = self.global_sample(case) if index % 2 else self._mask_sample(case)
        center = center + np.random.uniform(-self.random_translation, self.random_translation, size=[3])
        crop_spacing = self.spacing * np.random.uniform(self.random_scale[0], self.random_scale[1])
        return center, crop_spacing

    def sample_mirror(self):
        """(x, y, z) mirror flags of the next sample: one randint(0, 2, size=k) over the k random_mirror_axes, drawn after
        the scale draw; with no mirror axes nothing is drawn, so the RNG stream is the reference's"""
        flags = [False, False, False]
        if self.random_mirror_axes:
            draw = np.random.randint(0, 2, size=len(self.random_mirror_axes))
            for a, d in zip(self.random_mirror_axes, draw):
                flags['xyz'.index(a)] = bool(d)
        return tuple(flags)

    def sample_augmentation(self, crop_spacing):
        """the random decisions of the rotation / elastic / intensity augmentation of the next sample, drawn after the
        mirror draw with numpy's global RNG in this fixed order; a transform that is disabled (probability 0 or a
        neutral range) draws NOTHING, so with the section absent or all off the stream is the reference's plus the
        mirror draw.  An enabled transform first draws its gate, uniform() < prob, then -- if the gate is open -- its
        values:
          1. rotation:  gate; uniform(-a, a, size=3) degrees, a = rotation_deg (x, y, z)
          2. elastic:   gate; magnitude a = uniform(lo, hi); control tensor uniform(-a, a, size=(gz, gy, gx, 3)) with
                        (gx, gy, gz) = bspline_control_dims(crop_size, crop_spacing, elastic_grid_mm)
          3. per modality m = 0 .. M-1, each drawing independently:
                brightness: gate; uniform(lo, hi)      contrast: gate; uniform(lo, hi)
                gamma:      gate; uniform(lo, hi); then, if gamma_invert_prob > 0, uniform() < gamma_invert_prob
                noise:      gate; sigma = uniform(lo, hi)
          4. noise enabled: the noise seed, one randint(0, 2^63) (whether or not a gate opened)
        -> dict(rotation = (gx, gy, gz) radians or None, control = float32 [gz, gy, gx, 3] mm or None, intensity = list of
        M parameter dicts (image_tools.augment_intensity_device) or None, seed = int), or None without augmentation"""
        a = self.augmentation
        if a is None:
            return None
        on = a['enabled']
        rotation = control = None
        if on['rotation'] and np.random.uniform() < a['rotation_prob']:
            lim = np.array(a['rotation_deg'], dtype=np.double)
            deg = np.random.uniform(-lim, lim, size=[3])
            rotation = tuple(float(v) for v in np.deg2rad(deg))
        if on['elastic'] and np.random.uniform() < a['elastic_prob']:
            mag = np.random.uniform(a['elastic_magnitude_mm'][0], a['elastic_magnitude_mm'][1])
            gx, gy, gz = image_tools.bspline_control_dims(self.crop_size, crop_spacing, a['elastic_grid_mm'])
            control = np.random.uniform(-mag, mag, size=(gz, gy, gx, 3)).astype(np.float32)
        intensity, any_intensity = [], False
        for m in range(self._num_modality):
            p = {}
            if on['brightness'] and np.random.uniform() < a['brightness_prob']:
                p['brightness'] = float(np.random.uniform(a['brightness'][0], a['brightness'][1]))
            if on['contrast'] and np.random.uniform() < a['contrast_prob']:
                p['contrast'] = float(np.random.uniform(a['contrast'][0], a['contrast'][1]))
            if on['gamma'] and np.random.uniform() < a['gamma_prob']:
                p['gamma'] = float(np.random.uniform(a['gamma'][0], a['gamma'][1]))
                if a['gamma_invert_prob'] > 0.0:
                    p['invert'] = bool(np.random.uniform() < a['gamma_invert_prob'])
            if on['noise'] and np.random.uniform() < a['noise_prob']:
                p['sigma'] = float(np.random.uniform(a['noise_sigma'][0], a['noise_sigma'][1]))
            any_intensity = any_intensity or bool(p)
            intensity.append(p)
        seed = int(np.random.randint(0, 2 ** 63, dtype=np.int64)) if on['noise'] else 0
        return {'rotation': rotation, 'control': control, 'intensity': intensity if any_intensity else None, 'seed': seed}

    def sample_resolution_augmentation(self):
        """the random decisions of the blur / low-resolution simulation of the next sample, drawn after
        sample_augmentation -- after every other draw of the sample -- with numpy's global RNG in this fixed order; a
        transform that is off (validate_resolution_augmentation) draws NOTHING, so with the section absent or off the
        stream is what it was.  Per modality m = 0 .. M-1, each drawing independently:
          1. blur:    gate uniform() < blur_prob; if open, sigma = uniform(lo, hi) voxels
          2. lowres:  gate uniform() < lowres_prob; if open, zoom = uniform(lo, hi)
        -> dict(blur = list of M sigmas (0.0 = off for that modality) or None when no gate opened, lowres = list of M
        low-grid sizes (nx', ny', nz') (None = off for that modality) or None when no modality has a size below the
        crop's), or None without the section"""
        a = self.resolution_augmentation
        if a is None:
            return None
        on = a['enabled']
        size = tuple(int(v) for v in self.crop_size)
        sigmas, sizes = [], []
        for m in range(self._num_modality):
            sigma, low = 0.0, None
            if on['blur'] and np.random.uniform() < a['blur_prob']:
                sigma = float(np.random.uniform(a['blur_sigma_vox'][0], a['blur_sigma_vox'][1]))
            if on['lowres'] and np.random.uniform() < a['lowres_prob']:
                low = image_tools.lowres_sizes(size, float(np.random.uniform(a['lowres_zoom'][0], a['lowres_zoom'][1])))
                if low == size:
                    low = None
            sigmas.append(sigma)
            sizes.append(low)
        return {'blur': sigmas if any(s > 0.0 for s in sigmas) else None,
                'lowres': sizes if any(s is not None for s in sizes) else None}

    def _resolution_filters(self, res):
        """the out-of-place filters of one sample in their order -> list of callables (src, dst) -> dst"""
        filters = []
        if res is not None and res['blur'] is not None:
            filters.append(lambda src, dst, p=res['blur']: image_tools.blur_device(src, p, out=dst))
        if res is not None and res['lowres'] is not None:
            size = tuple(int(v) for v in self.crop_size)
            prm = image_tools.lowres_params(res['lowres'], self._num_modality, size)
            filters.append(lambda src, dst, p=prm: image_tools.lowres_device(src, p, out=dst))
        return filters

    # ---- the sample ---------------------------------------------------------------------------------------------------
    def __getitem__(self, index):
        """-> (image crop [M, z, y, x], mask crop [1, z, y, x] float labels, frame (15 floats), case name); device tensors.
        With random_mirror_axes image and mask are mirrored together inside their resampling launches (mirrored index
        map, no extra pass) and the frame describes the mirrored grid.
        With `augmentation` image and mask are rotated and elastically deformed together inside the same launches (one
        rotation and one control tensor for both, each with its own source frame) and the normalised image crop gets the
        intensity transforms in place; the frame stays the NOMINAL crop frame (un-rotated, un-deformed).
        With `resolution_augmentation` the normalised image crop is blurred and / or passed through the low-resolution
        simulation (out of place, one launch each for all modalities) before the intensity transforms; mask and frame
        are untouched.
        The image crop is a view of channels-last [z, y, x, M] memory (what the stem reads, without a copy)."""
        return self.sample(index)

    def sample(self, index, out=None):
        """__getitem__; `out` may be a contiguous [z, y, x, M] destination (a slot of an NDHWC batch) into which the crop
        is resampled (one launch for all modalities) and normalised in place (one launch)"""
        case = self.case(index)
        case_name = self.case_name(index)
        center, crop_spacing = self.sample_crop_geometry(index)
        mirror = self.sample_mirror()
        aug = self.sample_augmentation(crop_spacing)
        filters = self._resolution_filters(self.sample_resolution_augmentation())
        spatial = {}
        if aug is not None:
            # one small host-to-device copy on the current stream; nothing is read back
            deform = None if aug['control'] is None else (
                torch.from_numpy(aug['control']).to(self.device, non_blocking=True), self.augmentation['elastic_grid_mm'])
            spatial = {'rotation': aug['rotation'], 'deform': deform}
        # the k filters of this sample run out of place and the last one must write the destination, so the
        # resampling launch writes the destination for even k and a scratch buffer for odd k: no copy pass
        if filters:
            cz, cy, cx = (int(v) for v in self.crop_size[::-1])
            shape = (cz, cy, cx, self._num_modality)
            if out is None:
                out = torch.empty(shape, dtype=torch.float32, device=self.device)
            scratch = torch.empty(shape, dtype=torch.float32, device=self.device)
            first, other = (out, scratch) if len(filters) % 2 == 0 else (scratch, out)
        else:
            first = out
        # a staged case is uploaded here, on the current stream, and the two tensors die with this call: every launch
        # that reads them is queued by then, and the allocator hands the memory out again in stream order
        volume, seg_volume = case.tensors()
        im = image_tools.crop_image_device_mc(volume, case.frame, center, self.crop_size, crop_spacing,
                                              self.interpolation, out=first, mirror=mirror, prefiltered=True, **spatial)
        norm_params = self._norm_params if self._volume_normalizers is None else case.norm_params
        im = image_tools.normalize_crop_device_mc(im, norm_params, out=im)
        for f in filters:
            im, other = f(im, other), im
        if aug is not None and aug['intensity'] is not None:
            image_tools.augment_intensity_device(im, aug['intensity'], aug['seed'])
        im = im.permute(3, 0, 1, 2)
        seg = image_tools.crop_image_device(seg_volume, case.seg_frame, center, self.crop_size, crop_spacing,
                                            self.mask_interpolation, mirror=mirror, **spatial)
        origin = image_tools.crop_origin(center, self.crop_size, crop_spacing)
        direction = list(case.seg_frame[2])
        if any(mirror):
            _, origin, direction = image_tools.mirror_frame((crop_spacing, origin, direction), self.crop_size, mirror)
        frame = np.array(list(crop_spacing) + list(origin) + list(direction), dtype=np.float32)
        return im, seg.unsqueeze(0), frame, case_name


class DeviceCropLoader(object):
    """batches of device-resident samples in sampler order: iterable of (crops [B,M,z,y,x], masks [B,1,z,y,x], frames,
    case names).  Replaces torch's DataLoader + worker processes (core/seg_train.py:69-70) for the GPU data path."""

    def __init__(self, dataset, sampler, batch_size, drop_last=False):
        self.dataset, self.sampler, self.batch_size, self.drop_last = dataset, sampler, int(batch_size), drop_last

    def __len__(self):
        n = len(self.sampler)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        """every sample is resampled straight into slot b of a fresh [B, z, y, x, M] batch (no stack, no layout kernel);
        the batch is handed out as its [B, M, z, y, x] view"""
        M = self.dataset.num_modality()
        cz, cy, cx = (int(v) for v in self.dataset.crop_size[::-1])
        batch, segs, frames, names = None, [], [], []
        for index in self.sampler:
            if batch is None:
                batch = torch.empty((self.batch_size, cz, cy, cx, M), dtype=torch.float32, device=self.dataset.device)
            _, seg, frame, name = self.dataset.sample(index, out=batch[len(segs)])
            segs.append(seg)
            frames.append(frame)
            names.append(name)
            if len(segs) == self.batch_size:
                yield batch.permute(0, 4, 1, 2, 3), torch.stack(segs), np.stack(frames), names
                batch, segs, frames, names = None, [], [], []
        if segs and not self.drop_last:
            yield batch[:len(segs)].permute(0, 4, 1, 2, 3), torch.stack(segs), np.stack(frames), names


def collect_fixed_crops(dataset, crops_per_case, seed):
    """`crops_per_case` crops of every case of a SegmentationDataset, in case order: device tensors
    (crops [V, M, z, y, x], masks [V, 1, z, y, x]), V = len(dataset) * crops_per_case -- the fixed held-out set of the
    validation pass (core/seg_validate.py).  The dataset draws from numpy's GLOBAL stream, which the training run depends
    on: the state is saved, the stream seeded with `seed` for the draws, and the state restored whatever happens, so the
    caller's stream is exactly what it was and the same seed gives the same crops."""
    crops_per_case = int(crops_per_case)
    if crops_per_case < 1:
        raise ValueError('crops_per_case must be >= 1, got {}'.format(crops_per_case))
    state = np.random.get_state()
    crops, masks = [], []
    try:
        np.random.seed(int(seed))
        for index in range(len(dataset)):
            for _ in range(crops_per_case):
                sample = dataset[index]
                crops.append(sample[0].contiguous())
                masks.append(sample[1])
    finally:
        np.random.set_state(state)
    if not crops:
        raise ValueError('the data set has no cases')
    return torch.stack(crops), torch.stack(masks)


def intensity_fingerprint(imlist_file, percentiles=(0.5, 99.5), device=None, resident_bytes=8 << 30):
    """per-modality intensity statistics of a training list over the union of all cases' voxels under mask > 0 (nnU-Net's
    foreground intensity properties): the numbers of a ClipZScoreNormalizer for CT-like data.
    percentiles = (lo, hi) in percent: nearest-rank order statistics (utils.normalizer.nearest_rank) of the pooled
    foreground voxels; mean / population std are those of the values clamped to them.
    The statistics are accumulated on the device over the cases with the split entries of csrc/volume_stats.hip (four
    passes over the data set); cases stay resident up to `resident_bytes` in total and are re-read per pass beyond that.
    -> list of M dicts(n, min, max, mean, std, lower, upper, normalizer = ClipZScoreNormalizer).  The mask must have the
    image's size (ValueError naming the case otherwise)."""
    from segmentation3d.utils.normalizer import ClipZScoreNormalizer
    if imlist_file.endswith('txt'):
        im_list, seg_list = read_train_txt(imlist_file)
    elif imlist_file.endswith('csv'):
        im_list, seg_list = read_train_csv(imlist_file)
    else:
        raise ValueError('imseg_list must be a txt file')
    if not im_list:
        raise ValueError('the data set has no cases')
    lo, hi = (float(v) for v in percentiles)
    if not 0.0 <= lo < hi <= 100.0:
        raise ValueError('percentiles = {!r}: need 0 <= lo < hi <= 100'.format(tuple(percentiles)))
    device = device if device is not None else torch.device('cuda', torch.cuda.current_device())
    M = case_modalities(im_list[0])
    resident, used = {}, [0]

    def load(k):
        if k in resident:
            return resident[k]
        entry = im_list[k]
        first = entry if isinstance(entry, str) else entry[0]
        name = os.path.basename(os.path.dirname(first)) + '_' + os.path.basename(first)
        images = read_case_modalities(entry, name)
        if len(images) != M:
            raise ValueError('case {}: {} modalities, the first case has {}'.format(name, len(images), M))
        seg = read_image(seg_list[k], dtype=None)
        if tuple(seg.GetSize()) != tuple(images[0].GetSize()):
            raise ValueError('case {}: the mask has size {}, the image {}'.format(name, tuple(seg.GetSize()),
                                                                                 tuple(images[0].GetSize())))
        volume = image_tools.images_to_device(images, device).contiguous()
        sel = torch.from_numpy(np.ascontiguousarray(np.asarray(seg.array) > 0).astype(np.uint8)).to(device)
        nbytes = volume.numel() * 4 + sel.numel()
        if used[0] + nbytes <= resident_bytes:
            resident[k] = (volume, sel)
            used[0] += nbytes
        return volume, sel

    with torch.cuda.device(device):
        acc = image_tools.VolumeStatsAccumulator(M, 'mask', [lo / 100.0, hi / 100.0], True, device)
        for level in acc.levels():
            for k in range(len(im_list)):
                acc.add_hist(*load(k), level)
            acc.resolve(level)
        for k in range(len(im_list)):
            acc.add_moments(*load(k))
        stats = acc.finish()
    out = []
    for st in stats:
        if st['n'] == 0:
            raise ValueError('no voxel of the data set lies under mask > 0')
        out.append({'n': st['n'], 'min': st['min'], 'max': st['max'], 'mean': st['mean'], 'std': st['std'],
                    'lower': st['q'][0], 'upper': st['q'][1],
                    'normalizer': ClipZScoreNormalizer(st['mean'], st['std'], st['q'][0], st['q'][1])})
    return out
