"""Crop intensity normalisers with the reference's names, parameters and checkpoint dictionaries
(utils/normalizer.py:6-81).  At inference they are applied on the device by the patch batcher
(seg3d_patch_gather_normalize); the numpy `__call__` here is host glue for the training data path and for tests.
Beyond the reference (whose loader rejects them): VolumeNormalizer (type 2, the statistics of the whole volume per case
and modality) and ClipZScoreNormalizer (type 3, fixed numbers with raw clip bounds); DESIGN.md section 7 row f20.
"""
import numpy as np

from segmentation3d.utils.image3d import Image3d


def _apply(image, fn):
    if isinstance(image, Image3d):
        return image.like(fn(image.array))
    if isinstance(image, np.ndarray):
        return fn(image)
    if isinstance(image, (list, tuple)):
        for idx, im in enumerate(image):
            image[idx] = _apply(im, fn)
        return image
    raise ValueError('Unknown type of input. Normalizer only supports Image3d or Image3d list/tuple')


class FixedNormalizer(object):
    """intensity = (intensity - mean) / stddev, clipped to [-1, 1] when clip is enabled (type 0)"""

    def __init__(self, mean, stddev, clip=True):
        assert stddev > 0, 'stddev must be positive'
        assert isinstance(clip, bool), 'clip must be a boolean'
        self.mean, self.stddev, self.clip = mean, stddev, clip

    def __call__(self, image):
        def fn(a):
            out = ((a - self.mean) / self.stddev).astype(a.dtype)
            return np.clip(out, -1.0, 1.0) if self.clip else out
        return _apply(image, fn)

    def to_dict(self):
        return {'type': 0, 'mean': self.mean, 'stddev': self.stddev, 'clip': self.clip}


class AdaptiveNormalizer(object):
    """z-score with the crop's own mean / population std (floored at 1e-6), clipped to +-clip_sigma (type 1)"""

    def __init__(self, clip_sigma=3):
        assert clip_sigma > 0
        self.clip_sigma = clip_sigma

    def __call__(self, image):
        def fn(a):
            mean, std = np.mean(a), max(np.std(a), 1e-6)
            return np.clip(((a - mean) / std).astype(a.dtype), -self.clip_sigma, self.clip_sigma)
        return _apply(image, fn)

    def to_dict(self):
        return {'type': 1, 'clip_sigma': self.clip_sigma}


def nearest_rank(q, n):
    """index k = floor(q (n - 1) + 0.5) into the n sorted values: the nearest rank of the quantile q in [0, 1].  The device
    statistics (csrc/volume_stats.hip) use the same rule; it differs from numpy's linearly interpolated percentile by less
    than the gap between two neighbouring order statistics"""
    q, n = float(q), int(n)
    if not 0.0 <= q <= 1.0:
        raise ValueError('quantile {} not in [0, 1]'.format(q))
    if n < 1:
        raise ValueError('nearest_rank needs n >= 1, got {}'.format(n))
    return min(max(int(np.floor(q * (n - 1) + 0.5)), 0), n - 1)


def _number(name, v):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError('{} must be a number, got {!r}'.format(name, v))
    if isinstance(v, bool) or not np.isfinite(f):
        raise ValueError('{} must be a finite number, got {!r}'.format(name, v))
    return f


def host_volume_stats(a, foreground='nonzero', quantiles=(), clip=False):
    """the statistics of csrc/volume_stats.hip restated on the host for ONE modality: sort-based, float64.  a: array of any
    shape (taken as float32); foreground 'all' | 'nonzero' (x != 0).  -> dict(n, min, max, mean, std, q = [order statistics
    at the nearest ranks of `quantiles`]); clip: the moments are those of the values clamped to [q[0], q[1]].  n == 0: all
    0 and std = 1e-6."""
    x = np.asarray(a, dtype=np.float32).ravel()
    if foreground == 'nonzero':
        x = x[x != 0]
    elif foreground != 'all':
        raise ValueError("foreground must be 'all' or 'nonzero', got {!r}".format(foreground))
    quantiles = [float(q) for q in quantiles]
    if clip and (len(quantiles) < 2 or quantiles[0] > quantiles[1]):
        raise ValueError('the clamp needs two quantiles q0 <= q1')
    n = int(x.size)
    if n == 0:
        return {'n': 0, 'min': 0.0, 'max': 0.0, 'mean': 0.0, 'std': 1e-6, 'q': [0.0] * len(quantiles)}
    s = np.sort(x) + np.float32(0.0)                      # -0.0 -> +0.0
    qv = [float(s[nearest_rank(q, n)]) for q in quantiles]
    v = s.astype(np.float64)
    if clip:
        v = np.clip(v, qv[0], qv[1])
    return {'n': n, 'min': float(s[0]), 'max': float(s[-1]), 'mean': float(np.mean(v)), 'std': max(float(np.std(v)), 1e-6),
            'q': qv}


class ClipZScoreNormalizer(object):
    """fixed numbers (type 3): raw values are clipped to [lower, upper] (None: open on that side), then
    (x - mean) / stddev.  The CT rule with a data set's foreground percentiles and moments
    (dataloader.dataset.intensity_fingerprint prints them); also what a VolumeNormalizer resolves to for one case."""

    def __init__(self, mean, stddev, lower=None, upper=None):
        self.mean, self.stddev = _number('mean', mean), _number('stddev', stddev)
        if not self.stddev > 0.0:
            raise ValueError('stddev must be positive, got {!r}'.format(stddev))
        self.lower = None if lower is None else _number('lower', lower)
        self.upper = None if upper is None else _number('upper', upper)
        if self.lower is not None and self.upper is not None and not self.lower <= self.upper:
            raise ValueError('lower {} exceeds upper {}'.format(self.lower, self.upper))

    def __call__(self, image):
        def fn(a):
            v = np.asarray(a, dtype=np.float64)
            if self.lower is not None or self.upper is not None:
                v = np.clip(v, self.lower, self.upper)
            return ((v - self.mean) / self.stddev).astype(a.dtype)
        return _apply(image, fn)

    def to_dict(self):
        return {'type': 3, 'mean': self.mean, 'stddev': self.stddev, 'lower': self.lower, 'upper': self.upper}


class VolumeNormalizer(object):
    """z-score with the statistics of the WHOLE volume, per case and modality (type 2).
    foreground 'nonzero': mean / population std (floored at 1e-6) over the voxels x != 0 -- the MRI rule; 'all': over every
    voxel.  A case without a non-zero voxel falls back to 'all'.  clip_percentiles = (lo, hi) in percent: raw values are
    first clipped to the order statistics at the nearest ranks (nearest_rank) of lo / 100 and hi / 100 of the selected
    voxels, and the moments are those of the clipped values.  clip_sigma: the z-score is additionally clipped to
    +-clip_sigma.  Every voxel of the volume is normalised, selected or not.
    On the device the statistics come from csrc/volume_stats.hip (image_tools.resolve_normalizers); __call__ restates the
    rule on the host for one whole image: sort-based, float64."""

    def __init__(self, foreground='nonzero', clip_percentiles=None, clip_sigma=None):
        if foreground not in ('nonzero', 'all'):
            raise ValueError("foreground must be 'nonzero' or 'all', got {!r}".format(foreground))
        self.foreground = foreground
        if clip_percentiles is not None:
            try:
                lo, hi = clip_percentiles
            except (TypeError, ValueError):
                raise ValueError('clip_percentiles must be a (lo, hi) pair, got {!r}'.format(clip_percentiles))
            lo, hi = _number('clip_percentiles[0]', lo), _number('clip_percentiles[1]', hi)
            if not 0.0 <= lo < hi <= 100.0:
                raise ValueError('clip_percentiles = {!r}: need 0 <= lo < hi <= 100'.format(clip_percentiles))
            clip_percentiles = [lo, hi]
        self.clip_percentiles = clip_percentiles
        if clip_sigma is not None:
            clip_sigma = _number('clip_sigma', clip_sigma)
            if not clip_sigma > 0.0:
                raise ValueError('clip_sigma must be positive, got {!r}'.format(clip_sigma))
        self.clip_sigma = clip_sigma

    def __call__(self, image):
        def fn(a):
            q = [] if self.clip_percentiles is None else [p / 100.0 for p in self.clip_percentiles]
            st = host_volume_stats(a, self.foreground, q, clip=bool(q))
            if st['n'] == 0 and self.foreground != 'all':
                st = host_volume_stats(a, 'all', q, clip=bool(q))
            return resolved_normalizer(self.to_dict(), st)(a)
        return _apply(image, fn)

    def to_dict(self):
        return {'type': 2, 'foreground': self.foreground, 'clip_percentiles': self.clip_percentiles,
                'clip_sigma': self.clip_sigma}


def resolved_normalizer(d, stats):
    """a type-2 dict + the statistics of one modality of one volume (host_volume_stats / image_tools.volume_stats_device,
    taken with the dict's foreground and percentiles) -> the ClipZScoreNormalizer of that volume.  Raw bounds: the clip
    percentiles' order statistics (if any), narrowed by mean +- clip_sigma * std (if any) -- clipping the z-score to
    +-sigma is clipping the raw value to that interval."""
    mean, std = float(stats['mean']), float(stats['std'])
    lower = upper = None
    if d.get('clip_percentiles') is not None:
        lower, upper = float(stats['q'][0]), float(stats['q'][1])
    if d.get('clip_sigma') is not None:
        s = float(d['clip_sigma'])
        lower = mean - s * std if lower is None else max(lower, mean - s * std)
        upper = mean + s * std if upper is None else min(upper, mean + s * std)   # (the mean lies inside both windows)
    return ClipZScoreNormalizer(mean, std, lower, upper)


def normalizer_from_dict(d):
    """inverse of to_dict(); raises like core/seg_infer.py:151-162"""
    if d['type'] == 0:
        return FixedNormalizer(d['mean'], d['stddev'], d['clip'])
    if d['type'] == 1:
        return AdaptiveNormalizer(d['clip_sigma'])
    if d['type'] == 2:
        return VolumeNormalizer(d.get('foreground', 'nonzero'), d.get('clip_percentiles'), d.get('clip_sigma'))
    if d['type'] == 3:
        return ClipZScoreNormalizer(d['mean'], d['stddev'], d.get('lower'), d.get('upper'))
    raise ValueError('Unsupported normalization type.')
