"""GPU checks of the whole-volume statistics kernels (csrc/volume_stats.hip) against numpy: np.sort of the selected fp32
values and float64 moments.  n, min, max and every order statistic must be bit-equal (integers and selections: no
tolerance); float32(mean) and float32(std) must equal the float64 oracle rounded to fp32 or lie one fp32 ulp from it (the
fp64 accumulation error at these n is below 1e-10 relative, so only an oracle value next to a rounding boundary can move,
and then by one ulp)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(7, 5, 3), (33, 17, 9), (64, 40, 24)]
WIDTHS = [1, 2, 3, 4, 5, 8]
MODES = ['all', 'nonzero', 'mask']
QSETS = [(), (0.5,), (0.005, 0.995), (0.0, 0.005, 0.5, 1.0), (0.995, 0.5, 0.5, 1.0)]   # the last: a duplicated q


def _data(kind, shape, M, seed):
    rng = np.random.RandomState(seed)
    full = tuple(shape) + (M,)
    if kind == 'uniform':
        a = rng.uniform(-1.0, 1.0, size=full).astype(np.float32)
        a[rng.uniform(size=full) < 0.1] = 0.0
    elif kind == 'ct':       # integer-valued, 60 % of the voxels at one value: heavy ties at every radix level
        a = rng.randint(-1000, 3001, size=full).astype(np.float32)
        a[rng.uniform(size=full) < 0.6] = -1000.0
    elif kind == 'equal':
        a = np.full(full, 1000.25, dtype=np.float32)
    elif kind == 'tiny':     # +0.0 / -0.0 / +-tiny with denormals
        vals = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-40, 1.2e-38, -1.2e-38, 3e-38], dtype=np.float32)
        a = vals[rng.randint(0, vals.size, size=full)]
    else:
        raise AssertionError(kind)
    sel = (rng.uniform(size=shape) < 0.4).astype(np.uint8)
    return a, sel


def _oracle(a, sel, mode, quantiles, clip):
    """per modality: np.sort of the selected fp32 values, float64 moments"""
    rows = []
    for m in range(a.shape[-1]):
        x = a[..., m].ravel()
        if mode == 'nonzero':
            x = x[x != 0]
        elif mode == 'mask':
            x = x[sel.ravel() != 0]
        n = int(x.size)
        if n == 0:
            rows.append({'n': 0, 'min': 0.0, 'max': 0.0, 'mean': 0.0, 'std': 1e-6, 'q': [0.0] * len(quantiles)})
            continue
        s = np.sort(x) + np.float32(0.0)          # -0.0 is reported as +0.0
        q = [s[int(math.floor(qq * (n - 1) + 0.5))] for qq in quantiles]
        v = s.astype(np.float64)
        if clip:
            v = np.clip(v, float(q[0]), float(q[1]))
        rows.append({'n': n, 'min': float(s[0]), 'max': float(s[-1]), 'mean': float(v.mean()),
                     'std': max(float(v.std()), 1e-6), 'q': [float(t) for t in q]})
    return rows


def _bits64(x):
    return np.float64(x).view(np.int64).item()


def _ulps32(a, b):
    """distance in fp32 ulps between float32(a) and float32(b)"""
    def key(x):
        i = int(np.float32(x).view(np.int32))
        return i if i >= 0 else -(i & 0x7fffffff)
    return abs(key(a) - key(b))


def _check(got, want, what):
    assert len(got) == len(want)
    for m, (g, w) in enumerate(zip(got, want)):
        tag = '{} modality {}'.format(what, m)
        assert g['n'] == w['n'], tag
        for k in ('min', 'max'):
            assert _bits64(g[k]) == _bits64(w[k]), (tag, k, g[k], w[k])
        assert len(g['q']) == len(w['q'])
        for i, (a, b) in enumerate(zip(g['q'], w['q'])):
            assert _bits64(a) == _bits64(b), (tag, 'q', i, a, b)
        print('{}: mean {!r} vs {!r} ({} ulp), std {!r} vs {!r} ({} ulp)'.format(
            tag, g['mean'], w['mean'], _ulps32(g['mean'], w['mean']), g['std'], w['std'], _ulps32(g['std'], w['std'])))
        assert _ulps32(g['mean'], w['mean']) <= 1, (tag, 'mean', g['mean'], w['mean'])
        assert _ulps32(g['std'], w['std']) <= 1, (tag, 'std', g['std'], w['std'])


def _run(a, sel, mode, quantiles, clip, device):
    from segmentation3d.utils.image_tools import volume_stats_device
    vol = torch.from_numpy(a).to(device)
    s = torch.from_numpy(sel).to(device) if mode == 'mask' else None
    return volume_stats_device(vol, mode, sel=s, quantiles=quantiles, clip=clip)


@pytest.mark.parametrize('M', WIDTHS)
@pytest.mark.parametrize('shape', SHAPES)
def test_matches_numpy(hip_device, shape, M):
    """every shape and width, both data sets, every mode; the rank sets rotate over the combinations"""
    k = SHAPES.index(shape) + WIDTHS.index(M)
    for kind in ('uniform', 'ct'):
        a, sel = _data(kind, shape, M, 100 + k)
        for j, mode in enumerate(MODES):
            quantiles = QSETS[(k + j + (kind == 'ct')) % len(QSETS)]
            clip = len(quantiles) >= 2 and quantiles[0] <= quantiles[1] and (k + j) % 2 == 0
            got = _run(a, sel, mode, quantiles, clip, hip_device)
            _check(got, _oracle(a, sel, mode, quantiles, clip), '{} {} {} {} clip={}'.format(kind, shape, mode, quantiles, clip))


@pytest.mark.parametrize('quantiles', QSETS)
@pytest.mark.parametrize('clip', [False, True])
def test_rank_sets_with_and_without_clamp(hip_device, quantiles, clip):
    if clip and (len(quantiles) < 2 or quantiles[0] > quantiles[1]):
        from segmentation3d.utils.image_tools import volume_stats_device
        with pytest.raises(ValueError):
            volume_stats_device(torch.zeros((2, 2, 2, 1), device=hip_device), 'all', quantiles=quantiles, clip=True)
        return
    for kind, M in (('ct', 4), ('uniform', 3)):
        a, sel = _data(kind, (33, 17, 9), M, 7)
        for mode in MODES:
            _check(_run(a, sel, mode, quantiles, clip, hip_device), _oracle(a, sel, mode, quantiles, clip),
                   '{} {} {}'.format(kind, mode, quantiles))


@pytest.mark.parametrize('kind', ['equal', 'tiny'])
@pytest.mark.parametrize('M', [1, 4, 5])
def test_degenerate_values(hip_device, kind, M):
    a, sel = _data(kind, (33, 17, 9), M, 11)
    for mode in MODES:
        for quantiles, clip in (((0.005, 0.5, 0.995, 1.0), True), ((), False)):
            want = _oracle(a, sel, mode, quantiles, clip)
            got = _run(a, sel, mode, quantiles, clip, hip_device)
            _check(got, want, '{} {}'.format(kind, mode))
            if kind == 'equal':
                assert all(g['std'] == 1e-6 and g['mean'] == 1000.25 for g in got)
    if kind == 'tiny':       # the zeros of either sign are out of the non-zero selection, the denormals are in
        n = _run(a, sel, 'nonzero', (), False, hip_device)[0]['n']
        assert n == int((a[..., 0].view(np.int32) & 0x7fffffff != 0).sum()) and 0 < n < a[..., 0].size


@pytest.mark.parametrize('M', [1, 3, 4, 8])
def test_empty_selection(hip_device, M):
    zero = {'n': 0, 'min': 0.0, 'max': 0.0, 'mean': 0.0, 'std': 1e-6, 'q': [0.0, 0.0]}
    a = np.zeros((7, 5, 3, M), dtype=np.float32)
    a[::2] = -0.0
    assert _run(a, None, 'nonzero', (0.25, 0.75), True, hip_device) == [zero] * M
    b, _ = _data('uniform', (7, 5, 3), M, 5)
    assert _run(b, np.zeros((7, 5, 3), np.uint8), 'mask', (0.25, 0.75), False, hip_device) == [zero] * M
    if M > 1:                # one modality empty, the others not
        b[..., 1] = 0.0
        got = _run(b, None, 'nonzero', (0.25, 0.75), True, hip_device)
        assert got[1] == zero
        _check(got, _oracle(b, None, 'nonzero', (0.25, 0.75), True), 'one empty modality')


@pytest.mark.parametrize('M', [4, 2])
def test_unaligned_view_takes_the_scalar_path_and_agrees(hip_device, M):
    """a base that is not 16- (M = 4) / 8-byte (M = 2) aligned: scalar row loads, the same numbers bit for bit"""
    from segmentation3d.utils.image_tools import volume_stats_device
    shape = (33, 17, 9)
    a, sel = _data('ct', shape, M, 21)
    buf = torch.empty((a.size + 1,), dtype=torch.float32, device=hip_device)
    view = buf[1:].view(*a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and view.data_ptr() % (4 * M) == 4
    aligned = torch.from_numpy(a).to(hip_device)
    assert aligned.data_ptr() % 16 == 0
    s = torch.from_numpy(sel).to(hip_device)
    for mode in MODES:
        kw = dict(sel=s if mode == 'mask' else None, quantiles=(0.005, 0.5, 0.995), clip=True)
        got = volume_stats_device(view, mode, **kw)
        assert got == volume_stats_device(aligned, mode, **kw)
        _check(got, _oracle(a, sel, mode, (0.005, 0.5, 0.995), True), 'unaligned ' + mode)


def test_two_runs_are_bit_equal(hip_device):
    for kind, M in (('uniform', 4), ('ct', 5)):
        a, sel = _data(kind, (64, 40, 24), M, 33)
        first = _run(a, sel, 'nonzero', (0.005, 0.5, 0.995, 1.0), True, hip_device)
        for _ in range(2):
            again = _run(a, sel, 'nonzero', (0.005, 0.5, 0.995, 1.0), True, hip_device)
            for g, w in zip(again, first):
                assert all(_bits64(g[k]) == _bits64(w[k]) for k in ('min', 'max', 'mean', 'std')) and g == w


@pytest.mark.parametrize('M', [1, 3, 4])
def test_split_accumulation_equals_the_concatenation(hip_device, M):
    """three volumes of different shapes through the split entries == one call on their concatenation, bit for bit in the
    integers and order statistics; the moments keep the 1-ulp rule against the oracle of the concatenation"""
    from segmentation3d.utils.image_tools import VolumeStatsAccumulator, volume_stats_device
    quantiles = (0.005, 0.995, 0.5)
    parts = [_data(kind, shape, M, 40 + i) for i, (kind, shape) in
             enumerate((('ct', (7, 5, 3)), ('uniform', (33, 17, 9)), ('ct', (64, 40, 24))))]
    vols = [(torch.from_numpy(a).to(hip_device), torch.from_numpy(s).to(hip_device)) for a, s in parts]
    cat = np.concatenate([a.reshape(-1, 1, 1, M) for a, _ in parts])
    cat_sel = np.concatenate([s.reshape(-1, 1, 1) for _, s in parts])
    for mode in MODES:
        acc = VolumeStatsAccumulator(M, mode, quantiles, True, hip_device)
        for level in acc.levels():
            for v, s in vols:
                acc.add_hist(v, s, level)
            acc.resolve(level)
        for v, s in vols:
            acc.add_moments(v, s)
        got = acc.finish()
        one = volume_stats_device(torch.from_numpy(cat).to(hip_device), mode, sel=torch.from_numpy(cat_sel).to(hip_device),
                                  quantiles=quantiles, clip=True)
        for g, w in zip(got, one):
            assert g['n'] == w['n'] and all(_bits64(g[k]) == _bits64(w[k]) for k in ('min', 'max'))
            assert [_bits64(t) for t in g['q']] == [_bits64(t) for t in w['q']]
        want = _oracle(cat, cat_sel, mode, quantiles, True)
        _check(got, want, 'split ' + mode)
        _check(one, want, 'concatenated ' + mode)


def test_argument_checks(hip_device):
    from segmentation3d.utils.image_tools import volume_stats_device
    v = torch.zeros((4, 4, 4, 2), device=hip_device)
    with pytest.raises(ValueError):
        volume_stats_device(v, 'foreground')
    with pytest.raises(ValueError):
        volume_stats_device(v, 'mask')                                  # no selection plane
    with pytest.raises(ValueError):
        volume_stats_device(v, 'mask', sel=torch.zeros((4, 4, 3), dtype=torch.uint8, device=hip_device))
    with pytest.raises(ValueError):
        volume_stats_device(v, 'all', quantiles=(0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError):
        volume_stats_device(v, 'all', quantiles=(1.5,))
    with pytest.raises(ValueError):
        volume_stats_device(torch.zeros((4, 4, 4, 9), device=hip_device), 'all')
    with pytest.raises(ValueError):
        volume_stats_device(v.permute(3, 0, 1, 2), 'all')


def test_clip_identity_through_the_normalise_kernel(hip_device):
    """a type-3 struct through the existing gather / normalise kernel == numpy fp32 (clip(x, lo, hi) - mean) / std bit for
    bit: the bounds f(lo), f(hi) are rounded as the kernel rounds them"""
    from segmentation3d.utils.image_tools import normalize_crop_device_mc, normalizer_params
    from segmentation3d.utils.normalizer import ClipZScoreNormalizer
    rng = np.random.RandomState(3)
    x = (rng.normal(size=(9, 17, 33, 3)) * np.array([3.0, 400.0, 1e-3])).astype(np.float32)
    norms = [ClipZScoreNormalizer(0.1234567, 0.789, -2.7182818, 3.1415927),
             ClipZScoreNormalizer(-213.7, 391.3, -1000.0, 517.25),
             ClipZScoreNormalizer(1.1e-4, 9.7e-4, None, 1.3e-3)]
    x[0, 0, :6, 0] = np.array([-2.7182818, 3.1415927, np.nextafter(np.float32(-2.7182818), np.float32(0)),
                               np.nextafter(np.float32(3.1415927), np.float32(9)), -50.0, 50.0], dtype=np.float32)
    got = normalize_crop_device_mc(torch.from_numpy(x).to(hip_device), normalizer_params(norms, 3)).cpu().numpy()
    for m, n in enumerate(norms):
        lo = np.float32(-np.inf) if n.lower is None else np.float32(n.lower)
        hi = np.float32(np.inf) if n.upper is None else np.float32(n.upper)
        want = (np.clip(x[..., m], lo, hi) - np.float32(n.mean)) / np.float32(n.stddev)
        assert want.dtype == np.float32
        assert np.array_equal(got[..., m].view(np.int32), want.view(np.int32)), m
