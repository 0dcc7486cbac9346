"""Host side of Gaussian patch blending and mirror test-time augmentation: weight tables,
flip-set enumeration, config keys, CLI flags and the mirror augmentation of the training data set.  Nothing of this is
in the reference, so the definitions are restated here in numpy (the oracle) and the product is compared with them.
The oracle helpers are shared with tests/test_gpu_blend_tta.py."""
import os

import numpy as np
import pytest
import torch

from conftest import PKG


# ---------------------------------------------------------------------------------------------------------------------
# numpy oracle, written from the definitions
# ---------------------------------------------------------------------------------------------------------------------
def oracle_table(n, s):
    g = np.empty(n, np.float64)
    for i in range(n):
        g[i] = np.exp(-0.5 * ((i - (n - 1) / 2.0) / (s * n)) ** 2)
    return g.astype(np.float32)


def oracle_tables(box, s=0.125):
    return oracle_table(box[0], s), oracle_table(box[1], s), oracle_table(box[2], s)


def oracle_weight(box, s=0.125, blend='gaussian'):
    """float32 [bz, by, bx]: (g_z * g_y) * g_x, two rounded float32 multiplies in that order"""
    bx, by, bz = box
    if blend == 'constant':
        return np.ones((bz, by, bx), np.float32)
    gx, gy, gz = oracle_tables(box, s)
    zy = (gz[:, None] * gy[None, :]).astype(np.float32)
    return (zy[:, :, None] * gx[None, None, :]).astype(np.float32)


def oracle_flip_set(axes):
    bits = 0
    for a in axes:
        bits |= {'x': 1, 'y': 2, 'z': 4}[a]
    return [m for m in range(8) if (m | bits) == bits]


def oracle_flip(a, mask):
    """mirror the last three axes [z, y, x] of an array by a flip mask (bit 0 = x, 1 = y, 2 = z)"""
    ax = [a.ndim - 1 - b for b in range(3) if mask >> b & 1]
    return np.flip(a, ax) if ax else a


def oracle_accumulate(acc, cnt, start, box, probs, w):
    """acc[c] += w * probs[c]; cnt += w over the patch region, float32: a rounded multiply, then a rounded add"""
    bx, by, bz = box
    sl = (slice(start[2], start[2] + bz), slice(start[1], start[1] + by), slice(start[0], start[0] + bx))
    for c in range(acc.shape[0]):
        wp = (w * probs[c]).astype(np.float32)
        acc[c][sl] = (acc[c][sl] + wp).astype(np.float32)
    cnt[sl] = (cnt[sl] + w).astype(np.float32)


def oracle_finalize(acc, cnt):
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(cnt > 0, np.float32(1.0) / cnt, np.float32(0.0)).astype(np.float32)
    probs = (acc * r[None]).astype(np.float32)
    return probs, probs.argmax(0).astype(np.int8)


def oracle_sliding_window(patch_fn, net_fn, shape_zyx, starts, box, C, batch, axes, blend='gaussian', s=0.125):
    """the contract's loop: per batch, per flip of the flip set in order, per patch in list order.
    patch_fn(k) -> un-mirrored normalised patch [M, bz, by, bx]; net_fn([n, M, bz, by, bx]) -> [n, C, bz, by, bx]"""
    Z, Y, X = shape_zyx
    acc = np.zeros((C, Z, Y, X), np.float32)
    cnt = np.zeros((Z, Y, X), np.float32)
    w = oracle_weight(box, s, blend)
    for i in range(0, len(starts), batch):
        idx = list(range(i, min(i + batch, len(starts))))
        plain = np.stack([patch_fn(k) for k in idx])
        for f in oracle_flip_set(axes):
            out = net_fn(np.ascontiguousarray(oracle_flip(plain, f)))
            back = oracle_flip(out, f)
            for j, k in enumerate(idx):
                oracle_accumulate(acc, cnt, starts[k], box, back[j], w)
    return acc, cnt


# ---------------------------------------------------------------------------------------------------------------------
# weight tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('box', [(96, 96, 96), (32, 48, 16), (16, 16, 16)])
def test_weight_tables_equal_the_oracle_and_are_symmetric(box):
    from segmentation3d.core.seg_infer import blend_weight_tables
    got = blend_weight_tables(box, 0.125)
    want = oracle_tables(box, 0.125)
    assert len(got) == 3
    for g, w, n in zip(got, want, box):
        assert g.dtype == np.float32 and g.shape == (n,)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
        assert np.array_equal(g, g[::-1])
        assert g.max() <= 1.0 and g.min() > 0.0
    assert np.array_equal(blend_weight_tables(box)[0], got[0])            # default sigma_scale = 0.125


def test_corner_weights_named_in_the_contract():
    c96 = float(np.prod([t.min() for t in oracle_tables((96, 96, 96))], dtype=np.float64))
    c16 = float(np.prod([t.min() for t in oracle_tables((16, 16, 16))], dtype=np.float64))
    assert 5e-11 < c96 < 7e-11 and 6e-10 < c16 < 8e-10
    assert 1e-33 < float(np.prod([t.astype(np.float64).min() for t in oracle_tables((96, 96, 96), 0.07)])) < 1e-32
    assert float(np.prod([t.astype(np.float64).min() for t in oracle_tables((96, 96, 96), 0.02)])) == 0.0


@pytest.mark.parametrize('s', [0.0, -0.125, float('nan'), float('inf'), 0.07, 0.02])
def test_weight_tables_refuse_bad_sigma(s):
    from segmentation3d.core.seg_infer import blend_weight_tables
    with pytest.raises(ValueError):
        blend_weight_tables((96, 96, 96), s)


def test_weight_tables_accept_wide_sigma():
    from segmentation3d.core.seg_infer import blend_weight_tables
    for s in (0.08, 0.25, 1.0):
        g = blend_weight_tables((96, 96, 96), s)
        assert np.array_equal(g[2].view(np.uint32), oracle_table(96, s).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# flip set
# ---------------------------------------------------------------------------------------------------------------------
def test_flip_set_enumeration():
    from segmentation3d.core.seg_infer import mirror_flip_masks
    assert mirror_flip_masks(()) == [0]
    assert mirror_flip_masks(('x',)) == [0, 1]
    assert mirror_flip_masks(('z', 'x')) == [0, 1, 4, 5]
    assert mirror_flip_masks(('x', 'y', 'z')) == list(range(8))
    assert mirror_flip_masks(['y']) == [0, 2]
    assert mirror_flip_masks('xy') == [0, 1, 2, 3]
    assert mirror_flip_masks(('x', 'x')) == [0, 1]
    for axes in ((), ('x',), ('z', 'x'), ('y', 'z'), ('x', 'y', 'z')):
        assert mirror_flip_masks(axes) == oracle_flip_set(axes)
    with pytest.raises(ValueError, match='w'):
        mirror_flip_masks(('w',))
    with pytest.raises(ValueError):
        mirror_flip_masks(('x', 3))


def test_oracle_flip_is_an_involution_on_the_right_axes():
    a = np.arange(2 * 3 * 4 * 5).reshape(2, 3, 4, 5)
    assert np.array_equal(oracle_flip(a, 1), a[:, :, :, ::-1])
    assert np.array_equal(oracle_flip(a, 2), a[:, :, ::-1])
    assert np.array_equal(oracle_flip(a, 4), a[:, ::-1])
    assert np.array_equal(oracle_flip(oracle_flip(a, 5), 5), a)


def test_oracle_detects_a_wrong_unmirror():
    """the pipeline check of the GPU suite rests on this: with a position-dependent net the oracle's result changes when
    the outputs are not mirrored back (which is also what mirroring the symmetric weight instead of the data amounts to),
    while a mirror-equivariant net would hide that mistake"""
    rng = np.random.RandomState(3)
    box, shape, C = (8, 6, 4), (4, 6, 12), 2
    starts = [[0, 0, 0], [4, 0, 0]]
    vol = rng.randn(*shape).astype(np.float32)
    ramp = rng.rand(C, 4, 6, 8).astype(np.float32)

    def patch_fn(k):
        s = starts[k]
        return vol[None, s[2]:s[2] + 4, s[1]:s[1] + 6, s[0]:s[0] + 8]

    def net_fn(x):
        e = np.exp(x * ramp[None])
        return (e / e.sum(1, keepdims=True)).astype(np.float32)
    good, cnt = oracle_sliding_window(patch_fn, net_fn, shape, starts, box, C, 2, ('x',))
    # wrong: outputs accumulated without the un-mirror
    acc = np.zeros_like(good)
    c2 = np.zeros_like(cnt)
    w = oracle_weight(box)
    plain = np.stack([patch_fn(0), patch_fn(1)])
    for f in (0, 1):
        out = net_fn(np.ascontiguousarray(oracle_flip(plain, f)))
        for j in range(2):
            oracle_accumulate(acc, c2, starts[j], box, out[j], w)
    assert np.array_equal(c2, cnt) and np.abs(acc - good).max() > 1e-3
    # an equivariant net would hide the mistake: the ramp is what makes the check bite
    def eq_net(x):
        e = np.exp(x * np.array([1.0, 2.0], np.float32)[None, :, None, None, None])
        return (e / e.sum(1, keepdims=True)).astype(np.float32)
    a1, _ = oracle_sliding_window(patch_fn, eq_net, shape, starts, box, C, 2, ('x',))
    a0, _ = oracle_sliding_window(patch_fn, eq_net, shape, starts, box, C, 2, ())
    assert np.abs(a1 - 2 * a0).max() < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# config keys and CLI
# ---------------------------------------------------------------------------------------------------------------------
class _Stage(object):
    partition_type = 'SIZE'
    partition_size = [32, 32, 32]
    partition_stride = [16, 16, 16]


def test_stage_config_defaults_and_values():
    from segmentation3d.core.seg_infer import blend_options, _Model as edict      # attribute dict: missing keys read None
    assert blend_options(_Stage) == ('constant', 0.125, ())
    assert blend_options(edict({'partition_type': 'SIZE'})) == ('constant', 0.125, ())

    class Full(_Stage):
        blend_mode = 'gaussian'
        blend_sigma_scale = 0.25
        tta_mirror_axes = ['x', 'y']
    assert blend_options(Full) == ('gaussian', 0.25, ('x', 'y'))
    assert blend_options(edict({'blend_mode': 'gaussian', 'tta_mirror_axes': ['z']})) == ('gaussian', 0.125, ('z',))

    class BadMode(_Stage):
        blend_mode = 'hann'
    with pytest.raises(ValueError, match='hann'):
        blend_options(BadMode)

    class BadAxis(_Stage):
        tta_mirror_axes = ['x', 'w']
    with pytest.raises(ValueError, match='w'):
        blend_options(BadAxis)


def test_shipped_configs():
    import segmentation3d
    from segmentation3d.core.seg_infer import blend_options
    from segmentation3d.utils.file_io import load_config
    folder = os.path.join(os.path.dirname(segmentation3d.__file__), 'config')
    ic = load_config(os.path.join(folder, 'infer_config.py'))
    for section in ('coarse', 'fine'):
        keys = set(ic[section].keys())
        assert not keys & {'blend_mode', 'blend_sigma_scale', 'tta_mirror_axes'}      # optional: named in a comment only
        assert blend_options(ic[section]) == ('constant', 0.125, ())
    text = open(os.path.join(folder, 'infer_config.py')).read()
    for key in ('blend_mode', 'blend_sigma_scale', 'tta_mirror_axes'):
        assert key in text
    tc = load_config(os.path.join(folder, 'train_config.py'))
    assert tc.dataset.random_mirror_axes == []


def test_cli_flags():
    from segmentation3d.seg_infer import build_parser
    base = ['-i', 'a.mha', '-m', 'model', '-o', 'out']
    args = build_parser().parse_args(base)
    assert args.blend is None and args.tta_mirror is None
    args = build_parser().parse_args(base + ['--blend', 'gaussian', '--tta_mirror', 'xy'])
    assert args.blend == 'gaussian' and args.tta_mirror == 'xy'
    assert build_parser().parse_args(base + ['--tta_mirror', '']).tta_mirror == ''
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ['--blend', 'hann'])


def test_segmentation_refuses_unknown_mode_and_axis(tmp_path):
    from segmentation3d.core.seg_infer import segmentation
    with pytest.raises(ValueError, match='hann'):
        segmentation('a.mha', str(tmp_path), str(tmp_path), 'seg.mha', 0, False, False, False, False, blend='hann')
    with pytest.raises(ValueError, match='q'):
        segmentation('a.mha', str(tmp_path), str(tmp_path), 'seg.mha', 0, False, False, False, False, mirror_axes='xq')


# ---------------------------------------------------------------------------------------------------------------------
# mirror augmentation of the training data set
# ---------------------------------------------------------------------------------------------------------------------
def _toy_case(tmp_path):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    rng = np.random.RandomState(11)
    frame = ((0.9, 1.1, 1.3), (-4.0, 2.0, 7.0), tuple(np.eye(3).ravel()))
    write_mha(Image3d(rng.randn(20, 24, 28).astype(np.float32), *frame), str(tmp_path / 'im.mha'))
    seg = (rng.rand(20, 24, 28) > 0.7).astype(np.int8) + (rng.rand(20, 24, 28) > 0.9).astype(np.int8)
    write_mha(Image3d(seg, *frame), str(tmp_path / 'seg.mha'))
    lst = tmp_path / 'train.txt'
    lst.write_text('1\n{}\n{}\n'.format(tmp_path / 'im.mha', tmp_path / 'seg.mha'))
    return str(lst)


def _parent_geometry_draws(ds, index, method):
    """the RNG calls of sample_crop_geometry as they were before mirror augmentation existed, restated"""
    case = ds.case(index)

    def global_sample():
        im_size_mm = [case.seg_size[i] * case.seg_frame[0][i] for i in range(3)]
        crop_mm = ds.crop_size * ds.spacing
        for i in range(3):
            if im_size_mm[i] > crop_mm[i]:
                np.random.uniform(0, im_size_mm[i] - crop_mm[i])

    def mask_sample():
        label = np.random.randint(1, ds.num_classes)
        n = int((case.seg_host == label).sum())
        if n == 0:
            global_sample()
        else:
            np.random.randint(0, n)
    if method == 'GLOBAL':
        global_sample()
    elif method == 'MASK':
        mask_sample()
    elif method == 'HYBRID':
        global_sample() if index % 2 else mask_sample()
    np.random.uniform(-ds.random_translation, ds.random_translation, size=[3])
    np.random.uniform(ds.random_scale[0], ds.random_scale[1])


@pytest.mark.parametrize('method', ['CENTER', 'GLOBAL', 'MASK', 'HYBRID'])
def test_rng_stream_without_mirror_axes_is_unchanged(tmp_path, method):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    lst = _toy_case(tmp_path)
    args = (lst, 3, [1.0, 1.0, 1.0], [16, 16, 16], method, [3, 3, 3], [0.9, 1.1], 'LINEAR', [AdaptiveNormalizer()])
    ds = SegmentationDataset(*args, device=torch.device('cpu'))
    assert ds.random_mirror_axes == []
    np.random.seed(5)
    for _ in range(3):
        ds.sample_crop_geometry(0)
        assert ds.sample_mirror() == (False, False, False)
    got = np.random.get_state()
    np.random.seed(5)
    for _ in range(3):
        _parent_geometry_draws(ds, 0, method)
    want = np.random.get_state()
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    # with mirror axes: exactly one randint(0, 2, size=k) after the scale draw
    dm = SegmentationDataset(*args, device=torch.device('cpu'), random_mirror_axes=('x', 'z'))
    np.random.seed(5)
    dm.sample_crop_geometry(0)
    flags = dm.sample_mirror()
    got = np.random.get_state()
    np.random.seed(5)
    _parent_geometry_draws(dm, 0, method)
    draw = np.random.randint(0, 2, size=2)
    want = np.random.get_state()
    assert np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert flags == (bool(draw[0]), False, bool(draw[1]))
    with pytest.raises(ValueError, match='w'):
        SegmentationDataset(*args, device=torch.device('cpu'), random_mirror_axes=('w',))


def test_mirrored_index_matrix_and_frame():
    from segmentation3d.utils.image_tools import index_affine, mirror_index_affine, mirror_frame
    src = ((0.8, 1.1, 2.0), (1.0, 2.0, 3.0), np.diag([-1.0, 1.0, 1.0]).ravel())
    dst = ((0.9, 0.6, 0.8), (-9.0, 3.5, 0.5), np.diag([-1.0, 1.0, 1.0]).ravel())
    size = (11, 13, 17)
    M = index_affine(src, dst)
    keep = M.copy()
    for mirror in ((True, False, False), (False, True, True), (True, True, True)):
        Mm = mirror_index_affine(M, size, mirror)
        assert np.array_equal(M, keep)                                   # a copy: the caller's matrix is untouched
        for idx in ((0, 0, 0), (10, 12, 16), (3, 7, 5)):
            mirrored = [size[a] - 1 - idx[a] if mirror[a] else idx[a] for a in range(3)]
            got = Mm @ np.array(list(idx) + [1.0])
            want = M @ np.array(mirrored + [1.0])
            assert np.abs(got - want).max() < 1e-12
        # the frame of the mirrored grid gives the same index map through index_affine
        Mf = index_affine(src, mirror_frame(dst, size, mirror))
        assert np.abs(Mf - Mm).max() < 1e-12
    assert np.array_equal(mirror_index_affine(M, size, (False, False, False)), M)
