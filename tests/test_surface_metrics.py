"""Surface-distance metrics (HD, HD95, ASSD) on the CPU: the SciPy restatement of the definitions that the GPU tests
compare against, checked on closed-form cases; the host-side combination step against numpy; the Image3d frame checks;
the workspace size helper; and the `seg_eval` command line's argument parsing."""
import math
import os

import numpy as np
import pytest
from scipy import ndimage

from segmentation3d.utils.image3d import Image3d
from segmentation3d.utils.metrics import (cal_surface_distances, combine_directed, percentile_from_order_stats,
                                          percentile_ranks, _frame)
import segmentation3d.seg_eval as seg_eval_cli

_STRUCT6 = ndimage.generate_binary_structure(3, 1)


def _ref_surface(mask):
    """voxels of the mask with a 6-neighbour outside it; outside the volume counts as outside (border_value = 0)"""
    mask = np.asarray(mask, dtype=bool)
    return mask ^ ndimage.binary_erosion(mask, _STRUCT6, border_value=0)


def _ref_directed(query_surface, feature_surface, spacing):
    """d(p, feature surface) for every p of the query surface, raster order; spacing (sx, sy, sz), arrays [z][y][x]"""
    sx, sy, sz = spacing
    dt = ndimage.distance_transform_edt(~feature_surface, sampling=(sz, sy, sx))
    return dt[query_surface]


def _ref_surface_distances(gt, seg, label, spacing=(1.0, 1.0, 1.0)):
    """SciPy restatement: {'hd', 'hd95', 'assd'} of one label (NaN when the label is absent from gt or seg)"""
    a, b = np.asarray(gt) == label, np.asarray(seg) == label
    if not a.any() or not b.any():
        return {'hd': float('nan'), 'hd95': float('nan'), 'assd': float('nan')}
    sa, sb = _ref_surface(a), _ref_surface(b)
    d_ab, d_ba = _ref_directed(sa, sb, spacing), _ref_directed(sb, sa, spacing)
    return {'hd': float(max(d_ab.max(), d_ba.max())),
            'hd95': float(max(np.percentile(d_ab, 95), np.percentile(d_ba, 95))),
            'assd': float((d_ab.sum() + d_ba.sum()) / (d_ab.size + d_ba.size))}


# ---- the restatement on closed-form cases -----------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 3, 4])
def test_ref_shifted_box(k):
    spacing = (1.3, 0.7, 2.5)
    gt = np.zeros((16, 16, 22), np.uint8)
    seg = np.zeros_like(gt)
    gt[3:13, 3:13, 3:13] = 1
    seg[3:13, 3:13, 3 + k:13 + k] = 1
    r = _ref_surface_distances(gt, seg, 1, spacing)
    assert r['hd'] == pytest.approx(k * 1.3, rel=1e-12)
    assert r['hd95'] == pytest.approx(k * 1.3, rel=1e-12)


def test_ref_single_voxels():
    spacing = (1.3, 0.7, 2.5)
    gt = np.zeros((8, 9, 7), np.int16)
    seg = np.zeros_like(gt)
    gt[1, 2, 3] = 2
    seg[1 + 3, 2 + 4, 3 + 2] = 2
    want = math.sqrt((2 * 1.3) ** 2 + (4 * 0.7) ** 2 + (3 * 2.5) ** 2)
    r = _ref_surface_distances(gt, seg, 2, spacing)
    for key in ('hd', 'hd95', 'assd'):
        assert r[key] == pytest.approx(want, rel=1e-12), key


def test_ref_identical_masks_are_zero():
    rng = np.random.RandomState(5)
    gt = (ndimage.gaussian_filter(rng.rand(20, 24, 28), 2.0) > 0.5).astype(np.uint8)
    assert gt.any()
    assert _ref_surface_distances(gt, gt.copy(), 1, (0.7, 0.9, 2.0)) == {'hd': 0.0, 'hd95': 0.0, 'assd': 0.0}


def test_ref_full_volume_surface_has_border():
    full = np.ones((4, 5, 6), bool)
    assert int(_ref_surface(full).sum()) == 96          # 120 voxels minus the 4 x 3 x 2 interior


def test_ref_absent_label_is_nan():
    gt = np.zeros((5, 5, 5), np.uint8)
    seg = gt.copy()
    seg[2, 2, 2] = 1
    r = _ref_surface_distances(gt, seg, 1)
    assert all(math.isnan(v) for v in r.values())


# ---- host-side combination step against numpy ------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 3, 20, 21, 101, 1000, 4097])
def test_percentile_from_order_stats_matches_numpy(n):
    rng = np.random.RandomState(n)
    v = rng.rand(n) * 40.0
    s = np.sort(v)
    lo, hi, gamma = percentile_ranks(n)
    assert percentile_from_order_stats(s[lo], s[hi], gamma) == np.percentile(v, 95)


def test_percentile_with_ties_and_integers():
    v = np.sqrt(np.array([0, 1, 1, 2, 4, 4, 4, 5, 9, 9, 13, 25], np.float64))
    lo, hi, gamma = percentile_ranks(v.size)
    s = np.sort(v)
    assert percentile_from_order_stats(s[lo], s[hi], gamma) == np.percentile(v, 95)


def test_combine_directed_matches_numpy():
    rng = np.random.RandomState(3)
    d_ab, d_ba = rng.rand(57) * 3.0, rng.rand(91) * 5.0

    def summary(d):
        s = np.sort(d)
        lo, hi, gamma = percentile_ranks(d.size)
        return (d.size, d.max(), d.sum(), percentile_from_order_stats(s[lo], s[hi], gamma))

    r = combine_directed(summary(d_ab), summary(d_ba))
    assert r['hd'] == max(d_ab.max(), d_ba.max())
    assert r['hd95'] == max(np.percentile(d_ab, 95), np.percentile(d_ba, 95))
    assert r['assd'] == pytest.approx((d_ab.sum() + d_ba.sum()) / (d_ab.size + d_ba.size), rel=1e-15)
    assert all(isinstance(v, float) for v in r.values())


def test_combine_directed_nan_rule():
    for ab, ba in ((None, (3, 1.0, 2.0, 1.0)), ((3, 1.0, 2.0, 1.0), None), ((0, 0.0, 0.0, 0.0), (3, 1.0, 2.0, 1.0))):
        assert all(math.isnan(v) for v in combine_directed(ab, ba).values())


# ---- frame checks (no device work) ------------------------------------------------------------------------------------
def test_frame_spacing_from_images_and_default():
    a = Image3d(np.zeros((4, 5, 6), np.uint8), spacing=(0.7, 0.8, 2.5))
    b = Image3d(np.zeros((4, 5, 6), np.uint8), spacing=(0.7 * (1 + 5e-7), 0.8, 2.5))
    assert _frame(a, b, None) == (0.7, 0.8, 2.5)
    assert _frame(np.zeros((2, 2, 2)), np.zeros((2, 2, 2)), None) == (1.0, 1.0, 1.0)
    assert _frame(np.zeros((2, 2, 2)), np.zeros((2, 2, 2)), (3.0, 0.5, 1.1)) == (3.0, 0.5, 1.1)


def test_frame_mismatch_raises_naming_both():
    a = Image3d(np.zeros((4, 5, 6), np.uint8), spacing=(0.7, 0.8, 2.5))
    b = Image3d(np.zeros((4, 5, 6), np.uint8), spacing=(0.7, 0.8, 2.5 * (1 + 3e-6)))
    with pytest.raises(ValueError, match=r'spacing \(0\.7, 0\.8, 2\.5\).*spacing \(0\.7, 0\.8, 2\.5000'):
        _frame(a, b, None)
    c = Image3d(np.zeros((4, 5, 7), np.uint8), spacing=(0.7, 0.8, 2.5))
    with pytest.raises(ValueError, match=r'size \(6, 5, 4\).*size \(7, 5, 4\)'):
        cal_surface_distances(a, c, [1])


def test_workspace_helper_is_host_arithmetic():
    import __graft_entry__  # noqa: F401
    from segmentation3d import _engine as E
    if not os.path.isfile(E.LIB_PATH):
        __graft_entry__.build()
    n = 7 * 33 * 65
    nbytes = E.query('seg3d_surface_distance_workspace_bytes', 65, 33, 7)
    assert nbytes >= 28 * n                     # x distances, y-pass output, envelope stacks
    assert E.query('seg3d_surface_distance_workspace_bytes', 2 ** 16, 2 ** 15, 1) == -1   # 2^31 voxels
    assert E.query('seg3d_surface_distance_workspace_bytes', 0, 3, 3) == -1


# ---- command line -----------------------------------------------------------------------------------------------------
def test_cli_defaults():
    args = seg_eval_cli.build_parser().parse_args(['-i', 'test.txt', '--gt_folder', 'gt', '--seg_folder', 'res',
                                                   '-l', '1', '2'])
    assert args.input == 'test.txt' and args.gt_folder == 'gt' and args.seg_folder == 'res'
    assert args.gt_name == 'seg.mha' and args.seg_name == 'seg.mha'
    assert args.labels == [1, 2] and args.threshold == 10
    assert args.output is None and args.surface is False


def test_cli_all_options():
    args = seg_eval_cli.build_parser().parse_args(
        ['--input', 'cases', '--gt_folder', 'g', '--gt_name', 'mask.nii.gz', '--seg_folder', 's', '--seg_name', 'p.mha',
         '-l', '3', '-t', '0', '-o', 'out.csv', '--surface'])
    assert (args.gt_name, args.seg_name, args.labels, args.threshold, args.output, args.surface) == (
        'mask.nii.gz', 'p.mha', [3], 0, 'out.csv', True)


def test_cli_requires_labels_and_folders():
    for argv in (['-i', 'a.txt', '--gt_folder', 'g', '--seg_folder', 's'],
                 ['-i', 'a.txt', '--seg_folder', 's', '-l', '1'],
                 ['-i', 'a.txt', '--gt_folder', 'g', '-l', '1']):
        with pytest.raises(SystemExit):
            seg_eval_cli.build_parser().parse_args(argv)


def test_cli_case_names_from_list_and_folder(tmp_path):
    img = tmp_path / 'images'
    img.mkdir()
    for name in ('case_b', 'case_a'):
        (img / (name + '.mha')).write_bytes(b'')
    lst = tmp_path / 'test.txt'
    lst.write_text('2\ncase_b {}\ncase_a {}\n'.format(img / 'case_b.mha', img / 'case_a.mha'))
    assert seg_eval_cli.case_names(str(lst)) == ['case_b', 'case_a']
    assert seg_eval_cli.case_names(str(img)) == ['case_a', 'case_b']
    with pytest.raises(ValueError):
        seg_eval_cli.case_names(str(tmp_path / 'test.csv'))
