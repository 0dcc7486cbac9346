"""Lesion-wise evaluation without a GPU: the SciPy oracle (tests/lesion_oracle.py) on hand-computed cases, the pure-Python
aggregation `lesionwise_from_table` against the oracle, option checks, the CSV column layout and the command line."""
import math

import numpy as np
import pytest

import lesion_cases as C
import lesion_oracle as O


# ---- the oracle on cases whose numbers are written out in lesion_cases.py -------------------------------------------------
def test_oracle_two_blobs_merge_after_one_dilation():
    gt, _ = C.two_blobs_two_apart()
    assert O.components26(O.dilate18(gt, 0))[1:] == (2, [1, 1])
    ids, k, sizes = O.components26(O.dilate18(gt, 1))
    # each voxel grows to itself + its 18 neighbours = 19 voxels, all inside the volume; the two share the 5 voxels of the
    # plane x = 2 that differ from (8, 4, 2) in at most one of y, z
    assert k == 1 and sizes == [2 * 19 - 5] and int((ids > 0).sum()) == 33


def test_oracle_dilation_is_the_18_neighbourhood():
    v = np.zeros((5, 5, 5), bool)
    v[2, 2, 2] = True
    d = O.dilate18(v, 1)
    assert int(d.sum()) == 19 and not d[1, 1, 1] and d[1, 1, 2] and d[2, 1, 1]
    assert np.array_equal(O.dilate18(v, 0), v)
    corner = np.zeros((3, 4, 5), bool)
    corner[0, 0, 0] = True
    assert int(O.dilate18(corner, 1).sum()) == 7          # itself, 3 face and 3 edge neighbours: nothing wraps


def test_oracle_corner_contact_and_canonical_order():
    ids, k, sizes = O.components26(C.corner_touching())
    assert (k, sizes) == (3, [2, 1, 1])
    assert ids[2, 2, 1] == ids[3, 3, 2] == 1 and ids[9, 2, 1] == 2 and ids[11, 4, 3] == 3


def test_oracle_bridge_counts_in_both_lesions():
    gt, seg = C.bridge()
    r = O.lesionwise(gt, seg, [1], dilation_iters=0)
    assert O.pair_table(gt, seg, [1], 0)[7] == [(1, 1), (2, 1)]
    assert [l[2] for l in r['lesions']] == [2.0 / 9.0, 2.0 / 9.0]
    assert (r['n_gt'], r['n_tp'], r['n_fn'], r['n_fp']) == (2, 2, 0, 0)
    assert r['lw_dice'] == pytest.approx(2.0 / 9.0, abs=1e-15)


def test_oracle_halo_match():
    gt, seg = C.halo_only()
    r = O.lesionwise(gt, seg, [1], dilation_iters=1)
    assert r['lesions'] == [(1, 1, 0.0, 1.0, (1,))]
    assert (r['n_tp'], r['n_fn'], r['n_fp'], r['lw_dice'], r['lw_hd95']) == (1, 0, 0, 0.0, 1.0)
    r0 = O.lesionwise(gt, seg, [1], dilation_iters=0)          # without the halo: one FN and one FP
    assert (r0['n_tp'], r0['n_fn'], r0['n_fp'], r0['lw_dice'], r0['lw_hd95']) == (0, 1, 1, 0.0, 374.0)


@pytest.mark.parametrize('penalty', [374.0, 50.0])
def test_oracle_fn_fp_tp(penalty):
    gt, seg = C.fn_fp_tp()
    r = O.lesionwise(gt, seg, [1], dilation_iters=0, hd95_penalty=penalty)
    assert (r['n_gt'], r['n_tp'], r['n_fn'], r['n_fp']) == (2, 1, 1, 1)
    assert r['lesions'][0][2] == 0.5 and r['lesions'][0][3] == pytest.approx(0.95, abs=1e-12)
    assert r['lesions'][1] == (2, 1, 0.0, penalty, ())
    assert r['lw_dice'] == pytest.approx(0.5 / 3.0, abs=1e-15)
    assert r['lw_hd95'] == pytest.approx((0.95 + 2.0 * penalty) / 3.0, abs=1e-12)
    assert r['lesion_f1'] == 0.5


def test_oracle_empty_cases():
    empty = np.zeros(C.SHAPE_B, np.uint8)
    one = empty.copy()
    one[3, 3, 3] = 1
    r = O.lesionwise(empty, empty, [1])
    assert (r['lw_dice'], r['lw_hd95'], r['lesion_f1'], r['n_gt'], r['n_fp']) == (1.0, 0.0, 1.0, 0, 0)
    r = O.lesionwise(empty, one, [1])
    assert (r['lw_dice'], r['lw_hd95'], r['n_gt'], r['n_fp'], r['lesion_f1']) == (0.0, 374.0, 0, 1, 0.0)
    gt, _ = C.fn_fp_tp()
    r = O.lesionwise(gt, empty, [1], dilation_iters=0)
    assert (r['n_gt'], r['n_tp'], r['n_fn'], r['n_fp'], r['lw_dice'], r['lw_hd95']) == (2, 0, 2, 0, 0.0, 374.0)


def test_oracle_dropped_lesion_keeps_its_match():
    gt, seg = C.small_and_large()
    r = O.lesionwise(gt, seg, [1], dilation_iters=0, min_lesion_voxels=2)
    assert (r['n_gt'], r['n_tp'], r['n_fn'], r['n_fp'], r['lw_dice'], r['lw_hd95']) == (1, 1, 0, 0, 1.0, 0.0)
    assert r['lesions'] == [(2, 3, 1.0, 0.0, (2,))]
    r = O.lesionwise(gt, seg, [1], dilation_iters=0)
    assert r['n_gt'] == 2


def test_oracle_nsd():
    gt, seg = C.halo_only()                                    # two single voxels one apart
    assert O.nsd(gt, gt, 1, tau=0.0) == 1.0
    assert O.nsd(gt, seg, 1, tau=1.0) == 1.0                   # <=
    assert O.nsd(gt, seg, 1, tau=0.999) == 0.0
    assert math.isnan(O.nsd(gt, np.zeros_like(gt), 1))


# ---- lesionwise_from_table -------------------------------------------------------------------------------------------------
def _table_result(gt, seg, target, spacing=(1.0, 1.0, 1.0), **options):
    from segmentation3d.utils.metrics import lesionwise_from_table
    iters = options.pop('dilation_iters', 3)
    want = O.lesionwise(gt, seg, target, spacing, dilation_iters=iters, **options)
    _, _, _, _, psizes, gsize, inter, pairs = O.pair_table(gt, seg, target, iters)
    hd95 = {l[0]: l[3] for l in want['lesions']}
    got = lesionwise_from_table(gsize, inter, psizes, pairs, lambda i, ids: hd95[i], **options)
    return got, want


@pytest.mark.parametrize('case,options', [
    (C.bridge, {'dilation_iters': 0}), (C.halo_only, {'dilation_iters': 1}), (C.halo_only, {'dilation_iters': 0}),
    (C.fn_fp_tp, {'dilation_iters': 0}), (C.fn_fp_tp, {'dilation_iters': 0, 'hd95_penalty': 50.0}),
    (C.small_and_large, {'dilation_iters': 0, 'min_lesion_voxels': 2}), (C.faces, {'dilation_iters': 2}),
    (C.faces, {'dilation_iters': 3, 'min_lesion_voxels': 2, 'hd95_penalty': 0.0})])
def test_from_table_matches_oracle(case, options):
    gt, seg = case()
    got, want = _table_result(gt, seg, [1], **options)
    assert got == want                  # same integers, same doubles in the same order


def test_from_table_random_multi_id_target():
    gt = C.random_blobs(C.SHAPE_A, 5, count=9, labels=(1, 2, 4))
    seg = C.perturbed(gt, 6)
    got, want = _table_result(gt, seg, [1, 4], (0.7, 0.7, 2.5), dilation_iters=1)
    assert want['n_gt'] > 1
    assert got == want


def test_from_table_empty():
    from segmentation3d.utils.metrics import lesionwise_from_table
    r = lesionwise_from_table([], [], [], [], None)
    assert (r['lw_dice'], r['lw_hd95'], r['lesion_f1'], r['lesions']) == (1.0, 0.0, 1.0, [])
    r = lesionwise_from_table([], [], [5], [], None, hd95_penalty=10.0)
    assert (r['lw_dice'], r['lw_hd95'], r['n_fp'], r['lesion_f1']) == (0.0, 10.0, 1, 0.0)


# ---- option checks -----------------------------------------------------------------------------------------------------------
def test_option_checks():
    from segmentation3d.utils.metrics import check_lesion_options, check_nsd_tolerance, check_target
    assert check_lesion_options() == (3, 1, 374.0)
    assert check_lesion_options(0, 5, 0) == (0, 5, 0.0)
    for bad in ({'dilation_iters': -1}, {'dilation_iters': 17}, {'dilation_iters': 1.5}, {'min_lesion_voxels': 0},
                {'hd95_penalty': -1.0}, {'hd95_penalty': float('inf')}, {'hd95_penalty': float('nan')},
                {'hd95_penalty': 'x'}, {'dilation_iters': True}):
        with pytest.raises(ValueError):
            check_lesion_options(**bad)
    assert check_target(3) == [3] and check_target([3, 1, 2]) == [1, 2, 3] and check_target({255}) == [255]
    for bad in (0, 256, -1, [1, 300], [], 'abc', [1.5], None, True):
        with pytest.raises(ValueError):
            check_target(bad)
    assert check_nsd_tolerance(None) is None and check_nsd_tolerance(0) == 0.0 and check_nsd_tolerance(2.5) == 2.5
    for bad in (-0.1, float('inf'), float('nan'), 'x'):
        with pytest.raises(ValueError):
            check_nsd_tolerance(bad)


def test_cal_dsc_batch_rejects_bad_options_before_reading(tmp_path):
    from segmentation3d.core.seg_eval import cal_dsc_batch
    missing = [str(tmp_path / 'nowhere.mha')]
    for kwargs in ({'lesionwise': True, 'lesion_options': {'dilation_iters': 99}},
                   {'lesionwise': True, 'lesion_options': {'min_voxels': 2}},
                   {'lesionwise': True, 'lesion_options': {'hd95_penalty': -5}},
                   {'surface_metrics': True, 'nsd_tolerance': -1.0},
                   {'nsd_tolerance': float('nan')}):
        with pytest.raises(ValueError):
            cal_dsc_batch(missing, missing, [1], 10, None, **kwargs)
    with pytest.raises(ValueError):
        cal_dsc_batch(missing, missing, [1, 300], 10, None, lesionwise=True)


# ---- CSV layout ----------------------------------------------------------------------------------------------------------------
def _parent_columns(labels, surface_metrics=False, regions=None):
    """the column list of the table before the lesion-wise options existed"""
    cols = ['filename']
    for label in labels:
        cols += ['label{}_score'.format(label), 'label{}_type'.format(label)]
        if surface_metrics:
            cols += ['label{}_{}'.format(label, k) for k in ('hd', 'hd95', 'assd')]
    for k in range(len(regions or ())):
        cols += ['region{}_score'.format(k), 'region{}_type'.format(k)]
    return cols


def test_columns_without_the_new_options_are_unchanged():
    from segmentation3d.core.seg_eval import _columns
    regions = [[1, 2, 3], [1, 3]]
    for surface in (False, True):
        for reg in (None, regions):
            assert _columns([1, 2], surface, reg) == _parent_columns([1, 2], surface, reg)
            assert _columns([1, 2], surface, reg, False, False) == _parent_columns([1, 2], surface, reg)
    assert _columns([1], False, None, nsd=True) == _parent_columns([1])        # the NSD is a surface column


def test_columns_with_the_new_options():
    from segmentation3d.core.seg_eval import _columns
    lw = ['lw_dice', 'lw_hd95', 'n_gt', 'n_fn', 'n_fp', 'lesion_f1']
    assert _columns([2], True, [[1, 2]], lesionwise=True, nsd=True) == (
        ['filename', 'label2_score', 'label2_type', 'label2_hd', 'label2_hd95', 'label2_assd', 'label2_nsd']
        + ['label2_' + k for k in lw] + ['region0_score', 'region0_type'] + ['region0_' + k for k in lw])
    assert _columns([1, 3], False, None, lesionwise=True) == (
        ['filename', 'label1_score', 'label1_type'] + ['label1_' + k for k in lw]
        + ['label3_score', 'label3_type'] + ['label3_' + k for k in lw])


# ---- command line ----------------------------------------------------------------------------------------------------------------
_BASE = ['-i', 'x.txt', '--gt_folder', 'g', '--seg_folder', 's', '-l', '1']


def test_cli_defaults_and_flags():
    from segmentation3d.seg_eval import build_parser, lesion_options
    args = build_parser().parse_args(_BASE)
    assert not args.lesionwise and args.nsd_tolerance is None
    assert lesion_options(args) == {'dilation_iters': 3, 'min_lesion_voxels': 1, 'hd95_penalty': 374.0}
    args = build_parser().parse_args(_BASE + ['--lesionwise', '--lesion_dilation', '1', '--lesion_min_voxels', '5',
                                              '--hd95_penalty', '50', '--nsd_tolerance', '2.5', '--surface'])
    assert args.lesionwise and args.surface and args.nsd_tolerance == 2.5
    assert lesion_options(args) == {'dilation_iters': 1, 'min_lesion_voxels': 5, 'hd95_penalty': 50.0}


@pytest.mark.parametrize('extra', [['--lesion_dilation', '17'], ['--lesion_min_voxels', '0'], ['--hd95_penalty', '-1'],
                                   ['--nsd_tolerance', '-2'], ['--hd95_penalty', 'inf']])
def test_cli_bad_values_raise_before_the_case_list_is_read(extra):
    from segmentation3d import seg_eval
    with pytest.raises(ValueError):
        seg_eval.main(_BASE + ['--lesionwise'] + extra)      # x.txt does not exist: reading it would raise another error
