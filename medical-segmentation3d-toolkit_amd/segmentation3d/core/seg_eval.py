"""Batch Dice evaluation: `cal_dsc_batch` with the reference's signature, console output and CSV layout
(core/seg_eval.py:8-57) -- one row per case holding `label<k>_score` / `label<k>_type` pairs, followed by a `mean` and
a `std` row whose type cells read 'ignore_type'.

What differs underneath: label volumes come from the built-in MetaImage reader (no SimpleITK), every case is counted
in ONE device pass for all labels (utils/metrics.cal_dsc_labels -> csrc/metrics.hip), and the table is assembled from
records with `pandas.concat` (`DataFrame.append`, which the reference calls at :56, was removed from pandas).

`surface_metrics=True` (not in the reference) adds `label<k>_hd`, `label<k>_hd95` and `label<k>_assd` after each
label's score / type pair (utils/metrics.cal_surface_distances -> csrc/surface.hip, in the images' spacing); they are
NaN where the type is not TP, and the mean / std rows skip NaN.

`regions=[[1, 2, 3], [1, 3], [3]]` (not in the reference) adds `region<k>_score` / `region<k>_type` columns after the label
columns: the Dice of the union of each region's labels (utils/metrics.cal_region_dsc), with the same TN / FP / FN / TP
typing.  Surface metrics are reported for labels only.

`lesionwise=True` (not in the reference) adds `<prefix>_lw_dice`, `_lw_hd95`, `_n_gt`, `_n_fn`, `_n_fp` and `_lesion_f1`
after each label's columns and after each region's (utils/metrics.cal_lesionwise -> csrc/lesion.hip), and
`nsd_tolerance` with `surface_metrics` adds `label<k>_nsd` after `label<k>_assd`.  Without these options the table is
the one described above, byte for byte."""
import os

import pandas as pd

from segmentation3d.utils.metrics import (cal_dsc_labels, cal_lesionwise, cal_region_dsc, cal_surface_distances,
                                          check_lesion_options, check_nsd_tolerance, check_target)
from segmentation3d.utils.image_io import read_image


_SURFACE_KEYS = ('hd', 'hd95', 'assd')
_LESION_KEYS = ('lw_dice', 'lw_hd95', 'n_gt', 'n_fn', 'n_fp', 'lesion_f1')
_LESION_OPTIONS = ('dilation_iters', 'min_lesion_voxels', 'hd95_penalty')


def _columns(labels, surface_metrics=False, regions=None, lesionwise=False, nsd=False):
    cols = ['filename']
    for label in labels:
        cols += ['label{}_score'.format(label), 'label{}_type'.format(label)]
        if surface_metrics:
            cols += ['label{}_{}'.format(label, k) for k in _SURFACE_KEYS]
            if nsd:
                cols.append('label{}_nsd'.format(label))
        if lesionwise:
            cols += ['label{}_{}'.format(label, k) for k in _LESION_KEYS]
    for k in range(len(regions or ())):
        cols += ['region{}_score'.format(k), 'region{}_type'.format(k)]
        if lesionwise:
            cols += ['region{}_{}'.format(k, key) for key in _LESION_KEYS]
    return cols


def check_lesion_kwargs(lesion_options):
    """lesion_options of cal_dsc_batch -> checked keyword arguments of cal_lesionwise"""
    options = dict(lesion_options or {})
    unknown = sorted(set(options) - set(_LESION_OPTIONS))
    if unknown:
        raise ValueError('unknown lesion option(s) {}; known: {}'.format(unknown, list(_LESION_OPTIONS)))
    return dict(zip(_LESION_OPTIONS, check_lesion_options(**options)))


def _score_case(gt_path, seg_path, labels, threshold, surface_metrics=False, regions=None, lesion_kwargs=None,
                nsd_tolerance=None):
    """one table row: file name, then (score, type) per label; also echoes the reference's progress lines"""
    name = os.path.basename(gt_path)
    gt, seg = read_image(gt_path, dtype=None), read_image(seg_path, dtype=None)
    results = cal_dsc_labels(gt, seg, labels, threshold)
    surface = {}
    surface_keys = _SURFACE_KEYS + (('nsd',) if nsd_tolerance is not None else ())
    if surface_metrics:   # only the TP labels are measured; the others hold NaN
        tp = [label for label, (_, seg_type) in zip(labels, results) if seg_type == 'TP']
        surface = dict(zip(tp, cal_surface_distances(gt, seg, tp, nsd_tolerance=nsd_tolerance))) if tp else {}
    lesion = []
    if lesion_kwargs is not None:   # the labels' targets first, then the regions'
        lesion = cal_lesionwise(gt, seg, [[label] for label in labels] + list(regions or ()), **lesion_kwargs)
    row = [name]
    for n, (label, (score, seg_type)) in enumerate(zip(labels, results)):
        row += [score, seg_type]
        if not surface_metrics:
            print('case_name: {}, label: {}, score: {}, type: {}'.format(name, label, score, seg_type))
        else:
            values = [surface.get(label, {}).get(k, float('nan')) for k in surface_keys]
            print('case_name: {}, label: {}, score: {}, type: {}, hd: {}, hd95: {}, assd: {}'.format(
                name, label, score, seg_type, *values[:3]))
            row += values
        if lesion:
            print('case_name: {}, label: {}, '.format(name, label) + ', '.join(
                '{}: {}'.format(k, lesion[n][k]) for k in _LESION_KEYS))
            row += [lesion[n][k] for k in _LESION_KEYS]
    if regions:
        for k, (score, seg_type) in enumerate(cal_region_dsc(gt, seg, regions, threshold)):
            print('case_name: {}, region: {}, score: {}, type: {}'.format(name, k, score, seg_type))
            row += [score, seg_type]
            if lesion:
                r = lesion[len(labels) + k]
                print('case_name: {}, region: {}, '.format(name, k) + ', '.join(
                    '{}: {}'.format(key, r[key]) for key in _LESION_KEYS))
                row += [r[key] for key in _LESION_KEYS]
    return row


def cal_dsc_batch(gt_files, seg_files, labels, threshold, save_csv_file_path, surface_metrics=False, regions=None,
                  lesionwise=False, lesion_options=None, nsd_tolerance=None):
    """
    :param gt_files, seg_files: equally long lists of label-volume files (.mha / .mhd)
    :param labels: the labels to score
    :param threshold: minimal voxel count for a label to count as present (TN / FP / FN / TP typing)
    :param save_csv_file_path: result csv; None only returns the DataFrame
    :param surface_metrics: also report HD, HD95 and ASSD (physical units) per label, NaN unless the type is TP
    :param regions: list of label-id sets; adds region<k>_score / region<k>_type columns after the label columns
    :param lesionwise: adds <prefix>_lw_dice, _lw_hd95, _n_gt, _n_fn, _n_fp, _lesion_f1 after each label's columns and
                       after each region's (utils/metrics.cal_lesionwise); labels must then be in 1..255
    :param lesion_options: {'dilation_iters', 'min_lesion_voxels', 'hd95_penalty'}, defaults 3, 1, 374.0 (BraTS-GLI)
    :param nsd_tolerance: tolerance in millimetres; with surface_metrics adds label<k>_nsd after label<k>_assd
    Bad option values raise ValueError before any case is read.
    """
    if regions is not None:
        from segmentation3d.loss.region_loss import check_regions
        regions = check_regions(regions)
    nsd_tolerance = check_nsd_tolerance(nsd_tolerance)
    if not surface_metrics:
        nsd_tolerance = None        # the normalized surface Dice is one of the surface columns
    lesion_kwargs = None
    if lesionwise:
        lesion_kwargs = check_lesion_kwargs(lesion_options)
        for label in labels:
            check_target(label)
    elif lesion_options:
        check_lesion_kwargs(lesion_options)
    assert isinstance(gt_files, list) and isinstance(seg_files, list)
    assert len(gt_files) == len(seg_files)
    cols = _columns(labels, surface_metrics, regions, lesionwise, nsd_tolerance is not None)
    cases = pd.DataFrame([_score_case(g, s, labels, threshold, surface_metrics, regions, lesion_kwargs, nsd_tolerance)
                          for g, s in zip(gt_files, seg_files)], columns=cols)
    summary = {'mean': ['mean'], 'std': ['std']}

    def numeric(columns):
        for col in columns:
            values = cases[col].astype(float)
            summary['mean'].append(values.mean())
            summary['std'].append(values.std())

    for label in labels:
        scores = cases['label{}_score'.format(label)]
        mean, std = scores.mean(), scores.std()
        print(mean, std)
        summary['mean'] += [mean, 'ignore_type']
        summary['std'] += [std, 'ignore_type']
        if surface_metrics:
            numeric('label{}_{}'.format(label, k) for k in _SURFACE_KEYS + (('nsd',) if nsd_tolerance is not None else ()))
        if lesionwise:
            numeric('label{}_{}'.format(label, k) for k in _LESION_KEYS)
    for k in range(len(regions or ())):
        scores = cases['region{}_score'.format(k)]
        mean, std = scores.mean(), scores.std()
        print(mean, std)
        summary['mean'] += [mean, 'ignore_type']
        summary['std'] += [std, 'ignore_type']
        if lesionwise:
            numeric('region{}_{}'.format(k, key) for key in _LESION_KEYS)
    table = pd.concat([cases, pd.DataFrame([summary['mean'], summary['std']], columns=cols)])
    if save_csv_file_path:
        table.to_csv(save_csv_file_path)
    return table
