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
typing.  Surface metrics are reported for labels only."""
import os

import pandas as pd

from segmentation3d.utils.metrics import cal_dsc_labels, cal_region_dsc, cal_surface_distances
from segmentation3d.utils.image_io import read_image


_SURFACE_KEYS = ('hd', 'hd95', 'assd')


def _columns(labels, surface_metrics=False, regions=None):
    cols = ['filename']
    for label in labels:
        cols += ['label{}_score'.format(label), 'label{}_type'.format(label)]
        if surface_metrics:
            cols += ['label{}_{}'.format(label, k) for k in _SURFACE_KEYS]
    for k in range(len(regions or ())):
        cols += ['region{}_score'.format(k), 'region{}_type'.format(k)]
    return cols


def _score_case(gt_path, seg_path, labels, threshold, surface_metrics=False, regions=None):
    """one table row: file name, then (score, type) per label; also echoes the reference's progress lines"""
    name = os.path.basename(gt_path)
    gt, seg = read_image(gt_path, dtype=None), read_image(seg_path, dtype=None)
    results = cal_dsc_labels(gt, seg, labels, threshold)
    surface = {}
    if surface_metrics:   # only the TP labels are measured; the others hold NaN
        tp = [label for label, (_, seg_type) in zip(labels, results) if seg_type == 'TP']
        surface = dict(zip(tp, cal_surface_distances(gt, seg, tp))) if tp else {}
    row = [name]
    for label, (score, seg_type) in zip(labels, results):
        row += [score, seg_type]
        if not surface_metrics:
            print('case_name: {}, label: {}, score: {}, type: {}'.format(name, label, score, seg_type))
            continue
        values = [surface.get(label, {}).get(k, float('nan')) for k in _SURFACE_KEYS]
        print('case_name: {}, label: {}, score: {}, type: {}, hd: {}, hd95: {}, assd: {}'.format(
            name, label, score, seg_type, *values))
        row += values
    if regions:
        for k, (score, seg_type) in enumerate(cal_region_dsc(gt, seg, regions, threshold)):
            print('case_name: {}, region: {}, score: {}, type: {}'.format(name, k, score, seg_type))
            row += [score, seg_type]
    return row


def cal_dsc_batch(gt_files, seg_files, labels, threshold, save_csv_file_path, surface_metrics=False, regions=None):
    """
    :param gt_files, seg_files: equally long lists of label-volume files (.mha / .mhd)
    :param labels: the labels to score
    :param threshold: minimal voxel count for a label to count as present (TN / FP / FN / TP typing)
    :param save_csv_file_path: result csv; None only returns the DataFrame
    :param surface_metrics: also report HD, HD95 and ASSD (physical units) per label, NaN unless the type is TP
    :param regions: list of label-id sets; adds region<k>_score / region<k>_type columns after the label columns
    """
    if regions is not None:
        from segmentation3d.loss.region_loss import check_regions
        regions = check_regions(regions)
    assert isinstance(gt_files, list) and isinstance(seg_files, list)
    assert len(gt_files) == len(seg_files)
    cols = _columns(labels, surface_metrics, regions)
    cases = pd.DataFrame([_score_case(g, s, labels, threshold, surface_metrics, regions)
                          for g, s in zip(gt_files, seg_files)], columns=cols)
    summary = {'mean': ['mean'], 'std': ['std']}
    for label in labels:
        scores = cases['label{}_score'.format(label)]
        mean, std = scores.mean(), scores.std()
        print(mean, std)
        summary['mean'] += [mean, 'ignore_type']
        summary['std'] += [std, 'ignore_type']
        if surface_metrics:
            for k in _SURFACE_KEYS:
                values = cases['label{}_{}'.format(label, k)].astype(float)
                summary['mean'].append(values.mean())
                summary['std'].append(values.std())
    for k in range(len(regions or ())):
        scores = cases['region{}_score'.format(k)]
        mean, std = scores.mean(), scores.std()
        print(mean, std)
        summary['mean'] += [mean, 'ignore_type']
        summary['std'] += [std, 'ignore_type']
    table = pd.concat([cases, pd.DataFrame([summary['mean'], summary['std']], columns=cols)])
    if save_csv_file_path:
        table.to_csv(save_csv_file_path)
    return table
