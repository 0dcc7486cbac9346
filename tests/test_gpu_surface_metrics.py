"""Surface-distance metrics on the MI355X (csrc/surface.hip behind utils/metrics.cal_surface_distances), every case
against the SciPy restatement `_ref_surface_distances` of tests/test_surface_metrics.py: exact squared distances for unit
spacing, a relative 1e-6 for anisotropic spacing, all label dtypes and input kinds, stream capture, cal_dsc_batch and
the seg_eval command line end to end through .mha files, and a full-size volume."""
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch
from scipy import ndimage

from test_surface_metrics import _ref_surface, _ref_surface_distances

pytestmark = pytest.mark.gpu

_REL = 1e-6     # float64 oracle; see the issue's derivation (fp32 final rounding + a few ulps, >= 10x margin)


def _blob(shape, seed, level=0.55, sigma=2.0):
    """seeded smoothed-noise mask holding about (1 - level) of the volume, with at least one voxel"""
    rng = np.random.RandomState(seed)
    if min(shape) > 1:
        f = ndimage.gaussian_filter(rng.rand(*shape), sigma, mode='wrap')
        m = f > np.quantile(f, level)
    else:
        m = rng.rand(*shape) > level
    m = np.asarray(m, bool)
    m[tuple(int(rng.randint(0, s)) for s in shape)] = True
    return m


def _masks(kind, shape, seed):
    Z, Y, X = shape
    if kind == 'blobs':
        return _blob(shape, seed), _blob(shape, seed + 1)
    if kind == 'single':
        a = np.zeros(shape, bool)
        a[Z // 2, Y // 3, X - 1] = True
        return a, _blob(shape, seed + 2)
    if kind == 'faces':          # ground truth touches every face of the volume
        a = ~_blob(shape, seed + 3, level=0.6)
        a[0], a[-1], a[:, 0], a[:, -1], a[:, :, 0], a[:, :, -1] = True, True, True, True, True, True
        return a, _blob(shape, seed + 4)
    if kind == 'corner':         # both masks confined to the low corner: the EDT box is a small part of the volume
        a, b = np.zeros(shape, bool), np.zeros(shape, bool)
        c = tuple(max(1, s // 3) for s in shape)
        a[:c[0], :c[1], :c[2]] = _blob(c, seed + 5)
        b[:c[0], :c[1], :c[2]] = _blob(c, seed + 6)
        return a, b
    raise ValueError(kind)


def _check_exact(gt, seg):
    from segmentation3d.utils.metrics import directed_surface_distances
    (ia, da), (ib, db) = directed_surface_distances(gt.astype(np.uint8), seg.astype(np.uint8), 1)
    sa, sb = _ref_surface(gt), _ref_surface(seg)
    for idx, d2, query, feature in ((ia, da, sa, sb), (ib, db, sb, sa)):
        want_idx = np.flatnonzero(query)
        assert np.array_equal(idx, want_idx)                    # surface voxels and their count
        dt = ndimage.distance_transform_edt(~feature)
        want = np.round(dt.ravel()[want_idx] ** 2)
        bad = int((d2 != want).sum())
        print('surface voxels {}, squared-distance mismatches {}'.format(idx.size, bad))
        assert bad == 0


@pytest.mark.parametrize('shape', [(1, 1, 1), (1, 7, 300), (17, 33, 65), (96, 96, 96), (128, 160, 200)])
@pytest.mark.parametrize('kind', ['blobs', 'single', 'faces', 'corner'])
def test_exact_squared_edt_unit_spacing(hip_device, shape, kind):
    gt, seg = _masks(kind, shape, 11 + sum(shape))
    _check_exact(gt, seg)


@pytest.mark.parametrize('spacing', [(0.7, 0.7, 2.5), (3.0, 0.5, 1.1)])
@pytest.mark.parametrize('shape,kind', [((17, 33, 65), 'blobs'), ((96, 96, 96), 'faces'), ((128, 160, 200), 'corner'),
                                        ((40, 50, 60), 'single')])
def test_anisotropic_spacing(hip_device, spacing, shape, kind):
    from segmentation3d.utils.metrics import cal_surface_distances
    gt, seg = _masks(kind, shape, 7)
    got, = cal_surface_distances(gt.astype(np.uint8), seg.astype(np.uint8), [1], spacing=spacing)
    want = _ref_surface_distances(gt, seg, 1, spacing)
    for k in ('hd', 'hd95', 'assd'):
        rel = abs(got[k] - want[k]) / max(abs(want[k]), 1e-300)
        print('{} {} {}: got {!r} want {!r} rel {:.2e}'.format(shape, spacing, k, got[k], want[k], rel))
        assert rel <= _REL, k


def _two_label_volumes(shape=(30, 41, 52)):
    a, b = _blob(shape, 21), _blob(shape, 22)
    c, d = _blob(shape, 23, level=0.6), _blob(shape, 24, level=0.6)
    gt = np.zeros(shape, np.int32)
    seg = np.zeros(shape, np.int32)
    gt[a], gt[c & ~a] = 1, 2
    seg[b], seg[d & ~b] = 1, 2
    return gt, seg


def test_all_dtypes_agree(hip_device):
    from segmentation3d.utils.metrics import cal_surface_distances
    gt, seg = _two_label_volumes()
    spacing = (0.7, 0.8, 1.9)
    results = [cal_surface_distances(gt.astype(dt), seg.astype(dt), [1, 2], spacing)
               for dt in (np.int8, np.uint8, np.int16, np.int32, np.float32)]
    for r in results[1:]:
        assert r == results[0]
    for label, got in zip((1, 2), results[0]):
        want = _ref_surface_distances(gt, seg, label, spacing)
        for k in want:
            assert abs(got[k] - want[k]) <= _REL * want[k], (label, k)


def test_numpy_and_device_inputs_identical(hip_device):
    from segmentation3d.utils.metrics import cal_surface_distances
    gt, seg = _two_label_volumes()
    host = cal_surface_distances(gt, seg, [1, 2], (1.1, 0.9, 2.2))
    dev = cal_surface_distances(torch.from_numpy(gt).to(hip_device), torch.from_numpy(seg).to(hip_device), [1, 2],
                                (1.1, 0.9, 2.2))
    assert host == dev


def test_twenty_labels_with_absent_ones(hip_device):
    from segmentation3d.utils.metrics import cal_surface_distances
    shape = (24, 36, 48)
    rng = np.random.RandomState(9)
    smooth = ndimage.gaussian_filter(rng.rand(*shape), 3.0)
    edges = np.quantile(smooth, np.linspace(0, 1, 15))
    gt = np.digitize(smooth, edges[1:-1]).astype(np.int16) + 1                     # labels 1..14
    seg = np.digitize(ndimage.shift(smooth, (0.0, 1.0, -1.0), mode='nearest'), edges[1:-1]).astype(np.int16) + 1
    seg[seg == 5] = 0                                                               # 5 absent from seg only
    labels = list(range(1, 21))                                                     # 15..20 absent from both
    got = cal_surface_distances(gt, seg, labels, (0.9, 1.2, 2.0))
    assert len(got) == 20
    for label, r in zip(labels, got):
        want = _ref_surface_distances(gt, seg, label, (0.9, 1.2, 2.0))
        for k in want:
            if math.isnan(want[k]):
                assert math.isnan(r[k]), (label, k)
            else:
                assert abs(r[k] - want[k]) <= _REL * want[k], (label, k, r[k], want[k])
    assert all(math.isnan(v) for label in (5, 15, 20) for v in got[label - 1].values())


def test_identical_masks_give_zero(hip_device):
    from segmentation3d.utils.metrics import cal_surface_distances
    gt, _ = _two_label_volumes()
    assert cal_surface_distances(gt, gt.copy(), [1, 2], (0.7, 0.7, 2.5)) == [{'hd': 0.0, 'hd95': 0.0, 'assd': 0.0}] * 2


def test_image3d_spacing_and_mismatch(hip_device):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.metrics import cal_surface_distances
    gt, seg = _two_label_volumes()
    a, b = Image3d(gt, spacing=(0.7, 0.7, 2.5)), Image3d(seg, spacing=(0.7, 0.7, 2.5))
    assert cal_surface_distances(a, b, [1]) == cal_surface_distances(gt, seg, [1], (0.7, 0.7, 2.5))
    with pytest.raises(ValueError, match='spacing'):
        cal_surface_distances(a, Image3d(seg, spacing=(0.7, 0.7, 2.6)), [1])


def test_stream_capture_replays_identically(hip_device):
    from segmentation3d.utils.metrics import _SurfacePlan
    gt, seg = _two_label_volumes((40, 48, 56))
    plan = _SurfacePlan(gt, seg, (0.7, 0.9, 2.1))
    plan.surfaces(1)
    na, nb = plan.box[6:8].tolist()
    bufs = [torch.empty(na, dtype=torch.float64, device=hip_device), torch.empty(nb, dtype=torch.float64, device=hip_device)]

    def launches():
        plan.surfaces(1)
        plan.distances(0, bufs[0])
        plan.distances(1, bufs[1])

    launches()
    torch.cuda.synchronize()
    eager = (plan.stats.clone(), [torch.sort(b).values for b in bufs], plan.box.clone())
    for b in bufs:
        b.zero_()
    plan.stats.zero_()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):          # warm-up on the side stream, as torch.cuda.graph expects
        launches()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launches()
    for b in bufs:
        b.zero_()
    plan.stats.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(plan.stats, eager[0])
    assert torch.equal(plan.box, eager[2])
    for b, e in zip(bufs, eager[1]):
        assert torch.equal(torch.sort(b).values, e)
    assert int(plan.stats[0]) == na and int(plan.stats[3]) == nb


# ---- cal_dsc_batch and the command line through .mha files --------------------------------------------------------------
def _write_cases(root, spacing=(0.8, 0.8, 2.0)):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.image_io import write_image
    shape = (20, 30, 34)
    cases = []
    for i in range(3):
        gt, seg = _two_label_volumes(shape) if i < 2 else (np.zeros(shape, np.int32), np.zeros(shape, np.int32))
        if i == 1:
            seg[seg == 2] = 0                            # label 2 missed: FN
        if i == 2:
            gt[2:12, 3:20, 4:25] = 1
            seg[3:12, 3:21, 5:25] = 1                    # label 2 absent from both: TN
        name = 'case{}'.format(i)
        for folder, vol in (('gt', gt), ('seg', seg)):
            os.makedirs(os.path.join(root, folder, name), exist_ok=True)
            write_image(Image3d(vol.astype(np.int16), spacing=spacing), os.path.join(root, folder, name, 'seg.mha'))
        cases.append((name, gt, seg))
    return cases


def _ref_dice(gt, seg, label, threshold):
    a, b = int((gt == label).sum()), int((seg == label).sum())
    if a < threshold and b < threshold:
        return 1.0, 'TN'
    if a < threshold:
        return 0.0, 'FP'
    if b < threshold:
        return 0.0, 'FN'
    return 2 * int(((gt == label) & (seg == label)).sum()) / (a + b), 'TP'


def _check_table(table, cases, labels, spacing, surface):
    rows = table.iloc[:len(cases)]
    for (name, gt, seg), (_, row) in zip(cases, rows.iterrows()):
        assert row['filename'] == 'seg.mha'
        for label in labels:
            score, seg_type = _ref_dice(gt, seg, label, 10)
            assert row['label{}_type'.format(label)] == seg_type
            assert float(row['label{}_score'.format(label)]) == pytest.approx(score, abs=1e-12)
            if not surface:
                continue
            want = _ref_surface_distances(gt, seg, label, spacing)
            for k in ('hd', 'hd95', 'assd'):
                v = float(row['label{}_{}'.format(label, k)])
                if seg_type == 'TP':
                    assert abs(v - want[k]) <= _REL * want[k], (name, label, k)
                else:
                    assert math.isnan(v), (name, label, k)
    if surface:
        mean = table.iloc[len(cases)]
        for label in labels:
            col = 'label{}_hd95'.format(label)
            values = rows[col].astype(float).values
            assert np.isfinite(values).any()             # at least one TP case per label
            assert float(mean[col]) == pytest.approx(np.nanmean(values), rel=1e-12)


def test_cal_dsc_batch_columns_and_values(hip_device, tmp_path):
    from segmentation3d.core.seg_eval import cal_dsc_batch
    cases = _write_cases(str(tmp_path))
    gts = [os.path.join(str(tmp_path), 'gt', n, 'seg.mha') for n, _, _ in cases]
    segs = [os.path.join(str(tmp_path), 'seg', n, 'seg.mha') for n, _, _ in cases]
    plain = cal_dsc_batch(gts, segs, [1, 2], 10, None)
    assert list(plain.columns) == ['filename', 'label1_score', 'label1_type', 'label2_score', 'label2_type']
    _check_table(plain, cases, [1, 2], (0.8, 0.8, 2.0), False)
    full = cal_dsc_batch(gts, segs, [1, 2], 10, str(tmp_path / 'r.csv'), surface_metrics=True)
    assert list(full.columns) == ['filename'] + [c for l in (1, 2) for c in (
        'label{}_score'.format(l), 'label{}_type'.format(l), 'label{}_hd'.format(l), 'label{}_hd95'.format(l),
        'label{}_assd'.format(l))]
    _check_table(full, cases, [1, 2], (0.8, 0.8, 2.0), True)
    assert {'TP', 'FN', 'TN'} <= set(full['label2_type'])


def test_seg_eval_cli_on_toy_folder(hip_device, tmp_path):
    from segmentation3d import seg_eval
    root = str(tmp_path)
    cases = _write_cases(root)
    lst = tmp_path / 'test.txt'
    lst.write_text('{}\n'.format(len(cases)) + ''.join(
        '{} {}\n'.format(n, os.path.join(root, 'gt', n, 'seg.mha')) for n, _, _ in cases))
    out = tmp_path / 'out.csv'
    seg_eval.main(['-i', str(lst), '--gt_folder', os.path.join(root, 'gt'), '--seg_folder', os.path.join(root, 'seg'),
                   '-l', '1', '2', '-o', str(out), '--surface'])
    table = pd.read_csv(str(out), index_col=0)
    assert len(table) == len(cases) + 2
    _check_table(table, cases, [1, 2], (0.8, 0.8, 2.0), True)


def test_full_size_against_scipy(hip_device):
    from segmentation3d.utils.metrics import cal_surface_distances
    shape = (400, 512, 512)
    zz, yy, xx = np.ogrid[:shape[0], :shape[1], :shape[2]]
    gt = (((zz - 200) / 190.0) ** 2 + ((yy - 256) / 240.0) ** 2 + ((xx - 256) / 245.0) ** 2 <= 1.0)
    seg = (((zz - 203) / 186.0) ** 2 + ((yy - 250) / 243.0) ** 2 + ((xx - 260) / 241.0) ** 2 <= 1.0)
    seg[150:170, 200:260, 300:330] = False
    got, = cal_surface_distances(gt.astype(np.uint8), seg.astype(np.uint8), [1], (0.7, 0.7, 2.5))
    want = _ref_surface_distances(gt, seg, 1, (0.7, 0.7, 2.5))
    for k in want:
        print('full size {}: got {!r} want {!r}'.format(k, got[k], want[k]))
        assert abs(got[k] - want[k]) <= _REL * want[k], k
