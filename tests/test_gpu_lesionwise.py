"""Lesion-wise evaluation and the normalized surface Dice on the MI355X, through the C ABI (csrc/lesion.hip and the
labelling entry of csrc/postproc.hip) and through utils/metrics.cal_lesionwise, against tests/lesion_oracle.py.
Integers (id maps, K, sizes, |G_i|, |G_i n B|, pairs, detection counts) must be exact, Dice within 1e-12 (both sides
divide the same integers in double), HD95 / NSD exact for unit spacing and within test_gpu_surface_metrics' _REL else."""
import ctypes
import math
import os

import numpy as np
import pandas as pd
import pytest
import torch

import lesion_cases as C
import lesion_oracle as O
from test_gpu_surface_metrics import _REL

pytestmark = pytest.mark.gpu

_GUARD = 0x5a5a5a5a
_UNIT = (1.0, 1.0, 1.0)
_INT_KEYS = ('n_gt', 'n_tp', 'n_fn', 'n_fp')


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _close(got, want, spacing):
    if spacing == _UNIT:
        return got == want
    return abs(got - want) <= _REL * abs(want)


def _check_result(got, want, spacing):
    for k in _INT_KEYS:
        assert got[k] == want[k], k
    assert abs(got['lw_dice'] - want['lw_dice']) <= 1e-12
    assert abs(got['lesion_f1'] - want['lesion_f1']) <= 1e-12
    assert len(got['lesions']) == len(want['lesions'])
    for g, w in zip(got['lesions'], want['lesions']):
        assert (g[0], g[1], tuple(g[4])) == (w[0], w[1], tuple(w[4]))
        assert abs(g[2] - w[2]) <= 1e-12
        print('lesion {}: voxels {}, dice {!r}, hd95 got {!r} want {!r}'.format(g[0], g[1], g[2], g[3], w[3]))
        assert math.isfinite(g[3]) and _close(g[3], w[3], spacing), (g, w)
    print('lw_hd95 got {!r} want {!r}'.format(got['lw_hd95'], want['lw_hd95']))
    if spacing == _UNIT:
        assert got['lw_hd95'] == want['lw_hd95']
    else:
        assert abs(got['lw_hd95'] - want['lw_hd95']) <= _REL * abs(want['lw_hd95']) + 0.0


def _check_integers(gt, seg, target, iters, device):
    """masks, dilation, id maps, K, sizes, |G_i|, |G_i n B| and the pair list against the oracle, launch by launch"""
    from segmentation3d.utils import metrics as M
    dmap, kg, pmap, kp, psizes, gsize, inter, pairs = O.pair_table(gt, seg, target, iters)
    ids = M.check_target(target)
    shape = tuple(gt.shape)
    a, b = M._set_mask(_dev(gt, device), ids), M._set_mask(_dev(seg, device), ids)
    assert np.array_equal(a.cpu().numpy().reshape(shape), O.target_mask(gt, target))
    assert np.array_equal(b.cpu().numpy().reshape(shape), O.target_mask(seg, target))
    grown = M._dilate18(a, shape, iters)
    assert np.array_equal(grown.cpu().numpy().reshape(shape) != 0, O.dilate18(O.target_mask(gt, target), iters))
    d_ids, d_count, d_sizes = M._ccl26(grown, shape, max(kg, 1))
    p_ids, p_count, p_sizes = M._ccl26(b, shape, max(kp, 1))
    assert d_count.tolist() == [kg, 0] and p_count.tolist() == [kp, 0]
    assert np.array_equal(d_ids.cpu().numpy().reshape(shape), dmap)
    assert np.array_equal(p_ids.cpu().numpy().reshape(shape), pmap)
    assert p_sizes.tolist()[:kp] == psizes
    assert d_sizes.tolist()[:kg] == O.components26(O.dilate18(O.target_mask(gt, target), iters))[2]
    got_g, got_i, got_pairs, _ = M.lesion_pair_table(d_ids, a, p_ids, kg)
    assert got_g == gsize and got_i == inter and got_pairs == pairs
    return kg, kp


def _check_case(gt, seg, target, device, spacing=_UNIT, **options):
    from segmentation3d.utils.metrics import cal_lesionwise
    iters = options.get('dilation_iters', 3)
    _check_integers(gt, seg, target, iters, device)
    got, = cal_lesionwise(gt, seg, [target], spacing=spacing, **options)
    want = O.lesionwise(gt, seg, target, spacing, **options)
    _check_result(got, want, spacing)
    return got


# ---- cases 1-8 -------------------------------------------------------------------------------------------------------------------
def test_two_blobs_two_apart(hip_device):
    from segmentation3d.utils.metrics import lesion_components
    gt, seg = C.two_blobs_two_apart()
    assert lesion_components(gt, 1, 0)[1:] == (2, [1, 1])
    ids, k, sizes = lesion_components(gt, 1, 1)
    assert (k, sizes) == (1, [33]) and ids.dtype == torch.int32 and tuple(ids.shape) == C.SHAPE_B
    assert _check_case(gt, seg, [1], hip_device, dilation_iters=0)['n_fn'] == 2
    assert _check_case(gt, seg, [1], hip_device, dilation_iters=1)['n_fn'] == 1


def test_corner_contact_is_connected(hip_device):
    from segmentation3d.utils.metrics import lesion_components
    v = C.corner_touching()
    ids, k, sizes = lesion_components(v, [1])
    assert (k, sizes) == (3, [2, 1, 1])
    assert np.array_equal(ids.cpu().numpy(), O.components26(v)[0])


def test_bridge_counts_in_both_lesions(hip_device):
    gt, seg = C.bridge()
    r = _check_case(gt, seg, [1], hip_device, dilation_iters=0)
    assert [l[4] for l in r['lesions']] == [(1,), (1,)]
    assert [l[2] for l in r['lesions']] == [2.0 / 9.0, 2.0 / 9.0]          # |U_i| = 7 enters both
    assert (r['n_tp'], r['n_fn'], r['n_fp']) == (2, 0, 0)


def test_halo_only_match(hip_device):
    gt, seg = C.halo_only()
    r = _check_case(gt, seg, [1], hip_device, dilation_iters=1)
    assert r['lesions'] == [(1, 1, 0.0, 1.0, (1,))]
    assert (r['n_tp'], r['n_fn'], r['n_fp']) == (1, 0, 0)


@pytest.mark.parametrize('penalty', [374.0, 50.0])
def test_fn_fp_tp_with_penalty(hip_device, penalty):
    gt, seg = C.fn_fp_tp()
    r = _check_case(gt, seg, [1], hip_device, dilation_iters=0, hd95_penalty=penalty)
    assert (r['n_gt'], r['n_tp'], r['n_fn'], r['n_fp']) == (2, 1, 1, 1)
    assert abs(r['lw_dice'] - 0.5 / 3.0) <= 1e-12
    assert abs(r['lw_hd95'] - (0.95 + 2.0 * penalty) / 3.0) <= _REL * r['lw_hd95']
    assert r['lesion_f1'] == 0.5


def test_empty_cases(hip_device):
    empty = np.zeros(C.SHAPE_B, np.uint8)
    one = empty.copy()
    one[3, 3, 3] = 1
    r = _check_case(empty, empty, [1], hip_device)
    assert (r['lw_dice'], r['lw_hd95'], r['lesions']) == (1.0, 0.0, [])
    r = _check_case(empty, one, [1], hip_device)
    assert (r['lw_dice'], r['lw_hd95'], r['n_fp']) == (0.0, 374.0, 1)
    r = _check_case(C.fn_fp_tp()[0], empty, [1], hip_device, dilation_iters=0)
    assert (r['n_gt'], r['n_fn'], r['n_tp'], r['lw_dice'], r['lw_hd95']) == (2, 2, 0, 0.0, 374.0)


def test_dropped_lesion_keeps_its_match(hip_device):
    gt, seg = C.small_and_large()
    r = _check_case(gt, seg, [1], hip_device, dilation_iters=0, min_lesion_voxels=2)
    assert (r['n_gt'], r['n_tp'], r['n_fn'], r['n_fp'], r['lw_dice'], r['lw_hd95']) == (1, 1, 0, 0, 1.0, 0.0)


@pytest.mark.parametrize('shape', [C.SHAPE_B, C.SHAPE_A, C.SHAPE_2D])
@pytest.mark.parametrize('iters', [1, 3])
def test_blobs_on_every_face(hip_device, shape, iters):
    gt, seg = C.faces(shape)
    _check_case(gt, seg, [1], hip_device, dilation_iters=iters)


# ---- case 9: many components, scan blocks, the sizes capacity --------------------------------------------------------------------
def _abi_ccl(mask, shape, capacity, device):
    """seg3d_ccl26_label with guard words round the sizes array: (ids, (K, status), sizes incl. guards)"""
    from segmentation3d import _engine as E
    Z, Y, X = shape
    n = Z * Y * X
    ids = torch.empty(n, dtype=torch.int32, device=device)
    count = torch.full((2 + 4,), _GUARD, dtype=torch.int32, device=device)
    sizes = torch.full((4 + capacity + 4,), _GUARD, dtype=torch.int32, device=device)
    work = torch.empty(E.query('seg3d_ccl26_label_workspace_ints', n), dtype=torch.int32, device=device)
    E.call('seg3d_ccl26_label', E.ptr(mask), X, Y, Z, E.ptr(ids), E.ptr(count), E.ptr(sizes[4:]), capacity, E.ptr(work),
           E.stream_ptr())
    return ids.cpu().numpy().reshape(shape), count.tolist(), sizes.tolist()


def test_lattice_numbering_sizes_and_capacity(hip_device):
    v = C.lattice()
    want_ids, k, want_sizes = O.components26(v)
    assert k == 2688 and want_sizes == [1] * k
    assert want_ids[0, 0, 3] == 2 and want_ids[0, 3, 0] == 17 and want_ids[3, 0, 0] == 16 * 14 + 1
    mask = _dev(v, hip_device).reshape(-1)
    ids, count, sizes = _abi_ccl(mask, v.shape, 4096, hip_device)
    assert count == [k, 0] + [_GUARD] * 4
    assert np.array_equal(ids, want_ids)
    assert sizes == [_GUARD] * 4 + [1] * k + [0] * (4096 - k) + [_GUARD] * 4
    ids, count, sizes = _abi_ccl(mask, v.shape, 100, hip_device)          # K > capacity: status set, nothing beyond
    assert count == [k, 1] + [_GUARD] * 4
    assert np.array_equal(ids, want_ids)
    assert sizes == [_GUARD] * 4 + [1] * 100 + [_GUARD] * 4
    from segmentation3d.utils import metrics as M
    old = M._CCL_CAPACITY
    M._CCL_CAPACITY = 64                                                       # the wrappers repeat with K
    try:
        got_ids, got_k, got_sizes = M.lesion_components(v, 1)
        r, = M.cal_lesionwise(v, v, [1], dilation_iters=0)
    finally:
        M._CCL_CAPACITY = old
    assert got_k == k and got_sizes == want_sizes and np.array_equal(got_ids.cpu().numpy(), want_ids)
    assert (r['n_gt'], r['n_tp'], r['n_fn'], r['n_fp'], r['lw_dice'], r['lw_hd95']) == (k, k, 0, 0, 1.0, 0.0)


# ---- case 10: the pair table overflows, the wrapper doubles it -------------------------------------------------------------------
def test_pair_table_overflow_and_doubling(hip_device):
    from segmentation3d import _engine as E
    from segmentation3d.utils import metrics as M
    v = C.lattice()
    ids, k, _ = O.components26(v)
    n = v.size
    dmap = _dev(ids, hip_device).reshape(-1)
    a = _dev(v, hip_device).reshape(-1)
    capacity = 1024                                                            # 2688 distinct pairs (i, i)
    words = torch.full((4 + 2 * (k + 1) + capacity + 4,), _GUARD, dtype=torch.int64, device=hip_device)
    words[4:-4] = 0
    status = torch.tensor([0, _GUARD], dtype=torch.int32, device=hip_device)
    gsize, inter, table = words[4:5 + k], words[5 + k:6 + 2 * k], words[6 + 2 * k:-4]
    for collapse in (1, 0):
        words[4:-4] = 0
        status[0] = 0
        E.call('seg3d_lesion_pairs', E.ptr(dmap), E.ptr(a), E.ptr(dmap), n, k, E.ptr(gsize), E.ptr(inter), E.ptr(table),
               capacity, collapse, E.ptr(status), E.stream_ptr())
        assert status.tolist() == [1, _GUARD]
        host = words.tolist()
        assert host[:4] == [_GUARD] * 4 and host[-4:] == [_GUARD] * 4
        assert gsize.tolist() == [0] + [1] * k and inter.tolist() == [0] + [1] * k      # the counts lose nothing
        keys = [x for x in table.tolist() if x]
        assert len(keys) == len(set(keys)) == capacity and all((x >> 32) == (x & 0xffffffff) for x in keys)
    got_g, got_i, pairs, _ = M.lesion_pair_table(dmap, a, dmap, k, capacity=capacity)
    assert got_g == [1] * k and got_i == [1] * k and pairs == [(i, i) for i in range(1, k + 1)]
    with pytest.raises(ValueError):
        E.call('seg3d_lesion_pairs', E.ptr(dmap), E.ptr(a), E.ptr(dmap), n, k, E.ptr(gsize), E.ptr(inter), E.ptr(table),
               1000, 1, E.ptr(status), E.stream_ptr())


# ---- case 11: iterations, dtypes, multi-id targets, anisotropic spacing ----------------------------------------------------------
@pytest.mark.parametrize('iters', [0, 1, 3, 16])
@pytest.mark.parametrize('shape', [C.SHAPE_A, C.SHAPE_2D])
def test_dilation_iterations(hip_device, iters, shape):
    from segmentation3d.utils import metrics as M
    v = C.random_sparse(shape, 3, 0.004)
    v[0, 0, 0] = v[-1, -1, -1] = 1
    got = M._dilate18(_dev(v, hip_device).reshape(-1), shape, iters).cpu().numpy().reshape(shape)
    assert set(np.unique(got).tolist()) <= {0, 1}
    assert np.array_equal(got != 0, O.dilate18(v, iters))


def test_dilate_abi_checks(hip_device):
    from segmentation3d import _engine as E
    m = torch.zeros(60, dtype=torch.uint8, device=hip_device)
    out = torch.zeros_like(m)
    for args in ((E.ptr(m), E.ptr(out), None, 5, 4, 3, 2), (E.ptr(m), E.ptr(out), None, 5, 4, 3, 17),
                 (E.ptr(m), E.ptr(m), None, 5, 4, 3, 1), (E.ptr(m), E.ptr(out), None, 5, 4, 3, -1)):
        with pytest.raises(ValueError):
            E.call('seg3d_binary_dilate18', *args, E.stream_ptr())
    assert E.query('seg3d_ccl26_label_workspace_ints', 2 ** 31) == -1


@pytest.mark.parametrize('dtype', [np.int8, np.uint8, np.int16, np.int32, np.float32])
def test_label_dtypes_and_multi_id_target(hip_device, dtype):
    from segmentation3d.utils import metrics as M
    gt = C.random_blobs(C.SHAPE_A, 7, count=10, labels=(1, 2, 4, 100))
    seg = C.perturbed(gt, 8)
    gt, seg = gt.astype(dtype), seg.astype(dtype)
    if dtype == np.float32:
        gt[0, 0, :4] = (1.5, -1.0, 256.0, 2.0)               # only the last is an integer in the set
    elif dtype in (np.int16, np.int32):
        gt[0, 0, :4] = (257, -1, 300, 2)
    kg, kp = _check_integers(gt, seg, [1, 2, 100], 1, hip_device)
    assert kg > 1 and kp > 1
    m = M._set_mask(_dev(gt, hip_device), [2]).cpu().numpy().reshape(gt.shape)
    if dtype in (np.float32, np.int16, np.int32):
        assert m[0, 0, :4].tolist() == [0, 0, 0, 1]
    got, = M.cal_lesionwise(gt, seg, [[1, 2, 100]], dilation_iters=1)
    _check_result(got, O.lesionwise(gt, seg, [1, 2, 100], _UNIT, dilation_iters=1), _UNIT)


def test_anisotropic_spacing_and_several_targets(hip_device):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.metrics import cal_lesionwise
    spacing = (0.7, 0.7, 2.5)
    gt = C.random_blobs(C.SHAPE_A, 11, count=9, labels=(1, 2))
    seg = C.perturbed(gt, 12)
    got = cal_lesionwise(gt, seg, [1, [2], (1, 2)], spacing=spacing, dilation_iters=2)
    assert len(got) == 3
    for r, target in zip(got, ([1], [2], [1, 2])):
        _check_result(r, O.lesionwise(gt, seg, target, spacing, dilation_iters=2), spacing)
    assert sum(r['n_tp'] for r in got) > 0
    dev = cal_lesionwise(_dev(gt, hip_device), _dev(seg, hip_device), [1, [2], (1, 2)], spacing=spacing, dilation_iters=2)
    img = cal_lesionwise(Image3d(gt, spacing=spacing), Image3d(seg, spacing=spacing), [1, [2], (1, 2)], dilation_iters=2)
    assert dev == got and img == got
    with pytest.raises(ValueError):
        cal_lesionwise(gt, seg[:-1], [1])
    with pytest.raises(ValueError):
        cal_lesionwise(gt, seg, [300])
    with pytest.raises(ValueError, match='spacing'):
        cal_lesionwise(Image3d(gt, spacing=spacing), Image3d(seg, spacing=(0.7, 0.7, 2.6)), [1])


# ---- case 12: run to run ---------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(hip_device):
    from segmentation3d.utils import metrics as M
    gt = C.random_blobs(C.SHAPE_A, 21, count=12, labels=(1,))
    seg = C.perturbed(gt, 22)
    runs = []
    for _ in range(2):
        ids, k, sizes = M.lesion_components(gt, 1, 2)
        r = M.cal_lesionwise(gt, seg, [1], spacing=(0.7, 0.7, 2.5))
        runs.append((ids.cpu().numpy().tobytes(), k, sizes, repr(r)))
    assert runs[0] == runs[1]


# ---- case 13: cal_dsc_batch through .mha files -----------------------------------------------------------------------------------
def _write_cases(root, spacing):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.image_io import write_image
    cases = []
    for i in range(2):
        gt = C.random_blobs(C.SHAPE_B, 31 + i, count=5, labels=(1, 2))
        seg = C.perturbed(gt, 41 + i)
        name = 'case{}'.format(i)
        for folder, vol in (('gt', gt), ('seg', seg)):
            os.makedirs(os.path.join(root, folder, name), exist_ok=True)
            write_image(Image3d(vol.astype(np.int16), spacing=spacing), os.path.join(root, folder, name, 'seg.mha'))
        cases.append((name, gt, seg))
    return cases


def test_cal_dsc_batch_lesionwise_columns(hip_device, tmp_path):
    from segmentation3d.core.seg_eval import cal_dsc_batch
    from segmentation3d import seg_eval
    from test_lesionwise import _parent_columns
    spacing = (0.8, 0.8, 2.0)
    root = str(tmp_path)
    cases = _write_cases(root, spacing)
    gts = [os.path.join(root, 'gt', n, 'seg.mha') for n, _, _ in cases]
    segs = [os.path.join(root, 'seg', n, 'seg.mha') for n, _, _ in cases]
    regions = [[1, 2], [2]]
    plain = cal_dsc_batch(gts, segs, [1, 2], 1, str(tmp_path / 'plain.csv'), regions=regions)
    assert list(plain.columns) == _parent_columns([1, 2], False, regions)
    surf = cal_dsc_batch(gts, segs, [1, 2], 1, None, surface_metrics=True, regions=regions)
    assert list(surf.columns) == _parent_columns([1, 2], True, regions)
    lst = tmp_path / 'test.txt'
    lst.write_text('{}\n'.format(len(cases)) + ''.join('{} {}\n'.format(n, g) for (n, _, _), g in zip(cases, gts)))
    out = tmp_path / 'lw.csv'
    full = seg_eval.main(['-i', str(lst), '--gt_folder', os.path.join(root, 'gt'), '--seg_folder', os.path.join(root, 'seg'),
                          '-l', '1', '2', '-t', '1', '-o', str(out), '--lesionwise', '--regions', '1,2;2',
                          '--lesion_dilation', '1', '--hd95_penalty', '50'])
    lw = ['lw_dice', 'lw_hd95', 'n_gt', 'n_fn', 'n_fp', 'lesion_f1']
    assert list(full.columns) == (['filename'] + [c for l in (1, 2) for c in
                                                  ['label{}_score'.format(l), 'label{}_type'.format(l)]
                                                  + ['label{}_{}'.format(l, k) for k in lw]]
                                  + [c for r in (0, 1) for c in ['region{}_score'.format(r), 'region{}_type'.format(r)]
                                     + ['region{}_{}'.format(r, k) for k in lw]])
    assert full[list(plain.columns)].equals(plain)                         # the old columns hold what they held
    table = pd.read_csv(str(out), index_col=0)
    assert len(table) == len(cases) + 2
    for prefix, target in (('label1', [1]), ('label2', [2]), ('region0', [1, 2]), ('region1', [2])):
        wants = [O.lesionwise(gt, seg, target, spacing, dilation_iters=1, hd95_penalty=50.0) for _, gt, seg in cases]
        for k in lw:
            col = '{}_{}'.format(prefix, k)
            values = table[col].astype(float).values
            for row, want in enumerate(wants):
                tol = _REL * abs(want[k]) if k == 'lw_hd95' else 1e-12
                assert abs(values[row] - want[k]) <= tol, (col, row)
            assert values[len(cases)] == pytest.approx(np.mean(values[:len(cases)]), rel=1e-12, abs=1e-15)
            assert values[len(cases) + 1] == pytest.approx(np.std(values[:len(cases)], ddof=1), rel=1e-9, abs=1e-15)


# ---- case 14: normalized surface Dice --------------------------------------------------------------------------------------------
def test_nsd(hip_device):
    from segmentation3d.utils.metrics import cal_surface_distances
    gt = C.random_blobs(C.SHAPE_A, 51, count=8, labels=(1, 2))
    seg = C.perturbed(gt, 52)
    r, = cal_surface_distances(gt, gt.copy(), [1], nsd_tolerance=0.0)
    assert r['nsd'] == 1.0 and r['hd'] == 0.0
    far_a, far_b = np.zeros(C.SHAPE_A, np.uint8), np.zeros(C.SHAPE_A, np.uint8)
    far_a[1:4, 1:4, 1:4] = 1
    far_b[25:30, 12:18, 10:15] = 1
    r, = cal_surface_distances(far_a, far_b, [1], nsd_tolerance=0.5)
    assert r['nsd'] == 0.0
    one_a, one_b = C.halo_only()                                            # every distance is exactly 1
    assert cal_surface_distances(one_a, one_b, [1], nsd_tolerance=1.0)[0]['nsd'] == 1.0
    assert cal_surface_distances(one_a, one_b, [1], nsd_tolerance=0.999)[0]['nsd'] == 0.0
    for tau in (0.0, 1.0, 2.0, 3.0):                                        # integer tolerances: ties at d = tau
        got = cal_surface_distances(gt, seg, [1, 2, 3], nsd_tolerance=tau)
        for label, g in zip((1, 2, 3), got):
            want = O.nsd(gt, seg, label, _UNIT, tau)
            print('nsd label {} tau {}: got {!r} want {!r}'.format(label, tau, g['nsd'], want))
            assert (math.isnan(want) and math.isnan(g['nsd']) and math.isnan(g['hd95'])) or g['nsd'] == want
    spacing = (0.7, 0.7, 2.5)
    got, = cal_surface_distances(gt, seg, [1], spacing, nsd_tolerance=1.9)
    want = O.nsd(gt, seg, 1, spacing, 1.9)
    print('nsd anisotropic: got {!r} want {!r}'.format(got['nsd'], want))
    assert abs(got['nsd'] - want) <= _REL * want
    plain = cal_surface_distances(gt, seg, [1, 3], spacing)
    assert all(set(p) == {'hd', 'hd95', 'assd'} for p in plain)             # the key is absent without a tolerance
    with_nsd = cal_surface_distances(gt, seg, [1, 3], spacing, nsd_tolerance=1.9)
    assert all({k: w[k] for k in p} == p or all(math.isnan(v) for v in p.values()) for p, w in zip(plain, with_nsd))
    with pytest.raises(ValueError):
        cal_surface_distances(gt, seg, [1], nsd_tolerance=-1.0)


def test_nsd_column_in_cal_dsc_batch(hip_device, tmp_path):
    from segmentation3d.core.seg_eval import cal_dsc_batch
    spacing = (0.8, 0.8, 2.0)
    root = str(tmp_path)
    cases = _write_cases(root, spacing)
    gts = [os.path.join(root, 'gt', n, 'seg.mha') for n, _, _ in cases]
    segs = [os.path.join(root, 'seg', n, 'seg.mha') for n, _, _ in cases]
    t = cal_dsc_batch(gts, segs, [1], 1, None, surface_metrics=True, nsd_tolerance=2.0)
    assert list(t.columns) == ['filename', 'label1_score', 'label1_type', 'label1_hd', 'label1_hd95', 'label1_assd',
                               'label1_nsd']
    for row, (_, gt, seg) in enumerate(cases):
        want = O.nsd(gt, seg, 1, spacing, 2.0)
        got = float(t['label1_nsd'].iloc[row])
        assert (math.isnan(want) and math.isnan(got)) or abs(got - want) <= _REL * want
    assert list(cal_dsc_batch(gts, segs, [1], 1, None, nsd_tolerance=2.0).columns) == [
        'filename', 'label1_score', 'label1_type']
