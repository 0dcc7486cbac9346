"""Region-based models, host side (no GPU): the region lookup table, every validation error, state-dict and checkpoint
keys, and the region columns of seg_eval against a numpy restatement (the device counting is replaced by numpy here; the
kernel itself is compared with numpy in tests/test_gpu_regions.py)."""
import types

import numpy as np
import pytest
import torch

import conftest  # noqa: F401

BRATS = [[1, 2, 3], [1, 3], [3]]


def _net(name, *args, **kw):
    import importlib
    return importlib.import_module('segmentation3d.network.' + name).SegmentationNet(*args, **kw)


# ---- lookup table ---------------------------------------------------------------------------------------------------------
def test_lut_of_overlapping_regions():
    from segmentation3d.loss.region_loss import region_lut
    lut = region_lut(BRATS)
    assert len(lut) == 256
    assert lut[0] == 0 and lut[1] == 0b011 and lut[2] == 0b001 and lut[3] == 0b111
    assert lut[7] == 0 and lut[255] == 0 and sum(1 for v in lut if v) == 3      # a label in no region: all-zero targets
    for l in range(256):
        for r, region in enumerate(BRATS):
            assert ((lut[l] >> r) & 1) == int(l in region)


def test_lut_of_sixteen_disjoint_and_nested_regions():
    from segmentation3d.loss.region_loss import region_lut
    regions = [[k + 1] for k in range(15)] + [[255, 1]]
    lut = region_lut(regions)
    assert lut[1] == (1 | 1 << 15) and lut[255] == 1 << 15 and lut[15] == 1 << 14 and lut[16] == 0
    assert max(lut) < 1 << 16
    # the order of the ids inside a region does not matter
    assert region_lut([[3, 1, 2], [3, 1], [3]]) == region_lut(BRATS)


@pytest.mark.parametrize('bad', [None, [], [[]], [[0]], [[1, 1]], [[256]], [[1.5]], [[-1]], [[1]] * 17, 'abc', [3], [[True]]])
def test_bad_regions_raise(bad):
    from segmentation3d.loss.region_loss import check_regions
    with pytest.raises(ValueError):
        check_regions(bad)


@pytest.mark.parametrize('bad', [None, [1, 2], [1, 2, 0], [1, 2, 128], [1, 2, 2.5], 'abc'])
def test_bad_region_class_order_raises(bad):
    from segmentation3d.loss.region_loss import check_region_class_order
    with pytest.raises(ValueError):
        check_region_class_order(bad, 3)
    assert check_region_class_order([2, 1, 3], 3) == [2, 1, 3]


# ---- network --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['vnet', 'vbnet'])
def test_sigmoid_network_keeps_the_state_dict_keys(name):
    from segmentation3d.network.module.layers import Sigmoid, Softmax
    plain, region = _net(name, 4, 3), _net(name, 4, 3, output_activation='sigmoid')
    a, b = plain.state_dict(), region.state_dict()
    assert list(a) == list(b) and all(a[k].shape == b[k].shape for k in a)
    assert isinstance(plain.out_block.softmax, Softmax) and not hasattr(plain.out_block, 'sigmoid')
    assert isinstance(region.out_block.sigmoid, Sigmoid) and not hasattr(region.out_block, 'softmax')
    assert plain.output_activation == 'softmax' and region.output_activation == 'sigmoid'
    assert list(Sigmoid().parameters()) == []
    region.load_state_dict(a)


def test_network_option_errors():
    from segmentation3d.network.module.vnet_outblock import OutputBlock
    with pytest.raises(ValueError, match='tanh'):
        OutputBlock(32, 3, activation='tanh')
    for name in ('vnet', 'vbnet'):
        with pytest.raises(ValueError, match='tanh'):
            _net(name, 1, 2, output_activation='tanh')
        with pytest.raises(ValueError, match='deep supervision'):
            _net(name, 1, 3, deep_supervision=1, output_activation='sigmoid')


# ---- checkpoint -----------------------------------------------------------------------------------------------------------
def _cfg(num_classes):
    return types.SimpleNamespace(dataset=types.SimpleNamespace(spacing=[1, 1, 1], interpolation='LINEAR',
                                                                num_classes=num_classes, crop_normalizers=[None]),
                                 net=types.SimpleNamespace(name='vnet'))


def test_checkpoint_round_trip_of_the_region_keys(tmp_path):
    from segmentation3d.utils.model_io import checkpoint_state, checkpoint_regions, load_checkpoint, region_keys
    net = _net('vnet', 4, 3, output_activation='sigmoid')
    state = checkpoint_state(net, 7, 9, _cfg(3), 16, 4, regions=BRATS, region_class_order=[2, 1, 3])
    assert state['regions'] == BRATS and state['region_class_order'] == [2, 1, 3] and state['output_activation'] == 'sigmoid'
    assert state['in_channels'] == 4 and state['out_channels'] == 3
    folder = tmp_path / 'checkpoints' / 'chk_7'
    folder.mkdir(parents=True)
    torch.save(state, str(folder / 'params.pth'))
    assert checkpoint_regions(7, str(tmp_path)) == (BRATS, [2, 1, 3], 'sigmoid')
    # a network rebuilt from the keys takes the checkpoint; a soft-max network refuses it
    again = _net('vnet', 4, 3, output_activation=checkpoint_regions(7, str(tmp_path))[2])
    assert load_checkpoint(7, again, None, str(tmp_path)) == (7, 9)
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in net.state_dict().items())
    with pytest.raises(ValueError, match='output_activation'):
        load_checkpoint(7, _net('vnet', 4, 3), None, str(tmp_path))
    # an old-style checkpoint (no keys) means soft-max
    plain = checkpoint_state(_net('vnet', 1, 2), 1, 2, _cfg(2), 16, 1)
    assert (plain['regions'], plain['region_class_order'], plain['output_activation']) == (None, None, 'softmax')
    for key in ('regions', 'region_class_order', 'output_activation'):
        del plain[key]
    assert region_keys(plain) == (None, None, 'softmax')
    old = tmp_path / 'checkpoints' / 'chk_1'
    old.mkdir(parents=True)
    torch.save(plain, str(old / 'params.pth'))
    assert checkpoint_regions(1, str(tmp_path)) == (None, None, 'softmax')
    assert load_checkpoint(1, _net('vnet', 1, 2), None, str(tmp_path)) == (1, 2)
    with pytest.raises(ValueError, match='output_activation'):
        load_checkpoint(1, _net('vnet', 1, 2, output_activation='sigmoid'), None, str(tmp_path))


# ---- evaluation -----------------------------------------------------------------------------------------------------------
def _numpy_region_counts(gt, seg, regions):
    return [(int(np.isin(gt, r).sum()), int(np.isin(seg, r).sum()), int((np.isin(gt, r) & np.isin(seg, r)).sum()))
            for r in regions]


def test_seg_eval_region_columns(tmp_path, monkeypatch):
    """cal_dsc_batch(..., regions=...) on two tiny cases, with the device counting replaced by its numpy restatement:
    column names and order, TP / FN / TN typing by the threshold, the Dice values and the mean / std rows"""
    from segmentation3d.core import seg_eval
    from segmentation3d.utils import metrics
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    def classify(gt, seg, sets, threshold):
        return [metrics._classify(a, b, c, threshold) for a, b, c in _numpy_region_counts(gt.array, seg.array, sets)]
    monkeypatch.setattr(seg_eval, 'cal_region_dsc', classify)
    monkeypatch.setattr(seg_eval, 'cal_dsc_labels', lambda gt, seg, labels, threshold: classify(gt, seg, [[l] for l in labels],
                                                                                              threshold))
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    rng = np.random.RandomState(3)
    gts, segs, paths = [], [], ([], [])
    for k in range(2):
        gt = rng.randint(0, 4, size=(6, 7, 8)).astype(np.uint8)
        seg = gt.copy()
        seg[rng.rand(*gt.shape) < 0.3] = 2
        if k == 1:                      # case 1: no label 3 in the ground truth, two voxels of it in the segmentation
            gt[gt == 3] = 0
            seg[seg == 3] = 0
            seg[0, 0, :2] = 3
        gts.append(gt)
        segs.append(seg)
        for which, arr in ((0, gt), (1, seg)):
            path = str(tmp_path / '{}{}.mha'.format('gs'[which], k))
            write_mha(Image3d(arr, *frame), path)
            paths[which].append(path)
    table = seg_eval.cal_dsc_batch(paths[0], paths[1], [1, 2], 5, str(tmp_path / 'out.csv'), regions=BRATS)
    assert list(table.columns) == ['filename', 'label1_score', 'label1_type', 'label2_score', 'label2_type',
                                   'region0_score', 'region0_type', 'region1_score', 'region1_type',
                                   'region2_score', 'region2_type']
    assert len(table) == 4 and list(table['filename'])[2:] == ['mean', 'std']
    for k in range(2):
        for r, region in enumerate(BRATS):
            g, s = np.isin(gts[k], region), np.isin(segs[k], region)
            if g.sum() < 5 and s.sum() < 5:
                want = (1.0, 'TN')
            elif g.sum() < 5:
                want = (0.0, 'FP')
            elif s.sum() < 5:
                want = (0.0, 'FN')
            else:
                want = (2.0 * (g & s).sum() / (g.sum() + s.sum()), 'TP')
            assert table['region{}_type'.format(r)].iloc[k] == want[1]
            assert table['region{}_score'.format(r)].iloc[k] == pytest.approx(want[0], abs=1e-12)
    assert table['region2_type'].iloc[1] == 'TN' and table['region0_type'].iloc[0] == 'TP'
    assert table['region0_type'].iloc[2] == 'ignore_type'
    assert table['region0_score'].iloc[2] == pytest.approx(np.mean(list(table['region0_score'].iloc[:2])))
    # without regions the table is the one it always was
    plain = seg_eval.cal_dsc_batch(paths[0], paths[1], [1, 2], 5, None)
    assert list(plain.columns) == list(table.columns)[:5]
    assert plain.iloc[:, 1:].equals(table.iloc[:, 1:5])


def test_seg_eval_cli_parses_regions():
    from segmentation3d.seg_eval import build_parser, parse_regions
    assert parse_regions('1,2,3;1,3;3') == BRATS and parse_regions(None) is None
    with pytest.raises(ValueError):
        parse_regions('1,2;x')
    args = build_parser().parse_args(['-i', 'a.txt', '--gt_folder', 'g', '--seg_folder', 's', '-l', '1', '--regions', '1,2;2'])
    assert parse_regions(args.regions) == [[1, 2], [2]]
