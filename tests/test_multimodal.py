"""Multi-modality input (several co-registered images per case), host side: list formats, 4-D NIfTI reading, and the
checks that name a case -- no GPU needed."""
import gzip
import struct

import numpy as np
import pytest
import torch

import conftest  # noqa: F401  (sys.path)

_LPS = np.diag([-1.0, -1.0, 1.0])


def write_nifti_4d(path, planes, spacing, origin, direction, order='<'):
    """assemble a NIfTI-1 file byte by byte: planes [M, Z, Y, X] float32, dim = (4, X, Y, Z, M), sform holding the LPS
    frame (spacing, origin, row-major direction) converted to RAS"""
    planes = np.asarray(planes, dtype=np.float32)
    M, Z, Y, X = planes.shape
    rot = _LPS @ np.asarray(direction, dtype=np.float64).reshape(3, 3) * np.asarray(spacing, dtype=np.float64)
    offset = _LPS @ np.asarray(origin, dtype=np.float64)
    hdr = bytearray(352)
    struct.pack_into(order + 'i', hdr, 0, 348)
    struct.pack_into(order + '8h', hdr, 40, 4, X, Y, Z, M, 1, 1, 1)
    struct.pack_into(order + 'hh', hdr, 70, 16, 32)
    struct.pack_into(order + '8f', hdr, 76, 1.0, spacing[0], spacing[1], spacing[2], 1.0, 0.0, 0.0, 0.0)
    struct.pack_into(order + 'f', hdr, 108, 352.0)
    struct.pack_into(order + '2f', hdr, 112, 1.0, 0.0)
    struct.pack_into(order + '2h', hdr, 252, 0, 1)
    for r in range(3):
        struct.pack_into(order + '4f', hdr, 280 + 16 * r, rot[r, 0], rot[r, 1], rot[r, 2], offset[r])
    hdr[344:348] = b'n+1\x00'
    opener = gzip.open if str(path).endswith('.gz') else open
    with opener(str(path), 'wb') as f:
        f.write(bytes(hdr))
        f.write(planes.astype(np.dtype(np.float32).newbyteorder(order)).tobytes())


def _oblique(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def _touch(path):
    path.write_bytes(b'')
    return str(path)


@pytest.mark.parametrize('order', ['<', '>'])
def test_read_4d_nifti_modalities_both_byte_orders(tmp_path, order):
    from segmentation3d.utils.image_io import read_image, read_image_modalities, num_modalities
    rng = np.random.RandomState(3)
    planes = rng.randn(3, 5, 6, 7).astype(np.float32)
    spacing, origin, direction = (0.8, 1.25, 2.0), (-12.5, 30.0, 4.0), _oblique(30.0).ravel()
    path = tmp_path / ('brats.nii.gz' if order == '<' else 'brats.nii')
    write_nifti_4d(path, planes, spacing, origin, direction, order)
    assert num_modalities(str(path)) == 3
    ims = read_image_modalities(str(path))
    assert len(ims) == 3
    for m, im in enumerate(ims):
        assert im.array.dtype == np.float32 and im.array.shape == (5, 6, 7)
        assert np.array_equal(im.array, planes[m])
        assert im.GetSize() == (7, 6, 5)
        assert np.allclose(im.GetSpacing(), spacing, atol=1e-6)
        assert np.allclose(im.GetOrigin(), origin, atol=1e-5)
        assert np.allclose(im.GetDirection(), direction, atol=1e-6)
    with pytest.raises(ValueError):
        read_image(str(path))                       # the 3-D reader keeps rejecting 4-D files


def test_read_image_modalities_of_3d_files(tmp_path):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.image_io import read_image, read_image_modalities, write_image, num_modalities
    a = np.arange(60, dtype=np.float32).reshape(3, 4, 5)
    for name in ('a.nii.gz', 'a.mha'):
        write_image(Image3d(a, (1.0, 2.0, 3.0), (1.0, 2.0, 3.0)), str(tmp_path / name))
        ims = read_image_modalities(str(tmp_path / name))
        assert len(ims) == 1 and num_modalities(str(tmp_path / name)) == 1
        ref = read_image(str(tmp_path / name))
        assert np.array_equal(ims[0].array, ref.array) and ims[0].GetSpacing() == ref.GetSpacing()


def test_train_txt_with_modality_count(tmp_path):
    from segmentation3d.dataloader.dataset import read_train_txt
    files = {n: _touch(tmp_path / n) for n in ('c0_t1.mha', 'c0_t2.mha', 'c0_fl.mha', 'c0_seg.mha', 'c1_t1.mha',
                                                'c1_t2.mha', 'c1_fl.mha', 'c1_seg.mha')}
    lst = tmp_path / 'train.txt'
    lst.write_text('2 3\n' + '\n'.join(files[n] for n in sorted(files, key=lambda n: (n[:2], n.endswith('seg.mha')))) + '\n')
    ims, segs = read_train_txt(str(lst))
    assert len(ims) == 2 and all(isinstance(e, list) and len(e) == 3 for e in ims)
    assert segs == [files['c0_seg.mha'], files['c1_seg.mha']]
    assert all(p.startswith(str(tmp_path / 'c0_')) for p in ims[0])


def test_train_txt_with_4d_nifti_in_place_of_paths(tmp_path):
    from segmentation3d.dataloader.dataset import read_train_txt, SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    nii = tmp_path / 'case.nii.gz'
    write_nifti_4d(nii, np.zeros((4, 4, 4, 4), np.float32), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), np.eye(3).ravel())
    seg = _touch(tmp_path / 'seg.mha')
    for head in ('1', '1 4'):
        lst = tmp_path / 'train.txt'
        lst.write_text('{}\n{}\n{}\n'.format(head, nii, seg))
        ims, segs = read_train_txt(str(lst))
        assert ims == [str(nii)] and segs == [seg]
        ds = SegmentationDataset(str(lst), 2, [1, 1, 1], [16, 16, 16], 'GLOBAL', [0, 0, 0], [1, 1], 'LINEAR',
                                 [AdaptiveNormalizer()] * 4, device=torch.device('cpu'))
        assert ds.num_modality() == 4
    lst.write_text('1 3\n{}\n{}\n'.format(nii, seg))
    with pytest.raises(ValueError):
        read_train_txt(str(lst))                    # the list declares 3, the file holds 4


def test_legacy_lists_are_unchanged(tmp_path):
    from segmentation3d.dataloader.dataset import read_train_txt, read_train_csv, SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    a, b, c, d = (_touch(tmp_path / n) for n in ('a.mha', 'a_seg.mha', 'b.mha', 'b_seg.mha'))
    lst = tmp_path / 'train.txt'
    lst.write_text('2\n{}\n{}\n{}\n{}\n'.format(a, b, c, d))
    assert read_train_txt(str(lst)) == ([a, c], [b, d])
    csv = tmp_path / 'train.csv'
    csv.write_text('image_name,image_path,mask_path\nA,{},{}\nB,{},{}\n'.format(a, b, c, d))
    assert read_train_csv(str(csv)) == ([a, c], [b, d])
    assert read_train_csv(str(csv), 'test') == (['A', 'B'], [a, c])
    ds = SegmentationDataset(str(lst), 2, [1, 1, 1], [16, 16, 16], 'GLOBAL', [0, 0, 0], [1, 1], 'LINEAR',
                             [AdaptiveNormalizer()], device=torch.device('cpu'))
    assert ds.num_modality() == 1 and ds.im_list == [a, c]
    lst.write_text('2\n{}\n{}\n{}\n'.format(a, b, c))
    with pytest.raises(ValueError):
        read_train_txt(str(lst))


def test_train_csv_with_modality_columns(tmp_path):
    from segmentation3d.dataloader.dataset import read_train_csv
    p = {n: _touch(tmp_path / n) for n in ('a0.mha', 'a1.mha', 'as.mha', 'b0.mha', 'b1.mha', 'bs.mha')}
    csv = tmp_path / 'train.csv'
    csv.write_text('image_name,image_path,image_path_1,mask_path\nA,{},{},{}\nB,{},{},{}\n'.format(
        p['a0.mha'], p['a1.mha'], p['as.mha'], p['b0.mha'], p['b1.mha'], p['bs.mha']))
    ims, segs = read_train_csv(str(csv))
    assert ims == [[p['a0.mha'], p['a1.mha']], [p['b0.mha'], p['b1.mha']]] and segs == [p['as.mha'], p['bs.mha']]
    names, ims = read_train_csv(str(csv), 'test')
    assert names == ['A', 'B'] and ims[1] == [p['b0.mha'], p['b1.mha']]


def test_test_txt_with_several_paths_per_case(tmp_path):
    from segmentation3d.core.seg_infer import read_test_txt
    p = [_touch(tmp_path / 'm{}.mha'.format(k)) for k in range(5)]
    lst = tmp_path / 'test.txt'
    lst.write_text('2\ncaseA {} {} {}\ncaseB {}\n'.format(p[0], p[1], p[2], p[3]))
    names, paths = read_test_txt(str(lst))
    assert names == ['caseA', 'caseB'] and paths == [[p[0], p[1], p[2]], p[3]]


def test_mismatched_frames_name_the_case():
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.image_io import check_modalities
    a = np.zeros((4, 5, 6), np.float32)
    ok = [Image3d(a, (1.0, 1.0, 2.0), (3.0, 4.0, 5.0)), Image3d(a + 1, (1.0, 1.0, 2.0 * (1 + 1e-8)), (3.0, 4.0, 5.0))]
    check_modalities(ok, 'c0')                      # within the 1e-6 relative tolerance
    bad = [
        [Image3d(a), Image3d(np.zeros((4, 5, 7), np.float32))],
        [Image3d(a, (1.0, 1.0, 1.0)), Image3d(a, (1.0, 1.0, 1.1))],
        [Image3d(a, origin=(0.0, 0.0, 0.0)), Image3d(a, origin=(0.0, 0.5, 0.0))],
        [Image3d(a, direction=tuple(np.eye(3).ravel())), Image3d(a, direction=tuple(_oblique(5.0).ravel()))],
    ]
    for ims in bad:
        with pytest.raises(ValueError, match='case brats_007'):
            check_modalities(ims, 'brats_007')


def test_wrong_normalizer_count_raises(tmp_path):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    p = [_touch(tmp_path / n) for n in ('t1.mha', 't2.mha', 'seg.mha')]
    lst = tmp_path / 'train.txt'
    lst.write_text('1 2\n' + '\n'.join(p) + '\n')
    with pytest.raises(ValueError, match='t1.mha'):
        SegmentationDataset(str(lst), 2, [1, 1, 1], [16, 16, 16], 'GLOBAL', [0, 0, 0], [1, 1], 'LINEAR',
                            [AdaptiveNormalizer()], device=torch.device('cpu'))
    ds = SegmentationDataset(str(lst), 2, [1, 1, 1], [16, 16, 16], 'GLOBAL', [0, 0, 0], [1, 1], 'LINEAR',
                             [AdaptiveNormalizer(), None], device=torch.device('cpu'))
    assert ds.num_modality() == 2


def test_in_channels_must_equal_modalities():
    from segmentation3d.core.seg_infer import segmentation_volume, segmentation_voi
    from segmentation3d.utils.image3d import Image3d
    ims = [Image3d(np.zeros((16, 16, 16), np.float32)) for _ in range(3)]
    model = {'device': torch.device('cpu'), 'in_channels': 4, 'out_channels': 2, 'crop_normalizer_dicts': [None] * 4}
    with pytest.raises(ValueError, match='in_channels'):
        segmentation_volume(model, None, ims, None, None)
    with pytest.raises(ValueError, match='in_channels'):
        segmentation_voi(model, ims, [0, 0, 0], [16, 16, 16])


def test_normalizer_struct_and_workspace_query():
    from segmentation3d import _engine as E
    from segmentation3d.utils.image_tools import normalizer_params
    from segmentation3d.utils.normalizer import AdaptiveNormalizer, FixedNormalizer
    p = normalizer_params([FixedNormalizer(10.0, 4.0, False), AdaptiveNormalizer(2.5), None,
                           {'type': 0, 'mean': -1.0, 'stddev': 2.0, 'clip': True}], 4)
    got = [(p.n[m].type, p.n[m].mean, p.n[m].stddev, p.n[m].clip, p.n[m].clip_lo, p.n[m].clip_hi) for m in range(8)]
    assert got[:4] == [(0, 10.0, 4.0, 0, -1.0, 1.0), (1, 0.0, 1.0, 1, -2.5, 2.5), (-1, 0.0, 1.0, 0, -1.0, 1.0),
                       (0, -1.0, 2.0, 1, -1.0, 1.0)]
    assert all(g[0] == -1 for g in got[4:])
    with pytest.raises(ValueError):
        normalizer_params([None], 2)
    nblk = E.query('seg3d_patch_stats_blocks', 96, 96, 96)
    assert E.query('seg3d_patch_stats_mc_doubles', 96, 96, 96, 16, 4) == 16 * 4 * nblk * 2
