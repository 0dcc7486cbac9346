"""Compact resident training cases, host side: the storage_dtype table, the checks of the two
`dataset` keys and their defaults -- no GPU needed."""
import inspect
import os

import numpy as np
import pytest

from conftest import GOLDEN, PKG


def _full(dtype, lo, hi):
    a = np.zeros((3, 4, 5), dtype=dtype)
    a[0, 0, 0], a[2, 3, 4] = lo, hi
    return a


@pytest.mark.parametrize('array, want', [
    (_full(np.int16, -32768, 32767), np.int16),          # an int16 file
    (_full(np.uint8, 0, 255), np.int16),                 # a uint8 image
    (_full(np.int8, -128, 127), np.int16),
    (_full(np.uint16, 0, 32767), np.int16),
    (_full(np.uint16, 0, 32768), np.float32),            # one above: not exact in an int16
    (_full(np.int32, -32768, 32767), np.int16),
    (_full(np.int32, -32769, 0), np.float32),
    (_full(np.float32, 0.0, 1.0), np.float32),           # a float file, whatever it holds
    (_full(np.float64, 0.0, 1.0), np.float32),
])
def test_storage_dtype_of_an_image(array, want):
    from segmentation3d.utils.image_tools import storage_dtype
    assert storage_dtype(array, 'image') == np.dtype(want)


def test_storage_dtype_of_a_nifti_with_a_slope_is_float32():
    """_read_nifti has applied scl_slope / scl_inter: the int16 file arrives as floats"""
    from segmentation3d.utils.image_io import read_image
    from segmentation3d.utils.image_tools import storage_dtype, case_storage_dtype
    im = read_image(os.path.join(GOLDEN, 'images', 'sform_i16_slope.nii'), dtype=None)
    assert not np.issubdtype(im.array.dtype, np.integer)
    assert storage_dtype(im.array, 'image') == np.dtype(np.float32)
    assert case_storage_dtype([im]) == np.dtype(np.float32)


@pytest.mark.parametrize('array, want', [
    (_full(np.uint8, 0, 255), np.uint8),
    (_full(np.int16, 0, 255), np.uint8),
    (_full(np.int16, 0, 300), np.int16),
    (_full(np.int16, -1, 2), np.int16),
    (_full(np.int8, 0, 3), np.uint8),
    (_full(np.int32, 0, 70000), np.float32),
    (_full(np.float32, 0.0, 2.0), np.float32),
])
def test_storage_dtype_of_a_mask(array, want):
    from segmentation3d.utils.image_tools import storage_dtype
    assert storage_dtype(array, 'mask') == np.dtype(want)


def test_storage_dtype_kind_is_checked():
    from segmentation3d.utils.image_tools import storage_dtype
    with pytest.raises(ValueError):
        storage_dtype(_full(np.int16, 0, 1), 'label')


def test_one_modality_that_does_not_qualify_makes_the_case_float32():
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.image_tools import case_storage_dtype, images_to_host
    ok, bad = _full(np.int16, -1000, 3000), _full(np.uint16, 0, 40000)
    assert case_storage_dtype([Image3d(ok), Image3d(ok), Image3d(ok)]) == np.dtype(np.int16)
    assert case_storage_dtype([Image3d(ok), Image3d(bad), Image3d(ok)]) == np.dtype(np.float32)
    assert case_storage_dtype([Image3d(ok), Image3d(ok.astype(np.float32))]) == np.dtype(np.float32)
    # the channels-last host array of a compact case: np.stack(..., axis=-1), once
    host = images_to_host([Image3d(ok), Image3d((ok // 2).astype(np.uint8))], np.int16)
    assert host.dtype == np.int16 and host.shape == (3, 4, 5, 2) and host.flags['C_CONTIGUOUS']
    assert np.array_equal(host[..., 0], ok) and np.array_equal(host[..., 1], (ok // 2).astype(np.uint8))


@pytest.mark.parametrize('storage', ['FP32', 'int16', '', None, 16, b'compact'])
def test_unknown_storage_raises(storage):
    from segmentation3d.dataloader.dataset import validate_resident_options
    with pytest.raises(ValueError):
        validate_resident_options(storage, None)


@pytest.mark.parametrize('budget', [0, 0.0, -1, -0.5, float('inf'), float('-inf'), float('nan'), '4', [4], True])
def test_bad_budget_raises(budget):
    from segmentation3d.dataloader.dataset import validate_resident_options
    with pytest.raises(ValueError):
        validate_resident_options('compact', budget)


def test_valid_options_pass():
    from segmentation3d.dataloader.dataset import validate_resident_options
    assert validate_resident_options('fp32', None) == ('fp32', None)
    assert validate_resident_options('compact', None) == ('compact', None)
    assert validate_resident_options('compact', 2) == ('compact', 2e9)
    assert validate_resident_options('fp32', np.float32(0.5)) == ('fp32', 0.5e9)


def test_defaults_are_todays_behaviour():
    """the constructor defaults, and a shipped config that has neither key"""
    from segmentation3d.dataloader.dataset import SegmentationDataset
    params = inspect.signature(SegmentationDataset.__init__).parameters
    assert params['resident_storage'].default == 'fp32'
    assert params['resident_budget_gb'].default is None
    text = open(os.path.join(PKG, 'segmentation3d', 'config', 'train_config.py')).read()
    assert 'resident_storage' not in text and 'resident_budget_gb' not in text
    from segmentation3d.utils.file_io import load_config
    cfg = load_config(os.path.join(PKG, 'segmentation3d', 'config', 'train_config.py'))
    assert not hasattr(cfg.dataset, 'resident_storage') and not hasattr(cfg.dataset, 'resident_budget_gb')


def test_compact_case_on_the_host_device(tmp_path):
    """loading a single-modality case launches nothing, so the storage of a case can be seen without a GPU"""
    import torch
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.image_io import write_image
    rng = np.random.RandomState(2)
    image = rng.randint(-1000, 3000, size=(6, 7, 8)).astype(np.int16)
    write_image(Image3d(image), str(tmp_path / 'org.mha'))
    write_image(Image3d((rng.rand(6, 7, 8) > 0.5).astype(np.uint8)), str(tmp_path / 'seg.mha'))
    (tmp_path / 'train.txt').write_text('1\n{}\n{}\n'.format(tmp_path / 'org.mha', tmp_path / 'seg.mha'))

    def dataset(**kw):
        return SegmentationDataset(str(tmp_path / 'train.txt'), 2, [1, 1, 1], [4, 4, 4], 'GLOBAL', [0, 0, 0], [1, 1], 'LINEAR',
                                   [None], device=torch.device('cpu'), **kw)
    plain, compact = dataset(), dataset(resident_storage='compact')
    a, b = plain.case(0), compact.case(0)
    assert a.volume.dtype == torch.float32 and a.seg.dtype == torch.float32 and a.nbytes == 6 * 7 * 8 * 8
    assert b.volume.dtype == torch.int16 and b.seg.dtype == torch.uint8 and b.nbytes == 6 * 7 * 8 * 3
    assert torch.equal(b.volume.float(), a.volume) and torch.equal(b.seg.float(), a.seg)
    assert np.array_equal(a.seg_host, b.seg_host) and not a.staged and not b.staged
    assert plain.resident_bytes() == a.nbytes and compact.resident_bytes() == b.nbytes
    assert compact.num_staged() == 0 and not compact.has_budget()


def test_typed_entries_are_bound():
    """the two new C entries are in the ctypes table (tests/test_abi.py compares the table with the header)"""
    from segmentation3d import _engine as E
    assert 'seg3d_resample_affine_typed_mc' in E.symbols() and 'seg3d_resample_deform_typed_mc' in E.symbols()
