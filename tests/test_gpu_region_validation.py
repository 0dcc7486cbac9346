"""Region validation on the GPU: seg3d_region_confusion_counts (csrc/validation.hip) bit for bit against numpy boolean sums,
a Validator pass with regions against the same sums, and core/seg_train.train() on a toy multi-label data set with
`loss.regions`: log lines, checkpoints/best with the three region keys, a resume, and segmentation() composing a mask from the
trained checkpoint with its region_class_order.

One TrainStep exists at a time: every train() result is dropped, followed by gc.collect() and PACK_CACHE.clear(), before the
next is built."""
import gc
import json
import os
import shutil

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
from float64_util import Guarded, _engine
from oracle import detgen
from test_gpu_region_loss import NOWHERE, REGIONS, SHAPES, _inputs, _numel, _put
from test_region_loss import BRATS, region_targets

pytestmark = pytest.mark.gpu


def counts_ref(p, t, regions, ignore_label=None):
    """[R, 3] (tp, fp, fn) by numpy boolean sums; region r is predicted where p_r > 0.5, strictly, on counted voxels"""
    z, counted = region_targets(t, regions, ignore_label)
    z, counted = z.numpy(), counted.numpy()
    N, R = p.shape[0], p.shape[1]
    pred = (p.numpy().reshape(N, R, -1) > np.float32(0.5)) & counted[:, None, :]
    return np.stack([(pred & z).sum((0, 2)), (pred & ~z).sum((0, 2)), (~pred & z).sum((0, 2))], 1).astype(np.int64)


def _abi_counts(dev, p, t, regions, ignore_label, start, shift=0):
    from segmentation3d import _ops
    from segmentation3d.loss.region_loss import region_lut
    E = _engine()
    N, R, S = p.shape[0], p.shape[1], _numel(p.shape[2:])
    pd, td = _put(dev, p, shift), _put(dev, t, shift)
    out = Guarded(3 * R, 16, dev, dtype=torch.int64, fill=torch.from_numpy(start).to(dev))
    E.call('seg3d_region_confusion_counts', E.ptr(pd), E.ptr(td), _ops._region_table(region_lut(regions)), E.ptr(out.t), N, R, S,
           -1.0 if ignore_label is None else float(ignore_label), E.stream_ptr())
    torch.cuda.synchronize()
    assert out.guards_untouched()
    assert torch.equal(pd.cpu(), p.reshape(-1)) and torch.equal(td.cpu(), t.reshape(-1))
    return out.t.cpu().numpy().reshape(R, 3)


@pytest.mark.parametrize('shape', list(SHAPES))
@pytest.mark.parametrize('R', [1, 3, 16])
def test_counts_equal_numpy(hip_device, R, shape):
    """stray targets, p = 0.5 exactly (not predicted), accumulation into counts that are not zero; a 16-byte case a second
    time on the scalar path"""
    N = 3
    p, t = _inputs(7000 + R, N, R, SHAPES[shape])
    S = _numel(SHAPES[shape])
    flat = p.reshape(N, R, -1)
    for k in range(min(S, 6)):                        # exact 0.5 on targets of either kind
        flat[k % N, k % R, (7 * k) % S] = 0.5
    start = np.arange(3 * R, dtype=np.int64).reshape(R, 3) * 1000 + 7
    for ignore in (255, None, NOWHERE):
        want = start + counts_ref(p, t, REGIONS[R], ignore)
        for shift in [0] + ([1] if S % 4 == 0 else []):
            got = _abi_counts(hip_device, p, t, REGIONS[R], ignore, start, shift)
            assert np.array_equal(got, want), (ignore, shift, got.tolist(), want.tolist())
    # p = 0.5 everywhere predicts nothing: fp = 0 and tp = 0 for every region
    half = torch.full_like(p, 0.5)
    got = _abi_counts(hip_device, half, t, REGIONS[R], 255, np.zeros((R, 3), np.int64))
    assert np.array_equal(got, counts_ref(half, t, REGIONS[R], 255)) and int(got[:, :2].sum()) == 0


def test_counts_through_python_accumulate_and_an_uncounted_batch_adds_nothing(hip_device):
    from segmentation3d import _ops
    from segmentation3d.loss.region_loss import region_lut
    p, t = _inputs(7100, 3, 3, SHAPES['33x32x32'])
    lut = region_lut(BRATS)
    pd, td = p.to(hip_device), t.to(hip_device)
    first = _ops.region_confusion_counts(pd, td, lut, 255)
    assert first.dtype == torch.int64 and tuple(first.shape) == (3, 3)
    want = counts_ref(p, t, BRATS, 255)
    assert np.array_equal(first.cpu().numpy(), want)
    again = _ops.region_confusion_counts(pd, td, lut, 255, out=first)
    assert again is first and np.array_equal(first.cpu().numpy(), 2 * want)
    nothing = torch.full_like(t, 255.0)
    nothing.reshape(3, -1)[:, :4] = torch.tensor([-1.0, 1.5, 256.0, 300.0])
    _ops.region_confusion_counts(pd, nothing.to(hip_device), lut, 255, out=first)
    assert np.array_equal(first.cpu().numpy(), 2 * want)
    assert int(_ops.region_confusion_counts(pd, nothing.to(hip_device), lut, 255).abs().sum()) == 0
    for bad in (dict(out=torch.zeros((3, 3), dtype=torch.int32, device=hip_device)),
                dict(out=torch.zeros((2, 3), dtype=torch.int64, device=hip_device))):
        with pytest.raises(ValueError):
            _ops.region_confusion_counts(pd, td, lut, 255, **bad)
    with pytest.raises(ValueError):
        _ops.region_confusion_counts(pd, td, lut[:-1], 255)
    with pytest.raises(ValueError):
        _engine().call('seg3d_region_confusion_counts', _engine().ptr(pd), _engine().ptr(td), _ops._region_table(lut),
                       _engine().ptr(first), 3, 17, 8, -1.0, _engine().stream_ptr())


def _clear():
    from segmentation3d import _ops
    gc.collect()
    _ops.PACK_CACHE.clear()


def test_validator_pass_with_regions(hip_device):
    """5 crops in batches of 2, 2 and 1 through a sigmoid vnet: counts, Dice list, mean over all R regions and the loss are
    those of numpy on the probabilities of the same batches"""
    from segmentation3d.core.seg_validate import Validator
    from segmentation3d.loss.region_loss import RegionDiceBCELoss
    from segmentation3d.network import vnet
    torch.manual_seed(11)
    net = vnet.SegmentationNet(1, 3, output_activation='sigmoid')
    vnet.parameters_kaiming_init(net)
    net = net.to(hip_device)
    edge = net.max_stride()
    g = torch.Generator().manual_seed(12)
    masks = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0, 255.0])[torch.randint(0, 6, (5, 1, edge, edge, edge), generator=g)]
    crops = (masks.clamp(max=4.0) / 2.0 - 1.0 + 0.5 * torch.randn(masks.shape, generator=g)).float()
    v = Validator(net, RegionDiceBCELoss(BRATS, ignore_label=255), crops.to(hip_device), masks.to(hip_device), 2,
                  ignore_label=255, ema=0.5, regions=BRATS)
    result = v.run(1)
    want, loss_sum = np.zeros((3, 3), np.int64), 0.0
    loss_fn = RegionDiceBCELoss(BRATS, ignore_label=255)
    with torch.no_grad():
        for b in range(0, 5, 2):
            x, t = crops[b:b + 2].to(hip_device), masks[b:b + 2].to(hip_device)
            probs = net(x)
            loss_sum += float(loss_fn(probs, t)) * int(x.shape[0])
            want += counts_ref(probs.cpu(), masks[b:b + 2], BRATS, 255)
    assert np.array_equal(v.counts.cpu().numpy(), want)
    dice = [2.0 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else float('nan') for tp, fp, fn in want.tolist()]
    assert len(result['dice']) == 3 and all(a == b or (np.isnan(a) and np.isnan(b)) for a, b in zip(result['dice'], dice))
    finite = [d for d in dice if not np.isnan(d)]
    assert finite and result['mean_dice'] == sum(finite) / len(finite)          # region 0 is not left out as a background
    assert abs(result['val_loss'] - loss_sum / 5) < 1e-6 and result['ema_dice'] == result['mean_dice'] and result['improved']
    with pytest.raises(ValueError):                                             # a network with another number of outputs
        Validator(net, loss_fn, crops.to(hip_device), masks.to(hip_device), 2, regions=[[1], [2]]).run(1)
    del v, net
    _clear()


# ---- train() with loss.regions ----------------------------------------------------------------------------------------------------
_CFG = '''
from easydict import EasyDict as edict
from segmentation3d.utils.normalizer import AdaptiveNormalizer
__C = edict()
cfg = __C
__C.general = {{}}
__C.general.imseg_list = '{train}'
__C.general.save_dir = '{save}'
__C.general.model_scale = 'coarse'
__C.general.resume_epoch = {resume}
__C.general.num_gpus = 1
__C.general.seed = 0
__C.dataset = {{}}
__C.dataset.num_classes = 4
__C.dataset.spacing = [1.0, 1.0, 1.0]
__C.dataset.crop_size = [32, 32, 32]
__C.dataset.sampling_method = 'GLOBAL'
__C.dataset.random_translation = [2, 2, 2]
__C.dataset.random_scale = [0.95, 1.05]
__C.dataset.interpolation = 'LINEAR'
__C.dataset.crop_normalizers = [AdaptiveNormalizer()]
__C.loss = {{}}
__C.loss.name = 'RegionDiceBCE'
__C.loss.obj_weight = [1.0, 1.0, 1.0]
__C.loss.focal_gamma = 2
__C.loss.regions = [[1, 2, 3], [1, 3], [3]]
__C.loss.region_class_order = [2, 1, 3]
__C.net = {{}}
__C.net.name = 'vnet'
__C.train = {{}}
__C.train.epochs = {epochs}
__C.train.batchsize = 2
__C.train.num_threads = 0
__C.train.lr = 1e-3
__C.train.betas = (0.9, 0.999)
__C.train.save_epochs = 2
__C.validation = {{}}
__C.validation.imseg_list = '{val}'
__C.validation.crops_per_case = 2
__C.validation.ema = 0.5
'''

_INFER_CFG = """from easydict import EasyDict as edict
__C = edict()
cfg = __C
__C.general = {}
__C.general.single_scale = 'coarse'
__C.coarse = {}
__C.coarse.model_name = 'coarse'
__C.coarse.checkpoint = 'best'
__C.coarse.pick_largest_cc = False
__C.coarse.remove_small_cc = 0
__C.coarse.partition_type = 'SIZE'
__C.coarse.partition_size = [32.0, 32.0, 32.0]
__C.coarse.partition_stride = [16.0, 16.0, 16.0]
"""


def _write_cases(folder, first, count):
    """learnable multi-label toy cases: labels 0..3, the image is the label map plus noise"""
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    paths = []
    for k in range(first, first + count):
        os.makedirs(str(folder / 'c{}'.format(k)), exist_ok=True)
        seg = detgen.labels(900 + k, 'region/seg{}'.format(k), (48, 48, 48), 4).astype(np.int8)
        img = (seg.astype(np.float32) / 1.5 - 1.0 + 0.3 * detgen.normal(910 + k, 'region/n{}'.format(k), (48, 48, 48))).astype(np.float32)
        ip, sp = str(folder / 'c{}'.format(k) / 'org.mha'), str(folder / 'c{}'.format(k) / 'seg.mha')
        write_mha(Image3d(img, *frame), ip)
        write_mha(Image3d(seg, *frame), sp)
        paths += [ip, sp]
    return paths


def _run(root, name, epochs, resume=-1):
    import random
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import train
    save = root / name
    os.makedirs(str(save), exist_ok=True)
    cfg = save / 'cfg.py'
    cfg.write_text(_CFG.format(train=str(root / 'train.txt'), val=str(root / 'val.txt'), save=str(save), resume=resume,
                               epochs=epochs))
    random.seed(0)
    try:
        step = train(str(cfg))
    finally:
        _ops.set_activation_dtype('fp32')
    log = (save / 'coarse' / 'train_log.txt').read_text().strip().splitlines()
    return step, [l for l in log if 'train_loss' in l], [l for l in log if 'val_' in l], save / 'coarse'


def test_train_with_regions_end_to_end(hip_device, tmp_path):
    from segmentation3d.core.seg_infer import load_single_model, segmentation
    from segmentation3d.loss.region_loss import RegionDiceBCELoss
    from segmentation3d.utils.image_io import read_image
    root = tmp_path
    train_paths, val_paths = _write_cases(root, 0, 2), _write_cases(root, 2, 2)
    (root / 'train.txt').write_text('2\n' + '\n'.join(train_paths) + '\n')
    (root / 'val.txt').write_text('2\n' + '\n'.join(val_paths) + '\n')
    step, train_lines, val_lines, folder = _run(root, 'run', 6)
    assert isinstance(step.loss_func, RegionDiceBCELoss) and step.net.output_activation == 'sigmoid'
    assert step.regions == BRATS and step.region_class_order == [2, 1, 3] and step.validator.regions == BRATS
    assert isinstance(step.validator.loss_func, RegionDiceBCELoss) and step.validator.loss_func is not step.loss_func
    losses = [float(l.split('train_loss: ')[1].split(',')[0]) for l in train_lines]
    assert len(losses) == 6 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert [int(l.split('epoch: ')[1].split(',')[0]) for l in val_lines] == [1, 2, 3, 4, 5]
    for line in val_lines:
        assert all(key in line for key in ('val_loss: ', 'val_dice: ', 'val_dice_ema: ', 'val_dice_per_class: ['))
        per = [float(v) for v in line.split('val_dice_per_class: [')[1].rstrip(']').split(', ')]
        assert len(per) == 3                                                      # one value per region
        finite = [v for v in per if not np.isnan(v)]
        assert abs(float(line.split('val_dice: ')[1].split(',')[0]) - sum(finite) / len(finite)) < 1.01e-4
    best = folder / 'checkpoints' / 'best'
    record = json.loads((best / 'validation.json').read_text())
    assert set(record) == {'epoch', 'batch', 'val_loss', 'dice', 'mean_dice', 'ema_dice', 'improved'} and len(record['dice']) == 3
    for chk in (best, folder / 'checkpoints' / 'chk_4'):
        state = torch.load(str(chk / 'params.pth'), map_location='cpu', weights_only=True)
        assert state['regions'] == BRATS and state['region_class_order'] == [2, 1, 3] and state['output_activation'] == 'sigmoid'
        assert state['out_channels'] == 3 and state['in_channels'] == 1 and 'validation' in state
    del step
    _clear()

    # inference from the trained checkpoint with no further change: the mask is composed with region_class_order
    (root / 'run' / 'infer_config.py').write_text(_INFER_CFG)
    model = load_single_model(str(folder), 0, checkpoint='best')
    assert model.output_activation == 'sigmoid' and model.regions == BRATS and model.region_class_order == [2, 1, 3]
    del model
    masks = segmentation(val_paths[0], str(root / 'run'), str(root / 'out'), 'seg.mha', 0, True, True, False, True)
    out = root / 'out' / 'org.mha'
    written = read_image(str(out / 'seg.mha'), dtype=None).array
    assert np.array_equal(written, masks[0].array) and set(int(v) for v in np.unique(written)) <= {0, 1, 2, 3}
    probs = np.stack([read_image(str(out / 'mean_prob_{}.mha'.format(r))).array for r in range(3)])
    want = np.zeros(written.shape, np.int8)
    for r, label in enumerate([2, 1, 3]):
        want[probs[r] > np.float32(0.5)] = label
    assert np.array_equal(written, want)
    _clear()

    # a resume rebuilds the same network and continues
    save = root / 'resumed'
    shutil.copytree(str(folder), str(save / 'coarse'))
    os.remove(str(save / 'coarse' / 'train_log.txt'))
    step, train_lines, val_lines, _ = _run(root, 'resumed', 2, resume=4)
    assert step.net.output_activation == 'sigmoid' and step.regions == BRATS and len(train_lines) == 2
    assert [int(l.split('epoch: ')[1].split(',')[0]) for l in val_lines] == [5, 6]
    del step
    _clear()
