"""GPU tests of the online validation: seg3d_confusion_counts bit-equal to numpy on every path
and edge, the Validator inside a hipGraph, the fixed crops, and train() with a `validation` section end to end -- log lines,
`checkpoints/best`, inference from it, no interference with the training run, resume."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (sys.path)
from oracle import detgen

pytestmark = pytest.mark.gpu


# ---- the kernel against numpy ----------------------------------------------------------------------------------------------
def _ref_counts(p, t, ignore=None):
    """np.argmax (first maximum) + boolean sums; validity: 0 <= t < C and t != ignore"""
    N, C = p.shape[:2]
    pr, tt = p.reshape(N, C, -1), t.reshape(N, -1)
    pred = np.argmax(pr, 1)
    valid = (tt >= 0) & (tt < C)
    if ignore is not None:
        valid &= tt != ignore
    ti = tt.astype(np.int64)
    out = np.zeros((C, 3), dtype=np.int64)
    for c in range(C):
        out[c] = [np.sum(valid & (pred == c) & (ti == c)), np.sum(valid & (pred == c) & (ti != c)),
                  np.sum(valid & (pred != c) & (ti == c))]
    return out


def _inputs(seed, N, C, shape, stray=True):
    rng = np.random.RandomState(seed)
    p = rng.rand(N, C, *shape).astype(np.float32)
    t = rng.randint(0, C, size=(N, 1) + tuple(shape)).astype(np.float32)
    if stray:                                     # targets outside the classes: below, just above, the ignore label
        flat = t.reshape(-1)
        k = flat.size
        flat[rng.randint(0, k, size=max(1, k // 7))] = -1.0
        flat[rng.randint(0, k, size=max(1, k // 9))] = float(C)
        flat[rng.randint(0, k, size=max(1, k // 5))] = 255.0
    return p, t


def _gpu_counts(dev, p, t, ignore=None, out=None):
    from segmentation3d import _ops
    got = _ops.confusion_counts(torch.from_numpy(p).to(dev), torch.from_numpy(t).to(dev), ignore, out=out)
    assert got.dtype == torch.int64 and tuple(got.shape) == (p.shape[1], 3) and got.is_cuda
    return got.cpu().numpy()


@pytest.mark.parametrize('C', [1, 2, 3, 5, 16])
def test_confusion_counts_bit_equal_to_numpy(hip_device, C):
    """S = 5*7*9 (scalar path with tail), 4*4*8 (16-byte loads), 1; stray targets -1, C and 255 with ignore_label = 255"""
    for k, shape in enumerate([(5, 7, 9), (4, 4, 8), (1, 1, 1)]):
        p, t = _inputs(100 * C + k, 2, C, shape)
        assert np.array_equal(_gpu_counts(hip_device, p, t, 255), _ref_counts(p, t, 255)), (C, shape)
        assert np.array_equal(_gpu_counts(hip_device, p, t), _ref_counts(p, t)), (C, shape)   # no ignore label: 255 is out of range anyway
    p, t = _inputs(100 * C + 9, 2, C, (5, 7, 9), stray=False)
    ref = _ref_counts(p, t)
    assert ref.sum() > 0 and np.array_equal(_gpu_counts(hip_device, p, t), ref)
    assert int((ref[:, 0] + ref[:, 2]).sum()) == t.size                 # every voxel is some class's tp or fn


def test_confusion_counts_many_workgroups_and_grid_stride(hip_device):
    """33*32*32 voxels: more than one workgroup per sample; 300 samples: the per-sample grid shrinks to two workgroups (a
    grid sized from the CU count over the whole batch), so the grid-stride loop runs on both paths"""
    p, t = _inputs(7, 2, 3, (33, 32, 32))
    assert np.array_equal(_gpu_counts(hip_device, p, t, 255), _ref_counts(p, t, 255))
    for shape in [(33, 16, 16), (33, 7, 17)]:     # 16-byte loads / scalar with tail
        p, t = _inputs(8, 300, 2, shape)
        assert np.array_equal(_gpu_counts(hip_device, p, t, 255), _ref_counts(p, t, 255)), shape


def test_confusion_counts_ties_take_the_first_maximum(hip_device):
    for shape in [(4, 4, 8), (3, 5, 7)]:
        p, t = _inputs(21, 2, 4, shape, stray=False)
        p[:, 1, 0] = p[:, 3, 0] = 2.0             # two equal maxima: class 1 wins
        p[:, :, 1] = 0.25                          # all classes equal: class 0
        p[:, :, 2] = 0.0                           # p = 0 everywhere: class 0
        p[0, 2, 1, 1, :] = p[0, 0, 1, 1, :] = 0.5  # equal maxima, the first of them class 0
        ref = _ref_counts(p, t)
        assert np.array_equal(_gpu_counts(hip_device, p, t), ref), shape
    z = np.zeros((2, 5, 4, 4, 8), dtype=np.float32)
    t = _inputs(22, 2, 5, (4, 4, 8), stray=False)[1]
    got = _gpu_counts(hip_device, z, t)
    assert np.array_equal(got, _ref_counts(z, t)) and got[1:, 0].sum() == 0 and got[0, 0] == np.sum(t == 0)


def test_confusion_counts_ignore_accumulate_and_empty(hip_device):
    from segmentation3d import _ops
    p, t = _inputs(31, 2, 3, (5, 7, 9))
    ref1 = _ref_counts(p, t, 1)                   # an in-range ignore label
    assert np.array_equal(_gpu_counts(hip_device, p, t, 1), ref1) and ref1[1, 0] == 0 and ref1[1, 2] == 0
    # two calls with the same `out` add up
    q, u = _inputs(32, 2, 3, (4, 4, 8))
    out = torch.zeros((3, 3), dtype=torch.int64, device=hip_device)
    _gpu_counts(hip_device, p, t, 255, out=out)
    got = _gpu_counts(hip_device, q, u, 255, out=out)
    assert np.array_equal(got, _ref_counts(p, t, 255) + _ref_counts(q, u, 255))
    assert np.array_equal(_gpu_counts(hip_device, p, t, 255, out=out), 2 * _ref_counts(p, t, 255) + _ref_counts(q, u, 255))
    # a batch with every voxel invalid leaves zeros
    for value, ignore in [(-1.0, None), (255.0, 255), (3.0, None), (2.0, 2)]:
        none = np.full_like(t, value)
        assert not _gpu_counts(hip_device, p, none, ignore).any()
    # argument checks
    pd, td = torch.from_numpy(p).to(hip_device), torch.from_numpy(t).to(hip_device)
    with pytest.raises(ValueError):
        _ops.confusion_counts(pd.double(), td)
    with pytest.raises(ValueError):
        _ops.confusion_counts(torch.zeros((1, 17, 2, 2, 2), device=hip_device), torch.zeros((1, 1, 2, 2, 2), device=hip_device))
    with pytest.raises(ValueError):
        _ops.confusion_counts(pd, td[:, :, :4])
    with pytest.raises(ValueError):
        _ops.confusion_counts(pd, td, out=torch.zeros((3, 3), dtype=torch.int32, device=hip_device))


# ---- the Validator ---------------------------------------------------------------------------------------------------------
def _small_validator(dev, V=3, batchsize=2, ncls=2):
    from segmentation3d.core.seg_train import build_loss
    from segmentation3d.core.seg_validate import Validator
    from segmentation3d.network import vnet
    torch.manual_seed(3)
    net = vnet.SegmentationNet(1, ncls)
    vnet.parameters_kaiming_init(net)
    net = net.to(dev)
    crops = torch.from_numpy(detgen.normal(901, 'val/x', (V, 1, 32, 32, 32))).to(dev)
    masks = torch.from_numpy(detgen.labels(902, 'val/t', (V, 1, 32, 32, 32), ncls)).to(dev)
    return Validator(net, build_loss('DiceCE', ncls), crops, masks, batchsize, ema=0.5), net, crops, masks


def test_validator_pass_equals_numpy_and_is_capturable(hip_device):
    """the eager pass against argmax + numpy counts of the same forward; then the device side of a pass captured into ONE
    hipGraph and replayed once gives the same accumulators (the confusion-count entry neither allocates nor synchronises)"""
    from segmentation3d.utils.metrics import dice_from_counts, mean_foreground_dice
    v, net, crops, masks = _small_validator(hip_device)
    eager = v.run(1)
    with torch.no_grad():
        probs = torch.cat([net(crops[0:2]), net(crops[2:3])]).cpu().numpy()
    ref = _ref_counts(probs, masks.cpu().numpy())
    counts_eager, loss_eager = v.counts.clone(), v._loss.clone()
    assert np.array_equal(counts_eager.cpu().numpy(), ref)
    assert eager['dice'] == dice_from_counts(ref) and eager['mean_dice'] == mean_foreground_dice(ref)
    assert eager['ema_dice'] == eager['mean_dice'] and eager['improved'] is True and np.isfinite(eager['val_loss'])
    assert float(loss_eager[1]) == 3.0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        v.accumulate()
    v.counts.fill_(-7)
    v._loss.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(v.counts, counts_eager) and torch.equal(v._loss, loss_eager)
    again = v.finish(2)
    assert again['dice'] == eager['dice'] and again['val_loss'] == eager['val_loss']
    assert again['ema_dice'] == eager['ema_dice'] and again['improved'] is False      # the same score is no strict gain
    del graph


# ---- train() with a `validation` section ---------------------------------------------------------------------------------------
def _write_cases(folder, first, count):
    """learnable toy cases as tests/test_gpu_parity.py writes its own: the image is the label map plus noise"""
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    paths = []
    for k in range(first, first + count):
        os.makedirs(str(folder / 'c{}'.format(k)), exist_ok=True)
        seg = detgen.labels(800 + k, 'e2e/seg{}'.format(k), (48, 48, 48), 2).astype(np.int8)
        img = (seg.astype(np.float32) * 2.0 - 1.0 + 0.3 * detgen.normal(810 + k, 'e2e/n{}'.format(k), (48, 48, 48))).astype(np.float32)
        ip, sp = str(folder / 'c{}'.format(k) / 'org.mha'), str(folder / 'c{}'.format(k) / 'seg.mha')
        write_mha(Image3d(img, *frame), ip)
        write_mha(Image3d(seg, *frame), sp)
        paths += [ip, sp]
    return paths


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
__C.dataset.num_classes = 2
__C.dataset.spacing = [1.0, 1.0, 1.0]
__C.dataset.crop_size = [32, 32, 32]
__C.dataset.sampling_method = 'GLOBAL'
__C.dataset.random_translation = [2, 2, 2]
__C.dataset.random_scale = [0.95, 1.05]
__C.dataset.interpolation = 'LINEAR'
__C.dataset.crop_normalizers = [AdaptiveNormalizer()]
__C.loss = {{}}
__C.loss.name = 'DiceCE'
__C.loss.obj_weight = [1.0, 1.0]
__C.loss.focal_gamma = 2
__C.net = {{}}
__C.net.name = 'vnet'
__C.train = {{}}
__C.train.epochs = {epochs}
__C.train.batchsize = 2
__C.train.num_threads = 0
__C.train.lr = 1e-3
__C.train.betas = (0.9, 0.999)
__C.train.save_epochs = 2
{extra}'''

_VAL = '''
__C.validation = {{}}
__C.validation.imseg_list = '{val}'
__C.validation.crops_per_case = 2
__C.validation.ema = 0.5
'''


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    root = tmp_path_factory.mktemp('valdata')
    train_paths, val_paths = _write_cases(root, 0, 2), _write_cases(root, 2, 2)
    (root / 'train.txt').write_text('2\n' + '\n'.join(train_paths) + '\n')
    (root / 'val.txt').write_text('2\n' + '\n'.join(val_paths) + '\n')
    return root


def _run(toy, name, validation, extra='', epochs=6, resume=-1, val_extra=''):
    """train() from a config written under toy/<name>; returns (step, train_loss strings, val lines, model folder).
    train() seeds numpy and torch from the config; the sampler shuffles with python's global `random` stream, which is the
    caller's to seed"""
    import random
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import train
    save = toy / name
    os.makedirs(str(save), exist_ok=True)
    text = _CFG.format(train=str(toy / 'train.txt'), save=str(save), resume=resume, epochs=epochs, extra=extra)
    if validation:
        text += _VAL.format(val=str(toy / 'val.txt')) + val_extra
    cfg = save / 'cfg.py'
    cfg.write_text(text)
    random.seed(0)
    try:
        step = train(str(cfg))
    finally:
        _ops.set_activation_dtype('fp32')
    log = (save / 'coarse' / 'train_log.txt').read_text().strip().splitlines()
    losses = [l.split('train_loss: ')[1].split(',')[0] for l in log if 'train_loss' in l]
    return step, losses, [l for l in log if 'val_' in l], save / 'coarse'


@pytest.fixture(scope='module')
def validated_run(hip_device, toy):
    return _run(toy, 'on', True)


def _field(line, key):
    return float(line.split(key + ': ')[1].split(',')[0])


def test_collect_fixed_crops_keeps_the_global_stream(hip_device, toy):
    from segmentation3d.dataloader.dataset import SegmentationDataset, collect_fixed_crops
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    ds = SegmentationDataset(str(toy / 'val.txt'), 2, [1.0, 1.0, 1.0], [32, 32, 32], 'GLOBAL', [0, 0, 0], [1, 1], 'LINEAR',
                             [AdaptiveNormalizer()], device=hip_device)
    np.random.seed(1234)
    np.random.uniform()
    before = np.random.get_state()
    crops, masks = collect_fixed_crops(ds, 3, seed=5)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert tuple(crops.shape) == (6, 1, 32, 32, 32) and tuple(masks.shape) == (6, 1, 32, 32, 32)
    assert crops.is_cuda and masks.is_cuda and crops.dtype == torch.float32
    np.random.uniform(size=7)                      # wherever the caller's stream stands, the same seed gives the same crops
    crops2, masks2 = collect_fixed_crops(ds, 3, seed=5)
    assert torch.equal(crops, crops2) and torch.equal(masks, masks2)
    crops3, _ = collect_fixed_crops(ds, 3, seed=6)
    assert not torch.equal(crops, crops3)
    assert not torch.equal(crops[0], crops[1])      # the crops of one case differ from each other
    # case order: with the same seed the first draws belong to case 0, so its three crops are those of a data set that
    # holds case 0 alone -- and the last three are not
    lines = (toy / 'val.txt').read_text().splitlines()
    (toy / 'val_first.txt').write_text('1\n' + '\n'.join(lines[1:3]) + '\n')
    first = SegmentationDataset(str(toy / 'val_first.txt'), 2, [1.0, 1.0, 1.0], [32, 32, 32], 'GLOBAL', [0, 0, 0], [1, 1],
                                'LINEAR', [AdaptiveNormalizer()], device=hip_device)
    crops_first, masks_first = collect_fixed_crops(first, 3, seed=5)
    assert torch.equal(crops[:3], crops_first) and torch.equal(masks[:3], masks_first)
    assert not torch.equal(crops[3:], crops_first) and not torch.equal(masks[3:], masks_first)
    state = np.random.get_state()

    class Boom(object):
        def __len__(self):
            return 1

        def __getitem__(self, index):
            np.random.uniform()
            raise RuntimeError('boom')
    with pytest.raises(RuntimeError):
        collect_fixed_crops(Boom(), 1, seed=0)
    assert np.array_equal(state[1], np.random.get_state()[1]) and state[2] == np.random.get_state()[2]   # restored in a finally
    with pytest.raises(ValueError):
        collect_fixed_crops(ds, 0, seed=0)


def test_train_with_validation_logs_and_keeps_the_best(hip_device, validated_run):
    """6 epochs of one step each, validation every epoch: one `val_` line per validated epoch (1..5), the best moving average
    in checkpoints/best with validation.json, the average's state in every chk_<epoch>, and inference from `best`"""
    step, losses, val_lines, folder = validated_run
    assert len(losses) == 6 and [int(l.split('epoch: ')[1].split(',')[0]) for l in val_lines] == [1, 2, 3, 4, 5]
    for line in val_lines:
        assert all(key in line for key in ('val_loss: ', 'val_dice: ', 'val_dice_ema: ', 'val_dice_per_class: ['))
        assert len(line.split('val_dice_per_class: [')[1].rstrip(']').split(', ')) == 2
    means, emas = [_field(l, 'val_dice') for l in val_lines], [_field(l, 'val_dice_ema') for l in val_lines]
    assert emas[0] == means[0] and all(0.0 <= m <= 1.0 for m in means)
    for k in range(1, 5):                                                    # ema = 0.5: the printed values follow the rule
        assert abs(emas[k] - (0.5 * emas[k - 1] + 0.5 * means[k])) < 1.01e-4
    best = folder / 'checkpoints' / 'best'
    record = json.loads((best / 'validation.json').read_text())
    assert emas[record['epoch'] - 1] == max(emas) and record['improved'] is True
    assert set(record) == {'epoch', 'batch', 'val_loss', 'dice', 'mean_dice', 'ema_dice', 'improved'}
    assert abs(record['ema_dice'] - max(emas)) < 0.51e-4 and record['batch'] == record['epoch'] + 1
    assert (best / 'optimizer.pth').is_file()
    state = torch.load(str(best / 'params.pth'), map_location='cpu', weights_only=True)
    assert state['epoch'] == record['epoch'] and state['validation']['best_epoch'] == record['epoch']
    assert state['validation']['best_ema_dice'] == record['ema_dice']
    tracker = step.validator.tracker
    assert tracker.best_epoch == record['epoch'] and abs(tracker.ema_dice - emas[-1]) < 0.51e-4
    for epoch in (2, 4):                                                     # regular checkpoints carry the state of their epoch
        chk = torch.load(str(folder / 'checkpoints' / 'chk_{}'.format(epoch) / 'params.pth'), map_location='cpu',
                         weights_only=True)
        assert abs(chk['validation']['ema_dice'] - emas[epoch - 1]) < 0.51e-4
        assert abs(chk['validation']['best_ema_dice'] - max(emas[:epoch])) < 0.51e-4
    # "latest" is still the largest chk_<n>; the stage key `checkpoint = 'best'` loads the best one
    from segmentation3d.core.seg_infer import load_models, load_single_model
    from segmentation3d.utils.model_io import get_checkpoint_folder
    assert get_checkpoint_folder(str(folder / 'checkpoints'), -1) == str(folder / 'checkpoints' / 'chk_4')
    (folder.parent / 'infer_config.py').write_text(
        "from easydict import EasyDict as edict\n__C = edict()\ncfg = __C\n__C.general = {}\n"
        "__C.general.single_scale = 'coarse'\n__C.coarse = {}\n__C.coarse.model_name = 'coarse'\n"
        "__C.coarse.checkpoint = 'best'\n")
    models = load_models(str(folder.parent), 0)
    loaded = models.coarse_model.net.state_dict()
    assert loaded and all(torch.equal(v.cpu(), state['state_dict'][k]) for k, v in loaded.items())
    latest = load_single_model(str(folder), 0)
    chk4 = torch.load(str(folder / 'checkpoints' / 'chk_4' / 'params.pth'), map_location='cpu', weights_only=True)
    assert all(torch.equal(v.cpu(), chk4['state_dict'][k]) for k, v in latest.net.state_dict().items())
    by_epoch = load_single_model(str(folder), 0, checkpoint=2)
    chk2 = torch.load(str(folder / 'checkpoints' / 'chk_2' / 'params.pth'), map_location='cpu', weights_only=True)
    assert all(torch.equal(v.cpu(), chk2['state_dict'][k]) for k, v in by_epoch.net.state_dict().items())
    with pytest.raises(FileNotFoundError):
        load_single_model(str(folder), 0, checkpoint=3)


@pytest.mark.parametrize('mode', ['eager', 'graph'])
def test_validation_does_not_touch_the_training_run(hip_device, toy, validated_run, mode):
    """the train_loss strings of a seeded run are identical with validation on and off -- the fixed crops leave numpy's global
    stream alone and the pass changes nothing the next step reads -- with eager steps and with the step in a hipGraph"""
    extra = '' if mode == 'eager' else '__C.train.use_graph = True\n'
    if mode == 'eager':
        step_on, on, val_lines = validated_run[0], validated_run[1], validated_run[2]
    else:
        step_on, on, val_lines, _ = _run(toy, 'on_' + mode, True, extra)
    step_off, off, none, folder_off = _run(toy, 'off_' + mode, False, extra)
    assert len(on) == 6 and on == off, (on, off)
    assert len(val_lines) == 5 and none == []
    assert step_on.use_graph == (mode == 'graph') and (step_on._graph is not None) == (mode == 'graph')
    assert not hasattr(step_off, 'validator') and not (folder_off / 'checkpoints' / 'best').exists()
    chk = torch.load(str(folder_off / 'checkpoints' / 'chk_2' / 'params.pth'), map_location='cpu', weights_only=True)
    assert 'validation' not in chk                                           # without the section: today's key set
    # every pass scored the weights of ITS epoch (a pass that read stale weights would repeat the first one's loss)
    assert len({l.split('val_loss: ')[1].split(',')[0] + l.split('val_dice: ')[1].split(',')[0] for l in val_lines}) > 1


def test_frozen_weight_cache_is_left_alone(hip_device):
    """what the validation pass relies on next to a captured train step: inside PACK_CACHE.frozen() a conv uses an image that
    is current, packs one that is missing or stale into a buffer of its own, and neither the entries nor the job table (whose
    device address a captured step holds) change"""
    from segmentation3d import _ops
    cache = _ops.PACK_CACHE
    was = _ops.weight_cache(True)
    start = set(cache.entries)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn((1, 32, 8, 8, 8), generator=gen).to(hip_device)
    w_known, w_new = (torch.randn((32, 32, 3, 3, 3), generator=gen).to(hip_device) for _ in range(2))
    b = torch.randn(32, generator=gen).to(hip_device)
    try:
        with torch.no_grad():
            y_known = _ops.conv(x, w_known, b, 'k3')                 # registers w_known's image
            cache.repack_all()                                       # what an optimizer step does: builds the job table
            keys, table, epoch = list(cache.entries), cache._table, cache.epoch
            assert table is not None and len(keys) == len(start) + 1
            with cache.frozen():
                assert torch.equal(_ops.conv(x, w_known, b, 'k3'), y_known)      # a current image is used
                y_new = _ops.conv(x, w_new, b, 'k3')                             # never registered
                w_known.mul_(2.0)                                                # in-place update: the image is stale now
                y_stale = _ops.conv(x, w_known, b, 'k3')
            assert list(cache.entries) == keys and cache._table is table and cache.epoch == epoch
            _ops.weight_cache(False)                                 # the reference results: packed afresh, no cache
            assert torch.equal(y_new, _ops.conv(x, w_new, b, 'k3'))
            assert torch.equal(y_stale, _ops.conv(x, w_known, b, 'k3')) and not torch.equal(y_stale, y_known)
    finally:
        _ops.weight_cache(was)                                       # (switching it off above dropped every entry)


def test_graph_run_validates_with_another_batch_size(hip_device, toy, monkeypatch):
    """train step captured in a hipGraph with batch 2, validation over 4 crops in batches of 3 and 1: another N can select
    another conv plan and with it a packed image the train step never registered.  Every pass must leave the cache's entries
    and its job table -- the captured step reads that table on every replay -- the very same objects, and the run's
    train_loss strings must be those of the run without validation."""
    from segmentation3d import _ops
    from segmentation3d.core.seg_validate import Validator
    cache, seen = _ops.PACK_CACHE, []
    run = Validator.run

    def watched(self, epoch=None):
        before = (list(cache.entries), cache._table, cache.epoch, [(e['epoch'], e['version']) for e in cache.entries.values()])
        result = run(self, epoch)
        after = (list(cache.entries), cache._table, cache.epoch, [(e['epoch'], e['version']) for e in cache.entries.values()])
        seen.append((before[0] == after[0], before[1] is after[1], before[2] == after[2], before[3] == after[3],
                     [int(self.crops[k:k + self.batchsize].shape[0]) for k in range(0, self.crops.shape[0], self.batchsize)]))
        return result
    monkeypatch.setattr(Validator, 'run', watched)
    extra = '__C.train.use_graph = True\n'
    step_on, on, val_lines, _ = _run(toy, 'on_graph_b3', True, extra, val_extra='__C.validation.batchsize = 3\n')
    monkeypatch.undo()
    assert step_on._graph is not None and len(val_lines) == 5
    assert seen == [(True, True, True, True, [3, 1])] * 5, seen
    _, off, _, _ = _run(toy, 'off_graph_b3', False, extra)
    assert len(on) == 6 and on == off, (on, off)
    assert len({l.split('val_loss: ')[1].split(',')[0] + l.split('val_dice: ')[1].split(',')[0] for l in val_lines}) > 1


def test_resume_continues_the_moving_average(hip_device, toy, validated_run):
    """resume from chk_4 of the validated run into a fresh folder copy: the first validation after the resume (epoch 5)
    averages with the stored value instead of starting over, and the best value is carried"""
    import shutil
    _, _, val_lines, folder = validated_run
    save = toy / 'resumed'
    if save.exists():
        shutil.rmtree(str(save))
    shutil.copytree(str(folder), str(save / 'coarse'))
    shutil.rmtree(str(save / 'coarse' / 'checkpoints' / 'best'))
    os.remove(str(save / 'coarse' / 'train_log.txt'))
    stored = torch.load(str(save / 'coarse' / 'checkpoints' / 'chk_4' / 'params.pth'), map_location='cpu',
                        weights_only=True)['validation']
    step, losses, lines, _ = _run(toy, 'resumed', True, epochs=2, resume=4)
    epochs = [int(l.split('epoch: ')[1].split(',')[0]) for l in lines]
    assert len(losses) == 2 and epochs == [5, 6]                             # epoch 4 is not validated a second time
    mean, ema = _field(lines[0], 'val_dice'), _field(lines[0], 'val_dice_ema')
    assert abs(ema - (0.5 * stored['ema_dice'] + 0.5 * mean)) < 1.01e-4
    tracker = step.validator.tracker
    assert tracker.best_ema_dice >= stored['best_ema_dice']
    if tracker.best_ema_dice == stored['best_ema_dice']:
        assert tracker.best_epoch == stored['best_epoch']
        assert not (save / 'coarse' / 'checkpoints' / 'best').exists()          # nothing beat the stored best
    else:
        assert tracker.best_epoch >= 5 and (save / 'coarse' / 'checkpoints' / 'best' / 'validation.json').is_file()
