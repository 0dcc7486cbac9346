"""Multi-modality input on the MI355X: the MC = 2 / 3 / 4 / 0 instantiations of the two channels-last kernel templates
against their MC = 1 instantiation, which single-modality volumes run (bit for bit; the numpy oracle pins MC = 1 in
test_gpu_kernels.py), the file-backed dataset against the numpy oracle, train() -> segmentation() end to end against a CPU
oracle, and sharded inference."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gpu_util import report, max_err, mask_flips, TIE_GAP
from oracle import detgen, torch_ref
from test_multimodal import write_nifti_4d, _oblique

pytestmark = pytest.mark.gpu


def _frame(spacing, origin, direction):
    return (tuple(float(v) for v in spacing), tuple(float(v) for v in origin), tuple(float(v) for v in np.ravel(direction)))


# ---------------------------------------------------------------------------------------------------------------------
# seg3d_resample_affine_mc
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [2, 3, 4, 8])
@pytest.mark.parametrize('interp', ['LINEAR', 'NN'])
def test_resample_mc_equals_single_channel_bit_for_bit(hip_device, M, interp):
    from segmentation3d.utils import image_tools
    Z, Y, X = 21, 26, 30
    src = torch.from_numpy(detgen.normal(301 + M, 'mc/rs', (Z, Y, X, M)) * 50).float().to(hip_device)
    src_frame = _frame((0.7, 1.1, 2.3), (-5.0, 3.0, 1.0), _oblique(20.0))
    # output grid: other spacing, other (oblique) direction, shifted so that part of it lies outside the source
    dst_frame = _frame((0.9, 0.8, 1.7), (-9.0, -2.0, -4.0), _oblique(-35.0))
    size = (27, 33, 19)
    got = image_tools.resample_device_mc(src, src_frame, size, dst_frame, interp, 0.25)
    assert tuple(got.shape) == (19, 33, 27, M)
    inside = 0
    for m in range(M):
        ref = image_tools.resample_device(src[..., m].contiguous(), src_frame, size, dst_frame, interp, 0.25)
        assert torch.equal(got[..., m], ref), m
        inside = int((ref != 0.25).sum())
    assert 0 < inside < 19 * 33 * 27                      # both inside and padded voxels were exercised
    # into slot 1 of an NDHWC batch: the other slots stay untouched
    batch = torch.full((3, 19, 33, 27, M), 7.0, device=hip_device)
    image_tools.resample_device_mc(src, src_frame, size, dst_frame, interp, 0.25, out=batch[1])
    assert torch.equal(batch[1], got) and bool((batch[0] == 7.0).all()) and bool((batch[2] == 7.0).all())
    # padded destination rows (voxel stride M + 1): the scalar path of every width; the pad float is never written
    from segmentation3d import _engine as E
    rows = torch.full((19 * 33 * 27, M + 1), -3.0, device=hip_device)
    A = np.ascontiguousarray(image_tools.index_affine(src_frame, dst_frame), dtype=np.float64)
    E.call('seg3d_resample_affine_mc', E.ptr(src), E.ptr(rows), M, M + 1, X, Y, Z, 27, 33, 19,
           A.ctypes.data_as(ctypes.c_void_p), int(interp == 'LINEAR'), 0.25, E.stream_ptr())
    assert torch.equal(rows[:, :M].reshape(got.shape), got) and bool((rows[:, M] == -3.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# seg3d_patch_gather_normalize_mc
# ---------------------------------------------------------------------------------------------------------------------
_NORMS = [{'type': 0, 'mean': 20.0, 'stddev': 35.0, 'clip': True}, {'type': 0, 'mean': -4.0, 'stddev': 9.0, 'clip': False},
          {'type': 1, 'clip_sigma': 2.5}, None, {'type': 1, 'clip_sigma': 3}, None, {'type': 0, 'mean': 1.0,
                                                                                       'stddev': 2.0, 'clip': True},
          {'type': 1, 'clip_sigma': 1.5}]


def _gather_setup(hip_device, M):
    from segmentation3d.core.seg_infer import SlidingWindowBatcher
    from segmentation3d.utils.image_tools import image_partition_by_fixed_size
    Z, Y, X = 40, 44, 52
    vol = torch.from_numpy(detgen.normal(400 + M, 'mc/g', (Z, Y, X, M)) * 60 + 10).float().to(hip_device)
    box = (24, 20, 12)                                     # not multiples of 8
    starts, _ = image_partition_by_fixed_size(((48, 48, 48), (1.0, 1.0, 1.0)), [0, 0, 0], [48, 48, 48], [16] * 3, [8] * 3, 16)
    starts = [[min(s[0], X - box[0]), min(s[1], Y - box[1]), min(s[2], Z - box[2])] for s in starts]
    norms = _NORMS[:M]
    mc = SlidingWindowBatcher(vol, starts, box, 2, norms, max_batch=16)
    singles = [SlidingWindowBatcher(vol[..., m].contiguous(), starts, box, 2, norms[m], max_batch=16) for m in range(M)]
    return vol, starts, mc, singles


@pytest.mark.parametrize('M', [4, 3, 6])
def test_gather_mc_equals_single_channel_bit_for_bit(hip_device, M):
    from segmentation3d import _ops
    vol, starts, mc, singles = _gather_setup(hip_device, M)
    assert len(starts) > 20
    for idx in (list(range(16)), list(range(16, min(27, len(starts))))):   # full batch, then one with padding patches
        got = mc.gather(idx)
        assert tuple(got.shape) == (len(idx), M, 12, 20, 24)
        assert got.permute(0, 2, 3, 4, 1).is_contiguous()      # NDHWC memory: the stem reads it without a copy
        for m in range(M):
            ref = singles[m].gather(idx)
            assert torch.equal(got[:, m], ref[:, 0]), (M, m)
    full = mc.gather_current()
    assert _ops.to_ndhwc(full).data_ptr() == full.data_ptr()


def test_gather_mc_graph_replay_equals_eager(hip_device):
    vol, starts, mc, _ = _gather_setup(hip_device, 4)
    batches = [list(range(16)), list(range(16, min(27, len(starts))))]
    eager = [mc.gather(b).clone() for b in batches]
    mc.plan(batches)
    mc.select(0)
    static = mc.gather_current()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        mc.gather_current(out=static)
    for k, b in enumerate(batches):
        mc.select(k)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static[:len(b)], eager[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# the file-backed dataset
# ---------------------------------------------------------------------------------------------------------------------
_DS_FRAMES = [_frame((0.875, 1.125, 1.5), (-10.0, 4.0, 7.5), np.eye(3)), _frame((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), np.eye(3))]
_DS_SHAPES = [(40, 56, 64), (48, 48, 48)]


def _write_mc_case(folder, name, shape, frame, seed, num_classes, M, form):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    os.makedirs(str(folder / name), exist_ok=True)
    planes = np.stack([(detgen.normal(seed + m, '{}/img{}'.format(name, m), shape) * (40 + 30 * m) + 20 * m)
                       for m in range(M)]).astype(np.float32)
    seg = detgen.labels(seed + 50, name + '/seg', shape, num_classes).astype(np.int8)
    sp = str(folder / name / 'seg.mha')
    write_mha(Image3d(seg, *frame), sp)
    if form == 'mha':
        paths = []
        for m in range(M):
            paths.append(str(folder / name / 'mod{}.mha'.format(m)))
            write_mha(Image3d(planes[m], *frame), paths[-1])
    else:
        paths = [str(folder / name / 'case.nii.gz')]
        write_nifti_4d(paths[0], planes, *frame)
    return paths, sp, planes, seg


def _mc_normalizers():
    from segmentation3d.utils.normalizer import AdaptiveNormalizer, FixedNormalizer
    return [AdaptiveNormalizer(), FixedNormalizer(20.0, 50.0, True), FixedNormalizer(40.0, 70.0, False), None]


def _dataset(tmp_path, method, form, M=4):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    cases = [_write_mc_case(tmp_path / form, 'case{}'.format(k), _DS_SHAPES[k], _DS_FRAMES[k], 900 + 100 * k, 3, M, form)
             for k in range(2)]
    lst = tmp_path / form / 'train.txt'
    lst.write_text('2 {}\n'.format(M) + ''.join('\n'.join(c[0]) + '\n' + c[1] + '\n' for c in cases))
    ds = SegmentationDataset(str(lst), 3, [1.0, 1.0, 1.2], [32, 32, 16], method, [3, 3, 3], [0.9, 1.1], 'LINEAR',
                             _mc_normalizers(), device=torch.device('cuda:0'))
    return ds, cases


@pytest.mark.parametrize('method', ['GLOBAL', 'MASK', 'HYBRID', 'CENTER'])
def test_multimodal_dataset_matches_oracle(hip_device, tmp_path, method):
    from oracle import numpy_ref
    crop, spacing = [32, 32, 16], [1.0, 1.0, 1.2]
    norms = [None if n is None else n.to_dict() for n in _mc_normalizers()]
    got = {}
    for form in ('mha', 'nii'):
        ds, cases = _dataset(tmp_path, method, form)
        assert len(ds) == 2 and ds.num_modality() == 4
        np.random.seed(5)
        got[form] = [ds[k] for k in (0, 1, 0)]
    # the two file forms hold the same case: identical crops
    for a, b in zip(got['mha'], got['nii']):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    np.random.seed(5)
    worst = 0.0
    for (im, seg, frame, name), k in zip(got['mha'], (0, 1, 0)):
        _, _, planes, seg_h = cases[k]
        size_xyz = _DS_SHAPES[k][::-1]
        sp, org, dr = _DS_FRAMES[k]

        def mask_center():
            label = np.random.randint(1, 3)
            v = numpy_ref.select_random_voxel(seg_h, label, np.random)
            if v is None:
                return numpy_ref.global_sample(size_xyz, sp, org, crop, spacing, np.random)
            return np.asarray(org) + np.asarray(dr).reshape(3, 3) @ (np.asarray(sp) * np.asarray(v, dtype=np.float64))
        if method == 'CENTER':
            center = numpy_ref.center_sample(size_xyz, sp, org, dr)
        elif method == 'GLOBAL' or (method == 'HYBRID' and k % 2):
            center = numpy_ref.global_sample(size_xyz, sp, org, crop, spacing, np.random)
        else:
            center = mask_center()
        center = center + np.random.uniform(-np.array([3.0, 3.0, 3.0]), np.array([3.0, 3.0, 3.0]), size=[3])
        cs = np.array(spacing) * np.random.uniform(0.9, 1.1)
        assert tuple(im.shape) == (4, 16, 32, 32) and im.is_cuda and seg.is_cuda
        assert im.permute(1, 2, 3, 0).is_contiguous()
        for m in range(4):
            ref = numpy_ref.apply_normalizer(numpy_ref.crop_image(planes[m], _DS_FRAMES[k], center, crop, cs, True), norms[m])
            e = max_err(im[m], ref)
            worst = max(worst, e)
            assert e < 2e-5, (method, k, m, e)
        ref_seg = numpy_ref.crop_image(seg_h.astype(np.float32), _DS_FRAMES[k], center, crop, cs, False)
        assert np.array_equal(seg[0].cpu().numpy(), ref_seg), (method, k)
        assert np.allclose(frame[:3], cs, atol=1e-6) and np.allclose(frame[3:6], numpy_ref.crop_origin(center, crop, cs), atol=1e-4)
        assert name.startswith('case{}'.format(k))
    report('multimodal_dataset_' + method, crop=worst)


def test_multimodal_loader_batches_are_channels_last(hip_device, tmp_path):
    from segmentation3d import _ops
    from segmentation3d.dataloader.dataset import DeviceCropLoader
    ds, _ = _dataset(tmp_path, 'GLOBAL', 'mha')
    np.random.seed(11)
    ref = [ds[k][0].clone() for k in (0, 1, 1, 0, 0)]
    np.random.seed(11)
    batches = list(DeviceCropLoader(ds, [0, 1, 1, 0, 0], 2))
    assert [tuple(b[0].shape) for b in batches] == [(2, 4, 16, 32, 32)] * 2 + [(1, 4, 16, 32, 32)]
    for j, (crops, masks, frames, names) in enumerate(batches):
        assert _ops.to_ndhwc(crops).data_ptr() == crops.data_ptr()     # the stem reads the batch's own memory
        assert tuple(masks.shape) == (crops.shape[0], 1, 16, 32, 32)
        for i in range(crops.shape[0]):
            assert torch.equal(crops[i], ref[2 * j + i])
    # TrainStep's graph path keeps the layout: clone / copy_ preserve channels-last memory
    crops = batches[0][0]
    gx = crops.clone()
    assert gx.stride() == crops.stride() and _ops.to_ndhwc(gx).data_ptr() == gx.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
# train() -> checkpoint -> segmentation()
# ---------------------------------------------------------------------------------------------------------------------
_TRAIN_CFG = '''
from easydict import EasyDict as edict
from segmentation3d.utils.normalizer import AdaptiveNormalizer, FixedNormalizer
__C = edict()
cfg = __C
__C.general = {}
__C.general.imseg_list = '%s'
__C.general.save_dir = '%s'
__C.general.model_scale = 'coarse'
__C.general.resume_epoch = -1
__C.general.num_gpus = 1
__C.general.seed = 0
__C.dataset = {}
__C.dataset.num_classes = 2
__C.dataset.spacing = [1.0, 1.0, 1.0]
__C.dataset.crop_size = [32, 32, 32]
__C.dataset.sampling_method = 'GLOBAL'
__C.dataset.random_translation = [2, 2, 2]
__C.dataset.random_scale = [0.95, 1.05]
__C.dataset.interpolation = 'LINEAR'
__C.dataset.crop_normalizers = [AdaptiveNormalizer(), FixedNormalizer(0.0, 2.0, True), AdaptiveNormalizer(2),
                                FixedNormalizer(1.0, 3.0, False)]
__C.loss = {}
__C.loss.name = 'Dice'
__C.loss.obj_weight = [0.5, 0.5]
__C.loss.focal_gamma = 2
__C.net = {}
__C.net.name = 'vnet'
__C.train = {}
__C.train.epochs = 4
__C.train.batchsize = 2
__C.train.num_threads = 0
__C.train.lr = 1e-3
__C.train.betas = (0.9, 0.999)
__C.train.save_epochs = 2
%s'''

_SEG_CFG = """from easydict import EasyDict as edict
__C = edict()
cfg = __C
__C.general = {}
__C.general.single_scale = 'coarse'
__C.coarse = {}
__C.coarse.model_name = 'coarse'
__C.coarse.pick_largest_cc = False
__C.coarse.remove_small_cc = 0
__C.coarse.partition_type = 'SIZE'
__C.coarse.partition_size = [32.0, 32.0, 32.0]
__C.coarse.partition_stride = [16.0, 16.0, 16.0]
"""


def _e2e_cases(tmp_path):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    frame = _frame((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), np.eye(3))
    lines, cases = [], []
    for k in range(2):
        d = tmp_path / 'c{}'.format(k)
        os.makedirs(str(d), exist_ok=True)
        seg = detgen.labels(800 + k, 'mm/seg{}'.format(k), (48, 48, 48), 2).astype(np.int8)
        planes = np.stack([(seg.astype(np.float32) * (m + 1) - 0.5 * m + 0.4 * detgen.normal(810 + 10 * k + m,
                                                                                           'mm/n{}{}'.format(k, m),
                                                                                           (48, 48, 48)))
                           for m in range(4)]).astype(np.float32)
        paths = [str(d / 'mod{}.mha'.format(m)) for m in range(4)]
        for m in range(4):
            write_mha(Image3d(planes[m], *frame), paths[m])
        sp = str(d / 'seg.mha')
        write_mha(Image3d(seg, *frame), sp)
        lines += paths + [sp]
        cases.append((paths, planes))
    (tmp_path / 'train.txt').write_text('2 4\n' + '\n'.join(lines) + '\n')
    return cases, frame


@pytest.mark.parametrize('extra', ['', "__C.train.compute_dtype = 'bf16'\n__C.train.use_graph = True\n"])
def test_multimodal_train_then_segment_end_to_end(hip_device, tmp_path, extra):
    from oracle import numpy_ref
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import train
    from segmentation3d.core.seg_infer import segmentation
    from segmentation3d.utils.image_io import read_image
    cases, frame = _e2e_cases(tmp_path)
    cfg = tmp_path / 'cfg.py'
    cfg.write_text(_TRAIN_CFG % (str(tmp_path / 'train.txt'), str(tmp_path / 'model'), extra))
    try:
        step = train(str(cfg))
    finally:
        _ops.set_activation_dtype('fp32')
    assert step.use_graph == bool(extra) and (step._graph is not None) == bool(extra)
    log = (tmp_path / 'model' / 'coarse' / 'train_log.txt').read_text().strip().splitlines()
    losses = [float(l.split('train_loss: ')[1].split(',')[0]) for l in log if 'train_loss' in l]
    assert len(losses) == 4 and all(np.isfinite(losses)), losses
    state = torch.load(str(tmp_path / 'model' / 'coarse' / 'checkpoints' / 'chk_2' / 'params.pth'), weights_only=True)
    assert state['in_channels'] == 4 and len(state['crop_normalizers']) == 4
    assert [d['type'] for d in state['crop_normalizers']] == [1, 0, 1, 0]
    # segmentation() on the trained 4-modality model: a multi-path txt and a 4-D NIfTI of the same case
    (tmp_path / 'model' / 'infer_config.py').write_text(_SEG_CFG)
    paths, planes = cases[1]
    nii = str(tmp_path / 'case1.nii.gz')
    write_nifti_4d(nii, planes, *frame)
    (tmp_path / 'test.txt').write_text('1\ncase1 {}\n'.format(' '.join(paths)))
    masks = {}
    for key, src in (('txt', str(tmp_path / 'test.txt')), ('nii', nii)):
        out = tmp_path / ('out_' + key)
        masks[key] = segmentation(src, str(tmp_path / 'model'), str(out), 'seg.mha', 0, True, True, True, True)[0]
    assert np.array_equal(masks['txt'].array, masks['nii'].array)
    case_dir = tmp_path / 'out_txt' / 'case1'
    assert all((case_dir / 'org_{}.mha'.format(m)).is_file() for m in range(4)) and not (case_dir / 'org.mha').exists()
    got = np.stack([read_image(str(case_dir / 'mean_prob_{}.mha'.format(c))).array for c in range(2)])
    # oracle: partition, per-modality normalise, the CPU network, accumulate, finalize
    sd = {k: v.float() for k, v in state['state_dict'].items()}
    norms = state['crop_normalizers']
    starts, ends = numpy_ref.partition_by_fixed_size((48, 48, 48), (1.0, 1.0, 1.0), [0, 0, 0], [48, 48, 48], [32.0] * 3,
                                                     [16.0] * 3, 16)
    acc = np.zeros((2, 48, 48, 48), np.float32)
    count = np.zeros((48, 48, 48), np.float32)
    for s, e in zip(starts, ends):
        rois = [numpy_ref.apply_normalizer(planes[m][s[2]:e[2], s[1]:e[1], s[0]:e[0]].copy(), norms[m]) for m in range(4)]
        with torch.no_grad():
            p = torch_ref.segmentation_net(torch.from_numpy(np.stack(rois)[None]), sd, 'vnet').numpy()
        numpy_ref.accumulate_patch(acc, count, s, e, p[0])
    ref_probs, ref_mask = numpy_ref.finalize(acc, count)
    err = max_err(got, ref_probs)
    flips, gap = mask_flips(masks['txt'].array, ref_mask, ref_probs)
    report('multimodal_e2e' + ('_bf16_graph' if extra else ''), probs=err, mask_flips=float(flips), worst_gap=gap)
    assert err < 1e-4, err
    assert gap < TIE_GAP, (flips, gap)


# ---------------------------------------------------------------------------------------------------------------------
# sharded sliding window, M = 4
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


_SHARD_NORMS = [{'type': 1, 'clip_sigma': 3}, {'type': 0, 'mean': -50.0, 'stddev': 150.0, 'clip': True}, None,
                {'type': 1, 'clip_sigma': 2}]


def _shard_setup():
    from segmentation3d.utils.image_tools import image_partition_by_fixed_size
    Z, Y, X = 80, 48, 64
    vol = (detgen.normal(86, 'mm/ddp', (Z, Y, X, 4)) * 200 - 100).astype(np.float32)
    starts, _ = image_partition_by_fixed_size(((X, Y, Z), (1.0, 1.0, 1.0)), [0, 0, 0], [X, Y, Z], [32] * 3, [16] * 3, 16)
    return vol, starts


def _shard_net(device):
    from segmentation3d.network import vnet
    torch.manual_seed(5)
    net = vnet.SegmentationNet(4, 3)
    vnet.parameters_kaiming_init(net)
    return net.to(device).eval()


def _shard_worker(rank, world, port, out):
    from conftest import PKG  # noqa: F401  (sys.path)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from segmentation3d.core.seg_infer import sliding_window_inference
    net = _shard_net('cuda:0')
    vol, starts = _shard_setup()
    probs, mask, batcher = sliding_window_inference(net, torch.from_numpy(vol).cuda(), starts, (32, 32, 32), 3,
                                                    _SHARD_NORMS, batch_size=4, shard=True)
    torch.cuda.synchronize()
    torch.save({'probs': probs.cpu(), 'mask': mask.cpu(), 'mine': len(batcher.shard_plan.patches[rank])}, out.format(rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharded_multimodal_matches_single_rank(hip_device, tmp_path):
    from segmentation3d.core.seg_infer import sliding_window_inference
    world, port, out = 2, _free_port(), str(tmp_path / 'mm{}.pt')
    mp.spawn(_shard_worker, args=(world, port, out), nprocs=world, join=True)
    net = _shard_net(hip_device)
    vol, starts = _shard_setup()
    probs, mask, _ = sliding_window_inference(net, torch.from_numpy(vol).to(hip_device), starts, (32, 32, 32), 3,
                                              _SHARD_NORMS, batch_size=4)
    r = [torch.load(out.format(k), weights_only=True) for k in range(world)]
    assert r[0]['mine'] + r[1]['mine'] == len(starts) and abs(r[0]['mine'] - r[1]['mine']) <= 1
    for k in range(world):
        assert float((r[k]['probs'] - probs.cpu()).abs().max()) < 1e-6
        diff = r[k]['mask'] != mask.cpu()
        if bool(diff.any()):
            top2 = probs.cpu()[:, diff].topk(2, dim=0).values
            assert float((top2[0] - top2[1]).max()) < 4e-6, int(diff.sum())
    assert torch.equal(r[0]['probs'], r[1]['probs']) and torch.equal(r[0]['mask'], r[1]['mask'])
