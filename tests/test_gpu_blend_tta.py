"""GPU checks of Gaussian patch blending and mirror test-time augmentation:
seg3d_patch_gather_normalize_flip / _mc_flip, seg3d_patch_scatter_blend, the sliding window with the flip sequence in
its captured graph, the config / CLI plumbing and the mirror augmentation of the training crops.  The oracle is the numpy
restatement of the definitions in tests/test_blend_tta.py."""
import os

import numpy as np
import pytest
import torch

from conftest import PKG  # noqa: F401  (sys.path)
from test_blend_tta import (oracle_accumulate, oracle_finalize, oracle_flip, oracle_flip_set, oracle_sliding_window,
                            oracle_weight)

pytestmark = pytest.mark.gpu


def _flip_dims(mask, ndim=5):
    """tensor dims of a [.., z, y, x] tensor that flip mask `mask` mirrors"""
    return [ndim - 1 - b for b in range(3) if mask >> b & 1]


def _tflip(t, mask):
    dims = _flip_dims(mask, t.dim())
    return torch.flip(t, dims) if dims else t


def _axis_starts(n, b, stride):
    s = list(range(0, n - b + 1, stride))
    if s[-1] != n - b:
        s.append(n - b)                   # tail patch clamped to the volume
    return s


def _partition(shape_zyx, box, stride):
    """[x, y, z] starts, x fastest; tails clamped"""
    Z, Y, X = shape_zyx
    return [[x, y, z] for z in _axis_starts(Z, box[2], stride[2]) for y in _axis_starts(Y, box[1], stride[1])
            for x in _axis_starts(X, box[0], stride[0])]


# ---------------------------------------------------------------------------------------------------------------------
# 1. mirrored gather == torch.flip of the plain gather
# ---------------------------------------------------------------------------------------------------------------------
_NORMS = [{'type': 1, 'clip_sigma': 2.5}, {'type': 0, 'mean': -150.0, 'stddev': 280.0, 'clip': True}, None]


@pytest.mark.parametrize('norm', _NORMS, ids=['adaptive', 'fixed', 'none'])
def test_mirrored_gather_equals_flipped_plain_gather(hip_device, norm):
    from segmentation3d.core.seg_infer import SlidingWindowBatcher
    rng = np.random.RandomState(1)
    Z, Y, X = 48, 64, 80
    box = (32, 48, 16)
    starts = [[0, 0, 0], [48, 16, 32], [13, 7, 5], [21, 0, 30]]
    vol = torch.from_numpy((rng.randn(Z, Y, X) * 300 - 200).astype(np.float32)).to(hip_device)
    batcher = SlidingWindowBatcher(vol, starts, box, 2, norm, max_batch=5)
    idx = [0, 1, 2, 3]
    plain = batcher.gather(idx).clone()
    assert plain.shape == (4, 1, 16, 48, 32)
    assert torch.equal(batcher.gather(idx, flip=0), plain)
    for f in range(1, 8):
        got = batcher.gather(idx, flip=f)
        assert torch.equal(got, _tflip(plain, f)), (norm, f)
    with pytest.raises(ValueError):
        batcher.gather(idx, flip=8)


@pytest.mark.parametrize('M', [2, 3, 4])
def test_mirrored_multimodality_gather_equals_flipped_plain_gather(hip_device, M):
    from segmentation3d.core.seg_infer import SlidingWindowBatcher
    rng = np.random.RandomState(2 + M)
    Z, Y, X = 48, 64, 80
    box = (32, 48, 16)
    starts = [[0, 0, 0], [48, 16, 32], [13, 7, 5]]
    vol = torch.from_numpy((rng.randn(Z, Y, X, M) * 300 - 200).astype(np.float32)).to(hip_device)
    norms = [_NORMS[m % 3] for m in range(M)]
    batcher = SlidingWindowBatcher(vol, starts, box, 2, norms, max_batch=3)
    plain = batcher.gather([0, 1, 2]).clone()
    assert plain.shape == (3, M, 16, 48, 32)
    for f in range(1, 8):
        got = batcher.gather([0, 1, 2], flip=f)
        assert got.permute(0, 2, 3, 4, 1).is_contiguous()
        assert torch.equal(got, _tflip(plain, f)), (M, f)


def test_flip_entries_refuse_bad_arguments(hip_device):
    from segmentation3d import _engine as E
    t = torch.zeros(64, device=hip_device)
    i = torch.zeros(16, dtype=torch.int32, device=hip_device)
    with pytest.raises(ValueError, match='flip mask'):
        E.call('seg3d_patch_gather_normalize_flip', E.ptr(t), E.ptr(i), E.ptr(t), None, None, 4, 4, 4, 2, 2, 2, 1, -1, 0.0,
               1.0, 0, 1.0, 8, E.stream_ptr())
    with pytest.raises(ValueError, match='flip mask'):
        E.call('seg3d_patch_scatter_blend', E.ptr(t), E.ptr(i), E.ptr(i), None, E.ptr(t), E.ptr(t), 4, 4, 4, 2, 2, 2, 1, -1,
               8, E.stream_ptr())
    with pytest.raises(ValueError):
        E.call('seg3d_patch_scatter_blend', None, E.ptr(i), E.ptr(i), E.ptr(t), E.ptr(t), E.ptr(t), 4, 4, 4, 2, 2, 2, 1, 1,
               8, E.stream_ptr())
    with pytest.raises(ValueError):
        E.call('seg3d_patch_gather_normalize_flip', None, E.ptr(i), E.ptr(t), None, None, 4, 4, 4, 2, 2, 2, 1, -1, 0.0,
               1.0, 0, 1.0, 1, E.stream_ptr())


# ---------------------------------------------------------------------------------------------------------------------
# 2. blend entry with no table and no mirror == the plain accumulate entry
# ---------------------------------------------------------------------------------------------------------------------
def test_scatter_blend_without_table_and_mirror_is_the_plain_scatter(hip_device):
    from oracle import numpy_ref
    from segmentation3d import _engine as E
    from segmentation3d.core.seg_infer import SlidingWindowBatcher
    rng = np.random.RandomState(0)
    Z, Y, X, C, P = 48, 64, 80, 3, 5
    starts, _ = numpy_ref.partition_by_fixed_size((X, Y, Z), (1.0, 1.0, 1.0), [0, 0, 0], [X, Y, Z], (32, 32, 32),
                                                  (24, 24, 16), 16)
    vol = torch.zeros((Z, Y, X), device=hip_device)
    a = SlidingWindowBatcher(vol, starts, (32, 32, 32), C, None, max_batch=P)
    b = SlidingWindowBatcher(vol, starts, (32, 32, 32), C, None, max_batch=P)
    for i in range(0, len(starts), P):
        idx = list(range(i, min(i + P, len(starts))))
        probs = torch.from_numpy(rng.rand(P, C, 32, 32, 32).astype(np.float32)).to(hip_device)
        a.scatter(idx, probs)
        b.set_batch(idx)
        E.call('seg3d_patch_scatter_blend', E.ptr(probs), b._starts_ptr(), b._ctl_ptr(), None, E.ptr(b.acc), E.ptr(b.count),
               Z, Y, X, 32, 32, 32, C, 0, Z * Y * X, E.stream_ptr())
    assert float(a.count.max()) > 1.0
    assert torch.equal(a.acc, b.acc) and torch.equal(a.count, b.count)


# ---------------------------------------------------------------------------------------------------------------------
# 3. Gaussian scatter against the oracle loop, probabilities handed in mirrored
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flip', range(8))
def test_gaussian_scatter_equals_the_oracle_loop(hip_device, flip):
    from segmentation3d.core.seg_infer import SlidingWindowBatcher
    rng = np.random.RandomState(10 + flip)
    shape, box, C, P = (36, 40, 52), (16, 16, 16), 3, 5
    starts = _partition(shape, box, (8, 8, 8))
    assert len(starts) % P != 0 and [36, 24, 20] in starts                        # short last batch, clamped tails
    vol = torch.zeros(shape, device=hip_device)
    batcher = SlidingWindowBatcher(vol, starts, box, C, None, max_batch=P, blend='gaussian')
    acc = np.zeros((C,) + shape, np.float32)
    cnt = np.zeros(shape, np.float32)
    w = oracle_weight(box)
    hits = np.zeros(shape, np.int32)
    for i in range(0, len(starts), P):
        idx = list(range(i, min(i + P, len(starts))))
        probs = rng.rand(len(idx), C, 16, 16, 16).astype(np.float32)
        batcher.scatter(idx, torch.from_numpy(np.ascontiguousarray(oracle_flip(probs, flip))).to(hip_device), flip=flip)
        for j, k in enumerate(idx):
            oracle_accumulate(acc, cnt, starts[k], box, probs[j], w)
            s = starts[k]
            hits[s[2]:s[2] + 16, s[1]:s[1] + 16, s[0]:s[0] + 16] += 1
    assert hits.max() >= 8 and hits.min() >= 1                    # (the clamped tail patches overlap more than 8 deep)
    assert np.array_equal(batcher.acc.cpu().numpy(), acc)
    assert np.array_equal(batcher.count.cpu().numpy(), cnt)
    probs_d, mask_d = batcher.finalize()
    rp, rm = oracle_finalize(acc, cnt)
    err = float(np.abs(probs_d.cpu().numpy() - rp).max())
    print('gaussian scatter flip {}: max |probs - oracle| = {}'.format(flip, err))
    assert err == 0.0
    assert np.array_equal(mask_d.cpu().numpy(), rm)


def test_constant_scatter_with_mirror_equals_the_oracle_loop(hip_device):
    """constant weight + mirrored inputs (TTA without Gaussian blending) goes through the blend entry with a NULL table"""
    from segmentation3d.core.seg_infer import SlidingWindowBatcher
    rng = np.random.RandomState(4)
    shape, box, C = (20, 24, 28), (16, 12, 8), 2
    starts = _partition(shape, box, (6, 6, 4))
    batcher = SlidingWindowBatcher(torch.zeros(shape, device=hip_device), starts, box, C, None, max_batch=4)
    acc = np.zeros((C,) + shape, np.float32)
    cnt = np.zeros(shape, np.float32)
    w = oracle_weight(box, blend='constant')
    for i in range(0, len(starts), 4):
        idx = list(range(i, min(i + 4, len(starts))))
        for f in (0, 3, 6):
            probs = rng.rand(len(idx), C, 8, 12, 16).astype(np.float32)
            batcher.scatter(idx, torch.from_numpy(np.ascontiguousarray(oracle_flip(probs, f))).to(hip_device), flip=f)
            for j, k in enumerate(idx):
                oracle_accumulate(acc, cnt, starts[k], box, probs[j], w)
    assert np.array_equal(batcher.acc.cpu().numpy(), acc) and np.array_equal(batcher.count.cpu().numpy(), cnt)


# ---------------------------------------------------------------------------------------------------------------------
# 4. / 5. whole pipeline with a position-dependent (not mirror-equivariant) synthetic net
# ---------------------------------------------------------------------------------------------------------------------
_PIPE = dict(shape=(32, 40, 48), box=(16, 24, 8), stride=(8, 12, 4), C=3, batch=4, norm={'type': 1, 'clip_sigma': 2.5})
_PIPE_ORACLE = {}


def _pipe_inputs(device):
    rng = np.random.RandomState(21)
    vol = torch.from_numpy((rng.randn(*_PIPE['shape']) * 120 + 30).astype(np.float32)).to(device)
    bx, by, bz = _PIPE['box']
    ramp = torch.from_numpy((rng.rand(_PIPE['C'], bz, by, bx) * 2 - 0.5).astype(np.float32)).to(device)

    def net(x):                                        # [n, 1, bz, by, bx] -> [n, C, bz, by, bx], element-wise
        return torch.softmax(x * ramp[None], 1)
    return vol, net, _partition(_PIPE['shape'], _PIPE['box'], _PIPE['stride'])


def _pipe_oracle(device, axes):
    if axes not in _PIPE_ORACLE:
        from segmentation3d.core.seg_infer import SlidingWindowBatcher
        vol, net, starts = _pipe_inputs(device)
        batcher = SlidingWindowBatcher(vol, starts, _PIPE['box'], _PIPE['C'], _PIPE['norm'], max_batch=1)
        patches = [batcher.gather([k])[0].cpu().numpy() for k in range(len(starts))]

        def net_fn(a):
            return net(torch.from_numpy(a).to(device)).cpu().numpy()
        acc, cnt = oracle_sliding_window(lambda k: patches[k], net_fn, _PIPE['shape'], starts, _PIPE['box'], _PIPE['C'],
                                         _PIPE['batch'], axes)
        _PIPE_ORACLE[axes] = oracle_finalize(acc, cnt) + (cnt,)
    return _PIPE_ORACLE[axes]


@pytest.mark.parametrize('two_streams', [True, False])
@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('axes', [(), ('x',), ('x', 'y', 'z')])
def test_pipeline_with_position_dependent_net_equals_the_oracle(hip_device, axes, use_graph, two_streams):
    from segmentation3d.core.seg_infer import sliding_window_inference
    vol, net, starts = _pipe_inputs(hip_device)
    assert len(starts) > 2 * _PIPE['batch'] and len(starts) % _PIPE['batch'] != 0
    probs, mask, batcher = sliding_window_inference(net, vol, starts, _PIPE['box'], _PIPE['C'], _PIPE['norm'],
                                                    batch_size=_PIPE['batch'], use_graph=use_graph, two_streams=two_streams,
                                                    blend='gaussian', mirror_axes=axes)
    torch.cuda.synchronize()
    rp, rm, cnt = _pipe_oracle(hip_device, axes)
    assert np.array_equal(batcher.count.cpu().numpy(), cnt)
    err = float(np.abs(probs.cpu().numpy() - rp).max())
    print('pipeline axes {} graph {} two_streams {}: max |probs - oracle| = {}'.format(axes, use_graph, two_streams, err))
    assert err == 0.0
    assert np.array_equal(mask.cpu().numpy(), rm)
    if axes:
        # mirroring matters for this net: the result is not the un-augmented one
        assert float(np.abs(rp - _pipe_oracle(hip_device, ())[0]).max()) > 1e-3


def test_captured_replay_equals_eager_multimodality(hip_device):
    """graph against eager, bit for bit, on a two-modality (channels-last) volume with Gaussian blending and mirrors"""
    from segmentation3d.core.seg_infer import sliding_window_inference
    rng = np.random.RandomState(33)
    shape, box, C = (24, 32, 40), (16, 16, 8), 2
    vol = torch.from_numpy((rng.randn(*shape, 2) * 50).astype(np.float32)).to(hip_device)
    ramp = torch.from_numpy(rng.rand(C, 8, 16, 16).astype(np.float32)).to(hip_device)
    norms = [{'type': 1, 'clip_sigma': 3.0}, {'type': 0, 'mean': 5.0, 'stddev': 40.0, 'clip': False}]

    def net(x):
        return torch.softmax((x[:, :1] - 0.5 * x[:, 1:]) * ramp[None], 1)
    starts = _partition(shape, box, (8, 8, 4))
    out = {}
    for use_graph in (True, False):
        probs, mask, _ = sliding_window_inference(net, vol, starts, box, C, norms, batch_size=4, use_graph=use_graph,
                                                  blend='gaussian', mirror_axes=('y', 'z'))
        torch.cuda.synchronize()
        out[use_graph] = (probs.clone(), mask.clone())
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    plain, _, _ = sliding_window_inference(net, vol, starts, box, C, norms, batch_size=4, blend='gaussian')
    assert float((plain - out[True][0]).abs().max()) > 1e-3


def test_defaults_are_the_plain_path(hip_device):
    """blend='constant' without mirror axes calls the entries it called before: same result as the keyword-free call"""
    from segmentation3d.core.seg_infer import sliding_window_inference
    vol, net, starts = _pipe_inputs(hip_device)
    a, ma, ba = sliding_window_inference(net, vol, starts, _PIPE['box'], _PIPE['C'], _PIPE['norm'], batch_size=4)
    b, mb, bb = sliding_window_inference(net, vol, starts, _PIPE['box'], _PIPE['C'], _PIPE['norm'], batch_size=4,
                                         blend='constant', sigma_scale=0.125, mirror_axes=())
    assert ba._wtab is None and bb._wtab is None
    assert torch.equal(a, b) and torch.equal(ma, mb)
    assert float(ba.count.max()) == float(ba.count.round().max()) >= 2.0          # integer overlap counts


# ---------------------------------------------------------------------------------------------------------------------
# 6. real network
# ---------------------------------------------------------------------------------------------------------------------
def _kaiming_vnet(device, cin=1, cout=2, seed=7):
    from segmentation3d.network import vnet
    torch.manual_seed(seed)
    net = vnet.SegmentationNet(cin, cout)
    vnet.parameters_kaiming_init(net)
    return net.to(device).eval()


def test_vnet_gaussian_mirror_against_per_flip_oracle(hip_device):
    from segmentation3d.core.seg_infer import SlidingWindowBatcher, sliding_window_inference
    net = _kaiming_vnet(hip_device)
    rng = np.random.RandomState(41)
    shape, box, C, B = (64, 64, 64), (32, 32, 32), 2, 4
    vol = torch.from_numpy((rng.randn(*shape) * 200 - 100).astype(np.float32)).to(hip_device)
    starts = _partition(shape, box, (16, 16, 16))
    assert len(starts) == 27
    norm = {'type': 1, 'clip_sigma': 3.0}
    axes = ('x', 'z')
    probs, mask, _ = sliding_window_inference(net, vol, starts, box, C, norm, batch_size=B, blend='gaussian',
                                              mirror_axes=axes)
    torch.cuda.synchronize()
    batcher = SlidingWindowBatcher(vol, starts, box, C, norm, max_batch=B)
    acc = np.zeros((C,) + shape, np.float32)
    cnt = np.zeros(shape, np.float32)
    w = oracle_weight(box)
    assert oracle_flip_set(axes) == [0, 1, 4, 5]
    with torch.no_grad():
        for i in range(0, len(starts), B):
            idx = list(range(i, min(i + B, len(starts))))
            plain = batcher.gather(idx).clone()
            for f in oracle_flip_set(axes):
                out = _tflip(net(_tflip(plain, f).contiguous()), f).cpu().numpy()
                for j, k in enumerate(idx):
                    oracle_accumulate(acc, cnt, starts[k], box, out[j], w)
    rp, _ = oracle_finalize(acc, cnt)
    got = probs.cpu().numpy()
    err = float(np.abs(got - rp).max())
    print('vnet gaussian + mirror xz: max |probs - oracle| = {}'.format(err))
    assert err < 1e-4
    assert np.array_equal(mask.cpu().numpy(), got.argmax(0).astype(np.int8))


# ---------------------------------------------------------------------------------------------------------------------
# 7. segmentation_volume with the stage keys, and the command line
# ---------------------------------------------------------------------------------------------------------------------
def _save_model(folder, net, spacing):
    chk = folder / 'checkpoints' / 'chk_5'
    chk.mkdir(parents=True)
    torch.save({'epoch': 5, 'batch': 1, 'net': 'vnet', 'max_stride': 16, 'state_dict': net.state_dict(),
                'spacing': list(spacing), 'interpolation': 'LINEAR', 'in_channels': 1, 'out_channels': 2,
                'crop_normalizers': [{'type': 1, 'clip_sigma': 3}]}, str(chk / 'params.pth'))


class _StagePlain(object):
    partition_type = 'SIZE'
    partition_size = [32, 32, 32]
    partition_stride = [16, 16, 16]


class _StageTta(_StagePlain):
    blend_mode = 'gaussian'
    blend_sigma_scale = 0.2
    tta_mirror_axes = ['x', 'y']


def test_segmentation_volume_reads_the_stage_keys(hip_device, tmp_path):
    from segmentation3d.core.seg_infer import load_single_model, segmentation_volume, sliding_window_inference
    from segmentation3d.utils import image_tools
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.image_tools import image_partition_by_fixed_size
    _save_model(tmp_path / 'fine', _kaiming_vnet('cpu', seed=9), (1.0, 1.0, 1.0))
    model = load_single_model(str(tmp_path / 'fine'), 0)
    rng = np.random.RandomState(51)
    vol = (rng.randn(30, 52, 44) * 150 + 40).astype(np.float32)
    frame = ((1.3, 0.9, 1.7), (-20.0, 5.0, 12.5), tuple(np.eye(3).ravel()))
    image = Image3d(vol, *frame)
    mean_probs, mask = segmentation_volume(model, _StageTta, image, None, None, True, batch_size=4)
    got = np.stack([p.array for p in mean_probs])
    # the same job by hand: resample to the model grid, sliding window with the three options, resample back
    iso = ([1.0, 1.0, 1.0], frame[1], frame[2])
    X, Y, Z = image.GetSize()
    size = image_tools.resampled_size((X, Y, Z), frame[0], iso[0], 16)
    src = torch.from_numpy(vol).to(hip_device)
    res = image_tools.resample_device(src, frame, size, iso, 'LINEAR', 0.0)
    starts, ends = image_partition_by_fixed_size((size, iso[0]), [0, 0, 0], list(size), [32, 32, 32], [16, 16, 16], 16)
    assert len(starts) > 8
    probs, _, _ = sliding_window_inference(model['net'], res, starts, (32, 32, 32), 2, {'type': 1, 'clip_sigma': 3},
                                           batch_size=4, blend='gaussian', sigma_scale=0.2, mirror_axes=('x', 'y'))
    back = torch.stack([image_tools.resample_device(probs[c], iso, (X, Y, Z), frame, 'LINEAR', 1.0 if c == 0 else 0.0)
                        for c in range(2)])
    # the same kernels on the same data in the same order: equal bit for bit
    assert np.array_equal(got, back.cpu().numpy())
    assert np.array_equal(mask.array, back.argmax(0).to(torch.int8).cpu().numpy())
    # the keys are read: without them the result is the constant, un-mirrored one, and the arguments override the config
    plain_probs, _ = segmentation_volume(model, _StagePlain, image, None, None, True, batch_size=4)
    plain = np.stack([p.array for p in plain_probs])
    assert float(np.abs(plain - got).max()) > 1e-4
    over_probs, _ = segmentation_volume(model, _StageTta, image, None, None, True, batch_size=4, blend='constant',
                                        mirror_axes=())
    assert np.array_equal(np.stack([p.array for p in over_probs]), plain)


_INFER_CFG = """from easydict import EasyDict as edict
__C = edict()
cfg = __C
__C.general = {}
__C.general.single_scale = 'fine'
__C.fine = {}
__C.fine.model_name = 'fine'
__C.fine.pick_largest_cc = False
__C.fine.remove_small_cc = 0
__C.fine.partition_type = 'SIZE'
__C.fine.partition_size = [32.0, 32.0, 32.0]
__C.fine.partition_stride = [16.0, 16.0, 16.0]
"""


def test_seg_infer_cli_blend_and_tta_flags(hip_device, tmp_path):
    from segmentation3d import seg_infer as cli
    from segmentation3d.core.seg_infer import load_single_model, segmentation_volume
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.image_io import read_image
    from segmentation3d.utils.mha_io import write_mha
    root = tmp_path / 'model'
    _save_model(root / 'fine', _kaiming_vnet('cpu', seed=10), (1.0, 1.0, 1.0))
    (root / 'infer_config.py').write_text(_INFER_CFG)
    rng = np.random.RandomState(52)
    vol = (rng.randn(48, 48, 64) * 100).astype(np.float32)
    image = Image3d(vol, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    write_mha(image, str(tmp_path / 'case.mha'))
    base = ['-i', str(tmp_path / 'case.mha'), '-m', str(root), '--save_prob']
    cli.main(base + ['-o', str(tmp_path / 'tta'), '--blend', 'gaussian', '--tta_mirror', 'x'])
    cli.main(base + ['-o', str(tmp_path / 'plain')])
    out = {k: (read_image(str(tmp_path / k / 'case.mha' / 'seg.mha'), dtype=None).array,
               np.stack([read_image(str(tmp_path / k / 'case.mha' / 'mean_prob_{}.mha'.format(c))).array for c in range(2)]))
           for k in ('tta', 'plain')}
    model = load_single_model(str(root / 'fine'), 0)

    class Tta(_StagePlain):
        blend_mode = 'gaussian'
        tta_mirror_axes = ['x']
    for key, stage in (('tta', Tta), ('plain', _StagePlain)):
        probs, mask = segmentation_volume(model, stage, image, None, None, True)
        assert np.array_equal(out[key][1], np.stack([p.array for p in probs])), key
        assert np.array_equal(out[key][0], mask.array), key
    assert float(np.abs(out['tta'][1] - out['plain'][1]).max()) > 1e-4
    with pytest.raises(ValueError, match='q'):
        cli.main(base + ['-o', str(tmp_path / 'bad'), '--tta_mirror', 'xq'])


# ---------------------------------------------------------------------------------------------------------------------
# 9. mirror augmentation of the training crops
# ---------------------------------------------------------------------------------------------------------------------
def _write_case(tmp_path, M):
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    rng = np.random.RandomState(61)
    frame = ((0.9, 1.1, 1.3), (-4.0, 2.0, 7.0), tuple(np.eye(3).ravel()))
    paths = []
    for m in range(M):
        write_mha(Image3d((rng.randn(40, 44, 48) * 100).astype(np.float32), *frame), str(tmp_path / 'im{}.mha'.format(m)))
        paths.append(str(tmp_path / 'im{}.mha'.format(m)))
    seg = (rng.rand(40, 44, 48) > 0.6).astype(np.int8) + (rng.rand(40, 44, 48) > 0.85).astype(np.int8)
    write_mha(Image3d(seg, *frame), str(tmp_path / 'seg.mha'))
    lst = tmp_path / 'train.txt'
    lst.write_text(('1\n' if M == 1 else '1 {}\n'.format(M)) + '\n'.join(paths) + '\n{}\n'.format(tmp_path / 'seg.mha'))
    return str(lst), frame


def _min_tie_distance(frame, center, crop_size, crop_spacing):
    """smallest distance (in source voxels) of a nearest-neighbour sample point of the crop grid to a half-voxel tie"""
    from segmentation3d.utils.image_tools import crop_origin, index_affine
    spacing = [float(v) for v in crop_spacing]
    M = index_affine(frame, (spacing, crop_origin(center, crop_size, spacing), frame[2]))
    d = 1.0
    for a in range(3):                                    # identity directions: the map is separable
        c = M[a, a] * np.arange(int(crop_size[a]), dtype=np.float64) + M[a, 3]
        d = min(d, float(np.abs((c - np.floor(c)) - 0.5).min()))
    return d


@pytest.mark.parametrize('M', [1, 2])
def test_mirrored_training_crop_equals_flipped_plain_crop(hip_device, tmp_path, M):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer, FixedNormalizer
    lst, frame = _write_case(tmp_path, M)
    norms = [AdaptiveNormalizer(), FixedNormalizer(10.0, 90.0, False)][:M]
    args = (lst, 3, [1.0, 1.0, 1.2], [32, 32, 16], 'GLOBAL', [3, 3, 3], [0.9, 1.1], 'LINEAR', norms)
    plain = SegmentationDataset(*args, device=hip_device)
    mirrored = SegmentationDataset(*args, device=hip_device, random_mirror_axes=('x', 'y', 'z'))
    seen = np.zeros(3, bool)
    for seed in range(6):
        np.random.seed(seed)
        center, crop_spacing = plain.sample_crop_geometry(0)
        flags = np.random.randint(0, 2, size=3).astype(bool)
        assert _min_tie_distance(frame, center, plain.crop_size, crop_spacing) > 1e-3, seed
        np.random.seed(seed)
        im_p, seg_p, frame_p, _ = plain.sample(0)
        np.random.seed(seed)
        im_m, seg_m, frame_m, _ = mirrored.sample(0)
        dims = [3 - a for a in range(3) if flags[a]]             # [c, z, y, x]
        want_im = torch.flip(im_p, dims) if dims else im_p
        want_seg = torch.flip(seg_p, dims) if dims else seg_p
        assert tuple(im_m.shape) == (M, 16, 32, 32)
        err = float((im_m - want_im).abs().max())
        print('mirrored crop M {} seed {} flags {}: max |image - flip| = {}'.format(M, seed, flags, err))
        assert err < 2e-5
        assert torch.equal(seg_m, want_seg)
        # the frame describes the mirrored grid: origin at the plain grid's last voxel, axis direction negated
        for a in range(3):
            if flags[a]:
                n = int(plain.crop_size[a])
                assert abs(frame_m[3 + a] - (frame_p[3 + a] + (n - 1) * frame_p[a])) < 1e-3
                assert frame_m[6 + 4 * a] == -frame_p[6 + 4 * a]
            else:
                assert frame_m[3 + a] == frame_p[3 + a] and frame_m[6 + 4 * a] == frame_p[6 + 4 * a]
        seen |= flags
    assert seen.all()
