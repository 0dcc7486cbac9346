"""Region-based models on the GPU: the sigmoid head, the region mask composition and the region overlap counts against
float64 / numpy restatements written here with stock torch and numpy; the sliding window and the file-level engine with a
region model.

Bars are the project's parity bars (tests/test_gpu_compound_loss.py): O(1) loss terms and probabilities within 1e-4 of the
float64 oracle, gradients within gpu_util.rel_err < 1e-4, exact zeros and integer results bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
from gpu_util import max_err, rel_err, report
from test_blend_tta import oracle_finalize, oracle_sliding_window

pytestmark = pytest.mark.gpu

BRATS = [[1, 2, 3], [1, 3], [3]]
R16 = [[1, 2, 3], [1, 3], [3], [2], [7, 1], [2, 3]] + [[k] for k in range(10, 19)] + [[255, 3]]


# ---------------------------------------------------------------------------------------------------------------------
# 1. sigmoid head
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('spatial', [(5, 7, 9), (1, 1, 1)])
@pytest.mark.parametrize('C', [1, 3, 16])
def test_sigmoid_forward_backward_equal_float64(hip_device, C, spatial):
    """N = 2 on a ragged 5 x 7 x 9 volume (S = 315, no multiple of any vector width) and on S = 1; the inputs carry 0, +-20
    and +-100: finite outputs inside [0, 1]"""
    from segmentation3d import _ops
    g = torch.Generator().manual_seed(10 + C)
    x = 3.0 * torch.randn((2, C) + spatial, generator=g)
    special = torch.tensor([0.0, 20.0, -20.0, 100.0, -100.0])
    flat = x.reshape(-1)
    flat[:min(5, flat.numel())] = special[:min(5, flat.numel())]
    if flat.numel() > 10:
        flat[-5:] = special
    dp = torch.randn(x.shape, generator=g)
    xg = x.to(hip_device).requires_grad_(True)
    p = _ops.sigmoid_channels(xg)
    p.backward(dp.to(hip_device))
    torch.cuda.synchronize()
    assert p.is_contiguous() and p.shape == x.shape
    xr = x.double().requires_grad_(True)
    pr = torch.sigmoid(xr)
    pr.backward(dp.double())
    got = p.detach().cpu()
    errs = {'probs': max_err(got, pr.detach()), 'din_rel': rel_err(xg.grad, xr.grad)}
    report('sigmoid_C{}_S{}'.format(C, int(np.prod(spatial))), **errs)
    print('sigmoid', C, spatial, errs)
    assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert bool(torch.isfinite(xg.grad).all())
    assert errs['probs'] < 1e-4 and errs['din_rel'] < 1e-4, errs


def test_sigmoid_refuses_bf16_logits(hip_device):
    from segmentation3d import _ops
    with pytest.raises(ValueError, match='float32'):
        _ops.sigmoid_channels(torch.zeros((1, 16, 2, 2, 2), dtype=torch.bfloat16, device=hip_device))


# ---------------------------------------------------------------------------------------------------------------------
# 3. seg3d_finalize_regions
# ---------------------------------------------------------------------------------------------------------------------
def _numpy_finalize_regions(acc, cnt, order):
    with np.errstate(divide='ignore'):
        r = np.where(cnt > 0, np.float32(1.0) / cnt, np.float32(0.0)).astype(np.float32)
    probs = (acc * r[None]).astype(np.float32)
    mask = np.zeros(cnt.shape, np.int8)
    for k, label in enumerate(order):
        mask[probs[k] > np.float32(0.5)] = label
    return probs, mask


@pytest.mark.parametrize('order', [[1, 2, 3], [5, 127, 9]])
def test_finalize_regions_equals_numpy(hip_device, order):
    """nested regions (order 1, 2, 3 on planes that mostly nest) and non-nested ones, voxels nobody covered (count 0),
    p = 0.5 exactly (the bit is not set), a voxel count that is no multiple of the block"""
    from segmentation3d import _engine as E
    rng = np.random.RandomState(7)
    Z, Y, X, R = 5, 7, 11, 3
    cnt = rng.choice(np.array([0.0, 1.0, 2.0, 3.0, 4.0], np.float32), size=(Z, Y, X)).astype(np.float32)
    acc = (rng.rand(R, Z, Y, X).astype(np.float32) * cnt[None]).astype(np.float32)
    acc[1] = np.minimum(acc[1], acc[0])
    acc[:, 0, 0, :4] = np.array([1.0, 1.0, 1.0, 1.0], np.float32) * np.array([[1.0], [1.0], [0.5]], np.float32)
    cnt[0, 0, :4] = np.array([2.0, 1.0, 2.0, 4.0], np.float32)       # p = 0.5, 1, 0.5, 0.25 on planes 0 and 1
    cnt[0, 1, :3] = 0.0
    acc[:, 0, 1, :3] = 0.0
    want_p, want_m = _numpy_finalize_regions(acc, cnt, order)
    assert (want_p == 0.5).any() and (cnt == 0).any() and len(set(np.unique(want_m))) >= 3
    a, c = torch.from_numpy(acc).to(hip_device), torch.from_numpy(cnt).to(hip_device)
    m = torch.full((Z, Y, X), -7, dtype=torch.int8, device=hip_device)
    E.call('seg3d_finalize_regions', E.ptr(a), E.ptr(c), E.ptr(m), R, (ctypes.c_int * R)(*order), Z * Y * X, 0,
           E.stream_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy().view(np.uint32), want_p.view(np.uint32))
    assert np.array_equal(m.cpu().numpy(), want_m)
    assert np.array_equal(m.cpu().numpy()[cnt == 0], np.zeros(int((cnt == 0).sum()), np.int8))


def test_finalize_regions_z_slab_with_class_stride(hip_device):
    """a z-slab call as the sharded sliding window makes it: class_stride = the whole volume, voxels = the slab; planes
    outside the slab are not touched"""
    from segmentation3d.core.seg_infer import SlidingWindowBatcher
    rng = np.random.RandomState(8)
    Z, Y, X, R = 8, 6, 10, 3
    vol = torch.zeros((Z, Y, X), dtype=torch.float32, device=hip_device)
    b = SlidingWindowBatcher(vol, [[0, 0, 0]], (X, Y, Z), R, None, max_batch=1)
    cnt = rng.randint(0, 4, size=(Z, Y, X)).astype(np.float32)
    acc = (rng.rand(R, Z, Y, X).astype(np.float32) * cnt[None]).astype(np.float32)
    b.acc.copy_(torch.from_numpy(acc))
    b.count.copy_(torch.from_numpy(cnt))
    probs, mask = b.finalize((2, 5), regions_order=[1, 2, 3])
    torch.cuda.synchronize()
    want_p, want_m = _numpy_finalize_regions(acc, cnt, [1, 2, 3])
    got_p, got_m = probs.cpu().numpy(), mask.cpu().numpy()
    assert np.array_equal(got_p[:, 2:5], want_p[:, 2:5]) and np.array_equal(got_m[2:5], want_m[2:5])
    assert np.array_equal(got_p[:, :2], acc[:, :2]) and np.array_equal(got_p[:, 5:], acc[:, 5:])
    assert not got_m[:2].any() and not got_m[5:].any()
    with pytest.raises(ValueError):
        b.finalize(regions_order=[1, 2])
    with pytest.raises(ValueError):
        b.finalize(regions_order=[1, 2, 128])


# ---------------------------------------------------------------------------------------------------------------------
# 4. seg3d_region_overlap_counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.int8, np.uint8, np.int16, np.int32, np.float32])
def test_region_overlap_counts_equal_numpy(hip_device, dtype):
    """16 regions in one pass, n = 3 * 4099 (no multiple of the block), every dtype; values outside [0, 256), negative ones
    and -- for float -- fractions belong to no region"""
    from segmentation3d.utils.metrics import cal_region_dsc, region_overlap_counts
    rng = np.random.RandomState(11)
    n = 3 * 4099
    pool = np.array([0, 1, 2, 3, 7, 10, 11, 18, 100], np.int64)
    if dtype == np.uint8:
        pool = np.append(pool, [255, 200])
    elif dtype == np.int8:
        pool = np.append(pool, [-1, -128, 127])
    else:
        pool = np.append(pool, [255, 256, 300, -1, -255])
    gt = pool[rng.randint(0, len(pool), n)].astype(dtype)
    seg = np.where(rng.rand(n) < 0.6, gt, pool[rng.randint(0, len(pool), n)].astype(dtype)).astype(dtype)
    if dtype == np.float32:
        gt[:50], seg[25:75] = 1.5, 2.25
    want = [(int(np.isin(gt, r).sum()), int(np.isin(seg, r).sum()), int((np.isin(gt, r) & np.isin(seg, r)).sum()))
            for r in R16]
    got = region_overlap_counts(gt.reshape(3, 4099), seg.reshape(3, 4099), R16, device=hip_device)
    assert got == want
    assert sum(c for _, _, c in want) > 0
    # and the Dice convention on top of it
    scores = cal_region_dsc(gt, seg, BRATS, 10)
    for (score, kind), (a, b, c) in zip(scores, want[:3]):
        assert kind == 'TP' and score == 2 * c / (a + b)


_LABELS17 = {                                  # 17 labels the dtype represents: one pass of 16 and one of 1
    np.int8: [-128, -1, 127, 0, 1, 2, 3, 7, 10, 11, 18, 100, 5, 50, -100, 64, -64],
    np.uint8: [200, 255, 0, 1, 2, 3, 7, 10, 11, 18, 100, 5, 50, 128, 64, 254, 199],
    np.int16: [-255, 256, 300, 0, 1, 2, 3, 7, 10, 11, 18, 100, 255, -1, 5, 50, 1000],
    np.int32: [-255, 256, 300, 0, 1, 2, 3, 7, 10, 11, 18, 100, 255, -1, 5, 50, 1000],
    np.float32: [-255, 256, 300, 0, 1, 2, 3, 7, 10, 11, 18, 100, 255, -1, 5, 50, 1000],
}


@pytest.mark.parametrize('dtype', [np.int8, np.uint8, np.int16, np.int32, np.float32])
def test_label_overlap_counts_every_dtype(hip_device, dtype):
    """17 labels (two passes), n = 3 * 4099 (four blocks, the last partial) and n = 1, every dtype: negative labels, labels
    above 255 and -- for float -- fractional voxels, which equal no label; equal to the numpy restatement as Python ints"""
    from oracle import numpy_ref
    from segmentation3d.utils.metrics import label_overlap_counts
    labels = _LABELS17[dtype]
    assert len(labels) == 17 and all(dtype(l) == l for l in labels)
    rng = np.random.RandomState(12)
    n = 3 * 4099
    pool = np.array(labels[:14] + labels[16:] + [9, 33], np.int64)    # labels 14 and 15 stay absent, 9 and 33 are no labels
    gt = pool[rng.randint(0, len(pool), n)].astype(dtype)
    seg = np.where(rng.rand(n) < 0.6, gt, pool[rng.randint(0, len(pool), n)].astype(dtype)).astype(dtype)
    if dtype == np.float32:
        gt[:50], seg[25:75] = 1.5, 2.25
    one = np.array([labels[16]], dtype)                               # n = 1: counted by the second pass
    for g, s in ((gt.reshape(3, 4099), seg.reshape(3, 4099)), (one, one.copy())):
        want = numpy_ref.label_overlap_counts(g, s, labels)
        got = label_overlap_counts(g, s, labels, device=hip_device)
        assert got == want and all(type(v) is int for row in got for v in row)
        assert sum(c for _, _, c in want) > 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. the sigmoid network
# ---------------------------------------------------------------------------------------------------------------------
def _train_data(device):
    g = torch.Generator().manual_seed(31)
    t = torch.tensor([0.0, 1.0, 2.0, 3.0, 255.0])[torch.randint(0, 5, (2, 1, 8, 8, 8), generator=g)]
    t = t.repeat_interleave(4, 2).repeat_interleave(4, 3).repeat_interleave(4, 4)          # 2 x 1 x 32^3, blocky labels
    x = torch.cat([(t == l).float() for l in (1.0, 2.0, 3.0, 0.0)], 1) * 2.0 - 1.0 + 0.3 * torch.randn((2, 4, 32, 32, 32),
                                                                                                     generator=g)
    return x.to(device), t.to(device)


def test_sigmoid_network_in_bf16_mode(hip_device):
    """bf16 activation mode keeps a head below 16 channels in fp32, so the sigmoid receives what it receives in fp32 mode:
    one forward + backward, probabilities inside [0, 1] and close to the fp32 mode's"""
    from segmentation3d import _ops
    from segmentation3d.network import vnet
    x, _ = _train_data(hip_device)
    torch.manual_seed(5)
    net = vnet.SegmentationNet(4, 3, output_activation='sigmoid')
    vnet.parameters_kaiming_init(net)
    net = net.to(hip_device)
    out = {}
    try:
        for mode in ('fp32', 'bf16'):
            with _ops.activation_dtype(mode):
                p = net(x)
                p.sum().backward()
                torch.cuda.synchronize()
                out[mode] = p.detach().cpu()
                assert p.dtype == torch.float32 and bool(torch.isfinite(net.out_block.conv2.weight.grad).all())
            _ops.PACK_CACHE.clear()
    finally:
        _ops.PACK_CACHE.clear()
    assert float(out['bf16'].min()) >= 0.0 and float(out['bf16'].max()) <= 1.0
    err = max_err(out['bf16'], out['fp32'])
    print('sigmoid net bf16 vs fp32', err)
    assert err < 3e-2       # the bf16 mode's bar on probabilities (tests/test_gpu_bf16.py)


# ---------------------------------------------------------------------------------------------------------------------
# 6. sliding window and the file-level engine
# ---------------------------------------------------------------------------------------------------------------------
def _region_vnet(device, cin, seed):
    from segmentation3d.network import vnet
    torch.manual_seed(seed)
    net = vnet.SegmentationNet(cin, 3, output_activation='sigmoid')
    vnet.parameters_kaiming_init(net)
    return net.to(device).eval()


def _axis_starts(n, b, stride):
    s = list(range(0, n - b + 1, stride))
    if s[-1] != n - b:
        s.append(n - b)
    return s


@pytest.mark.parametrize('blend,axes', [('constant', ()), ('gaussian', ('x',))])
def test_sliding_window_with_regions_equals_the_host_restatement(hip_device, blend, axes):
    """a sigmoid network on a 40^3 volume, box 32 at stride 16: the second patch of every axis is clamped to the border, so
    all eight patches overlap.  Probabilities and mask equal the float32 numpy accumulate / divide / compose of the per-batch
    network outputs (the same forwards on the same inputs, accumulated in the contract's order)"""
    from segmentation3d.core.seg_infer import SlidingWindowBatcher, sliding_window_inference
    net = _region_vnet(hip_device, 1, 12)
    rng = np.random.RandomState(13)
    shape, box, B, order = (40, 40, 40), (32, 32, 32), 4, [2, 1, 3]
    vol = torch.from_numpy((rng.randn(*shape) * 150 + 20).astype(np.float32)).to(hip_device)
    starts = [[x, y, z] for z in _axis_starts(40, 32, 16) for y in _axis_starts(40, 32, 16) for x in _axis_starts(40, 32, 16)]
    assert len(starts) == 8 and starts[-1] == [8, 8, 8]
    norm = {'type': 1, 'clip_sigma': 3.0}
    probs, mask, _ = sliding_window_inference(net, vol, starts, box, 3, norm, batch_size=B, two_streams=False, blend=blend,
                                              mirror_axes=axes, regions_order=order)
    torch.cuda.synchronize()
    batcher = SlidingWindowBatcher(vol, starts, box, 3, norm, max_batch=1)
    patches = [batcher.gather([k])[0].cpu().numpy() for k in range(len(starts))]

    def net_fn(a):
        with torch.no_grad():
            return net(torch.from_numpy(a).to(hip_device)).cpu().numpy()
    acc, cnt = oracle_sliding_window(lambda k: patches[k], net_fn, shape, starts, box, 3, B, axes, blend=blend)
    want_p, _ = oracle_finalize(acc, cnt)
    want_m = np.zeros(shape, np.int8)
    for r, label in enumerate(order):
        want_m[want_p[r] > np.float32(0.5)] = label
    got_p, got_m = probs.cpu().numpy(), mask.cpu().numpy()
    err = float(np.abs(got_p - want_p).max())
    print('region sliding window', blend, axes, 'max |probs - restatement| =', err, 'mask differs at',
          int((got_m != want_m).sum()))
    report('region_sliding_{}'.format(blend), probs=err, mask_diff=float((got_m != want_m).sum()))
    assert cnt.min() > 0 and float(cnt.max()) > float(cnt.min())
    assert len(np.unique(want_m)) >= 3          # the composition has something to compose
    assert np.array_equal(got_p, want_p)
    assert np.array_equal(got_m, want_m)


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


def test_end_to_end_through_files(hip_device, tmp_path):
    """a randomly initialised region checkpoint + infer_config.py -> segmentation() on a small .mha -> the written mask holds
    only 0 and the region_class_order labels, and scores 1.0 against itself for every present region"""
    import types
    from segmentation3d.core.seg_eval import cal_dsc_batch
    from segmentation3d.core.seg_infer import load_single_model, segmentation
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.image_io import read_image
    from segmentation3d.utils.mha_io import write_mha
    from segmentation3d.utils.model_io import checkpoint_state
    order = [2, 1, 3]
    net = _region_vnet('cpu', 1, 14)
    cfg = types.SimpleNamespace(dataset=types.SimpleNamespace(spacing=[1.0, 1.0, 1.0], interpolation='LINEAR', num_classes=3,
                                                              crop_normalizers=[None]),
                                net=types.SimpleNamespace(name='vnet'))
    state = checkpoint_state(net, 5, 1, cfg, 16, 1, regions=BRATS, region_class_order=order)
    state['crop_normalizers'] = [{'type': 1, 'clip_sigma': 3}]
    root = tmp_path / 'model'
    chk = root / 'fine' / 'checkpoints' / 'chk_5'
    chk.mkdir(parents=True)
    torch.save(state, str(chk / 'params.pth'))
    (root / 'infer_config.py').write_text(_INFER_CFG)
    model = load_single_model(str(root / 'fine'), 0)
    assert model.output_activation == 'sigmoid' and model.regions == BRATS and model.region_class_order == order
    assert hasattr(model.net.out_block, 'sigmoid')
    rng = np.random.RandomState(15)
    image = Image3d((rng.randn(40, 48, 40) * 100).astype(np.float32), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0),
                    tuple(np.eye(3).ravel()))
    write_mha(image, str(tmp_path / 'case.mha'))
    masks = segmentation(str(tmp_path / 'case.mha'), str(root), str(tmp_path / 'out'), 'seg.mha', 0, True, True, False, True)
    seg_path = str(tmp_path / 'out' / 'case.mha' / 'seg.mha')
    written = read_image(seg_path, dtype=None).array
    assert np.array_equal(written, masks[0].array) and written.shape == (40, 48, 40)
    values = set(int(v) for v in np.unique(written))
    assert values <= {0} | set(order) and len(values) >= 2
    # the written probabilities compose to the written mask
    probs = np.stack([read_image(str(tmp_path / 'out' / 'case.mha' / 'mean_prob_{}.mha'.format(r))).array for r in range(3)])
    want = np.zeros(written.shape, np.int8)
    for r, label in enumerate(order):
        want[probs[r] > np.float32(0.5)] = label
    assert np.array_equal(written, want)
    # every region of the order's labels scores 1.0 against itself where it is present
    regions = [[l] for l in sorted(set(order))] + [sorted(set(order))]
    table = cal_dsc_batch([seg_path], [seg_path], [1, 2, 3], 1, None, regions=regions)
    for k, region in enumerate(regions):
        present = np.isin(written, region).sum() >= 1
        assert table['region{}_type'.format(k)].iloc[0] == ('TP' if present else 'TN')
        assert table['region{}_score'.format(k)].iloc[0] == 1.0
