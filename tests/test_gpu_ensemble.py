"""Model ensembling on the GPU: seg3d_ensemble_accumulate against the existing resampler
(bit for bit), against float64 restatements that do not use the resampler, the region rule, the identity grid, bad
arguments, and the file-level engine -- ensemble stages and the single-model path, which is the K = 1 case of the same
code -- against every member's probabilities brought to the image grid plane by plane with the resampler and labelled in
numpy, plus the single model's same-grid exit.

Bars: bit equality wherever the contract promises it.  General floats against float64: the accumulator holds values <= 1
and takes two float32 roundings per member (product and sum, each at most 2^-24) plus the float cast of the interpolated
value, under 4e-7 for three members; the bar is 1e-6.  The label map must equal the float64 arg-max wherever the float64
top-two gap is at least 2e-6 (twice the bar), and at most 0.1 % of the voxels may be closer than that."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
from test_ensemble import (EYE, accumulate_f32, argmax_first, compose_regions, dyadic_case, ensemble_f64,
                           member_planes_f64)

pytestmark = pytest.mark.gpu

# image grids (Z, Y, X): X = 10 takes the scalar path, X = 12 the 16-byte path
IMAGE_GRIDS = {'scalar': (11, 13, 10), 'vec': (11, 13, 12)}
IMG_FRAME = ((0.9, 1.1, 1.0), (-3.0, 2.0, 5.0), EYE)
# three members (Z, Y, X) with their own spacing and an origin shifted against the image's: part of the image grid lies
# outside each of them
MEMBER_GRIDS = [((6, 7, 9), (1.2, 1.9, 2.1), (-0.7, 0.4, -0.3)),
                ((5, 5, 5), (1.7, 2.3, 1.9), (1.1, 0.9, 1.3)),
                ((9, 8, 7), (1.3, 1.6, 1.1), (-0.2, 1.5, 0.6))]


def _member_frames():
    return [(sp, tuple(o + d for o, d in zip(IMG_FRAME[1], shift)), EYE) for _, sp, shift in MEMBER_GRIDS]


def _softmax_members(C, seed):
    rng = np.random.RandomState(seed)
    out = []
    for (shape, _, _), frame in zip(MEMBER_GRIDS, _member_frames()):
        logits = rng.randn(C, *shape) * 2.0
        e = np.exp(logits - logits.max(0))
        out.append(((e / e.sum(0)).astype(np.float32), frame))
    return out


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def _resampler_planes(probs_dev, frame, out_size, pad0, dst_frame=IMG_FRAME):
    """the s_c of one member from the existing single-plane resampler"""
    from segmentation3d.utils import image_tools
    return np.stack([image_tools.resample_device(probs_dev[c], frame, out_size, dst_frame, 'LINEAR',
                                                 pad0 if c == 0 else 0.0).cpu().numpy() for c in range(probs_dev.shape[0])])


# ---------------------------------------------------------------------------------------------------------------------
# 1. against the existing resampler, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', ['scalar', 'vec'])
@pytest.mark.parametrize('C', [1, 2, 3, 5, 16])
def test_equals_resampler_then_numpy_float32(hip_device, C, grid):
    from segmentation3d.core.seg_infer import ensemble_weights
    from segmentation3d.utils import image_tools
    Zo, Yo, Xo = IMAGE_GRIDS[grid]
    weights = ensemble_weights([5, 3, 2], 3)
    members = _softmax_members(C, 100 + C)
    acc = torch.full((C, Zo, Yo, Xo), float('nan'), dtype=torch.float32, device=hip_device)
    mask = torch.full((Zo, Yo, Xo), -7, dtype=torch.int8, device=hip_device)
    want = None
    for k, (p, frame) in enumerate(members):
        pd = _dev(p, hip_device)
        s = _resampler_planes(pd, frame, (Xo, Yo, Zo), 1.0)
        outside = s[0] == 1.0 if C > 1 else None
        if C > 1:       # a soft-max plane of C > 1 classes is below 1 inside: the padding and the interior both occur
            assert outside.any() and not outside.all()
        want = accumulate_f32(want, s, weights[k], k == 0)
        last = k == len(members) - 1
        got = image_tools.ensemble_accumulate_device(pd, frame, acc, IMG_FRAME, weights[k], k == 0, pad0=1.0,
                                                     mask=mask if last else None)
        assert got is acc
        assert np.array_equal(_bits(acc.cpu().numpy()), _bits(want)), 'member {}'.format(k)
        if not last:    # mask = None: the buffer is not touched
            assert bool((mask == -7).all())
    assert np.array_equal(mask.cpu().numpy(), argmax_first(want))
    assert C == 1 or len(np.unique(argmax_first(want))) >= 2


# ---------------------------------------------------------------------------------------------------------------------
# 2. against float64 without the resampler: the dyadic case is exact
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [3, 5, 7])
def test_dyadic_case_equals_float64(hip_device, C):
    from segmentation3d.utils import image_tools
    members, img_frame, (Xo, Yo, Zo), weights, ties = dyadic_case(C)
    want = ensemble_f64([member_planes_f64(p, f, img_frame, (Xo, Yo, Zo), 1.0) for p, f in members], weights)
    acc = torch.full((C, Zo, Yo, Xo), float('nan'), dtype=torch.float32, device=hip_device)
    mask = torch.full((Zo, Yo, Xo), -7, dtype=torch.int8, device=hip_device)
    for k, (p, frame) in enumerate(members):
        image_tools.ensemble_accumulate_device(_dev(p, hip_device), frame, acc, img_frame, weights[k], k == 0, pad0=1.0,
                                               mask=mask if k == 2 else None)
    got, got_m = acc.cpu().numpy(), mask.cpu().numpy()
    assert np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(got_m, argmax_first(want))
    for z, y, x in ties:        # classes C-2 and C-1 tie exactly: the lower index wins
        assert want[C - 2, z, y, x] == want[C - 1, z, y, x] == 0.5 and got_m[z, y, x] == C - 2


# ---------------------------------------------------------------------------------------------------------------------
# 3. regions
# ---------------------------------------------------------------------------------------------------------------------
ORDER16 = [5, 1, 9, 127, 2, 3, 3, 8, 100, 4, 6, 7, 11, 12, 13, 1]


@pytest.mark.parametrize('grid', ['scalar', 'vec'])
@pytest.mark.parametrize('order', [[2, 1, 3], [1, 4, 2], ORDER16], ids=['nested', 'plain', 'c16'])
def test_region_rule_equals_numpy(hip_device, order, grid):
    """two sigmoid-like members with pad0 = 0: accumulator and composed mask bit-equal to the resampler + numpy rule"""
    from segmentation3d.utils import image_tools
    C = len(order)
    Zo, Yo, Xo = IMAGE_GRIDS[grid]
    rng = np.random.RandomState(300 + C)
    weights = [0.625, 0.375]
    acc = torch.full((C, Zo, Yo, Xo), float('nan'), dtype=torch.float32, device=hip_device)
    mask = torch.full((Zo, Yo, Xo), -7, dtype=torch.int8, device=hip_device)
    want = None
    for k, ((shape, _, _), frame) in enumerate(list(zip(MEMBER_GRIDS, _member_frames()))[:2]):
        p = rng.rand(C, *shape).astype(np.float32)
        pd = _dev(p, hip_device)
        want = accumulate_f32(want, _resampler_planes(pd, frame, (Xo, Yo, Zo), 0.0), weights[k], k == 0)
        image_tools.ensemble_accumulate_device(pd, frame, acc, IMG_FRAME, weights[k], k == 0, pad0=0.0,
                                               mask=mask if k == 1 else None, regions_order=order)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(want))
    want_m = compose_regions(want, order)
    assert np.array_equal(mask.cpu().numpy(), want_m)
    assert (want_m == 0).any() and len(np.unique(want_m)) >= 3


@pytest.mark.parametrize('grid', ['scalar', 'vec'])
def test_region_threshold_is_strict(hip_device, grid):
    """identity grid, one member of weight 1: a plane at exactly 0.5 does not fire, the next float above does"""
    from segmentation3d.utils import image_tools
    Zo, Yo, Xo = IMAGE_GRIDS[grid]
    order = [2, 1, 3]
    frame = ((0.5, 2.0, 1.0), (4.0, -1.0, 0.25), EYE)          # (1 / s) * s is exactly 1: the index map is the identity
    above = np.nextafter(np.float32(0.5), np.float32(1.0))
    p = np.zeros((3, Zo, Yo, Xo), np.float32)
    p[0, :, :, 0::2] = 0.5              # never fires
    p[1, :, 0::2, :] = above            # fires where set
    p[2, 0::3] = 0.5
    p[2, 1::3] = above
    acc = torch.full(p.shape, float('nan'), dtype=torch.float32, device=hip_device)
    mask = torch.full((Zo, Yo, Xo), -7, dtype=torch.int8, device=hip_device)
    image_tools.ensemble_accumulate_device(_dev(p, hip_device), frame, acc, frame, 1.0, True, pad0=0.0, mask=mask,
                                           regions_order=order)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(p))
    want = compose_regions(p, order)
    assert set(np.unique(want)) == {0, 1, 3}            # label 2 (the plane at exactly 0.5) never appears
    assert np.array_equal(mask.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------------
# 4. identity grid
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', ['scalar', 'vec'])
def test_identity_grid_is_exact(hip_device, grid):
    from segmentation3d.utils import image_tools
    Zo, Yo, Xo = IMAGE_GRIDS[grid]
    frame = ((0.5, 2.0, 1.0), (4.0, -1.0, 0.25), EYE)          # (1 / s) * s is exactly 1: the index map is the identity
    rng = np.random.RandomState(41)
    p = rng.rand(4, Zo, Yo, Xo).astype(np.float32)
    p[0, 0, 0, 0], p[1, 1, 1, 1] = np.float32(1e-30), np.float32(3e-39)   # tiny and subnormal values survive
    w = np.float32(0.3)
    acc = torch.full(p.shape, float('nan'), dtype=torch.float32, device=hip_device)
    image_tools.ensemble_accumulate_device(_dev(p, hip_device), frame, acc, frame, float(w), True)
    first = acc.cpu().numpy()
    assert np.array_equal(_bits(first), _bits(w * p))
    image_tools.ensemble_accumulate_device(_dev(p, hip_device), frame, acc, frame, float(w), False)
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(first + w * p))


# ---------------------------------------------------------------------------------------------------------------------
# 5. bad arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_and_write_nothing(hip_device):
    from segmentation3d import _engine as E
    from segmentation3d.utils import image_tools
    src = torch.rand((17, 4, 5, 6), dtype=torch.float32, device=hip_device)
    acc = torch.full((17, 4, 5, 8), 3.5, dtype=torch.float32, device=hip_device)
    mask = torch.full((4, 5, 8), -7, dtype=torch.int8, device=hip_device)
    M = np.ascontiguousarray(np.eye(4)[:3], dtype=np.float64)

    def entry(C, order=None, s=src, a=acc):
        o = None if order is None else (ctypes.c_int * len(order))(*order)
        E.call('seg3d_ensemble_accumulate', E.ptr(s), E.ptr(a), E.ptr(mask), C, 6, 5, 4, 8, 5, 4,
               M.ctypes.data_as(ctypes.c_void_p), 1.0, 1, 1.0, o, E.stream_ptr())
    for C, order in ((0, None), (17, None), (-1, None), (3, [1, 0, 2]), (3, [1, 128, 2]), (3, [-1, 1, 2])):
        with pytest.raises(ValueError):
            entry(C, order)
    with pytest.raises(ValueError):
        entry(3, None, s=None)
    with pytest.raises(ValueError):
        entry(3, None, a=None)
    # the Python layer: C, dtypes, shapes, order
    good_p, good_a = src[:3].contiguous(), acc[:3].contiguous()
    bad = [dict(probs=src, acc=acc),                                                    # C = 17
           dict(probs=src[:0].contiguous(), acc=acc[:0].contiguous()),                  # C = 0
           dict(probs=good_p, acc=good_a.to(torch.int8)),                               # int8 acc
           dict(probs=good_p.double(), acc=good_a),
           dict(probs=good_p, acc=acc[:4].contiguous()),                                # plane counts differ
           dict(probs=good_p, acc=good_a, mask=mask.to(torch.int32)),
           dict(probs=good_p, acc=good_a, mask=mask[:3].contiguous()),
           dict(probs=good_p, acc=good_a[:, :, :, ::2]),                                # not contiguous
           dict(probs=good_p.cpu(), acc=good_a),
           dict(probs=good_p, acc=good_a, mask=mask, regions_order=[1, 0, 2]),
           dict(probs=good_p, acc=good_a, mask=mask, regions_order=[1, 128, 2]),
           dict(probs=good_p, acc=good_a, mask=mask, regions_order=[1, 2])]
    for kw in bad:
        kw = dict(kw)
        with pytest.raises(ValueError):
            image_tools.ensemble_accumulate_device(kw.pop('probs'), IMG_FRAME, kw.pop('acc'), IMG_FRAME, 1.0, True, **kw)
    torch.cuda.synchronize()
    assert bool((acc == 3.5).all()) and bool((good_a == 3.5).all()) and bool((mask == -7).all())


# ---------------------------------------------------------------------------------------------------------------------
# 7. general floats against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', ['scalar', 'vec'])
@pytest.mark.parametrize('C', [2, 3, 5])
def test_general_floats_against_float64(hip_device, C, grid):
    from segmentation3d.core.seg_infer import ensemble_weights
    from segmentation3d.utils import image_tools
    Zo, Yo, Xo = IMAGE_GRIDS[grid]
    weights = ensemble_weights([5, 3, 2], 3)
    members = _softmax_members(C, 700 + C)
    want = ensemble_f64([member_planes_f64(p, f, IMG_FRAME, (Xo, Yo, Zo), 1.0) for p, f in members], weights)
    acc = torch.full((C, Zo, Yo, Xo), float('nan'), dtype=torch.float32, device=hip_device)
    mask = torch.full((Zo, Yo, Xo), -7, dtype=torch.int8, device=hip_device)
    for k, (p, frame) in enumerate(members):
        image_tools.ensemble_accumulate_device(_dev(p, hip_device), frame, acc, IMG_FRAME, weights[k], k == 0, pad0=1.0,
                                               mask=mask if k == 2 else None)
    err = float(np.abs(acc.cpu().numpy().astype(np.float64) - want).max())
    top = np.sort(want, axis=0)
    decided = (top[-1] - top[-2]) >= 2e-6
    excluded = 1.0 - float(decided.mean())
    differs = int((mask.cpu().numpy() != argmax_first(want))[decided].sum())
    print('ensemble C = {} {}: max |acc - float64| = {:.3e}, excluded share = {:.5f}, mask differs at {} decided voxels'.format(
        C, grid, err, excluded, differs))
    assert err <= 1e-6
    assert excluded <= 1e-3
    assert differs == 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. end to end: the file-level engine
# ---------------------------------------------------------------------------------------------------------------------
_STAGE = """__C.{stage} = {{}}
__C.{stage}.model_name = '{name}'
__C.{stage}.pick_largest_cc = False
__C.{stage}.remove_small_cc = 0
__C.{stage}.partition_type = 'SIZE'
__C.{stage}.partition_size = [32.0, 32.0, 32.0]
__C.{stage}.partition_stride = [16.0, 16.0, 16.0]
"""


def _infer_cfg(scale, fine_extra='', coarse_name='coarse'):
    return ("from easydict import EasyDict as edict\n__C = edict()\ncfg = __C\n__C.general = {}\n"
            "__C.general.single_scale = '" + scale + "'\n" + _STAGE.format(stage='coarse', name=coarse_name)
            + _STAGE.format(stage='fine', name='fold_0') + fine_extra)


def _write_member(root, name, seed, spacing, sigmoid_order=None):
    """a randomly initialised vnet checkpoint as the model folder <root>/<name>"""
    import types
    from segmentation3d.network import vnet
    from segmentation3d.utils.model_io import checkpoint_state
    torch.manual_seed(seed)
    C = 2 if sigmoid_order is None else len(sigmoid_order)
    net = vnet.SegmentationNet(1, C) if sigmoid_order is None else vnet.SegmentationNet(1, C, output_activation='sigmoid')
    vnet.parameters_kaiming_init(net)
    cfg = types.SimpleNamespace(dataset=types.SimpleNamespace(spacing=[spacing] * 3, interpolation='LINEAR', num_classes=C,
                                                              crop_normalizers=[None]),
                                net=types.SimpleNamespace(name='vnet'))
    if sigmoid_order is None:
        state = checkpoint_state(net, 5, 1, cfg, 16, 1)
    else:
        state = checkpoint_state(net, 5, 1, cfg, 16, 1, regions=[[1, 2, 3], [1, 3], [3]], region_class_order=sigmoid_order)
    state['crop_normalizers'] = [{'type': 1, 'clip_sigma': 3}]
    chk = root / name / 'checkpoints' / 'chk_5'
    chk.mkdir(parents=True)
    torch.save(state, str(chk / 'params.pth'))


def _frame(image):
    return image.GetSpacing(), image.GetOrigin(), image.GetDirection()


def _model_grid(model, stage_cfg, image, start=None, end=None):
    """one model up to its finalized probabilities on its own grid -> (planes [C, Zp, Yp, Xp] on the device, iso_frame)"""
    from segmentation3d.core.seg_infer import _member_probabilities, blend_options
    blend, sigma_scale, axes = blend_options(stage_cfg)
    with torch.cuda.device(model['device']):
        probs, _, iso_frame, _ = _member_probabilities(model, stage_cfg, [image], start, end, 8, blend, sigma_scale, axes)
    return probs, iso_frame


def _alone(model, stage_cfg, image, start=None, end=None):
    """the image-grid result of one model WITHOUT the accumulate kernel: _member_probabilities, one resampler launch per
    plane (pad 1.0 for class 0 of a soft-max model, 0.0 for region planes), the label rule in numpy -> (planes, mask)"""
    probs, iso_frame = _model_grid(model, stage_cfg, image, start, end)
    order = model.get('region_class_order')
    planes = _resampler_planes(probs, iso_frame, image.GetSize(), 1.0 if order is None else 0.0, _frame(image))
    return planes, (argmax_first(planes) if order is None else compose_regions(planes, order))


@pytest.fixture(scope='module')
def e2e(tmp_path_factory, hip_device):
    """two soft-max members (spacings 1.0 and 1.5) and a coarse model as model folders, one 40 x 36 x 33 image at spacing
    0.8 as a file, and every member alone on the whole image, composed without the accumulate kernel (_alone: the shared
    reference)"""
    from segmentation3d.core.seg_infer import load_single_model
    from segmentation3d.utils.file_io import load_config
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    tmp = tmp_path_factory.mktemp('ensemble')
    root = tmp / 'model'
    _write_member(root, 'fold_0', 35, 1.0)
    _write_member(root, 'fold_1', 41, 1.5)
    _write_member(root, 'coarse', 37, 1.2)
    rng = np.random.RandomState(34)
    image = Image3d((rng.randn(40, 36, 33) * 100).astype(np.float32), (0.8, 0.8, 0.8), (1.0, -2.0, 3.0), EYE)
    write_mha(image, str(tmp / 'case.mha'))
    (root / 'infer_config.py').write_text(_infer_cfg('fine'))
    cfg = load_config(str(root / 'infer_config.py'))
    members = [load_single_model(str(root / n), 0) for n in ('fold_0', 'fold_1')]
    alone = [_alone(m, cfg.fine, image) for m in members]
    return dict(tmp=tmp, root=root, image=image, members=members, cfg=cfg, alone=alone)


REGION_ORDER = [2, 1, 3]


@pytest.fixture(scope='module')
def region_members(e2e):
    """two sigmoid members (spacings 1.0 and 1.5) with region order [2, 1, 3]"""
    from segmentation3d.core.seg_infer import load_single_model
    _write_member(e2e['root'], 'region_0', 51, 1.0, sigmoid_order=REGION_ORDER)
    _write_member(e2e['root'], 'region_1', 52, 1.5, sigmoid_order=REGION_ORDER)
    return [load_single_model(str(e2e['root'] / n), 0) for n in ('region_0', 'region_1')]


def _combine(alone, weights):
    """the members' image-grid probabilities (each from _alone) combined in the kernel's order"""
    acc = None
    for k, (planes, _) in enumerate(alone):
        acc = accumulate_f32(acc, planes, weights[k], k == 0)
    return acc


def _read_case(out):
    from segmentation3d.utils.image_io import read_image
    probs = np.stack([read_image(str(out / 'case.mha' / 'mean_prob_{}.mha'.format(c))).array for c in range(2)])
    return probs, read_image(str(out / 'case.mha' / 'seg.mha'), dtype=None).array


def test_segmentation_with_a_fine_ensemble(e2e):
    from segmentation3d.core.seg_infer import ensemble_weights, load_models, segmentation
    root, tmp = e2e['root'], e2e['tmp']
    (root / 'infer_config.py').write_text(_infer_cfg(
        'fine', "__C.fine.ensemble = ['fold_0', 'fold_1']\n__C.fine.ensemble_weights = [2, 1]\n"))
    models = load_models(str(root), 0)
    assert len(models.fine_members) == 2 and models.fine_model is models.fine_members[0]
    assert models.fine_weights == ensemble_weights([2, 1], 2) and models.coarse_model is None
    assert [list(m.spacing) for m in models.fine_members] == [[1.0] * 3, [1.5] * 3]
    masks = segmentation(str(tmp / 'case.mha'), str(root), str(tmp / 'out_ens'), 'seg.mha', 0, True, True, False, True)
    probs, written = _read_case(tmp / 'out_ens')
    want = _combine(e2e['alone'], ensemble_weights([2, 1], 2))
    assert np.array_equal(_bits(probs), _bits(want))
    assert np.array_equal(written, argmax_first(want)) and np.array_equal(masks[0].array, written)
    assert len(np.unique(written)) == 2
    # and the two members do differ: the mean is neither of them
    assert not np.array_equal(want, e2e['alone'][0][0])


def test_single_member_ensemble_writes_the_plain_files(e2e):
    from segmentation3d.core.seg_infer import load_models, segmentation
    root, tmp = e2e['root'], e2e['tmp']
    (root / 'infer_config.py').write_text(_infer_cfg('fine'))
    plain = load_models(str(root), 0)       # a stage without `ensemble`: one member, weight 1.0
    assert len(plain.fine_members) == 1 and plain.fine_model is plain.fine_members[0]
    assert plain.fine_weights == [1.0] and plain.coarse_model is None
    segmentation(str(tmp / 'case.mha'), str(root), str(tmp / 'out_plain'), 'seg.mha', 0, False, True, False, True)
    (root / 'infer_config.py').write_text(_infer_cfg('fine', "__C.fine.ensemble = ['fold_0']\n"))
    segmentation(str(tmp / 'case.mha'), str(root), str(tmp / 'out_one'), 'seg.mha', 0, False, True, False, True)
    for name in ('seg.mha', 'mean_prob_0.mha', 'mean_prob_1.mha'):
        a = (tmp / 'out_plain' / 'case.mha' / name).read_bytes()
        b = (tmp / 'out_one' / 'case.mha' / name).read_bytes()
        assert a == b and len(a) > 40 * 36 * 33, name


def test_cascade_with_a_fine_ensemble(e2e):
    """coarse: one model, fine: both members inside the coarse mask's bounding box = the manual composition"""
    from segmentation3d.core.seg_infer import ensemble_weights, load_single_model, segmentation, segmentation_volume
    from segmentation3d.utils.image_tools import get_bounding_box
    root, tmp, image, cfg = e2e['root'], e2e['tmp'], e2e['image'], e2e['cfg']
    (root / 'infer_config.py').write_text(_infer_cfg('DISABLE', "__C.fine.ensemble = ['fold_0', 'fold_1']\n"))
    segmentation(str(tmp / 'case.mha'), str(root), str(tmp / 'out_cascade'), 'seg.mha', 0, False, True, False, True)
    probs, written = _read_case(tmp / 'out_cascade')
    coarse = load_single_model(str(root / 'coarse'), 0)
    _, coarse_mask = segmentation_volume(coarse, cfg.coarse, image, None, None)
    start, end = get_bounding_box(coarse_mask, None)
    if start is None:
        start, end = [0, 0, 0], list(coarse_mask.GetSize())
    alone = [_alone(m, cfg.fine, image, list(start), list(end)) for m in e2e['members']]
    want = _combine(alone, ensemble_weights(None, 2))
    assert np.array_equal(_bits(probs), _bits(want))
    assert np.array_equal(written, argmax_first(want))


def test_sigmoid_members_compose_the_mask(e2e, region_members):
    from segmentation3d.core.seg_infer import segmentation_volume_ensemble
    image, cfg = e2e['image'], e2e['cfg']
    order, members = REGION_ORDER, region_members
    weights = [0.75, 0.25]
    probs, mask = segmentation_volume_ensemble(members, cfg.fine, image, None, None, weights=[3, 1])
    alone = [_alone(m, cfg.fine, image) for m in members]
    want = _combine(alone, weights)
    assert np.array_equal(_bits(np.stack([p.array for p in probs])), _bits(want))
    assert np.array_equal(mask.array, compose_regions(want, order)) and mask.array.dtype == np.int8
    with pytest.raises(ValueError):     # a soft-max and a sigmoid member do not mix
        segmentation_volume_ensemble([members[0], e2e['members'][0]], cfg.fine, image, None, None)


# ---------------------------------------------------------------------------------------------------------------------
# 8. a single model is the K = 1 case
# ---------------------------------------------------------------------------------------------------------------------
def _record_calls(monkeypatch):
    from segmentation3d import _engine as E
    calls = []
    real_call = E.call
    monkeypatch.setattr(E, 'call', lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    return calls


# (start, end) in image voxels (x, y, z); the fixture's image array is [Z, Y, X] = 40 x 36 x 33, so this is the whole x (33)
# and y (36) extent and 12 of the 40 z planes -- one 32 x 32 x 16 patch on either member's grid
BBOX = ([0, 0, 10], [33, 36, 22])


@pytest.mark.parametrize('bbox', [None, BBOX], ids=['whole', 'bbox'])
@pytest.mark.parametrize('kind', ['softmax', 'sigmoid'])
def test_single_model_equals_the_resampler_composition(e2e, region_members, monkeypatch, kind, bbox):
    """segmentation_volume on an image that is not on the model's grid: probabilities and mask bit-equal to the planes
    resampled one by one and labelled in numpy, from exactly one accumulate launch and no resampler launch behind the
    sliding window"""
    from segmentation3d.core.seg_infer import segmentation_volume
    image, cfg = e2e['image'], e2e['cfg']
    start, end = (None, None) if bbox is None else bbox
    for k, model in enumerate(e2e['members'] if kind == 'softmax' else region_members):
        if kind == 'softmax' and bbox is None:
            want, want_m = e2e['alone'][k]
        else:
            want, want_m = _alone(model, cfg.fine, image, None if start is None else list(start),
                                  None if end is None else list(end))
        calls = _record_calls(monkeypatch)
        probs, mask = segmentation_volume(model, cfg.fine, image, None if start is None else list(start),
                                          None if end is None else list(end))
        monkeypatch.undo()
        got = np.stack([p.array for p in probs])
        uncovered = (want == 0).all(0)
        print('single {} member {} {}: labels {}, uncovered voxels {}'.format(
            kind, k, 'whole' if bbox is None else 'bbox', np.unique(want_m).tolist(), int(uncovered.sum())))
        assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(mask.array, want_m) and mask.array.dtype == np.int8
        assert len(np.unique(want_m)) >= 2
        if bbox is not None:        # no patch covered them: count 0, every probability 0, label 0
            assert uncovered.any() and (got[:, uncovered] == 0).all() and (mask.array[uncovered] == 0).all()
        assert calls.count('seg3d_ensemble_accumulate') == 1
        tail = max(i for i, n in enumerate(calls) if n.startswith('seg3d_finalize_'))
        assert not [n for n in calls[tail:] if n.startswith('seg3d_resample_affine')]


@pytest.mark.parametrize('kind', ['softmax', 'sigmoid'])
def test_single_model_same_grid_exit(e2e, region_members, monkeypatch, kind):
    """a 32^3 image at the model's spacing (stride 16 divides it): segmentation_volume returns the sliding window's
    finalized planes as they stand and their label map, and launches no accumulate"""
    from segmentation3d.core.seg_infer import segmentation_volume
    from segmentation3d.utils.image3d import Image3d
    model = e2e['members'][0] if kind == 'softmax' else region_members[0]
    rng = np.random.RandomState(77)
    image = Image3d((rng.randn(32, 32, 32) * 100).astype(np.float32), (1.0, 1.0, 1.0), (1.0, -2.0, 3.0), EYE)
    planes, _ = _model_grid(model, e2e['cfg'].fine, image)
    want = planes.cpu().numpy()
    assert want.shape[1:] == (32, 32, 32)
    calls = _record_calls(monkeypatch)
    probs, mask = segmentation_volume(model, e2e['cfg'].fine, image, None, None)
    monkeypatch.undo()
    assert np.array_equal(_bits(np.stack([p.array for p in probs])), _bits(want))
    want_m = argmax_first(want) if kind == 'softmax' else compose_regions(want, REGION_ORDER)
    assert np.array_equal(mask.array, want_m) and mask.array.dtype == np.int8
    assert calls.count('seg3d_ensemble_accumulate') == 0 and any(n.startswith('seg3d_finalize_') for n in calls)


def test_single_model_plane_limit_names_out_channels(e2e):
    """the image-grid launch takes 1..16 planes: a wider model on another grid is refused in Python, before any launch"""
    from segmentation3d.core.seg_infer import segmentation_volume
    model = dict(e2e['members'][0], out_channels=17)
    with pytest.raises(ValueError, match='out_channels = 17'):
        segmentation_volume(model, e2e['cfg'].fine, e2e['image'], None, None)
