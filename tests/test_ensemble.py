"""Model ensembling, host side: the weight normalisation, the stage keys of infer_config.py and
the member compatibility check, plus the numpy restatements of seg3d_ensemble_accumulate that tests/test_gpu_ensemble.py
compares the kernel with.  Nothing here needs a GPU."""
import types

import numpy as np
import pytest

from conftest import REPO  # noqa: F401
from segmentation3d.core.seg_infer import check_ensemble_members, ensemble_options, ensemble_weights
from segmentation3d.utils.image_tools import index_affine


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatements of the kernel's contract (include/seg3d_hip.h, seg3d_ensemble_accumulate)
# ---------------------------------------------------------------------------------------------------------------------
def resample_linear_f64(src, M, out_size):
    """src [Zi, Yi, Xi] sampled at c = M (x, y, z, 1) for every index of the (Xo, Yo, Zo) grid, in float64 and in the
    contract's order: inside iff -0.5 <= c < size - 0.5 per axis, the 8-neighbourhood clamped at the borders, lerp along x,
    then y, then z.  -> (values float64 [Zo, Yo, Xo] (0 outside), inside bool [Zo, Yo, Xo])"""
    src = np.asarray(src, dtype=np.float64)
    Zi, Yi, Xi = src.shape
    Xo, Yo, Zo = out_size
    z, y, x = np.meshgrid(np.arange(Zo, dtype=np.float64), np.arange(Yo, dtype=np.float64),
                          np.arange(Xo, dtype=np.float64), indexing='ij')
    M = np.asarray(M, dtype=np.float64)
    cx = M[0, 0] * x + M[0, 1] * y + M[0, 2] * z + M[0, 3]
    cy = M[1, 0] * x + M[1, 1] * y + M[1, 2] * z + M[1, 3]
    cz = M[2, 0] * x + M[2, 1] * y + M[2, 2] * z + M[2, 3]
    inside = (cx >= -0.5) & (cx < Xi - 0.5) & (cy >= -0.5) & (cy < Yi - 0.5) & (cz >= -0.5) & (cz < Zi - 0.5)
    fx, fy, fz = np.clip(cx, 0.0, Xi - 1.0), np.clip(cy, 0.0, Yi - 1.0), np.clip(cz, 0.0, Zi - 1.0)
    x0, y0, z0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64), np.floor(fz).astype(np.int64)
    x1, y1, z1 = np.minimum(x0 + 1, Xi - 1), np.minimum(y0 + 1, Yi - 1), np.minimum(z0 + 1, Zi - 1)
    dx, dy, dz = fx - x0, fy - y0, fz - z0
    v000, v100, v010, v110 = src[z0, y0, x0], src[z0, y0, x1], src[z0, y1, x0], src[z0, y1, x1]
    v001, v101, v011, v111 = src[z1, y0, x0], src[z1, y0, x1], src[z1, y1, x0], src[z1, y1, x1]
    a00, a01 = v000 + (v100 - v000) * dx, v010 + (v110 - v010) * dx
    a10, a11 = v001 + (v101 - v001) * dx, v011 + (v111 - v011) * dx
    b0, b1 = a00 + (a01 - a00) * dy, a10 + (a11 - a10) * dy
    return np.where(inside, b0 + (b1 - b0) * dz, 0.0), inside


def member_planes_f64(probs, src_frame, dst_frame, out_size, pad0):
    """the s_c of one member in float64 (not yet rounded to float32): probs [C, Zi, Yi, Xi] -> [C, Zo, Yo, Xo]"""
    M = index_affine(src_frame, dst_frame)
    out = []
    for c in range(probs.shape[0]):
        v, inside = resample_linear_f64(probs[c], M, out_size)
        out.append(np.where(inside, v, pad0 if c == 0 else 0.0))
    return np.stack(out)


def accumulate_f32(acc, s, weight, first):
    """a = first ? w * s : acc + w * s in float32: one rounding for the product, one for the sum"""
    p = np.float32(weight) * np.asarray(s, dtype=np.float32)
    assert p.dtype == np.float32
    return p if first else (np.asarray(acc, dtype=np.float32) + p).astype(np.float32)


def ensemble_f32(planes, weights):
    """planes: per member the float32 s_c [C, Zo, Yo, Xo] -> the accumulator after every member (list of float32 arrays)"""
    out, acc = [], None
    for k, (s, w) in enumerate(zip(planes, weights)):
        acc = accumulate_f32(acc, s, w, k == 0)
        out.append(acc)
    return out


def ensemble_f64(planes, weights):
    acc = np.zeros(planes[0].shape, dtype=np.float64)
    for s, w in zip(planes, weights):
        acc = acc + float(np.float32(w)) * np.asarray(s, dtype=np.float64)      # (the kernel takes the weight as a float32)
    return acc


def argmax_first(acc):
    """first maximum wins: class 0, replaced only by a strictly greater value"""
    return np.argmax(acc, axis=0).astype(np.int8)


def compose_regions(acc, order):
    mask = np.zeros(acc.shape[1:], dtype=np.int8)
    for r, label in enumerate(order):
        mask[acc[r] > np.float32(0.5)] = label
    return mask


EYE = tuple(np.eye(3).ravel())


def dyadic_case(C=3, seed=5):
    """the case in which every intermediate is exact in float32: members at exactly twice the image spacing with the image's
    origin (lerp fractions in {0, 0.5}), probabilities multiples of 1/64, weights 0.5, 0.25, 0.25.  At the source voxels
    (1, 1, 1) and (2, 3, 2) of every member the classes C-2 and C-1 tie at 0.5 (all others 0), so they tie in the mean at
    the image voxels (2, 2, 2) and (4, 6, 4).
    -> (members [(probs [C, Zi, Yi, Xi] float32, frame)], image frame, (Xo, Yo, Zo), weights, tie voxels (z, y, x))"""
    rng = np.random.RandomState(seed)
    img_frame = ((1.0, 1.0, 1.0), (-3.0, 2.0, 5.0), EYE)
    out_size = (12, 13, 11)
    members = []
    for Zi, Yi, Xi in ((6, 7, 6), (5, 6, 5), (6, 7, 7)):
        p = (rng.randint(0, 65, size=(C, Zi, Yi, Xi)) / 64.0).astype(np.float32)
        for z, y, x in ((1, 1, 1), (2, 3, 2)):
            p[:, z, y, x] = 0.0
            p[max(C - 2, 0):, z, y, x] = 0.5
        members.append((p, ((2.0, 2.0, 2.0), img_frame[1], EYE)))
    return members, img_frame, out_size, [0.5, 0.25, 0.25], [(2, 2, 2), (4, 6, 4)]


def test_float32_restatement_equals_float64_on_the_dyadic_case():
    members, img_frame, out_size, weights, ties = dyadic_case()
    s64 = [member_planes_f64(p, f, img_frame, out_size, 1.0) for p, f in members]
    s32 = [s.astype(np.float32) for s in s64]
    for a, b in zip(s32, s64):
        assert np.array_equal(a.astype(np.float64), b)          # the interpolated values are float32 numbers already
    inside = resample_linear_f64(members[1][0][0], index_affine(members[1][1], img_frame), out_size)[1]
    assert inside.any() and not inside.all()                    # the padding takes part
    got = ensemble_f32(s32, weights)[-1]
    want = ensemble_f64(s64, weights)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    for z, y, x in ties:
        assert want[1, z, y, x] == want[2, z, y, x] == 0.5 and want[0, z, y, x] == 0.0
        assert argmax_first(got)[z, y, x] == 1                  # the lower index of the tie
    frac = np.unique(np.modf(want * 2048.0)[0])
    assert frac.tolist() == [0.0]                               # multiples of 2^-11: 12 bits, exact in float32


def test_accumulate_rule_rounds_twice():
    """w * s is rounded before the sum: with these numbers a fused multiply-add gives another float"""
    w, s, a = np.float32(0.5448831915855408), np.float32(0.42365479469299316), np.float32(0.6458941102027893)
    two = accumulate_f32(np.array([a]), np.array([s]), w, False)[0]
    fused = np.float32(float(a) + float(w) * float(s))          # exact product (48 bits), one rounding
    assert two == np.float32(a + np.float32(w * s)) and two != fused
    assert accumulate_f32(None, np.array([s]), w, True)[0] == np.float32(w * s)


# ---------------------------------------------------------------------------------------------------------------------
# ensemble_weights
# ---------------------------------------------------------------------------------------------------------------------
def test_ensemble_weights_equal_and_normalised():
    assert ensemble_weights(None, 4) == [0.25] * 4
    w = ensemble_weights([5, 3, 2], 3)
    assert w == [0.5, 0.3, 0.2] and all(type(v) is float for v in w)
    w = ensemble_weights((0.1, 0.2, 0.7, 1.5, 3.0), 5)
    assert abs(sum(w) - 1.0) <= 2e-16 and w == [v / (0.1 + 0.2 + 0.7 + 1.5 + 3.0) for v in (0.1, 0.2, 0.7, 1.5, 3.0)]
    assert ensemble_weights(np.array([1.0, 3.0], dtype=np.float32), 2) == [0.25, 0.75]


def test_ensemble_weights_single_member_is_exactly_one():
    assert ensemble_weights(None, 1) == [1.0]
    assert ensemble_weights([0.3], 1) == [1.0]
    assert ensemble_weights([7], 1) == [1.0]


@pytest.mark.parametrize('weights,K', [([1.0, 2.0], 3), ([1.0, 2.0, 3.0], 2), ([], 1), ([1.0, 0.0], 2), ([1.0, -2.0], 2),
                                       ([1.0, float('nan')], 2), ([float('inf'), 1.0], 2), ([1.0, 'a'], 2), ('12', 2),
                                       (3.0, 1), ([1.0, None], 2), ([True, 1.0], 2), (None, 0)])
def test_ensemble_weights_refuses(weights, K):
    with pytest.raises(ValueError):
        ensemble_weights(weights, K)


# ---------------------------------------------------------------------------------------------------------------------
# ensemble_options
# ---------------------------------------------------------------------------------------------------------------------
def _stage(**keys):
    return types.SimpleNamespace(model_name='fine', partition_type='SIZE', **keys)


def test_ensemble_options_absent_is_the_single_model():
    assert ensemble_options(_stage()) == (None, None, None)
    assert ensemble_options(_stage(ensemble=None, checkpoint='best')) == (None, None, None)
    from segmentation3d.utils.file_io import ensure_easydict
    ensure_easydict()
    from segmentation3d.config.infer_config import cfg          # the shipped config has none of the keys
    assert ensemble_options(cfg.fine) == (None, None, None) and ensemble_options(cfg.coarse) == (None, None, None)


def test_ensemble_options_reads_the_keys():
    assert ensemble_options(_stage(ensemble=['fold_0', 'fold_1'])) == (['fold_0', 'fold_1'], [0.5, 0.5], ['latest', 'latest'])
    names, weights, chk = ensemble_options(_stage(ensemble=('a', 'b', 'c'), ensemble_weights=[5, 3, 2], checkpoint='best'))
    assert names == ['a', 'b', 'c'] and weights == [0.5, 0.3, 0.2] and chk == ['best'] * 3
    assert ensemble_options(_stage(ensemble=['a', 'b'], checkpoint=['best', 4]))[2] == ['best', 4]
    assert ensemble_options(_stage(ensemble=['a']))[:2] == (['a'], [1.0])
    from segmentation3d.utils.file_io import ensure_easydict
    ensure_easydict()
    from easydict import EasyDict
    sec = EasyDict({'model_name': 'fine', 'ensemble': ['x', 'y'], 'ensemble_weights': [1, 3]})
    assert ensemble_options(sec) == (['x', 'y'], [0.25, 0.75], ['latest', 'latest'])


@pytest.mark.parametrize('keys', [dict(ensemble=[]), dict(ensemble='fold_0'), dict(ensemble=3), dict(ensemble=['a', 'a']),
                                  dict(ensemble=['a', 5]), dict(ensemble=['a', '']),
                                  dict(ensemble=['a', 'b'], checkpoint=['best']),
                                  dict(ensemble=['a', 'b'], checkpoint=['best', 'best', 'best']),
                                  dict(ensemble=['a', 'b'], ensemble_weights=[1.0]),
                                  dict(ensemble=['a', 'b'], ensemble_weights=[1.0, -1.0]),
                                  dict(checkpoint=['best', 'best']), dict(ensemble_weights=[1.0])])
def test_ensemble_options_refuses(keys):
    with pytest.raises(ValueError):
        ensemble_options(_stage(**keys))


# ---------------------------------------------------------------------------------------------------------------------
# check_ensemble_members
# ---------------------------------------------------------------------------------------------------------------------
def _member(**over):
    m = dict(in_channels=1, out_channels=3, output_activation='softmax', region_class_order=None, spacing=[1.0, 1.0, 1.0],
             max_stride=16, interpolation='LINEAR', net='vnet', crop_normalizer_dicts=[None])
    m.update(over)
    return m


def test_members_may_differ_in_geometry_network_and_normalisers():
    members = [_member(), _member(spacing=[1.5, 1.5, 2.0], max_stride=32, net='vbnet', interpolation='NN',
                                  crop_normalizer_dicts=[{'type': 1, 'clip_sigma': 3}]),
               _member(output_activation=None)]                 # a checkpoint without the key is a soft-max one
    assert check_ensemble_members(members) == members
    regions = [_member(output_activation='sigmoid', region_class_order=[2, 1, 3]),
               _member(output_activation='sigmoid', region_class_order=(2, 1, 3), spacing=[2.0, 2.0, 2.0])]
    assert len(check_ensemble_members(regions)) == 2
    assert len(check_ensemble_members([_member()])) == 1


@pytest.mark.parametrize('key,value', [('in_channels', 2), ('out_channels', 4), ('output_activation', 'sigmoid'),
                                       ('region_class_order', [1, 2, 3])])
@pytest.mark.parametrize('where', [1, 2])
def test_members_must_agree(key, value, where):
    members = [_member(), _member(), _member()]
    members[where] = _member(**{key: value})
    with pytest.raises(ValueError) as e:
        check_ensemble_members(members)
    assert key in str(e.value) and 'member {}'.format(where) in str(e.value)


def test_no_members():
    with pytest.raises(ValueError):
        check_ensemble_members([])
