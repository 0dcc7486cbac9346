"""Host side of the on-device training augmentation: the float64 numpy oracle of the rotation,
the cubic B-spline deformation, the intensity transforms and the Philox noise, pinned here on the CPU; the index-map
composition, the RNG order of `SegmentationDataset.sample_augmentation` and the option checks.  Nothing of this is in the
reference, so the definitions are restated from the contract.  The oracle helpers are shared with
tests/test_gpu_augment.py."""
import os

import numpy as np
import pytest
import torch

from test_blend_tta import _toy_case, _parent_geometry_draws


# ---------------------------------------------------------------------------------------------------------------------
# numpy oracle, written from the definitions
# ---------------------------------------------------------------------------------------------------------------------
def oracle_philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of uint32 values, key: 2 -> the 4 output words as uint64 arrays holding uint32 values"""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(0xffffffff) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k = [int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff]
    mask = np.uint64(0xffffffff)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & mask]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    return c


def oracle_normal(seed, shape_zyx, m):
    """float64 [Z, Y, X] standard normals of modality m: counter (v_lo, v_hi, m, 0), v the linear voxel index"""
    Z, Y, X = shape_zyx
    v = np.arange(Z * Y * X, dtype=np.uint64).reshape(Z, Y, X)
    r = oracle_philox4x32_10((v & np.uint64(0xffffffff), v >> np.uint64(32), m, 0), (seed & 0xffffffff, seed >> 32))
    u1 = (r[0].astype(np.float64) + 1.0) * 2.0 ** -32
    u2 = r[1].astype(np.float64) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def oracle_basis(f):
    f = np.asarray(f, dtype=np.float64)
    return np.stack([(1 - f) ** 3 / 6, (3 * f ** 3 - 6 * f ** 2 + 4) / 6, (-3 * f ** 3 + 3 * f ** 2 + 3 * f + 1) / 6, f ** 3 / 6])


def oracle_control_dims(size_xyz, spacing, h):
    return tuple(int(np.floor((int(size_xyz[a]) - 1) * (float(spacing[a]) / float(h)))) + 4 for a in range(3))


def _axis_weights(n, t):
    """k [n] and weights [4, n] of one axis"""
    tt = np.arange(n, dtype=np.float64) * t
    k = np.floor(tt)
    return k.astype(np.int64), oracle_basis(tt - k)


def oracle_field(ctrl, size_xyz, t_xyz, mirror=(False, False, False)):
    """u [Zo, Yo, Xo, 3] float64 (mm): the tensor-product cubic B-spline of ctrl [gz, gy, gx, 3]; with `mirror` the field
    is evaluated at the mirrored index n - 1 - i of the flagged axes"""
    ctrl = np.asarray(ctrl, dtype=np.float64)
    Xo, Yo, Zo = (int(v) for v in size_xyz)
    kx, wx = _axis_weights(Xo, t_xyz[0])
    ky, wy = _axis_weights(Yo, t_xyz[1])
    kz, wz = _axis_weights(Zo, t_xyz[2])
    u = np.zeros((Zo, Yo, Xo, 3))
    for jz in range(4):
        for jy in range(4):
            for jx in range(4):
                w = wz[jz][:, None, None] * wy[jy][None, :, None] * wx[jx][None, None, :]
                u += w[..., None] * ctrl[(kz + jz)[:, None, None], (ky + jy)[None, :, None], (kx + jx)[None, None, :]]
    for a, ax in ((0, 2), (1, 1), (2, 0)):
        if mirror[a]:
            u = np.flip(u, ax)
    return u


def oracle_field_nested(ctrl, size_xyz, t_xyz):
    """the same field as three nested 1-D spline evaluations (x, then y, then z)"""
    ctrl = np.asarray(ctrl, dtype=np.float64)

    def along(a, axis, n, t):
        k, w = _axis_weights(n, t)
        out = 0
        for j in range(4):
            shape = [1] * a.ndim
            shape[axis] = n
            out = out + w[j].reshape(shape) * np.take(a, k + j, axis=axis)
        return out
    Xo, Yo, Zo = (int(v) for v in size_xyz)
    return along(along(along(ctrl, 2, Xo, t_xyz[0]), 1, Yo, t_xyz[1]), 0, Zo, t_xyz[2])


def oracle_rotation(angles):
    gx, gy, gz = angles
    Rx = np.array([[1, 0, 0], [0, np.cos(gx), -np.sin(gx)], [0, np.sin(gx), np.cos(gx)]])
    Ry = np.array([[np.cos(gy), 0, np.sin(gy)], [0, 1, 0], [-np.sin(gy), 0, np.cos(gy)]])
    Rz = np.array([[np.cos(gz), -np.sin(gz), 0], [np.sin(gz), np.cos(gz), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def oracle_coords(src_frame, dst_frame, size_xyz, rotation=None, ctrl=None, grid_mm=None, mirror=(False, False, False)):
    """continuous source index [3, Zo, Yo, Xo] (rows x, y, z) of every destination voxel, point by point: index (mirrored)
    -> physical point -> rotated about the grid centre -> displaced by the field -> source index"""
    s_sp, s_or, s_dir = (np.asarray(v, dtype=np.float64) for v in src_frame)
    d_sp, d_or, d_dir = (np.asarray(v, dtype=np.float64) for v in dst_frame)
    Xo, Yo, Zo = (int(v) for v in size_xyz)
    n = np.array([Xo, Yo, Zo], dtype=np.float64)
    z, y, x = np.meshgrid(np.arange(Zo), np.arange(Yo), np.arange(Xo), indexing='ij')
    idx = np.stack([x, y, z]).astype(np.float64)
    for a in range(3):
        if mirror[a]:
            idx[a] = n[a] - 1 - idx[a]
    A = d_dir.reshape(3, 3) @ np.diag(d_sp)
    p = d_or[:, None, None, None] + np.einsum('ij,jzyx->izyx', A, idx)
    if rotation is not None:
        c = d_or + A @ ((n - 1) / 2)
        p = c[:, None, None, None] + np.einsum('ij,jzyx->izyx', oracle_rotation(rotation), p - c[:, None, None, None])
    if ctrl is not None:
        u = oracle_field(ctrl, size_xyz, [sp / float(grid_mm) for sp in d_sp], mirror)
        p = p + np.moveaxis(u, 3, 0)
    to_src = np.diag(1.0 / s_sp) @ np.linalg.inv(s_dir.reshape(3, 3))
    return np.einsum('ij,jzyx->izyx', to_src, p - s_or[:, None, None, None])


def oracle_sample(src, c, linear=True, pad=0.0):
    """src [Z, Y, X] sampled at the continuous indices c [3, ...] (x, y, z) with the resampling semantics of the affine
    entries: inside iff -0.5 <= c < size - 0.5, clamped trilinear neighbourhood / nearest neighbour rounding half up"""
    src = np.asarray(src, dtype=np.float64)
    Zi, Yi, Xi = src.shape
    size = (Xi, Yi, Zi)
    inside = np.ones(c[0].shape, dtype=bool)
    for r in range(3):
        inside &= (c[r] >= -0.5) & (c[r] < size[r] - 0.5)
    if linear:
        f = [np.clip(c[r], 0.0, size[r] - 1) for r in range(3)]
        i0 = [np.floor(v).astype(np.int64) for v in f]
        i1 = [np.minimum(i0[r] + 1, size[r] - 1) for r in range(3)]
        d = [f[r] - i0[r] for r in range(3)]
        g = lambda zz, yy, xx: src[zz, yy, xx]
        a00 = g(i0[2], i0[1], i0[0]) + (g(i0[2], i0[1], i1[0]) - g(i0[2], i0[1], i0[0])) * d[0]
        a01 = g(i0[2], i1[1], i0[0]) + (g(i0[2], i1[1], i1[0]) - g(i0[2], i1[1], i0[0])) * d[0]
        a10 = g(i1[2], i0[1], i0[0]) + (g(i1[2], i0[1], i1[0]) - g(i1[2], i0[1], i0[0])) * d[0]
        a11 = g(i1[2], i1[1], i0[0]) + (g(i1[2], i1[1], i1[0]) - g(i1[2], i1[1], i0[0])) * d[0]
        b0 = a00 + (a01 - a00) * d[1]
        b1 = a10 + (a11 - a10) * d[1]
        val = b0 + (b1 - b0) * d[2]
    else:
        n = [np.clip(np.floor(c[r] + 0.5).astype(np.int64), 0, size[r] - 1) for r in range(3)]
        val = src[n[2], n[1], n[0]]
    return np.where(inside, val, pad).astype(np.float32)


def oracle_tie_distance(c):
    """per voxel: distance (source voxels) of the sample point to the nearest half-voxel tie of nearest-neighbour rounding
    (which is also where the inside test switches)"""
    d = np.full(c[0].shape, 1.0)
    for r in range(3):
        d = np.minimum(d, np.abs((c[r] - np.floor(c[r])) - 0.5))
    return d


NEUTRAL = {'brightness': 1.0, 'contrast': 1.0, 'gamma': 1.0, 'invert': False, 'sigma': 0.0}


def oracle_intensity(crop, params, seed=0):
    """crop [Z, Y, X, M] -> float64 result of brightness, contrast, gamma, noise per modality, in that order"""
    x = np.array(crop, dtype=np.float64)
    Z, Y, X, M = x.shape
    for m in range(M):
        p = dict(NEUTRAL)
        p.update(params[m] or {})
        y = x[..., m]
        mn, mx, mean = y.min(), y.max(), y.mean()
        if p['brightness'] != 1.0:
            y, mn, mx, mean = y * p['brightness'], mn * p['brightness'], mx * p['brightness'], mean * p['brightness']
        lo, hi = mn, mx
        if p['contrast'] != 1.0:
            y = np.clip(mean + p['contrast'] * (y - mean), mn, mx)
            lo = np.clip(mean + p['contrast'] * (mn - mean), mn, mx)
            hi = np.clip(mean + p['contrast'] * (mx - mean), mn, mx)
        if p['gamma'] != 1.0 and hi - lo >= 1e-7:
            r = (y - lo) / (hi - lo)
            if p['invert']:
                r = 1.0 - r
            r = np.clip(r, 0.0, 1.0) ** p['gamma']
            if p['invert']:
                r = 1.0 - r
            y = lo + r * (hi - lo)
        if p['sigma'] != 0.0:
            y = y + p['sigma'] * oracle_normal(seed, (Z, Y, X), m)
        x[..., m] = y
    return x


# ---------------------------------------------------------------------------------------------------------------------
# Philox
# ---------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """the Random123 known-answer vectors of philox4x32-10"""
    F = 0xffffffff
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((F, F, F, F), (F, F), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        got = tuple(int(v) for v in oracle_philox4x32_10(ctr, key))
        assert got == want, [hex(v) for v in got]
    # vectorised over counters = the scalar calls
    r = oracle_philox4x32_10((np.arange(5), 0, 2, 0), (7, 9))
    for i in range(5):
        assert tuple(int(v[i]) for v in r) == tuple(int(v) for v in oracle_philox4x32_10((i, 0, 2, 0), (7, 9)))


def test_oracle_normals_are_standard_and_depend_on_voxel_and_modality_only():
    n0 = oracle_normal(12345, (24, 24, 24), 0)
    n1 = oracle_normal(12345, (24, 24, 24), 1)
    se = 1.0 / np.sqrt(n0.size)
    assert abs(n0.mean()) < 5 * se and abs(n0.var() - 1.0) < 5 * np.sqrt(2.0) * se
    assert abs(np.corrcoef(n0.ravel(), n1.ravel())[0, 1]) < 5 * se
    assert np.array_equal(oracle_normal(12345, (12, 24, 24), 0), n0[:12])          # a function of the linear index
    assert not np.array_equal(oracle_normal(12346, (24, 24, 24), 0), n0)


# ---------------------------------------------------------------------------------------------------------------------
# B-spline field
# ---------------------------------------------------------------------------------------------------------------------
_SIZE, _SP, _H = (20, 17, 12), (0.9, 1.1, 1.7), 6.0


def _t():
    return [sp / _H for sp in _SP]


def test_bspline_partition_of_unity_and_linear_reproduction():
    from segmentation3d.utils.image_tools import bspline_control_dims
    g = oracle_control_dims(_SIZE, _SP, _H)
    assert bspline_control_dims(_SIZE, _SP, _H) == g
    assert g == tuple(int(np.floor((_SIZE[a] - 1) * _SP[a] / _H)) + 4 for a in range(3))
    const = np.empty((g[2], g[1], g[0], 3))
    const[...] = [1.5, -2.0, 0.25]
    u = oracle_field(const, _SIZE, _t())
    assert np.abs(u - np.array([1.5, -2.0, 0.25])).max() < 1e-13
    # control values linear in the grid index -> a field linear in the voxel index: sum_j B_j(f) (k + j) = t + 1
    gz, gy, gx = np.meshgrid(np.arange(g[2]), np.arange(g[1]), np.arange(g[0]), indexing='ij')
    lin = np.stack([2.0 * gx - gy, 0.5 * gy + gz, gz - 3.0 * gx + 1.0], -1).astype(np.float64)
    u = oracle_field(lin, _SIZE, _t())
    z, y, x = np.meshgrid(np.arange(_SIZE[2]), np.arange(_SIZE[1]), np.arange(_SIZE[0]), indexing='ij')
    tx, ty, tz = (v * t + 1.0 for v, t in zip((x, y, z), _t()))
    want = np.stack([2.0 * tx - ty, 0.5 * ty + tz, tz - 3.0 * tx + 1.0], -1)
    assert np.abs(u - want).max() < 1e-12


def test_bspline_tensor_product_equals_nested_evaluations_and_mirror_is_a_flip():
    g = oracle_control_dims(_SIZE, _SP, _H)
    ctrl = np.random.RandomState(4).uniform(-1, 1, size=(g[2], g[1], g[0], 3)).astype(np.float32)
    u = oracle_field(ctrl, _SIZE, _t())
    assert np.abs(u - oracle_field_nested(ctrl, _SIZE, _t())).max() < 1e-13
    um = oracle_field(ctrl, _SIZE, _t(), mirror=(True, False, True))
    assert np.array_equal(um, u[::-1, :, ::-1])


def test_folding_bound_keeps_the_jacobian_norm_below_one():
    """control displacements in [-a, a] with a just under h / 6: the Frobenius norm of the finite-difference Jacobian of u
    (per millimetre) stays below 1 everywhere, so id + u does not fold"""
    h, sp, size = 8.0, (0.5, 0.5, 0.5), (48, 48, 48)
    a = h / 6.0 * 0.999
    g = oracle_control_dims(size, sp, h)
    worst = 0.0
    for seed in range(4):
        rng = np.random.RandomState(seed)
        ctrl = rng.uniform(-a, a, size=(g[2], g[1], g[0], 3))
        if seed == 3:
            ctrl = np.where(rng.rand(*ctrl.shape) < 0.5, -a, a)             # the extreme corners of the box
        u = oracle_field(ctrl, size, [s / h for s in sp])
        J = np.stack([np.diff(u, axis=2)[:-1, :-1] / sp[0], np.diff(u, axis=1)[:-1, :, :-1] / sp[1],
                      np.diff(u, axis=0)[:, :-1, :-1] / sp[2]], -1)        # [.., component, direction]
        worst = max(worst, float(np.sqrt((J ** 2).sum((-1, -2))).max()))
        assert np.abs(J).max() <= 2 * a / h + 1e-12
    assert worst < 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------
# rotation of the index map
# ---------------------------------------------------------------------------------------------------------------------
_SRC = ((0.8, 1.1, 2.0), (1.0, 2.0, 3.0), oracle_rotation((0.1, -0.2, 0.3)).ravel())
_DST = ((0.9, 0.6, 0.8), (-9.0, 3.5, 0.5), oracle_rotation((-0.05, 0.15, 0.2)).ravel())


def test_rotate_index_affine_zero_angles_is_the_input_bit_for_bit():
    from segmentation3d.utils.image_tools import index_affine, rotate_index_affine
    M = index_affine(_SRC, _DST)
    keep = M.copy()
    R = rotate_index_affine(M, _SRC, _DST, (11, 13, 17), (0.0, 0.0, 0.0))
    assert R is not M and np.array_equal(R.view(np.uint64), keep.view(np.uint64)) and np.array_equal(M, keep)


def test_rotate_index_affine_quarter_turn_about_z():
    from segmentation3d.utils.image_tools import index_affine, rotate_index_affine
    src = ((0.7, 0.7, 0.7), (1.0, 2.0, 3.0), np.eye(3).ravel())
    dst = ((1.0, 1.0, 1.0), (-3.0, 0.5, 2.0), np.eye(3).ravel())
    n = 12
    M = index_affine(src, dst)
    R = rotate_index_affine(M, src, dst, (n, n, n), (0.0, 0.0, np.pi / 2))
    for idx in ((0, 0, 0), (11, 0, 3), (4, 9, 11), (11, 11, 11)):
        turned = (n - 1 - idx[1], idx[0], idx[2])              # c + Rz(90) (i - c): (dx, dy) -> (-dy, dx)
        assert np.abs(R @ np.array(list(idx) + [1.0]) - M @ np.array(list(turned) + [1.0])).max() < 1e-12
    # the array identity the GPU test uses: rot[z, y, x] = plain[z, x, n - 1 - y] is torch.rot90 by one turn in (y, x)
    a = torch.arange(2 * n * n).reshape(2, n, n)
    want = a.transpose(1, 2).flip(1)
    assert all(int(want[z, y, x]) == int(a[z, x, n - 1 - y]) for z, y, x in ((0, 0, 0), (1, 3, 7), (1, 11, 2)))
    assert torch.equal(want, torch.rot90(a, 1, (1, 2)))


def test_rotation_composed_with_mirror_matches_the_point_formula():
    from segmentation3d.utils.image_tools import index_affine, rotate_index_affine, mirror_index_affine
    size = (11, 13, 17)
    angles = (0.3, -0.2, 0.5)
    M = index_affine(_SRC, _DST)
    for mirror in ((False, False, False), (True, False, True), (True, True, True)):
        Mm = mirror_index_affine(rotate_index_affine(M, _SRC, _DST, size, angles), size, mirror)
        c = oracle_coords(_SRC, _DST, size, rotation=angles, mirror=mirror)
        z, y, x = np.meshgrid(np.arange(size[2]), np.arange(size[1]), np.arange(size[0]), indexing='ij')
        got = np.stack([Mm[r, 0] * x + Mm[r, 1] * y + Mm[r, 2] * z + Mm[r, 3] for r in range(3)])
        assert np.abs(got - c).max() < 1e-11


def test_oracle_sampler_is_the_repository_resampling_oracle_and_scipy_trilinear():
    """the coordinate-based sampler equals oracle/numpy_ref.resample_affine on an affine map, and its trilinear part equals
    scipy.ndimage.map_coordinates(order=1) on interior points"""
    from oracle import numpy_ref
    from scipy import ndimage
    rng = np.random.RandomState(2)
    src = rng.randn(14, 15, 16)
    size = (11, 13, 9)
    dst = ((0.9, 0.6, 0.8), (2.0, 3.5, 4.5), _SRC[2])
    M = numpy_ref.index_affine(_SRC, dst)
    c = oracle_coords(_SRC, dst, size)
    for linear in (True, False):
        assert np.array_equal(oracle_sample(src, c, linear, -7.0), numpy_ref.resample_affine(src, M, size, linear, -7.0))
    g = oracle_control_dims(size, dst[0], 5.0)
    ctrl = rng.uniform(-0.8, 0.8, size=(g[2], g[1], g[0], 3))
    c = oracle_coords(_SRC, dst, size, rotation=(0.1, 0.2, -0.1), ctrl=ctrl, grid_mm=5.0)
    interior = np.ones(c[0].shape, bool)
    for r, n in enumerate((16, 15, 14)):
        interior &= (c[r] > 0) & (c[r] < n - 1)
    assert interior.mean() > 0.2
    sp = ndimage.map_coordinates(src, [c[2][interior], c[1][interior], c[0][interior]], order=1)
    assert np.abs(oracle_sample(src, c, True)[interior] - sp).max() < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# intensity oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_intensity_oracle_properties():
    rng = np.random.RandomState(1)
    x = np.clip(rng.randn(6, 7, 9, 2), -1, 1)
    assert np.array_equal(oracle_intensity(x, [None, {}]), x)
    b = oracle_intensity(x, [{'brightness': 1.2}, None])
    assert np.allclose(b[..., 0], 1.2 * x[..., 0]) and np.array_equal(b[..., 1], x[..., 1])
    c = oracle_intensity(x, [{'contrast': 1.4}, {'contrast': 0.6}])
    for m in range(2):
        assert c[..., m].min() >= x[..., m].min() and c[..., m].max() <= x[..., m].max()       # range preserved
    g = oracle_intensity(x, [{'gamma': 0.7}, {'gamma': 1.5, 'invert': True}])
    for m in range(2):
        assert abs(g[..., m].min() - x[..., m].min()) < 1e-12 and abs(g[..., m].max() - x[..., m].max()) < 1e-12
        assert np.array_equal(np.argsort(g[..., m].ravel(), kind='stable'), np.argsort(x[..., m].ravel(), kind='stable'))
    const = np.full((3, 4, 5, 1), 0.25)
    assert np.array_equal(oracle_intensity(const, [{'gamma': 0.5, 'invert': True}]), const)    # hi == lo: unchanged
    n = oracle_intensity(np.zeros((6, 7, 9, 2)), [{'sigma': 1.0}, {'sigma': 2.0}], seed=99)
    assert np.array_equal(n[..., 0], oracle_normal(99, (6, 7, 9), 0)) and np.array_equal(n[..., 1], 2.0 * oracle_normal(99, (6, 7, 9), 1))


def test_intensity_params_struct_and_checks():
    from segmentation3d import _engine as E
    from segmentation3d.utils.image_tools import intensity_params
    p = intensity_params([{'brightness': 1.25, 'sigma': 0.5}, None], 2, seed=(7 << 32) | 5)
    assert isinstance(p, E.IntensityParams) and (p.seed_lo, p.seed_hi) == (5, 7)
    assert (p.m[0].brightness, p.m[0].contrast, p.m[0].gamma, p.m[0].invert, p.m[0].sigma) == (1.25, 1.0, 1.0, 0, 0.5)
    for m in range(1, 8):
        assert (p.m[m].brightness, p.m[m].contrast, p.m[m].gamma, p.m[m].invert, p.m[m].sigma) == (1.0, 1.0, 1.0, 0, 0.0)
    for bad in ([{'brightness': 0.0}], [{'contrast': -1.0}], [{'gamma': float('nan')}], [{'sigma': -0.1}], [{'blur': 1.0}],
                [None, None]):
        with pytest.raises(ValueError):
            intensity_params(bad, 1)
    with pytest.raises(ValueError):
        intensity_params([None], 1, seed=-1)


# ---------------------------------------------------------------------------------------------------------------------
# configuration and RNG order
# ---------------------------------------------------------------------------------------------------------------------
ALL_ON = {'rotation_deg': [10, 20, 30], 'rotation_prob': 0.8, 'elastic_grid_mm': 8.0, 'elastic_magnitude_mm': [0.2, 1.2],
          'elastic_prob': 0.7, 'brightness': [0.75, 1.25], 'brightness_prob': 0.6, 'contrast': [0.75, 1.25],
          'contrast_prob': 0.6, 'gamma': [0.7, 1.5], 'gamma_prob': 0.6, 'gamma_invert_prob': 0.4, 'noise_sigma': [0.0, 0.1],
          'noise_prob': 0.6}
ALL_OFF_BY_PROB = dict(ALL_ON, rotation_prob=0.0, elastic_prob=0.0, brightness_prob=0.0, contrast_prob=0.0, gamma_prob=0.0,
                       noise_prob=0.0)


def _dataset(tmp_path, method='GLOBAL', **kw):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    from segmentation3d.utils.normalizer import AdaptiveNormalizer
    lst = _toy_case(tmp_path)
    args = (lst, 3, [1.0, 1.0, 1.0], [16, 16, 16], method, [3, 3, 3], [0.9, 1.1], 'LINEAR', [AdaptiveNormalizer()])
    return SegmentationDataset(*args, device=torch.device('cpu'), **kw)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize('method', ['CENTER', 'GLOBAL', 'MASK', 'HYBRID'])
def test_rng_stream_without_augmentation_is_the_parents(tmp_path, method):
    from segmentation3d.utils.file_io import ensure_easydict
    ensure_easydict()
    from easydict import EasyDict as edict
    np.random.seed(5)
    ref = _dataset(tmp_path, method)
    for _ in range(3):
        _parent_geometry_draws(ref, 0, method)
    want = np.random.get_state()
    for aug in (None, {}, edict(ALL_OFF_BY_PROB), {'rotation_deg': [0, 0, 0], 'rotation_prob': 1.0, 'noise_prob': 1.0}):
        ds = _dataset(tmp_path, method, augmentation=aug)
        assert ds.augmentation is None
        np.random.seed(5)
        for _ in range(3):
            _, sp = ds.sample_crop_geometry(0)
            assert ds.sample_mirror() == (False, False, False)
            assert ds.sample_augmentation(sp) is None
        assert _same_state(np.random.get_state(), want)


def test_rng_order_with_everything_on(tmp_path):
    """the documented order, restated draw by draw"""
    ds = _dataset(tmp_path, augmentation=ALL_ON, random_mirror_axes=('x',))
    a = ALL_ON
    seen = {'rotation': 0, 'control': 0, 'intensity': 0, 'invert': 0}
    for seed in range(12):
        np.random.seed(seed)
        _, sp = ds.sample_crop_geometry(0)
        ds.sample_mirror()
        got = ds.sample_augmentation(sp)
        state = np.random.get_state()
        np.random.seed(seed)
        _parent_geometry_draws(ds, 0, 'GLOBAL')
        np.random.randint(0, 2, size=1)
        rot = ctrl = None
        if np.random.uniform() < a['rotation_prob']:
            lim = np.array(a['rotation_deg'], dtype=np.double)
            rot = np.deg2rad(np.random.uniform(-lim, lim, size=[3]))
        if np.random.uniform() < a['elastic_prob']:
            mag = np.random.uniform(*a['elastic_magnitude_mm'])
            g = oracle_control_dims(ds.crop_size, sp, a['elastic_grid_mm'])
            ctrl = np.random.uniform(-mag, mag, size=(g[2], g[1], g[0], 3)).astype(np.float32)
        p = {}
        if np.random.uniform() < a['brightness_prob']:
            p['brightness'] = np.random.uniform(*a['brightness'])
        if np.random.uniform() < a['contrast_prob']:
            p['contrast'] = np.random.uniform(*a['contrast'])
        if np.random.uniform() < a['gamma_prob']:
            p['gamma'] = np.random.uniform(*a['gamma'])
            p['invert'] = bool(np.random.uniform() < a['gamma_invert_prob'])
        if np.random.uniform() < a['noise_prob']:
            p['sigma'] = np.random.uniform(*a['noise_sigma'])
        noise_seed = int(np.random.randint(0, 2 ** 63, dtype=np.int64))
        assert _same_state(state, np.random.get_state()), seed
        assert (got['rotation'] is None) == (rot is None) and (rot is None or np.allclose(got['rotation'], rot, rtol=0, atol=0))
        assert (got['control'] is None) == (ctrl is None)
        if ctrl is not None:
            assert got['control'].dtype == np.float32 and np.array_equal(got['control'], ctrl)
            assert np.abs(ctrl).max() <= a['elastic_magnitude_mm'][1]
        assert got['seed'] == noise_seed and 0 <= got['seed'] < 2 ** 63
        assert (got['intensity'] is None) == (not p) and (not p or got['intensity'] == [p])
        seen['rotation'] += rot is not None
        seen['control'] += ctrl is not None
        seen['intensity'] += bool(p)
        seen['invert'] += bool(p.get('invert'))
    assert all(v > 0 for v in seen.values()), seen


def test_each_modality_draws_independently_and_disabled_transforms_draw_nothing(tmp_path):
    from segmentation3d.dataloader.dataset import SegmentationDataset
    ds = _dataset(tmp_path, augmentation={'brightness': [0.5, 2.0], 'brightness_prob': 1.0})
    ds._num_modality = 3                                      # the draws depend on the modality count alone
    np.random.seed(3)
    got = ds.sample_augmentation([1.0, 1.0, 1.0])
    state = np.random.get_state()
    np.random.seed(3)
    want = []
    for _ in range(3):
        assert np.random.uniform() < 1.0
        want.append({'brightness': np.random.uniform(0.5, 2.0)})
    assert _same_state(state, np.random.get_state())
    assert got == {'rotation': None, 'control': None, 'intensity': want, 'seed': 0}
    assert len({p['brightness'] for p in want}) == 3


def test_shipped_train_config_has_the_section_with_everything_off():
    import segmentation3d
    from segmentation3d.dataloader.dataset import AUGMENTATION_DEFAULTS, validate_augmentation
    from segmentation3d.utils.file_io import load_config
    tc = load_config(os.path.join(os.path.dirname(segmentation3d.__file__), 'config', 'train_config.py'))
    section = tc.dataset.augmentation
    assert set(section.keys()) == set(AUGMENTATION_DEFAULTS)
    for key, value in AUGMENTATION_DEFAULTS.items():
        assert section[key] == value, key
    assert validate_augmentation(section) is None
    full = validate_augmentation(ALL_ON)
    assert all(full['enabled'].values()) and full['elastic_grid_mm'] == 8.0


@pytest.mark.parametrize('bad', [
    {'rotate': [1, 2, 3]},                                     # unknown key
    {'rotation_deg': [10, 10]}, {'rotation_deg': [-5, 0, 0]}, {'rotation_deg': [0, 0, 200]}, {'rotation_deg': 'x'},
    {'rotation_prob': 1.5}, {'elastic_prob': -0.1}, {'noise_prob': 'often'}, {'gamma_invert_prob': 2},
    {'elastic_grid_mm': 0.0}, {'elastic_grid_mm': -4.0},
    {'elastic_grid_mm': 12.0, 'elastic_magnitude_mm': [0.0, 2.0]},          # folding bound: 2.0 is not < 12 / 6
    {'elastic_grid_mm': 12.0, 'elastic_magnitude_mm': [0.0, 2.5], 'elastic_prob': 0.0},
    {'elastic_magnitude_mm': [2.0, 1.0]}, {'elastic_magnitude_mm': [-1.0, 1.0]}, {'elastic_magnitude_mm': 3.0},
    {'brightness': [0.0, 1.0]}, {'brightness': [1.2, 0.8]}, {'contrast': [-0.5, 1.0]}, {'gamma': [0.0, 2.0]},
    {'gamma': [0.5, float('inf')]}, {'noise_sigma': [-0.1, 0.1]}, {'noise_sigma': [0.2, 0.1]},
])
def test_invalid_options_raise(tmp_path, bad):
    from segmentation3d.dataloader.dataset import validate_augmentation
    with pytest.raises(ValueError):
        validate_augmentation(bad)
    with pytest.raises(ValueError):
        _dataset(tmp_path, augmentation=bad)


def test_folding_bound_is_strict_and_named(tmp_path):
    from segmentation3d.dataloader.dataset import validate_augmentation
    ok = validate_augmentation({'elastic_grid_mm': 12.0, 'elastic_magnitude_mm': [0.0, 1.99], 'elastic_prob': 1.0})
    assert ok['enabled']['elastic']
    with pytest.raises(ValueError, match='elastic_grid_mm / 6'):
        validate_augmentation({'elastic_grid_mm': 12.0, 'elastic_magnitude_mm': [0.0, 2.0], 'elastic_prob': 1.0})
    with pytest.raises(ValueError, match='dict'):
        validate_augmentation([1, 2])
    # a control grid finer than the crop's voxels is refused by the data set (the kernel's factor sp / h must be <= 1)
    with pytest.raises(ValueError, match='coarsest'):
        _dataset(tmp_path, augmentation={'elastic_grid_mm': 1.0, 'elastic_magnitude_mm': [0.0, 0.1], 'elastic_prob': 1.0})
