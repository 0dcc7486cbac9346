"""numpy restatement of the 'LABEL_LINEAR' label interpolation (definition in
include/seg3d_hip.h), affine index maps only.  Everything is float64 in the operation order of the device functions
(affine12_apply, SEG3D_INSIDE_BUFFER, trilinear_tap, trilinear_lerp of csrc/seg3d_imagegrid.h, compiled without
contraction): per label one membership plane, rounded to float32 as trilinear_lerp rounds it, the labels in ascending
order, and the FIRST maximum over the planes.  Pinned on the CPU by tests/test_label_interp.py.

Volumes are numpy [Z, Y, X]; `affine` is the 3 x 4 matrix with c = affine @ (x, y, z, 1); out_size = (Xo, Yo, Zo)."""
import numpy as np


def coordinates(affine, out_size):
    """(cx, cy, cz), float64 [Zo, Yo, Xo]: each row summed left to right as affine12_apply does"""
    A = np.asarray(affine, dtype=np.float64).reshape(3, 4)
    Xo, Yo, Zo = (int(v) for v in out_size)
    z, y, x = np.meshgrid(np.arange(Zo, dtype=np.float64), np.arange(Yo, dtype=np.float64),
                          np.arange(Xo, dtype=np.float64), indexing='ij')
    return tuple(A[r, 0] * x + A[r, 1] * y + A[r, 2] * z + A[r, 3] for r in range(3))


def inside(c, shape):
    """ITK's IsInsideBuffer: -0.5 <= c < size - 0.5 per axis; shape = (Z, Y, X)"""
    cx, cy, cz = c
    Z, Y, X = shape
    return ((cx >= -0.5) & (cx < X - 0.5) & (cy >= -0.5) & (cy < Y - 0.5) & (cz >= -0.5) & (cz < Z - 0.5))


def _tap(c, n):
    f = np.minimum(np.maximum(c, 0.0), float(n - 1))
    i0 = np.floor(f).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), f - i0


def lerp(volume, c):
    """trilinear_tap + trilinear_lerp of a float64 volume at the coordinates c (clamped taps; x, then y, then z), rounded
    to float32 once"""
    v = np.asarray(volume, dtype=np.float64)
    Z, Y, X = v.shape
    x0, x1, dx = _tap(c[0], X)
    y0, y1, dy = _tap(c[1], Y)
    z0, z1, dz = _tap(c[2], Z)
    v000, v100, v010, v110 = v[z0, y0, x0], v[z0, y0, x1], v[z0, y1, x0], v[z0, y1, x1]
    v001, v101, v011, v111 = v[z1, y0, x0], v[z1, y0, x1], v[z1, y1, x0], v[z1, y1, x1]
    a00, a01 = v000 + (v100 - v000) * dx, v010 + (v110 - v010) * dx
    a10, a11 = v001 + (v101 - v001) * dx, v011 + (v111 - v011) * dx
    b0, b1 = a00 + (a01 - a00) * dy, a10 + (a11 - a10) * dy
    return (b0 + (b1 - b0) * dz).astype(np.float32)


def label_list(volume, pad):
    """the values of the volume in ascending order, with `pad` in its sorted place"""
    return np.unique(np.concatenate([np.asarray(volume, dtype=np.float32).ravel(), np.array([pad], dtype=np.float32)]))


def memberships(volume, affine, out_size, pad=0.0):
    """(labels ascending [L] float32, planes [L, Zo, Yo, Xo] float32): plane l is the 'LINEAR' resampling of the indicator
    (volume == l) with the padding value 1 for l == pad and 0 otherwise"""
    vol = np.asarray(volume, dtype=np.float32)
    c = coordinates(affine, out_size)
    ins = inside(c, vol.shape)
    labels = label_list(vol, pad)
    planes = [np.where(ins, lerp((vol == l).astype(np.float64), c), np.float32(1.0 if l == np.float32(pad) else 0.0))
              for l in labels]
    return labels, np.stack(planes).astype(np.float32)


def label_linear(volume, affine, out_size, pad=0.0):
    """the 'LABEL_LINEAR' resampling, float32 [Zo, Yo, Xo]: the label of the first maximum over the membership planes"""
    labels, planes = memberships(volume, affine, out_size, pad)
    return labels[np.argmax(planes, axis=0)]          # np.argmax: the first occurrence of the maximum


def nearest(volume, affine, out_size, pad=0.0):
    """the 'NN' resampling, for contrast: round half up, clamped, `pad` outside"""
    vol = np.asarray(volume, dtype=np.float32)
    Z, Y, X = vol.shape
    c = coordinates(affine, out_size)
    xn = np.clip(np.floor(c[0] + 0.5).astype(np.int64), 0, X - 1)
    yn = np.clip(np.floor(c[1] + 0.5).astype(np.int64), 0, Y - 1)
    zn = np.clip(np.floor(c[2] + 0.5).astype(np.int64), 0, Z - 1)
    return np.where(inside(c, vol.shape), vol[zn, yn, xn], np.float32(pad)).astype(np.float32)
