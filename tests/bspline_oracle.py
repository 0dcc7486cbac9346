"""float64 numpy restatement of the cubic B-spline interpolation (include/seg3d_hip.h), and
the same algorithm with fp32 storage and fp32 arithmetic -- the "fp32 run" whose error against the float64 oracle sets the
bars of tests/test_gpu_bspline.py.  Volumes are [Z, Y, X] or [Z, Y, X, M]; sizes and coordinates are (x, y, z)."""
import numpy as np

POLE = np.sqrt(3.0) - 2.0
HORIZON = 24


def mirror(i, n):
    """whole-sample mirror of any integer index onto 0 .. n-1: -1 -> 1, n -> n - 2, period 2 (n - 1); n = 1 -> 0"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def system_matrix(n):
    """A with s = A c:  s[i] = (c[i-1] + 4 c[i] + c[i+1]) / 6, outside indices mirrored; n = 1: identity"""
    A = np.zeros((n, n))
    if n == 1:
        A[0, 0] = 1.0
        return A
    for i in range(n):
        for j, w in ((i - 1, 1.0), (i, 4.0), (i + 1, 1.0)):
            A[i, int(mirror(j, n))] += w / 6.0
    return A


def prefilter(vol):
    """samples -> coefficients, float64: the dense solve of the mirror system per axis, x then y then z"""
    c = np.asarray(vol, dtype=np.float64)
    for axis in (2, 1, 0):
        n = c.shape[axis]
        moved = np.moveaxis(c, axis, 0)
        solved = np.linalg.solve(system_matrix(n), moved.reshape(n, -1)).reshape(moved.shape)
        c = np.moveaxis(solved, 0, axis)
    return c


def prefilter_recursive(vol, dtype=np.float64):
    """the recursive form, every value and every operation in `dtype` (np.float32: the fp32 run)"""
    t = dtype
    z = t(POLE)
    last = t(z / (z * z - t(1.0)))
    c = np.array(vol, dtype=t)
    for axis in (2, 1, 0):
        n = c.shape[axis]
        if n == 1:
            continue
        s = np.moveaxis(c, axis, 0)                       # a view: writes go to c
        cp = np.empty_like(s)
        acc, zk = s[0].copy(), z
        for k in range(1, HORIZON):
            acc = (acc + zk * s[int(mirror(k, n))]).astype(t)
            zk = t(zk * z)
        cp[0] = acc
        for i in range(1, n):
            cp[i] = (s[i] + z * cp[i - 1]).astype(t)
        cm = (last * (cp[n - 1] + z * cp[n - 2])).astype(t)
        s[n - 1] = t(6.0) * cm
        for i in range(n - 2, -1, -1):
            cm = (z * (cm - cp[i])).astype(t)
            s[i] = t(6.0) * cm
    return c


def affine_coords(affine, out_size):
    """continuous source index (cx, cy, cz), each [Zo, Yo, Xo] float64, of a 3 x 4 index map written as the device
    writes it: m0 * x + m1 * y + m2 * z + m3, left to right -- bitwise the device's coordinates"""
    m = np.asarray(affine, dtype=np.float64).reshape(12)
    Xo, Yo, Zo = (int(v) for v in out_size)
    z, y, x = np.meshgrid(np.arange(Zo, dtype=np.float64), np.arange(Yo, dtype=np.float64),
                          np.arange(Xo, dtype=np.float64), indexing='ij')
    return tuple(((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] for r in range(3))


def basis(f):
    """B_0 .. B_3(f), the operation order of the header"""
    f2 = f * f
    f3 = f2 * f
    o = 1.0 - f
    six = f.dtype.type(6.0)
    return [o * o * o / six, (3.0 * f3 - 6.0 * f2 + 4.0) / six, (-3.0 * f3 + 3.0 * f2 + 3.0 * f + 1.0) / six, f3 / six]


def evaluate(coef, coords, pad, dtype=np.float64):
    """the spline of the coefficients coef [Z, Y, X] or [Z, Y, X, M] at coords = (cx, cy, cz): inside iff
    -0.5 <= c < size - 0.5 per axis, else pad; taps k-1 .. k+2 mirrored; sums x, then y, then z, each left to right, in
    `dtype` (np.float32: the fp32 run -- coefficients, weights and sums in fp32).  -> float64 array [Zo, Yo, Xo(, M)]"""
    t = dtype
    coef = np.asarray(coef, dtype=t)
    planar = coef.ndim == 3
    if planar:
        coef = coef[..., None]
    Zi, Yi, Xi, M = coef.shape
    size = (Xi, Yi, Zi)
    inside = np.ones(coords[0].shape, dtype=bool)
    idx, w = [], []
    for r in range(3):
        c = np.asarray(coords[r], dtype=np.float64)
        inside &= (c >= -0.5) & (c < size[r] - 0.5)
        k = np.floor(c)
        w.append(basis((c - k).astype(t)))
        idx.append([mirror(k.astype(np.int64) - 1 + j, size[r]) for j in range(4)])
    out = None
    for jz in range(4):
        b = None
        for jy in range(4):
            a = None
            for jx in range(4):
                term = w[0][jx][..., None] * coef[idx[2][jz], idx[1][jy], idx[0][jx]]
                a = term if a is None else a + term
            term = w[1][jy][..., None] * a
            b = term if b is None else b + term
        term = w[2][jz][..., None] * b
        out = term if out is None else out + term
    assert out.dtype == t
    out = np.where(inside[..., None], out.astype(np.float32).astype(np.float64), np.float64(np.float32(pad)))
    return out[..., 0] if planar else out
