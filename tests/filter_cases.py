"""The case tables, the inputs and the references of the two stencil transforms of csrc/augment_filter.hip: seg3d_augment_blur
(augment_blur_kernel<MC, VEC>) and seg3d_augment_lowres (augment_lowres_kernel<KC, VEC>).  Shared by tests/test_filter_cases.py (host
only: every case reaches the launch, radius set, tile count and patch extent it is named for; the references agree with the oracles of
tests/test_resolution_augment.py) and tests/test_gpu_filter_float64.py (the same cases on the device, through the C ABI).

The references are plain numpy, written from the header comment of include/seg3d_hip.h; each takes a `dtype`: float64 is the
reference, the same code in float32 on the CPU is the yardstick of the device tests.  They take what the C ABI takes -- the blur the
values of Seg3dBlurParams (radius and taps w[|k|] per modality, no sigma), the low-resolution simulation the low-grid sizes
(nx', ny', nz') per modality -- on a channels-last crop [Z][Y][X][M].  What is integer arithmetic in the operation (reflection, the
low-grid index k, the numerator of the fraction, the source index) is integer arithmetic in both evaluations; the taps are the float32
values the entry receives in both.

Launch arithmetic restated from csrc/augment_filter.hip and csrc/mc_device.h: one workgroup per TZ x TY x TX = 8 x 8 x 32 output tile;
mc_vec_rows: M == 4 and 16-byte bases, or M == 2 and 8-byte bases; the blur runs <4, true> / <2, true> on vector rows and <1, false>
with grid y = M otherwise, a maximum radius of 0 is the copy kernel; the low-resolution simulation goes through MC_DISPATCH on the
alignment of dst alone (M = 3 and M >= 5 run the runtime width <0, false>), every modality at full size is the copy kernel; its LDS
patch is LR_P = 35 x 11 x 11 (x, y, z) low voxels.
"""
from collections import namedtuple

import numpy as np

from float64_util import _noise

TX, TY, TZ = 32, 8, 8
LR_P = (TX + 3, TY + 3, TZ + 3)              # (x, y, z)
MAX_RADIUS, MAX_M, LOWRES_MAX_AXIS = 6, 8, 1 << 14
CAP = 1e-5                                   # x max|x|: the derived bar of tests/test_gpu_resolution_augment.py
FLOOR = 2e-6                                 # x max|x|
AMPLITUDE = 1.5

Blur = namedtuple('Blur', 'name zyx M radii kinds')          # kinds: 'g' Gaussian / 'f' free taps, one letter per modality
Lowres = namedtuple('Lowres', 'name zyx M lows')             # lows: (nx', ny', nz') per modality


def case_id(c):
    return c.name


def cdiv(a, b):
    return (a + b - 1) // b


def tiles(zyx):
    """(tiles x, tiles y, tiles z)"""
    return cdiv(zyx[2], TX), cdiv(zyx[1], TY), cdiv(zyx[0], TZ)


def vec_rows(M, shift):
    """mc_vec_rows for bases `shift` floats past a 16-byte boundary"""
    return M in (2, 4) and (4 * shift) % (4 * M) == 0


def launches(c):
    """the case's own launch (aligned bases) and, for a case on vector rows, the launch one float past alignment"""
    return [('', 0)] + ([('shifted_', 1)] if vec_rows(c.M, 0) else [])


def crop(c, seed=0):
    """[Z][Y][X][M] float32"""
    return (_noise(4100 + seed, 'filter/' + c.name, tuple(c.zyx) + (c.M,)) * AMPLITUDE).numpy().astype(np.float32)


# ---- blur ----------------------------------------------------------------------------------------------------------------------------
def gaussian_taps(R):
    """w[|k|], k = 0..6, float32: exp(-k^2 / (2 s^2)) normalised over -R..R in double, s = R / 3 (so that R = ceil(3 s))"""
    w = np.zeros(7, dtype=np.float32)
    if R == 0:
        w[0] = 1.0
        return w
    s = R / 3.0
    k = np.arange(-R, R + 1, dtype=np.float64)
    g = np.exp(-k * k / (2.0 * s * s))
    g = g / g.sum()
    w[:R + 1] = g[R:].astype(np.float32)
    return w


_FREE = (0.4, 0.9, 0.0, 0.7, 0.1, 0.5, 0.3)      # distinct, not monotone (the centre is not the largest), an exact 0 at |k| = 2


def free_taps(R, m):
    """w[|k|], k = 0..6, float32: distinct, not monotone, w[2] == 0 for R >= 2, another set per modality m, normalised so
    that w0 + 2 sum_k w_k = 1 (to float32 rounding): each pass is still a convex combination, which the derivation of the cap uses"""
    w = np.zeros(7, dtype=np.float32)
    raw = np.array([v * (1.0 + 0.07 * m * k) for k, v in enumerate(_FREE[:R + 1])], dtype=np.float64)
    raw = raw / (raw[0] + 2.0 * raw[1:].sum())
    w[:R + 1] = raw.astype(np.float32)
    return w


def blur_taps(c):
    """[M][7] float32"""
    return np.stack([gaussian_taps(r) if k == 'g' else free_taps(r, m) for m, (r, k) in enumerate(zip(c.radii, c.kinds))])


def reflect(i, n):
    """half-sample reflection: i' = i mod 2n, i' >= n -> 2n - 1 - i'"""
    r = np.mod(np.asarray(i, dtype=np.int64), 2 * n)
    return np.where(r >= n, 2 * n - 1 - r, r)


def blur_ref(x, radius, taps, dtype):
    """x [Z][Y][X][M]; radius[m] and taps[m][|k|] as in Seg3dBlurParams.  Separable x, then y, then z; the taps are added in the
    order -R..R onto 0; radius 0 leaves the modality as it is"""
    x = np.asarray(x)
    out = np.empty(x.shape, dtype=dtype)
    for m in range(x.shape[3]):
        y, R = x[..., m].astype(dtype), int(radius[m])
        if R > 0:
            w = np.asarray(taps[m], dtype=np.float32).astype(dtype)
            for axis in (2, 1, 0):
                n = y.shape[axis]
                acc = np.zeros_like(y)
                for k in range(-R, R + 1):
                    acc = acc + w[abs(k)] * np.take(y, reflect(np.arange(n) + k, n), axis=axis)
                y = acc
        out[..., m] = y
    return out


def blur_launch(c, shift):
    """('copy' | (MC, VEC), grid y, staged halo R, LDS bytes)"""
    R = max(c.radii)
    if R == 0:
        return 'copy', 1, 0, 0
    MC = (4 if c.M == 4 else 2) if vec_rows(c.M, shift) else 1
    PW, PH, PZ = TX + 2 * R, TY + 2 * R, TZ + 2 * R
    return (MC, MC > 1), c.M // MC, R, 4 * (MC * (PH * PW + PH * TX + 8) + PW + PH + PZ)


# (z, y, x): exactly one tile, one voxel more on every axis, three tiles along every axis with X = 65, an axis of 1, every axis
# shorter than the radius (z = 2 under R = 6: three reflections), y = 2 beside x = 1
_ONE, _ODD, _THREE, _FLAT, _SHORT, _THIN = (8, 8, 32), (9, 9, 33), (17, 17, 65), (1, 7, 33), (2, 3, 5), (5, 2, 1)
BLUR_CASES = [
    Blur('m4_r0_6_1_5_odd', _ODD, 4, (0, 6, 1, 5), 'gfgf'),            # 0 beside 6, 1 beside 5: the halo is 6, each channel its own
    Blur('m4_r2_3_4_1_one', _ONE, 4, (2, 3, 4, 1), 'fgfg'),
    Blur('m4_r6_0_5_2_three', _THREE, 4, (6, 0, 5, 2), 'ffgg'),        # a z column's planes cross two tile borders
    Blur('m4_r6_5_1_0_short', _SHORT, 4, (6, 5, 1, 0), 'gffg'),
    Blur('m4_r3_3_3_3_flat', _FLAT, 4, (3, 3, 3, 3), 'gfgf'),
    Blur('m2_r0_6_odd', _ODD, 2, (0, 6), 'gf'),
    Blur('m2_r1_5_one', _ONE, 2, (1, 5), 'fg'),
    Blur('m2_r2_4_three', (17, 5, 65), 2, (2, 4), 'gf'),
    Blur('m2_r3_6_flat', _FLAT, 2, (3, 6), 'fg'),
    Blur('m2_r6_1_thin', _THIN, 2, (6, 1), 'ff'),
    Blur('m1_r1_odd', _ODD, 1, (1,), 'f'),
    Blur('m1_r5_three', (17, 9, 33), 1, (5,), 'g'),
    Blur('m1_r6_short', _SHORT, 1, (6,), 'f'),
    Blur('m3_r3_4_1_one', _ONE, 3, (3, 4, 1), 'gfg'),
    Blur('m3_r0_2_6_thin', _THIN, 3, (0, 2, 6), 'gfg'),
    Blur('m5_r6_0_5_1_2_odd', _ODD, 5, (6, 0, 5, 1, 2), 'fgfgf'),
    Blur('m8_r0_to_6_three', (17, 8, 65), 8, (0, 1, 2, 3, 4, 5, 6, 3), 'gfgfgfgf'),
]
BLUR_LAUNCHES = ((4, True), (2, True), (1, False))


def swapped_taps(taps, radii):
    """the disagreement trial: w[1] and w[R] of every modality with R >= 2 change places (the sum of the taps is unchanged)"""
    t = np.array(taps, copy=True)
    for m, R in enumerate(radii):
        if R >= 2:
            t[m, 1], t[m, R] = taps[m][R], taps[m][1]
    return t


# ---- low-resolution simulation -------------------------------------------------------------------------------------------------------
def lowres_k(i, n, nl):
    """low-grid index k of output index i (the taps are k - 1 .. k + 2): floor(((2 i + 1) n' - n) / 2n), >= -1"""
    return np.floor_divide((2 * np.asarray(i, dtype=np.int64) + 1) * nl - n, 2 * n)


def lowres_axis(n, nl, dtype):
    """source indices [4][n] (integer) and Keys a = -0.5 weights [4][n] (dtype) of one axis"""
    i = np.arange(n, dtype=np.int64)
    t = (2 * i + 1) * nl - n
    k = lowres_k(i, n, nl)
    f = (t - 2 * n * k).astype(dtype) / dtype(2 * n)
    f2 = f * f
    f3 = f2 * f
    h, one = dtype(0.5), dtype(1.0)
    w = [-h * f3 + f2 - h * f, dtype(1.5) * f3 - dtype(2.5) * f2 + one, -dtype(1.5) * f3 + dtype(2.0) * f2 + h * f, h * f3 - h * f2]
    q = np.clip(np.stack([k - 1, k, k + 1, k + 2]), 0, nl - 1)
    s = np.minimum(n - 1, ((2 * q + 1) * n) // (2 * nl))
    return s, w


def lowres_ref(x, lows, dtype):
    """x [Z][Y][X][M]; lows[m] = (nx', ny', nz').  x innermost, then y, then z; the taps are added in the order k-1 .. k+2 (the
    first product starts the sum).  A modality with all three sizes equal to the crop's is left as it is"""
    x = np.asarray(x)
    Z, Y, X, M = x.shape
    out = np.empty(x.shape, dtype=dtype)
    for m in range(M):
        y = x[..., m].astype(dtype)
        if tuple(lows[m]) != (X, Y, Z):
            for axis, nl in ((2, lows[m][0]), (1, lows[m][1]), (0, lows[m][2])):
                n = y.shape[axis]
                s, w = lowres_axis(n, int(nl), dtype)
                shape = [1, 1, 1]
                shape[axis] = n
                acc = w[0].reshape(shape) * np.take(y, s[0], axis=axis)
                for j in range(1, 4):
                    acc = acc + w[j].reshape(shape) * np.take(y, s[j], axis=axis)
                y = acc
        out[..., m] = y
    return out


def lowres_launch(c, shift):
    """'copy' or (KC, VEC) as MC_DISPATCH picks it from M and the alignment of dst"""
    Z, Y, X = c.zyx
    if all(tuple(low) == (X, Y, Z) for low in c.lows):
        return 'copy'
    if c.M == 1:
        return 1, False
    if c.M in (2, 4):
        return c.M, vec_rows(c.M, shift)
    return 0, False


def lowres_extents(n, nl, tile):
    """the patch extent k(last) - k(first) + 4 of every tile of one axis"""
    out = []
    for i0 in range(0, n, tile):
        i1 = min(i0 + tile, n) - 1
        out.append(int(lowres_k(i1, n, nl)) - int(lowres_k(i0, n, nl)) + 4)
    return out


def lowres_patch(c, m):
    """(largest extent along x, y, z) over the tiles, for modality m"""
    Z, Y, X = c.zyx
    nx, ny, nz = c.lows[m]
    return max(lowres_extents(X, nx, TX)), max(lowres_extents(Y, ny, TY)), max(lowres_extents(Z, nz, TZ))


def zoom_sizes(xyz, zoom):
    """n' = max(1, floor(n zoom + 0.5))"""
    return tuple(max(1, int(np.floor(n * zoom + 0.5))) for n in xyz)


_CROP, _FULL = (9, 9, 33), (33, 9, 9)                 # (z, y, x) and its sizes (x, y, z)
_EXT, _EXT_LOW = (16, 16, 64), (63, 15, 15)           # n' = n - 1 on full tiles: the patch is exactly 35 x 11 x 11
_EXT1, _EXT1_LOW = (17, 17, 65), (64, 16, 16)         # the same with a partial tile behind every full one
_ZOOMED = (9, 16, 64)                                 # zoom 0.99 gives (63, 16, 9): no copy, unlike the shapes of the older test
LOWRES_CASES = [
    Lowres('m1_patch_35_11_11', _EXT, 1, (_EXT_LOW,)),
    Lowres('m1_patch_partial_tiles', _EXT1, 1, (_EXT1_LOW,)),
    Lowres('m2_patch_35_11_11', _EXT, 2, (_EXT_LOW, (64, 15, 16))),
    Lowres('m4_patch_partial_tiles', _EXT1, 4, (_EXT1_LOW, (65, 17, 16), (1, 16, 17), (64, 1, 1))),
    Lowres('m4_one_low_voxel', _CROP, 4, ((1, 9, 9), (33, 1, 9), (33, 9, 1), (1, 1, 1))),       # the k = -1 branch, every tap clamped
    Lowres('m2_full_axes', _CROP, 2, ((33, 9, 4), (33, 5, 4))),                                   # n' = n on two axes, on one
    Lowres('m4_one_copied', _CROP, 4, ((17, 5, 5), _FULL, (20, 9, 3), (33, 4, 9))),
    Lowres('m5_one_copied', _CROP, 5, ((17, 5, 5), (32, 8, 8), _FULL, (33, 9, 8), (2, 2, 2))),
    Lowres('m3_zooms', _ZOOMED, 3, tuple(zoom_sizes(_ZOOMED[::-1], z) for z in (0.5, 0.26, 0.99))),
    Lowres('m3_one_low_voxel', _CROP, 3, ((1, 1, 1), (1, 9, 9), (32, 8, 8))),
    Lowres('m5_zooms', _ZOOMED, 5, tuple(zoom_sizes(_ZOOMED[::-1], z) for z in (0.99, 0.5, 0.26, 0.99, 0.5))),
    Lowres('m8_patch_partial_tiles', _EXT1, 8, (_EXT1_LOW, (65, 17, 17), (64, 17, 17), (65, 16, 17), (65, 17, 16), (1, 1, 1),
                                                (33, 9, 9), (17, 4, 4))),
    Lowres('m1_one_low_voxel', _CROP, 1, ((1, 1, 1),)),
]
LOWRES_LAUNCHES = ((1, False), (2, True), (2, False), (4, True), (4, False), (0, False))


def off_by_one(c):
    """the disagreement trial: every reduced axis one low voxel shorter (or longer where n' = 1)"""
    Z, Y, X = c.zyx
    return tuple(tuple(nl if nl == n else (nl - 1 if nl > 1 else 2) for nl, n in zip(low, (X, Y, Z))) for low in c.lows)


def bar(yard, scale):
    """min(4 * yardstick + FLOOR * max|x|, CAP * max|x|)"""
    return min(4.0 * yard + FLOOR * scale, CAP * scale)


REFUSALS = {
    'seg3d_augment_blur': ('radius 7', 'a tap of 1.5', 'src and dst overlap', 'M = 9'),
    'seg3d_augment_lowres': ("n' = 0", "n' = n + 1", 'an axis of 16385'),
}
