"""The case table, the targets and the references of the dense signed distance map of csrc/boundary_loss.hip: seg3d_signed_distance
(sdf_x_kernel<J>, sdf_line_kernel<false> for pass y, sdf_line_kernel<true> for pass z).  Shared by tests/test_sdf_cases.py (host only:
every case reaches the J, tile counts, LDS bytes and grid it is named for) and tests/test_gpu_sdf_float64.py (the same cases on the
device, through the C ABI).  The loss half of the file is covered by tests/compound_cases.py.

The reference is the brute force over all voxel pairs of tests/boundary_oracle.py (signed_distance_oracle, float64; its class rule is
trunc(t) with 0 <= t < num_class and t != ignore_label, the header's "its class is (int)t", so it needed no extension).  sdf_ref
restates it with a `dtype`: float64 agrees with the oracle to rounding (tests/test_sdf_cases.py), float32 -- the weights s^2 rounded
once to float32 as the entry does, three float32 products and two sums per pair, one float32 root -- is the yardstick.  What stays
float32 in both is the counting rule on the float32 target.

Launch arithmetic restated from csrc/boundary_loss.hip: pass x runs sdf_x_kernel<J>, J = min(4, ceil(X / 64)), one wave per row, grid
(ceil(N Z Y / 4), K); pass y stages 32 neighbouring lines of length Y, grid (Z ceil(X / 32), N K), 2 * Y * 32 floats of LDS; pass z the
same over lines of length Z with inner = X Y, grid (ceil(X Y / 32), N K); four outputs per thread.  The workspace is two float32 fields
per (n, k): 8 N K X Y Z bytes.
"""
from collections import namedtuple

import numpy as np

from boundary_oracle import counted_mask

MAX_AXIS, TILE, MAXK, MAX_NK = 256, 32, 16, 65535
MIN_SPACING, MAX_SPACING = 1e-6, 1e6
CAP, FLOOR = 1e-6, 2e-7                     # relative, per non-zero element; the cap is the derived bar of tests/test_gpu_boundary_loss.py
NO_IGNORE = -1.0                            # what the entry takes for "no ignore label"
UNIT, ANISO = (1.0, 1.0, 1.0), (0.7, 1.3, 2.5)
EXTREME = ((1e-6, 1e-6, 1e-6), (1e6, 1e6, 1e6), (1e6, 1e-6, 1.0))

# name -> (ids, num_class): one id; a permuted list with an id >= num_class (G is empty: the plane is all zero); 16 ids
CLASS_LISTS = {'k1': ((1,), 3), 'k3': ((2, 0, 5), 4), 'k16': (tuple(range(16)), 16)}
PATTERNS = ('random', 'single_voxel', 'empty', 'everything', 'ignore_wall', 'out_of_range', 'fractional', 'fractional_ignore')

Sdf = namedtuple('Sdf', 'name N xyz classes spacing patterns')


def case_id(c):
    return c.name


def workspace_bytes(N, K, X, Y, Z):
    return N * K * 2 * X * Y * Z * 4


def plan(c):
    """J of pass x, (grid x, grid y) of the three passes, LDS bytes of pass y and z, partial tiles of pass y and z"""
    X, Y, Z = c.xyz
    K = len(CLASS_LISTS[c.classes][0])
    ty, tz = -(-X // TILE), -(-(X * Y) // TILE)
    return {'J': min(4, (X + 63) // 64), 'grid_x': (-(-(c.N * Z * Y) // 4), K), 'grid_y': (Z * ty, c.N * K), 'grid_z': (tz, c.N * K),
            'tiles_y': ty, 'tiles_z': tz, 'partial_y': X % TILE != 0, 'partial_z': (X * Y) % TILE != 0,
            'lds_y': 2 * Y * TILE * 4, 'lds_z': 2 * Z * TILE * 4, 'line4_y': Y % 4 == 0, 'line4_z': Z % 4 == 0}


def labels(pattern, c, seed):
    """(t [N][Z][Y][X] float32, ignore label as the entry takes it).  The first six are the patterns of
    tests/test_gpu_boundary_loss.py; 'fractional' adds in-contract non-integers (0.5, 1.7, num_class - 0.25, -0.0) and -0.5, which does
    not count; 'fractional_ignore' an ignore label that is itself fractional beside values that truncate to the same class"""
    X, Y, Z = c.xyz
    ids, nlab = CLASS_LISTS[c.classes]
    rng = np.random.RandomState(seed)
    cid = ids[0]
    other = [v for v in range(nlab) if v != cid]
    ignore, shape = NO_IGNORE, (c.N, Z, Y, X)
    if pattern == 'random':
        t = rng.randint(0, nlab, size=shape).astype(np.float32)
    elif pattern == 'single_voxel':
        t = np.full(shape, other[0], dtype=np.float32)
        t[0, Z // 2, Y // 2, X // 3] = cid
        t[-1, Z - 1, 0, X - 1] = cid
    elif pattern == 'empty':
        t = np.asarray(other)[rng.randint(0, len(other), size=shape)].astype(np.float32)
    elif pattern == 'everything':
        t = np.full(shape, cid, dtype=np.float32)
        t[-1] = rng.randint(0, nlab, size=(Z, Y, X))                 # the last sample keeps the batch index honest
    elif pattern == 'ignore_wall':
        t = np.full(shape, other[0], dtype=np.float32)
        ax = int(np.argmax((Z, Y, X)))
        n = (Z, Y, X)[ax]
        sl = [slice(None)] * 3
        sl[ax] = slice(0, n // 3)
        t[(slice(None),) + tuple(sl)] = cid
        sl[ax] = slice(n // 3, max(n // 3 + 1, n // 2))
        t[(slice(None),) + tuple(sl)] = 255
        ignore = 255.0
    elif pattern == 'out_of_range':
        t = rng.randint(0, nlab, size=shape).astype(np.float32)
        r = rng.rand(*shape)
        t[r < 0.1] = nlab
        t[(r >= 0.1) & (r < 0.2)] = -1
        t[(r >= 0.2) & (r < 0.25)] = 1000
    elif pattern == 'fractional':
        pool = np.array([0.0, 1.0, 0.5, 1.7, nlab - 0.25, -0.0, -0.5, float(cid), cid + 0.75, float(other[0])], dtype=np.float32)
        t = pool[rng.randint(0, len(pool), size=shape)]
    else:
        assert pattern == 'fractional_ignore'
        ignore = cid + 0.5                                           # counts as no class; cid + 0.25 and cid + 0.75 are class cid
        pool = np.array([ignore, cid + 0.25, cid + 0.75, float(cid), float(other[0]), other[0] + 0.5, other[-1] + 0.125, -0.5],
                        dtype=np.float32)
        t = pool[rng.randint(0, len(pool), size=shape)]
    if c.name == 'n3_one_sample_ignored':
        t[1] = 255.0 if ignore == NO_IGNORE else ignore              # (255 is out of range: it does not count either way)
    return t, ignore


def sdf_ref(t, ids, spacing, num_class, ignore, dtype, squared=False):
    """phi [N][K][Z][Y][X] in `dtype` by brute force over all (query, feature) pairs: the counting rule and the class trunc(t) on the
    float32 target; w = s^2 (for float32: computed in double and rounded once, as the entry does); d^2 = wx dx^2 + wy dy^2 + wz dz^2,
    x first; phi = +sqrt on H, -sqrt on G, 0 elsewhere and where G or H is empty.  Samples with equal targets are evaluated once"""
    t = np.asarray(t, dtype=np.float32)
    N, Z, Y, X = t.shape
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    px, py, pz = (a.ravel().astype(dtype) for a in (xx, yy, zz))
    wx, wy, wz = (dtype(float(s) * float(s)) for s in spacing)
    valid = counted_mask(t, num_class, None if ignore == NO_IGNORE else ignore).reshape(N, -1)
    cls = np.trunc(t).reshape(N, -1)
    phi, d2 = np.zeros((N, len(ids), Z * Y * X), dtype=dtype), np.zeros((N, len(ids), Z * Y * X), dtype=dtype)
    done = {}
    for n in range(N):
        key = t[n].tobytes()
        if key in done:
            phi[n], d2[n] = phi[done[key]], d2[done[key]]
            continue
        done[key] = n
        for k, cid in enumerate(ids):
            G = np.flatnonzero(valid[n] & (cls[n] == cid))
            H = np.flatnonzero(valid[n] & (cls[n] != cid))
            if len(G) == 0 or len(H) == 0:
                continue
            dx, dy, dz = (p[H][:, None] - p[G][None, :] for p in (px, py, pz))
            D = dx * dx * wx + dy * dy * wy + dz * dz * wz
            d2[n, k, H], d2[n, k, G] = D.min(1), D.min(0)
            phi[n, k, H], phi[n, k, G] = np.sqrt(d2[n, k, H]), -np.sqrt(d2[n, k, G])
    shape = (N, len(ids), Z, Y, X)
    return (phi.reshape(shape), d2.reshape(shape)) if squared else phi.reshape(shape)


def rel_err(got, ref):
    """largest |got - ref| / |ref| over the non-zero elements of ref (0.0 if there is none)"""
    nz = ref != 0
    return float((np.abs(got.astype(np.float64) - ref)[nz] / np.abs(ref)[nz]).max()) if nz.any() else 0.0


def bar(yard):
    return min(4.0 * yard + FLOOR, CAP)


# (X, Y, Z): J = 1..4 at both edges of each, a 256 line in pass z, one and two 32-line tiles full and partial in pass y and z, lines
# that are no multiple of 4
SHAPES = [(64, 1, 1), (128, 2, 1), (129, 1, 2), (192, 1, 1), (193, 2, 1), (2, 1, 256), (33, 1, 2), (31, 2, 3), (5, 7, 3)]
_LISTS = ('k1', 'k3', 'k16')
# the patterns over pairs of voxels are cheap: every one everywhere except on the 512-voxel line (random, wall and fractional there)
_LONG = ('random', 'ignore_wall', 'fractional')
CASES = [Sdf('{}x{}x{}_{}_{}'.format(*s, 'unit' if sp == UNIT else 'aniso', _LISTS[(i + j) % 3]), 2, s, _LISTS[(i + j) % 3], sp,
             _LONG if s[2] == 256 else PATTERNS)
         for i, s in enumerate(SHAPES) for j, sp in enumerate((UNIT, ANISO))]
CASES += [Sdf('{}x{}x{}_s{}_{}'.format(*s, j, _LISTS[(i + j) % 3]), 2, s, _LISTS[(i + j) % 3], sp, ('random', 'ignore_wall', 'fractional'))
          for i, s in enumerate(((9, 7, 5), (193, 2, 1))) for j, sp in enumerate(EXTREME)]
CASES += [Sdf('n3_one_sample_ignored', 3, (5, 7, 3), 'k3', ANISO, ('random', 'fractional', 'fractional_ignore')),
          Sdf('n4095_k16_grid_y', 4095, (2, 1, 1), 'k16', UNIT, ('fractional',)),          # N * K = 65520, next to the 65535 of grid y
          Sdf('n4095_k16_grid_y_aniso', 4095, (2, 1, 1), 'k16', ANISO, ('random',))]

REFUSALS = ('an axis of 257', 'K = 0', 'K = 17', 'spacing 0', 'spacing NaN', 'spacing 1e7', 'N * K = 65536', 'a null workspace')
