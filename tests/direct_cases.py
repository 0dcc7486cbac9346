"""The case tables of the VALU fallback conv family (csrc/conv_direct.hip) and of the head's per-voxel tail (seg3d_softmax_* and
seg3d_sigmoid_* of csrc/loss.hip), shared by tests/test_direct_variants.py (host only: every weight-gradient case reaches the
kernel, chunk count, PAIRS and reducer it is named for, every code of the queries is named by a case) and
tests/test_gpu_direct_float64.py (the same cases against float64 on the device).

The codes are those of include/seg3d_hip.h:
  seg3d_wgrad_direct_variant   0 wgrad_direct_kernel<3,1,1>, 1 <2,2,0>, 2 <1,1,0>, 3 wgrad_k1_thin_kernel
  seg3d_wgrad_reduce_variant   0 wgrad_reduce_kernel, 1 wgrad_reduce_wide_kernel
Extents are those the ENTRY takes: the input's for the forward kernels (the fine grid for k2s2, the coarse one for convT), P's for
the weight gradient (the fine grid for stride 2).
"""
from collections import namedtuple

FWD_KERNELS = {'k3': (3, 1), 'k2s2': (2, 2), 'k1': (1, 1), 'convT': None}      # (ksize, stride) of seg3d_conv3d_fwd_direct
WGRAD_KERNELS = {'k3': 0, 'k2s2': 1, 'k1': 2, 'k1_thin': 3}
WGRAD_KS = {'k3': (3, 1), 'k2s2': (2, 2), 'k1': (1, 1), 'k1_thin': (1, 1)}
ITEMS_PER_TRIP = 8192 * 256           # seg3d_ew_grid caps the grid at 8192 workgroups of 256 threads

# role 'fwd': the weight in its forward layout, bias given; 'dgrad': the weight image _ops.conv_dgrad packs for this kernel (k3:
# flipped taps), bias = NULL.  Cin / Cout are the KERNEL's (its reduction / output channels), whatever the role
Fwd = namedtuple('Fwd', 'kernel role N D H W Cin Cout')
# role 'conv': P = x, Q = dy; 'convT': P = dy on the fine grid, Q = x (the same kernel, roles swapped).  chunks, pairs, wide: the launch
# plan the queries must report.  swapped: dw[a][b][t] instead of dw[b][a][t] (the layout every role of _ops.conv_wgrad asks for).
# Every case runs with accumulate = 0; accumulate = 1: it also runs from a known base
Wgrad = namedtuple('Wgrad', 'kernel role N D H W CA CB chunks pairs wide accumulate swapped')
Tail = namedtuple('Tail', 'op N S C')


def case_id(c):
    vals = [('T' if v else 'F') if isinstance(v, bool) else str(v) for v in c]
    return type(c).__name__.lower() + '-' + '-'.join(vals)


def wgrad_code(c):
    return WGRAD_KERNELS[c.kernel]


def reduce_code(c):
    return int(c.wide)


def taps(c):
    return WGRAD_KS[c.kernel][0] ** 3


def q_dims(c):
    s = WGRAD_KS[c.kernel][1]
    return c.D // s, c.H // s, c.W // s


def out_voxels(c):
    """output voxels of a forward case"""
    v = c.N * c.D * c.H * c.W
    return v // 8 if c.kernel == 'k2s2' else v * 8 if c.kernel == 'convT' else v


def items(c):
    """(voxel, quad) work items of a forward case"""
    return out_voxels(c) * ((c.Cout + 3) // 4)


def launch_plan(nvox, T, CA, CB):
    """the launcher's arithmetic, restated: (chunks, chunk_vox, voxels of the last chunk, PAIRS, gridDim.y, slabs the workspace holds)"""
    CBP = (CB + 3) // 4 * 4
    upper = max(1, min((nvox + 2047) // 2048, 512, (64 << 20) // (T * CA * CBP * 4)))
    chunk_vox = (nvox + upper - 1) // upper
    chunks = (nvox + chunk_vox - 1) // chunk_vox
    total_pairs = CA * (CBP // 4)
    pairs = 1
    while pairs < total_pairs and pairs < 256:
        pairs *= 2
    return chunks, chunk_vox, nvox - (chunks - 1) * chunk_vox, pairs, (total_pairs + pairs - 1) // pairs, upper


def _f(kernel, role, N, dims, Cin, Cout):
    return Fwd(kernel, role, N, dims[0], dims[1], dims[2], Cin, Cout)


FWD_CASES = [
    _f('k3', 'fwd', 3, (5, 7, 9), 3, 5),               # scalar loads, a partial last quad; halos between three samples
    _f('k3', 'fwd', 1, (1, 3, 40), 12, 8),             # float4 loads and stores, extent 1
    _f('k3', 'dgrad', 1, (9, 11, 23), 10, 6),          # flip = 1, no bias; Cout % 4 = 2
    _f('k3', 'dgrad', 3, (3, 1, 5), 4, 7),             # float4 loads with a partial quad (Cout % 4 = 3)
    _f('k3', 'fwd', 1, (32, 32, 36), 3, 256),          # 2.36 M items: the second grid-stride trip
    _f('k2s2', 'fwd', 3, (6, 10, 14), 6, 10),          # scalar loads, partial quad
    _f('k2s2', 'dgrad', 1, (4, 6, 8), 8, 12),          # float4 loads and stores
    _f('k2s2', 'dgrad', 3, (2, 2, 6), 5, 3),           # a single, partial quad (Cout % 4 = 3)
    _f('k2s2', 'fwd', 1, (64, 64, 66), 4, 256),        # 2.16 M items
    _f('k1', 'fwd', 3, (5, 7, 9), 5, 5),               # the head's shape
    _f('k1', 'dgrad', 1, (9, 11, 23), 2, 3),           # scalar loads, partial quad
    _f('k1', 'fwd', 1, (9, 11, 23), 32, 8),            # float4 loads and stores
    _f('k1', 'fwd', 3, (1, 1, 7), 4, 6),               # extents of 1; float4 loads with a partial quad (Cout % 4 = 2)
    _f('k1', 'dgrad', 1, (63, 127, 131), 5, 9),        # 3.1 M items
    _f('convT', 'fwd', 3, (2, 3, 5), 6, 10),           # scalar loads, partial quad
    _f('convT', 'dgrad', 1, (3, 4, 6), 12, 8),         # float4 loads and stores
    _f('convT', 'dgrad', 3, (1, 1, 3), 3, 5),          # extents of 1, Cout % 4 = 1
    _f('convT', 'fwd', 1, (32, 32, 33), 4, 32),        # 2.16 M items
]


def _w(kernel, role, N, dims, CA, CB, chunks, pairs, wide, accumulate, swapped):
    return Wgrad(kernel, role, N, dims[0], dims[1], dims[2], CA, CB, chunks, pairs, wide, accumulate, swapped)


WGRAD_CASES = [
    _w('k3', 'conv', 3, (5, 7, 9), 3, 5, 1, 8, False, 0, False),               # 6 pairs: two idle pair lanes, 32 voxel lanes
    _w('k3', 'conv', 1, (9, 11, 23), 10, 6, 2, 32, False, 1, False),           # 2277 voxels in chunks of 1139 / 1138; scalar Q loads
    _w('k3', 'conv', 1, (9, 11, 23), 24, 40, 2, 256, False, 0, True),          # 240 pairs: one voxel lane
    _w('k3', 'conv', 2, (5, 7, 9), 20, 56, 1, 256, False, 1, False),           # 280 pairs: gridDim.y = 2, 24 live pairs in row 1
    _w('k3', 'conv', 1, (63, 127, 131), 3, 5, 512, 8, True, 1, False),         # 1 048 131 voxels: 512 chunks, the last one 1603
    _w('k2s2', 'conv', 3, (6, 10, 14), 6, 10, 1, 32, False, 1, False),
    _w('k2s2', 'conv', 1, (4, 6, 8), 8, 12, 1, 32, False, 0, True),            # float4 Q loads
    _w('k2s2', 'convT', 1, (18, 22, 46), 12, 5, 2, 32, False, 1, False),       # P = dy on the fine grid, Q = x
    _w('k1_thin', 'conv', 3, (5, 7, 9), 5, 5, 1, 16, False, 0, False),         # the head
    _w('k1_thin', 'conv', 2, (17, 19, 23), 2, 3, 8, 2, False, 1, True),        # 8 chunks, the last one 1852 voxels
    _w('k1_thin', 'conv', 1, (9, 11, 23), 8, 8, 2, 16, False, 0, False),       # the upper edge of the thin rule
    _w('k1_thin', 'conv', 1, (63, 127, 131), 5, 5, 512, 16, True, 1, True),    # thin kernel + wide reducer: the production pair
    _w('k1', 'conv', 1, (9, 11, 23), 32, 5, 2, 64, False, 1, False),
    _w('k1', 'conv', 1, (9, 11, 23), 9, 8, 2, 32, False, 0, True),             # just outside the thin rule
]
# voxels of the ragged last chunk, by position in WGRAD_CASES
LAST_CHUNK = {1: 1138, 4: 1603, 9: 1852}

ALL_WGRAD_CODES, ALL_REDUCE_CODES = [0, 1, 2, 3], [0, 1]

# the reducer on its own: chunks x (T, A, B) x layout; T * A * B in {1, 2048, 2049}
REDUCE_CHUNKS = [1, 511, 512, 700]
REDUCE_TAB = [(1, 1, 1), (8, 16, 16), (1, 3, 683)]

# packer: (T, A, B)
PACK_CASES = [(T, A, B) for T in (27, 8, 1) for (A, B) in ((3, 1), (5, 3), (2, 5), (6, 8))]

BIG_S = 699071                       # 3 * 699 071 = 2 097 213 voxels > 8192 * 256
TAIL_CASES = [Tail(op, 3, 5 * 7 * 9, C) for op in ('softmax', 'sigmoid') for C in (1, 2, 5, 16)] + \
             [Tail('softmax', 3, BIG_S, 2), Tail('sigmoid', 3, BIG_S, 2)]

# argument sets seg3d_wgrad_direct refuses before a launch: (N, Dp, Hp, Wp, CA, CB, ksize, stride), what is wrong
REFUSALS = [
    ((1, 5, 6, 8, 4, 4, 2, 2), 'an odd extent with stride 2'),
    ((1, 4, 6, 8, 4, 4, 3, 2), 'ksize 3 with stride 2'),
    ((1, 4, 6, 8, 4, 4, 2, 1), 'ksize 2 with stride 1'),
    ((1, 4, 6, 8, 4, 4, 5, 1), 'ksize 5'),
    ((1, 4, 6, 8, 4, 4, 0, 1), 'ksize 0'),
    ((0, 4, 6, 8, 4, 4, 3, 1), 'no samples'),
    ((1, 4, 0, 8, 4, 4, 3, 1), 'an extent of 0'),
    ((1, 4, 6, 8, 0, 4, 1, 1), 'CA = 0'),
    ((1, 4, 6, 8, 4, -1, 1, 1), 'CB < 0'),
]
