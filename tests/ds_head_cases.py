"""The case table, the inputs and the float64 reference of the deep-supervision head (ds_head_fwd_kernel, ds_head_bwd_kernel and
ds_head_bwd_finalize_kernel of csrc/deep_supervision.hip) and of the label pyramid.  Shared by tests/test_ds_head_cases.py (host only:
every <C, VPI, NQ> of both kernels is named by a case, every case has the tiles, the tail, the slab count and the grid-stride trip it
is named for) and tests/test_gpu_ds_head_float64.py (the same cases on the device, through the C ABI).

The reference is plain torch from the header text of include/seg3d_hip.h: p = softmax_c(x w^T + b) with the maximum subtracted,
g_c = p_c (dp_c - sum_k p_k dp_k), dx = g w, dw = g^T x, db = sum_v g.  It takes a `dtype`: float64 is the reference, float32 on the
CPU the yardstick.

Rules restated from csrc/deep_supervision.hip: a voxel row is spread over GROUP = 16 lanes, lane j holding the channel quads j, j + 16,
..; NQ = nq(Cin) quads per lane; a workgroup has GROUPS = 16 groups of VPI voxels, so a tile is 16 * VPI voxels: fwd_vpi(NQ) forward,
bwd_vpi(C, NQ) backward; the forward grid is min(tiles, 8 * CUs), the backward's min(slabs, 4 * CUs) with slabs = min(tiles,
BWD_MAX_BLOCKS) slabs of C * Cin + C floats in the workspace.  The tables are built for CUS = 256 compute units; the device test reads
the count from the device and holds every claimed trip against it.
"""
from collections import namedtuple

import torch

from float64_util import _noise

MAX_CIN, MAX_C, GROUP, GROUPS, BWD_MAX_BLOCKS, CUS = 256, 8, 16, 16, 1024, 256
NQS = (1, 2, 4)
FULL_CIN = {1: 64, 2: 128, 4: 256}
PARTIAL_CIN = {1: (4, 36, 60), 2: (68, 100, 124), 4: (132, 200, 252)}

# ldx / ld_dx: 'packed' = 0, 'pad' = Cin + 4 (+ 8 for dx), 'slice' = 2 Cin (+ 4 for dx), the row the LAST Cin floats of the wider one
Head = namedtuple('Head', 'N S Cin C ldx ld_dx bias accumulate dw db values dprobs')


def case_id(c):
    return 'head-' + '-'.join(str(v) for v in c)


# ---- plans -------------------------------------------------------------------------------------------------------------------------
def nq(Cin):
    return 1 if Cin <= 64 else (2 if Cin <= 128 else 4)


def fwd_vpi(NQ):
    return 8 if NQ == 1 else 4


def bwd_vpi(C, NQ):
    return 8 if C * NQ <= 4 else (4 if C * NQ <= 8 else (2 if C * NQ <= 16 else 1))


def tiles(V, vpi):
    return (V + GROUPS * vpi - 1) // (GROUPS * vpi)


def bwd_slabs(V, Cin, C):
    return min(tiles(V, bwd_vpi(C, nq(Cin))), BWD_MAX_BLOCKS)


def workspace_floats(c):
    return bwd_slabs(c.N * c.S, c.Cin, c.C) * (c.C * c.Cin + c.C)


def fwd_plan(c, cus=CUS):
    """(<C, VPI, NQ>, tiles, workgroups, second grid-stride trip)"""
    q = nq(c.Cin)
    t = tiles(c.N * c.S, fwd_vpi(q))
    return (c.C, fwd_vpi(q), q), t, min(t, 8 * cus), t > 8 * cus


def bwd_plan(c, cus=CUS):
    q = nq(c.Cin)
    t = tiles(c.N * c.S, bwd_vpi(c.C, q))
    g = min(bwd_slabs(c.N * c.S, c.Cin, c.C), 4 * cus)
    return (c.C, bwd_vpi(c.C, q), q), t, g, t > g


def partial_group(c):
    """some lane of the group holds fewer than NQ quads: a `q < nq` guard is taken"""
    return c.Cin // 4 < GROUP * nq(c.Cin)


def strides(c):
    """(ldx argument, row stride of x, ld_dx argument, row stride of dx) in floats"""
    ldx = {'packed': 0, 'pad': c.Cin + 4, 'slice': 2 * c.Cin}[c.ldx]
    ldd = {'packed': 0, 'pad': c.Cin + 8, 'slice': 2 * c.Cin + 4}[c.ld_dx]
    return ldx, ldx or c.Cin, ldd, ldd or c.Cin


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def _split(V):
    """(N, S) with N * S = V: the largest N of 3, 2 that divides V with an odd S > 1, so that a sample boundary falls inside a
    group's run of voxels; else one sample"""
    for N in (3, 2):
        if V % N == 0 and (V // N) % 2 == 1 and V // N > 1:
            return N, V // N
    return 1, V


LDS = ('packed', 'pad', 'slice')
VALUES = ('std', 'equal', 'wide', 'zero')


def _table():
    cases, i = [], 0
    for C in range(1, MAX_C + 1):
        for q in NQS:
            for Cin in (FULL_CIN[q], PARTIAL_CIN[q][(C + NQS.index(q)) % 3]):
                tf, tb = GROUPS * fwd_vpi(q), GROUPS * bwd_vpi(C, q)
                V = (1, tf - 1, tb + 1, 2 * tf + 3, tb - 1, tf + 1, 2 * tb + 3, 2 * tb + 2)[i % 8]
                N, S = _split(V)
                values = VALUES[i % 4]
                cases.append(Head(N, S, Cin, C, LDS[i % 3], LDS[(i + 1 + i // 3) % 3], 0 if (i % 5 == 3 or values == 'zero') else 1, i % 4,
                                  0 if i % 7 == 3 else 1, 0 if i % 7 == 5 else 1, values, 'plane' if i % 3 == 1 else 'dense'))
                i += 1
    return cases


CASES = _table()
# the second grid-stride trip, sizes from the rules above: one tile more than the grid holds workgroups, the last tile partial
FWD_TRIP_4 = Head(2, ((8 * CUS + 1) * GROUPS * fwd_vpi(1) - 122) // 2, 4, 2, 'packed', 'packed', 1, 0, 1, 1, 'std', 'dense')
FWD_TRIP_68 = Head(1, (8 * CUS + 1) * GROUPS * fwd_vpi(2) - 59, 68, 3, 'packed', 'pad', 1, 0, 1, 1, 'std', 'plane')
BWD_TRIP_VPI1 = Head(1, (BWD_MAX_BLOCKS + 1) * GROUPS * bwd_vpi(5, 4) - 3, 132, 5, 'pad', 'packed', 1, 0, 1, 1, 'std', 'dense')
BWD_TRIP_VPI8 = Head(3, ((BWD_MAX_BLOCKS + 1) * GROUPS * bwd_vpi(4, 1) - 5) // 3, 36, 4, 'packed', 'packed', 1, 0, 1, 1, 'std', 'dense')
TRIP_CASES = [FWD_TRIP_4, FWD_TRIP_68, BWD_TRIP_VPI1, BWD_TRIP_VPI8]

PYRAMID_SHAPE = (2, 8, 16, 24)       # N, D, H, W
REFUSALS = {'seg3d_ds_head_fwd': 'ldx = Cin + 2', 'seg3d_ds_head_bwd': 'ld_dx below Cin', 'seg3d_ds_head_bwd_finalize': 'accumulate = 4',
            'seg3d_label_pyramid': 'a size that 2^levels does not divide'}


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def inputs(c):
    """(x [V, Cin], w [C, Cin], b [C], dprobs [N, C, S], dw0 [C, Cin], db0 [C]): 'std' -- logits of unit spread; 'equal' -- equal biases
    and every other row of x zero, so every other row of logits is one value C times (probabilities of exactly 1 / C there); 'wide' --
    logits spread over +-80; 'zero' -- a zero weight matrix (the probabilities are exactly 1 / C; such a case has no bias).  dprobs 'plane': kept on one plane per voxel.  dw0 / db0: what
    the gradient buffers hold before an accumulating finalize"""
    V, Cin, C = c.N * c.S, c.Cin, c.C
    tag = 'dshead/' + case_id(c)
    x = _noise(3200, tag + '/x', (V, Cin))
    w = _noise(3201, tag + '/w', (C, Cin)) / float(Cin) ** 0.5
    b = 0.5 * _noise(3202, tag + '/b', (C,))
    if c.values == 'equal':
        x[0::2], b = 0.0, b[:1].repeat(C)
    elif c.values == 'wide':
        w = w * 30.0
    elif c.values == 'zero':
        w = torch.zeros_like(w)
    d = _noise(3203, tag + '/d', (c.N, C, c.S))
    if c.dprobs == 'plane':
        keep = (torch.arange(c.S).view(1, 1, -1) + torch.arange(c.N).view(-1, 1, 1)) % C == torch.arange(C).view(1, -1, 1)
        d = torch.where(keep, d, torch.zeros_like(d))
    return x, w, b, d, _noise(3204, tag + '/dw0', (C, Cin)), _noise(3205, tag + '/db0', (C,))


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def fwd_ref(x, w, b, N, S, dtype):
    """-> probs [N, C, S]"""
    l = x.to(dtype) @ w.to(dtype).t()
    if b is not None:
        l = l + b.to(dtype)
    e = torch.exp(l - l.max(1, keepdim=True).values)
    return (e / e.sum(1, keepdim=True)).reshape(N, S, -1).permute(0, 2, 1).contiguous()


def bwd_ref(p, d, x, w, dtype):
    """probs, dprobs [N, C, S] float32 -> (dx [V, Cin], dw [C, Cin], db [C])"""
    C = p.shape[1]
    P, D = p.to(dtype).permute(0, 2, 1).reshape(-1, C), d.to(dtype).permute(0, 2, 1).reshape(-1, C)
    g = P * (D - (P * D).sum(1, keepdim=True))
    return g @ w.to(dtype), g.t() @ x.to(dtype), g.sum(0)


def pyramid_input():
    """class ids, -1 and 255, +-0.0, infinities and NaNs with payloads: the pyramid copies bit patterns"""
    N, D, H, W = PYRAMID_SHAPE
    m = torch.floor(_noise(3210, 'dshead/pyramid', (N, D, H, W)).abs() * 4.0)
    bits = m.view(torch.int32).reshape(-1)
    special = torch.tensor([0x7FC00001, -0x400000 + 0x1234, 0x7F800001, -0x80000000, 0x7F800000, -0x800000, 0x437F0000, -0x40800000],
                           dtype=torch.int32)               # quiet / signalling NaNs with payloads, -0.0, +-inf, 255.0, -1.0
    for i in range(bits.numel() // 3):
        bits[3 * i] = special[i % 8]
    return m
