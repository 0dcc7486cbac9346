"""The case tables, the inputs and the float64 references of the compound loss family and what shares its code: the head activations
(softmax_fwd/bwd_kernel, sigmoid_fwd/bwd_kernel of csrc/loss.hip), the compound loss (compound_partial/finalize/bwd_kernel), Dice +
top-k (the seven kernels of csrc/topk_loss.hip), the streaming passes of the boundary loss (boundary_partial/finalize/bwd_kernel of
csrc/boundary_loss.hip, phi a given input) and confusion_counts_kernel of csrc/validation.hip.  Shared by tests/test_compound_cases.py
(host only: every case has the property it is named for, the references agree with the existing oracles) and
tests/test_gpu_compound_float64.py (the same cases on the device, through the C ABI).

The references are plain torch, written from the header comments of include/seg3d_hip.h; each takes a `dtype`: float64 is the
reference, the same code in float32 on the CPU is the yardstick of the device tests.  They take what the C ABI takes (wdice and
alpha as given, not normalised here) and return what it writes (loss[3], the coef block, ell, the gradient).  The oracles of
tests/test_compound_loss.py, tests/test_topk_loss.py and tests/boundary_oracle.py say the same for integer class ids
(tests/test_compound_cases.py holds the two against each other there); for a target that is no integer they build their one-hot
planes with `t == c` while the header's rule is "its class is (int)t", so the references here are written out in full.
What stays float32 in BOTH evaluations is what the operation itself defines on float32 values:
  the counting rule  0 <= t < C and t != ignore_label, compared on the float32 target; the class is trunc(t)
  the clamp          pt = max(p_t, float32(1e-12)) and the gradient's gate p_t >= float32(1e-12), on the float32 probability
  the arg-max        the first maximum of the float32 probabilities (a later class wins only if strictly greater)
  the top-k order    n, k, m, n_eq, r and the weights w_v are decided on ell rounded to float32 (equal inputs tie exactly)
Outside the tables: p_t == 1 with 0 < gamma < 1 (the derivative is inf * 0 there); loss_inputs keeps such a case below 1.

Constants restated from csrc/ (tests/test_compound_cases.py holds them against the library's queries where one exists): DICE_VPB
voxels per workgroup of the forward walk; the region finalize walks the blocks of one item with FIN_LANES lanes, FIN_ITEMS items
per round; compound_column_sum strides by COLUMN_THREADS; the backward grid is capped at BWD_MAX_GRID / N workgroups of 256
threads, one access each; a top-k histogram / sum pass at TOPK_MAX_GRID workgroups (two per compute unit of the 256); the confusion
pass at ceil(TOPK_MAX_GRID / N) workgroups of CONF_THREADS; the head kernels at ITEMS_PER_TRIP threads.
"""
import math
from collections import namedtuple

import torch

from float64_util import _noise
from loss_cases import DICE_VPB, ITEMS_PER_TRIP, MAXC, _labels, _uniform, case_id  # noqa: F401  (case_id: the tests' ids)

FIN_LANES, FIN_ITEMS, COLUMN_THREADS = 32, 8, 256
BWD_MAX_GRID, BWD_THREADS = 8192, 256
TOPK_MAX_GRID, TOPK_BITS = 512, (11, 11, 10)
TOPK_CTRL_BYTES, TOPK_HIST_BYTES, TOPK_SLOT_BYTES = 64, 3 * 2048 * 4, TOPK_MAX_GRID * 8
CONF_THREADS = 1024
EPS, PMIN = 1e-5, torch.tensor(1e-12, dtype=torch.float32)
NO_IGNORE = 255.0                     # an ignore label outside [0, C) for every C of the tables
BOUNDARY_WEIGHT = float(torch.tensor(0.01, dtype=torch.float32))     # the device float the finalize reads
MARGIN = 1e-5                         # the top-k rule on the inputs: the neighbours of tau are this far away (relative) or equal

Compound = namedtuple('Compound', 'N C S shift batch_dice ignore fill gamma dice_weight ce_weight')
TopK = namedtuple('TopK', 'N C S shift batch_dice ignore fill k_percent dice_weight ce_weight')
Boundary = namedtuple('Boundary', 'N C S shift batch_dice ignore fill include_background dice_weight')
Head = namedtuple('Head', 'kind N C S')
Confusion = namedtuple('Confusion', 'N C S shift ignore')

BLOCKS34 = 33 * DICE_VPB + 4          # 34 blocks: lanes 0 and 1 of the finalize take a second step; a multiple of 4
# (N, C, S, shift, batch_dice, ignore, fill): every C of 1..5, 6 and 16 on the 16-byte path (S % 4 == 0, shift 0), on the scalar
# path by S % 4 != 0 and on the scalar path by `shift` = 1 float past a 16-byte boundary with S % 4 == 0
SHAPES = [
    (1, 1, 1, 0, 0, NO_IGNORE, 'std'),                 # the smallest call; R * C = 1
    (1, 1, 4096, 0, 1, NO_IGNORE, 'std'),              # exactly one block
    (2, 1, 4096, 1, 0, -1.0, 'std'),                   # "no ignore label"
    (4, 2, 4096, 0, 0, NO_IGNORE, 'std'),              # R * C = 8: one finalize round, exactly full
    (4, 2, 4095, 0, 1, 1.0, 'std'),                    # one voxel short of a block; the ignore label inside [0, C)
    (1, 2, 64, 1, 0, NO_IGNORE, 'std'),
    (3, 3, 4096, 0, 0, 2.0, 'std'),                    # R * C = 9: a second round with one item
    (3, 3, 4097, 0, 0, NO_IGNORE, 'std'),              # a second block of one voxel
    (2, 3, 4100, 1, 1, NO_IGNORE, 'std'),
    (2, 4, BLOCKS34, 0, 0, NO_IGNORE, 'std'),          # 34 blocks
    (2, 4, BLOCKS34 + 1, 0, 1, 3.0, 'std'),            # its odd neighbour; batch_dice: 68 entries per item
    (1, 4, 64, 1, 0, NO_IGNORE, 'std'),
    (2, 5, 8192, 0, 1, NO_IGNORE, 'std'),
    (1, 5, 4097, 0, 0, 4.0, 'std'),
    (3, 5, 4096, 1, 0, NO_IGNORE, 'std'),
    (2, 6, 4096, 0, 0, NO_IGNORE, 'std'),              # the generic instantiation with planes predicated off
    (1, 6, 4095, 0, 1, NO_IGNORE, 'std'),
    (2, 6, 64, 1, 0, 5.0, 'std'),
    (3, 16, 4096, 0, 0, NO_IGNORE, 'std'),             # R * C = 48: six rounds
    (3, 16, 4097, 0, 0, 15.0, 'std'),
    (1, 16, 4100, 1, 1, NO_IGNORE, 'std'),
    (129, 2, 4100, 0, 1, NO_IGNORE, 'std'),            # N * nblk = 258: the second 256-stride of compound_column_sum
    (3, 3, 4096, 0, 0, NO_IGNORE, 'empty'),            # nothing counts at all
]
# the backward's second grid-stride trip: 8192 / N * N is smallest at N = 4097 (one workgroup per sample)
TRIP_N = BWD_MAX_GRID // 2 + 1
TRIP_SHAPES = [(TRIP_N, 1, BWD_THREADS * 4 + 4, 0, 0, NO_IGNORE, 'std'),       # 16-byte path: 4 211 716 voxels
               (TRIP_N, 2, BWD_THREADS + 1, 0, 0, NO_IGNORE, 'std')]           # scalar path: 1 052 929 voxels

GAMMAS = (0.0, 1.0, 2.0, 1.5, 0.5)
TERM_WEIGHTS = ((1.0, 1.0), (0.5, 2.0), (0.0, 1.0), (1.0, 0.0))                # (dice_weight, ce_weight)
K_PERCENTS = (0.01, 10.0, 50.0, 100.0)

COMPOUND_CASES = [Compound(*s, GAMMAS[i % 5], *TERM_WEIGHTS[i % 4]) for i, s in enumerate(SHAPES)] + \
                 [Compound(*TRIP_SHAPES[0], 2.0, 1.0, 1.0), Compound(*TRIP_SHAPES[1], 0.0, 0.5, 2.0)]
TOPK_TERM_WEIGHTS = ((1.0, 1.0), (0.0, 1.0), (0.5, 2.0), (1.0, 1.0), (1.0, 0.0))
# the histogram / sum passes' second trip: more than TOPK_MAX_GRID * 256 accesses, with an aligned and a misaligned ell
TOPK_HIST_TRIPS = [TopK(2, 2, TOPK_MAX_GRID * 256 * 2 + 8, 0, 0, NO_IGNORE, 'std', 10.0, 1.0, 1.0),
                   TopK(1, 2, TOPK_MAX_GRID * 256 + 8, 1, 0, NO_IGNORE, 'std', 50.0, 1.0, 1.0)]
TOPK_CASES = [TopK(*s, K_PERCENTS[i % 4], *TOPK_TERM_WEIGHTS[i % 5]) for i, s in enumerate(SHAPES)] + \
             [TopK(*TRIP_SHAPES[0], 10.0, 1.0, 1.0), TopK(*TRIP_SHAPES[1], 50.0, 0.5, 2.0)] + TOPK_HIST_TRIPS
TIE_CASE = TopK(1, 2, 200, 0, 0, NO_IGNORE, 'tie', 20.0, 1.0, 1.0)             # tests/test_topk_loss.py tie_fixture
BOUNDARY_CASES = [Boundary(*s, 0 if (s[1] >= 2 and i % 4 == 1) else 1, 0.0 if i % 5 == 2 else 1.0) for i, s in enumerate(SHAPES)] + \
                 [Boundary(*TRIP_SHAPES[0], 1, 1.0), Boundary(*TRIP_SHAPES[1], 0, 1.0)]

HEAD_C = (1, 2, 5, 7, 16)
HEAD_TRIP_S = (ITEMS_PER_TRIP + 78) // 2
HEAD_CASES = [Head(kind, 2 if C != 7 else 1, C, 1543 if C != 2 else 1) for kind in ('softmax', 'sigmoid') for C in HEAD_C] + \
             [Head(kind, 3, 2, 1001) for kind in ('softmax', 'sigmoid')] + \
             [Head(kind, 2, 2, HEAD_TRIP_S) for kind in ('softmax', 'sigmoid')]     # v / S crosses a sample on the second trip

CONF_SMALL = [(2, 1, 2052, 0), (1, 1, 2049, 0), (1, 1, 64, 1), (3, 2, 4096, 0), (2, 2, 1027, 0), (1, 2, 2048, 1),
              (2, 3, 4100, 0), (1, 3, 1, 0), (2, 3, 64, 1), (1, 4, 4096, 0), (3, 4, 1025, 0), (1, 4, 4100, 1),
              (2, 5, 4096, 0), (2, 5, 4097, 0), (1, 5, 64, 1), (2, 6, 4096, 0), (1, 6, 4099, 0), (2, 6, 2048, 1),
              (2, 16, 4096, 0), (1, 16, 4097, 0), (1, 16, 4096, 1)]
CONFUSION_CASES = [Confusion(N, C, S, shift, float(C - 1) if i % 4 == 2 and C > 1 else NO_IGNORE)
                   for i, (N, C, S, shift) in enumerate(CONF_SMALL)] + [
    Confusion(2, 2, (TOPK_MAX_GRID // 2) * CONF_THREADS * 4 + 4, 0, NO_IGNORE),      # 16-byte path, second trip
    Confusion(2, 2, (TOPK_MAX_GRID // 2) * CONF_THREADS + 3, 0, NO_IGNORE)]           # scalar path, second trip

# one refusal per entry, from its SEG3D_REQUIRE list
REFUSALS = {'seg3d_softmax_fwd': 'C = 17', 'seg3d_softmax_bwd': 'C = 17', 'seg3d_sigmoid_fwd': 'C = 17', 'seg3d_sigmoid_bwd': 'C = 17',
            'seg3d_compound_loss_fwd': 'both term weights 0', 'seg3d_compound_loss_bwd': 'gamma < 0',
            'seg3d_topk_loss_fwd': 'k_percent = 0', 'seg3d_topk_loss_bwd': 'C = 17',
            'seg3d_boundary_loss_fwd': 'C = 1 without the background', 'seg3d_boundary_loss_bwd': 'C = 1 without the background',
            'seg3d_confusion_counts': 'C = 17'}


TINY = 1e-30                          # per-element comparisons are relative to max(|ref|, TINY): below it float32 runs out of exponent


def per_element(x, ref):
    """|x - ref| / max(|ref|, TINY) per element, in float64"""
    return (x.double().reshape(ref.shape) - ref).abs() / ref.abs().clamp(min=TINY)


# ---- plans: what the host code of csrc/ decides for a case ---------------------------------------------------------------------------
def vec(c):
    """compound_vec_ok on the tests' buffers: 16-byte aligned before `shift` floats"""
    return c.S % 4 == 0 and c.shift % 4 == 0


def ct(C):
    """the compile-time class count COMPOUND_DISPATCH picks"""
    return C if C <= 5 else MAXC


def blocks(S):
    return (S + DICE_VPB - 1) // DICE_VPB


def part_floats(N, C, S):
    return N * blocks(S) * (3 * C + 2)


def coef_rows(c):
    return 1 if c.batch_dice else c.N


def finalize_plan(c):
    """(blocks, entries one region item walks, rounds of FIN_ITEMS items, a second step of the lanes, a second 256-stride of
    compound_column_sum over the N * nblk entries)"""
    nblk = blocks(c.S)
    cnt = c.N * nblk if c.batch_dice else nblk
    return nblk, cnt, (coef_rows(c) * c.C + FIN_ITEMS - 1) // FIN_ITEMS, cnt > FIN_LANES, c.N * nblk > COLUMN_THREADS


def bwd_plan(c):
    """(workgroups per sample, second trip) of compound_bwd_grid"""
    items = c.S // 4 if vec(c) else c.S
    gx, cap = (items + BWD_THREADS - 1) // BWD_THREADS, max(1, BWD_MAX_GRID // c.N)
    return min(gx, cap), gx > cap


def topk_hist_plan(c, cus=256):
    """(workgroups, 16-byte loads, second trip) of the histogram and sum passes over the N * S keys"""
    total = c.N * c.S
    nvec = total // 4 if c.shift % 4 == 0 else 0
    g, cap = ((nvec if nvec else total) + 255) // 256, min(2 * cus, TOPK_MAX_GRID)
    return min(g, cap), nvec > 0, g > cap


def topk_workspace_bytes(N, C, S):
    return TOPK_CTRL_BYTES + TOPK_HIST_BYTES + TOPK_SLOT_BYTES + 4 * part_floats(N, C, S)


def boundary_workspace_bytes(N, C, S):
    return 4 * (part_floats(N, C, S) + N * blocks(S) * (C + 1))


def confusion_plan(c, cus=256):
    items = c.S // 4 if vec(c) else c.S
    gx, cap = (items + CONF_THREADS - 1) // CONF_THREADS, max(1, (2 * cus + c.N - 1) // c.N)
    return min(gx, cap), gx > cap


def head_trip(c):
    return c.N * c.S > ITEMS_PER_TRIP


def device_count(n, k_percent):
    """max(1, (long long)((double)n * k_percent / 100.0)); 0 for n == 0"""
    return 0 if n == 0 else max(1, int(math.trunc(float(n) * float(k_percent) / 100.0)))


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
PT_VALUES = (0.0, 1e-30, 1e-12, 1.0, 0.5)            # the selected probability of the first voxels


def target_values(C):
    """the targets of the last voxels: outside [0, C); in-contract non-integers (classes 0, 1, C - 1, 0); -0.5 does not count,
    -0.0 counts with class 0"""
    return (-1.0, float(C), float(C + 3), 1000.0, 0.5, 1.7, C - 0.25, 0.3, -0.5, -0.0)


def safe_class(c):
    """a class that counts: 0, or 1 where 0 is the ignore label"""
    return 1 if c.ignore == 0.0 else 0


def quantised(c):
    """top-k cases above 20000 voxels take probabilities on the 2^-10 grid: their ell are equal or far apart (MARGIN)"""
    return isinstance(c, TopK) and c.N * c.S > 20000


def loss_inputs(c):
    """(p [N, C, S], t [N, S], wdice [C], alpha [C], gout) of a Compound, TopK or Boundary case: a soft-max of noise (C = 1: a
    sigmoid); on the first voxels the selected probability takes PT_VALUES; the last voxels take target_values(C); every 11th
    voxel the ignore label when that lies outside [0, C) (inside, the class itself is ignored); class 1 is absent from sample 0
    (N > 1), nothing counts in sample 1 (N > 2); fill 'empty': nothing counts at all; 'tie': the fixture of test_topk_loss"""
    N, C, S = c.N, c.C, c.S
    tag = 'compound/{}-{}-{}-{}'.format(N, C, S, c.fill)
    if c.fill == 'tie':
        from test_topk_loss import tie_fixture
        p, t = tie_fixture()
        return p.reshape(1, 2, 200).contiguous(), t.reshape(1, 200).contiguous(), torch.tensor([0.5, 0.5]), torch.ones(2), 1.0
    x = _noise(3000, tag + '/x', (N, C, S)) * 3.0
    p = torch.softmax(x, 1) if C > 1 else torch.sigmoid(x)
    if quantised(c):
        p = (torch.round(p * 1024.0) / 1024.0).clamp(min=1.0 / 1024.0)
    below_one = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))
    if 0.0 < getattr(c, 'gamma', 0.0) < 1.0:
        p = p.clamp(max=below_one)
    t = _labels(3001, tag + '/t', (N, S), C)
    total, tf = N * S, t.reshape(-1)
    if c.ignore < 0.0 or c.ignore >= C:
        tf[5::11] = c.ignore
    if N > 1 and C > 1:
        t[0][t[0] == 1.0] = 0.0
    if N > 2:
        t[1] = -1.0
    if c.fill == 'empty':
        tf[0::2], tf[1::2] = float(C), c.ignore
    elif total >= 32:
        for v, val in enumerate(PT_VALUES):
            tf[v] = float(safe_class(c))
            if val == 1.0 and 0.0 < getattr(c, 'gamma', 0.0) < 1.0:
                val = below_one
            p[v // S, safe_class(c), v % S] = val
        for i, val in enumerate(target_values(C)):
            tf[total - 1 - i] = val
            if 0.0 < val < C and val != int(val):        # in-contract non-integers: a small p_t, so a large ell (inside the top k)
                p[(total - 1 - i) // S, int(val), (total - 1 - i) % S] = 0.03125 * (1 + i % 4)
    else:
        tf[0] = float(safe_class(c))
    wdice = 0.2 + _uniform(3002, tag + '/w', C)
    wdice = wdice / wdice.sum()
    if C > 1 and (N % 2 == 0 or not getattr(c, 'include_background', 1)):
        wdice[0] = 0.0                                   # an excluded background; the rest no longer sums to 1 (unnormalised)
    alpha = 0.1 + _uniform(3003, tag + '/a', C)          # unnormalised
    if C > 2:
        alpha[C - 1] = 0.0
    return p, t, wdice, alpha, (-2.5 if (N + C) % 2 else 1.5)


def phi_input(c, t):
    """[N, C - c0, S] noise in place of a distance map, with a distance map's signs: negative on the plane of the voxel's own class,
    positive on the others -- so (A t_c + B) and coef_c phi_c never cancel and the gradient can be compared per element.  Voxels
    that do not count keep their noise (the kernels gate them)"""
    c0 = 0 if c.include_background else 1
    phi = (_noise(3004, 'compound/phi-{}-{}-{}'.format(c.N, c.C, c.S), (c.N, c.C - c0, c.S)) * 3.0).abs()
    _, cls = counting(t, c.C, c.ignore)
    own = cls.unsqueeze(1) == torch.arange(c0, c.C).view(1, -1, 1)
    return torch.where(own, -phi, phi)


def head_inputs(c):
    """(x [N, S, C] logits, dprobs [N, C, S] dense noise): rows of equal values, one logit of +1e4 or -1e4 (probabilities of exactly
    0 and 1), rows of zeros, rows thirty times as wide"""
    N, C, S = c.N, c.C, c.S
    tag = 'compound/{}-{}-{}-{}'.format(c.kind, N, C, S)
    x = _noise(3010, tag + '/x', (N, S, C)) * 3.0
    xf = x.reshape(N * S, C)
    xf[4::5] = 2.5
    xf[6::7, C // 2] = 1e4
    xf[10::11, 0] = -1e4
    xf[12::13] = 0.0
    xf[16::17] *= 30.0                                    # differences near 100: exp underflows in float32 only
    d = _noise(3011, tag + '/d', (N, C, S))
    return x, d


def sparse_dprobs(p, d):
    """d kept on the plane of the smallest probability of every voxel (the first such plane), zero elsewhere: like the gradient of
    a cross-entropy, one plane per voxel, and p_c (d_c - sum p d) has no cancellation there"""
    idx = p.argmin(1, keepdim=True)
    return torch.zeros_like(d).scatter_(1, idx, d.gather(1, idx))


def confusion_inputs(c):
    """(p [N, C, S], t [N, S], counts0 [3 C] int64): every 5th voxel two classes share the maximum, every 9th all classes are
    equal; targets as in loss_inputs; the counters start from non-zero values"""
    N, C, S = c.N, c.C, c.S
    tag = 'compound/conf-{}-{}-{}'.format(N, C, S)
    x = _noise(3020, tag + '/x', (N, C, S)) * 2.0
    p = torch.softmax(x, 1) if C > 1 else torch.sigmoid(x)
    pf = p.permute(1, 0, 2).reshape(C, N * S)            # a copy for N > 1: written back below
    if C > 1:
        pf[(C - 1) // 2, 4::5] = 0.9375
        pf[C - 1, 4::5] = 0.9375
    pf[:, 8::9] = 0.25
    p = pf.reshape(C, N, S).permute(1, 0, 2).contiguous()
    t = _labels(3021, tag + '/t', (N, S), C)
    tf, total = t.reshape(-1), N * S
    if c.ignore >= C:
        tf[5::11] = c.ignore
    if total >= 32:
        for i, val in enumerate(target_values(C)):
            tf[total - 1 - i] = val
    counts0 = torch.arange(3 * C, dtype=torch.int64) * 7 + 3
    return p, t, counts0


# ---- references --------------------------------------------------------------------------------------------------------------------
def counting(t, C, ignore):
    """(valid [N, S] bool, cls [N, S] int64 -- 0 where the voxel does not count), decided on the float32 target"""
    valid = (t >= 0.0) & (t < float(C)) & (t != torch.tensor(ignore, dtype=torch.float32))
    return valid, torch.where(valid, torch.trunc(t), torch.zeros_like(t)).long()


def region_ref(p, valid, cls, wdice, dice_weight, batch_dice, dtype):
    """L_region, A [R, C], B [R, C], onehot [N, C, S] (carries valid)
      I = sum p_c t_c, U = sum p_c + sum t_c + 1e-5 over counted voxels (batch_dice: over n as well), nu = 2 I + 1e-5, k = 1 / N or 1
      L_region = sum_{r, c} w_c k (1 - nu / U);  A = -dice_weight w k 2 / U,  B = dice_weight w k nu / U^2 (0 for w = 0 or weight 0)"""
    N, C, S = p.shape
    P, v = p.to(dtype), valid.to(dtype)
    onehot = torch.zeros((N, C, S), dtype=dtype).scatter_(1, cls.unsqueeze(1), v.unsqueeze(1))
    I, Ps, T = (P * onehot).sum(2), (P * v.unsqueeze(1)).sum(2), onehot.sum(2)
    if batch_dice:
        I, Ps, T = I.sum(0, keepdim=True), Ps.sum(0, keepdim=True), T.sum(0, keepdim=True)
    k = 1.0 if batch_dice else 1.0 / N
    U, nu, w = Ps + T + EPS, 2.0 * I + EPS, wdice.to(dtype).unsqueeze(0)
    l_region = (w * k * (1.0 - nu / U)).sum()
    on = (w > 0) & (dice_weight > 0.0)
    zero = torch.zeros((), dtype=dtype)
    A = torch.where(on, -dice_weight * w * k * 2.0 / U, zero)
    B = torch.where(on, dice_weight * w * k * nu / (U * U), zero)
    return l_region, A, B, onehot


def _selected(p, cls):
    """the float32 probability of every voxel's class, its clamp, and the gate of the gradient"""
    p_t = p.gather(1, cls.unsqueeze(1)).squeeze(1)
    return p_t, torch.maximum(p_t, PMIN), p_t >= PMIN


def _total(dtype, *terms):
    """sum of weight * term over the terms whose weight is > 0"""
    out = torch.zeros((), dtype=dtype)
    for weight, term in terms:
        if weight > 0.0:
            out = out + weight * term
    return out


def compound_ref(p, t, wdice, alpha, c, gout, dtype):
    """-> dict(loss [3] = (L, L_region, L_dist), coef [2 R C + 1], dprobs [N, C, S], valid, cls, onehot)
      L_dist = sum a_t (1 - pt)^gamma (-log pt) / sum a_t over counted voxels, pt = max(p_t, 1e-12); 0 when nothing counts
      dL/dp[n, c, s] = gout v ((A t_c + B) + [c == t] coef_dist a_t (gamma q^(gamma - 1) log pt - q^gamma / pt) [p_t >= 1e-12]),
      q = 1 - pt, coef_dist = ce_weight / sum a_t (0 when the term is off or empty)"""
    C, gamma = p.shape[1], c.gamma
    valid, cls = counting(t, C, c.ignore)
    lr, A, B, onehot = region_ref(p, valid, cls, wdice, c.dice_weight, c.batch_dice, dtype)
    _, pt32, gate = _selected(p, cls)
    pt, v = pt32.to(dtype), valid.to(dtype)
    a = alpha.to(dtype)[cls] * v
    q, lp = (1.0 - pt).clamp(min=0.0), torch.log(pt)
    if gamma == 0.0:
        dist, dg = -lp, -1.0 / pt
    else:
        qg1 = q if gamma == 2.0 else (torch.ones_like(q) if gamma == 1.0 else torch.where(q > 0, q ** (gamma - 1.0), torch.zeros_like(q)))
        dist, dg = q ** gamma * -lp, gamma * qg1 * lp - q ** gamma / pt
    num, den = (a * dist).sum(), a.sum()
    ld = num / den if float(den) > 0.0 else num * 0.0
    coef_dist = c.ce_weight / den if (c.ce_weight > 0.0 and float(den) > 0.0) else den * 0.0
    dt = torch.where(gate, coef_dist * a * dg, torch.zeros_like(a))
    d = gout * (v.unsqueeze(1) * (A.unsqueeze(2) * onehot + B.unsqueeze(2)) + onehot * dt.unsqueeze(1))
    loss = torch.stack([_total(dtype, (c.dice_weight, lr), (c.ce_weight, ld)), lr, ld])
    coef = torch.cat([torch.stack([A, B], 2).reshape(-1), coef_dist.reshape(1)])
    return {'loss': loss, 'coef': coef, 'dprobs': d, 'valid': valid, 'cls': cls, 'onehot': onehot}


def topk_ref(p, t, wdice, alpha, c, gout, dtype):
    """-> dict(loss [3] = (L, L_region, L_topk), coef [2 R C + 3], ell [N, S] (-1 where the voxel does not count), selection =
    (n, k, m, n_eq, r), tau, dprobs, valid, cls, onehot, margin = (below, above): the relative gaps of the values next to tau, 0.0
    for a neighbour equal to tau, inf where there is none)
      ell = a_t (-log max(p_t, 1e-12)), -0.0 as +0.0;  k = device_count(n);  tau = the k-th largest, m = #{ell > tau}, r = k - m
      L_topk = (sum_{ell > tau} ell + r tau) / k;  dL/dp_t = gout ce_weight w_v / k (p_t >= 1e-12 ? -a_t / p_t : 0),
      w_v = 1 above tau, r / n_eq at tau, 0 below -- decided on ell rounded to float32"""
    C = p.shape[1]
    valid, cls = counting(t, C, c.ignore)
    lr, A, B, onehot = region_ref(p, valid, cls, wdice, c.dice_weight, c.batch_dice, dtype)
    p_t, pt32, gate = _selected(p, cls)
    v = valid.to(dtype)
    a = alpha.to(dtype)[cls]
    ell = a * -torch.log(pt32.to(dtype))
    ell = torch.where(ell > 0, ell, torch.zeros_like(ell))
    vals = ell[valid]
    n = int(vals.numel())
    k = device_count(n, c.k_percent)
    tau, m, n_eq, r, margin = torch.zeros((), dtype=dtype), 0, 0, 0, (float('inf'), float('inf'))
    W = torch.zeros_like(ell)
    if n > 0:
        srt = torch.sort(vals, descending=True).values
        tau = srt[k - 1]
        e32, tau32 = ell.float(), tau.float()
        above, at = valid & (e32 > tau32), valid & (e32 == tau32)
        m, n_eq = int(above.sum()), int(at.sum())
        r = k - m
        W = above.to(dtype) + at.to(dtype) * (float(r) / float(n_eq)) if n_eq else W
        gap = lambda x: abs(float(x) - float(tau)) / float(tau) if float(tau) > 0.0 else 0.0
        m64 = int((vals > tau).sum())
        margin = (gap(srt[k]) if k < n else float('inf'), gap(srt[m64 - 1]) if m64 > 0 else float('inf'))
    lt = (W * ell).sum() / k if k > 0 else ell.sum() * 0.0
    on = c.ce_weight > 0.0 and k > 0 and n_eq > 0
    c_above = c.ce_weight / k if on else 0.0
    c_at = c.ce_weight * (float(r) / float(n_eq)) / k if on else 0.0
    zero = torch.zeros_like(ell)
    dt = torch.where(gate & valid, (c.ce_weight / k if on else 0.0) * W * -a / p_t.to(dtype).clamp(min=1e-30), zero)
    d = gout * (v.unsqueeze(1) * (A.unsqueeze(2) * onehot + B.unsqueeze(2)) + onehot * dt.unsqueeze(1))
    loss = torch.stack([_total(dtype, (c.dice_weight, lr), (c.ce_weight, lt)), lr, lt])
    coef = torch.cat([torch.stack([A, B], 2).reshape(-1), torch.stack([tau, torch.tensor(c_above, dtype=dtype), torch.tensor(c_at, dtype=dtype)])])
    return {'loss': loss, 'coef': coef, 'ell': torch.where(valid, ell, -torch.ones_like(ell)), 'selection': (n, k, m, n_eq, r),
            'tau': tau, 'dprobs': d, 'valid': valid, 'cls': cls, 'onehot': onehot, 'margin': margin}


def boundary_ref(p, t, phi, wdice, c, gout, dtype):
    """-> dict(loss [3] = (L, L_region, L_boundary), coef [2 R C + C], dprobs, valid, cls, onehot)
      L_boundary = sum_{c >= c0} w_c sum_{counted} phi_c p_c / max(1, n_counted);  L = dice_weight L_region + boundary_weight L_boundary
      coef_c = boundary_weight w_c / max(1, n_counted);  dL/dp = gout v ((A t_c + B) + coef_c phi_c [c >= c0])"""
    N, C, S = p.shape
    c0 = 0 if c.include_background else 1
    valid, cls = counting(t, C, c.ignore)
    lr, A, B, onehot = region_ref(p, valid, cls, wdice, c.dice_weight, c.batch_dice, dtype)
    v, w = valid.to(dtype), wdice.to(dtype)
    ncnt = max(1.0, float(valid.sum()))
    PHI = torch.zeros((N, C, S), dtype=dtype)
    PHI[:, c0:] = phi.to(dtype)
    tot = (PHI * p.to(dtype) * v.unsqueeze(1)).sum((0, 2))
    lb = (w * tot).sum() / ncnt
    cb = BOUNDARY_WEIGHT * w / ncnt
    cb_used = cb.clone()
    cb_used[:c0] = 0.0
    d = gout * v.unsqueeze(1) * (A.unsqueeze(2) * onehot + B.unsqueeze(2) + cb_used.view(1, C, 1) * PHI)
    loss = torch.stack([BOUNDARY_WEIGHT * lb + _total(dtype, (c.dice_weight, lr)), lr, lb])
    return {'loss': loss, 'coef': torch.cat([torch.stack([A, B], 2).reshape(-1), cb]), 'dprobs': d, 'valid': valid, 'cls': cls,
            'onehot': onehot}


def head_fwd_ref(kind, x, dtype):
    """x [N, S, C] -> probs [N, C, S]: softmax_c with the maximum subtracted, or 1 / (1 + exp(-x)) through exp(-|x|)"""
    X = x.to(dtype)
    if kind == 'softmax':
        e = torch.exp(X - X.max(2, keepdim=True).values)
        p = e / e.sum(2, keepdim=True)
    else:
        e = torch.exp(-X.abs())
        p = torch.where(X >= 0, torch.ones_like(e), e) / (1.0 + e)
    return p.permute(0, 2, 1).contiguous()


def head_bwd_ref(kind, p, d, dtype):
    """probs, dprobs [N, C, S] float32 -> din [N, S, C]: p_c (d_c - sum_k p_k d_k), or d p (1 - p)"""
    P, D = p.to(dtype), d.to(dtype)
    g = P * (D - (P * D).sum(1, keepdim=True)) if kind == 'softmax' else D * P * (1.0 - P)
    return g.permute(0, 2, 1).contiguous()


def confusion_ref(p, t, ignore):
    """[C, 3] int64 = (tp, fp, fn): pred is the first maximum, a voxel counts by the counting rule"""
    N, C, S = p.shape
    valid, cls = counting(t, C, ignore)
    best, pred = p[:, 0].clone(), torch.zeros((N, S), dtype=torch.int64)
    for k in range(1, C):
        up = p[:, k] > best
        best, pred = torch.where(up, p[:, k], best), torch.where(up, torch.full_like(pred, k), pred)
    out = torch.zeros((C, 3), dtype=torch.int64)
    for k in range(C):
        P_, G_ = valid & (pred == k), valid & (cls == k)
        out[k] = torch.tensor([int((P_ & G_).sum()), int((P_ & ~G_).sum()), int((~P_ & G_).sum())])
    return out
