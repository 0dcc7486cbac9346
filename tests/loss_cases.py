"""The case tables, the inputs and the float64 references of the reference project's own losses (seg3d_dice_*, seg3d_binary_dice_*,
seg3d_focal_* of csrc/loss.hip) and of the layout bridges (seg3d_ncdhw_to_ndhwc, seg3d_ndhwc_to_ncdhw, seg3d_copy_channels of
csrc/layout.hip), shared by tests/test_loss_cases.py (host only: the references reproduce the reference project's recorded results,
every case has the property it is named for) and tests/test_gpu_loss_float64.py / tests/test_gpu_layout_bits.py (the same cases on
the device).

The references are plain torch, written from the formulas in the kernel and header comments; each takes a `dtype`: float64 is the
reference, the same code in float32 on the CPU is the yardstick of the device tests.  What stays float32 in BOTH evaluations is what
the operation itself defines on float32 values:
  Dice         the gate p > float32(1 / C), compared on the float32 probabilities (ties are not above the gate)
  binary Dice  the gate p1 > p0
  focal        class k = trunc(t); pt = float32(p_k) + float32(1e-10), rounded ONCE in float32 (the reference module adds 1e-10 to a
               float32 tensor): without that rounding 1 - pt differs by up to 100 % where p_k rounds to 1 and is negative at p_k = 1
Outside the tables: focal with p_k == 1 and 0 < gamma < 1 -- the formula's own derivative is inf * 0 there (q^(gamma - 1) log pt at
q = 0); focal_inputs keeps every probability of such a case below 1.

Constants restated from csrc/ (tests/test_loss_cases.py holds them against the library's queries): DICE_VPB voxels per workgroup of
the Dice partial pass; the finalize walks the blocks of one (n, c) pair with FIN_LANES lanes and FIN_PAIRS pairs per round; the focal
forward gives FOCAL_VPB voxels to a workgroup; seg3d_ew_grid caps an element-wise grid at ITEMS_PER_TRIP threads.
"""
from collections import namedtuple

import torch

from float64_util import _noise
from oracle import detgen

DICE_VPB, FIN_LANES, FIN_PAIRS, FOCAL_VPB, MAXC = 4096, 32, 8, 2048, 16
ITEMS_PER_TRIP = 8192 * 256
BIG = ITEMS_PER_TRIP + 77            # voxels of a case whose element-wise backward takes a second grid-stride trip
EPS = 1e-6

Dice = namedtuple('Dice', 'N C S')
BDice = namedtuple('BDice', 'N S')
Focal = namedtuple('Focal', 'layout N C S gamma size_average')
Layout = namedtuple('Layout', 'N C S')
Copy = namedtuple('Copy', 'nvox C src_ld src_off dst_ld dst_off in_place shift')


def case_id(c):
    return type(c).__name__.lower() + '-' + '-'.join(str(v) for v in c)


# ---- tables ------------------------------------------------------------------------------------------------------------------------
DICE_CASES = [
    Dice(1, 1, 1),                    # the smallest call
    Dice(4, 2, 4095),                 # one finalize round, exactly full; one voxel short of a block
    Dice(3, 3, 4096),                 # nine pairs: a second round with one pair; exactly one block
    Dice(2, 16, 4097),                # SEG3D_MAXC, a second block of one voxel, four rounds
    Dice(3, 5, 33 * DICE_VPB + 5),    # 34 blocks: lanes 0 and 1 take the second strided step, the last block is partial
    Dice(1, 2, BIG),                  # the backward's second grid-stride trip
]
ABSENT = (1, 3)                       # (sample, class) of the C = 5 case: no such target, every probability below the gate

BDICE_CASES = [BDice(1, 1), BDice(3, 4096), BDice(9, 4097), BDice(2, 33 * DICE_VPB + 5)]

GAMMAS, FOCAL_C, FOCAL_TOTALS = (0.0, 1.0, 2.0, 1.5, 0.5), (2, 5, 16), (1, 2047, 2048, 2049, 70001)


def _planar_n(total):
    """samples of a planar focal case of `total` voxels: more than one wherever `total` has a small divisor"""
    for n in (3, 2, 23):
        if total % n == 0:
            return n
    return 1


def _focal_cases():
    cases = []
    for li, layout in enumerate(('planar', 'matrix')):
        for ci, C in enumerate(FOCAL_C):
            for ti, total in enumerate(FOCAL_TOTALS):
                # gamma and size_average rotate over the shapes (and differently in the two layouts) instead of the full product
                gamma, avg = GAMMAS[(ti + ci + 2 * li) % 5], (ci * 5 + ti + li) % 2
                N = _planar_n(total) if layout == 'planar' else 1
                cases.append(Focal(layout, N, C, total // N, gamma, avg))
    cases.append(Focal('planar', 1, 2, BIG, 2.0, 1))
    return cases


FOCAL_CASES = _focal_cases()

LAYOUT_CASES = [Layout(1, 1, 1), Layout(3, 16, 257), Layout(2, 33, 100), Layout(1, 2, BIG)]

COPY_VEC = (8, 24, 12, 20, 4)        # (C, src_ld, src_off, dst_ld, dst_off): every number a multiple of 4
# each breaks ONE of the five conditions of the 16-byte path and keeps the other four
COPY_BROKEN = {'C': (6, 24, 12, 20, 4), 'src_ld': (8, 22, 12, 20, 4), 'src_off': (8, 24, 13, 20, 4), 'dst_ld': (8, 24, 12, 18, 4),
               'dst_off': (8, 24, 12, 20, 5)}
COPY_CASES = [Copy(nvox, *tab, False, 0) for tab in [COPY_VEC] + list(COPY_BROKEN.values()) for nvox in (1, 255, 257)] + [
    Copy(131075, 64, 128, 0, 128, 64, True, 0),      # 16-byte path, second trip; channels [0, 64) onto [64, 128) of the same rows
    Copy(699053, 3, 3, 0, 5, 1, False, 0),           # scalar path, second trip
    Copy(257, *COPY_VEC, False, 1),                  # both bases one float past a 16-byte boundary: the scalar path
]
# (nvox, C, src_ld, src_off, dst_ld, dst_off) the entry refuses
COPY_REFUSALS = [((16, 8, 12, 8, 16, 0), 'src_off + C > src_ld'), ((16, 8, 16, 0, 12, 8), 'dst_off + C > dst_ld'),
                 ((16, 0, 8, 0, 8, 0), 'C = 0')]


def copy_vec(c):
    """whether the case takes the 16-byte path (both bases of the tests' buffers are 16-byte aligned before `shift` floats)"""
    return all(v % 4 == 0 for v in (c.C, c.src_ld, c.src_off, c.dst_ld, c.dst_off)) and c.shift % 4 == 0


def copy_items(c):
    return c.nvox * (c.C // 4 if copy_vec(c) else c.C)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _labels(seed, tag, shape, C):
    """float32 class ids in [0, C), from the generator of float64_util._noise"""
    return torch.floor(_noise(seed, tag, shape).abs() * 997.0) % C


def _uniform(seed, tag, n):
    return torch.from_numpy(detgen.uniform(seed, tag, (n,))).float()


def dice_thr(C):
    return torch.tensor(1.0 / C, dtype=torch.float32)


def gate_voxel(S, C, cls, j):
    """voxel of sample 0 whose class-`cls` probability is set to the gate value j (0: thr, 1: the float above, 2: the float below);
    spread over the blocks.  A sample too short for all of them (S = 1) takes the value above the gate alone"""
    if S >= 3 * C + 8:
        return (3 * cls + j) * ((S - 8) // (3 * C))
    return 0 if (cls, j) == (0, 1) else None


def dice_inputs(c):
    """(p [N, C, S], t [N, S], w [C], gout): softmax probabilities; in sample 0, per class, one voxel AT the gate, one a float above
    and one a float below, one of the three with t == c (so the gate decides a term of I); the targets -1, C and 0.5 on the last
    voxels of the last sample; in the C = 5 case class ABSENT[1] is absent from sample ABSENT[0] and below the gate there"""
    N, C, S = c
    tag = 'loss/' + case_id(c)
    p = torch.softmax(_noise(2000, tag + '/x', (N, C, S)) * 2.0, 1)
    t = _labels(2001, tag + '/t', (N, S), C)
    thr = dice_thr(C)
    vals = (thr, torch.nextafter(thr, torch.tensor(2.0)), torch.nextafter(thr, torch.tensor(0.0)))     # (C = 1: thr is 1.0)
    for cls in range(C):
        for j in range(3):
            v = gate_voxel(S, C, cls, j)
            if v is not None:
                p[0, cls, v] = vals[j]
                if j == cls % 3 or S < 3 * C + 8:
                    t[0, v] = float(cls)
    if S >= 8:
        t[N - 1, S - 1], t[N - 1, S - 2], t[N - 1, S - 3] = -1.0, float(C), 0.5
    if C == 5:
        n, cls = ABSENT
        t[n][t[n] == float(cls)] = float(cls + 1)
        p[n, cls] = p[n, cls].clamp(max=float(thr) * 0.5)
    w = 0.2 + _uniform(2002, tag + '/w', C)
    w[0] = 0.0
    return p, t, w, -2.5


def bdice_inputs(c):
    """(p [N, 2, S], t [N, S], gout): p1 == p0 on every seventh voxel; float targets in {0, 1} with 0.3 and 2.0 among them"""
    N, S = c
    tag = 'loss/' + case_id(c)
    p = torch.softmax(_noise(2010, tag + '/x', (N, 2, S)) * 2.0, 1)
    t = _labels(2011, tag + '/t', (N, S), 2)
    p[:, 1, 3::7] = p[:, 0, 3::7]
    t[:, 1::11] = 0.3
    t[:, 2::13] = 2.0
    if S == 1:
        p[0, :, 0] = torch.tensor([0.25, 0.75])
        t[0, 0] = 2.0
    return p, t, 0.75


FOCAL_PROBS = (1e-12, 0.0, 1e-30, 0.5)                      # the selected probability of the first voxels


def FOCAL_TARGETS(C):
    """the targets of the last voxels: three outside [0, C), then trunc -> class 1 and class 0"""
    return (-1.0, float(C), float(C + 3), 1.7, -0.5)


def focal_inputs(c):
    """(p [N, C, S] -- the LOGICAL tensor, whatever the layout --, t [N, S], alpha [C], gout)"""
    N, C, S = c.N, c.C, c.S
    tag = 'loss/' + case_id(c)
    p = torch.softmax(_noise(2020, tag + '/x', (N, C, S)) * 3.0, 1)
    if 0.0 < c.gamma < 1.0:
        p = p.clamp(max=float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0))))       # (module docstring)
    t = _labels(2021, tag + '/t', (N, S), C)
    total = N * S
    tf = t.reshape(total)                                                                   # a view: voxel v = n S + s
    for v, val in enumerate(FOCAL_PROBS):
        if v < total:
            p[v // S, int(tf[v]), v % S] = val
    if total >= 16:
        for i, val in enumerate(FOCAL_TARGETS(C)):
            tf[total - 1 - i] = val
    alpha = 0.1 + _uniform(2022, tag + '/a', C)
    alpha[C - 1] = 0.0
    return p, t, alpha, 1.5


# ---- references --------------------------------------------------------------------------------------------------------------------
def dice_ref(p, t, w, gout, dtype):
    """p [N, C, S] float32, t [N, S] float32, w [C] -> loss, sums [N, C, 2] = (I, den), dprobs [N, C, S], l [N, C]
      phat = p [p > float32(1 / C)],  t_c = [t == c],  I = sum phat t_c,  den = sum phat^2 + sum t_c,
      l = 1 - (2 I + 1e-6) / (den + 1e-6),  L = sum_c w_c mean_n l
      dL/dp = gout w_c / N [p > thr] * -(2 t_c (den + eps) - (2 I + eps) 2 p) / (den + eps)^2"""
    N, C, S = p.shape
    gate = p > dice_thr(C)
    tc = (t.unsqueeze(1) == torch.arange(C, dtype=torch.float32).view(1, C, 1)).to(dtype)
    p = p.to(dtype)
    ph = p * gate
    I = (ph * tc).sum(2)
    den = (ph * ph).sum(2) + tc.sum(2)
    l = 1.0 - (2.0 * I + EPS) / (den + EPS)
    w = w.to(dtype)
    loss = (w * l.mean(0)).sum()
    de, num = (den + EPS).unsqueeze(2), (2.0 * I + EPS).unsqueeze(2)
    d = -(2.0 * tc * de - num * 2.0 * p) / (de * de) * gate * (gout * w / N).view(1, C, 1)
    return loss, torch.stack([I, den], 2), d, l


def bdice_ref(p, t, gout, dtype):
    """p [N, 2, S] float32, t [N, S] float32 -> loss, sums [N, 2] = (I, den), dprobs [N, 2, S]
      pred = p1 [p1 > p0],  I = sum pred t,  den = sum pred^2 + sum t^2,  L = mean_n 1 - (2 I + 1e-6) / (den + 1e-6);
      the gradient is on plane 1, where p1 > p0"""
    N = p.shape[0]
    gate = p[:, 1] > p[:, 0]
    p1, t = p[:, 1].to(dtype), t.to(dtype)
    pred = p1 * gate
    I = (pred * t).sum(1)
    den = (pred * pred).sum(1) + (t * t).sum(1)
    loss = (1.0 - (2.0 * I + EPS) / (den + EPS)).mean()
    de, num = (den + EPS).unsqueeze(1), (2.0 * I + EPS).unsqueeze(1)
    d1 = -(2.0 * t * de - num * 2.0 * p1) / (de * de) * gate * (gout / N)
    return loss, torch.stack([I, den], 1), torch.stack([torch.zeros_like(d1), d1], 1)


def focal_ref(p, t, alpha, gamma, size_average, gout, dtype):
    """p [N, C, S] float32, t [N, S] float32, alpha [C] -> loss, dprobs [N, C, S], selected [N, C, S] (bool: plane k of a valid voxel)
      k = trunc(t), valid iff 0 <= k < C;  pt = float32(p_k + 1e-10);  l = -alpha_k (1 - pt)^gamma log pt  (gamma = 0: no power)
      L = sum l * (size_average ? 1 / (N S) : 1)
      dL/dp_k = gout scale alpha_k (gamma q^(gamma - 1) log pt - q^gamma / pt), q = 1 - pt  (gamma = 0: -alpha_k / pt); 0 elsewhere"""
    N, C, S = p.shape
    k = torch.trunc(t).long()
    valid = (k >= 0) & (k < C)
    kk = k.clamp(0, C - 1).unsqueeze(1)
    pt = (p.gather(1, kk).squeeze(1) + torch.tensor(1e-10, dtype=torch.float32)).to(dtype)
    a = alpha.to(dtype)[kk.squeeze(1)]
    q, lp = 1.0 - pt, torch.log(pt)
    scale = 1.0 / (N * S) if size_average else 1.0
    if gamma > 0.0:
        l = -a * q ** gamma * lp
        dt = a * (gamma * q ** (gamma - 1.0) * lp - q ** gamma / pt)
    else:
        l = -a * lp
        dt = -a / pt
    zero = torch.zeros((), dtype=dtype)
    loss = torch.where(valid, l, zero).sum() * scale
    dt = torch.where(valid, dt * (gout * scale), zero)
    sel = torch.zeros((N, C, S), dtype=torch.bool).scatter_(1, kk, valid.unsqueeze(1))
    d = torch.zeros((N, C, S), dtype=dtype).scatter_(1, kk, dt.unsqueeze(1))
    return loss, d, sel
