"""The case tables, the inputs and the selection-rule reference of the soft skeleton and the Dice + clDice loss (the eight kernels of
csrc/cldice_loss.hip).  Shared by tests/test_cldice_cases.py (host only: every case has the tile count, block count and instantiation
it is named for, the reference agrees with tests/cldice_oracle.py where that oracle is defined, the float32 and the float64 evaluation
take the same selections and gates on every case) and tests/test_gpu_cldice_float64.py (the same cases on the device, through the C
ABI).

The reference is plain torch without autograd, written from the header text of include/seg3d_hip.h; it takes a `dtype`: float64 is the
reference, the same code in float32 on the CPU the yardstick of the device test.
  E(x)(v)  the FIRST minimum over the 7 positions (-z, -y, -x, centre, +x, +y, +z), +inf outside the volume
  D(x)(v)  the FIRST maximum over the 27 positions in (z, y, x) order, -inf outside the volume
  stage j  keeps the linear index E took and the one D took per voxel, and a_j = ds_j / dz_j, b_j = ds_j / ds_{j-1}:
           stage 0: a = [d > 0], b = 0;  later: u = d - s d, a = u > 0 ? 1 - s : 0, b = u > 0 ? 1 - d : 1   (relu' is 1 for a positive argument)
  backward, stage k..0:  gz = gs a;  gE = dL/dx_{j+1}, gE[selD(v)] -= gz(v);  gx = gz, gx[selE(u)] += gE(u);  gs <- gs b
tests/cldice_oracle.py differentiates max_pool3d instead, which sends the gradient of a tied window elsewhere: the two agree on
pairwise-distinct planes only (test_cldice_cases.py holds them together there), so that oracle cannot see the selection rule.
What stays float32 in BOTH evaluations: the counting rule and the class (int)t of compound_cases.counting, decided on the float32 target.

Value classes of a plane: 'ranked' -- a permutation of (1..S) / (S + 1), pairwise distinct; 'mask' -- 0 / 1; 'dyadic' -- multiples of
1/8 per voxel; 'plateau' -- multiples of 1/8 constant on every other 3 x 3 x 4 brick (per voxel between them) with a slab of exact ones
and a slab of exact zeros: ties in every window, as saturated probabilities give them.  On the last two every float32 operation of
the forward is exact.

Constants restated from csrc/cldice_loss.hip: a workgroup owns a TX x TY x TZ tile; MAX_AXIS, MAX_ITERS; the sums kernel walks DICE_VPB
voxels per workgroup; CldLayout (layout()) in floats, every offset rounded up to a multiple of 4.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

import compound_cases as K
from float64_util import _noise
from loss_cases import DICE_VPB, MAXC, _labels, _uniform

TX, TY, TZ = 32, 8, 8
MAX_AXIS, MAX_ITERS = 256, 16
NO_IGNORE = K.NO_IGNORE
DYADIC_MAX_ITERS = 10                 # multiples of 1/8: the forward stays exact in float32 up to here (test_cldice_cases.py)

Skel = namedtuple('Skel', 'Z Y X planes iters fill')
Loss = namedtuple('Loss', 'N C Z Y X classes iters dice_weight cldice_weight batch_dice ignore fill')


def case_id(c):
    return type(c).__name__.lower() + '-' + '-'.join('.'.join(str(i) for i in v) if isinstance(v, tuple) else str(v) for v in c)


# ---- tables ------------------------------------------------------------------------------------------------------------------------
SKEL_SHAPES = [(1, 1, 1, 2), (1, 1, 32, 2), (1, 1, 33, 2),      # one voxel, a full row, one past it
               (8, 8, 32, 2),                                  # exactly one full tile
               (9, 9, 33, 2),                                  # one voxel into a second tile on every axis
               (17, 17, 65, 2),                                # three tiles per axis: an interior tile with both neighbours
               (2, 3, 256, 2), (256, 1, 2, 2), (1, 256, 3, 2),  # the axis limit
               (2, 3, 5, 600)]                                 # grid.y
ITERS = (1, 3, 16)
SKEL_FILLS = ('ranked', 'mask', 'dyadic', 'plateau')


def _skel_iters(i, fill):
    it = ITERS[i % 3]
    return min(it, DYADIC_MAX_ITERS) if fill in ('dyadic', 'plateau') else it


SKEL_CASES = [Skel(Z, Y, X, planes, _skel_iters(i + f, fill), fill)
              for i, (Z, Y, X, planes) in enumerate(SKEL_SHAPES) for f, fill in enumerate(SKEL_FILLS)]

BIG, MID, SMALL, ROW = (18, 20, 72), (17, 17, 65), (9, 9, 33), (1, 1, 33)
PERM16 = (5, 12, 0, 9, 15, 3, 7, 1, 14, 10, 2, 8, 13, 6, 11, 4)
LOSS_CASES = [
    # (18, 20, 72): three tiles per axis, 25 920 voxels, 7 blocks with the last partial, S % 4 == 0: the 16-byte path
    Loss(1, 1, *BIG, (0,), 1, 1.0, 1.0, 0, NO_IGNORE, 'ranked'),
    Loss(3, 2, *BIG, (1,), 3, 0.7, 0.3, 1, NO_IGNORE, 'ranked'),                # batch_dice: the column sum over 21 entries
    Loss(3, 2, *BIG, (1, 0), 2, 1.0, 1.0, 0, NO_IGNORE, 'plateau'),
    Loss(1, 3, *BIG, (1, 2), 16, 0.0, 1.0, 0, NO_IGNORE, 'ranked'),
    Loss(2, 4, *BIG, (1, 2, 3), 2, 1.0, 1.0, 0, 2.0, 'dyadic'),                 # the ignore label inside [0, C)
    Loss(1, 5, *BIG, (3, 1), 3, 1.0, 1.0, 0, NO_IGNORE, 'ranked'),              # an unsorted class list in the gradient's kof[]
    Loss(1, 6, *BIG, (1, 2, 3, 4, 5), 1, 1.0, 0.0, 0, NO_IGNORE, 'ranked'),     # no stage state saved, no skeleton passes backward
    Loss(1, 7, *BIG, (6, 2), 3, 0.7, 0.3, 1, NO_IGNORE, 'plateau'),
    Loss(1, 16, *BIG, PERM16, 1, 1.0, 1.0, 0, NO_IGNORE, 'ranked'),             # K = 16, permuted
    Loss(2, 2, *BIG, (1,), 3, 1.0, 0.0, 0, -1.0, 'dyadic'),
    Loss(2, 3, *BIG, (2, 1), 10, 0.0, 1.0, 1, NO_IGNORE, 'plateau'),
    # (17, 17, 65): 18 785 voxels, 5 blocks, the scalar path by S
    Loss(2, 3, *MID, (1, 2), 3, 1.0, 1.0, 0, NO_IGNORE, 'ranked'),
    Loss(1, 2, *MID, (1,), 16, 1.0, 1.0, 0, NO_IGNORE, 'ranked'),
    Loss(3, 4, *MID, (3, 0, 1), 2, 0.7, 0.3, 1, 3.0, 'plateau'),
    # (9, 9, 33) and (1, 1, 33)
    Loss(2, 5, *SMALL, (1, 2, 3, 4), 2, 1.0, 1.0, 1, NO_IGNORE, 'dyadic'),
    Loss(1, 6, *SMALL, (5, 0, 3), 3, 0.0, 1.0, 0, NO_IGNORE, 'ranked'),
    Loss(1, 16, *SMALL, PERM16[::-1], 1, 0.7, 0.3, 0, 15.0, 'plateau'),
    Loss(2, 3, *SMALL, (1, 2), 3, 1.0, 1.0, 0, NO_IGNORE, 'empty'),             # nothing counts at all
    Loss(2, 1, *ROW, (0,), 3, 1.0, 1.0, 0, NO_IGNORE, 'ranked'),
    Loss(1, 2, *ROW, (1,), 1, 1.0, 1.0, 1, NO_IGNORE, 'ranked'),
    Loss(3, 3, *ROW, (2, 1), 16, 0.7, 0.3, 0, NO_IGNORE, 'dyadic'),
]

# one refusal per entry, from its SEG3D_REQUIRE list
REFUSALS = {'seg3d_soft_skeleton': ('iters = 17', 'an axis of 257'),
            'seg3d_cldice_loss_fwd': ('a class id listed twice', 'a workspace 4 bytes past a 16-byte boundary', 'both term weights 0'),
            'seg3d_cldice_loss_bwd': ('an axis of 257', 'a workspace 4 bytes past a 16-byte boundary')}


# ---- plans: what the host code of csrc/cldice_loss.hip decides for a case ------------------------------------------------------------
def voxels(c):
    return c.Z * c.Y * c.X


def tiles(c):
    """(tiles along x, y, z)"""
    return (c.X + TX - 1) // TX, (c.Y + TY - 1) // TY, (c.Z + TZ - 1) // TZ


def vec(c, shift=0):
    """compound_vec_ok on the tests' buffers: 16-byte aligned before `shift` floats"""
    return voxels(c) % 4 == 0 and shift % 4 == 0


def coef_rows(c):
    return 1 if c.batch_dice else c.N


def coef_floats(c):
    return 2 * coef_rows(c) * c.C + 3 * coef_rows(c) * len(c.classes)


def column_entries(c):
    """the entries compound_column_sum adds for one (r, k) of cld_finalize_kernel"""
    return (c.N if c.batch_dice else 1) * K.blocks(voxels(c))


def _up4(v):
    return (v + 3) & ~3


def layout(N, C, nk, S, iters):
    """CldLayout: offsets in floats of cpart, SP, ST, the four planes, a_j, b_j, the selection bytes; then the total in bytes"""
    P = _up4(N * nk * S)
    cpart = _up4(K.part_floats(N, C, S))
    sp = cpart + _up4(nk * N * K.blocks(S) * 4)
    st = sp + P
    buf = st + P
    sa = buf + 4 * P
    sb = sa + (iters + 1) * P
    sel = sb + (iters + 1) * P
    return dict(cpart=cpart, sp=sp, st=st, buf=buf, sa=sa, sb=sb, sel=sel, P=P, total_bytes=sel * 4 + _up4((iters + 1) * P))


def loss_workspace_bytes(c):
    return layout(c.N, c.C, len(c.classes), voxels(c), c.iters)['total_bytes']


def skel_workspace_bytes(c):
    return 2 * c.planes * voxels(c) * 4


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _bricks(values, Z, Y, X):
    """[B, Z, Y, X] constant on 3 x 3 x 4 bricks: voxel (z, y, x) takes values[.., z // 3, y // 3, x // 4]"""
    iz, iy, ix = torch.arange(Z) // 3, torch.arange(Y) // 3, torch.arange(X) // 4
    return values[:, iz][:, :, iy][:, :, :, ix]


def planes_input(seed, tag, B, Z, Y, X, fill):
    """[B, Z, Y, X] float32 of one value class"""
    S = Z * Y * X
    if fill == 'ranked':
        order = _noise(seed, tag, (B, S)).argsort(1)
        rank = torch.empty_like(order)
        rank.scatter_(1, order, torch.arange(S).repeat(B, 1))
        return ((rank + 1).double() / (S + 1)).float().reshape(B, Z, Y, X)
    if fill == 'mask':                                   # blobs of ones: a smoothed noise field above its median
        n = _noise(seed, tag, (B, 1, Z, Y, X))
        sm = F.avg_pool3d(F.pad(n, (1, 1, 1, 1, 1, 1), mode='replicate'), 3, 1)
        return (sm > 0.0).float().reshape(B, Z, Y, X)
    if fill == 'dyadic':
        return (torch.floor(_noise(seed, tag, (B, S)).abs() * 5.0).clamp(max=8.0) / 8.0).reshape(B, Z, Y, X)
    if fill == 'plateau':
        bz, by, bx = (Z + 2) // 3, (Y + 2) // 3, (X + 3) // 4
        v = torch.floor(_noise(seed, tag, (B, bz * by * bx)).abs() * 5.0).clamp(max=8.0) / 8.0
        odd = ((torch.arange(bz).view(-1, 1, 1) + torch.arange(by).view(1, -1, 1) + torch.arange(bx).view(1, 1, -1)) % 2).expand(B, bz, by, bx)
        x = torch.where(_bricks(odd, Z, Y, X) == 1, planes_input(seed + 50, tag, B, Z, Y, X, 'dyadic'), _bricks(v.reshape(B, bz, by, bx), Z, Y, X))
        x[:, :, :, X // 4:X // 4 + max(1, X // 6)] = 1.0          # saturated: a slab of exact ones, a slab of exact zeros
        x[:, :, :, X // 2:X // 2 + max(1, X // 6)] = 0.0
        return x
    raise ValueError(fill)


def skel_input(c):
    return planes_input(3100, 'cldice/skel-{}'.format(case_id(c)), c.planes, c.Z, c.Y, c.X, c.fill)


def loss_inputs(c):
    """(p [N, C, Z, Y, X], t [N, Z, Y, X], wdice [C], wcl [K], gout).  The probabilities are planes of the case's value class (the
    C ABI asks no normalisation of them).  Target: blob ids on 3 x 4 x 5 bricks; the last voxels take -1, C, 1000 and, for C >= 2,
    1.7 (counts as class 1); a z slab of the ignore label when that lies outside [0, C) (inside, the class itself is ignored);
    nothing counts in sample 1 (N > 2); fill 'empty': nothing counts at all.  wdice and wcl are unnormalised with a zero entry
    each (C >= 2, K >= 2)"""
    N, C, Z, Y, X = c.N, c.C, c.Z, c.Y, c.X
    S, nk, tag = Z * Y * X, len(c.classes), 'cldice/' + case_id(c)
    p = planes_input(3101, tag + '/p', N * C, Z, Y, X, 'ranked' if c.fill == 'empty' else c.fill).reshape(N, C, Z, Y, X)
    bz, by, bx = (Z + 2) // 3, (Y + 3) // 4, (X + 4) // 5
    ids = _labels(3102, tag + '/t', (N, bz, by, bx), C)
    t = ids[:, torch.arange(Z) // 3][:, :, torch.arange(Y) // 4][:, :, :, torch.arange(X) // 5].clone()
    tf = t.reshape(-1)
    if not 0.0 <= c.ignore < C and Z >= 3:
        t[:, Z // 2] = c.ignore                           # an ignored wall across z
    elif not 0.0 <= c.ignore < C:
        tf[5::11] = c.ignore
    for i, val in enumerate((-1.0, float(C), 1000.0) + ((1.7,) if C >= 2 else ())):
        tf[N * S - 1 - 2 * i] = val
    if N > 2:
        t[1] = -1.0
    if c.fill == 'empty':
        tf[0::2], tf[1::2] = float(C), -3.0
    wdice = 0.2 + _uniform(3103, tag + '/w', C)
    wcl = 0.3 + _uniform(3104, tag + '/k', nk)
    if C >= 2:
        wdice[0] = 0.0
    if nk >= 2:
        wcl[1] = 0.0
    return p, t, wdice, wcl, (-2.5 if (N + C) % 2 else 1.5)


# ---- the selection-rule reference ----------------------------------------------------------------------------------------------------
E_ORDER = ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0))          # (dz, dy, dx), lowest linear index first
D_ORDER = tuple((dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))


def _select(x, order, outside, less):
    """the first extremum of x [B, Z, Y, X] over `order` with `outside` beyond the volume -> (values, linear index it was taken at)"""
    B, Z, Y, X = x.shape
    xp = F.pad(x, (1, 1, 1, 1, 1, 1), value=outside)
    lin = torch.arange(Z * Y * X).reshape(1, Z, Y, X)
    best = sel = None
    for dz, dy, dx in order:
        v = xp[:, 1 + dz:1 + dz + Z, 1 + dy:1 + dy + Y, 1 + dx:1 + dx + X]
        at = (lin + (dz * Y + dy) * X + dx).expand(B, Z, Y, X)
        if best is None:
            best, sel = v.clone(), at.clone()
            continue
        up = (v < best) if less else (v > best)           # strict: a later position wins only if it is better
        best, sel = torch.where(up, v, best), torch.where(up, at, sel)
    return best, sel


def erode(x):
    return _select(x, E_ORDER, float('inf'), True)


def dilate(x):
    return _select(x, D_ORDER, float('-inf'), False)


def skeleton_ref(x, iters, dtype, keep=False):
    """x [B, Z, Y, X] -> skel [B, Z, Y, X] of `dtype`; keep=True: also the stages' records, a list over j = 0..iters of
    dict(sel_e, sel_d [B, S] int64, a, b [B, S])"""
    B, S = x.shape[0], x[0].numel()
    xj, s, stages = x.to(dtype), None, []
    for j in range(iters + 1):
        e, sel_e = erode(xj)
        o, sel_d = dilate(e)
        d = torch.relu(xj - o)
        if j == 0:
            s, a, b = d, (d > 0).to(dtype), torch.zeros_like(d)
        else:
            u = d - s * d
            on = u > 0
            a, b = torch.where(on, 1.0 - s, torch.zeros_like(s)), torch.where(on, 1.0 - d, torch.ones_like(d))
            s = s + torch.relu(u)
        if keep:
            stages.append(dict(sel_e=sel_e.reshape(B, S), sel_d=sel_d.reshape(B, S), a=a.reshape(B, S), b=b.reshape(B, S)))
        xj = e
    return (s, stages) if keep else s


def skeleton_bwd_ref(stages, gs):
    """dL/dx_0 [B, S] from dL/ds_k [B, S], through the stages' records"""
    B, S = gs.shape
    base = (torch.arange(B) * S).reshape(B, 1)
    gxn = torch.zeros_like(gs)
    for st in reversed(stages):
        gz = gs * st['a']
        ge = gxn.clone().reshape(-1).index_add_(0, (st['sel_d'] + base).reshape(-1), -gz.reshape(-1))
        gxn = gz.clone().reshape(-1).index_add_(0, (st['sel_e'] + base).reshape(-1), ge).reshape(B, S)
        gs = gs * st['b']
    return gxn


def gates(stages):
    """what must not depend on the precision: every selection index, a > 0 and b == 1 of every stage"""
    return [(st['sel_e'], st['sel_d'], st['a'] > 0, st['b'] == 1) for st in stages]


def cldice_ref(p, t, wdice, wcl, c, gout, dtype):
    """-> dict(loss [3] = (L, L_dice, L_cl), coef [2 R C + 3 R K], dprobs [N, C, S], sp, st [N, K, S], sums [R, K, 4], valid, cls,
    onehot, stages)"""
    N, C, S, ks, R = c.N, c.C, voxels(c), list(c.classes), coef_rows(c)
    nk = len(ks)
    tf, pf = t.reshape(N, S), p.reshape(N, C, S)
    valid, cls = K.counting(tf, C, c.ignore)
    lr, A, B, onehot = K.region_ref(pf, valid, cls, wdice, c.dice_weight, c.batch_dice, dtype)
    v = valid.to(dtype)
    P = (pf.to(dtype) * v.unsqueeze(1))[:, ks]                                       # P_c [N, K, S]
    T = onehot[:, ks]                                                                # T_c
    vol = lambda a: a.reshape(N * nk, c.Z, c.Y, c.X)
    sp, stages = skeleton_ref(vol(P), c.iters, dtype, keep=True)
    st = skeleton_ref(vol(T), c.iters, dtype)
    sp, st = sp.reshape(N, nk, S), st.reshape(N, nk, S)
    sums = torch.stack([(sp * T).sum(2), sp.sum(2), (st * P).sum(2), st.sum(2)], 2)   # [N, K, 4]
    if c.batch_dice:
        sums = sums.sum(0, keepdim=True)
    tp, ts = (sums[..., 0] + 1.0) / (sums[..., 1] + 1.0), (sums[..., 2] + 1.0) / (sums[..., 3] + 1.0)
    cl = 2.0 * tp * ts / (tp + ts)                                                   # [R, K]
    w = wcl.to(dtype).unsqueeze(0)
    lc = (w * (1.0 - cl) / R).sum()
    q = -c.cldice_weight * w / R
    dtp, dts = q * 2.0 * ts * ts / ((tp + ts) ** 2), q * 2.0 * tp * tp / ((tp + ts) ** 2)
    a1, a2, a3 = dtp / (sums[..., 1] + 1.0), -dtp * (sums[..., 0] + 1.0) / (sums[..., 1] + 1.0) ** 2, dts / (sums[..., 3] + 1.0)
    row = lambda a: a.expand(N, nk).unsqueeze(2)                                     # [R, K] -> [N, K, 1]
    d = v.unsqueeze(1) * (A.unsqueeze(2) * onehot + B.unsqueeze(2))
    if c.cldice_weight > 0.0:
        gx0 = skeleton_bwd_ref(stages, (row(a1) * T + row(a2)).reshape(N * nk, S)).reshape(N, nk, S)
        d[:, ks] = d[:, ks] + v.unsqueeze(1) * (row(a3) * st + gx0)
    loss = torch.stack([K._total(dtype, (c.dice_weight, lr), (c.cldice_weight, lc)), lr, lc])
    coef = torch.cat([torch.stack([A, B], 2).reshape(-1), torch.stack([a1, a2, a3], 2).reshape(-1)])
    return {'loss': loss, 'coef': coef, 'dprobs': gout * d, 'sp': sp, 'st': st, 'sums': sums, 'valid': valid, 'cls': cls,
            'onehot': onehot, 'stages': stages}


def dice_case(c):
    """the compound case whose loss[1] the clDice loss's must equal bit for bit (the Dice term alone)"""
    return K.Compound(c.N, c.C, voxels(c), 0, c.batch_dice, c.ignore, 'std', 0.0, 1.0, 1.0)


assert MAXC == 16 and DICE_VPB == 4096
