"""Small hand-made volumes for the lesion-wise tests, shared by the CPU tests (oracle against the numbers written out here)
and the GPU tests (device against the oracle).  Arrays are [z, y, x]; no axis is a multiple of the dilation tile
(32 x 8 x 8 in x, y, z)."""
import numpy as np

SHAPE_A = (33, 20, 17)
SHAPE_B = (17, 9, 5)
SHAPE_2D = (1, 19, 23)


def _vol(shape, voxels, label=1, dtype=np.uint8):
    v = np.zeros(shape, dtype)
    for z, y, x in voxels:
        v[z, y, x] = label
    return v


def two_blobs_two_apart():
    """ground truth: voxels at x = 1 and x = 3 of one row: two lesions without dilation, one after one dilation"""
    return _vol(SHAPE_B, [(8, 4, 1), (8, 4, 3)]), _vol(SHAPE_B, [])


def corner_touching():
    """(2, 2, 1) and (3, 3, 2) share only a corner: one 26-connected component; (9, 2, 1) and (11, 4, 3) are two apart
    diagonally: two components.  Three components in all, sizes 2, 1, 1 in canonical order."""
    return _vol(SHAPE_B, [(2, 2, 1), (3, 3, 2), (9, 2, 1), (11, 4, 3)])


def bridge():
    """two 2-voxel lesions and one 7-voxel predicted column that touches one voxel of each (no dilation):
    pairs (1, 1), (2, 1); |U_1| = |U_2| = 7; dice_1 = dice_2 = 2 * 1 / (2 + 7) = 2 / 9; no FN, no FP; lw_dice = 2 / 9"""
    gt = _vol(SHAPE_B, [(8, 1, 1), (8, 1, 2), (8, 7, 1), (8, 7, 2)])
    seg = _vol(SHAPE_B, [(8, y, 1) for y in range(1, 8)])
    return gt, seg


def halo_only():
    """ground truth (8, 4, 1), prediction (8, 4, 2), one dilation: the prediction lies in D_1 \\ G_1: matched, dice 0,
    hd95 = 1 (two single voxels one apart), neither FN nor FP"""
    return _vol(SHAPE_B, [(8, 4, 1)]), _vol(SHAPE_B, [(8, 4, 2)])


def fn_fp_tp():
    """no dilation.  Lesion 1 = {(2,2,1), (2,2,2)} against component 1 = {(2,2,2), (2,2,3)}: dice = 2 * 1 / (2 + 2) = 0.5,
    both directed distance sets are {0, 1}, P95 = 0.95, hd95 = 0.95.  Lesion 2 = {(12,6,3)} is missed (FN), component
    2 = {(8,1,1)} is spurious (FP).  n = 2 + 1 = 3: lw_dice = 0.5 / 3, lw_hd95 = (0.95 + 2 * penalty) / 3,
    lesion_f1 = 2 / (2 + 1 + 1) = 0.5"""
    gt = _vol(SHAPE_B, [(2, 2, 1), (2, 2, 2), (12, 6, 3)])
    seg = _vol(SHAPE_B, [(2, 2, 2), (2, 2, 3), (8, 1, 1)])
    return gt, seg


def small_and_large():
    """lesion 1 is one voxel, lesion 2 three voxels; both are predicted exactly.  With min_lesion_voxels = 2 lesion 1 is
    dropped and its component is no false positive: n_gt = 1, n_tp = 1, n_fn = n_fp = 0, lw_dice = 1, lw_hd95 = 0"""
    vox = [(2, 2, 1), (12, 6, 1), (12, 6, 2), (12, 6, 3)]
    return _vol(SHAPE_B, vox), _vol(SHAPE_B, vox)


def faces(shape=SHAPE_B):
    """ground truth: the eight corners and the centre voxel of every face; prediction: a shifted subset plus a centre blob"""
    Z, Y, X = shape
    gt = np.zeros(shape, np.uint8)
    for z in (0, Z - 1):
        for y in (0, Y - 1):
            for x in (0, X - 1):
                gt[z, y, x] = 1
    gt[0, Y // 2, X // 2] = gt[Z - 1, Y // 2, X // 2] = 1
    gt[Z // 2, 0, X // 2] = gt[Z // 2, Y - 1, X // 2] = 1
    gt[Z // 2, Y // 2, 0] = gt[Z // 2, Y // 2, X - 1] = 1
    seg = np.zeros(shape, np.uint8)
    seg[0, 0, 0] = seg[Z - 1, Y - 1, X - 1] = seg[Z - 1, 0, X - 1] = 1
    seg[0, Y // 2, X // 2 - 1] = seg[Z // 2, Y - 1, X // 2] = 1
    seg[Z // 2, Y // 2, X // 2] = 1
    return gt, seg


def lattice():
    """isolated voxels on a stride-3 lattice of 48 x 40 x 36 ([z, y, x] = 36 x 40 x 48): 16 * 14 * 12 = 2688 components"""
    v = np.zeros((36, 40, 48), np.uint8)
    v[::3, ::3, ::3] = 1
    return v


def random_sparse(shape, seed, density=0.01):
    rng = np.random.RandomState(seed)
    return (rng.rand(*shape) < density).astype(np.uint8)


def random_blobs(shape, seed, count=6, labels=(1,)):
    """`count` random boxes of 1..4 voxels a side, labelled round-robin from `labels`"""
    rng = np.random.RandomState(seed)
    v = np.zeros(shape, np.int32)
    for k in range(count):
        lo = [int(rng.randint(0, s)) for s in shape]
        hi = [min(s, l + int(rng.randint(1, 5))) for l, s in zip(lo, shape)]
        v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = labels[k % len(labels)]
    return v


def perturbed(gt, seed):
    """a prediction: the ground truth shifted by one voxel, one slab removed and a few spurious voxels added"""
    rng = np.random.RandomState(seed)
    seg = np.roll(gt, 1, axis=2)
    seg[:, :, 0] = 0
    seg[: gt.shape[0] // 3] = 0
    for _ in range(3):
        z, y, x = (int(rng.randint(0, s)) for s in gt.shape)
        seg[z, y, x] = gt.max() if gt.max() > 0 else 1
    return seg
