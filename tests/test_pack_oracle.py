"""CPU checks of tests/pack_oracle.py, the statement of the MFMA weight images the GPU tests compare the packers with:
the plain images un-permute to W, the T = 48 step order is a permutation, and the T = 36 / 48 transforms are the Winograd
weight transforms (float64 identities against a direct correlation), so the oracle is not a copy of the kernel."""
import numpy as np
import pytest
import torch

import pack_oracle as PO

ORIENTATIONS = ('fwd', 'dgrad')


def _weight(seed, A, B, T, orient, dtype=np.float32):
    """(flat storage, sa, sb, flip): fwd = w[b][a][t]; dgrad = w[a][b][t] read with flipped taps"""
    w = (np.random.RandomState(seed).standard_normal(A * B * T) * 0.1).astype(dtype)
    return (w, T, A * T, 0) if orient == 'fwd' else (w, B * T, T, 1)


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('orient', ORIENTATIONS)
@pytest.mark.parametrize('T', [1, 8, 27])
@pytest.mark.parametrize('AB_', [(4, 8), (12, 40), (40, 72)])
def test_plain_image_unpermutes_to_w(AB_, T, orient, bf16):
    """element (bb, ab, t, h, j, r) of the image, by index arithmetic: W(ab*AW + HW*h + r, bb*32 + j, t) inside, 0 in the padding"""
    A, B = AB_
    w, sa, sb, flip = _weight(1, A, B, T, orient)
    img = PO.packed_image(w, A, B, T, sa, sb, flip, bf16=bf16)
    HW = 8 if bf16 else 4
    nab, nbb = -(-A // (2 * HW)), -(-B // 32)
    assert img.numel() == nbb * nab * T * 64 * HW
    bb, ab, t, h, j, r = np.indices((nbb, nab, T, 2, 32, HW)).reshape(6, -1)
    a, b = ab * 2 * HW + HW * h + r, bb * 32 + j
    inside = (a < A) & (b < B)
    src = a * sa + b * sb + (T - 1 - t if flip else t)
    want = torch.from_numpy(np.where(inside, w[np.where(inside, src, 0)], np.float32(0)))
    if bf16:
        assert np.array_equal(img.view(torch.int16).numpy(), want.bfloat16().view(torch.int16).numpy())
    else:
        assert np.array_equal(img.numpy().view(np.int32), want.numpy().view(np.int32))
    assert inside.sum() == A * B * T and (inside.sum() < inside.size) == (A % (2 * HW) != 0 or B % 32 != 0)


def test_step_order_is_a_permutation():
    steps = [PO.step_t(s) for s in range(48)]
    assert sorted(steps) == list(range(48))
    # the corner points of every kz come in the last two pairs (steps 36..47)
    assert sorted(t & 15 for t in steps[36:]) == sorted(3 * list(PO.CORNER_POINTS))


AT = np.array([[1., 1., 1., 0.], [0., 1., -1., -1.]])                                   # F(2, 3) output transform
BT = np.array([[1., 0., -1., 0.], [0., 1., 1., 0.], [0., -1., 1., 0.], [0., 1., 0., -1.]])   # input transform


@pytest.mark.parametrize('orient', ORIENTATIONS)
def test_wino36_is_f23_along_kx(orient):
    """A^T [(G g) * (B^T d)] = the two outputs of the 3-tap correlation along x, for every (a, b, kz, ky)"""
    A, B = 3, 5
    w, sa, sb, flip = _weight(2, A, B, 27, orient, np.float64)
    W = PO.source_taps(w, A, B, 27, sa, sb, flip)
    U = PO.wino_taps(W, 36).reshape(A, B, 9, 4)
    assert U.dtype == np.float64
    g = W.reshape(A, B, 9, 3)
    assert np.array_equal(g[1, 2, 4], w[1 * sa + 2 * sb + (np.arange(14, 11, -1) if flip else np.arange(12, 15))])
    d = np.random.RandomState(3).standard_normal(4)
    y = np.einsum('op,abtp->abto', AT, U * (BT @ d))
    ref = np.stack([g @ d[0:3], g @ d[1:4]], -1)
    assert np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize('orient', ORIENTATIONS)
def test_wino48_is_f2x2_3x3_over_ky_kx(orient):
    """A^T [(G g G^T) * (B^T d B)] A = the 2 x 2 outputs of the 3 x 3 correlation on one 4 x 4 input tile, for every (a, b, kz)"""
    A, B = 3, 5
    w, sa, sb, flip = _weight(4, A, B, 27, orient, np.float64)
    W = PO.source_taps(w, A, B, 27, sa, sb, flip)
    U = PO.wino_taps(W, 48).reshape(A, B, 3, 4, 4)                                      # [a][b][kz][py][px]
    assert U.dtype == np.float64
    g = W.reshape(A, B, 3, 3, 3)                                                        # [a][b][kz][ky][kx]
    d = np.random.RandomState(5).standard_normal((4, 4))                                # [y][x]
    y = np.einsum('op,abzpq,nq->abzon', AT, U * (BT @ d @ BT.T), AT)
    ref = np.empty((A, B, 3, 2, 2))
    for oy in range(2):
        for ox in range(2):
            ref[..., oy, ox] = np.einsum('abzyx,yx->abz', g, d[oy:oy + 3, ox:ox + 3])
    assert np.abs(y - ref).max() <= 1e-12 * np.abs(ref).max()


def test_wino_images_place_the_transformed_taps():
    """T = 36 keeps the plain [t][h][j][r] order on the 36 transformed taps; T = 48 is [h][g][r][j][s] in step order"""
    A, B = 12, 40
    w, sa, sb, flip = _weight(6, A, B, 27, 'fwd')
    W = PO.source_taps(w, A, B, 27, sa, sb, flip)
    for T in (36, 48):
        U = PO.wino_taps(W, T)
        img = PO.packed_image(w, A, B, T, sa, sb, flip).numpy()
        nab = 2
        for (a, b, s) in ((0, 0, 0), (5, 33, 7), (11, 39, T - 1), (9, 31, 20)):
            ab, h, r, bb, j = a // 8, (a % 8) // 4, a % 4, b // 32, b % 32
            chunk = (bb * nab + ab) * T * 256
            if T == 36:
                assert img[chunk + ((s * 2 + h) * 32 + j) * 4 + r] == U[a, b, s]
            else:
                assert img[chunk + (((h * 12 + s // 4) * 4 + r) * 32 + j) * 4 + s % 4] == U[a, b, PO.step_t(s)]
        # chunk ab = 1, half h = 1: a >= 12 = A is padding (T = 36: t 0, h 1, j 0, r 3; T = 48: h 1, g 0, r 0, j 0, s 0)
        assert img[(0 * nab + 1) * T * 256 + (128 + 3 if T == 36 else 12 * 512)] == 0
