"""Oracle of the MFMA weight images (csrc/layout.hip: seg3d_pack_weights_mfma[_bf16] and their _multi forms), shared by
tests/test_pack_oracle.py and tests/test_gpu_pack.py: numpy on the CPU, written from the layout definitions.

A weight is W(a, b, t) = w[a*sa + b*sb + (flip ? Tsrc-1-t : t)], a = reduction channel (A of them), b = output channel
(B of them), t = source tap (Tsrc of them); W = 0 for a >= A or b >= B (the images are padded to whole chunks).

  fp32, T <= 27   wp[bb][ab][t][h 2][j 32][r 4] = W(ab*8 + 4h + r, bb*32 + j, t)
  bf16, T <= 27   wp[bb][ab][t][h 2][j 32][r 8] = bf16(W(ab*16 + 8h + r, bb*32 + j, t)), round to nearest even
  fp32, T = 36    the same [bb][ab][tw 36][h][j][r] with tw = (kz*3 + ky)*4 + p: the Winograd F(2, 3) weight transform u_p over
                  the three kx taps of a 27-tap weight
  fp32, T = 48    wp[bb][ab][h 2][g 12][r 4][j 32][s 4] = U(a, b, step_t(4g + s)): U(t48 = kz*16 + py*4 + px) is the F(2x2, 3x3)
                  transform G g G^T of the (ky, kx) taps, u_px along kx first, u_py along ky of those results second; step_t is
                  the K-chunk step order of the forward kernels (csrc/seg3d_common.h)

  u_0 = g0, u_1 = 0.5*((g0 + g2) + g1), u_2 = 0.5*((g0 + g2) - g1), u_3 = g2   (rows of G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]])

The float32 images are bit-exact statements: the transforms run in the dtype of `w` in exactly this association, and the only
multiplications are by 0.5 (exact for normal values), so a fused multiply-add on the device changes nothing.
"""
import numpy as np
import torch

WINO_T, WINO2D_T = 36, 48
CORNER_POINTS = (0, 3, 12, 15)
# the 16 Winograd points py*4 + px in the order the forward kernels visit them: the twelve ordinary ones ascending, the four
# corners (whose accumulators may wait for a fused addend) last
POINT_ORDER = tuple(p for p in range(16) if p not in CORNER_POINTS) + CORNER_POINTS


def step_t(s):
    """t48 = kz*16 + point of step s (0..47): the points in pairs (a, b), each pair's six steps a0 b0 a1 b1 a2 b2 (digit = kz)"""
    pair, within = divmod(s, 6)
    return (within >> 1) * 16 + POINT_ORDER[2 * pair + (within & 1)]


def source_taps(w, A, B, T, sa, sb, flip):
    """W[a][b][t] of the flat storage `w` (numpy, any float dtype), T source taps"""
    w = np.asarray(w).reshape(-1)
    a, b, t = np.meshgrid(np.arange(A), np.arange(B), np.arange(T), indexing='ij')
    return w[a * sa + b * sb + (T - 1 - t if flip else t)]


def wino_u(g0, g1, g2, p):
    half = g0.dtype.type(0.5)
    return (g0, half * ((g0 + g2) + g1), half * ((g0 + g2) - g1), g2)[p]


def wino_taps(W27, T):
    """[A][B][27] source taps -> the [A][B][T] transformed "taps" of the T = 36 / 48 images, in W27's dtype"""
    g = W27.reshape(W27.shape[:2] + (3, 3, 3))                                            # [a][b][kz][ky][kx]
    ux = np.stack([wino_u(g[..., 0], g[..., 1], g[..., 2], p) for p in range(4)], -1)     # [a][b][kz][ky][px]
    if T == WINO_T:
        return ux.reshape(W27.shape[:2] + (36,))
    assert T == WINO2D_T
    u = np.stack([wino_u(ux[..., 0, :], ux[..., 1, :], ux[..., 2, :], p) for p in range(4)], -2)   # [a][b][kz][py][px]
    return u.reshape(W27.shape[:2] + (48,))


def packed_image(w, A, B, T, sa, sb, flip, bf16=False):
    """the image the packers write for these arguments: flat CPU torch tensor, float32 or bfloat16"""
    w = np.asarray(w, dtype=np.float32)
    if T in (WINO_T, WINO2D_T):
        assert not bf16, 'the Winograd images exist in fp32 only'
        Wt = wino_taps(source_taps(w, A, B, 27, sa, sb, flip), T)
    else:
        Wt = source_taps(w, A, B, T, sa, sb, flip)
    assert Wt.dtype == np.float32
    HW = 8 if bf16 else 4                                                                 # channels per half
    AB, BB = -(-A // (2 * HW)), -(-B // 32)
    Wp = np.zeros((AB * 2 * HW, BB * 32, T), np.float32)
    Wp[:A, :B] = Wt
    if T == WINO2D_T:
        Wp = Wp[:, :, [step_t(s) for s in range(48)]]
        img = Wp.reshape(AB, 2, HW, BB, 32, 12, 4).transpose(3, 0, 1, 5, 2, 4, 6)          # (ab h r bb j g s) -> [bb][ab][h][g][r][j][s]
    else:
        img = Wp.reshape(AB, 2, HW, BB, 32, T).transpose(3, 0, 5, 1, 4, 2)                 # (ab h r bb j t) -> [bb][ab][t][h][j][r]
    img = torch.from_numpy(np.ascontiguousarray(img).reshape(-1))
    return img.bfloat16() if bf16 else img
