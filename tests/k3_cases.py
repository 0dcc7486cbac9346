"""The case table of the direct 3x3x3 kernel family (csrc/conv_mfma.hip: forward / data gradient and weight gradient, fp32 and
bf16), shared by tests/test_k3_variants.py (host only: every case maps to the kernels it is named for, every reachable kernel is
named by a case) and tests/test_gpu_k3_float64.py (the same cases against float64 on the device).

Forward codes (seg3d_conv3d_k3_mfma_variant, seg3d_conv3d_k3_bf16_variant), see FWD_KERNELS:
  1..4               conv3d_k3_mfma_kernel<MA>                    first generation: Cin % 8 == 4 or Cout % 4 != 0
  100 + 10 MA + NB   conv3d_k3_mfma2_kernel<MA, NB>               / conv3d_k3_mfma2_splitk_kernel<MA, NB> when split-K
  300 + 10 MA + 1    conv3d_k3_mfma2w8_kernel<MA, 1>              8 waves, tiles of 256 MA voxels (MA = 2 also the 384-voxel tile)
  200 + 10 MA + NB   conv3d_k3_mfma2_bf16_kernel<MA, NB, OUT_BF>  / conv3d_k3_mfma2_bf16_splitk_kernel<MA, NB>
  400 + 10 MA + 1    conv3d_k3_mfma2w8_bf16_kernel<MA, 1, OUT_BF>
A split-K launch (the *_fwd_workspace_floats query is not 0) is followed by conv3d_splitk_finish_kernel, with a bf16 output by
conv3d_splitk_finish_bf16out_kernel.  What the queries do not say is derived from them:
  K slabs     ks = *_fwd_workspace_floats / (N D H W Cout)
  work items  N * *_stats_count / nw for a whole-K second-generation plan, nw = 8 waves for 3xx / 4xx codes and 4 otherwise

ALL_FWD lists the (bf16, code, split-K) triples a host-only scan of the two plan functions reaches over N in {1, 2, 3}, Cin in
{4 .. 256}, Cout in {4 .. 256} and extents up to 25 x 32 x 65, at most 1.5 GMAC and 4M elements per tensor.  Instantiations the
launchers can never select, and the rule that excludes them:
  * whole-K conv3d_k3_mfma2_kernel<2, 1> and <4, 1>: seg3d_fwd_plan sends ks == 1, nb == 1, ma in {2, 4} to the 8-wave kernel
    (311 / 321); both run as split-K kernels only.  <3, 1> runs both ways.
  * whole-K conv3d_k3_mfma2_bf16_kernel<2, 1>, <3, 1>, <4, 1>: seg3d_fwd_plan_bf16 sends ks == 1, nb == 1, ma >= 2 to the 8-wave
    kernel (411 / 421, ma 3 and 4 share <2, 1>); split-K only.
  * an 8-wave kernel with NB = 2, and NB = 2 with MA > 2: the 8-wave rule needs nb == 1, and a two-block tile has at most 256 voxels.
Within the scanned range the scan also finds no shape for
  * split-K of the first-generation <2>, <3>, <4> (seg3d_fwd_ksplit splits below 192 workgroups only, and every such shape of
    the scan gets a tile of at most 128 voxels from seg3d_pick_tile), nor <4> with N = 1 or with Cout % 4 != 0 (N3_ONLY);
  * whole-K bf16 <1, 2> (212), whole-K bf16 <1, 1> with more than 256 items and whole-K fp32 <2, 2> with more than 256 items
    (NO_MANY_ITEMS): the cost model prices another tile, or a K split, lower on all of them.

Weight-gradient codes (seg3d_conv3d_k3_wgrad_variant): 10 k + r, see WGRAD_KERNELS; r = 1: conv3d_k3_wgrad_reduce_kernel<16>
(32 or more slabs), r = 0: <4>.
"""
from collections import namedtuple

# role 'fwd': plain pack, GroupNorm statistics; 'dgrad': the data-gradient role -- flip = 1 pack of the transposed weight,
# stats = NULL.  bias / addend: which optional operands are passed ('fwd' defaults to bias only, 'dgrad' to the addend only)
Fwd = namedtuple('Fwd', 'kernel splitk bf16 out_bf16 N D H W Cin Cout role bias addend')
Wgrad = namedtuple('Wgrad', 'kernel reducer bf16 N D H W Cin Cout accumulate')

FWD_KERNELS = {1: 'mfma<1>', 2: 'mfma<2>', 3: 'mfma<3>', 4: 'mfma<4>',
               111: 'mfma2<1,1>', 112: 'mfma2<1,2>', 121: 'mfma2<2,1>', 122: 'mfma2<2,2>', 131: 'mfma2<3,1>', 141: 'mfma2<4,1>',
               311: 'mfma2w8<1,1>', 321: 'mfma2w8<2,1>',
               211: 'mfma2_bf16<1,1>', 212: 'mfma2_bf16<1,2>', 221: 'mfma2_bf16<2,1>', 222: 'mfma2_bf16<2,2>',
               231: 'mfma2_bf16<3,1>', 241: 'mfma2_bf16<4,1>', 411: 'mfma2w8_bf16<1,1>', 421: 'mfma2w8_bf16<2,1>'}
WGRAD_KERNELS = {'wgrad2_4x4x8': 0, 'wgrad2_4x4x4': 1, 'wgrad2_2x6x6': 2, 'wgrad3_8': 3, 'wgrad3_8_irr': 4, 'wgrad3_4': 5,
                 'wgrad3_4_irr': 6, 'widening': 7}
CUS = 256             # the constant of the cost model (not the device's CU count)


def fwd_code(c):
    return c.kernel


def wgrad_code(c):
    return 10 * WGRAD_KERNELS[c.kernel] + (1 if c.reducer == 16 else 0)


def case_id(c):
    vals = [('T' if v else 'F') if isinstance(v, bool) else str(v) for v in c]
    return type(c).__name__.lower() + '-' + '-'.join(vals)


def body(c):
    """the four kernel bodies the bias / addend epilogues live in"""
    if c.kernel < 100:
        return 'gen1'
    if c.kernel >= 300:
        return 'w8'
    return 'v2_splitk' if c.splitk else 'v2'


def persistent(c):
    """whole-K second-generation launches walk N * stats_count / nw items with min(items, CUs) workgroups"""
    return c.kernel >= 100 and not c.splitk


def waves(c):
    return 8 if c.kernel >= 300 else 4


def chunks(c):
    """K chunks: 16 channels for bf16, else 8"""
    return c.Cin // 16 if c.bf16 else (c.Cin + 7) // 8


def ragged(c):
    """no candidate tile extent above 1 (z: 2, 3, 4, 6, 8; y: 2 .. 16, x: 4 .. 32, all multiples of 2 or 3) divides D, H or W"""
    return c.D > 1 and c.D % 2 and c.D % 3 and c.H % 2 and c.H % 3 and c.W % 2 == 1


def partial_block(c):
    """a partial 32-channel column block; NB = 2 kernels need an even block count"""
    nb2 = c.kernel >= 100 and c.kernel % 10 == 2
    return c.Cout % 32 != 0 and (not nb2 or ((c.Cout + 31) // 32) % 2 == 0)


ITEM_CLASS = {}       # persistent cases: 'many' (more than CUS items, not a multiple of CUS) or 'few' (fewer than CUS)


def _f(kernel, splitk, out_bf16, N, dims, Cin, Cout, role, bias=None, addend=None, items=None):
    c = Fwd(kernel, splitk, int(200 <= kernel < 300 or kernel >= 400), out_bf16, N, dims[0], dims[1], dims[2], Cin, Cout, role,
            int(role == 'fwd') if bias is None else bias, int(role == 'dgrad') if addend is None else addend)
    if items:
        ITEM_CLASS[c] = items
    return c


T, F_ = True, False
FWD_CASES = [
    # ---- fp32, first generation (Cin % 8 == 4: the last chunk is half empty) ----
    _f(1, F_, 0, 1, (5, 5, 5), 4, 4, 'dgrad'),
    _f(1, F_, 0, 3, (5, 5, 5), 12, 6, 'fwd'),                     # Cout % 4 != 0
    _f(1, F_, 0, 2, (5, 7, 9), 12, 20, 'fwd', 1, 1),
    _f(1, F_, 0, 2, (5, 7, 9), 12, 20, 'dgrad', 0, 0),
    _f(1, T, 0, 1, (5, 5, 5), 36, 4, 'fwd'),                      # its own split-K (seg3d_fwd_ksplit): 5 chunks in slabs of 3
    _f(1, T, 0, 3, (3, 5, 7), 44, 8, 'dgrad'),
    _f(1, T, 0, 3, (5, 5, 5), 36, 20, 'fwd', 1, 1),
    _f(1, T, 0, 1, (5, 5, 5), 36, 4, 'dgrad', 0, 0),
    _f(2, F_, 0, 3, (13, 25, 49), 4, 4, 'dgrad'),
    _f(2, F_, 0, 1, (24, 25, 49), 4, 36, 'fwd'),
    _f(2, F_, 0, 3, (13, 25, 49), 4, 6, 'fwd'),
    _f(3, F_, 0, 3, (25, 25, 65), 4, 4, 'fwd'),
    _f(3, F_, 0, 3, (24, 25, 65), 4, 6, 'fwd'),
    _f(3, F_, 0, 1, (25, 25, 17), 4, 256, 'dgrad'),
    _f(4, F_, 0, 3, (13, 25, 49), 4, 72, 'fwd'),
    _f(4, F_, 0, 3, (13, 25, 49), 4, 72, 'dgrad'),
    # ---- fp32, second generation, whole K (persistent) ----
    _f(111, F_, 0, 1, (5, 5, 5), 8, 4, 'fwd', items='few'),
    _f(111, F_, 0, 3, (25, 13, 49), 16, 4, 'dgrad', items='many'),
    _f(111, F_, 0, 2, (5, 7, 9), 16, 36, 'fwd', 1, 1, items='few'),
    _f(111, F_, 0, 2, (5, 7, 9), 16, 36, 'dgrad', 0, 0, items='few'),
    _f(112, F_, 0, 3, (25, 13, 49), 8, 36, 'fwd', items='many'),
    _f(112, F_, 0, 1, (13, 25, 33), 8, 128, 'dgrad', items='few'),
    _f(122, F_, 0, 2, (25, 25, 33), 8, 36, 'fwd', items='few'),
    _f(122, F_, 0, 3, (24, 24, 33), 8, 36, 'dgrad', items='few'),
    _f(122, F_, 0, 1, (25, 25, 33), 8, 128, 'fwd', items='few'),
    _f(131, F_, 0, 3, (13, 25, 49), 8, 4, 'fwd', items='few'),
    _f(131, F_, 0, 1, (25, 25, 49), 8, 72, 'dgrad', items='many'),
    # ---- fp32, second generation, split-K + finish pass ----
    _f(111, T, 0, 3, (7, 25, 9), 64, 4, 'fwd'),
    _f(111, T, 0, 1, (1, 2, 4), 48, 4, 'dgrad'),
    _f(111, T, 0, 2, (7, 25, 9), 64, 20, 'fwd', 1, 1),
    _f(111, T, 0, 2, (7, 25, 9), 64, 20, 'dgrad', 0, 0),
    _f(112, T, 0, 3, (25, 5, 17), 128, 36, 'dgrad'),
    _f(112, T, 0, 1, (1, 2, 65), 256, 256, 'fwd'),
    _f(121, T, 0, 3, (5, 5, 33), 128, 36, 'fwd'),
    _f(121, T, 0, 1, (5, 25, 9), 256, 4, 'dgrad'),
    _f(122, T, 0, 3, (5, 13, 17), 128, 36, 'fwd'),
    _f(122, T, 0, 1, (25, 25, 9), 96, 36, 'dgrad'),
    _f(122, T, 0, 3, (5, 5, 33), 64, 256, 'dgrad'),
    _f(131, T, 0, 3, (25, 25, 5), 128, 4, 'dgrad'),
    _f(131, T, 0, 1, (25, 25, 5), 192, 4, 'fwd'),
    _f(141, T, 0, 3, (25, 5, 65), 64, 4, 'fwd'),
    _f(141, T, 0, 1, (5, 24, 33), 256, 4, 'dgrad'),
    # ---- fp32, 8 waves (persistent) ----
    _f(311, F_, 0, 3, (5, 25, 65), 8, 4, 'fwd', items='few'),
    _f(311, F_, 0, 1, (24, 25, 49), 8, 4, 'dgrad', items='few'),
    _f(311, F_, 0, 3, (5, 25, 65), 8, 72, 'dgrad', items='many'),
    _f(311, F_, 0, 3, (5, 25, 65), 8, 4, 'fwd', 1, 1, items='few'),
    _f(311, F_, 0, 3, (5, 25, 65), 8, 4, 'dgrad', 0, 0, items='few'),
    _f(321, F_, 0, 1, (25, 25, 65), 8, 36, 'fwd', items='few'),
    _f(321, F_, 0, 3, (24, 25, 49), 8, 36, 'dgrad', items='many'),
    # ---- bf16, whole K (persistent) ----
    _f(211, F_, 0, 1, (5, 5, 5), 16, 4, 'fwd', items='few'),
    _f(211, F_, 1, 3, (1, 2, 4), 16, 4, 'dgrad', items='few'),
    _f(211, F_, 0, 2, (5, 7, 9), 16, 20, 'fwd', 1, 1, items='few'),
    _f(211, F_, 1, 2, (5, 7, 9), 16, 20, 'dgrad', 0, 0, items='few'),
    _f(222, F_, 0, 1, (25, 25, 65), 16, 36, 'fwd', items='few'),
    _f(222, F_, 1, 3, (5, 25, 17), 16, 256, 'dgrad', items='few'),
    _f(222, F_, 1, 2, (25, 25, 65), 16, 36, 'dgrad', items='many'),
    # ---- bf16, split-K + finish pass (out_bf16: conv3d_splitk_finish_bf16out_kernel) ----
    _f(211, T, 1, 1, (5, 5, 5), 128, 4, 'fwd'),
    _f(211, T, 0, 3, (25, 2, 4), 256, 72, 'dgrad'),
    _f(211, T, 1, 3, (5, 5, 5), 128, 20, 'fwd', 1, 1),
    _f(211, T, 0, 2, (5, 5, 5), 128, 36, 'dgrad', 0, 0),
    _f(212, T, 0, 3, (5, 25, 5), 256, 36, 'fwd'),
    _f(212, T, 1, 3, (1, 2, 65), 256, 256, 'dgrad'),
    _f(212, T, 1, 1, (5, 25, 5), 192, 256, 'fwd'),
    _f(221, T, 0, 1, (25, 25, 5), 192, 4, 'fwd'),
    _f(221, T, 1, 3, (25, 2, 9), 256, 72, 'dgrad'),
    _f(222, T, 1, 3, (7, 25, 9), 256, 36, 'fwd'),
    _f(222, T, 0, 1, (5, 24, 33), 256, 36, 'dgrad'),
    _f(231, T, 0, 3, (7, 25, 17), 256, 4, 'dgrad'),
    _f(231, T, 1, 1, (5, 25, 49), 192, 4, 'fwd'),
    _f(241, T, 0, 3, (13, 25, 9), 256, 4, 'fwd'),
    _f(241, T, 1, 1, (13, 25, 17), 256, 4, 'dgrad'),
    # ---- bf16, 8 waves (persistent) ----
    _f(411, F_, 0, 3, (5, 25, 65), 16, 4, 'fwd', items='few'),
    _f(411, F_, 1, 1, (24, 25, 49), 16, 4, 'dgrad', items='few'),
    _f(411, F_, 0, 3, (25, 24, 17), 16, 72, 'dgrad', items='many'),
    _f(411, F_, 1, 3, (5, 25, 65), 16, 4, 'fwd', 1, 1, items='few'),
    _f(411, F_, 0, 3, (5, 25, 65), 16, 4, 'dgrad', 0, 0, items='few'),
    _f(421, F_, 1, 3, (13, 25, 49), 16, 4, 'fwd', items='few'),
    _f(421, F_, 0, 1, (25, 25, 49), 16, 72, 'dgrad', items='many'),
]

# (bf16, code, split-K) triples the scan reaches
ALL_FWD = sorted([(0, k, False) for k in (1, 2, 3, 4, 111, 112, 122, 131, 311, 321)] +
                 [(0, k, True) for k in (1, 111, 112, 121, 122, 131, 141)] +
                 [(1, k, False) for k in (211, 222, 411, 421)] +
                 [(1, k, True) for k in (211, 212, 221, 222, 231, 241)])
# persistent (bf16, code) pairs for which the scan finds no shape with more than CUS items (see the docstring)
NO_MANY_ITEMS = {(0, 122), (1, 211)}
# kernels the scan reaches with N = 3 only
N3_ONLY = {(0, 4)}


def _w(kernel, reducer, N, dims, Cin, Cout, accumulate):
    return Wgrad(kernel, reducer, int(WGRAD_KERNELS[kernel] >= 3), N, dims[0], dims[1], dims[2], Cin, Cout, accumulate)


WGRAD_CASES = [
    # fp32 4 x 4 x 8 tile: the default, and the fallback of every shape no tile divides
    _w('wgrad2_4x4x8', 4, 3, (5, 7, 9), 20, 36, 0),
    _w('wgrad2_4x4x8', 4, 1, (4, 8, 16), 40, 24, 1),
    _w('wgrad2_4x4x8', 16, 3, (13, 9, 25), 36, 40, 1),            # 144 tiles in 64 slabs: not a divisor
    _w('wgrad2_4x4x8', 16, 2, (8, 16, 32), 8, 72, 0),
    _w('wgrad2_4x4x8', 4, 1, (3, 4, 7), 36, 20, 0),               # one tile, one slab
    _w('wgrad2_4x4x4', 4, 3, (4, 8, 12), 20, 36, 0),
    _w('wgrad2_4x4x4', 4, 1, (8, 4, 4), 36, 12, 1),
    _w('wgrad2_4x4x4', 16, 3, (8, 16, 12), 24, 40, 1),
    _w('wgrad2_4x4x4', 16, 2, (8, 16, 20), 8, 36, 0),
    _w('wgrad2_2x6x6', 4, 3, (2, 6, 6), 20, 36, 0),               # 3 tiles in 2 slabs
    _w('wgrad2_2x6x6', 4, 1, (6, 12, 18), 36, 12, 1),
    _w('wgrad2_2x6x6', 16, 3, (6, 18, 18), 24, 20, 1),            # 81 tiles in 41 slabs
    _w('wgrad2_2x6x6', 16, 2, (8, 12, 30), 12, 72, 0),
    # bf16 MFMA kernel, whole tiles
    _w('wgrad3_8', 4, 3, (4, 8, 16), 24, 40, 0),
    _w('wgrad3_8', 4, 1, (8, 8, 8), 40, 16, 1),
    _w('wgrad3_8', 16, 3, (8, 12, 32), 16, 72, 1),
    _w('wgrad3_8', 16, 2, (8, 16, 32), 72, 24, 0),
    _w('wgrad3_4', 4, 3, (4, 8, 12), 24, 40, 0),
    _w('wgrad3_4', 4, 1, (8, 4, 4), 40, 16, 1),                   # one slab
    _w('wgrad3_4', 16, 3, (8, 16, 12), 16, 72, 1),
    _w('wgrad3_4', 16, 2, (8, 16, 20), 72, 24, 0),
    # bf16 MFMA kernel, IRR: ragged in z only, y only, x only, all three
    _w('wgrad3_8_irr', 4, 3, (5, 8, 16), 24, 40, 0),
    _w('wgrad3_8_irr', 4, 1, (4, 7, 16), 40, 24, 1),
    _w('wgrad3_8_irr', 4, 1, (4, 8, 13), 8, 72, 0),
    _w('wgrad3_8_irr', 4, 3, (5, 7, 13), 40, 24, 1),
    _w('wgrad3_8_irr', 16, 3, (9, 11, 29), 24, 40, 1),
    _w('wgrad3_8_irr', 16, 3, (8, 12, 31), 16, 72, 0),
    _w('wgrad3_4_irr', 4, 3, (5, 8, 12), 24, 40, 0),
    _w('wgrad3_4_irr', 4, 1, (4, 7, 12), 40, 24, 1),
    _w('wgrad3_4_irr', 4, 1, (4, 8, 9), 8, 72, 0),
    _w('wgrad3_4_irr', 4, 3, (5, 7, 9), 40, 24, 1),
    _w('wgrad3_4_irr', 16, 3, (9, 11, 17), 24, 40, 1),            # 135 tiles in 68 slabs
    _w('wgrad3_4_irr', 16, 3, (8, 12, 17), 16, 72, 0),
    # bf16 operands widened while staging (a channel count that is not a multiple of 8), 4 x 4 x 8 tiles
    _w('widening', 4, 3, (5, 7, 9), 20, 36, 0),
    _w('widening', 4, 1, (4, 8, 16), 36, 12, 1),                  # one slab
    _w('widening', 16, 3, (13, 9, 25), 12, 40, 1),
    _w('widening', 16, 3, (9, 13, 33), 44, 20, 0),
]

ALL_WGRAD_CODES = sorted(10 * k + r for k in range(8) for r in (0, 1))
WGRAD_TILES = {0: (4, 4, 8), 1: (4, 4, 4), 2: (2, 6, 6), 3: (4, 4, 8), 4: (4, 4, 8), 5: (4, 4, 4), 6: (4, 4, 4), 7: (4, 4, 8)}


def wgrad_tiles(c):
    tz, ty, tx = WGRAD_TILES[WGRAD_KERNELS[c.kernel]]
    return c.N * (-(-c.D // tz)) * (-(-c.H // ty)) * (-(-c.W // tx))


# argument sets the launchers refuse: (entry point family, (N, D, H, W, Cin, Cout), what is wrong)
#   'fp32' seg3d_conv3d_k3_mfma_fwd, 'bf16' seg3d_conv3d_k3_bf16_fwd; '*_no_ws': a split-K shape called with workspace = NULL
REFUSALS = [
    ('fp32', (1, 5, 5, 5, 10, 16), 'Cin % 4 != 0'),
    ('bf16', (1, 5, 5, 5, 24, 16), 'bf16 with Cin % 16 != 0'),
    ('bf16', (1, 5, 5, 5, 16, 6), 'bf16 with Cout % 4 != 0'),
    ('fp32_no_ws', (3, 7, 25, 9, 64, 4), 'fp32 split-K without a workspace'),
    ('bf16_no_ws', (1, 5, 5, 5, 128, 4), 'bf16 split-K without a workspace'),
]
