"""The case table of the stride-2 2x2x2 kernel family (csrc/conv_k2_mfma.hip), shared by tests/test_k2_variants.py (host only:
every case maps to the kernel instantiation it is named for, every instantiation is named by a case) and
tests/test_gpu_k2_float64.py (the same cases against float64 on the device).

The variant codes are those of include/seg3d_hip.h:
  gather   100 x_mode + 10 out_bf16 + k         k: 0 staged, 1 direct<1,1>, 2 direct<2,1>, 3 direct<1,4>
  scatter  100 x_mode + 10 out_bf16 + 4 direct + 2 ADD + PAIR
  wgrad    10 k + r                              k: 0 mfma<false>, 1 pair, 2 bf16_mfma, 3 mfma<true>;  r: 1 reduce4, 0 reduce
Extents are COARSE (the conv's output / the transposed conv's input / Q of the weight gradient); the fine side is twice that.
"""
from collections import namedtuple

GATHER_KERNELS = {'staged': 0, 'direct_1_1': 1, 'direct_2_1': 2, 'direct_1_4': 3}
WGRAD_KERNELS = {'mfma_f32': 0, 'pair': 1, 'bf16_mfma': 2, 'mfma_bf16in': 3}
MODE_PAIRS = [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1)]      # (x_mode, out_bf16) the entry points can express

# role 'fwd': bias + GroupNorm statistics; 'dgrad': the data-gradient role, bias = NULL and stats = NULL.  ld_x > 0: x is the channel
# slice of a [.., ld_x] buffer (seg3d_conv3d_k2s2_mfma_fwd_ld)
Gather = namedtuple('Gather', 'kernel mode out_bf16 N D H W Cin Cout role ld_x')
# addend: ld_addend (> Cout: a channel slice) or 0 = none; an addend implies the data-gradient role
Scatter = namedtuple('Scatter', 'direct add pair mode out_bf16 N D H W Cin Cout role ld_addend')
# swapped: dw[a * 8 CB + b * 8 + t] instead of dw[a * 8 + b * 8 CA + t]
Wgrad = namedtuple('Wgrad', 'kernel reduce4 bf16 N D H W CA CB accumulate swapped')


def gather_code(c):
    return 100 * c.mode + 10 * c.out_bf16 + GATHER_KERNELS[c.kernel]


def scatter_code(c):
    return 100 * c.mode + 10 * c.out_bf16 + 4 * int(c.direct) + 2 * int(c.add) + int(c.pair)


def wgrad_code(c):
    return 10 * WGRAD_KERNELS[c.kernel] + int(c.reduce4)


def case_id(c):
    vals = [('T' if v else 'F') if isinstance(v, bool) else str(v) for v in c]
    return type(c).__name__.lower() + '-' + '-'.join(vals)


def _g(kernel, pair, N, dims, Cin, Cout, role, ld_x=0):
    return Gather(kernel, pair[0], pair[1], N, dims[0], dims[1], dims[2], Cin, Cout, role, ld_x)


P00, P10, P11, P20, P21 = MODE_PAIRS
GATHER_CASES = [
    # LDS-staged kernel: an odd number of chunks (8 channels; mode 2: 16)
    _g('staged', P00, 3, (5, 7, 9), 24, 20, 'fwd'),
    _g('staged', P00, 1, (3, 4, 6), 8, 36, 'fwd', ld_x=16),
    _g('staged', P10, 1, (3, 4, 6), 40, 36, 'dgrad'),
    _g('staged', P10, 3, (1, 3, 5), 20, 8, 'fwd'),              # three chunks, the last one partial; 40-byte bf16 rows
    _g('staged', P11, 3, (1, 3, 33), 8, 16, 'fwd'),
    _g('staged', P20, 1, (5, 7, 9), 48, 40, 'fwd'),
    _g('staged', P21, 3, (2, 3, 5), 16, 12, 'dgrad'),
    # direct kernel, one column block per wave, whole K per wave
    _g('direct_1_1', P00, 3, (5, 7, 9), 16, 32, 'fwd'),
    _g('direct_1_1', P00, 1, (3, 5, 6), 12, 20, 'fwd', ld_x=20),   # the last chunk is partial
    _g('direct_1_1', P00, 1, (1, 3, 40), 16, 72, 'dgrad'),
    _g('direct_1_1', P10, 1, (3, 4, 6), 12, 24, 'dgrad'),           # 24-byte bf16 rows
    _g('direct_1_1', P11, 3, (3, 1, 9), 16, 8, 'fwd'),
    _g('direct_1_1', P20, 1, (5, 7, 9), 32, 32, 'fwd'),
    _g('direct_1_1', P21, 3, (2, 3, 5), 32, 20, 'dgrad'),
    # direct kernel, K split over the four waves of a workgroup: chunk count % 4 == 0, fewer than 3072 waves
    _g('direct_1_4', P00, 1, (5, 7, 9), 32, 96, 'dgrad'),
    _g('direct_1_4', P00, 3, (1, 3, 5), 28, 12, 'fwd'),            # the last chunk is partial
    _g('direct_1_4', P10, 3, (2, 3, 5), 64, 40, 'fwd'),
    _g('direct_1_4', P11, 1, (3, 4, 6), 32, 16, 'dgrad'),
    _g('direct_1_4', P20, 1, (3, 5, 9), 64, 64, 'fwd'),
    _g('direct_1_4', P21, 3, (1, 3, 5), 128, 36, 'fwd'),
    # direct kernel, two column blocks per wave: Cout % 64 == 0 and at least 16384 waves ((1, 1, W) extents: 32-voxel tiles)
    _g('direct_2_1', P00, 1, (1, 1, 16384), 16, 256, 'fwd'),
    _g('direct_2_1', P00, 2, (32, 128, 8), 16, 256, 'dgrad'),      # 128-voxel tiles with all three extents above 1
    _g('direct_2_1', P10, 3, (1, 1, 7290), 16, 192, 'dgrad'),      # three column-block pairs, a ragged last tile
    _g('direct_2_1', P11, 1, (1, 1, 16380), 16, 256, 'fwd'),
    _g('direct_2_1', P20, 1, (1, 1, 16384), 32, 256, 'fwd'),
    _g('direct_2_1', P21, 1, (1, 1, 16384), 32, 256, 'dgrad'),
]


def _s(direct, add, pair, mp, N, dims, Cin, Cout, role='fwd', extra=0):
    if add:
        role = 'dgrad'
    return Scatter(direct, add, pair, mp[0], mp[1], N, dims[0], dims[1], dims[2], Cin, Cout, role, Cout + extra if add else 0)


SCATTER_CASES = []
for _mp in (P00, P10, P20):
    _c = 64 if _mp[0] == 2 else 32
    SCATTER_CASES += [
        # direct kernel (fp32 y): whole steps of four chunks, Cout 16 (tap pairs) or whole column blocks
        _s(True, False, False, _mp, 1, (5, 7, 9), _c, 64, 'fwd'),
        _s(True, False, True, _mp, 3, (3, 5, 6), _c, 16, 'dgrad' if _mp[0] == 1 else 'fwd'),
        _s(True, True, False, _mp, 3, (5, 7, 9), _c, 32, extra=8),
        _s(True, True, True, _mp, 1, (3, 5, 6), _c, 16, extra=16),
    ]
SCATTER_CASES += [
    _s(True, False, False, P00, 1, (2, 3, 5), 64, 96, 'dgrad'),         # three column blocks, eight steps
    # staged kernel with fp32 y: one case for each reason the direct kernel is not eligible
    _s(False, False, False, P00, 1, (1, 1, 8192), 32, 32, 'fwd'),       # a grid of 256 workgroups
    _s(False, False, False, P10, 3, (5, 7, 9), 16, 20, 'fwd'),          # Cin 16: not whole steps; Cout % 8 != 0 epilogue
    _s(False, False, False, P20, 1, (3, 5, 6), 48, 40, 'dgrad'),
    _s(False, False, True, P00, 3, (3, 5, 6), 32, 8, 'fwd'),            # Cout 8: tap pairs, no direct form
    _s(False, False, True, P10, 1, (5, 7, 9), 16, 16, 'dgrad'),
    _s(False, False, True, P20, 1, (3, 5, 6), 64, 8, 'fwd'),
    _s(False, True, False, P00, 1, (5, 7, 9), 16, 40, extra=8),
    _s(False, True, False, P10, 3, (3, 5, 6), 24, 24, extra=4),
    _s(False, True, False, P20, 1, (3, 5, 6), 32, 72, extra=8),
    _s(False, True, True, P00, 1, (5, 7, 9), 32, 8, extra=8),
    _s(False, True, True, P10, 3, (3, 5, 6), 32, 8, extra=4),
    _s(False, True, True, P20, 1, (3, 5, 6), 16, 16, extra=16),
    # staged kernel, bf16 y
    _s(False, False, False, P11, 3, (5, 7, 9), 32, 36, 'fwd'),
    _s(False, False, True, P11, 1, (3, 5, 6), 32, 16, 'dgrad'),
    _s(False, True, False, P11, 1, (5, 7, 9), 32, 64, extra=8),
    _s(False, True, True, P11, 3, (3, 5, 6), 16, 8, extra=8),
    _s(False, False, False, P21, 1, (5, 7, 9), 64, 32, 'dgrad'),
    _s(False, False, True, P21, 3, (3, 5, 6), 64, 16, 'fwd'),
    _s(False, True, False, P21, 3, (3, 5, 6), 64, 40, extra=8),
    _s(False, True, True, P21, 1, (5, 7, 9), 32, 16, extra=16),
]


def _w(kernel, reduce4, N, dims, CA, CB, accumulate, swapped):
    return Wgrad(kernel, reduce4, int(kernel in ('bf16_mfma', 'mfma_bf16in')), N, dims[0], dims[1], dims[2], CA, CB, accumulate, swapped)


# reduce4 needs 32 slabs: at least 125 tiles of 2 x 4 x 8 Q voxels and at most 16 channel-block pairs.
# 3 x (5, 11, 38): 3 * 3 * 3 * 5 = 135 tiles in 33 slabs (not a divisor); 2 x (6, 12, 56): 126 tiles in 32 slabs
WGRAD_CASES = [
    _w('mfma_f32', False, 3, (3, 5, 9), 20, 36, 0, False),
    _w('mfma_f32', True, 3, (5, 11, 38), 24, 16, 1, True),
    _w('mfma_f32', False, 1, (4, 8, 16), 72, 40, 1, True),
    _w('mfma_f32', True, 2, (6, 12, 56), 40, 36, 0, False),
    _w('pair', False, 3, (3, 5, 9), 16, 32, 0, False),
    _w('pair', True, 3, (5, 11, 38), 12, 20, 1, True),
    _w('pair', False, 1, (4, 8, 16), 8, 72, 1, True),
    _w('pair', True, 2, (16, 16, 16), 16, 32, 0, False),
    _w('bf16_mfma', False, 3, (3, 5, 9), 16, 32, 0, False),
    _w('bf16_mfma', True, 3, (5, 11, 38), 24, 8, 1, True),
    _w('bf16_mfma', False, 1, (4, 8, 16), 72, 40, 1, True),
    _w('bf16_mfma', True, 2, (6, 12, 56), 40, 64, 0, False),
    _w('mfma_bf16in', False, 3, (3, 5, 9), 12, 32, 0, False),
    _w('mfma_bf16in', True, 3, (5, 11, 38), 16, 20, 1, True),
    _w('mfma_bf16in', False, 1, (4, 8, 16), 68, 40, 1, True),
    _w('mfma_bf16in', True, 2, (6, 12, 56), 36, 28, 0, False),
]

ALL_GATHER_CODES = sorted(100 * m + 10 * o + k for (m, o) in MODE_PAIRS for k in range(4))
ALL_SCATTER_CODES = sorted([100 * m + 10 * o + 2 * a + p for (m, o) in MODE_PAIRS for a in (0, 1) for p in (0, 1)] +
                           [100 * m + 4 + 2 * a + p for m in (0, 1, 2) for a in (0, 1) for p in (0, 1)])
ALL_WGRAD_CODES = sorted(10 * k + r for k in range(4) for r in (0, 1))

# argument sets the launchers refuse: (family, arguments of the variant query, what is wrong)
#   gather: (N, D, H, W, Cin, Cout, x_mode, out_bf16);  scatter: (.., has_addend, ld_addend)
REFUSALS = [
    ('gather', (1, 2, 3, 4, 10, 16, 0, 0), 'Cin % 4 != 0'),
    ('scatter', (1, 2, 3, 4, 16, 10, 0, 0, 0, 0), 'Cout % 4 != 0'),
    ('gather', (1, 2, 3, 4, 24, 16, 2, 0), 'mode 2 with Cin % 16 != 0'),
    ('scatter', (1, 2, 3, 4, 24, 16, 2, 1, 0, 0), 'mode 2 with Cin % 16 != 0'),
    ('scatter', (1, 2, 3, 4, 16, 12, 0, 0, 1, 16), 'an addend with Cout % 8 != 0'),
    ('scatter', (1, 2, 3, 4, 16, 16, 1, 0, 1, 12), 'an addend with ld_addend < Cout'),
    ('scatter', (1, 2, 3, 4, 16, 16, 0, 1, 1, 24), 'an addend with x_mode 0 and a bf16 output'),
]
