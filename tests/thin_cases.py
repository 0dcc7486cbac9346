"""The case table of the thin 3x3x3 kernel family (csrc/conv_thin.hip and csrc/conv_thin_f32.hip: the stem, Cin <= 8, and the
head, Cout <= 8 -- forward / data gradient and weight gradient, fp32 and bf16 mode), shared by tests/test_thin_variants.py (host
only: every case reaches the instantiation it is named for, every instantiation is named by a case) and
tests/test_gpu_thin_float64.py (the same cases against float64 on the device).

Every instantiation of the family is selected by the entry point and the channel counts alone, so every one of them has a case
(ALL_IN 50, ALL_OUT 26, ALL_WGRAD 16, ALL_REDUCE 2), and all six z extents of the fp32 head kernel are reached through its
launcher.  Case name -> kernel, and the launcher rule behind it:

  thin_in, out_bf16 = 0 / 1   conv3d_k3_thin_in_kernel<CT> / conv3d_k3_thin_in_bf16out_kernel<CT>
                              seg3d_conv3d_k3_thin_in_fwd / _bf16out_fwd switch on CT = 1 .. 8; one 4 x 8 x 8 tile per workgroup
  persistent                  seg3d_conv3d_k3_thin_in_persistent_fwd, switch on CT = 1 .. 8 and on out_bf16;
                              Cout <= 16 and Cout % 4 == 0:  conv3d_k3_thin_in_persistent16_kernel<CT, OUT_BF>  (16-row MFMA)
                              otherwise:                     conv3d_k3_thin_in_persistent_kernel<CT, OUT_BF>    (32-row MFMA)
                              (seg3d_conv3d_k3_thin_in_persistent_variant).  grid.x = min(1024 / ceil(Cout / 32), tiles)
                              (seg3d_conv3d_k3_thin_in_persistent_workgroups): TILE_CLASS 'one' = every workgroup has one tile,
                              'many' = more tiles than workgroups and not a multiple -- the walk prefetches the next halo, keeps
                              per-wave statistics across tiles, and some workgroups take one tile more than others.
                              `regular` = whole 4 x 8 x 8 tiles; the 32-row body's `fast` epilogue = regular and Cout % 8 == 0
  mfma16                      conv3d_k3_thin_in_mfma16_kernel<CT>, CT in {1, 2}, Cout % 4 == 0, bf16 output
  thin_out / thin_out_bf16    conv3d_k3_thin_out_kernel<CO> / conv3d_k3_thin_out_bf16_kernel<CO>: CO in {2, 4, 8} is an argument,
                              Cout <= CO, Cin % 4 == 0 (Cin % 8 == 4: the last 8-channel chunk is half empty); tile 8 x 8 x 16
  thin_out_mfma               conv3d_k3_thin_out_mfma_kernel<Cin, CO>: Cin in {16, 32}, CO = 2 for Cout <= 2, else 3; bf16 x
  thin_out_f32mfma            conv3d_k3_thin_out_f32mfma_kernel<Cin, CO, RING>: Cin in {16, 32}, CO = 2 for Cout <= 2, else Cout
                              (<= 5).  Each (Cin, CO) has two tile bodies: MASKED for a wave's tile at either x end of the
                              volume, the plain one for an interior tile -- which exists only when W >= 33.  The z extent tz of a
                              tile comes from the cost model thin_out_f32_tz (seg3d_conv3d_k3_thin_out_f32mfma_tz):
                              ceil(tiles / 1024) * (tz + 2.5), times 1.2 up to 1024 tiles, so tz = 8 for every shape with at most
                              1024 tiles of 8 x 8 x 16; many samples of thin columns reach the other five cheaply
  wgrad, fat_bf16 = 0 / 1     k3_thin_wgrad_kernel<CT> / k3_thin_wgrad_bf16_mfma_kernel<CT> (seg3d_k3_thin_wgrad / _fatbf16, switch
                              on CT = 1 .. 8), then k3_thin_wgrad_reduce_kernel.  slabs = min(ceil(tiles / 8), 512) of 4 x 8 x 8
                              tiles = seg3d_k3_thin_wgrad_workspace_floats / (CFB * RB * 1024); the reduce kernel's threads stride
                              the slabs by 64: REDUCE 'le64' is one trip, 'gt64' a second one.  SLAB_CLASS: '1', 'few' (2 .. 64),
                              'many' (65 .. 511), 'cap' (512: more than 8 tiles per slab).
                              conv 'stem': thin = x, fat = dy, s_ct = 27, s_cf = 27 CT, flip = 0;
                              conv 'head': thin = dy, fat = x, s_ct = 27 CF, s_cf = 27, flip = 1

role 'fwd': plain pack of w[Cout][Cin][27]; 'dgrad': flip = 1 pack of the forward layer's weight with the transposed strides.
full = 1: bias and statistics are passed; full = 0: both NULL.

The forward edges (both roles, full and bare, N = 1 and N = 3, a shape smaller than one tile, ragged in z / y / x only, ragged in
all three, whole tiles) are read per kernel BODY -- the template, whose CT / CO / Cin instantiations share every line of the tile
and edge handling -- not per instantiation: thin_in<CT> has two cases per CT, and the eight CT together carry the set.  Within a
body every shape class meets full = 1 and full = 0 and both roles (_edge), so bias and statistics are checked on x-ragged,
all-ragged and whole tiles as well as on the small and z / y-ragged ones; every instantiation runs both roles.  What is particular
to a body (every CT on each persistent body, the mask-only and the interior shape of every (Cin, CO), ...) is listed per body.  tests/test_thin_variants.py asserts the spread.  Size limit: at most 20M elements per tensor.
"""
from collections import namedtuple

In = namedtuple('In', 'kernel CT out_bf16 N D H W Cout role full')
Out = namedtuple('Out', 'kernel N D H W Cin Cout CO role full tz')
Wg = namedtuple('Wg', 'fat_bf16 CT CF N D H W conv accumulate slabs')

MAX_ELEMS = 20_000_000
IN_TILE, OUT_TILE = (4, 8, 8), (8, 8, 16)
TZ_VALUES = (8, 12, 16, 24, 32, 48)
WG_CAP = 1024            # persistent workgroups per Cout block row: 1024 / cobs
TILES_PER_SLAB, REDUCE_STRIDE, SLAB_CAP = 8, 64, 512

ALL_IN = sorted([('thin_in', ct) for ct in range(1, 9)] + [('thin_in_bf16out', ct) for ct in range(1, 9)] +
                [(k, ct, bf) for k in ('thin_in_persistent', 'thin_in_persistent16') for ct in range(1, 9) for bf in (0, 1)] +
                [('thin_in_mfma16', 1), ('thin_in_mfma16', 2)], key=str)
ALL_OUT = sorted([(k, co) for k in ('thin_out', 'thin_out_bf16') for co in (2, 4, 8)] +
                 [('thin_out_mfma', ci, co) for ci in (16, 32) for co in (2, 3)] +
                 [('thin_out_f32mfma', ci, co, m) for ci in (16, 32) for co in (2, 3, 4, 5) for m in ('masked', 'plain')], key=str)
ALL_WGRAD = sorted([(k, ct) for k in ('k3_thin_wgrad', 'k3_thin_wgrad_bf16_mfma') for ct in range(1, 9)])
ALL_REDUCE = ['gt64', 'le64']


def case_id(c):
    return type(c).__name__.lower() + '-' + '-'.join(str(v) for v in c)


def cdiv(a, b):
    return -(-a // b)


def tiles(c, tile):
    return c.N * cdiv(c.D, tile[0]) * cdiv(c.H, tile[1]) * cdiv(c.W, tile[2])


def shape_class(c, tile):
    """'small' (inside one tile in every axis), 'whole', 'z' / 'y' / 'x' (ragged on that axis only), 'all', or 'mixed'"""
    if c.D < tile[0] and c.H < tile[1] and c.W < tile[2]:
        return 'small'
    off = (c.D % tile[0] != 0, c.H % tile[1] != 0, c.W % tile[2] != 0)
    return {(False, False, False): 'whole', (True, False, False): 'z', (False, True, False): 'y', (False, False, True): 'x',
            (True, True, True): 'all'}.get(off, 'mixed')


SHAPE_CLASSES = {'small', 'whole', 'z', 'y', 'x', 'all'}


# ---- thin-in ---------------------------------------------------------------------------------------------------------------
def persistent_rows(Cout):
    return 16 if Cout <= 16 and Cout % 4 == 0 else 32


def in_key(c):
    if c.kernel == 'thin_in':
        return ('thin_in_bf16out' if c.out_bf16 else 'thin_in', c.CT)
    if c.kernel == 'mfma16':
        return ('thin_in_mfma16', c.CT)
    return ('thin_in_persistent16' if persistent_rows(c.Cout) == 16 else 'thin_in_persistent', c.CT, c.out_bf16)


def in_body(c):
    k = in_key(c)
    return k[0] if len(k) == 2 else (k[0], k[2])


def in_regular(c):
    return shape_class(c, IN_TILE) == 'whole'


IN_BODIES = ['thin_in', 'thin_in_bf16out', 'thin_in_mfma16', ('thin_in_persistent', 0), ('thin_in_persistent', 1),
             ('thin_in_persistent16', 0), ('thin_in_persistent16', 1)]
TILE_CLASS = {}          # persistent cases: 'one' or 'many'

_IN_SHAPES = [(1, 2, 3), (5, 8, 8), (4, 9, 8), (4, 8, 11), (5, 9, 11), (4, 8, 16)]
_OUT_SHAPES = [(1, 2, 3), (9, 8, 16), (8, 9, 16), (8, 8, 17), (9, 9, 19), (8, 8, 16)]


def _edge(k):
    """the k-th combination of the common forward edges: (shape index, role, N, full).  The shape is k % 6; role and full also
    take the round k // 6, so that a body's twelve or more consecutive k pair every shape with both roles and with full = 1 and
    full = 0 (the statistics of an x-ragged, an all-ragged and a whole tile are checked, not only those of the first three shapes).
    k and k + 1 differ in role when k is even"""
    rnd = k // 6
    return k % 6, ('fwd', 'dgrad')[(k + rnd) % 2], (1, 3)[(k // 2) % 2], (1, 0)[(k // 3 + rnd) % 2]


def _in(kernel, CT, out_bf16, N, dims, Cout, role, full, tile_class=None):
    c = In(kernel, CT, out_bf16, N, dims[0], dims[1], dims[2], Cout, role, full)
    if kernel == 'persistent':
        TILE_CLASS[c] = tile_class or 'one'
    return c


IN_CASES = []
# one-tile-per-workgroup kernels: two cases per instantiation; Cout a multiple of 32, a partial last block, <= 16 in fours, and 6
# (element stores)
_COUTS = [32, 20, 48, 16, 4, 64, 12, 8, 6]
for _bf in (0, 1):
    for _ct in range(1, 9):
        for _j in range(2):
            _k = 2 * (_ct - 1) + _j
            _s, _role, _n, _full = _edge(_k)
            IN_CASES.append(_in('thin_in', _ct, _bf, _n, _IN_SHAPES[_s], _COUTS[(_k + 4 * _bf) % 9], _role, _full))
# bf16 matrix cores, CT in {1, 2}, Cout % 4 == 0
_COUTS16 = [16, 32, 20, 48, 4, 12, 8, 64]
for _ct in (1, 2):
    for _j in range(8):
        _s, _role, _n, _full = _edge(_j + 8 * (_ct - 1))
        IN_CASES.append(_in('mfma16', _ct, 1, _n, _IN_SHAPES[_s], _COUTS16[(_j + 3 * (_ct - 1)) % 8], _role, _full))
# persistent walk: every CT on each of the four bodies, one tile per workgroup
_COUTS_P32 = [32, 20, 48, 64, 6, 40]
_COUTS_P16 = [16, 4, 12, 8]
for _bf in (0, 1):
    for _ct in range(1, 9):
        for _j in range(2):
            _k = 2 * (_ct - 1) + _j
            _s, _role, _n, _full = _edge(_k)
            IN_CASES.append(_in('persistent', _ct, _bf, _n, _IN_SHAPES[_s], _COUTS_P32[(_k + _k // 6 + _bf) % 6], _role, _full))
            _s, _role, _n, _full = _edge(_k + 4)
            IN_CASES.append(_in('persistent', _ct, _bf, _n, _IN_SHAPES[_s], _COUTS_P16[(_k + _k // 4 + _bf) % 4], _role, _full))
for _bf in (0, 1):
    IN_CASES += [
        # `regular`: the fast epilogue of the 32-row body (Cout % 8 == 0: 32, and 48 with two quads in the last block) and its
        # element-wise one (20); the 16-row body with Cout 16 and 12
        _in('persistent', 4 - _bf, _bf, 1, (4, 8, 16), 32, 'fwd', 1),
        _in('persistent', 5 + _bf, _bf, 3, (8, 8, 8), 48, 'dgrad', 1),
        _in('persistent', 2 + _bf, _bf, 1, (4, 16, 8), 20, 'fwd', 1),
        _in('persistent', 7 - _bf, _bf, 1, (8, 8, 8), 16, 'dgrad', 0),
        _in('persistent', 3 + _bf, _bf, 3, (4, 8, 16), 12, 'fwd', 1),
        # more tiles than workgroups, not a multiple, ragged at the end: 1155 tiles on 1024, 550 on 512 (two Cout blocks), 1188 on
        # 1024 -- one even and one odd CT per body -- and a regular volume of 880 tiles on 512 for the fast epilogue
        _in('persistent', 3 + 2 * _bf, _bf, 3, (27, 37, 83), 20, 'fwd', 1, 'many'),
        _in('persistent', 2 + 2 * _bf, _bf, 2, (19, 40, 88), 48, 'dgrad', 1, 'many'),
        _in('persistent', 6 - 4 * _bf, _bf, 1, (44, 64, 80), 48, 'fwd', 1, 'many'),
        _in('persistent', 1 + 6 * _bf, _bf, 3, (27, 37, 83), 16, 'dgrad', 1, 'many'),
        _in('persistent', 8 - 4 * _bf, _bf, 1, (45, 65, 81), 12, 'fwd', 1, 'many'),
    ]


# ---- thin-out --------------------------------------------------------------------------------------------------------------
def f32_co(Cout):
    return 2 if Cout <= 2 else Cout


def out_keys(c):
    """the instantiations a case runs (an fp32 MFMA case with W >= 33 runs both tile bodies)"""
    if c.kernel in ('thin_out', 'thin_out_bf16'):
        return [(c.kernel, c.CO)]
    if c.kernel == 'thin_out_mfma':
        return [(c.kernel, c.Cin, c.CO)]
    return [(c.kernel, c.Cin, c.CO, 'masked')] + ([(c.kernel, c.Cin, c.CO, 'plain')] if c.W >= 33 else [])


OUT_BODIES = ['thin_out', 'thin_out_bf16', 'thin_out_mfma', 'thin_out_f32mfma']


def _out(kernel, N, dims, Cin, Cout, CO, role, full, tz=0):
    return Out(kernel, N, dims[0], dims[1], dims[2], Cin, Cout, CO, role, full, tz if kernel != 'thin_out_f32mfma' else (tz or 8))


OUT_CASES = []
# VALU kernels: six cases per instantiation; Cout < CO and Cout == CO, Cin % 8 == 4 and Cin % 8 == 0
_COUT_OF = {2: [1, 2, 2, 1, 2, 1], 4: [3, 4, 1, 4, 3, 2], 8: [5, 8, 6, 7, 8, 3]}
_CINS = [12, 16, 20, 8, 32, 4]
for _i, _kern in enumerate(('thin_out', 'thin_out_bf16')):
    for _ci, _co in enumerate((2, 4, 8)):
        for _j in range(6):
            _s, _role, _n, _full = _edge(6 * _ci + _j)
            OUT_CASES.append(_out(_kern, _n, _OUT_SHAPES[_s], _CINS[(_j + _ci + _i) % 6], _COUT_OF[_co][_j], _co, _role, _full))
# matrix-core kernels: per (Cin, CO) the common edges on mask-only shapes (W <= 32), then shapes with an interior x tile (W >= 33);
# Cout = 1 on the two-class instantiation, Cout = 2 with W odd and even (the 16-byte pair store)
for _i, _cin in enumerate((16, 32)):
    for _ci, _co in enumerate((2, 3)):
        for _j in range(6):
            _s, _role, _n, _full = _edge(6 * (2 * _i + _ci) + _j)
            _cout = _co if _co == 3 else (1 if _j == 2 else 2)
            OUT_CASES.append(_out('thin_out_mfma', _n, _OUT_SHAPES[_s], _cin, _cout, _co, _role, _full))
        OUT_CASES.append(_out('thin_out_mfma', 1, (3, 9, 35), _cin, _co, _co, 'fwd', 1))
        OUT_CASES.append(_out('thin_out_mfma', 2, (9, 5, 48), _cin, _co, _co, 'dgrad', 0))
        if _co == 2:
            OUT_CASES.append(_out('thin_out_mfma', 1, (2, 3, 34), _cin, 1, _co, ('fwd', 'dgrad')[_i], 1))
    for _ci, _co in enumerate((2, 3, 4, 5)):
        for _j in range(3):
            _s, _role, _n, _full = _edge(3 * (4 * _i + _ci) + _j)
            _cout = _co if _co > 2 else (1 if _j == 1 else 2)
            OUT_CASES.append(_out('thin_out_f32mfma', _n, _OUT_SHAPES[_s], _cin, _cout, _co, _role, _full))
        OUT_CASES.append(_out('thin_out_f32mfma', 1, (3, 9, 35), _cin, _co, _co, 'dgrad', 1))
        OUT_CASES.append(_out('thin_out_f32mfma', 2, (9, 5, 48), _cin, _co, _co, 'fwd', 0))
        if _co == 2:
            OUT_CASES.append(_out('thin_out_f32mfma', 1, (2, 3, 34), _cin, 1, _co, ('fwd', 'dgrad')[_i], 1))
OUT_CASES += [
    # z extents beyond 8: more than 1024 tiles of thin columns, D not a multiple of tz (a short last march) ...
    _out('thin_out_f32mfma', 342, (17, 3, 5), 16, 2, 2, 'fwd', 1, 12),
    _out('thin_out_f32mfma', 342, (17, 3, 5), 32, 5, 5, 'dgrad', 0, 12),
    _out('thin_out_f32mfma', 769, (25, 3, 5), 16, 3, 3, 'dgrad', 1, 16),
    _out('thin_out_f32mfma', 769, (25, 3, 5), 32, 4, 4, 'fwd', 1, 16),
    _out('thin_out_f32mfma', 854, (41, 3, 5), 16, 4, 4, 'fwd', 1, 24),
    _out('thin_out_f32mfma', 878, (49, 3, 5), 16, 5, 5, 'dgrad', 1, 32),
    _out('thin_out_f32mfma', 878, (81, 3, 5), 16, 2, 2, 'fwd', 1, 48),
    # ... D a multiple of tz ...
    _out('thin_out_f32mfma', 342, (24, 3, 5), 32, 3, 3, 'fwd', 1, 12),
    _out('thin_out_f32mfma', 769, (32, 3, 5), 16, 1, 2, 'dgrad', 1, 16),
    # ... and with an interior x tile
    _out('thin_out_f32mfma', 114, (17, 3, 34), 32, 2, 2, 'fwd', 1, 12),
    _out('thin_out_f32mfma', 257, (25, 2, 33), 16, 5, 5, 'dgrad', 1, 16),
]


# ---- weight gradient -------------------------------------------------------------------------------------------------------
def wg_key(c):
    return ('k3_thin_wgrad_bf16_mfma' if c.fat_bf16 else 'k3_thin_wgrad', c.CT)


def slab_class(slabs):
    return '1' if slabs == 1 else 'few' if slabs <= REDUCE_STRIDE else 'many' if slabs < SLAB_CAP else 'cap'


def reduce_class(c):
    return 'le64' if c.slabs in ('1', 'few') else 'gt64'


def _wg(fat_bf16, CT, CF, N, dims, conv, accumulate, slabs):
    return Wg(fat_bf16, CT, CF, N, dims[0], dims[1], dims[2], conv, accumulate, slabs)


WGRAD_CASES = []
_CFS = [4, 20, 32, 48]
_WG_SHAPES = [((1, 2, 3), 1, '1'), ((5, 9, 11), 3, 'few'), ((4, 8, 16), 1, '1'), ((9, 17, 19), 1, 'few'), ((8, 16, 24), 3, 'few'),
              ((4, 8, 8), 3, '1')]
for _fb in (0, 1):
    for _ct in range(1, 9):
        for _j in range(3):
            _k = 3 * (_ct - 1) + _j + _fb
            _dims, _n, _sl = _WG_SHAPES[_k % 6]
            WGRAD_CASES.append(_wg(_fb, _ct, _CFS[(_k + _fb) % 4], _n, _dims, ('stem', 'head')[(_k + _j // 2) % 2], (_k // 2) % 2, _sl))
for _fb in (0, 1):
    WGRAD_CASES += [
        # a second trip of the reduce loop: 72 slabs (regular), 145 (ragged); the 512-slab cap with 4410 tiles
        _wg(_fb, 2 + _fb, 32, 1, (32, 64, 72), 'stem', _fb, 'many'),
        _wg(_fb, 5 - _fb, 20, 1, (32, 64, 72), 'head', 1 - _fb, 'many'),
        _wg(_fb, 3 + 4 * _fb, 48, 3, (27, 37, 83), 'head', 1, 'many'),
        _wg(_fb, 8 - 4 * _fb, 4, 3, (27, 37, 83), 'stem', 0, 'many'),
        _wg(_fb, 1 + 5 * _fb, 32, 70, (9, 17, 50), 'head', _fb, 'cap'),
        _wg(_fb, 6 - 5 * _fb, 20, 70, (9, 17, 50), 'stem', 1 - _fb, 'cap'),
    ]


# ---- refusals: (entry point -- its message starts with this name, which call, arguments, what is wrong) --------------------------
#   'in'    (CT, Cout)        seg3d_conv3d_k3_thin_in_fwd / seg3d_conv3d_k3_thin_in_persistent_fwd / seg3d_conv3d_k3_thin_in_mfma16_fwd
#   'out'   (Cin, Cout, CO)   seg3d_conv3d_k3_thin_out_fwd; (Cin, Cout) for the two matrix-core entries
#   'wgrad' (CT, CF)          seg3d_k3_thin_wgrad
REFUSALS = [
    ('seg3d_conv3d_k3_thin_in_fwd', 'in', (0, 16), 'CT = 0'),
    ('seg3d_conv3d_k3_thin_in_fwd', 'in', (9, 16), 'CT = 9'),
    ('seg3d_conv3d_k3_thin_in_persistent_fwd', 'in', (0, 16), 'persistent CT = 0'),
    ('seg3d_conv3d_k3_thin_in_persistent_fwd', 'in', (9, 32), 'persistent CT = 9'),
    ('seg3d_conv3d_k3_thin_in_mfma16_fwd', 'in', (3, 16), 'thin_in_mfma16 with CT = 3'),
    ('seg3d_conv3d_k3_thin_out_fwd', 'out', (10, 2, 2), 'thin-out Cin % 4 != 0'),
    ('seg3d_conv3d_k3_thin_out_fwd', 'out', (16, 5, 4), 'thin-out Cout > CO'),
    ('seg3d_conv3d_k3_thin_out_fwd', 'out', (16, 3, 3), 'thin-out CO = 3'),
    ('seg3d_conv3d_k3_thin_out_mfma_fwd', 'out', (32, 4), 'thin_out_mfma with Cout = 4'),
    ('seg3d_conv3d_k3_thin_out_mfma_fwd', 'out', (24, 2), 'thin_out_mfma with Cin = 24'),
    ('seg3d_conv3d_k3_thin_out_f32mfma_fwd', 'out', (32, 6), 'thin_out_f32mfma with Cout = 6'),
    ('seg3d_conv3d_k3_thin_out_f32mfma_fwd', 'out', (24, 2), 'thin_out_f32mfma with Cin = 24'),
    ('seg3d_k3_thin_wgrad', 'wgrad', (0, 16), 'wgrad CT = 0'),
    ('seg3d_k3_thin_wgrad', 'wgrad', (9, 16), 'wgrad CT = 9'),
    ('seg3d_k3_thin_wgrad', 'wgrad', (2, 18), 'wgrad CF % 4 != 0'),
]
