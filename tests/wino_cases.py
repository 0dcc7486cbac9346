"""The case table of the Winograd 3x3x3 kernel family (csrc/conv_wino.hip: F(2, 3) / F(3, 2) along x; csrc/conv_wino2d.hip:
F(2x2, 3x3) / F(3x3, 2x2) over (y, x) -- the C -> C layers' forward, data gradient and weight gradient), shared by
tests/test_wino_variants.py (host only: every case reaches the kernel and the class it is named for, every kernel and class is
named by a case) and tests/test_gpu_wino_float64.py (the same cases against float64 on the device).  The table is written for the
256 CUs of the MI355X, which is also what the queries assume without a device.

Every instantiation a launcher can select, and the rule that selects it (body -> kernel):

  wino      conv3d_k3_wino_kernel                  seg3d_conv3d_k3_wino_fwd: whole 8^3 tiles, Cin % 8 == 0, Cout % 32 == 0; one
                                                   instantiation (bias, addend and statistics are run-time pointers); K chunks of 8
  tile      conv3d_k3_wino2d_kernel<BIAS, ADD>     seg3d_conv3d_k3_wino2d_fwd(_ws): whole 8^3 tiles (w2_tiles; variant 8), BIAS / ADD =
                                                   the pointer is not null: four instantiations; K chunks of 4; sk_per = 0: every
                                                   workgroup walks whole items -- a null workspace, or w2_sk_per declines
  tile_sk   the same four with sk_per > 0, then    a workspace is passed and w2_sk_per (seg3d_conv3d_k3_wino2d_fwd_sk_chunks) > 0: at
            conv3d_k3_wino2d_sk_finish_kernel      least 256 items, Cin >= 32, the plain walk would fill at most W2_SK_FILL = 0.94 of
                                                   its CU rounds; ranges of sk_per chunks (a multiple of Cin / 16), an item is cut at
                                                   most once, the finish kernel adds the two pieces of each cut item
  c4_4      conv3d_k3_wino2d_c4_kernel<B, A, 4>    whole 4^3 cells that are not whole 8^3 tiles; four cells per item where that makes
  c4_2      conv3d_k3_wino2d_c4_kernel<B, A, 2>    at least 192 items (w2_cells_per_item; variant 4), else two (variant 2): 8 in all
  wgrad, form 'wino'     conv3d_k3_wgrad_wino_kernel<4, 4, 8> (W % 8 == 0; k = 0) or <4, 4, 4> (k = 1), then
                         conv3d_k3_wgrad_wino_reduce_kernel<8> (32 slabs or more; r = 1) or <4> (r = 0): wn_wgrad_plan, and
                         seg3d_conv3d_k3_wino_wgrad_variant = 10 k + r
  wgrad, form 'wino2d'   conv3d_k3_wgrad_wino2d_kernel (k = 0), then conv3d_k3_wgrad_wino2d_reduce16_kernel<16> (64 slabs or more;
                         r = 1) or <4> (r = 0): g2_slabs, seg3d_conv3d_k3_wino2d_wgrad_variant
  What can never run: conv3d_k3_wgrad_wino2d_il_kernel is compiled only with G2_INLOOP == 1, and G2_INLOOP is 0 (it measured 4 %
  slower and is kept as a reproducible negative result) -- it has no case and no test.

role 'fwd': plain pack of w[Cout][Cin][27] (T = 36 for wino, 48 for the others); 'dgrad': flip = 1 pack of the forward layer's
weight with the transposed strides, as in tests/thin_cases.py.  bias / addend / stats: the pointer is passed, or NULL.  ws (tile
bodies): the workspace is passed.

Forward classes are read per kernel BODY (wino, tile, tile_sk, c4_4, c4_2): each has both roles, all four bias / addend
combinations, statistics and none, N = 1 and N >= 2, and
  ITEMS against the 256 workgroups: 'fewer' (< 256: one item each), 'many' (more, and not a multiple: some workgroups take one item
      more -- the prefetch of the next item's halo across the item boundary, the weight double-buffer parity across items),
      'multiple' (exactly 2 x 256).  tile_sk exists only as 'many' (w2_sk_per wants at least 256 items and an unfilled round), and
      c4_2 has no 'multiple' (512 items of two cells are 256 of four, which is c4_4);
  DIVISORS of the float-reciprocal index decodes: 3, 5 and 7 tiles / cells along each axis, and ncog = Cout / 32 = 3;
  CHUNKS: wino Cin 8, 24, 40 (1, 3, 5 chunks: the weight-buffer parity flips between items) in 'many' cases, and an even count;
      tile and c4 Cin 8 (two chunks: the zero-padded thin head), 40 and 64; tile_sk Cin 32 (its minimum), 40 and 64;
  CELLS (c4): a partial last item with 1, 2 and 3 cells left (NC = 4) and with 1 (NC = 2), an item whose cells lie in two samples,
      extents 4 mod 8 along z only, y only, x only, and along all three;
  STREAM-K (tile_sk), by hand from w2_sk_per at 256 CUs: 1 x (48, 48, 32) 32 -> 64 is 288 items of 8 chunks in ranges of 10 (every
      fourth boundary falls on an item boundary, the last 25 workgroups are empty); 3 x (16, 24, 40) 64 -> 96 is 270 items of 16
      chunks in ranges of 20, ncog = 3, cut items in every sample -- in the dgrad role with bias and addend, which the piece that
      holds chunk 0 of a cut item carries; a tile shape where the query declines (512 items: whole rounds) is run with a workspace
      all the same and must give the bits of the run without; every tile_sk case is also run without a workspace.

Weight-gradient classes, for both forms: SLABS '1', 'few', 'cap' (= 256 / npairs, npairs = ceil(Cin / 32) ceil(Cout / 32): reached
from 512 / npairs tiles, so 32^3 at npairs = 1); both reducers; both tile widths of F(3, 2); tags (wg_tags) 'uneven' (slabs do not
all take the same number of tiles), 'cross_sample' (a slab's tiles lie in two samples), 'empty' (a slab without a tile: zeros), and
for F(3x3, 2x2), whose slabs are contiguous ranges of tiles numbered z fastest, 'inside_column' (a range starts inside a z column:
the six-plane ring starts at another slot) with ntz in {1, 2, 3, 5} and >= 4 -- F(3, 2) deals its tiles x fastest with a stride, so
it has no such class; npairs > 1 with a partial last block on each side (36 -> 44); Cin = Cout = 4; Cin % 8 == 4 and
Cout % 8 == 4; accumulate 0 and 1; 3, 5 and 7 tiles per axis.

REFUSALS: arguments the host check rejects before any launch.  Size limit: at most 20M elements per tensor.
"""
from collections import namedtuple

Fwd = namedtuple('Fwd', 'body N D H W Cin Cout role bias addend stats ws items')
Wg = namedtuple('Wg', 'form N D H W Cin Cout accumulate slabs variant')

MAX_ELEMS = 20_000_000
CUS = 256
BODIES = ['wino', 'tile', 'tile_sk', 'c4_4', 'c4_2']
BODY_VARIANT = {'tile': 8, 'tile_sk': 8, 'c4_4': 4, 'c4_2': 2}      # seg3d_conv3d_k3_wino2d_fwd_variant
ALL_FWD = sorted([('wino',)] + [('tile', b, a, sk) for b in (0, 1) for a in (0, 1) for sk in (0, 1)] + [('sk_finish',)] +
                 [('c4', b, a, nc) for b in (0, 1) for a in (0, 1) for nc in (4, 2)], key=str)
ALL_WGRAD = sorted([('wgrad_wino', 8), ('wgrad_wino', 4), ('wino_reduce', 8), ('wino_reduce', 4), ('wgrad_wino2d',),
                    ('wino2d_reduce16', 16), ('wino2d_reduce16', 4)], key=str)
WS_PER_SLAB = {'wino': 36 * 1024, 'wino2d': 48 * 1024}              # workspace floats per slab and block pair


def case_id(c):
    return type(c).__name__.lower() + '-' + '-'.join(str(v) for v in c)


def cdiv(a, b):
    return -(-a // b)


# ---- forward / data gradient ---------------------------------------------------------------------------------------------------
def edge(c):
    """tile (8) or cell (4) edge of a forward case"""
    return 4 if c.body in ('c4_4', 'c4_2') else 8


def counts(c):
    """tiles / cells along (z, y, x)"""
    e = edge(c)
    return c.D // e, c.H // e, c.W // e


def n_items(c):
    nz, ny, nx = counts(c)
    per = {'c4_4': 4, 'c4_2': 2}.get(c.body, 1)
    return cdiv(c.N * nz * ny * nx, per) * (c.Cout // 32)


def item_class(n):
    return 'fewer' if n < CUS else 'multiple' if n == 2 * CUS else 'many' if n % CUS else 'other'


def cells_left(c):
    """cells of the last item of a cell case (NC: whole)"""
    nz, ny, nx = counts(c)
    nc = 4 if c.body == 'c4_4' else 2
    return (c.N * nz * ny * nx - 1) % nc + 1


def mod8_class(c):
    """which extents are 4 mod 8: 'z', 'y', 'x', 'all', or 'mixed'"""
    off = (c.D % 8 == 4, c.H % 8 == 4, c.W % 8 == 4)
    return {(True, False, False): 'z', (False, True, False): 'y', (False, False, True): 'x', (True, True, True): 'all'}.get(off, 'mixed')


def fwd_keys(c):
    """the instantiations a case runs"""
    if c.body == 'wino':
        return [('wino',)]
    if c.body in ('tile', 'tile_sk'):
        sk = int(c.body == 'tile_sk')
        return [('tile', c.bias, c.addend, sk)] + ([('sk_finish',)] if sk else [])
    return [('c4', c.bias, c.addend, 4 if c.body == 'c4_4' else 2)]


def cut_items(c, per):
    """stream-K: the items cut by a range boundary (ranges of `per` chunks of four channels over items of Cin / 4 chunks)"""
    nsc, total = c.Cin // 4, n_items(c) * (c.Cin // 4)
    return sorted({g // nsc for g in range(per, total, per) if g % nsc})


def _fw(body, N, dims, Cin, Cout, role, bias, addend, stats, items, ws=None):
    return Fwd(body, N, dims[0], dims[1], dims[2], Cin, Cout, role, bias, addend, stats, int(body == 'tile_sk') if ws is None else ws,
               items)


FWD_CASES = [
    # F(2, 3) along x.  1 x (24, 40, 56) -> 96 and its two rotations are 315 items with 3, 5 and 7 tiles on every axis in turn
    _fw('wino', 1, (8, 16, 24), 16, 32, 'fwd', 1, 1, 1, 'fewer'),
    _fw('wino', 2, (24, 8, 16), 8, 96, 'dgrad', 0, 0, 0, 'fewer'),
    _fw('wino', 1, (24, 40, 56), 24, 96, 'fwd', 1, 0, 1, 'many'),
    _fw('wino', 3, (56, 24, 40), 8, 32, 'dgrad', 0, 1, 1, 'many'),
    _fw('wino', 1, (40, 56, 24), 40, 96, 'fwd', 1, 1, 0, 'many'),
    _fw('wino', 2, (16, 24, 40), 16, 160, 'dgrad', 0, 0, 1, 'many'),          # 300 items, two chunks, ncog = 5
    _fw('wino', 1, (32, 32, 64), 8, 128, 'fwd', 1, 1, 1, 'multiple'),
    # F(2x2, 3x3) tile kernel, whole items: no workspace -- or one that the plan declines (512 items)
    _fw('tile', 1, (8, 16, 24), 8, 32, 'dgrad', 1, 1, 1, 'fewer'),
    _fw('tile', 2, (24, 8, 16), 64, 96, 'fwd', 0, 0, 0, 'fewer'),
    _fw('tile', 1, (24, 40, 56), 8, 96, 'fwd', 1, 0, 1, 'many'),
    _fw('tile', 3, (56, 24, 40), 8, 32, 'dgrad', 0, 1, 1, 'many'),
    _fw('tile', 1, (40, 56, 24), 40, 96, 'fwd', 1, 1, 0, 'many'),
    _fw('tile', 1, (32, 32, 64), 32, 128, 'fwd', 1, 1, 1, 'multiple', ws=1),
    # ... with stream-K
    _fw('tile_sk', 1, (48, 48, 32), 32, 64, 'fwd', 1, 1, 1, 'many'),
    _fw('tile_sk', 3, (16, 24, 40), 64, 96, 'dgrad', 1, 1, 1, 'many'),
    _fw('tile_sk', 1, (24, 40, 56), 40, 96, 'fwd', 0, 0, 0, 'many'),
    _fw('tile_sk', 2, (40, 56, 8), 32, 128, 'dgrad', 1, 0, 1, 'many'),
    _fw('tile_sk', 1, (56, 40, 24), 32, 96, 'fwd', 0, 1, 1, 'many'),
    # four cells per item (at least 192 such items)
    _fw('c4_4', 5, (12, 12, 12), 8, 256, 'fwd', 1, 1, 1, 'many'),              # 135 cells: 34 groups, three cells in the last
    _fw('c4_4', 3, (8, 16, 20), 40, 256, 'dgrad', 0, 0, 0, 'fewer'),           # x only
    _fw('c4_4', 3, (16, 28, 24), 64, 96, 'fwd', 1, 0, 1, 'many'),              # y only, ncog = 3
    _fw('c4_4', 2, (28, 8, 16), 8, 288, 'dgrad', 0, 1, 1, 'fewer'),            # z only
    _fw('c4_4', 2, (12, 20, 28), 8, 160, 'dgrad', 1, 1, 0, 'many'),            # 210 cells: two in the last item
    _fw('c4_4', 3, (20, 4, 28), 8, 256, 'fwd', 0, 0, 1, 'fewer'),              # 105 cells: one in the last item
    _fw('c4_4', 1, (4, 64, 64), 8, 256, 'fwd', 1, 1, 1, 'multiple'),
    # two cells per item
    _fw('c4_2', 5, (12, 12, 12), 8, 128, 'fwd', 1, 1, 1, 'many'),              # 68 groups, one cell in the last
    _fw('c4_2', 1, (20, 4, 12), 8, 32, 'dgrad', 0, 0, 0, 'fewer'),
    _fw('c4_2', 2, (8, 16, 20), 40, 96, 'fwd', 1, 0, 1, 'fewer'),              # x only, ncog = 3
    _fw('c4_2', 1, (16, 28, 8), 64, 320, 'dgrad', 0, 1, 1, 'many'),            # y only
    _fw('c4_2', 3, (28, 8, 16), 8, 128, 'fwd', 1, 1, 0, 'many'),               # z only
    _fw('c4_2', 1, (12, 20, 28), 8, 96, 'dgrad', 1, 1, 1, 'fewer'),            # 105 cells
]


# ---- weight gradient -------------------------------------------------------------------------------------------------------------
def npairs(c):
    return cdiv(c.Cin, 32) * cdiv(c.Cout, 32)


def wg_tx(c):
    """x extent of the tile: 8 or 4 for F(3, 2) (variant // 10), 4 for F(3x3, 2x2)"""
    return 4 if c.form == 'wino2d' or c.variant // 10 else 8


def wg_counts(c):
    return c.D // 4, c.H // 4, c.W // wg_tx(c)


def wg_tiles(c):
    nz, ny, nx = wg_counts(c)
    return c.N * nz * ny * nx


def slab_class(c, slabs):
    return '1' if slabs == 1 else 'cap' if slabs == CUS // npairs(c) else 'few'


def wg_keys(c):
    if c.form == 'wino':
        return [('wgrad_wino', wg_tx(c)), ('wino_reduce', 8 if c.variant % 10 else 4)]
    return [('wgrad_wino2d',), ('wino2d_reduce16', 16 if c.variant % 10 else 4)]


def slab_tiles(c, slabs):
    """the tiles of every slab, as the two kernels deal them: F(3, 2) numbers its tiles x fastest and strides them over the slabs
    (by eighths of the tiles when slabs % 8 == 0); F(3x3, 2x2) numbers them z fastest and gives every slab one contiguous range"""
    nt = wg_tiles(c)
    out = []
    for s in range(slabs):
        if c.form == 'wino2d':
            per = cdiv(nt, slabs)
            o = (s & 7) * (slabs >> 3) + (s >> 3) if slabs % 8 == 0 else s
            out.append(list(range(min(o * per, nt), min(o * per + per, nt))))
        elif slabs % 8 == 0:
            per_xcd, xcd = cdiv(nt, 8), s & 7
            out.append(list(range(xcd * per_xcd + (s >> 3), min((xcd + 1) * per_xcd, nt), slabs >> 3)))
        else:
            out.append(list(range(s, nt, slabs)))
    return out


def wg_tags(c, slabs):
    nz, ny, nx = wg_counts(c)
    tiles = slab_tiles(c, slabs)
    assert sorted(t for ts in tiles for t in ts) == list(range(wg_tiles(c)))
    tags = set()
    if len({len(ts) for ts in tiles}) > 1:
        tags.add('uneven')
    if any(not ts for ts in tiles):
        tags.add('empty')
    if any(ts and ts[0] // (nz * ny * nx) != ts[-1] // (nz * ny * nx) for ts in tiles):
        tags.add('cross_sample')
    if c.form == 'wino2d' and any(ts and ts[0] % nz for ts in tiles):
        tags.add('inside_column')
    return tags


def _wg(form, N, dims, Cin, Cout, accumulate, slabs, variant):
    return Wg(form, N, dims[0], dims[1], dims[2], Cin, Cout, accumulate, slabs, variant)


WGRAD_CASES = [
    # F(3, 2) along x: tile 4 x 4 x 8 where W % 8 == 0 (variants 0, 1), else 4 x 4 x 4 (10, 11)
    _wg('wino', 1, (4, 4, 8), 4, 4, 0, '1', 0),
    _wg('wino', 1, (4, 4, 4), 4, 4, 1, '1', 10),
    _wg('wino', 1, (12, 20, 28), 36, 44, 1, 'few', 11),                        # 105 tiles on 53 slabs
    _wg('wino', 3, (20, 12, 8), 12, 20, 0, 'few', 0),                          # 45 tiles on 23 slabs
    _wg('wino', 2, (28, 12, 40), 36, 44, 0, 'cap', 1),                         # 210 tiles on 64 slabs, by eighths
    _wg('wino', 1, (32, 32, 36), 8, 24, 1, 'cap', 11),                         # 576 tiles on 256 slabs
    _wg('wino', 1, (8, 8, 64), 32, 64, 1, 'few', 0),                           # 32 tiles on 16 slabs, by eighths
    _wg('wino', 1, (4, 28, 12), 8, 4, 0, 'few', 10),
    _wg('wino', 1, (12, 76, 8), 128, 128, 1, 'cap', 0),                        # 57 tiles on 16 slabs by eighths of 8: one slab is empty
    # F(3x3, 2x2) over (y, x)
    _wg('wino2d', 1, (4, 4, 8), 4, 4, 0, '1', 0),
    _wg('wino2d', 1, (12, 20, 28), 36, 44, 1, 'few', 0),                       # 105 tiles on 53 slabs of two: ranges start inside columns of 3
    _wg('wino2d', 3, (20, 12, 4), 12, 20, 0, 'few', 0),                        # 45 tiles on 23 slabs; tiles 14, 15 are in two samples
    _wg('wino2d', 2, (28, 12, 20), 36, 44, 0, 'cap', 1),                       # 210 tiles on 64 slabs of four: 11 slabs are empty
    _wg('wino2d', 1, (32, 32, 32), 8, 24, 1, 'cap', 1),                        # 512 tiles on 256 slabs
    _wg('wino2d', 1, (8, 8, 16), 32, 64, 1, 'few', 0),                         # 16 tiles on 8 slabs, in the order of the eighths
    _wg('wino2d', 1, (4, 28, 12), 8, 4, 0, 'few', 0),
    _wg('wino2d', 2, (16, 8, 40), 20, 32, 1, 'few', 1),                        # 160 tiles on 80 slabs: <16> below the cap
]


# ---- refusals: (the name the message starts with, the entry point, kind, what is changed from a supported call, why) ---------------
#   base call: N = 1, (8, 8, 16), 16 -> 32; 'W+' adds to W, 'Cin+' to Cin, 'Cout=' sets Cout, 'null' names the pointer left out
_F, _F2, _G, _G2 = ('seg3d_conv3d_k3_wino_fwd', 'seg3d_conv3d_k3_wino2d_fwd', 'seg3d_conv3d_k3_wino_wgrad',
                    'seg3d_conv3d_k3_wino2d_wgrad')
REFUSALS = [
    (_F, _F, 'fwd', ('W+', 4), 'wino fwd: W + 4'),
    (_F, _F, 'fwd', ('Cin+', 4), 'wino fwd: Cin + 4'),
    (_F, _F, 'fwd', ('Cout=', 48), 'wino fwd: Cout = 48'),
    (_F, _F, 'fwd', ('null', 'x'), 'wino fwd: null x'),
    (_F2, _F2, 'fwd', ('W+', 2), 'wino2d fwd: W + 2'),
    (_F2, _F2, 'fwd', ('Cin+', 4), 'wino2d fwd: Cin + 4'),
    (_F2, _F2 + '_ws', 'fwd', ('Cout=', 48), 'wino2d fwd_ws: Cout = 48'),
    (_F2, _F2 + '_ws', 'fwd', ('null', 'x'), 'wino2d fwd_ws: null x'),
    (_G, _G, 'wgrad', ('W+', 2), 'wino wgrad: W + 2'),
    (_G, _G, 'wgrad', ('Cin+', 2), 'wino wgrad: Cin + 2'),
    (_G, _G, 'wgrad', ('null', 'workspace'), 'wino wgrad: null workspace'),
    (_G2, _G2, 'wgrad', ('W+', 2), 'wino2d wgrad: W + 2'),
    (_G2, _G2, 'wgrad', ('Cin+', 2), 'wino2d wgrad: Cin + 2'),
    (_G2, _G2, 'wgrad', ('null', 'workspace'), 'wino2d wgrad: null workspace'),
]
REFUSAL_BASE = (1, 8, 8, 16, 16, 32)


def refusal_dims(change):
    N, D, H, W, Cin, Cout = REFUSAL_BASE
    if change[0] == 'W+':
        W += change[1]
    elif change[0] == 'Cin+':
        Cin += change[1]
    elif change[0] == 'Cout=':
        Cout = change[1]
    return N, D, H, W, Cin, Cout
