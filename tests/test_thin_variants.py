"""Host-only: every case of tests/thin_cases.py reaches the kernel of csrc/conv_thin.hip / csrc/conv_thin_f32.hip it is named for
(the row form of the persistent thin-input kernels, the z extent of the fp32 head kernel, tiles against workgroups, weight-gradient
slabs -- all through read-only queries that call the functions the launchers call), every instantiation of the family is named by
a case, and the edges the device test relies on are spread over all of them -- so a retuned plan function, or a kernel without a
test, fails here, without a GPU."""
import ctypes
import os

import pytest

import thin_cases as T

QUERIES = ('seg3d_conv3d_k3_thin_out_f32mfma_tz', 'seg3d_conv3d_k3_thin_in_persistent_variant',
           'seg3d_conv3d_k3_thin_in_persistent_workgroups', 'seg3d_k3_thin_wgrad_workspace_floats',
           'seg3d_conv3d_k3_thin_in_mfma16_supported', 'seg3d_conv3d_k3_thin_out_mfma_supported',
           'seg3d_conv3d_k3_thin_out_f32mfma_supported', 'seg3d_conv3d_k3_thin_out_f32mfma_stats_count',
           'seg3d_conv3d_k3_thin_in_persistent_stats_count')


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__  # noqa: F401  (repo root is on sys.path)
    from segmentation3d import _engine
    if not os.path.isfile(_engine.LIB_PATH):
        __graft_entry__.build()
    handle = ctypes.CDLL(_engine.LIB_PATH)
    for name in QUERIES:
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _engine._SIGNATURES[name]
    return handle


def wgrad_slabs(lib, N, D, H, W, CT, CF):
    per = ((CF + 31) // 32) * ((27 * CT + 31) // 32) * 1024
    ws = lib.seg3d_k3_thin_wgrad_workspace_floats(N, D, H, W, CT, CF)
    assert ws % per == 0
    return ws // per


def tile_class(lib, c):
    tiles = T.tiles(c, T.IN_TILE)
    wgs = lib.seg3d_conv3d_k3_thin_in_persistent_workgroups(c.N, c.D, c.H, c.W, c.Cout)
    assert wgs == min(T.WG_CAP // ((c.Cout + 31) // 32), tiles)
    return 'one' if tiles == wgs else 'many' if tiles % wgs else 'multiple'


@pytest.mark.parametrize('case', T.IN_CASES, ids=T.case_id)
def test_thin_in_case_reaches_its_kernel(lib, case):
    c = case
    assert 1 <= c.CT <= 8 and c.role in ('fwd', 'dgrad') and c.out_bf16 in (0, 1) and c.full in (0, 1)
    assert T.in_key(c) in T.ALL_IN
    if c.kernel == 'persistent':
        assert lib.seg3d_conv3d_k3_thin_in_persistent_variant(c.Cout) == T.persistent_rows(c.Cout)
        assert tile_class(lib, c) == T.TILE_CLASS[c]
        cobs = (c.Cout + 31) // 32
        assert lib.seg3d_conv3d_k3_thin_in_persistent_stats_count(c.D, c.H, c.W, cobs) * c.N == 4 * T.tiles(c, T.IN_TILE) * cobs
    elif c.kernel == 'mfma16':
        assert c.out_bf16 == 1 and lib.seg3d_conv3d_k3_thin_in_mfma16_supported(c.CT, c.Cout) == 1
    else:
        assert c.kernel == 'thin_in'
    assert c.N * c.D * c.H * c.W * max(c.CT, c.Cout) <= T.MAX_ELEMS


@pytest.mark.parametrize('case', T.OUT_CASES, ids=T.case_id)
def test_thin_out_case_reaches_its_kernel(lib, case):
    c = case
    assert c.role in ('fwd', 'dgrad') and c.full in (0, 1) and all(k in T.ALL_OUT for k in T.out_keys(c))
    if c.kernel in ('thin_out', 'thin_out_bf16'):
        assert c.CO in (2, 4, 8) and 1 <= c.Cout <= c.CO and c.Cin % 4 == 0 and c.tz == 0
    elif c.kernel == 'thin_out_mfma':
        assert lib.seg3d_conv3d_k3_thin_out_mfma_supported(c.Cin, c.Cout) == 1 and c.CO == (2 if c.Cout <= 2 else 3) and c.tz == 0
    else:
        assert c.kernel == 'thin_out_f32mfma' and lib.seg3d_conv3d_k3_thin_out_f32mfma_supported(c.Cin, c.Cout) == 1
        assert c.CO == T.f32_co(c.Cout)
        assert lib.seg3d_conv3d_k3_thin_out_f32mfma_tz(c.N, c.D, c.H, c.W) == c.tz
        assert lib.seg3d_conv3d_k3_thin_out_f32mfma_stats_count(c.N, c.D, c.H, c.W) * c.N == T.tiles(c, (c.tz, 8, 16))
    assert c.N * c.D * c.H * c.W * max(c.Cin, c.Cout) <= T.MAX_ELEMS


@pytest.mark.parametrize('case', T.WGRAD_CASES, ids=T.case_id)
def test_wgrad_case_reaches_its_slab_class(lib, case):
    c = case
    assert 1 <= c.CT <= 8 and c.CF % 4 == 0 and c.conv in ('stem', 'head') and T.wg_key(c) in T.ALL_WGRAD
    slabs = wgrad_slabs(lib, c.N, c.D, c.H, c.W, c.CT, c.CF)
    assert slabs == min(T.cdiv(T.tiles(c, T.IN_TILE), T.TILES_PER_SLAB), T.SLAB_CAP)
    assert T.slab_class(slabs) == c.slabs
    assert (slabs > T.REDUCE_STRIDE) == (T.reduce_class(c) == 'gt64')
    assert c.N * c.D * c.H * c.W * max(c.CT, c.CF) <= T.MAX_ELEMS


def test_every_instantiation_has_a_case():
    assert sorted({T.in_key(c) for c in T.IN_CASES}, key=str) == T.ALL_IN
    assert sorted({k for c in T.OUT_CASES for k in T.out_keys(c)}, key=str) == T.ALL_OUT
    assert sorted({T.wg_key(c) for c in T.WGRAD_CASES}) == T.ALL_WGRAD
    assert sorted({T.reduce_class(c) for c in T.WGRAD_CASES}) == T.ALL_REDUCE
    assert (len(T.ALL_IN), len(T.ALL_OUT), len(T.ALL_WGRAD)) == (50, 26, 16)
    assert {c.tz for c in T.OUT_CASES if c.kernel == 'thin_out_f32mfma'} == set(T.TZ_VALUES)
    for cases in (T.IN_CASES, T.OUT_CASES, T.WGRAD_CASES):
        assert len(set(cases)) == len(cases)


def _common_edges(cs, tile, what):
    assert {c.role for c in cs} == {'fwd', 'dgrad'}, what
    assert {c.full for c in cs} == {0, 1}, what
    assert {1, 3} <= {c.N for c in cs}, what
    assert T.SHAPE_CLASSES <= {T.shape_class(c, tile) for c in cs}, what
    # ... and paired, not only each on its own: every shape class with bias and statistics and without, and in both roles
    for cls in sorted(T.SHAPE_CLASSES):
        of = [c for c in cs if T.shape_class(c, tile) == cls]
        assert {c.full for c in of} == {0, 1}, (what, cls)
        assert {c.role for c in of} == {'fwd', 'dgrad'}, (what, cls)
    assert {c.N for c in cs if c.full} >= {1, 3}, what


def test_thin_in_edges_are_spread_over_the_kernels():
    for body in T.IN_BODIES:
        cs = [c for c in T.IN_CASES if T.in_body(c) == body]
        _common_edges(cs, T.IN_TILE, body)
        couts = {c.Cout for c in cs}
        if body in ('thin_in', 'thin_in_bf16out', 'thin_in_mfma16'):
            assert {32, 64, 20, 48, 4, 8, 12, 16} <= couts, body
        elif body[0] == 'thin_in_persistent':
            assert {32, 64, 20, 48} <= couts and any(co % 4 for co in couts), body
            regular = [c for c in cs if T.in_regular(c)]
            assert any(c.Cout % 8 == 0 and c.Cout % 32 == 0 for c in regular) and any(c.Cout % 8 == 0 and c.Cout % 32 for c in regular)
            assert any(c.Cout % 8 for c in regular), body
            assert any(T.in_regular(c) and T.TILE_CLASS[c] == 'many' and c.Cout % 8 == 0 for c in cs), body
        else:
            assert couts == {4, 8, 12, 16}, body
            assert {c.Cout for c in cs if T.in_regular(c)} >= {12, 16}, body
        if body[0] in ('thin_in_persistent', 'thin_in_persistent16'):
            assert {c.CT for c in cs} == set(range(1, 9)), body
            many = [c for c in cs if T.TILE_CLASS[c] == 'many']
            assert {c.CT % 2 for c in many} == {0, 1} and any(not T.in_regular(c) for c in many), body
            assert all(c.full for c in many), body              # (the statistics across tiles)
            assert {c.role for c in many} == {'fwd', 'dgrad'} and len({(c.D, c.H, c.W) for c in many}) >= 2, body
    for key in T.ALL_IN:                                        # every instantiation in both roles
        assert {c.role for c in T.IN_CASES if T.in_key(c) == key} == {'fwd', 'dgrad'}, key
    assert any(T.in_key(c)[0] == 'thin_in_persistent' and c.Cout == 48 and T.TILE_CLASS[c] == 'many' and not T.in_regular(c)
               for c in T.IN_CASES)                            # 550 tiles on 512 workgroups


def test_thin_out_edges_are_spread_over_the_kernels():
    for body in T.OUT_BODIES:
        cs = [c for c in T.OUT_CASES if c.kernel == body]
        _common_edges(cs, T.OUT_TILE, body)
    for key in T.ALL_OUT:
        cs = [c for c in T.OUT_CASES if key in T.out_keys(c)]
        assert {c.role for c in cs} == {'fwd', 'dgrad'}, key
        if key[0] in ('thin_out', 'thin_out_bf16'):
            co = key[1]
            assert any(c.Cout == co for c in cs) and any(c.Cout < co for c in cs), key
            assert any(c.Cin % 8 == 4 for c in cs) and any(c.Cin % 8 == 0 for c in cs), key
        else:
            assert key[-1] == 'plain' or any(c.W <= 32 for c in cs), key                 # masked tiles only
            assert any(c.W >= 33 for c in cs), key              # an interior x tile
            if key[-1] == 'plain':
                assert all(c.W >= 33 for c in cs), key
            if key[2] == 2:
                assert any(c.Cout == 1 for c in cs), key
                assert {c.W % 2 for c in cs if c.Cout == 2} == {0, 1}, key
    valu = [c for c in T.OUT_CASES if c.kernel in ('thin_out', 'thin_out_bf16')]
    assert {1, 3, 5, 6, 7} <= {c.Cout for c in valu} and {12, 20} <= {c.Cin for c in valu}
    f32 = [c for c in T.OUT_CASES if c.kernel == 'thin_out_f32mfma']
    for tz in T.TZ_VALUES:
        assert any(c.tz == tz and c.D % tz for c in f32), tz    # a short last march
    assert any(c.tz > 8 and c.D % c.tz == 0 for c in f32)
    assert {12, 16} <= {c.tz for c in f32 if c.W >= 33}
    assert any(c.N > 3 for c in f32)


def test_wgrad_edges_are_spread_over_the_kernels():
    for key in T.ALL_WGRAD:
        cs = [c for c in T.WGRAD_CASES if T.wg_key(c) == key]
        assert {c.conv for c in cs} == {'stem', 'head'} and {c.accumulate for c in cs} == {0, 1}, key
        assert {'1', 'few'} <= {c.slabs for c in cs}, key
        assert any(T.shape_class(c, T.IN_TILE) == 'whole' for c in cs) and any(T.shape_class(c, T.IN_TILE) != 'whole' for c in cs), key
    for fb in (0, 1):
        cs = [c for c in T.WGRAD_CASES if c.fat_bf16 == fb]
        assert {c.CF for c in cs} == {4, 20, 32, 48}, fb
        assert {(c.conv, c.accumulate) for c in cs} == {('stem', 0), ('stem', 1), ('head', 0), ('head', 1)}, fb
        assert {'1', 'few', 'many', 'cap'} == {c.slabs for c in cs}, fb
        many = [c for c in cs if c.slabs in ('many', 'cap')]
        assert {(c.conv, c.accumulate) for c in many} == {('stem', 0), ('stem', 1), ('head', 0), ('head', 1)}, fb
        assert any(T.shape_class(c, T.IN_TILE) == 'whole' for c in many) and any(T.shape_class(c, T.IN_TILE) == 'all' for c in many)


def test_refusal_table():
    names = {r[0] for r in T.REFUSALS}
    assert names == {'seg3d_conv3d_k3_thin_in_fwd', 'seg3d_conv3d_k3_thin_in_persistent_fwd', 'seg3d_conv3d_k3_thin_in_mfma16_fwd',
                     'seg3d_conv3d_k3_thin_out_fwd', 'seg3d_conv3d_k3_thin_out_mfma_fwd', 'seg3d_conv3d_k3_thin_out_f32mfma_fwd',
                     'seg3d_k3_thin_wgrad'}
    assert len({r[3] for r in T.REFUSALS}) == len(T.REFUSALS) == 15


def test_supported_queries_refuse_what_the_launchers_refuse(lib):
    for name, kind, args, why in T.REFUSALS:
        if name == 'seg3d_conv3d_k3_thin_in_mfma16_fwd':
            assert lib.seg3d_conv3d_k3_thin_in_mfma16_supported(*args) == 0, why
        elif name == 'seg3d_conv3d_k3_thin_out_mfma_fwd':
            assert lib.seg3d_conv3d_k3_thin_out_mfma_supported(*args) == 0, why
        elif name == 'seg3d_conv3d_k3_thin_out_f32mfma_fwd':
            assert lib.seg3d_conv3d_k3_thin_out_f32mfma_supported(*args) == 0, why
    assert lib.seg3d_conv3d_k3_thin_out_f32mfma_tz(0, 8, 8, 8) == 0 and lib.seg3d_conv3d_k3_thin_in_persistent_variant(0) == 0
    assert lib.seg3d_conv3d_k3_thin_in_persistent_workgroups(1, 0, 8, 8, 16) == 0


def test_thresholds_of_the_plan_functions(lib):
    """the thresholds named in the three plan functions, from both sides"""
    # thin_out_f32_tz: D = 17 in one 8 x 16 column per sample is 3 N tiles of tz = 8 or 2 N of tz = 12; up to 1024 tiles tz = 8 wins
    # (1.2 * 10.5 against 1.2 * 14.5), beyond them a second round of tz = 8 tiles (2 * 10.5) loses to one of tz = 12 (1.2 * 14.5)
    tz = lib.seg3d_conv3d_k3_thin_out_f32mfma_tz
    assert T.WG_CAP == 1024 and 3 * 341 <= 1024 < 3 * 342
    assert tz(341, 17, 3, 5) == 8 and tz(342, 17, 3, 5) == 12
    assert tz(4, 96, 96, 96) == 16                                       # the headline workload
    assert tz(2000, 7, 3, 5) == 8                                        # a candidate above 8 is never longer than D
    # the persistent walk: 1024 / cobs workgroups, or one per tile
    wg = lib.seg3d_conv3d_k3_thin_in_persistent_workgroups
    for cout, cobs in ((4, 1), (16, 1), (32, 1), (33, 2), (64, 2), (96, 3), (160, 5)):
        cap = 1024 // cobs
        assert wg(1, 4, 8, 8 * cap, cout) == cap and wg(1, 4, 8, 8 * (cap + 1), cout) == cap and wg(1, 4, 8, 8 * (cap - 1), cout) == cap - 1
    assert wg(1, 5, 9, 9, 16) == 8 and wg(1, 4, 8, 8, 16) == 1
    rows = lib.seg3d_conv3d_k3_thin_in_persistent_variant
    assert [rows(co) for co in (4, 8, 12, 16)] == [16] * 4 and [rows(co) for co in (1, 6, 15, 17, 20, 32, 48)] == [32] * 7
    # weight gradient: 8 tiles of 4 x 8 x 8 per slab, the reduce kernel's 64-slab stride, the cap of 512
    sl = lambda ntx: wgrad_slabs(lib, 1, 4, 8, 8 * ntx, 3, 32)
    assert (T.TILES_PER_SLAB, T.REDUCE_STRIDE, T.SLAB_CAP) == (8, 64, 512)
    assert sl(1) == 1 and sl(8) == 1 and sl(9) == 2 and sl(16) == 2 and sl(17) == 3
    assert sl(8 * 64) == 64 and sl(8 * 64 + 1) == 65 and T.slab_class(64) == 'few' and T.slab_class(65) == 'many'
    assert sl(8 * 511) == 511 and sl(8 * 511 + 1) == 512 and sl(8 * 512 + 1) == 512 and sl(100000) == 512
    assert T.slab_class(511) == 'many' and T.slab_class(512) == 'cap'
    # the slab count depends on the volume alone
    assert wgrad_slabs(lib, 3, 27, 37, 83, 1, 4) == wgrad_slabs(lib, 3, 27, 37, 83, 8, 48) == 145
    assert wgrad_slabs(lib, 1, 32, 64, 72, 2, 32) == 72 and wgrad_slabs(lib, 70, 9, 17, 50, 5, 20) == 512
