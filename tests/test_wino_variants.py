"""Host-only: every case of tests/wino_cases.py reaches the kernel of csrc/conv_wino.hip / csrc/conv_wino2d.hip it is named for
(tile or cell kernel and the cells per item, the stream-K chunk count, items against workgroups, weight-gradient tile width, slabs
and reducer -- all through read-only queries that call the functions the launchers call: w2_tiles, w2_cells_per_item, w2_sk_per,
wn_wgrad_plan, g2_slabs), every selectable instantiation is named by a case, and the edges the device test relies on are spread
over all bodies -- so a retuned plan function, or a kernel without a test, fails here, without a GPU (the queries assume the 256
CUs of the MI355X when there is no device)."""
import ctypes
import os

import pytest
import torch

import wino_cases as T
from float64_util import _conv_def, _wgrad_def, _wino_f23_conv, _wino_f2x2_conv, _wino_f32_wgrad, _wino_f3x3_wgrad

QUERIES = ('seg3d_conv3d_k3_wino_supported', 'seg3d_conv3d_k3_wino_preferred', 'seg3d_conv3d_k3_wino_stats_count',
           'seg3d_conv3d_k3_wino2d_supported', 'seg3d_conv3d_k3_wino2d_preferred', 'seg3d_conv3d_k3_wino2d_stats_count',
           'seg3d_conv3d_k3_wino2d_fwd_variant', 'seg3d_conv3d_k3_wino2d_fwd_sk_chunks', 'seg3d_conv3d_k3_wino2d_fwd_workspace_floats',
           'seg3d_conv3d_k3_wino_wgrad_supported', 'seg3d_conv3d_k3_wino_wgrad_variant', 'seg3d_conv3d_k3_wino_wgrad_workspace_floats',
           'seg3d_conv3d_k3_wino2d_wgrad_supported', 'seg3d_conv3d_k3_wino2d_wgrad_variant',
           'seg3d_conv3d_k3_wino2d_wgrad_workspace_floats')


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


def dims(c):
    return c.N, c.D, c.H, c.W, c.Cin, c.Cout


def wgrad_slabs(lib, c):
    ws = getattr(lib, 'seg3d_conv3d_k3_{}_wgrad_workspace_floats'.format(c.form))(*dims(c))
    per = T.npairs(c) * T.WS_PER_SLAB[c.form]
    assert ws % per == 0
    return ws // per


@pytest.mark.parametrize('case', T.FWD_CASES, ids=T.case_id)
def test_forward_case_reaches_its_kernel(lib, case):
    c = case
    assert c.body in T.BODIES and c.role in ('fwd', 'dgrad') and {c.bias, c.addend, c.stats, c.ws} <= {0, 1}
    assert all(k in T.ALL_FWD for k in T.fwd_keys(c))
    nz, ny, nx = T.counts(c)
    if c.body == 'wino':
        assert lib.seg3d_conv3d_k3_wino_supported(*dims(c)) == 1 and c.ws == 0
        assert lib.seg3d_conv3d_k3_wino_stats_count(*dims(c)) * c.N == T.n_items(c) * 8
    else:
        assert lib.seg3d_conv3d_k3_wino2d_supported(*dims(c)) == 1
        assert lib.seg3d_conv3d_k3_wino2d_fwd_variant(*dims(c)) == T.BODY_VARIANT[c.body]
        sk = lib.seg3d_conv3d_k3_wino2d_fwd_sk_chunks(*dims(c))
        nws = lib.seg3d_conv3d_k3_wino2d_fwd_workspace_floats(*dims(c))
        assert nws == (2 * T.CUS * 512 * 32 if sk else 0)
        if c.body == 'tile_sk':
            nsc = c.Cin // 4
            assert c.ws == 1 and sk >= nsc >= 8 and sk % (nsc // 4) == 0 and sk < 2 * nsc
            assert T.cdiv(T.n_items(c) * nsc, sk) <= T.CUS                # one range per workgroup
            assert T.cut_items(c, sk), 'no item is cut'
        else:
            assert sk == 0 or c.ws == 0                                # whole items: the plan declines, or no workspace is passed
        if c.body in ('tile', 'tile_sk'):
            assert lib.seg3d_conv3d_k3_wino2d_stats_count(*dims(c)) * c.N == T.n_items(c) * 8
        else:
            assert lib.seg3d_conv3d_k3_wino2d_stats_count(*dims(c)) == nz * ny * nx * (c.Cout // 32) * 2
    assert T.item_class(T.n_items(c)) == c.items
    assert c.N * c.D * c.H * c.W * max(c.Cin, c.Cout) <= T.MAX_ELEMS


@pytest.mark.parametrize('case', T.WGRAD_CASES, ids=T.case_id)
def test_wgrad_case_reaches_its_kernels(lib, case):
    c = case
    assert c.form in ('wino', 'wino2d') and c.accumulate in (0, 1) and all(k in T.ALL_WGRAD for k in T.wg_keys(c))
    assert getattr(lib, 'seg3d_conv3d_k3_{}_wgrad_supported'.format(c.form))(*dims(c)) == 1
    assert getattr(lib, 'seg3d_conv3d_k3_{}_wgrad_variant'.format(c.form))(*dims(c)) == c.variant
    slabs = wgrad_slabs(lib, c)
    assert T.slab_class(c, slabs) == c.slabs
    assert slabs == max(1, min(T.CUS // T.npairs(c), (T.wg_tiles(c) + 1) // 2))
    T.wg_tags(c, slabs)                                                # (every tile belongs to exactly one slab)
    assert c.N * c.D * c.H * c.W * max(c.Cin, c.Cout) <= T.MAX_ELEMS


def test_every_instantiation_has_a_case():
    assert sorted({k for c in T.FWD_CASES for k in T.fwd_keys(c)}, key=str) == T.ALL_FWD
    assert sorted({k for c in T.WGRAD_CASES for k in T.wg_keys(c)}, key=str) == T.ALL_WGRAD
    assert (len(T.ALL_FWD), len(T.ALL_WGRAD)) == (1 + 8 + 1 + 8, 7)
    for cases in (T.FWD_CASES, T.WGRAD_CASES):
        assert len(set(cases)) == len(cases)
    assert {c.variant for c in T.WGRAD_CASES if c.form == 'wino'} == {0, 1, 10, 11}
    assert {c.variant for c in T.WGRAD_CASES if c.form == 'wino2d'} == {0, 1}


def test_forward_edges_are_spread_over_the_bodies(lib):
    for body in T.BODIES:
        cs = [c for c in T.FWD_CASES if c.body == body]
        assert {c.role for c in cs} == {'fwd', 'dgrad'}, body
        assert {(c.bias, c.addend) for c in cs} == {(0, 0), (0, 1), (1, 0), (1, 1)}, body
        assert {c.stats for c in cs} == {0, 1}, body
        assert 1 in {c.N for c in cs} and any(c.N >= 2 for c in cs), body
        want = {'tile_sk': {'many'}, 'c4_2': {'fewer', 'many'}}.get(body, {'fewer', 'many', 'multiple'})
        assert {c.items for c in cs} == want, body
        for axis in range(3):
            assert {3, 5, 7} <= {T.counts(c)[axis] for c in cs}, (body, axis)
        assert 3 in {c.Cout // 32 for c in cs}, body
        cins = {c.Cin for c in cs}
        if body == 'wino':
            assert {8, 24, 40} <= {c.Cin for c in cs if c.items == 'many'} and any(c.Cin % 16 == 0 for c in cs if c.items == 'many')
        else:
            assert ({32, 40, 64} if body == 'tile_sk' else {8, 40, 64}) <= cins, body
        # statistics where a workgroup takes a second item, in both roles over the family
        assert any(c.stats and c.items == 'many' for c in cs), body
    c4 = [c for c in T.FWD_CASES if c.body in ('c4_4', 'c4_2')]
    assert {T.cells_left(c) for c in c4 if c.body == 'c4_4'} == {1, 2, 3, 4}
    assert {T.cells_left(c) for c in c4 if c.body == 'c4_2'} == {1, 2}
    for body in ('c4_4', 'c4_2'):
        cs = [c for c in c4 if c.body == body]
        assert {'z', 'y', 'x', 'all'} <= {T.mod8_class(c) for c in cs}, body
        nc = 4 if body == 'c4_4' else 2
        assert any(c.N > 1 and (c.D // 4) * (c.H // 4) * (c.W // 4) % nc for c in cs), body        # an item in two samples
    # stream-K: the two shapes worked out by hand, the dgrad case with bias and addend, and a declined workspace
    sk = {(c.N, c.D, c.H, c.W, c.Cin, c.Cout): c for c in T.FWD_CASES if c.body == 'tile_sk'}
    a, b = sk[(1, 48, 48, 32, 32, 64)], sk[(3, 16, 24, 40, 64, 96)]
    assert T.n_items(a) == 288 and lib.seg3d_conv3d_k3_wino2d_fwd_sk_chunks(*dims(a)) == 10
    cuts = T.cut_items(a, 10)
    assert len(cuts) == 230 - 230 // 4 and T.cdiv(288 * 8, 10) == T.CUS - 25                       # every fourth boundary is whole
    assert T.n_items(b) == 270 and lib.seg3d_conv3d_k3_wino2d_fwd_sk_chunks(*dims(b)) == 20
    assert {i // 90 for i in T.cut_items(b, 20)} == {0, 1, 2} and (b.role, b.bias, b.addend) == ('dgrad', 1, 1)
    assert any(c.body == 'tile' and c.ws == 1 and lib.seg3d_conv3d_k3_wino2d_fwd_sk_chunks(*dims(c)) == 0 for c in T.FWD_CASES)
    # a tile case that stream-K would take, run on whole items because no workspace is passed
    assert any(c.body == 'tile' and c.ws == 0 and lib.seg3d_conv3d_k3_wino2d_fwd_sk_chunks(*dims(c)) > 0 for c in T.FWD_CASES)


def test_wgrad_edges_are_spread_over_the_forms(lib):
    for form in ('wino', 'wino2d'):
        cs = [c for c in T.WGRAD_CASES if c.form == form]
        assert {c.slabs for c in cs} == {'1', 'few', 'cap'}, form
        assert {c.accumulate for c in cs} == {0, 1}, form
        tags = {c: T.wg_tags(c, wgrad_slabs(lib, c)) for c in cs}
        want = {'uneven', 'cross_sample', 'empty'} | ({'inside_column'} if form == 'wino2d' else set())
        assert want <= set().union(*tags.values()), form
        for axis in range(3):
            assert {3, 5, 7} <= {T.wg_counts(c)[axis] for c in cs}, (form, axis)
        assert any(T.npairs(c) > 1 and c.Cin % 32 and c.Cout % 32 for c in cs), form
        assert any(c.Cin == 4 and c.Cout == 4 for c in cs), form
        assert any(c.Cin % 8 == 4 and c.Cin > 4 for c in cs) and any(c.Cout % 8 == 4 and c.Cout > 4 for c in cs), form
        for key in (k for k in T.ALL_WGRAD if any(k in T.wg_keys(c) for c in cs)):
            assert {c.accumulate for c in cs if key in T.wg_keys(c)} == {0, 1}, key
        assert any(c.slabs == 'cap' and T.npairs(c) == 1 for c in cs) and any(c.slabs == 'cap' and T.npairs(c) > 1 for c in cs), form
        if form == 'wino2d':
            inside = {T.wg_counts(c)[0] for c in cs if 'inside_column' in tags[c]}
            assert {3, 5} <= inside and any(nz >= 4 for nz in inside), inside
            assert {1, 2, 3, 5} <= {T.wg_counts(c)[0] for c in cs}
            assert any(c.variant == 1 and c.slabs == 'few' for c in cs)


def test_refusal_table(lib):
    assert {r[0] for r in T.REFUSALS} == {'seg3d_conv3d_k3_wino_fwd', 'seg3d_conv3d_k3_wino2d_fwd', 'seg3d_conv3d_k3_wino_wgrad',
                                          'seg3d_conv3d_k3_wino2d_wgrad'}
    assert len({r[4] for r in T.REFUSALS}) == len(T.REFUSALS) == 14
    base = T.REFUSAL_BASE
    for q in ('wino_supported', 'wino2d_supported', 'wino_wgrad_supported', 'wino2d_wgrad_supported'):
        assert getattr(lib, 'seg3d_conv3d_k3_' + q)(*base) == 1
    for prefix, entry, kind, change, why in T.REFUSALS:
        if change[0] == 'null':
            continue
        q = prefix.replace('_fwd', '_supported') if kind == 'fwd' else prefix + '_supported'
        assert getattr(lib, q)(*T.refusal_dims(change)) == 0, why
    assert lib.seg3d_conv3d_k3_wino2d_fwd_variant(1, 8, 8, 18, 16, 32) == 0
    assert lib.seg3d_conv3d_k3_wino2d_fwd_sk_chunks(1, 8, 8, 18, 16, 32) == 0
    assert lib.seg3d_conv3d_k3_wino_wgrad_variant(1, 8, 8, 18, 16, 32) == -1
    assert lib.seg3d_conv3d_k3_wino2d_wgrad_variant(1, 8, 8, 16, 18, 32) == -1


def test_thresholds_of_the_plan_functions(lib):
    """the thresholds named in the plan functions, from both sides"""
    # w2_cells_per_item: four cells per item from 192 such items.  Cells of 4 x 4 x 4 in a 4 x 4 x 4 n volume, Cout = 256: 8 items per
    # four cells
    var = lib.seg3d_conv3d_k3_wino2d_fwd_variant
    assert var(1, 4, 4, 4 * 96, 8, 256) == 4 and var(1, 4, 4, 4 * 93, 8, 256) == 4 and var(1, 4, 4, 4 * 92, 8, 256) == 2   # 192, 192, 184
    assert var(5, 12, 12, 12, 8, 128) == 2 and var(5, 12, 12, 12, 8, 256) == 4 and var(4, 12, 12, 12, 128, 128) == 2
    assert var(1, 8, 8, 8, 8, 32) == 8 and var(1, 8, 8, 12, 8, 32) == 2 and var(1, 8, 8, 10, 8, 32) == 0
    # w2_sk_per: at least 256 items, at least 8 chunks, a fill of at most W2_SK_FILL = 0.94 of the rounds; ranges a multiple of
    # NSC / 4.  Tiles of 8^3 in an 8 x 8 x 8 n volume with Cout = 32: n items
    sk = lambda n, cin=32: lib.seg3d_conv3d_k3_wino2d_fwd_sk_chunks(1, 8, 8, 8 * n, cin, 32)
    assert sk(255) == 0 and sk(256) == 0 and sk(257) == 10                     # 257 * 8 / 256 = 8.03 -> 9 -> 10
    assert sk(481) == 16 and sk(482) == 0                                      # 481 / 512 = 0.9395, 482 / 512 = 0.9414
    assert sk(512) == 0 and sk(513) == 18 and sk(721) == 24 and sk(722) == 0   # 721 / 768 = 0.9388, 722 / 768 = 0.9401
    assert sk(300, 24) == 0 and sk(300, 28) == 0 and sk(300, 40) == 12         # 6, 7 chunks: none; 10: 11.7 -> 12
    assert lib.seg3d_conv3d_k3_wino2d_fwd_sk_chunks(4, 24, 24, 24, 128, 128) == 56                 # the 24^3 level of the train step
    assert lib.seg3d_conv3d_k3_wino2d_fwd_sk_chunks(4, 12, 12, 12, 128, 128) == 0                   # cells
    # wn_wgrad_plan: tile width from W, slabs = min(256 / npairs, (tiles + 1) / 2), reduce<8> from 32 slabs
    w = lambda W, cin=32: lib.seg3d_conv3d_k3_wino_wgrad_variant(1, 4, 4, W, cin, 32)
    assert w(8) == 0 and w(12) == 10 and w(16) == 0 and w(4) == 10
    assert w(8 * 62) == 0 and w(8 * 63) == 1 and w(8 * 64) == 1                # 31, 32, 32 slabs
    assert w(4 * 61) == 10 and w(4 * 63) == 11
    assert w(8 * 200, 64) == 1 and w(8 * 62, 64) == 0                          # npairs = 2: the cap of 128 is above 32
    sl = lambda W, cin, cout: lib.seg3d_conv3d_k3_wino_wgrad_workspace_floats(1, 4, 4, W, cin, cout) // (
        ((cin + 31) // 32) * ((cout + 31) // 32) * 36 * 1024)
    assert sl(8, 32, 32) == 1 and sl(16, 32, 32) == 1 and sl(24, 32, 32) == 2 and sl(8 * 511, 32, 32) == 256 and sl(8 * 600, 32, 32) == 256
    assert sl(8 * 600, 36, 44) == 64 and sl(8 * 600, 96, 96) == 28
    # g2_slabs and the reduce16<16> threshold of 64 slabs
    g = lambda W, cin=32: lib.seg3d_conv3d_k3_wino2d_wgrad_variant(1, 4, 4, W, cin, 32)
    assert g(4 * 126) == 0 and g(4 * 127) == 1 and g(4 * 128) == 1             # 63, 64, 64 slabs
    assert g(4 * 600, 96) == 1 and g(4 * 600, 160) == 0                        # caps of 85 and 51
    sl2 = lambda W, cin, cout: lib.seg3d_conv3d_k3_wino2d_wgrad_workspace_floats(1, 4, 4, W, cin, cout) // (
        ((cin + 31) // 32) * ((cout + 31) // 32) * 48 * 1024)
    assert sl2(4, 32, 32) == 1 and sl2(8, 32, 32) == 1 and sl2(12, 32, 32) == 2 and sl2(4 * 511, 32, 32) == 256 and sl2(4 * 600, 32, 32) == 256
    assert sl2(4 * 600, 36, 44) == 64


def test_winograd_restatements_are_the_convolution():
    """the fp32 yardsticks of the device test, run in float64 on a shape with odd tile counts, are the definition's sums in another
    order: 1e-12 of the scale"""
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 4, 6, 12, 5), dtype=torch.float64, generator=g) + 0.5
    w = torch.randn((7, 5, 3, 3, 3), dtype=torch.float64, generator=g)
    dy = torch.randn((2, 4, 6, 12, 7), dtype=torch.float64, generator=g) - 0.25
    ref, gref = _conv_def(x, w), _wgrad_def(x, dy)
    for f in (_wino_f23_conv, _wino_f2x2_conv):
        assert float((f(x, w) - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), f.__name__
    for f in (_wino_f32_wgrad, _wino_f3x3_wgrad):
        assert float((f(x, dy) - gref).abs().max()) <= 1e-12 * float(gref.abs().max()), f.__name__
