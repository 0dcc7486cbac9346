"""Host-only: every case of tests/k3_cases.py reaches the kernels of csrc/conv_mfma.hip it is named for (through the
seg3d_conv3d_k3_*_variant, *_workspace_floats and *_stats_count queries, which run the plan functions the launchers run), every
kernel the launchers can reach is named by a case, and the edges the device test relies on (second trip of the persistent loop,
short last K slab, ragged extents, partial column blocks, roles, optional operands) are spread over all of them -- so a retuned
cost model, or a kernel without a test, fails here, without a GPU.  The cost model prices 256 CUs whatever the device has."""
import ctypes
import os

import pytest

import k3_cases as K

QUERIES = ('seg3d_conv3d_k3_mfma_variant', 'seg3d_conv3d_k3_bf16_variant', 'seg3d_conv3d_k3_mfma_fwd_workspace_floats',
           'seg3d_conv3d_k3_bf16_fwd_workspace_floats', 'seg3d_conv3d_k3_mfma_stats_count', 'seg3d_conv3d_k3_bf16_stats_count',
           'seg3d_conv3d_k3_wgrad_variant', 'seg3d_conv3d_k3_mfma_wgrad_workspace_floats',
           'seg3d_conv3d_k3_bf16_wgrad_workspace_floats')


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
    handle.seg3d_last_error.restype = ctypes.c_char_p
    return handle


def fwd_plan(lib, c):
    """(code, K slabs, work items of a persistent launch or None), all from the queries"""
    t = 'bf16' if c.bf16 else 'mfma'
    dims = (c.N, c.D, c.H, c.W, c.Cin, c.Cout)
    code = getattr(lib, 'seg3d_conv3d_k3_{}_variant'.format(t))(*dims)
    ws = getattr(lib, 'seg3d_conv3d_k3_{}_fwd_workspace_floats'.format(t))(*dims)
    cnt = getattr(lib, 'seg3d_conv3d_k3_{}_stats_count'.format(t))(*dims)
    vox = c.N * c.D * c.H * c.W * c.Cout
    assert ws % vox == 0
    ks = ws // vox if ws else 1
    items = None
    if code >= 100 and ks == 1:
        assert (c.N * cnt) % K.waves(c) == 0
        items = c.N * cnt // K.waves(c)
    return code, ks, items


def short_last_slab(c, ks):
    cpk = -(-K.chunks(c) // ks)
    return K.chunks(c) % cpk != 0


def wgrad_slabs(lib, c):
    fn = lib.seg3d_conv3d_k3_bf16_wgrad_workspace_floats if c.bf16 else lib.seg3d_conv3d_k3_mfma_wgrad_workspace_floats
    npairs = ((c.Cin + 31) // 32) * ((c.Cout + 31) // 32)
    ws = fn(c.N, c.D, c.H, c.W, c.Cin, c.Cout)
    assert ws % (npairs * 27 * 1024) == 0
    return ws // (npairs * 27 * 1024)


@pytest.mark.parametrize('case', K.FWD_CASES, ids=K.case_id)
def test_fwd_case_reaches_its_variant(lib, case):
    c = case
    code, ks, items = fwd_plan(lib, c)
    assert code == K.fwd_code(c) and (ks > 1) == c.splitk
    assert (items is not None) == K.persistent(c)
    if K.persistent(c):
        want = K.ITEM_CLASS[c]
        assert (items > K.CUS and items % K.CUS != 0) if want == 'many' else items < K.CUS, items
    assert c.role in ('fwd', 'dgrad') and c.bf16 == int(c.kernel in range(200, 300) or c.kernel >= 400)
    assert c.Cin % (16 if c.bf16 else 4) == 0 and (c.out_bf16 == 0 or c.bf16)
    assert c.Cout % 4 == 0 or (c.kernel < 100 and not c.addend)            # (a float4 addend needs whole quads)
    # the size limits of the table
    assert c.N * c.D * c.H * c.W * 27 * c.Cin * c.Cout <= 1.5e9 and c.N * c.D * c.H * c.W * max(c.Cin, c.Cout) <= 4e6


@pytest.mark.parametrize('case', K.WGRAD_CASES, ids=K.case_id)
def test_wgrad_case_reaches_its_variant(lib, case):
    c = case
    assert lib.seg3d_conv3d_k3_wgrad_variant(c.N, c.D, c.H, c.W, c.Cin, c.Cout, c.bf16) == K.wgrad_code(c)
    assert (wgrad_slabs(lib, c) >= 32) == (c.reducer == 16) and c.reducer in (4, 16)


def test_every_reachable_kernel_has_a_case():
    assert sorted({(c.bf16, c.kernel, c.splitk) for c in K.FWD_CASES}) == K.ALL_FWD
    assert sorted({K.wgrad_code(c) for c in K.WGRAD_CASES}) == K.ALL_WGRAD_CODES
    assert len(K.ALL_FWD) == 27 and len(K.ALL_WGRAD_CODES) == 16
    assert {k for (_, k, _) in K.ALL_FWD} == set(K.FWD_KERNELS)


def test_fwd_edges_are_spread_over_the_kernels(lib):
    for key in K.ALL_FWD:
        bf16, code, splitk = key
        cs = [c for c in K.FWD_CASES if (c.bf16, c.kernel, c.splitk) == key]
        assert {c.role for c in cs} == {'fwd', 'dgrad'}, key
        assert {1, 3} <= {c.N for c in cs} or ((bf16, code) in K.N3_ONLY and 3 in {c.N for c in cs}), key
        assert any(K.ragged(c) for c in cs), key
        assert any(K.partial_block(c) for c in cs), key
        if bf16:
            assert {c.out_bf16 for c in cs} == {0, 1}, key
        if splitk:       # a last K slab shorter than the others
            assert any(short_last_slab(c, fwd_plan(lib, c)[1]) for c in cs), key
        elif code >= 100:
            classes = {K.ITEM_CLASS[c] for c in cs}
            assert classes == ({'few'} if (bf16, code) in K.NO_MANY_ITEMS else {'few', 'many'}), key
    # all four (bias, addend) combinations on each kernel body, fp32 and bf16
    for bf16 in (0, 1):
        for b in ('gen1', 'v2', 'v2_splitk', 'w8'):
            if bf16 and b == 'gen1':
                continue
            combos = {(c.bias, c.addend) for c in K.FWD_CASES if c.bf16 == bf16 and K.body(c) == b}
            assert combos == {(0, 0), (0, 1), (1, 0), (1, 1)}, (bf16, b)
    for c in K.FWD_CASES:
        if (c.bias, c.addend) not in ((1, 1), (0, 0)):
            assert (c.bias, c.addend) == ((1, 0) if c.role == 'fwd' else (0, 1)), c
    # the first-generation kernel: a half chunk, Cout % 4 != 0, and its own split-K
    gen1 = [c for c in K.FWD_CASES if c.kernel < 100]
    assert all(c.Cin % 8 == 4 or c.Cout % 4 for c in gen1)
    assert any(c.Cin % 8 == 4 and c.splitk for c in gen1) and any(c.Cout % 4 for c in gen1)
    # split-K with a bf16 output: the bf16-out finish kernel
    assert any(c.splitk and c.out_bf16 and c.bias for c in K.FWD_CASES) and any(c.splitk and c.out_bf16 and c.addend for c in K.FWD_CASES)


def test_wgrad_edges_are_spread_over_the_kernels(lib):
    for k in K.WGRAD_KERNELS:
        cs = [c for c in K.WGRAD_CASES if c.kernel == k]
        assert {(c.reducer, c.accumulate) for c in cs} == {(4, 0), (4, 1), (16, 0), (16, 1)}, k
        assert any(c.N == 3 and c.Cin % 32 and c.Cout % 32 and c.Cin != c.Cout for c in cs), k
    off = lambda c: (bool(c.D % 4), bool(c.H % 4), bool(c.W % K.WGRAD_TILES[K.WGRAD_KERNELS[c.kernel]][2]))
    for k in ('wgrad3_8_irr', 'wgrad3_4_irr'):
        assert {(True, False, False), (False, True, False), (False, False, True), (True, True, True)} <= \
            {off(c) for c in K.WGRAD_CASES if c.kernel == k}, k
    for k in ('wgrad3_8', 'wgrad3_4'):
        assert all(off(c) == (False, False, False) for c in K.WGRAD_CASES if c.kernel == k)
    # the two fallbacks on the shapes they are the fallback for
    for k in ('wgrad2_4x4x8', 'widening'):
        assert any(off(c) == (True, True, True) for c in K.WGRAD_CASES if c.kernel == k), k
    slabs = [(wgrad_slabs(lib, c), K.wgrad_tiles(c)) for c in K.WGRAD_CASES]
    assert any(s == 1 for s, _ in slabs) and any(t % s for s, t in slabs)


@pytest.mark.parametrize('family,dims,why', K.REFUSALS, ids=[r[2] for r in K.REFUSALS])
def test_refused_arguments(lib, family, dims, why):
    """what the host can see of a refusal (the launchers themselves are called in tests/test_gpu_k3_float64.py)"""
    if family == 'fp32':          # the forward query has no failure code; the weight-gradient one shares the rule
        assert dims[4] % 4 and lib.seg3d_conv3d_k3_wgrad_variant(*dims, 0) < 0 and lib.seg3d_last_error(), why
    elif family == 'bf16':
        assert lib.seg3d_conv3d_k3_bf16_variant(*dims) == 0 and lib.seg3d_conv3d_k3_bf16_stats_count(*dims) == 0, why
    else:
        fn = lib.seg3d_conv3d_k3_mfma_fwd_workspace_floats if family == 'fp32_no_ws' else lib.seg3d_conv3d_k3_bf16_fwd_workspace_floats
        assert fn(*dims) > 0, why


def test_wgrad_query_refuses_what_the_launchers_refuse(lib):
    q = lib.seg3d_conv3d_k3_wgrad_variant
    for bf16 in (0, 1):
        assert q(1, 4, 4, 8, 32, 32, bf16) >= 0
        for args in ((0, 4, 4, 8, 32, 32), (1, 4, 4, 8, 30, 32), (1, 4, 4, 8, 32, 34), (8, 128, 128, 128, 128, 128)):
            assert q(*args, bf16) < 0 and lib.seg3d_last_error(), args
    assert q(1, 1024, 1024, 1024, 4, 4, 0) < 0             # fp32: 2^31 elements before the 2^22-tile limit can be met


def test_thresholds_of_the_selection_rules(lib):
    """the thresholds named in the plan functions, from both sides"""
    v = lib.seg3d_conv3d_k3_mfma_variant
    ws = lib.seg3d_conv3d_k3_mfma_fwd_workspace_floats
    # seg3d_fwd_ksplit (first generation, Cin % 8 == 4): cib < 4 never splits, cib == 4 does
    assert v(1, 5, 5, 5, 20, 4) == 1 and ws(1, 5, 5, 5, 20, 4) == 0                      # cib 3
    assert v(1, 5, 5, 5, 28, 4) == 1 and ws(1, 5, 5, 5, 28, 4) == 2 * 125 * 4            # cib 4: two slabs
    # ... and wgs >= 192: (1, 2, W) volumes get 1 x 2 x 32 tiles, one workgroup per 32 voxels of W
    assert v(1, 1, 2, 32 * 191, 28, 4) == 1 and ws(1, 1, 2, 32 * 191, 28, 4) > 0
    assert v(1, 1, 2, 32 * 191 + 1, 28, 4) == 1 and ws(1, 1, 2, 32 * 191 + 1, 28, 4) == 0
    # the 16-wave reducer: slabs >= 32.  4 x 4 x 8 tiles, one channel-block pair: slabs = (tiles + 1) / 2
    w = lambda W, bf16: lib.seg3d_conv3d_k3_wgrad_variant(1, 4, 4, 8 * W, 32, 32, bf16)
    assert w(62, 0) == 0 and w(63, 0) == 1 and w(62, 1) == 30 and w(63, 1) == 31
    w7 = lambda W: lib.seg3d_conv3d_k3_wgrad_variant(1, 4, 4, 8 * W, 12, 32, 1)           # widening: slabs = (tiles + 3) / 4
    assert w7(124) == 70 and w7(125) == 71
    # nw = 8: whole-K plans with one column block per item and two or four row blocks per wave go to the 8-wave kernels
    # (fp32 ma in {2, 4}; bf16 ma >= 2), so their slot count is 8 per item and the 4-wave codes x21 / x41 appear split-K only
    for c in K.FWD_CASES:
        code, ks, items = fwd_plan(lib, c)
        if ks == 1:
            assert code not in (121, 141, 221, 231, 241), c
        t = 'bf16' if c.bf16 else 'mfma'
        cnt = getattr(lib, 'seg3d_conv3d_k3_{}_stats_count'.format(t))(c.N, c.D, c.H, c.W, c.Cin, c.Cout)
        if ks > 1:
            assert cnt == -(-c.D * c.H * c.W * c.Cout // 4096), c
    # the same (2, 8 -> 4 / 36) volume on both sides of the rule: 131 (ma 3, four waves) against 311 / 321
    assert v(3, 13, 25, 49, 8, 4) == 131 and v(3, 5, 25, 65, 8, 4) == 311 and v(1, 25, 25, 65, 8, 36) == 321
