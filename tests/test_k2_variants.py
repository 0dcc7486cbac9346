"""Host-only: every case of tests/k2_cases.py reaches the kernel instantiation of csrc/conv_k2_mfma.hip it is named for (through
the seg3d_*k2*_variant queries, which share their selection code with the launchers), and every instantiation the three
launchers can run is named by at least one case -- so a retuned threshold, or a kernel without a test, fails here, without a GPU."""
import ctypes
import os

import pytest

import k2_cases as K


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__  # noqa: F401  (repo root is on sys.path)
    from segmentation3d import _engine
    if not os.path.isfile(_engine.LIB_PATH):
        __graft_entry__.build()
    handle = ctypes.CDLL(_engine.LIB_PATH)
    for name in ('seg3d_conv3d_k2s2_variant', 'seg3d_convT3d_k2s2_variant', 'seg3d_k2_wgrad_variant'):
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _engine._SIGNATURES[name]
    handle.seg3d_last_error.restype = ctypes.c_char_p
    return handle


def gather_query(lib, c):
    return lib.seg3d_conv3d_k2s2_variant(c.N, c.D, c.H, c.W, c.Cin, c.Cout, c.mode, c.out_bf16)


def scatter_query(lib, c):
    return lib.seg3d_convT3d_k2s2_variant(c.N, c.D, c.H, c.W, c.Cin, c.Cout, c.mode, c.out_bf16, int(c.add), c.ld_addend)


def wgrad_query(lib, c):
    return lib.seg3d_k2_wgrad_variant(c.N, c.D, c.H, c.W, c.CA, c.CB, c.bf16)


@pytest.mark.parametrize('case', K.GATHER_CASES, ids=K.case_id)
def test_gather_case_reaches_its_variant(lib, case):
    assert gather_query(lib, case) == K.gather_code(case)
    assert case.ld_x == 0 or (case.ld_x > case.Cin and case.mode == 0)
    assert case.role in ('fwd', 'dgrad')


@pytest.mark.parametrize('case', K.SCATTER_CASES, ids=K.case_id)
def test_scatter_case_reaches_its_variant(lib, case):
    assert scatter_query(lib, case) == K.scatter_code(case)
    assert (case.ld_addend > case.Cout) == case.add      # addends are channel slices
    assert not case.add or case.role == 'dgrad'


@pytest.mark.parametrize('case', K.WGRAD_CASES, ids=K.case_id)
def test_wgrad_case_reaches_its_variant(lib, case):
    assert wgrad_query(lib, case) == K.wgrad_code(case)


def test_every_variant_code_has_a_case():
    assert sorted({K.gather_code(c) for c in K.GATHER_CASES}) == K.ALL_GATHER_CODES
    assert sorted({K.scatter_code(c) for c in K.SCATTER_CASES}) == K.ALL_SCATTER_CODES
    assert sorted({K.wgrad_code(c) for c in K.WGRAD_CASES}) == K.ALL_WGRAD_CODES
    assert len(K.ALL_GATHER_CODES) == 20 and len(K.ALL_SCATTER_CODES) == 32 and len(K.ALL_WGRAD_CODES) == 8


def test_roles_and_edges_are_spread_over_the_kernels():
    """each gather / scatter kernel in both roles, each weight-gradient kernel with both reducers, both layouts and both
    `accumulate` values; N in {1, 3}, ragged extents and partial column blocks on every kernel"""
    for k in K.GATHER_KERNELS:
        cs = [c for c in K.GATHER_CASES if c.kernel == k]
        assert {c.role for c in cs} == {'fwd', 'dgrad'}, k
        assert {1, 3} <= {c.N for c in cs}, k
        assert any(c.Cout % 32 for c in cs) or k == 'direct_2_1', k
    assert {c.kernel for c in K.GATHER_CASES if c.ld_x} == {'staged', 'direct_1_1'}
    assert any(c.kernel == 'direct_2_1' and (c.Cout // 64) % 2 == 1 for c in K.GATHER_CASES)
    for direct in (True, False):
        cs = [c for c in K.SCATTER_CASES if c.direct == direct]
        assert {c.role for c in cs} == {'fwd', 'dgrad'} and {1, 3} <= {c.N for c in cs}
    for k in K.WGRAD_KERNELS:
        cs = [c for c in K.WGRAD_CASES if c.kernel == k]
        assert {(c.reduce4, c.accumulate) for c in cs} == {(False, 0), (True, 1), (False, 1), (True, 0)}, k
        assert {c.swapped for c in cs} == {False, True} and any(max(c.CA, c.CB) > 32 for c in cs), k


@pytest.mark.parametrize('family,args,why', K.REFUSALS, ids=[r[2] for r in K.REFUSALS])
def test_refused_arguments_have_no_variant(lib, family, args, why):
    fn = lib.seg3d_conv3d_k2s2_variant if family == 'gather' else lib.seg3d_convT3d_k2s2_variant
    assert fn(*args) < 0, why
    assert lib.seg3d_last_error()


def test_thresholds_of_the_selection_rules(lib):
    """the grid-size thresholds named in the launchers: 3072 and 16384 gather waves, 256 scatter workgroups, 32 slabs"""
    g = lambda W, Cin, Cout: lib.seg3d_conv3d_k2s2_variant(1, 1, 1, W, Cin, Cout, 0, 0)
    assert g(32 * 767, 32, 32) == 3 and g(32 * 768, 32, 32) == 1          # waves = tiles * 4
    assert g(32 * 2047, 16, 64) == 1 and g(32 * 2048, 16, 64) == 2        # waves = tiles * 2 * 4
    s = lambda W: lib.seg3d_convT3d_k2s2_variant(1, 1, 1, W, 32, 32, 0, 0, 0, 0)
    assert s(32 * 255) == 4 and s(32 * 256) == 0
    w = lambda W: lib.seg3d_k2_wgrad_variant(1, 2, 4, 8 * W, 16, 32, 0)
    assert w(124) == 10 and w(125) == 11
