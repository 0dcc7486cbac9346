"""Host-only: every weight-gradient case of tests/direct_cases.py reaches the kernel of csrc/conv_direct.hip, the chunk count, PAIRS
and the reducer it is named for (through the seg3d_wgrad_direct_* / seg3d_wgrad_reduce_variant queries, which share their selection
code with the launchers), every code of the queries is named by at least one case, and the thresholds of the selection rules sit
where the launchers' comments put them -- so a retuned threshold, or a kernel without a test, fails here, without a GPU."""
import ctypes
import os

import pytest

import direct_cases as K

QUERIES = ('seg3d_wgrad_direct_variant', 'seg3d_wgrad_direct_chunks', 'seg3d_wgrad_direct_pairs', 'seg3d_wgrad_reduce_variant',
           'seg3d_wgrad_direct_workspace_floats')


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


def _args(c):
    ks, stride = K.WGRAD_KS[c.kernel]
    return c.N, c.D, c.H, c.W, c.CA, c.CB, ks, stride


@pytest.mark.parametrize('case', K.WGRAD_CASES, ids=K.case_id)
def test_wgrad_case_reaches_its_plan(lib, case):
    c = case
    assert lib.seg3d_wgrad_direct_variant(*_args(c)) == K.wgrad_code(c)
    assert lib.seg3d_wgrad_direct_chunks(*_args(c)) == c.chunks
    assert lib.seg3d_wgrad_direct_pairs(c.CA, c.CB) == c.pairs
    assert lib.seg3d_wgrad_reduce_variant(c.chunks, K.taps(c), c.CA, c.CB) == K.reduce_code(c)
    # the restated arithmetic agrees, and the workspace holds at least the chunks that are written
    dq, hq, wq = K.q_dims(c)
    chunks, _, last, pairs, _, upper = K.launch_plan(c.N * dq * hq * wq, K.taps(c), c.CA, c.CB)
    assert (chunks, pairs) == (c.chunks, c.pairs) and 0 < last and chunks <= upper
    CBP = (c.CB + 3) // 4 * 4
    assert lib.seg3d_wgrad_direct_workspace_floats(c.N, dq, hq, wq, c.CA, c.CB, K.taps(c)) == upper * K.taps(c) * c.CA * CBP
    assert c.role == 'conv' or c.kernel == 'k2s2'


def test_every_code_has_a_case_and_the_edges_are_spread():
    assert sorted({K.wgrad_code(c) for c in K.WGRAD_CASES}) == K.ALL_WGRAD_CODES
    assert sorted({K.reduce_code(c) for c in K.WGRAD_CASES}) == K.ALL_REDUCE_CODES
    for k in K.WGRAD_KERNELS:
        cs = [c for c in K.WGRAD_CASES if c.kernel == k]
        assert any(c.accumulate for c in cs) and {c.swapped for c in cs} == {False, True}, k
        assert any(c.chunks > 1 for c in cs), k
    for wide in (False, True):                 # (every case also runs with accumulate = 0)
        assert any(c.accumulate for c in K.WGRAD_CASES if c.wide == wide)
    assert {c.kernel for c in K.WGRAD_CASES if c.wide} == {'k3', 'k1_thin'}       # the generic and the thin kernel in front of it
    assert any(c.role == 'convT' for c in K.WGRAD_CASES)
    # ragged last chunks, idle pair lanes, a second row of pairs, one voxel lane
    for i, last in K.LAST_CHUNK.items():
        c = K.WGRAD_CASES[i]
        dq, hq, wq = K.q_dims(c)
        plan = K.launch_plan(c.N * dq * hq * wq, K.taps(c), c.CA, c.CB)
        assert plan[2] == last and last != plan[1]
    quads = lambda c: c.CA * ((c.CB + 3) // 4)
    generic = [c for c in K.WGRAD_CASES if c.kernel != 'k1_thin']
    assert any(quads(c) < c.pairs for c in generic) and any(quads(c) > 256 and quads(c) % 256 for c in generic)
    assert any(c.pairs == 256 for c in generic) and any(c.CB % 4 for c in generic) and any(c.CB % 4 == 0 for c in generic)


def test_forward_cases_cover_every_branch():
    """per kernel: float4 and scalar loads, whole and partial last quads, both roles, N in {1, 3}, a second grid-stride trip"""
    for k in K.FWD_KERNELS:
        cs = [c for c in K.FWD_CASES if c.kernel == k]
        assert {c.Cin % 4 == 0 for c in cs} == {False, True}, k
        assert {c.Cout % 4 == 0 for c in cs} == {False, True}, k
        assert {c.role for c in cs} == {'fwd', 'dgrad'} and {1, 3} <= {c.N for c in cs}, k
        assert any(K.items(c) > K.ITEMS_PER_TRIP for c in cs), k
        assert all(K.items(c) < 2 * K.ITEMS_PER_TRIP for c in cs), k            # (no larger than the second trip needs)
        if k in ('k3', 'k1'):
            assert any(1 in (c.D, c.H, c.W) for c in cs) and any(c.D % 2 and c.H % 2 and c.W % 2 for c in cs), k
        if k == 'k2s2':
            assert all(c.D % 2 == 0 and c.H % 2 == 0 and c.W % 2 == 0 for c in cs)
    assert {c.Cout % 4 for c in K.FWD_CASES} == {0, 1, 2, 3}
    tails = K.TAIL_CASES
    assert {c.C for c in tails} == {1, 2, 5, 16} and {c.op for c in tails} == {'softmax', 'sigmoid'}
    assert all(any(c.op == op and c.N * c.S > K.ITEMS_PER_TRIP and c.C == 2 for c in tails) for op in ('softmax', 'sigmoid'))
    assert all(c.S % 256 for c in tails)


def test_thresholds_of_the_selection_rules(lib):
    v = lambda CA, CB: lib.seg3d_wgrad_direct_variant(1, 4, 6, 8, CA, CB, 1, 1)
    assert (v(8, 8), v(9, 8), v(8, 9), v(1, 1)) == (3, 2, 2, 3)                  # thin 1x1x1: CA <= 8 && CB <= 8
    assert lib.seg3d_wgrad_direct_variant(1, 4, 6, 8, 2, 2, 3, 1) == 0 and lib.seg3d_wgrad_direct_variant(1, 4, 6, 8, 2, 2, 2, 2) == 1
    r = lib.seg3d_wgrad_reduce_variant
    assert (r(511, 8, 16, 16), r(512, 8, 16, 16), r(512, 1, 3, 683), r(700, 1, 1, 1), r(1, 1, 1, 1)) == (0, 1, 0, 1, 0)
    assert r(0, 1, 1, 1) < 0 and r(1, 1, 0, 1) < 0 and lib.seg3d_last_error()
    # PAIRS: the (a, b-quad) pairs rounded up to a power of two, 256 at most
    p = lib.seg3d_wgrad_direct_pairs
    assert [p(n, 4) for n in (1, 2, 3, 4, 5, 128, 129, 255, 256, 257, 4096)] == [1, 2, 4, 4, 8, 128, 256, 256, 256, 256, 256]
    assert (p(1, 1), p(1, 4), p(1, 5), p(3, 8), p(3, 9)) == (1, 1, 2, 8, 16)
    assert p(0, 4) < 0 and p(4, 0) < 0
    # chunks: one per 2048 voxels, 512 at most, re-divided so that none is empty
    ch = lambda W, CA=2, CB=2, ks=1: lib.seg3d_wgrad_direct_chunks(1, 1, 1, W, CA, CB, ks, 1)
    assert (ch(1), ch(2048), ch(2049), ch(511 * 2048), ch(511 * 2048 + 1), ch(1 << 24)) == (1, 1, 2, 511, 512, 512)
    assert ch(5 * 2048 + 5) == 6 and ch(10 * 2048 + 1) == 11
    for W in (1, 7, 2049, 12289, 14858, 1048131, 3000001):
        for (CA, CB, ks) in ((2, 3, 1), (5, 5, 1), (3, 5, 3), (64, 64, 3), (40, 24, 1)):
            plan = K.launch_plan(W, ks ** 3, CA, CB)
            assert ch(W, CA, CB, ks) == plan[0] and (plan[0] - 1) * plan[1] < W <= plan[0] * plan[1], (W, CA, CB, ks)


def test_slab_cap(lib):
    """at most 64 MiB of partial slabs: 27 x 64 x 64 floats per slab leave room for 151, fewer than the 160 chunks of 2048 voxels
    (host only: reaching the cap on a device takes 3.4e10 multiply-adds in a VALU kernel)"""
    N, D, H, W, CA, CB = 1, 64, 64, 80, 64, 64
    slab = 27 * CA * CB
    floats = lib.seg3d_wgrad_direct_workspace_floats(N, D, H, W, CA, CB, 27)
    cap = (64 << 20) // (slab * 4)
    assert cap == 151 and (N * D * H * W + 2047) // 2048 == 160
    assert floats == cap * slab and floats * 4 <= (64 << 20) < (floats + slab) * 4
    chunks = lib.seg3d_wgrad_direct_chunks(N, D, H, W, CA, CB, 3, 1)
    assert chunks == K.launch_plan(N * D * H * W, 27, CA, CB)[0] == 151
    # below the cap the same voxels give the uncapped count
    assert lib.seg3d_wgrad_direct_chunks(N, D, H, W, 32, 32, 3, 1) == 160
    assert lib.seg3d_wgrad_direct_workspace_floats(N, D, H, W, 32, 32, 27) == 160 * 27 * 32 * 32
    # a slab above 64 MiB on its own still gets one chunk
    assert lib.seg3d_wgrad_direct_workspace_floats(1, 4, 4, 4, 1024, 1024, 27) == 27 * 1024 * 1024
    assert lib.seg3d_wgrad_direct_chunks(1, 4, 4, 4, 1024, 1024, 3, 1) == 1


@pytest.mark.parametrize('args,why', K.REFUSALS, ids=[r[1] for r in K.REFUSALS])
def test_refused_arguments_have_no_variant(lib, args, why):
    assert lib.seg3d_wgrad_direct_variant(*args) < 0, why
    assert lib.seg3d_last_error().startswith(b'seg3d_wgrad_direct:'), why
    assert lib.seg3d_wgrad_direct_chunks(*args) < 0, why
