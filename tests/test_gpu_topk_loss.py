"""The Dice + top-k loss kernels (seg3d_topk_loss_fwd / _bwd) on the GPU against the float64 oracle of
tests/test_topk_loss.py, evaluated on the same float32 probabilities: selection integers, threshold, selected set, loss,
gradient; ties; edges; run-to-run and hipGraph behaviour; training.

Every parity case first asserts the oracle's own margin: the relative gap between the k-th and the (k+1)-th largest float64
per-voxel loss is at least 1e-5 (the fp32 error of a per-voxel loss is about 2e-7), unless the two are exactly equal --
equal float32 inputs, a tie in every precision.  With that margin the selection is compared exactly.  Bars: the integers
exact, tau within 4 ulp of the fp32 value of the oracle's k-th element, the three loss figures within
1e-4 * max(1, |ref|), gpu_util.rel_err(grad) < 1e-4 (the project's parity bars), exact zeros where the definition says
zero.  Measured on the MI355X over this file's cases: DESIGN.md section 7, row f15."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401
from gpu_util import rel_err, report
from oracle import detgen
from test_gpu_compound_loss import _inputs
from test_topk_loss import TIE_CASES, tie_fixture, topk_oracle

pytestmark = pytest.mark.gpu

SEED = 2
WEIGHTS = [1.0, 2.0, 3.0, 0.5, 1.5]
IGNORE = dict(ignore_frac=0.2, out_of_range=True)

# (id, C, shape, k_percent, ignored)
CASES = [('5x7x9_C{}'.format(C), C, (2, 5, 7, 9), 10.0, False) for C in (1, 2, 3, 5, 16)]        # scalar path
CASES += [('4x4x8_C3_k25', 3, (2, 4, 4, 8), 25.0, False),                                        # 16-byte path
          ('1x1x1_C2', 2, (1, 1, 1, 1), 10.0, False),
          ('17^3_C3', 3, (3, 17, 17, 17), 10.0, False),
          ('33x32x32_C2', 2, (2, 33, 32, 32), 10.0, False),                                      # several workgroups (66 of a cap of 512:
          ('33x32x32_C5', 5, (2, 33, 32, 32), 10.0, False)]                                      # no stride; tests/compound_cases.py has those)
CASES += [('5x7x9_C{}_ignore'.format(C), C, (2, 5, 7, 9), 10.0, True) for C in (1, 2, 3, 5, 16)]
CASES += [('17^3_C3_ignore', 3, (3, 17, 17, 17), 10.0, True)]
CASES += [('5x7x9_C3_k{}'.format(k), 3, (2, 5, 7, 9), k, False) for k in (0.01, 50.0, 100.0)]


def _weights(C, weighted):
    if not weighted:
        return None
    return (WEIGHTS * 4)[:C] if C > 5 else WEIGHTS[:C]


def _gpu(dev, p, t, C, **opts):
    from segmentation3d.loss.topk_loss import DiceTopKLoss
    loss_fn = DiceTopKLoss(C, **opts)
    pg = p.to(dev).requires_grad_(True)
    loss = loss_fn(pg, t.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return {'loss': loss.detach().cpu(), 'terms': loss_fn.last_terms.detach().cpu(),
            'selection': tuple(int(v) for v in loss_fn.last_selection.cpu()),
            'tau': loss_fn.last_threshold.detach().cpu(), 'grad': pg.grad.detach().cpu()}


def _ulps(a, b):
    """distance of two non-negative float32 values in units of the last place"""
    ia = int(np.float32(a).view(np.int32))
    ib = int(np.float32(b).view(np.int32))
    return abs(ia - ib)


def _assert_margin(o):
    assert o['margin'] >= 1e-5 or o['margin'] == 0.0, o['margin']   # 0.0: exactly equal values of equal float32 inputs


def _dead_planes(t, C, ignore_label):
    valid = (t >= 0) & (t < C)
    if ignore_label is not None:
        valid = valid & (t != float(ignore_label))
    return (~valid).expand(-1, C, *([-1] * (t.dim() - 2)))


def _check(name, dev, p, t, C, **opts):
    assert float(p.min()) > 1e-9                         # the comparison never sits on the clamp's kink
    ign = opts.get('ignore_label')
    # the oracle: all terms with autograd's gradient, and the top-k term alone for the selected set
    pr = p.clone().requires_grad_(True)
    o = topk_oracle(pr, t, **opts)
    _assert_margin(o)
    (ref_grad,) = torch.autograd.grad(o['total'], pr)
    got = _gpu(dev, p, t, C, **opts)
    assert got['selection'] == o['selection'], (got['selection'], o['selection'])
    n, k, m, n_eq, r = o['selection']
    tau_ulps = _ulps(float(got['tau']), o['tau'])
    terms = got['terms']
    refs = [o['total'].item(), o['region'].item(), o['topk'].item()]
    errs = {'loss': abs(float(terms[0]) - refs[0]), 'region': abs(float(terms[1]) - refs[1]),
            'topk': abs(float(terms[2]) - refs[2]), 'dprobs_rel': rel_err(got['grad'], ref_grad), 'tau_ulps': float(tau_ulps)}
    report('topk_' + name, **errs)
    print('topk_' + name, got['selection'], errs)
    assert float(got['loss']) == float(terms[0])
    assert torch.isfinite(terms).all() and torch.isfinite(got['grad']).all()
    assert tau_ulps <= 4, (float(got['tau']), o['tau'])
    for key, ref in zip(('loss', 'region', 'topk'), refs):
        assert errs[key] < 1e-4 * max(1.0, abs(ref)), errs
    assert errs['dprobs_rel'] < 1e-4, errs
    dead = _dead_planes(t, C, ign)
    if bool(dead.any()):
        assert float(got['grad'][dead].abs().max()) == 0.0
    # the selected set, exactly: the top-k term alone leaves a gradient on plane c == t of the selected voxels only
    alone = dict(opts, dice_weight=0.0)
    g0 = _gpu(dev, p, t, C, **alone)
    assert g0['selection'] == o['selection']
    N = p.shape[0]
    onplane = torch.zeros(N, C, p[0, 0].numel(), dtype=torch.bool)
    tt = t.reshape(N, -1)
    for c in range(C):
        onplane[:, c] = (tt == c) & o['valid'] & (o['w'] > 0)
    assert torch.equal((g0['grad'] != 0).reshape(N, C, -1), onplane)
    qr = p.clone().requires_grad_(True)
    o0 = topk_oracle(qr, t, **alone)
    (ref0,) = torch.autograd.grad(o0['total'], qr)
    e0 = rel_err(g0['grad'], ref0)
    report('topk_' + name + '_alone', dprobs_rel=e0, loss=abs(float(g0['terms'][0]) - o0['total'].item()))
    assert e0 < 1e-4 and abs(float(g0['terms'][0]) - o0['total'].item()) < 1e-4 * max(1.0, abs(o0['total'].item()))
    return errs


@pytest.mark.parametrize('weighted', [False, True], ids=['unit', 'weighted'])
@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_forward_backward_equal_the_oracle(hip_device, case, weighted):
    name, C, shape, k_percent, ignored = case
    p, t = _inputs(SEED, shape, C, **(IGNORE if ignored else {}))
    opts = dict(weights=_weights(C, weighted), k_percent=k_percent)
    if ignored:
        opts['ignore_label'] = 255
    _check('{}_{}'.format(name, 'w' if weighted else 'u'), hip_device, p, t, C, **opts)


# ---- ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k_percent', list(TIE_CASES))
def test_tie_fixture(hip_device, k_percent):
    """three plateaus (30 x ln 8, 50 x ln 4, 120 x ln 2): the integers exact, the tied voxels share the r places equally"""
    p, t = tie_fixture()
    got = _gpu(hip_device, p, t, 2, k_percent=k_percent, dice_weight=0.0)
    n, k, m, n_eq, r = TIE_CASES[k_percent]
    assert got['selection'] == (n, k, m, n_eq, r)
    o = topk_oracle(p, t, k_percent=k_percent, dice_weight=0.0)
    assert o['selection'] == got['selection']
    assert abs(float(got['terms'][2]) - o['topk'].item()) < 1e-6 and _ulps(float(got['tau']), o['tau']) <= 4
    g1, p1 = got['grad'][0, 1].reshape(-1), p[0, 1].reshape(-1)
    assert float(got['grad'][0, 0].abs().max()) == 0.0
    tau_p = min((0.125, 0.25, 0.5), key=lambda v: abs(-math.log(v) - o['tau']))   # the plateau tau sits on
    tied = g1[p1 == tau_p]
    assert tied.numel() == n_eq
    assert bool((tied == tied[0]).all())                                   # bit-equal to each other
    expect = -(r / n_eq) / (k * tau_p)
    assert abs(float(tied[0]) - expect) <= 1e-6 * abs(expect)
    above = g1[p1 < tau_p]
    assert above.numel() == m
    if m:
        assert float(((above.double() + 1.0 / (k * p1[p1 < tau_p].double())).abs() * k * p1[p1 < tau_p].double()).max()) < 1e-6
    assert float(g1[p1 > tau_p].abs().max() if bool((p1 > tau_p).any()) else 0.0) == 0.0
    w_sum = float((g1.double() * (-(k * p1.double()))).sum())                 # sum w_v == k
    assert abs(w_sum - k) < 1e-4 * k


def test_one_hot_probabilities(hip_device):
    """every ell is -0.0 -> +0: tau == 0, L_topk == 0.0 exactly, the gradient is -1 / n on every counted voxel"""
    C = 3
    _, t = _inputs(SEED, (2, 5, 7, 9), C, ignore_frac=0.2)
    t0 = torch.where(t == 255.0, torch.zeros_like(t), t)
    p = torch.stack([(t0[:, 0] == c).float() for c in range(C)], dim=1)
    got = _gpu(hip_device, p, t, C, k_percent=10.0, ignore_label=255, dice_weight=0.0)
    n = int((t != 255.0).sum())
    k = max(1, int(n * 10.0 / 100.0))
    assert got['selection'] == (n, k, 0, n, k)
    assert float(got['tau']) == 0.0 and math.copysign(1.0, float(got['tau'])) == 1.0
    assert float(got['terms'][2]) == 0.0 and float(got['loss']) == 0.0
    G = got['grad'].reshape(2, C, -1)
    tt = t.reshape(2, -1)
    for c in range(C):
        on = tt == c
        assert torch.allclose(G[:, c][on].double(), torch.full((int(on.sum()),), -1.0 / n, dtype=torch.float64), rtol=1e-6, atol=0.0)
        assert float(G[:, c][~on].abs().max()) == 0.0


def test_half_certain_half_even(hip_device):
    """half of the voxels at p_t = 1 (ell = -0.0), half at 0.5, k = 10 %: tau = ln 2 and m = 0 -- a -0.0 keyed as the largest
    value would put tau at 0"""
    S = 5 * 5 * 8
    p1 = torch.cat([torch.ones(S // 2), torch.full((S // 2,), 0.5)])
    p1 = p1[torch.randperm(S, generator=torch.Generator().manual_seed(1))].reshape(1, 1, 5, 5, 8)
    p = torch.cat([1.0 - p1, p1], dim=1).float()
    t = torch.ones(1, 1, 5, 5, 8)
    got = _gpu(hip_device, p, t, 2, k_percent=10.0, dice_weight=0.0)
    assert got['selection'] == (S, S // 10, 0, S // 2, S // 10)
    assert _ulps(float(got['tau']), math.log(2.0)) <= 4
    assert abs(float(got['terms'][2]) - math.log(2.0)) < 1e-6
    g1 = got['grad'][0, 1].reshape(-1)
    assert float(g1[p1.reshape(-1) == 1.0].abs().max()) == 0.0


def test_clamped_voxels_are_selected_first_and_send_no_gradient(hip_device):
    C = 3
    p, t = _inputs(SEED, (2, 5, 7, 9), C)
    P, tt = p.reshape(2, C, -1), t.reshape(2, -1)
    where = [(0, 0), (0, 17), (1, 314)]
    for n, s in where:
        c = int(tt[n, s])
        P[n, (c + 1) % C, s] += P[n, c, s]
        P[n, c, s] = 0.0
    got = _gpu(hip_device, p, t, C, k_percent=10.0, dice_weight=0.0)
    o = topk_oracle(p, t, k_percent=10.0, dice_weight=0.0)
    assert o['margin'] >= 1e-5
    assert got['selection'] == o['selection'] and got['selection'][2] >= len(where)
    assert abs(float(got['terms'][2]) - o['topk'].item()) < 1e-4 * o['topk'].item()
    assert o['topk'].item() > len(where) * (-math.log(1e-12)) / got['selection'][1]
    G = got['grad'].reshape(2, C, -1)
    for n, s in where:
        assert float(G[n, :, s].abs().max()) == 0.0


# ---- edges --------------------------------------------------------------------------------------------------------------
def test_everything_ignored(hip_device):
    C = 3
    p, t = _inputs(SEED, (2, 5, 7, 9), C)
    t[:] = 255.0
    got = _gpu(hip_device, p, t, C, ignore_label=255)
    assert got['selection'] == (0, 0, 0, 0, 0)
    assert float(got['terms'][2]) == 0.0 and torch.isfinite(got['terms']).all()
    assert float(got['grad'].abs().max()) == 0.0


def test_one_counted_voxel(hip_device):
    C = 3
    p, t = _inputs(SEED, (2, 5, 7, 9), C)
    t[:] = 255.0
    t[1, 0, 2, 3, 4] = 1.0
    got = _gpu(hip_device, p, t, C, ignore_label=255, dice_weight=0.0)
    pt = float(p[1, 1, 2, 3, 4])
    assert got['selection'] == (1, 1, 0, 1, 1)
    assert abs(float(got['terms'][2]) + math.log(pt)) < 1e-6
    assert abs(float(got['grad'][1, 1, 2, 3, 4]) + 1.0 / pt) < 1e-6 / pt
    assert int((got['grad'] != 0).sum()) == 1


def test_term_weights_and_agreement_with_dicece(hip_device):
    """ce_weight = 0: the Dice term alone, L_region that of DiceCELoss; dice_weight = 0: planes c != t exactly zero;
    k_percent = 100 with unit weights is DiceCELoss(gamma = 0)"""
    from segmentation3d.loss.compound_loss import DiceCELoss
    C = 3
    p, t = _inputs(SEED, (3, 17, 17, 17), C, **IGNORE)
    dev = hip_device

    def dicece(**opts):
        fn = DiceCELoss(C, ignore_label=255, **opts)
        pg = p.to(dev).requires_grad_(True)
        loss = fn(pg, t.to(dev))
        loss.backward()
        torch.cuda.synchronize()
        return loss.item(), fn.last_terms.cpu(), pg.grad.cpu()

    ref = dicece(gamma=0.0)
    dice_only = _gpu(dev, p, t, C, ignore_label=255, ce_weight=0.0)
    assert float(dice_only['terms'][1]) == float(ref[1][1])     # the same forward code: the same number
    assert float(dice_only['loss']) == float(dice_only['terms'][1])
    ref_dice = dicece(ce_weight=0.0)
    assert rel_err(dice_only['grad'], ref_dice[2]) < 1e-6
    for shape in ((2, 5, 7, 9), (2, 16, 20, 24)):               # the scalar path; the 16-byte path over two workgroups
        ps, ts = _inputs(SEED, shape, C, **IGNORE)
        ce = DiceCELoss(C, ignore_label=255)
        ce(ps.to(dev), ts.to(dev))
        got = _gpu(dev, ps, ts, C, ignore_label=255, ce_weight=0.0)
        print('topk_region_vs_dicece', shape, float(got['terms'][1]), float(ce.last_terms[1]))
        assert np.float32(float(got['terms'][1])).tobytes() == np.float32(float(ce.last_terms[1])).tobytes()

    topk_only = _gpu(dev, p, t, C, ignore_label=255, dice_weight=0.0)
    for c in range(C):
        assert float(topk_only['grad'][:, c:c + 1][t != c].abs().max()) == 0.0
    assert abs(float(topk_only['loss']) - float(topk_only['terms'][2])) < 1e-7

    full = _gpu(dev, p, t, C, ignore_label=255, k_percent=100.0)
    errs = {'loss': abs(float(full['loss']) - ref[0]), 'dprobs_rel': rel_err(full['grad'], ref[2])}
    report('topk_k100_vs_dicece', **errs)
    print('topk_k100_vs_dicece', errs)
    assert errs['loss'] < 1e-6 and errs['dprobs_rel'] < 1e-6, errs
    n = full['selection'][0]
    assert full['selection'][1] == n and full['selection'][2] + full['selection'][4] == n


def test_entry_refuses_bad_arguments(hip_device):
    from segmentation3d import _engine as E
    from segmentation3d.loss.topk_loss import DiceTopKLoss
    dev = hip_device
    N, S = 1, 64
    t = torch.zeros(N, S, device=dev)
    w = torch.ones(17, device=dev)
    work = torch.zeros(1 << 16, dtype=torch.int64, device=dev)
    ell, coef, terms = torch.zeros(N * S, device=dev), torch.zeros(64, device=dev), torch.zeros(3, device=dev)
    sel, thr = torch.zeros(5, dtype=torch.int64, device=dev), torch.zeros(1, device=dev)

    def call(C, k_percent):
        p = torch.full((N, max(C, 1), S), 0.5, device=dev)
        E.call('seg3d_topk_loss_fwd', E.ptr(p), E.ptr(t), E.ptr(w), E.ptr(w), E.ptr(work), E.ptr(ell), E.ptr(coef),
               E.ptr(terms), E.ptr(sel), E.ptr(thr), N, C, S, float(k_percent), 1.0, 1.0, 0, -1.0, E.stream_ptr())

    for C, k_percent in ((0, 10.0), (17, 10.0), (2, 0.0), (2, 101.0), (2, float('nan'))):
        with pytest.raises(ValueError):
            call(C, k_percent)
    call(2, 10.0)
    torch.cuda.synchronize()
    assert sel.tolist() == [64, 6, 0, 64, 6]
    p, tt = _inputs(SEED, (2, 4, 4, 8), 3)
    with pytest.raises(ValueError):
        DiceTopKLoss(3)(p.to(dev).bfloat16(), tt.to(dev))


# ---- reproducibility and graph ------------------------------------------------------------------------------------------
def test_two_runs_bit_equal_and_one_graph_replays_other_contents(hip_device):
    """integer atomics only: two eager runs agree bit for bit.  ONE graph of forward + backward on static buffers, replayed
    on three inputs whose ignored fractions (0, 0.2, 0.6) give three different n and k: each replay equals the eager run on
    the same contents bit for bit, selection included -- a host-baked k or a histogram that is not re-zeroed would not."""
    from segmentation3d.loss.topk_loss import DiceTopKLoss
    C, shape = 3, (2, 16, 16, 16)
    opts = dict(weights=[1.0, 2.0, 3.0], ignore_label=255, k_percent=10.0)
    inputs = [_inputs(SEED + i, shape, C, ignore_frac=f) for i, f in enumerate((0.0, 0.2, 0.6))]
    eager = [_gpu(hip_device, p, t, C, **opts) for p, t in inputs]
    again = _gpu(hip_device, inputs[1][0], inputs[1][1], C, **opts)
    assert torch.equal(eager[1]['terms'], again['terms']) and torch.equal(eager[1]['grad'], again['grad'])
    assert eager[1]['selection'] == again['selection']
    assert len({e['selection'][1] for e in eager}) == 3

    loss_fn = DiceTopKLoss(C, **opts)
    pg = inputs[0][0].to(hip_device).requires_grad_(True)
    tg = inputs[0][1].to(hip_device)

    def step():
        pg.grad = None
        loss = loss_fn(pg, tg)
        loss.backward()
        return loss

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):          # warm-up on the side stream, as torch.cuda.graph expects
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    terms, sel, thr, grad = loss_fn.last_terms, loss_fn.last_selection, loss_fn.last_threshold, pg.grad
    for (p, t), ref in zip(inputs, eager):
        with torch.no_grad():
            pg.copy_(p.to(hip_device))
            tg.copy_(t.to(hip_device))
        graph.replay()
        torch.cuda.synchronize()
        assert tuple(int(v) for v in sel.cpu()) == ref['selection']
        assert torch.equal(terms.cpu(), ref['terms']) and torch.equal(grad.cpu(), ref['grad'])
        assert float(thr) == float(ref['tau']) and float(loss) == float(ref['loss'])
    del graph
    torch.cuda.synchronize()


# ---- training -----------------------------------------------------------------------------------------------------------
def _train_batch(dev):
    t = detgen.labels(700, 'cl/t', (2, 1, 32, 32, 32), 2).astype(np.float32)
    x = (t * 2.0 - 1.0 + 0.3 * detgen.normal(701, 'cl/x', (2, 1, 32, 32, 32))).astype(np.float32)
    return torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)


@pytest.mark.parametrize('use_graph', [False, True], ids=['eager', 'graph'])
def test_train_step_with_dicetopk(hip_device, use_graph):
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import TrainStep
    from segmentation3d.loss.topk_loss import DiceTopKLoss
    x, t = _train_batch(hip_device)
    step = TrainStep('vnet', 1, 2, loss_name='DiceTopK', loss_options={'topk_percent': 10.0}, lr=1e-3, device=hip_device,
                     seed=3, use_graph=use_graph)
    assert isinstance(step.loss_func, DiceTopKLoss) and step.loss_func.k_percent == 10.0
    losses = []
    for _ in range(6):
        loss = step(x, t)
        terms = step.loss_func.last_terms
        losses.append(float(loss))
        assert float(terms[0]) == float(loss)
        assert int(step.loss_func.last_selection[1]) == (2 * 32 ** 3) // 10
    _ops.PACK_CACHE.clear()
    report('topk_train_{}'.format('graph' if use_graph else 'eager'), **{'loss_{}'.format(i): v for i, v in enumerate(losses)})
    assert step.use_graph == use_graph and (step._graph is not None) == use_graph
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_train_step_with_deep_supervision_is_reproducible(hip_device):
    """one loss object is called once per level before any backward runs: nothing may be cached on the module"""
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import TrainStep
    x, t = _train_batch(hip_device)
    runs = []
    for _ in range(2):
        step = TrainStep('vnet', 1, 2, loss_name='DiceTopK', loss_options={'topk_percent': 10.0}, lr=1e-3,
                         device=hip_device, seed=3, deep_supervision=2)
        losses = []
        for _ in range(6):
            losses.append(float(step(x, t)))
            assert torch.isfinite(step.loss_func.last_levels).all()
        _ops.PACK_CACHE.clear()
        runs.append(losses)
    assert all(np.isfinite(runs[0])) and runs[0] == runs[1], runs


def test_train_engine_end_to_end_with_dicetopk_and_validation(hip_device, tmp_path):
    """core/seg_train.train() from a config file with loss.name = 'DiceTopK', loss.topk_percent = 20 and a `validation`
    section: the train step's loss and the validator's second loss object both come from build_loss(**loss_options)"""
    from segmentation3d.core.seg_train import train
    from segmentation3d.loss.topk_loss import DiceTopKLoss
    from segmentation3d.utils.image3d import Image3d
    from segmentation3d.utils.mha_io import write_mha
    frame = ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), tuple(np.eye(3).ravel()))
    lists = {}
    for name, first in (('train', 0), ('val', 2)):
        paths = []
        for k in range(first, first + 2):
            os.makedirs(str(tmp_path / 'c{}'.format(k)), exist_ok=True)
            lab = detgen.labels(800 + k, 'tke2e/seg{}'.format(k), (48, 48, 48), 2)
            img = (lab.astype(np.float32) * 2.0 - 1.0 + 0.3 * detgen.normal(810 + k, 'tke2e/n{}'.format(k), (48, 48, 48))).astype(np.float32)
            ip, sp = str(tmp_path / 'c{}'.format(k) / 'org.mha'), str(tmp_path / 'c{}'.format(k) / 'seg.mha')
            write_mha(Image3d(img, *frame), ip)
            write_mha(Image3d(lab.astype(np.int8), *frame), sp)
            paths += [ip, sp]
        (tmp_path / (name + '.txt')).write_text('2\n' + '\n'.join(paths) + '\n')
        lists[name] = str(tmp_path / (name + '.txt'))
    cfg = tmp_path / 'cfg.py'
    cfg.write_text('''
from easydict import EasyDict as edict
from segmentation3d.utils.normalizer import AdaptiveNormalizer
__C = edict()
cfg = __C
__C.general = {}
__C.general.imseg_list = '%s'
__C.general.save_dir = '%s'
__C.general.model_scale = 'coarse'
__C.general.resume_epoch = -1
__C.general.num_gpus = 1
__C.general.seed = 0
__C.dataset = {}
__C.dataset.num_classes = 2
__C.dataset.spacing = [1.0, 1.0, 1.0]
__C.dataset.crop_size = [32, 32, 32]
__C.dataset.sampling_method = 'GLOBAL'
__C.dataset.random_translation = [2, 2, 2]
__C.dataset.random_scale = [0.95, 1.05]
__C.dataset.interpolation = 'LINEAR'
__C.dataset.crop_normalizers = [AdaptiveNormalizer()]
__C.loss = {}
__C.loss.name = 'DiceTopK'
__C.loss.obj_weight = [1.0, 1.0]
__C.loss.focal_gamma = 2
__C.loss.topk_percent = 20
__C.net = {}
__C.net.name = 'vnet'
__C.train = {}
__C.train.epochs = 4
__C.train.batchsize = 2
__C.train.num_threads = 0
__C.train.lr = 1e-3
__C.train.betas = (0.9, 0.999)
__C.train.save_epochs = 2
__C.validation = {}
__C.validation.imseg_list = '%s'
__C.validation.crops_per_case = 2
__C.validation.ema = 0.5
''' % (lists['train'], str(tmp_path / 'model'), lists['val']))
    from segmentation3d import _ops
    try:
        step = train(str(cfg))
    finally:
        _ops.set_activation_dtype('fp32')
    assert isinstance(step.loss_func, DiceTopKLoss) and step.loss_func.k_percent == 20.0
    log = (tmp_path / 'model' / 'coarse' / 'train_log.txt').read_text().strip().splitlines()
    losses = [float(l.split('train_loss: ')[1].split(',')[0]) for l in log if 'train_loss' in l]
    val = [float(l.split('val_loss: ')[1].split(',')[0]) for l in log if 'val_loss' in l]
    report('topk_train_e2e', **{'loss_{}'.format(i): v for i, v in enumerate(losses)})
    assert len(losses) == 4 and all(np.isfinite(losses)), losses
    assert len(val) >= 1 and all(np.isfinite(val)), val
