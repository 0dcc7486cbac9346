"""Deep supervision on the GPU: the label pyramid, the fused head kernels (seg3d_ds_head_fwd / _bwd / _bwd_finalize) through
`_ops` against float64, the whole deeply supervised network and its loss against the float64 oracle, the train step (eager,
hipGraph) and the checkpoint round trip.

Bars are the project's parity bars (tests/test_gpu_compound_loss.py): O(1) outputs and losses within 1e-4 of the float64
oracle, gradients with gpu_util.rel_err < 1e-4, copies and repeat runs bit-exact.  One looser bar is taken over from an existing
test: the stem's weight gradient (`in_block.conv.weight`, the deepest parameter of the encoder) through the whole fp32 network
is held to 1e-4 under the smooth DiceCE loss like every other gradient here, and to 1e-3 under the reference's Dice: that
loss gates every probability with [p > 1/C], a voxel whose gate falls the other way than in float64 moves the gradient by
about 1 / 65536 = 1.5e-5 of its size on the 2 x 32^3 input, and the bar leaves room for some sixty of them
(tests/test_gpu_parity.py::test_network_matches_reference allows the same gradient 2e-2 for that reason)."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO  # noqa: F401
from gpu_util import max_err, rel_err, report
from oracle import detgen, torch_ref
from test_compound_loss import oracle as dicece_oracle

pytestmark = pytest.mark.gpu

HEADS = (('ds_out_64', 'up_64'), ('ds_out_128', 'up_128'), ('ds_out_256', 'up_256'))
STEM_BAR = {'DiceCE': 1e-4, 'Dice': 1e-3}     # see the module docstring


# ---- 1. label pyramid -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('levels', [1, 2, 3])
def test_label_pyramid_is_strided_copy(hip_device, levels):
    from segmentation3d import _ops
    g = torch.Generator().manual_seed(10 + levels)
    mask = torch.randint(0, 4, (2, 1, 8, 16, 24), generator=g).float()
    mask[torch.rand(mask.shape, generator=g) < 0.1] = 255.0
    mask[torch.rand(mask.shape, generator=g) < 0.1] = -1.0
    outs = _ops.label_pyramid(mask.to(hip_device), levels)
    assert len(outs) == levels
    for k, out in enumerate(outs, start=1):
        f = 2 ** k
        assert out.is_contiguous() and torch.equal(out.cpu(), mask[:, :, ::f, ::f, ::f])
    flat = _ops.label_pyramid(mask[:, 0].to(hip_device), levels)        # [N,D,H,W] is taken as well
    assert all(torch.equal(a, b) for a, b in zip(flat, outs))


def test_label_pyramid_refuses_indivisible_sizes(hip_device):
    from segmentation3d import _engine as E
    from segmentation3d import _ops
    with pytest.raises(ValueError):
        _ops.label_pyramid(torch.zeros(1, 1, 8, 12, 8, device=hip_device), 3)
    with pytest.raises(ValueError):
        _ops.label_pyramid(torch.zeros(1, 1, 8, 8, 8, device=hip_device), 4)
    m, o = torch.zeros(1, 6, 8, 8, device=hip_device), torch.zeros(512, device=hip_device)
    with pytest.raises(ValueError):                                       # the C entry itself refuses, too
        E.call('seg3d_label_pyramid', E.ptr(m), E.ptr(o), E.ptr(o), None, 1, 6, 8, 8, 2, E.stream_ptr())


# ---- 2. head kernels --------------------------------------------------------------------------------------------------
_HEAD_REF = {}


def _head_case(cin, C):
    """inputs and the float64 CPU reference of one head, computed once per (Cin, C) and shared"""
    key = (cin, C)
    if key not in _HEAD_REF:
        g = torch.Generator().manual_seed(1000 * cin + C)
        xn = torch.randn((2, 3, 5, 7, cin), generator=g)                  # NDHWC rows; 105 voxels per item
        w = torch.randn((C, cin, 1, 1, 1), generator=g) / float(np.sqrt(cin))
        b = 0.5 * torch.randn((C,), generator=g)
        r = torch.randn((2, C, 3, 5, 7), generator=g)                     # dprobs
        x64 = xn.permute(0, 4, 1, 2, 3).double().requires_grad_(True)
        w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
        p64 = F.softmax(F.conv3d(x64, w64, b64), dim=1)
        (p64 * r.double()).sum().backward()
        _HEAD_REF[key] = dict(xn=xn, w=w, b=b, r=r, p=p64.detach(), dx=x64.grad, dw=w64.grad, db=b64.grad)
    return _HEAD_REF[key]


def _run_head(dev, case, sliced):
    from segmentation3d import _ops
    cin = case['xn'].shape[-1]
    if sliced:      # the feature is the second half of a [.., 2 Cin] buffer: read in place with ldx = 2 Cin
        buf = torch.cat((torch.full_like(case['xn'], 7.0), case['xn']), dim=-1).to(dev).requires_grad_(True)
        x = buf[..., cin:].permute(0, 4, 1, 2, 3)
        assert not _ops.to_ndhwc(x, allow_slice=True).is_contiguous()
    else:
        buf = case['xn'].to(dev).requires_grad_(True)
        x = buf.permute(0, 4, 1, 2, 3)
    w = case['w'].to(dev).requires_grad_(True)
    b = case['b'].to(dev).requires_grad_(True)
    p = _ops.ds_head(x, w, b)
    (p * case['r'].to(dev)).sum().backward()
    torch.cuda.synchronize()
    gx = buf.grad.detach().cpu()
    if sliced:
        assert float(gx[..., :cin].abs().max()) == 0.0
        gx = gx[..., cin:]
    return p.detach().cpu(), gx.permute(0, 4, 1, 2, 3), w.grad.detach().cpu(), b.grad.detach().cpu()


@pytest.mark.parametrize('sliced', [False, True], ids=['packed', 'slice'])
@pytest.mark.parametrize('C', [2, 3, 5, 8])
@pytest.mark.parametrize('cin', [64, 128, 256])
def test_head_matches_float64(hip_device, cin, C, sliced):
    case = _head_case(cin, C)
    p, dx, dw, db = _run_head(hip_device, case, sliced)
    assert p.is_contiguous() and tuple(p.shape) == (2, C, 3, 5, 7)
    errs = dict(probs=max_err(p, case['p']), dx=rel_err(dx, case['dx']), dw=rel_err(dw, case['dw']), db=rel_err(db, case['db']))
    report('ds_head_{}_{}_{}'.format(cin, C, 'slice' if sliced else 'packed'), **errs)
    print('ds_head', cin, C, sliced, errs)
    assert errs['probs'] < 1e-4, errs
    assert errs['dx'] < 1e-4 and errs['dw'] < 1e-4 and errs['db'] < 1e-4, errs
    assert max_err(p.sum(1), torch.ones(2, 3, 5, 7)) < 1e-6


def test_head_grid_stride_loop(hip_device):
    """1 x 52^3 = 140608 voxels of 64 channels, C = 2: both kernels walk 16 groups x 8 voxels = 128 voxels a tile, 1099 tiles, the
    last one half full.  The forward grid holds up to 8 x 256 = 2048 workgroups, so it launches 1099 and NO workgroup takes a second
    tile; the backward grid is capped at 1024, so 75 workgroups walk two tiles and all 1024 slabs of the workspace are filled
    (tests/test_ds_head_cases.py derives these counts; the forward's second trip is taken in tests/test_gpu_ds_head_float64.py)"""
    from segmentation3d import _ops
    g = torch.Generator().manual_seed(5)
    xn = torch.randn((1, 52, 52, 52, 64), generator=g)
    w = torch.randn((2, 64, 1, 1, 1), generator=g) / 8.0
    b = torch.tensor([0.3, -0.2])
    r = torch.randn((1, 2, 52, 52, 52), generator=g)
    x64 = xn.permute(0, 4, 1, 2, 3).double().requires_grad_(True)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    p64 = F.softmax(F.conv3d(x64, w64, b64), dim=1)
    (p64 * r.double()).sum().backward()
    p, dx, dw, db = _run_head(hip_device, dict(xn=xn, w=w, b=b, r=r), False)
    errs = dict(probs=max_err(p, p64.detach()), dx=rel_err(dx, x64.grad), dw=rel_err(dw, w64.grad), db=rel_err(db, b64.grad))
    report('ds_head_grid_stride', **errs)
    print('ds_head_grid_stride', errs)
    assert errs['probs'] < 1e-4 and errs['dx'] < 1e-4 and errs['dw'] < 1e-4 and errs['db'] < 1e-4, errs


def test_head_zero_weights_give_uniform_probabilities(hip_device):
    from segmentation3d import _ops
    for C in (2, 3, 5, 8):
        x = torch.randn(2, 3, 5, 7, 64, device=hip_device).permute(0, 4, 1, 2, 3)
        p = _ops.ds_head(x, torch.zeros(C, 64, 1, 1, 1, device=hip_device), torch.zeros(C, device=hip_device))
        assert torch.equal(p.cpu(), torch.full((2, C, 3, 5, 7), 1.0, dtype=torch.float32) / C)
        p = _ops.ds_head(x, torch.zeros(C, 64, 1, 1, 1, device=hip_device), None)          # no bias: the same
        assert torch.equal(p.cpu(), torch.full((2, C, 3, 5, 7), 1.0, dtype=torch.float32) / C)


@pytest.mark.parametrize('cin,C', [(66, 2), (260, 2), (64, 9), (2, 2)])
def test_head_refuses_unsupported_sizes(hip_device, cin, C):
    from segmentation3d import _engine as E
    from segmentation3d import _ops
    assert not _ops.ds_head_supported(cin, C)
    x = torch.randn(1, 2, 2, 2, cin, device=hip_device).permute(0, 4, 1, 2, 3)
    w, b = torch.zeros(C, cin, 1, 1, 1, device=hip_device), torch.zeros(C, device=hip_device)
    with pytest.raises(ValueError):
        _ops.ds_head(x, w, b)
    p = torch.full((1, C, 2, 2, 2), -1.0, device=hip_device)
    with pytest.raises(NotImplementedError):                               # the C entry itself refuses, too ...
        E.call('seg3d_ds_head_fwd', E.ptr(x), 0, E.ptr(w), E.ptr(b), E.ptr(p), 1, 8, cin, C, E.stream_ptr())
    assert 'Cin' in E.last_error()
    torch.cuda.synchronize()
    assert float(p.max()) == -1.0                                          # ... and writes nothing


def test_head_gradients_are_reproducible_and_honour_sinks(hip_device):
    from segmentation3d import _grad_sink as G
    case = _head_case(128, 3)
    a = _run_head(hip_device, case, False)
    b = _run_head(hip_device, case, False)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    # sink mode: the finalize ADDS into the registered buffers and autograd gets nothing for those inputs
    from segmentation3d import _ops
    w = case['w'].to(hip_device).requires_grad_(True)
    bias = case['b'].to(hip_device).requires_grad_(True)
    fill_w, fill_b = torch.randn_like(case['w']), torch.randn_like(case['b'])
    sink_w, sink_b = fill_w.to(hip_device), fill_b.to(hip_device)
    G.register(w, sink_w)
    G.register(bias, sink_b)
    try:
        x = case['xn'].to(hip_device).permute(0, 4, 1, 2, 3)
        (_ops.ds_head(x, w, bias) * case['r'].to(hip_device)).sum().backward()
        torch.cuda.synchronize()
    finally:
        G.unregister([w, bias])
    assert w.grad is None and bias.grad is None
    assert torch.equal(sink_w.cpu(), fill_w + a[2]) and torch.equal(sink_b.cpu(), fill_b + a[3])


# ---- 3. / 4. whole net, loss and gradient ----------------------------------------------------------------------------------
def _oracle_deep(x, sd, plugin, levels):
    """oracle/torch_ref.segmentation_net restated with the decoder features kept, plus conv3d + softmax per head"""
    bott = torch_ref.VBNET_BOTTLENECK if plugin == 'vbnet' else ()
    feats = {'in_block': torch_ref.input_block(x, sd)}
    y = feats['in_block']
    for stage, _, convs in torch_ref.VNET_ENCODER:
        y = torch_ref.down_block(y, sd, stage, convs, stage in bott)
        feats[stage] = y
    decoded = {}
    for stage, _, _, convs, skip in torch_ref.VNET_DECODER:
        y = torch_ref.up_block(y, feats[skip], sd, stage, convs, stage in bott)
        decoded[stage] = y
    outs = [torch_ref.output_block(y, sd)]
    for name, stage in HEADS[:levels]:
        outs.append(F.softmax(F.conv3d(decoded[stage], sd[name + '.conv.weight'], sd[name + '.conv.bias']), dim=1))
    return outs


_NET_CASES = {}


def _net_case(plugin, ncls):
    """a deeply supervised net (3 levels), a 2 x 1 x 32^3 input, and the float64 oracle's outputs (graph kept): built once"""
    key = (plugin, ncls)
    if key not in _NET_CASES:
        import importlib
        mod = importlib.import_module('segmentation3d.network.' + plugin)
        torch.manual_seed(31)
        net = mod.SegmentationNet(1, ncls, deep_supervision=3)
        mod.parameters_kaiming_init(net)
        for name, _ in HEADS:                                            # biases are zero after the initialiser: move them
            getattr(net, name).conv.bias.data.normal_(0.0, 0.3)
        x = torch.from_numpy(detgen.normal(41, 'ds/x/' + plugin, (2, 1, 32, 32, 32)))
        t = torch.from_numpy(detgen.labels(42, 'ds/t/' + plugin, (2, 1, 32, 32, 32), ncls)).float()
        sd64 = {k: v.detach().double().requires_grad_(True) for k, v in net.state_dict().items()}
        outs64 = _oracle_deep(x.double(), sd64, plugin, 3)
        _NET_CASES[key] = dict(net=net, x=x, t=t, sd64=sd64, outs64=outs64, mod=mod)
    return _NET_CASES[key]


@pytest.mark.parametrize('plugin,ncls', [('vnet', 2), ('vbnet', 3)])
def test_forward_deep_matches_oracle(hip_device, plugin, ncls):
    from segmentation3d import _ops
    case = _net_case(plugin, ncls)
    net = case['net'].to(hip_device)
    x = case['x'].to(hip_device)
    try:
        outs = net.forward_deep(x)
        plain_out = net(x)
        with torch.no_grad():
            outs_ng = net.forward_deep(x)
            plain_ng = net(x)
        torch.cuda.synchronize()
        assert [tuple(o.shape) for o in outs] == [(2, ncls, 32, 32, 32), (2, ncls, 16, 16, 16), (2, ncls, 8, 8, 8),
                                                   (2, ncls, 4, 4, 4)]
        errs = {'p{}'.format(k): max_err(o, r.detach()) for k, (o, r) in enumerate(zip(outs, case['outs64']))}
        errs.update({'p{}_nograd'.format(k): max_err(o, r.detach()) for k, (o, r) in enumerate(zip(outs_ng, case['outs64']))})
        report('ds_forward_deep_' + plugin, **errs)
        print('ds_forward_deep', plugin, errs)
        assert all(v < 1e-4 for v in errs.values()), errs
        assert all(o.is_contiguous() for o in outs)
        # net(x) is the same computation as forward_deep(x)[0], with and without autograd
        assert torch.equal(plain_out, outs[0]) and torch.equal(plain_ng, outs_ng[0])
        # ... and the same as a network without the heads that holds the shared parameters
        plain = case['mod'].SegmentationNet(1, ncls)
        plain.load_state_dict({k: v for k, v in net.state_dict().items() if not k.startswith('ds_out_')})
        plain = plain.to(hip_device)
        assert torch.equal(plain(x), outs[0])
        with torch.no_grad():
            assert torch.equal(plain(x), outs_ng[0])
    finally:
        case['net'].cpu()
        _ops.PACK_CACHE.clear()


@pytest.mark.parametrize('loss_name', ['DiceCE', 'Dice'])
def test_loss_and_gradients_match_oracle(hip_device, loss_name):
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import build_loss
    from segmentation3d.loss.deep_supervision_loss import DeepSupervisionLoss
    case = _net_case('vnet', 2)
    net = case['net'].to(hip_device)
    weights = [8 / 15, 4 / 15, 2 / 15, 1 / 15]
    try:
        loss_fn = DeepSupervisionLoss(build_loss(loss_name, 2, [0.5, 0.5] if loss_name == 'Dice' else None), 3)
        assert loss_fn.weights == pytest.approx(weights)
        net.zero_grad()
        loss = loss_fn(net.forward_deep(case['x'].to(hip_device)), case['t'].to(hip_device))
        loss.backward()
        torch.cuda.synchronize()
        levels = loss_fn.last_levels.cpu()
        grads = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
        # float64 oracle: the same base loss on the oracle's probabilities and the strided label maps
        ref_levels = []
        for k, p64 in enumerate(case['outs64']):
            f = 2 ** k
            tk = case['t'][:, :, ::f, ::f, ::f]
            if loss_name == 'DiceCE':
                ref_levels.append(dicece_oracle(p64, tk)[0])
            else:
                ref_levels.append(torch_ref.multi_dice_loss(p64, tk, [0.5, 0.5]))
        ref_loss = sum(w * l for w, l in zip(weights, ref_levels))
        names = [k for k in case['sd64'] if k.startswith('ds_out_')] + ['in_block.conv.weight']
        ref_grads = dict(zip(names, torch.autograd.grad(ref_loss, [case['sd64'][k] for k in names], retain_graph=True)))
        errs = {'loss': abs(float(loss) - float(ref_loss)),
                'levels': max(abs(float(a) - float(b)) for a, b in zip(levels, ref_levels))}
        errs.update({'g_' + k: rel_err(grads[k], ref_grads[k]) for k in names})
        report('ds_loss_' + loss_name, **errs)
        print('ds_loss', loss_name, errs)
        assert levels.shape == (4,) and errs['loss'] < 1e-4 and errs['levels'] < 1e-4, errs
        assert len(names) == 7
        for k in names:
            assert errs['g_' + k] < (STEM_BAR[loss_name] if k == 'in_block.conv.weight' else 1e-4), (k, errs)
        if loss_name == 'DiceCE':
            assert torch.equal(loss_fn.last_terms, loss_fn.base_loss.last_terms) and loss_fn.last_terms.shape == (3,)
            assert abs(float(loss_fn.last_terms[0]) - float(ref_levels[0])) < 1e-4
    finally:
        case['net'].cpu()
        _ops.PACK_CACHE.clear()


def test_ignored_block_contributes_nothing_at_any_level(hip_device):
    from segmentation3d.loss.compound_loss import DiceCELoss
    from segmentation3d.loss.deep_supervision_loss import DeepSupervisionLoss
    g = torch.Generator().manual_seed(77)
    t = torch.randint(0, 2, (2, 1, 32, 32, 32), generator=g).float()
    t[:, :, 8:24, 4:20, 16:32] = 255.0
    probs = [torch.softmax(2.0 * torch.randn((2, 2, 32 >> k, 32 >> k, 32 >> k), generator=g), dim=1) for k in range(4)]
    loss_fn = DeepSupervisionLoss(DiceCELoss(2, ignore_label=255), 3)

    def run(ps):
        leaves = [p.to(hip_device).requires_grad_(True) for p in ps]
        loss = loss_fn(leaves, t.to(hip_device))
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().cpu(), loss_fn.last_levels.cpu(), [p.grad.cpu() for p in leaves]

    loss, levels, grads = run(probs)
    ref_levels = [dicece_oracle(p.double(), t[:, :, ::2 ** k, ::2 ** k, ::2 ** k], ignore_label=255)[0] for k, p in enumerate(probs)]
    ref = sum(w * l for w, l in zip(loss_fn.weights, ref_levels))
    assert abs(float(loss) - float(ref)) < 1e-4
    assert max(abs(float(a) - float(b)) for a, b in zip(levels, ref_levels)) < 1e-4
    swapped = []
    for k, (p, gr) in enumerate(zip(probs, grads)):
        f = 2 ** k
        dead = (t[:, :, ::f, ::f, ::f] == 255.0).expand(-1, 2, -1, -1, -1)
        assert bool(dead.any()) and float(gr[dead].abs().max()) == 0.0          # zero dprobs there at every level
        assert float(gr[~dead].abs().max()) > 0.0
        swapped.append(torch.where(dead, p.flip(1), p))                         # other probabilities on the ignored voxels ...
    loss2, levels2, _ = run(swapped)
    assert torch.equal(loss2, loss) and torch.equal(levels2, levels)            # ... change no bit of any level's loss


# ---- 5. TrainStep --------------------------------------------------------------------------------------------------------
def _train_data(dev):
    t = detgen.labels(700, 'ds/train/t', (2, 1, 32, 32, 32), 2).astype(np.float32)
    x = (t * 2.0 - 1.0 + 0.3 * detgen.normal(701, 'ds/train/x', (2, 1, 32, 32, 32))).astype(np.float32)
    return torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)


def test_train_step_eager_and_graph(hip_device):
    """three steps from the same seed, eager and with the whole step captured in a hipGraph (two eager warm-up steps, then
    the capture and its replay).  tests/test_gpu_compound_loss.py asks of its eager / graph pair that every loss is finite
    and that the graph run really captured; the two runs compute the same arithmetic in the same order, so their O(1) losses
    are also held to the 1e-4 parity bar against each other."""
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import TrainStep
    from segmentation3d.loss.deep_supervision_loss import DeepSupervisionLoss
    x, t = _train_data(hip_device)
    runs = {}
    try:
        for use_graph in (False, True):
            step = TrainStep('vnet', 1, 2, loss_name='DiceCE', lr=1e-3, device=hip_device, seed=3, use_graph=use_graph,
                             deep_supervision=3)
            assert isinstance(step.loss_func, DeepSupervisionLoss) and step.net.deep_supervision == 3
            before = {k: p.detach().clone() for k, p in step.net.named_parameters() if k.startswith('ds_out_')}
            losses = [float(step(x, t)) for _ in range(3)]
            torch.cuda.synchronize()
            assert step.use_graph == use_graph and (step._graph is not None) == use_graph
            assert len(before) == 6
            for k, p in step.net.named_parameters():
                if k in before:
                    assert not torch.equal(p.detach(), before[k]), k
            assert bool(torch.isfinite(step.loss_func.last_levels).all()) and step.loss_func.last_levels.shape == (4,)
            runs[use_graph] = losses
            _ops.PACK_CACHE.clear()
    finally:
        _ops.PACK_CACHE.clear()
    report('ds_train_step', **{'{}_{}'.format('graph' if g else 'eager', i): v for g, ls in runs.items() for i, v in enumerate(ls)})
    print('ds_train_step', runs)
    assert all(np.isfinite(runs[False])) and all(np.isfinite(runs[True])), runs
    assert max(abs(a - b) for a, b in zip(runs[False], runs[True])) < 1e-4, runs


def test_train_step_without_deep_supervision_is_unchanged(hip_device):
    from segmentation3d import _ops
    from segmentation3d.core.seg_train import TrainStep
    x, t = _train_data(hip_device)
    flats = []
    try:
        for kw in ({}, {'deep_supervision': 0}):
            step = TrainStep('vnet', 1, 2, loss_name='DiceCE', lr=1e-3, device=hip_device, seed=3, **kw)
            for _ in range(2):
                step(x, t)
            torch.cuda.synchronize()
            assert len(step.opt._flat) >= 1 and not any(k.startswith('ds_out_') for k, _ in step.net.named_parameters())
            flats.append([f['params'].detach().cpu().clone() for f in step.opt._flat if f is not None])
            _ops.PACK_CACHE.clear()
    finally:
        _ops.PACK_CACHE.clear()
    assert len(flats[0]) == len(flats[1]) and all(torch.equal(a, b) for a, b in zip(*flats))


# ---- 6. checkpoint -------------------------------------------------------------------------------------------------------
def test_deeply_supervised_checkpoint_runs_through_the_inference_loader(hip_device, tmp_path):
    from segmentation3d import _ops
    from segmentation3d.core.seg_infer import load_single_model
    from segmentation3d.core.seg_train import TrainStep
    from segmentation3d.utils.model_io import load_checkpoint, save_checkpoint
    x, t = _train_data(hip_device)
    cfg = types.SimpleNamespace(
        general=types.SimpleNamespace(save_dir=str(tmp_path), model_scale='fine'), net=types.SimpleNamespace(name='vnet'),
        dataset=types.SimpleNamespace(spacing=[1.0, 1.0, 1.0], interpolation='LINEAR', num_classes=2, crop_normalizers=[None]))
    try:
        step = TrainStep('vnet', 1, 2, loss_name='DiceCE', lr=1e-3, device=hip_device, seed=5, deep_supervision=3)
        step(x, t)
        save_checkpoint(step.net, step.opt, 1, 1, cfg, step.max_stride, 1)
        with torch.no_grad():
            want = step.net(x)
        model = load_single_model(str(tmp_path / 'fine'), 0)
        assert not any(k.startswith('ds_out_') for k in model.net.state_dict())
        with torch.no_grad():
            got = model.net(x)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
        # a training resume with the same deep_supervision takes the heads back; another level count is refused
        again = TrainStep('vnet', 1, 2, loss_name='DiceCE', lr=1e-3, device=hip_device, seed=6, deep_supervision=3)
        assert load_checkpoint(1, again.net, again.opt, str(tmp_path / 'fine')) == (1, 1)
        for (k, a), (_, b) in zip(again.net.state_dict().items(), step.net.state_dict().items()):
            assert torch.equal(a, b), k
        for levels in (2, 0):
            other = TrainStep('vnet', 1, 2, loss_name='DiceCE', lr=1e-3, device=hip_device, seed=6, deep_supervision=levels)
            with pytest.raises(ValueError, match='deep_supervision = 3'):
                load_checkpoint(1, other.net, other.opt, str(tmp_path / 'fine'))
        assert load_checkpoint(1, other.net, None, str(tmp_path / 'fine')) == (1, 1)      # network alone, heads dropped
        _ops.PACK_CACHE.invalidate()
        with torch.no_grad():
            assert torch.equal(other.net(x), want)
    finally:
        _ops.PACK_CACHE.clear()
