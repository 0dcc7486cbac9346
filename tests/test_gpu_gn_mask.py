"""ReLU mask of a residual unit (out = relu(x_in + GN(conv(..))), residual_block3.py:24,46): the forward apply writes
[out > 0] as one byte per channel quad and GroupNorm backward reads that byte instead of the saved forward output.  The mask
holds exactly the comparison the kernels make on the stored `out`, so every result must equal the old path bit for bit."""
import pytest
import torch

from oracle import detgen

pytestmark = pytest.mark.gpu

DIMS = [(6, 6, 6), (12, 12, 12), (24, 24, 24), (5, 7, 9)]


def _t(seed, name, shape, std=1.0):
    return torch.from_numpy(detgen.normal(seed, name, shape, std=std))


def _packed_mask(out):
    """[N,D,H,W,C] forward output -> the specified mask: byte q of a voxel has bit k set iff out[..., 4 q + k] > 0"""
    N, D, H, W, C = out.shape
    bits = (out > 0).reshape(N, D, H, W, C // 4, 4).to(torch.int32)
    weights = torch.tensor([1, 2, 4, 8], dtype=torch.int32, device=out.device)
    return (bits * weights).sum(-1).to(torch.uint8)


@pytest.mark.parametrize('sliced', [False, True], ids=['dout_contiguous', 'dout_slice'])
@pytest.mark.parametrize('dims', DIMS, ids=lambda d: 'x'.join(map(str, d)))
@pytest.mark.parametrize('N', [1, 4])
@pytest.mark.parametrize('C', [16, 32, 64, 128, 256])
def test_gn_mask_entries_equal_saved_output_entries(hip_device, C, N, dims, sliced):
    from segmentation3d import _engine as E, _ops
    D, H, W = dims
    S = D * H * W
    y = _t(301, 'my', (N, D, H, W, C)).to(hip_device)
    res = _t(302, 'mr', (N, D, H, W, C)).to(hip_device)
    gamma = (1.0 + 0.5 * _t(303, 'mg', (C,))).to(hip_device)
    beta = (0.3 * _t(304, 'mb', (C,))).to(hip_device)
    mean_rstd = _ops.gn_stats(y)
    assert E.query('seg3d_gn_mask_supported', C) == 1

    # forward: same `out`, and the mask is [out > 0] packed as specified
    out_ref = _ops.gn_apply(y, mean_rstd, gamma, beta, res, True)
    mask = torch.full((N, D, H, W, C // 4), 0xFF, dtype=torch.uint8, device=hip_device)
    out = _ops.gn_apply(y, mean_rstd, gamma, beta, res, True, mask=mask)
    assert torch.equal(out, out_ref)
    assert torch.equal(mask, _packed_mask(out_ref))
    frac = float((out_ref > 0).float().mean())
    assert 0.2 < frac < 0.8, frac            # (the inputs exercise both branches of the select)

    if sliced:
        wide = _t(305, 'md', (N, D, H, W, C + 8)).to(hip_device)
        dout = wide[..., 4:4 + C]
        assert not dout.is_contiguous()
    else:
        dout = _t(305, 'md', (N, D, H, W, C)).to(hip_device)
    ldd = _ops._row_stride(dout, C)
    assert (ldd > C) == sliced

    # backward reduce: the partial sums
    nblk = E.query('seg3d_gn_bwd_blocks', S)
    part_ref = torch.full((N, nblk, C, 3), float('nan'), device=hip_device)
    part = torch.full((N, nblk, C, 3), float('nan'), device=hip_device)
    E.call('seg3d_gn_bwd_reduce', E.ptr(dout), E.ptr(out_ref), E.ptr(y), E.ptr(mean_rstd), E.ptr(gamma), E.ptr(beta),
           E.ptr(part_ref), N, S, C, 1, ldd, E.stream_ptr())
    E.call('seg3d_gn_bwd_reduce_mask', E.ptr(dout), E.ptr(mask), E.ptr(y), E.ptr(mean_rstd), E.ptr(part), N, S, C, ldd,
           E.stream_ptr())
    assert torch.isfinite(part_ref).all()
    assert torch.equal(part, part_ref)

    # backward apply: dy and the masked identity-path gradient
    abx, s12 = torch.empty((N, C, 3), device=hip_device), torch.empty((N, 2), device=hip_device)
    dgamma, dbeta = torch.empty(C, device=hip_device), torch.empty(C, device=hip_device)
    E.call('seg3d_gn_bwd_finalize', E.ptr(part_ref), E.ptr(gamma), E.ptr(mean_rstd), E.ptr(abx), E.ptr(s12), E.ptr(dgamma),
           E.ptr(dbeta), None, N, S, C, 0, E.stream_ptr())
    dy_ref, dres_ref = torch.full_like(y, float('nan')), torch.full_like(y, float('nan'))
    dy, dres, dy_only = torch.full_like(y, float('nan')), torch.full_like(y, float('nan')), torch.full_like(y, float('nan'))
    E.call('seg3d_gn_bwd_apply', E.ptr(dout), E.ptr(out_ref), E.ptr(y), E.ptr(mean_rstd), E.ptr(s12), E.ptr(gamma),
           E.ptr(beta), E.ptr(dy_ref), E.ptr(dres_ref), N, S, C, 1, ldd, E.stream_ptr())
    E.call('seg3d_gn_bwd_apply_mask', E.ptr(dout), E.ptr(mask), E.ptr(y), E.ptr(mean_rstd), E.ptr(s12), E.ptr(gamma),
           E.ptr(dy), E.ptr(dres), N, S, C, ldd, E.stream_ptr())
    E.call('seg3d_gn_bwd_apply_mask', E.ptr(dout), E.ptr(mask), E.ptr(y), E.ptr(mean_rstd), E.ptr(s12), E.ptr(gamma),
           E.ptr(dy_only), None, N, S, C, ldd, E.stream_ptr())
    assert torch.isfinite(dy_ref).all()
    assert torch.equal(dy, dy_ref) and torch.equal(dy_only, dy_ref)
    assert torch.equal(dres, dres_ref)
    assert torch.equal(dres, torch.where(out_ref > 0, dout, torch.zeros_like(dout)))

    # the operator-level call: all five results
    ref = _ops.gn_backward(dout, out_ref, y, mean_rstd, gamma, beta, True, want_dres=True)
    new = _ops.gn_backward(dout, None, y, mean_rstd, gamma, beta, True, want_dres=True, mask=mask)
    for a, b in zip(new, ref):
        assert torch.equal(a, b)


def test_gn_mask_entries_refuse_what_they_cannot_serve(hip_device):
    from segmentation3d import _engine as E
    assert E.query('seg3d_gn_mask_supported', 6) == 0 and E.query('seg3d_gn_mask_supported', 48) == 0
    y = torch.zeros((1, 2, 2, 2, 48), device=hip_device)
    mr = torch.zeros((1, 2), device=hip_device)
    g = torch.ones(48, device=hip_device)
    m = torch.zeros((1, 2, 2, 2, 12), dtype=torch.uint8, device=hip_device)
    with pytest.raises(ValueError):
        E.call('seg3d_gn_apply_mask', E.ptr(y), E.ptr(mr), E.ptr(g), E.ptr(g), None, E.ptr(y), E.ptr(m), 1, 8, 48, 1, 0,
               E.stream_ptr())
    with pytest.raises(ValueError):
        E.call('seg3d_gn_apply_mask', E.ptr(y), E.ptr(mr), E.ptr(g), E.ptr(g), None, E.ptr(y), None, 1, 8, 32, 1, 0,
               E.stream_ptr())


def _block_grads(hip_device, C, dims, N, two_units):
    """forward + backward of a residual block built from fused units (one unit with residual = its own input, or two units
    joined by a ResidualLink); returns the output and every gradient"""
    from segmentation3d import _ops
    D, H, W = dims
    xin = _ops.from_ndhwc(_t(311, 'bx', (N, D, H, W, C)).to(hip_device)).requires_grad_(True)   # NDHWC memory, as between units
    params = []
    for u in range(2 if two_units else 1):
        w = _t(312 + 10 * u, 'bw', (C, C, 3, 3, 3), 0.05).to(hip_device).requires_grad_(True)
        b = _t(313 + 10 * u, 'bb', (C,), 0.1).to(hip_device).requires_grad_(True)
        g = (1.0 + 0.5 * _t(314 + 10 * u, 'bg', (C,))).to(hip_device).requires_grad_(True)
        be = (0.3 * _t(315 + 10 * u, 'be', (C,))).to(hip_device).requires_grad_(True)
        params += [w, b, g, be]
    if two_units:
        link = _ops.ResidualLink()
        h = _ops.conv_gn_act(xin, *params[:4], kind='k3', relu=True, link_in=link)
        out = _ops.conv_gn_act(h, *params[4:], residual=xin, kind='k3', relu=True, link_out=link)
    else:
        out = _ops.conv_gn_act(xin, *params, residual=xin, kind='k3', relu=True)
    dout = _t(316, 'bd', tuple(out.shape)).to(hip_device)
    grads = torch.autograd.grad(out, [xin] + params, _ops.from_ndhwc(_ops.to_ndhwc(dout)))
    torch.cuda.synchronize()
    return [out.detach()] + [t.detach() for t in grads]


@pytest.mark.parametrize('force_direct', [False, True], ids=['mfma', 'force_direct'])
@pytest.mark.parametrize('two_units', [False, True], ids=['res_is_x', 'linked'])
@pytest.mark.parametrize('C,dims,N', [(32, (8, 8, 8), 2), (16, (6, 10, 12), 1), (64, (12, 12, 12), 1)])
def test_residual_block_backward_is_unchanged_by_the_mask(hip_device, monkeypatch, C, dims, N, two_units, force_direct):
    """the whole unit: output and every gradient (dx with the identity-path gradient folded into the data-gradient kernel, or
    added behind the direct kernels) equal the saved-output path bit for bit"""
    from segmentation3d import _engine as E, _ops
    monkeypatch.setattr(_ops, 'FORCE_DIRECT', force_direct)
    monkeypatch.setattr(_ops, 'WGRAD_SIDE_STREAM', False)
    calls = []
    real_call = E.call
    monkeypatch.setattr(E, 'call', lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(_ops, 'RELU_MASK', False)
    ref = _block_grads(hip_device, C, dims, N, two_units)
    assert 'seg3d_gn_apply_mask' not in calls and 'seg3d_gn_bwd_reduce_mask' not in calls
    del calls[:]
    monkeypatch.setattr(_ops, 'RELU_MASK', True)
    new = _block_grads(hip_device, C, dims, N, two_units)
    assert calls.count('seg3d_gn_apply_mask') == 1 and calls.count('seg3d_gn_bwd_reduce_mask') == 1 and \
        calls.count('seg3d_gn_bwd_apply_mask') == 1
    assert len(ref) == len(new)
    for a, b in zip(new, ref):
        assert torch.isfinite(b).all()
        assert torch.equal(a, b)


def test_no_mask_without_a_backward_pass(hip_device, monkeypatch):
    """inference / no_grad take the existing apply entry and write nothing extra; bf16 mode stays on the saved-output path"""
    from segmentation3d import _engine as E, _ops
    C = 32
    x = _ops.from_ndhwc(_t(321, 'nx', (1, 8, 8, 8, C)).to(hip_device))
    w = _t(322, 'nw', (C, C, 3, 3, 3), 0.05).to(hip_device).requires_grad_(True)
    b, g, be = (_t(323 + k, 'np', (C,), 0.1).to(hip_device).requires_grad_(True) for k in range(3))
    calls = []
    real_call = E.call
    monkeypatch.setattr(E, 'call', lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    with torch.no_grad():
        out0 = _ops.conv_gn_act(x, w, b, g, be, residual=x, kind='k3', relu=True)
    assert 'seg3d_gn_apply_mask' not in calls and 'seg3d_gn_apply' in calls
    del calls[:]
    out1 = _ops.conv_gn_act(x, w, b, g, be, residual=x, kind='k3', relu=True)
    assert 'seg3d_gn_apply_mask' in calls
    assert torch.equal(out0, out1.detach())
    del calls[:]
    _ops.conv_gn_act(x, w, b, g, be, residual=x, kind='k3', relu=False)      # no ReLU: nothing to mask
    _ops.conv_gn_act(x, w, b, g, be, kind='k3', relu=True)                   # no residual: recomputed from y
    assert 'seg3d_gn_apply_mask' not in calls
    with _ops.activation_dtype('bf16'):
        assert not _ops.relu_mask_usable(C)


def test_train_step_is_unchanged_by_the_mask(hip_device, monkeypatch):
    """one V-Net train step (forward, Dice loss, backward): loss and every parameter gradient bit for bit"""
    from segmentation3d import _ops
    from segmentation3d.network import vnet
    from segmentation3d.loss.multi_dice_loss import MultiDiceLoss
    net = vnet.SegmentationNet(1, 2)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = detgen.state_dict_like(shapes, 331)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to(hip_device)
    x = torch.from_numpy(detgen.normal(332, 'ts/x', (2, 1, 32, 32, 32))).to(hip_device)
    t = torch.from_numpy(detgen.labels(333, 'ts/t', (2, 1, 32, 32, 32), 2)).to(hip_device)
    loss_fn = MultiDiceLoss([1.0, 1.0], 2, use_gpu=True)
    monkeypatch.setattr(_ops, 'WGRAD_SIDE_STREAM', False)
    results = []
    for use_mask in (False, True):
        monkeypatch.setattr(_ops, 'RELU_MASK', use_mask)
        net.zero_grad(set_to_none=True)
        loss = loss_fn(net(x), t)
        loss.backward()
        torch.cuda.synchronize()
        results.append([loss.detach().clone()] + [p.grad.detach().clone() for p in net.parameters()])
    for a, b in zip(*results):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)
