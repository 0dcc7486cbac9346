"""GPU tests of the MFMA weight packers (csrc/layout.hip) against tests/pack_oracle.py, bit for bit: the per-tensor entry
points seg3d_pack_weights_mfma[_bf16] and the multi-job launch of PackedWeightCache.repack_all().  The oracle is an independent
statement of the images (tests/test_pack_oracle.py checks it on the CPU), so equality with it on both sides of a change to the
packers shows that the images did not change."""
import pytest
import torch

import pack_oracle as PO
from oracle import detgen

pytestmark = pytest.mark.gpu


def _t(seed, name, shape, std=1.0):
    return torch.from_numpy(detgen.normal(seed, name, shape, std=std))


def _bits(t):
    return t.cpu().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _pack_one(w_dev, A, B, T, sa, sb, flip, bf16):
    """the per-tensor entry point's image, written into a NaN-filled buffer of the queried size"""
    from segmentation3d import _engine as E
    n = E.query('seg3d_packed_mfma_bf16_elems' if bf16 else 'seg3d_packed_mfma_floats', A, B, T)
    wp = torch.full((n,), float('nan'), dtype=torch.bfloat16 if bf16 else torch.float32, device=w_dev.device)
    E.call('seg3d_pack_weights_mfma_bf16' if bf16 else 'seg3d_pack_weights_mfma', E.ptr(w_dev), E.ptr(wp), A, B, T, sa, sb,
           flip, E.stream_ptr())
    return wp


def _oracle(w, A, B, T, sa, sb, flip, bf16=False):
    return PO.packed_image(w.numpy(), A, B, T, sa, sb, flip, bf16=bf16)


# (A, B): smaller than one chunk; exactly one fp32 / one bf16 chunk; a partial last block on both sides, two blocks each way;
# the shape of the multi-pack test
SHAPES = [(4, 8), (8, 32), (16, 32), (12, 40), (40, 72)]
FORMAT_T = [(False, 1), (False, 8), (False, 27), (False, 36), (False, 48), (True, 8), (True, 27)]


@pytest.mark.parametrize('AB_', SHAPES)
@pytest.mark.parametrize('bf16,T', FORMAT_T)
def test_single_pack_equals_oracle(hip_device, bf16, T, AB_):
    """both weight orientations (w[b][a][t] and w[a][b][t]: one of the channel strides equals the source tap count), with and
    without flipped taps where the source has 27"""
    A, B = AB_
    Ts = 27 if T in (36, 48) else T
    w = _t(300 + T, 'pack1_{}_{}'.format(A, B), (A * B * Ts,), std=0.1)
    wd = w.to(hip_device)
    for (sa, sb) in ((Ts, A * Ts), (B * Ts, Ts)):
        for flip in ((0, 1) if Ts == 27 else (0,)):
            got = _pack_one(wd, A, B, T, sa, sb, flip, bf16)
            assert torch.equal(_bits(got), _bits(_oracle(w, A, B, T, sa, sb, flip, bf16))), (sa, sb, flip)


@pytest.mark.parametrize('bf16,T', [(False, 8), (False, 27), (False, 36), (True, 8), (True, 27)])
def test_single_pack_generic_strides_equals_oracle(hip_device, bf16, T):
    """the taps of a [B][A][32] buffer: sa = 32, sb = 32 * A, neither equals the tap count (the packer's strided branch)"""
    A, B = 12, 40
    Ts = 27 if T == 36 else T
    w = _t(320 + T, 'pack1s', (B * A * 32,), std=0.1)
    wd = w.to(hip_device)
    for flip in ((0, 1) if Ts == 27 else (0,)):
        got = _pack_one(wd, A, B, T, 32, 32 * A, flip, bf16)
        assert torch.equal(_bits(got), _bits(_oracle(w, A, B, T, 32, 32 * A, flip, bf16))), flip


@pytest.mark.parametrize('T', [28, 64])
def test_single_pack_refuses_unsupported_tap_counts(hip_device, T):
    """the packer stages at most 27 source taps per channel pair: T is <= 27, or 36 / 48 (fp32 Winograd images of 27 taps)"""
    from segmentation3d import _engine as E
    A, B = 8, 32
    wd = torch.zeros(A * B * T, device=hip_device)
    wp = torch.zeros(E.query('seg3d_packed_mfma_floats', A, B, T), device=hip_device)   # (at least the bf16 image's bytes)
    for name in ('seg3d_pack_weights_mfma', 'seg3d_pack_weights_mfma_bf16'):
        with pytest.raises(ValueError):
            E.call(name, E.ptr(wd), E.ptr(wp), A, B, T, T, A * T, 0, E.stream_ptr())


def test_bf16_multi_pack_equals_single_pack(hip_device):
    """PackedWeightCache.repack_all() refreshes every bf16 weight image with ONE launch (pack_mfma_bf16_multi_kernel,
    coalesced read / LDS transpose); the images equal the oracle's bit for bit, and so do those of the per-tensor entry point,
    both weight orientations (forward: w[b][a][t]; data-gradient: flipped taps, w[a][b][t] strides), partial channel blocks
    included"""
    from segmentation3d import _ops
    cache = _ops.PackedWeightCache()
    cache.enabled = True
    specs = [(32, 32), (64, 16), (16, 48), (256, 128)]
    ws, images = [], []
    for k, (cin, cout) in enumerate(specs):
        w = _t(80 + k, 'pk', (cout, cin, 3, 3, 3), std=0.1).to(hip_device)
        ws.append(w)
        images.append(cache.get(w, cin, cout, 27, 27, cin * 27, 0, bf16=True))          # forward orientation
        images.append(cache.get(w, cout, cin, 27, cin * 27, 27, 1, bf16=True))          # data-gradient orientation
    for w in ws:
        w.mul_(1.5).add_(0.01)
    cache.repack_all()
    k = 0
    for w, (cin, cout) in zip(ws, specs):
        for (A, B, sa, sb, flip) in ((cin, cout, 27, cin * 27, 0), (cout, cin, cin * 27, 27, 1)):
            ref = _bits(_oracle(w.cpu(), A, B, 27, sa, sb, flip, bf16=True))
            assert torch.equal(_bits(images[k]), ref), (cin, cout, flip)
            assert torch.equal(_bits(_pack_one(w, A, B, 27, sa, sb, flip, True)), ref), (cin, cout, flip)
            k += 1


def test_fp32_multi_pack_equals_single_pack(hip_device):
    """PackedWeightCache.repack_all() in fp32: ONE launch (pack_mfma_multi_kernel) refreshes the 27-tap images, the Winograd
    F(2, 3) (T = 36) and F(2x2, 3x3) (T = 48: one thread per channel pair, twelve 16-byte words each) images and the 8-tap
    stride-2 images; every image equals the oracle's bit for bit, and so does the per-tensor entry point's, both weight
    orientations (the data-gradient one with flipped taps), partial channel blocks included"""
    from segmentation3d import _ops
    cache = _ops.PackedWeightCache()
    cache.enabled = True
    specs = [(32, 32), (64, 16), (16, 48), (256, 128), (40, 72)]
    ws, images = [], []
    for k, (cin, cout) in enumerate(specs):
        w = _t(180 + k, 'pk32', (cout, cin, 3, 3, 3), std=0.1).to(hip_device)
        ws.append(w)
        for T in (27, 36, 48):
            images.append(cache.get(w, cin, cout, T, 27, cin * 27, 0))          # forward orientation
            images.append(cache.get(w, cout, cin, T, cin * 27, 27, 1))          # data-gradient orientation
    w8 = _t(190, 'pk8', (32, 16, 2, 2, 2), std=0.1).to(hip_device)               # stride-2 conv 16 -> 32
    img8 = cache.get(w8, 16, 32, 8, 8, 16 * 8, 0)
    for w in ws + [w8]:
        w.mul_(1.5).add_(0.01)
    cache.repack_all()
    k = 0
    for w, (cin, cout) in zip(ws, specs):
        for T in (27, 36, 48):
            for (A, B, sa, sb, flip) in ((cin, cout, 27, cin * 27, 0), (cout, cin, cin * 27, 27, 1)):
                ref = _bits(_oracle(w.cpu(), A, B, T, sa, sb, flip))
                assert torch.equal(_bits(images[k]), ref), (cin, cout, T, flip)
                assert torch.equal(_bits(_pack_one(w, A, B, T, sa, sb, flip, False)), ref), (cin, cout, T, flip)
                k += 1
    ref = _bits(_oracle(w8.cpu(), 16, 32, 8, 8, 16 * 8, 0))
    assert torch.equal(_bits(img8), ref)
    assert torch.equal(_bits(_pack_one(w8, 16, 32, 8, 8, 16 * 8, 0, False)), ref)
