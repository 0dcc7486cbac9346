"""The layout bridges at the plugin API edge (csrc/layout.hip: ncdhw_to_ndhwc_kernel, ndhwc_to_ncdhw_kernel, both branches of
copy_channels_kernel), driven through the C ABI, bit for bit against permute(...).contiguous() / slicing on the CPU.  The cases are
those of tests/loss_cases.py; tests/test_loss_cases.py shows on the host which of them take a second grid-stride trip and which
copy cases take the 16-byte path.

They are byte movers, so the operands are bit patterns, not numbers: element i of a buffer holds the 32-bit hash of (i, salt) -- every
element differs from every other, NaN payloads and denormals included -- and everything is compared as int32.  Sources and
destinations sit inside NaN guard bands; the sources must come back unchanged.  seg3d_copy_channels writes into a destination that
already holds a pattern of its own: the channels outside [dst_off, dst_off + C) must keep it.

seg3d_copy_channels picks its 16-byte path on the host: C, both row pitches and both offsets multiples of 4 AND both bases 16-byte
aligned.  Five cases break one of the five numbers each; one keeps all five and moves both bases one float past a 16-byte boundary
(it runs only because the launcher looks at the bases: the float4 path would fault there).
"""
import pytest
import torch

import loss_cases as K
from float64_util import Guarded, _engine
from gpu_util import report

pytestmark = pytest.mark.gpu

GUARD = 1024


def _bits(t):
    return t.view(torch.int32)


def _hash_bits(n, salt):
    """int32 [n]: (i * 2654435761 + salt) mod 2^32, a bijection of i"""
    x = (torch.arange(n, dtype=torch.int64) * 2654435761 + salt) & 0xFFFFFFFF
    return torch.where(x >= (1 << 31), x - (1 << 32), x).to(torch.int32)


class _Slot:
    """`n` floats holding `bits`, `shift` floats past a 16-byte boundary, NaN around them inside a Guarded buffer"""

    def __init__(self, n, bits, dev, shift=0):
        self.g = Guarded(n + (4 if shift else 0), GUARD, dev)
        self.n, self.shift = n, shift
        self.t = self.g.t[shift:shift + n]
        _bits(self.t).copy_(bits.to(dev))
        assert self.t.data_ptr() % 16 == 4 * shift

    def holds(self, bits):
        around = torch.cat([self.g.t[:self.shift], self.g.t[self.shift + self.n:]])
        return self.g.guards_untouched() and bool(torch.isnan(around).all()) and bool(torch.equal(_bits(self.t).cpu(), bits))


@pytest.mark.parametrize('case', K.LAYOUT_CASES, ids=K.case_id)
@pytest.mark.parametrize('entry', ['seg3d_ncdhw_to_ndhwc', 'seg3d_ndhwc_to_ncdhw'])
def test_layout_bridge(hip_device, entry, case):
    E, dev = _engine(), hip_device
    N, C, S = case
    n = N * C * S
    bits = _hash_bits(n, 17)
    shape = (N, C, S) if entry == 'seg3d_ncdhw_to_ndhwc' else (N, S, C)
    want = bits.reshape(shape).permute(0, 2, 1).contiguous().reshape(-1)
    src, out = _Slot(n, bits, dev), Guarded(n, GUARD, dev)
    E.call(entry, E.ptr(src.t), E.ptr(out.t), N, C, S, E.stream_ptr())
    torch.cuda.synchronize()
    assert out.guards_untouched(), 'the guard bands of the output were written'
    wrong = int((_bits(out.t).cpu() != want).sum())
    assert wrong == 0, '{} of {} elements differ'.format(wrong, n)
    assert src.holds(bits), 'the input was written'
    report('layout/{}/{}'.format(entry, K.case_id(case)), exact=1.0)


@pytest.mark.parametrize('case', K.COPY_CASES, ids=K.case_id)
def test_copy_channels(hip_device, case):
    E, dev, c = _engine(), hip_device, case
    dst_bits = _hash_bits(c.nvox * c.dst_ld, 29)
    dst = _Slot(c.nvox * c.dst_ld, dst_bits, dev, c.shift)
    if c.in_place:
        src_bits, src = dst_bits, dst
    else:
        src_bits = _hash_bits(c.nvox * c.src_ld, 23)
        src = _Slot(c.nvox * c.src_ld, src_bits, dev, c.shift)
    want = dst_bits.reshape(c.nvox, c.dst_ld).clone()
    want[:, c.dst_off:c.dst_off + c.C] = src_bits.reshape(c.nvox, c.src_ld)[:, c.src_off:c.src_off + c.C]
    E.call('seg3d_copy_channels', E.ptr(src.t), E.ptr(dst.t), c.nvox, c.C, c.src_ld, c.src_off, c.dst_ld, c.dst_off, E.stream_ptr())
    torch.cuda.synchronize()
    got = _bits(dst.t).cpu().reshape(c.nvox, c.dst_ld)
    inside = torch.zeros(c.dst_ld, dtype=torch.bool)
    inside[c.dst_off:c.dst_off + c.C] = True
    assert bool(torch.equal(got[:, inside], want[:, inside])), '{} copied elements differ'.format(int((got != want)[:, inside].sum()))
    assert bool(torch.equal(got[:, ~inside], want[:, ~inside])), '{} elements outside the slice were written'.format(
        int((got != want)[:, ~inside].sum()))
    assert dst.holds(want.reshape(-1)), 'written around the destination'
    assert c.in_place or src.holds(src_bits), 'the source was written'
    report('layout/copy/' + K.case_id(c), vec=float(K.copy_vec(c)), exact=1.0)


@pytest.mark.parametrize('args,why', K.COPY_REFUSALS, ids=[r[1] for r in K.COPY_REFUSALS])
def test_copy_channels_refusals_write_nothing(hip_device, args, why):
    E, dev = _engine(), hip_device
    nvox, C, src_ld, src_off, dst_ld, dst_off = args
    src_bits, dst_bits = _hash_bits(nvox * src_ld, 23), _hash_bits(nvox * dst_ld, 29)
    src, dst = _Slot(nvox * src_ld, src_bits, dev), _Slot(nvox * dst_ld, dst_bits, dev)
    with pytest.raises(ValueError) as info:
        E.call('seg3d_copy_channels', E.ptr(src.t), E.ptr(dst.t), nvox, C, src_ld, src_off, dst_ld, dst_off, E.stream_ptr())
    assert str(info.value).startswith('seg3d_copy_channels:'), (why, str(info.value))
    torch.cuda.synchronize()
    assert dst.holds(dst_bits) and src.holds(src_bits), why
