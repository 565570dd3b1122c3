"""The device's operand split (csrc/ac_split_bf16.h) against the packers' split (kernels.split_bf16), bit for bit.

Both sides of the ABI split an f32 value into hi = RNE_bf16(x), lo = RNE_bf16(x - hi): the kernels split the
activations with the hardware convert, the packers split the weights with torch on the host.  One launch of
ac_split_bf16_probe on 4 096 values - normal values over 2^-100 ... 2^100 with both signs, exact halfway cases between two
bf16 neighbours (even and odd lower neighbour: ties-to-even decides), the f32 values one ulp either side of those ties,
values that are already bf16 (their lo is a zero, with the sign torch gives it) and +-0 - must give the same 16 bits as the
host, for hi and for lo.  f32 denormals and non-finite values are outside the contract (activations and weights are finite
and BN-scaled; a lo of the smallest value here is still a normal f32) and are left out.
"""
import pytest
import torch

from audiocaption_amd import kernels

pytestmark = pytest.mark.gpu


def probe_inputs():
    i = torch.arange(4096, dtype=torch.int64)
    h = (i * 2654435761) % (1 << 32)                       # integer hash: the same bits under every torch version
    sign = (i & 1) << 31
    exp = 27 + (h >> 8) % 201                              # biased exponents of 2^-100 ... 2^100
    mant = h & 0x7fffff
    normal = sign | (exp << 23) | mant
    upper = sign | (exp << 23) | (mant & 0x7f0000)         # a bf16 value; bit 16 (its last place) even or odd with the hash
    tie = upper | 0x8000
    bits = torch.cat([normal[:2048], tie[2048:2560], tie[2560:3072] - 1, tie[3072:3584] + 1, upper[3584:4088],
                      torch.tensor([0, 1 << 31] * 4, dtype=torch.int64)])
    assert bits.numel() == 4096
    x = torch.from_numpy(bits.numpy().astype("uint32").view("float32").copy())
    assert bool(torch.isfinite(x).all()) and bool(((x == 0) | (x.abs() >= 2.0 ** -101)).all())
    odd = (tie[2048:2560] >> 16) & 1
    assert 0 < int(odd.sum()) < 512                        # both kinds of tie are present
    return x


def test_device_split_equals_the_packers_split():
    x = probe_inputs()
    hi_ref, lo_ref = kernels.split_bf16(x)
    hi, lo = kernels.split_bf16_device(x.cuda())
    torch.cuda.synchronize()
    assert hi.shape == x.shape and lo.shape == x.shape
    for name, got, ref in (("hi", hi, hi_ref), ("lo", lo, lo_ref)):
        got, ref = got.cpu().view(torch.int16), ref.view(torch.int16)
        bad = (got != ref).nonzero().flatten()
        assert bad.numel() == 0, (f"{name}: {bad.numel()} of 4096 differ, first at {int(bad[0])}: x = {float(x[bad[0]])!r}, "
                                  f"device {int(got[bad[0]]) & 0xffff:#06x}, host {int(ref[bad[0]]) & 0xffff:#06x}")


def test_probe_rejects_a_length_that_is_no_multiple_of_four():
    from audiocaption_amd import _lib
    with pytest.raises(_lib.HipLibraryError):
        kernels.split_bf16_device(torch.zeros(6, device="cuda"))
