"""The weight packers of kernels.py, byte for byte, and the split they share (CPU only).

Every packer pre-splits the weights the way the kernels split the activations (kernels.split_bf16, csrc/ac_split_bf16.h)
and lays them out in the order a kernel reads them; a changed rounding or a transposed axis only shows up as a conv tier
missing its error bar somewhere downstream.  So the packed BYTES are pinned here.  The weights come from an integer hash, not
a random generator (the bytes must not depend on the torch version), with a few exact bf16 ties (even and odd neighbour),
an output channel and an input channel of zeros.  The shapes are the smallest that give every axis of the layouts more than
one step: two 32-channel chunks / four 16-channel steps of Cin and up to four 32-channel tiles of Cout.
"""
import hashlib

import pytest
import torch

from audiocaption_amd import kernels

SHAPES = [(64, 32), (128, 64)]   # (Cout, Cin)


def hashed_weight(cout, cin, kh=3, kw=3):
    n = cout * cin * kh * kw
    i = torch.arange(n, dtype=torch.int64)
    w = (((i * 2654435761) % (1 << 32)).double() / float(1 << 32) - 0.5).float().reshape(cout, cin, kh, kw)
    w[3] = 0.0                                   # an output channel of zeros
    w[:, 5] = 0.0                                # an input channel of zeros
    flat = w.view(-1)
    # exact halfway cases between two bf16 neighbours: the lower neighbour even (1, 0.25) and odd (1 + 2^-7, 0.25 (1 + 2^-7))
    ties = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), 0.25 + 2.0 ** -10,
            0.25 + 3 * 2.0 ** -10]
    for j, t in enumerate(ties):
        flat[7 * cin * kh * kw + 100 + 37 * j] = t   # from output channel 7 on: clear of the zeros in every shape used
    assert not bool(w[3].any()) and not bool(w[:, 5].any()) and sum(int((w == t).sum()) for t in ties) == len(ties)
    return w


def sha(t):
    t = t.contiguous()
    return hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest()


def pack_digests(k=kernels):
    """name -> SHA-256 of the packed bytes, for every packer and both shapes."""
    out = {}
    for cout, cin in SHAPES:
        w = hashed_weight(cout, cin)
        tag = f"{cout}x{cin}"
        for name in ("pack_conv_weight", "pack_conv_weight_winograd", "pack_conv_weight_bf16x3", "pack_conv_weight_bf16x3_frag",
                     "pack_conv_weight_wino1d_frag", "pack_conv_weight_wino43_frag", "pack_conv_weight_wino63_frag"):
            out[f"{name}:{tag}"] = sha(getattr(k, name)(w))
        frag, inv_scale = k.pack_conv_weight_f16x2_frag(w)
        out[f"pack_conv_weight_f16x2_frag:{tag}"] = sha(frag)
        out[f"pack_conv_weight_f16x2_frag.inv_scale:{tag}"] = sha(inv_scale)
        out[f"pack_linear_weight_bf16x3_frag:{tag}"] = sha(k.pack_linear_weight_bf16x3_frag(hashed_weight(cout, cin, 1, 1)[:, :, 0, 0]))
    return out


# pack_digests() of kernels.py as it stood BEFORE the packers were rebuilt on split_bf16 / _frag_order (the parent commit of
# that change), written down once: the rebuilt packers must produce the same bytes.
EXPECTED = {
    "pack_conv_weight:128x64": "6d94878bdb08affcebef68325aa373bd1abb06a89e83533f0ac0900b0f052456",
    "pack_conv_weight:64x32": "fbf2c1b08bd85958f2c68860704298df7c4c6ba106e4270e6d9bf5718157842f",
    "pack_conv_weight_bf16x3:128x64": "3f789e5e4614feda568b602915aed4088dff3dd37bb1fea1069465effae0af1e",
    "pack_conv_weight_bf16x3:64x32": "6754264318c29aa67322d41bb2b61a2bdcded4936872f039df65f37787d566ab",
    "pack_conv_weight_bf16x3_frag:128x64": "bf70c811770857e816d56f205715646790827bf16717ad4048e55e3034a36df7",
    "pack_conv_weight_bf16x3_frag:64x32": "ee391f92599fc56b7a3a25296a6e84f9e3caed2cf9239b4465285d02e86bf6d0",
    "pack_conv_weight_f16x2_frag.inv_scale:128x64": "4ebaf10a0e28604b34c4fb327f683d68fec649df89574f4117c8ae4817f454fd",
    "pack_conv_weight_f16x2_frag.inv_scale:64x32": "f2dc18c39ea50baf32a68cbc73bea7e3cfc3c613089e580a10d471ee7049dac4",
    "pack_conv_weight_f16x2_frag:128x64": "563335a5f00da9998ec06ccfbe20ae259b11513d8eb07e38d87b7d32c8c73644",
    "pack_conv_weight_f16x2_frag:64x32": "132b92a9bee9f7568f5420f146aaf1546d606e3961486e3c58d653322c27e1fb",
    "pack_conv_weight_wino1d_frag:128x64": "c4e6430e21915bfc13c1cb68de441ab316ecd4bb3178556f874fa481048d9654",
    "pack_conv_weight_wino1d_frag:64x32": "c8868066e33cfe8f4e567c8bcd9bc81fc8af09d5834f0a6cd241762d9f9ac28e",
    "pack_conv_weight_wino43_frag:128x64": "2c9525324a21b41a1467834824bab091dee111e70819243aa05198dd54012e18",
    "pack_conv_weight_wino43_frag:64x32": "2b2385267b40edd8da7feec28adc64a69f35386188c8c337789b8b12383455ff",
    "pack_conv_weight_wino63_frag:128x64": "9b5a85ee677a84c7fa5218121ca4e825218af1475dd33bfed6b3be1d0c1886ee",
    "pack_conv_weight_wino63_frag:64x32": "37f6532292de20d21403f7a9b475d92f2fc9d6ceb8f15a6ee31b4d30d793ae11",
    "pack_conv_weight_winograd:128x64": "a83f2fb9d42a59ec6cc684649d399ed0798725c5095ec23fd9c7e0b7aa170653",
    "pack_conv_weight_winograd:64x32": "d20aab05f86f95fc2863a000bf52d14880f3bac845a9445702c6322b73b80fac",
    "pack_linear_weight_bf16x3_frag:128x64": "152e63aebeb70a142d9eacc743496b65e6a62880f4a1da7fb4a1b18cd2d18679",
    "pack_linear_weight_bf16x3_frag:64x32": "58c26a2a4157432605339dcd7e0494998c87f66f6f82784517e1b7ad9670877d",
}


@pytest.fixture(scope="module")
def digests():
    return pack_digests()


@pytest.mark.parametrize("key", sorted(EXPECTED))
def test_packed_bytes_are_unchanged(digests, key):
    assert digests[key] == EXPECTED[key]


def test_every_packer_is_pinned(digests):
    assert set(digests) == set(EXPECTED)
    conv_packers = {n for n in dir(kernels) if n.startswith("pack_conv_weight")}
    assert conv_packers == {k.split(":")[0].split(".")[0] for k in EXPECTED if k.startswith("pack_conv_weight")}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_split_bf16_contract(dtype):
    """hi + lo is within 2^-16 |u| of u, both halves are bf16, and the subtraction runs in u's own precision."""
    u = hashed_weight(128, 64).to(dtype).view(-1)
    u = torch.cat([u, u * 2.0 ** 40, u * 2.0 ** -40])
    hi, lo = kernels.split_bf16(u)
    assert hi.dtype == torch.bfloat16 and lo.dtype == torch.bfloat16
    assert torch.equal(hi, u.to(torch.bfloat16))
    assert torch.equal(lo, (u - hi.to(dtype)).to(torch.bfloat16))
    err = (hi.float() + lo.float()).double() - u.double()
    assert bool((err.abs() <= 2.0 ** -16 * u.double().abs()).all())
