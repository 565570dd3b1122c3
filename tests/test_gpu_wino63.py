"""GPU tests of the row-SEXTET form of the F(4,3) conv kernel (F(6,3) along time, csrc/conv3x3_wino43.hip), through the C ABI
entries ac_conv3x3_bn_relu_wino63 / _drop.

Reference: F.conv2d in fp32 on the CPU (+ folded BatchNorm, ReLU, 2x2 average pool).  Error bar, componentwise: the bound
``_split_ref.layer_bound`` derives for a split-bf16 Winograd layer - 2^-15 of the transform-aware magnitude - evaluated for
m = 6 with the sextets where the kernel puts them (over the stacked rows of the batch: tests/_wino63_ref.py), plus the fp32
reference's own distance from the float64 result.  Nothing is taken from the kernel under test.  Rows at or beyond H must be
exactly zero."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import _split_ref as S
import _wino63_ref as R6

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    from audiocaption_amd import build
    build.build()
    from audiocaption_amd import kernels
    return kernels


@functools.lru_cache(maxsize=None)
def _case(B, H, Hp, W, Cin, Cout, mode):
    """Inputs, the fp32 reference and the bar of one layer, computed once and shared by the launch variants."""
    x, w, sc, sh = S.draw_layer("randn", B, H, W, Cin, Cout, 1000 * B + 10 * H + W + Cin + mode)
    ref32 = S._epilogue(F.relu(F.conv2d(x, w, padding=1) * sc[None, :, None, None] + sh[None, :, None, None]), mode)
    exact, _ = S.layer_exact(x, w, sc, sh, mode)
    bar = R6.stacked_bound(x, w, sc, mode, Hp) + (ref32.double() - exact).abs()
    return x, w, sc, sh, ref32, bar


def _out_buffer(B, Hp, W, Cout, mode):
    return torch.full((B * Hp, W, Cout) if mode == 0 else (B * Hp // 2, W // 2, Cout), 7.0, device="cuda")


def _valid(out, B, rows):
    """The kernel's buffer -> (B, rows, W', Cout) valid rows; every row from ``rows`` on must be exactly zero."""
    got = out.cpu().reshape(B, -1, *out.shape[1:])
    assert torch.equal(got[:, rows:], torch.zeros_like(got[:, rows:])), "rows at or beyond H are zeros"
    return got[:, :rows]


def _hold(name, got, ref32, bar):
    assert got.shape == ref32.shape and bool(torch.isfinite(got).all())
    err = (got.double() - ref32.double()).abs()
    worst = float((err / bar).max())
    print(f"[{name}] max|diff| {float(err.max()):.3e}, worst |diff| / bar {worst:.3f}", flush=True)
    assert bool((err <= bar).all()), (name, worst)


# B, H, Hp, W, Cin, Cout
TWO_K_STEPS = (3, 13, 16, 32, 32, 128)    # 48 rows = 8 sextets: rows no multiple of 6, sextets straddle clips, the kernel's shortest K loop
SMALL_W = (5, 7, 8, 8, 64, 256)           # 40 rows: a partial last sextet; a tile of 4 (8) sextets spans every clip; two channel tiles
HALF_SIZE = (2, 21, 24, 32, 64, 128)      # conv1 of block 2: four K steps = half-size workgroups by default
W16 = (2, 10, 12, 16, 64, 128)            # the 16-column instance


@pytest.mark.parametrize("map_mode", [-1, 0])
@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [TWO_K_STEPS, SMALL_W, W16], ids=["two-k-steps", "w8", "w16"])
def test_wino63_vs_conv2d(K, shape, mode, tiles, map_mode):
    """Full and pooled output, both workgroup sizes and block maps, against F.conv2d in fp32."""
    B, H, Hp, W, Cin, Cout = shape
    x, w, sc, sh, ref32, bar = _case(*shape, mode)
    out = _out_buffer(B, Hp, W, Cout, mode)
    K.conv3x3_bn_relu_wino63(S.to_rows(x, Hp).cuda(), K.pack_conv_weight_wino63_frag(w.cuda()), sc.cuda(), sh.cuda(), out, B, Hp, H,
                             W, Cin, Cout, mode, map_mode, tiles_per_wave=tiles)
    _hold(f"wino63 x{tiles} map{map_mode} {B}x{H}x{W} {Cin}->{Cout} mode{mode}", _valid(out, B, ref32.shape[1]), ref32, bar)


@pytest.mark.parametrize("mode", [0, 1])
def test_wino63_half_size_form_is_the_default_for_short_k(K, mode):
    """Cin = 64 at W = 32: tiles_per_wave = 0 picks the half-size workgroups (bit-identical to asking for them), and both
    sizes hold the bar."""
    B, H, Hp, W, Cin, Cout = HALF_SIZE
    x, w, sc, sh, ref32, bar = _case(*HALF_SIZE, mode)
    xr, wp, scd, shd = S.to_rows(x, Hp).cuda(), K.pack_conv_weight_wino63_frag(w.cuda()), sc.cuda(), sh.cuda()
    outs = {}
    for tiles in (0, 1, 2):
        outs[tiles] = _out_buffer(B, Hp, W, Cout, mode)
        K.conv3x3_bn_relu_wino63(xr, wp, scd, shd, outs[tiles], B, Hp, H, W, Cin, Cout, mode, tiles_per_wave=tiles)
        _hold(f"wino63 x{tiles} {B}x{H}x{W} {Cin}->{Cout} mode{mode}", _valid(outs[tiles], B, ref32.shape[1]), ref32, bar)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[1], outs[2]), "a pixel's sum does not depend on the workgroup's size"


def _dead_rows(B, Hp, H, rows_blk, need):
    """Stacked rows of the row blocks (``rows_blk`` rows each, from row 0) in which every row lies at or beyond
    min(H, need[b]) of its clip: the blocks the kernel does not convolve (csrc/ac_conv_tile.h rows_live)."""
    dead = torch.zeros(B * Hp, dtype=torch.bool)
    for r0 in range(0, B * Hp, rows_blk):
        r1 = min(r0 + rows_blk, B * Hp)
        live = any(max(r0, b * Hp) - b * Hp < min(H, need[b]) for b in range(r0 // Hp, (r1 - 1) // Hp + 1))
        dead[r0:r1] = not live
    return dead


@pytest.mark.parametrize("tiles", [1, 2])
@pytest.mark.parametrize("mode", [0, 1])
def test_wino63_ragged_batch_kills_whole_sextets(K, mode, tiles):
    """``clip_frames``: row blocks (6 * tiles sextet rows at W = 32) wholly at or beyond a clip's need store zeros, every
    other row is bit-identical to the dense launch - also where a live block straddles a dead clip's padding."""
    B, H, Hp, W, Cin, Cout = 4, 17, 20, 32, 64, 128
    x, w, sc, sh, ref32, bar = _case(B, H, Hp, W, Cin, Cout, mode)
    xr, wp, scd, shd = S.to_rows(x, Hp).cuda(), K.pack_conv_weight_wino63_frag(w.cuda()), sc.cuda(), sh.cuda()
    frames = torch.tensor([17, 5, 12, 0], dtype=torch.int32)
    full, skip = _out_buffer(B, Hp, W, Cout, mode), _out_buffer(B, Hp, W, Cout, mode)
    K.conv3x3_bn_relu_wino63(xr, wp, scd, shd, full, B, Hp, H, W, Cin, Cout, mode, tiles_per_wave=tiles)
    K.conv3x3_bn_relu_wino63(xr, wp, scd, shd, skip, B, Hp, H, W, Cin, Cout, mode, tiles_per_wave=tiles, need=(frames.cuda(), 1, 0))
    _hold(f"wino63 dense x{tiles} mode{mode}", _valid(full, B, ref32.shape[1]), ref32, bar)
    dead = _dead_rows(B, Hp, H, 6 * tiles, [int(f) for f in frames])
    assert bool(dead.any()) and not bool(dead[:H].any())
    if mode == 1:
        dead = dead[::2]        # a block's rows pool among themselves (an even number from an even row)
    want = full.cpu().clone()
    want[dead] = 0
    assert torch.equal(skip.cpu(), want)
    assert not torch.equal(skip.cpu(), full.cpu()), "at least one block with non-zero results was skipped"


@pytest.mark.parametrize("seed", [1234, 99])
@pytest.mark.parametrize("shape,mode", [(TWO_K_STEPS, 0), (SMALL_W, 1)], ids=["full", "pooled"])
def test_wino63_dropout_twin(K, shape, mode, seed):
    """F.dropout inside the epilogue equals, bit for bit, the layer followed by the counter-hash dropout pass over its
    output buffer - with and without the device-side step seed."""
    B, H, Hp, W, Cin, Cout = shape
    x, w, sc, sh, _, _ = _case(*shape, mode)
    xr, wp, scd, shd = S.to_rows(x, Hp).cuda(), K.pack_conv_weight_wino63_frag(w.cuda()), sc.cuda(), sh.cuda()
    step = torch.tensor([5], dtype=torch.int64, device="cuda")
    for seed_dev in (None, step.data_ptr()):
        two, one = _out_buffer(B, Hp, W, Cout, mode), _out_buffer(B, Hp, W, Cout, mode)
        K.conv3x3_bn_relu_wino63(xr, wp, scd, shd, two, B, Hp, H, W, Cin, Cout, mode)
        K.dropout_(two, two.numel(), 0.2, seed, seed_dev)
        K.conv3x3_bn_relu_wino63(xr, wp, scd, shd, one, B, Hp, H, W, Cin, Cout, mode, dropout=(0.2, seed, seed_dev))
        assert torch.equal(one, two)
        valid = one.reshape(B, -1, *one.shape[1:])[:, :(H if mode == 0 else H // 2)]
        assert 0.1 < float((valid == 0).float().mean()) < 0.9


def test_wino63_rejects_what_it_does_not_cover(K):
    from audiocaption_amd._lib import HipLibraryError
    wp = torch.zeros(4, 24, 4, 2, 64, 8, dtype=torch.bfloat16).cuda()
    sc = torch.ones(128).cuda()
    out = torch.zeros(2 * 8, 4, 128).cuda()
    with pytest.raises(HipLibraryError):
        K.conv3x3_bn_relu_wino63(torch.zeros(2 * 8, 4, 64).cuda(), wp, sc, sc, out, 2, 8, 5, 4, 64, 128, 0)      # W = 4: blocks 5-6 keep quads
    with pytest.raises(HipLibraryError):
        K.conv3x3_bn_relu_wino63(torch.zeros(2 * 6, 8, 64).cuda(), wp, sc, sc, out, 2, 6, 5, 8, 64, 128, 0)      # Hp % 4 != 0
    assert tuple(K.pack_conv_weight_wino63_frag(torch.zeros(128, 64, 3, 3).cuda()).shape) == (4, 24, 4, 2, 64, 8)


def test_default_route_takes_sextets_only_where_measured(K):
    """``cnn_encoder.sextet_route``: never single clips or small launches, never conv blocks 5-6."""
    from audiocaption_amd import cnn_encoder as CE
    for W, Cin in ((4, 512), (4, 1024), (2, 1024), (2, 2048)):
        assert not CE.sextet_route(64, 64, W, Cin, 1024)
    for W, Cin, Cout in CE.SEXTET_LAYERS:
        assert W in (32, 16, 8)
        assert not CE.sextet_route(1, 504 * W // 32, W, Cin, Cout)
