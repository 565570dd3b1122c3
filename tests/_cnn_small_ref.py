"""CPU references for the Cnn6 / Cnn10 encoders and the 5x5 conv kernels (torch on the CPU only: neither oracle/ nor the
library), shared by tests/test_cnn_small_cpu.py, tests/test_gpu_conv5x5.py, tests/test_gpu_cnn_small.py and the generator
tests/golden/make_golden_cnn_small.py.

  * ``fixture_state`` / ``fixture_model_state``: the procedural weights the fixture g28_cnn_small.npz was made with - one BN
    channel in five of every conv block gets a NEGATIVE scale, so ReLU-before-pool and pool-before-ReLU differ visibly.
  * ``forward_f64``: both encoders from a log-mel (B, 64, T) in float64 plain torch - a restatement of the reference's
    Cnn6Encoder / Cnn10Encoder.forward (eval mode), not its code.
  * ``layer5`` / ``draw_layer5``: one 5x5 layer in float64, in the split-bf16 arithmetic of csrc/conv5x5.hip (built on
    ``_split_ref.split_products``: hi = RNE(x), lo = RNE(x - hi), hi*hi + hi*lo + lo*hi, f32 accumulation) and its
    magnitude, on the two input families of ``_split_ref``.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import _split_ref as S

CHANNELS = [1, 64, 128, 256, 512]
KINDS = {"cnn6": (5, 1), "cnn10": (3, 2)}      # kind -> (kernel size, convs per block)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g28_cnn_small.npz")
REPORT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "REPORT_cnn_small.txt")
BLOCK_CH_STRIDE = 16                            # the fixture keeps every 16th channel of a block output, and all channels' sums
VOCAB, MAX_LENGTH, BEAM = 64, 8, 3
# fixture cases: name -> (sample rate, frames T of the batch, frames of each clip)
CASES = {"a": (32000, 60, (60, 33, 16)), "b": (16000, 60, (60, 60)), "c": (32000, 1001, (1001, 626))}


def hop(sample_rate):
    return 10 * sample_rate // 1000


def wav_lens(case):
    sr, _, frames = CASES[case]
    return [hop(sr) * (t - 1) for t in frames]


def logmel(case):
    from audiocaption_amd import procedural as P
    _, T, frames = CASES[case]
    return torch.from_numpy(P.synthetic_logmel(len(frames), T))


def _negate_bn(state, prefix):
    for k in state:
        if k.startswith(prefix + "conv_block") and k.endswith(".weight") and ".bn" in k:
            state[k] = state[k].copy()
            state[k][::5] *= -1.0
    return state


def fixture_state(kind, prefix=""):
    """numpy state dict of the encoder ``kind`` ("cnn6" | "cnn10") as the fixture uses it."""
    from audiocaption_amd import procedural as P
    return _negate_bn({"cnn6": P.cnn6_state, "cnn10": P.cnn10_state}[kind](prefix), prefix)


def fixture_model_state(kind, seed):
    """numpy state dict of the captioner ``config.cnn6rnn_trm_config`` / ``cnn10rnn_trm_config`` (vocabulary ``VOCAB``)."""
    from audiocaption_amd import procedural as P
    fn = {"cnn6": P.cnn6_state, "cnn10": P.cnn10_state}[kind]
    return _negate_bn(P.cnn_small_rnn_trm_state(fn, vocab_size=VOCAB, seed=seed), "encoder.cnn.")


def feat_len(wav_len, sample_rate):
    return [(int(n) // hop(sample_rate) + 1) // 16 for n in wav_len]


def forward_f64(kind, state, lms, lens, prefix=""):
    """lms (B, 64, T) log-mel, ``lens``: attn_emb_len per clip -> attn_emb (B, T // 16, 512), fc_emb (B, 512) and the four
    pooled block outputs (B, C, H, W), all float64."""
    k, convs = KINDS[kind]
    t = {n[len(prefix):]: torch.as_tensor(v).double() for n, v in state.items() if n.startswith(prefix)}

    def bn(x, p):
        sc = t[p + ".weight"] / torch.sqrt(t[p + ".running_var"] + 1e-5)
        sh = t[p + ".bias"] - t[p + ".running_mean"] * sc
        return x * sc[None, :, None, None] + sh[None, :, None, None]

    x = lms.double().transpose(1, 2).unsqueeze(1)                 # (B, 1, T, 64)
    x = bn(x.transpose(1, 3), "bn0").transpose(1, 3)
    blocks = []
    for b in range(1, 5):
        for j in range(1, convs + 1):
            x = F.relu(bn(F.conv2d(x, t[f"conv_block{b}.conv{j}.weight"], padding=k // 2), f"conv_block{b}.bn{j}"))
        x = F.avg_pool2d(x, 2)
        blocks.append(x)
    attn = x.mean(dim=3).transpose(1, 2)                          # (B, T // 16, 512)
    pooled = torch.stack([attn[i, :n].max(dim=0).values + attn[i, :n].mean(dim=0) for i, n in enumerate(lens)])
    fc = F.relu(pooled @ t["fc1.weight"].t() + t["fc1.bias"])
    return {"attn_emb": attn, "fc_emb": fc, "blocks": blocks}


def block_digest(blk):
    """What the fixture keeps of a block output (B, C, H, W): every ``BLOCK_CH_STRIDE``-th channel in full (f32) and the sum
    and absolute sum of every channel (f64) - the whole of it does not fit the size limit of a committed file."""
    blk = torch.as_tensor(blk).double()
    return {"sub": blk[:, ::BLOCK_CH_STRIDE].float().numpy(), "sum": blk.sum(dim=(2, 3)).numpy(),
            "abs_sum": blk.abs().sum(dim=(2, 3)).numpy()}


def x0_rows(lms, scale, shift, Hp0):
    """The encoders' ``_logmel`` input from a log-mel (B, 64, T): bn0 applied with torch, rows >= T zero, [B*Hp0][64]."""
    B, _, T = lms.shape
    x0 = torch.zeros(B, Hp0, 64, device=lms.device)
    x0[:, :T] = lms.transpose(1, 2) * scale + shift
    return x0.reshape(B * Hp0, 64).contiguous()


# ---- one 5x5 layer ------------------------------------------------------------------------------------------------------
def draw_layer5(family, B, H, W, Cin, Cout, seed):
    """``_split_ref.draw_layer`` with 5x5 weights: x (B, Cin, H, W), w OIHW, scale, shift."""
    assert family in S.FAMILIES, family
    g = S._gen(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    gain = None
    if family == "checkpoint-like":
        gain = torch.exp(torch.randn(Cin, generator=g))
        x = F.relu(x + 0.5) * gain.view(1, -1, 1, 1)
    w = S._weights_draw(g, family, Cout, Cin, (5, 5), gain)
    sc, sh = S._bn_draw(g, family, Cout)
    return x, w, sc, sh


def conv5_split(x, w, ar=S.FAITHFUL):
    """conv5x5 (padding 2) of x (B, C, H, W) f32 with w OIHW f32 in the kernel's arithmetic: (B, O, H, W) f32."""
    B, C, H, W = x.shape
    O = w.shape[0]
    xp = F.pad(x.float(), (2, 2, 2, 2))
    V = torch.stack([xp[:, :, ky:ky + H, kx:kx + W].permute(1, 0, 2, 3).reshape(C, -1) for ky in range(5) for kx in range(5)], 0)
    U = w.float().permute(2, 3, 0, 1).reshape(1, 25, O, C)
    y = S.split_products(U, V[None], ar)[0]                        # (O, B * H * W)
    return y.reshape(O, B, H, W).permute(1, 0, 2, 3)


def layer5(x, w, sc, sh, mode, ar=S.FAITHFUL):
    """``_split_ref.Case`` of relu(scale * conv5x5(x, w) + shift) (+ 2x2 average pool, mode 1): exact (float64), emul (the
    kernel's arithmetic), mag = |scale| * conv5x5(|x|, |w|), each (B, H', W', Cout)."""
    y = F.relu(S._bn(F.conv2d(x.double(), w.double(), padding=2), sc.double(), sh.double()))
    mag = F.conv2d(x.double().abs(), w.double().abs(), padding=2) * sc.double().abs()[None, :, None, None]
    emul = F.relu(S._fma_bn(conv5_split(x, w, ar), sc, sh))
    return S.Case(S._epilogue(y, mode), S._epilogue(emul, mode), S._epilogue(mag, mode), dict(form="conv5x5", mode=mode, cin=x.shape[1]))


SMALLEST_MUTANT = S.Arith(x_lo="trunc")   # "lo = trunc(x - hi), activations only": the smallest of ``_split_ref.mutants``


def abs_bar(cin):
    """The absolute bar of tests/test_gpu_kernels.py for the split-bf16 convs on randn data, at K = 25 * Cin."""
    return 1e-3 * max(1.0, math.sqrt(25 * cin / 576))


def report(line):
    """Print a figure and, when CNN_SMALL_REPORT names a file, append it there (how the measured section of
    tests/golden/REPORT_cnn_small.txt is collected)."""
    print(line, flush=True)
    path = os.environ.get("CNN_SMALL_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")
