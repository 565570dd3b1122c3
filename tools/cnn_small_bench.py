#!/usr/bin/env python
"""Development tool: the light encoders (Cnn6Encoder, Cnn10Encoder) on 64 ten-second clips.

* ms per batch of each encoder alone (wav -> attn_emb, fc_emb) and under CrnnEncoder + a greedy decode of 20 tokens;
* per 5x5 layer of Cnn6 (blocks 2-4, with the pool): time and the bf16 MFMA rate it achieves, beside
  ``conv3x3_bn_relu_bf16x3_gw`` (the 3x3 direct split-bf16 kernel) on the 3x3 layer of the same (W, Cin, Cout), alternating
  the two in one process.  MFMA work is counted from the shapes: 3 products x 2 x (B * Hp * W pixels) x Cout x taps x Cin -
  both kernels run the matrix cores over the padded rows too (tiles made of padding alone excepted).

Timing: device events around ``--iters`` back-to-back calls after ``--warmup`` calls, median of ``--repeats`` windows.
Prints a table and one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import audiocaption_amd as A  # noqa: E402
from audiocaption_amd import kernels as K, procedural as P  # noqa: E402

LAYERS = [(32, 64, 128), (16, 128, 256), (8, 256, 512)]   # (W, Cin, Cout) of Cnn6's blocks 2-4


def timed(fn, warmup, iters, repeats):
    """Median over ``repeats`` windows of the device time of one call, in ms."""
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-length", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cnn_small_bench: needs the GPU (there is no CPU timing to report)")
    B, L = args.batch, int(args.seconds * 32000)
    wav = torch.from_numpy(P.synthetic_wav(B, L, varied=True)).cuda()
    res = {"batch": B, "seconds": args.seconds}

    for kind, cfg, state in (("cnn6", A.cnn6rnn_trm_config, P.cnn6_state), ("cnn10", A.cnn10rnn_trm_config, P.cnn10_state)):
        model = A.init_model_from_config(cfg(4368), print_fn=lambda s: None)
        model.load_state_dict(P.to_torch(P.cnn_small_rnn_trm_state(state, 4368)), strict=False)
        model = model.eval().to("cuda:0")
        enc_in = {"wav": wav, "wav_len": [L] * B}
        med, lo, hi = timed(lambda: model.encoder.cnn(enc_in), args.warmup, args.iters, args.repeats)
        res[f"{kind}_encoder_ms"] = round(med, 3)
        print(f"{kind}: encoder alone {med:.3f} ms per {B} clips (windows {lo:.3f} .. {hi:.3f})")
        cap_in = dict(enc_in, mode="inference", specaug=False, sample_method="greedy", max_length=args.max_length)
        med, lo, hi = timed(lambda: model(cap_in), args.warmup, args.iters, args.repeats)
        res[f"{kind}_caption_ms"] = round(med, 3)
        print(f"{kind}: CrnnEncoder + greedy decode ({args.max_length} tokens) {med:.3f} ms per {B} clips (windows {lo:.3f} .. {hi:.3f})")
        if kind == "cnn6":
            Hp = model.encoder.cnn.geometry(L)[2]
            H = model.encoder.cnn.geometry(L)[1]
        del model

    g = torch.Generator().manual_seed(5)
    for lvl, (W, Cin, Cout) in enumerate(LAYERS, start=1):
        hp, h = Hp[lvl], H[lvl]
        x = torch.randn(B * hp, W, Cin, generator=g).cuda()
        x.view(B, hp, W, Cin)[:, h:] = 0
        sc, sh = torch.ones(Cout).cuda(), torch.zeros(Cout).cuda()
        out = torch.empty(B * hp // 2, W // 2, Cout, device="cuda")
        w5 = K.pack_conv5x5_weight((torch.randn(Cout, Cin, 5, 5, generator=g) * 0.02).cuda())
        w3 = K.pack_conv_weight_bf16x3_frag((torch.randn(Cout, Cin, 3, 3, generator=g) * 0.03).cuda())
        f5 = lambda: K.conv5x5_bn_relu_bf16x3(x, w5, sc, sh, out, B, hp, h, W, Cin, Cout, 1)       # noqa: E731
        f3 = lambda: K.conv3x3_bn_relu_bf16x3_gw(x, w3, sc, sh, out, B, hp, h, W, Cin, Cout, 1)    # noqa: E731
        t5, t3 = [], []
        for _ in range(args.repeats):              # alternate the two kernels: both see the same machine
            t5.append(timed(f5, args.warmup, args.iters, 1)[0])
            t3.append(timed(f3, args.warmup, args.iters, 1)[0])
        m5, m3 = statistics.median(t5), statistics.median(t3)
        px = B * hp * W
        r5, r3 = 6.0 * px * Cout * 25 * Cin / (m5 * 1e-3) / 1e12, 6.0 * px * Cout * 9 * Cin / (m3 * 1e-3) / 1e12
        res[f"layer{lvl + 1}"] = {"W": W, "Cin": Cin, "Cout": Cout, "conv5x5_ms": round(m5, 4), "conv3x3_gw_ms": round(m3, 4),
                                 "conv5x5_tflops": round(r5, 1), "conv3x3_gw_tflops": round(r3, 1), "rate_ratio": round(r5 / r3, 3)}
        print(f"block {lvl + 1} (W {W}, {Cin} -> {Cout}, {B} x {hp} rows): 5x5 {m5 * 1e3:.0f} us = {r5:.0f} TFLOP/s bf16 MFMA "
              f"(windows {min(t5) * 1e3:.0f} .. {max(t5) * 1e3:.0f}); 3x3 gw {m3 * 1e3:.0f} us = {r3:.0f} TFLOP/s "
              f"(windows {min(t3) * 1e3:.0f} .. {max(t3) * 1e3:.0f}); rate ratio 5x5 / 3x3 = {r5 / r3:.3f}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
