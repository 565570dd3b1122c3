"""Timing of on-device caption sampling (csrc/sample.hip) next to greedy decoding.

  python tools/sample_bench.py [--out FILE]

1. ac_sample_rows alone at 64 and 768 rows of V = 4981 logits for plain ("sample"), top-50 and top-0.9 sampling (HIP
   events around 200 back-to-back launches).  greedy_pick_kernel has no entry point of its own: its time per launch comes
   from a kernel trace of part 2 (rocprofv3 --kernel-trace --stats), as does the sampler's inside the chain.
2. The whole chain-route decode of 64 clips x 10 s (31 memory frames, max_length 20, HIP-graph replay): ac_trm_greedy
   against ac_trm_sample per method, median over replays.  Prints one JSON object.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

METHODS = [("sample", 1.0), ("top50", 1.0), ("top0.9", 1.0)]


def rows_bench(lib, R, V=4981, iters=200):
    from audiocaption_amd import _lib
    from audiocaption_amd import sampling as SM
    g = torch.Generator().manual_seed(R)
    x = (torch.randn(R, V, generator=g) * 3.0).cuda()
    word = torch.empty(R, device="cuda", dtype=torch.int32)
    lp = torch.empty(R, device="cuda", dtype=torch.float32)
    seed = torch.tensor([12345], device="cuda", dtype=torch.int64)
    res = {}
    for name, temp in METHODS:
        code, k, p, t = SM.parse_sample_method(name, V, temp)

        def launch(step):
            _lib.check(lib.ac_sample_rows(_lib.ptr(x), V, R, V, code, k, p, t, _lib.ptr(seed), step, _lib.ptr(word),
                                          _lib.ptr(lp), _lib.stream()), "ac_sample_rows")
        for s in range(20):
            launch(s)
        torch.cuda.synchronize()
        times = []
        for rep in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for s in range(iters):
                launch(s)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3 / iters)
        res[name] = round(statistics.median(times), 2)
    return res


def decode_bench(reps=30):
    import audiocaption_amd as A
    from audiocaption_amd import procedural as P
    from audiocaption_amd import sampling as SM
    V = 4981
    st = P.to_torch(P.decoder_state_diverse("greedy", vocab_size=V))
    dec = A.TransformerDecoder(emb_dim=256, vocab_size=V, fc_emb_dim=512, attn_emb_dim=512, dropout=0.2, nlayers=2)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in st.items()}, strict=True)
    dec = dec.eval().cuda()
    g = np.load(os.path.join(REPO, "tests", "golden", "g4_greedy.npz"))
    emb = torch.from_numpy(g["attn_emb"])
    emb = torch.cat([torch.roll(emb[i % 4:i % 4 + 1], i // 4, dims=1) for i in range(64)]).cuda()   # 64 x 10 s clips
    lens = torch.full((64,), emb.shape[1], dtype=torch.int64)

    def timed(fn):
        for _ in range(3):      # plain launches, capture, replay
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        return round(statistics.median(times), 1)

    res = {"greedy_chain": timed(lambda: dec.greedy(emb, lens, 20, 1, 2, 0, mode="chain"))}
    for name, temp in METHODS:
        code, k, p, t = SM.parse_sample_method(name, V, temp)
        res[name] = timed(lambda: dec.sample(emb, lens, 20, 1, 2, 0, code, k, p, t, 777))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    out = {"device": torch.cuda.get_device_name(0),
           "sample_rows_us": {str(R): rows_bench(lib, R) for R in (64, 768)},
           "decode_64x10s_20steps_us": decode_bench()}
    d = out["decode_64x10s_20steps_us"]
    out["decode_ratio_vs_greedy_chain"] = {k: round(v / d["greedy_chain"], 3) for k, v in d.items() if k != "greedy_chain"}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
