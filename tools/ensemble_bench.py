"""Timing of ensemble decoding (audiocaption_amd/ensemble.py, csrc/ensemble.hip) next to the single-model decode.

  python tools/ensemble_bench.py [--out FILE] [--reps 7]        (default FILE: profiles/ensemble_bench.json)

64 clips x 10 s (31 memory frames of 512 features), V = 4981, max_length 20, decoders whose <end> row is zero, so
that every search runs its 20 steps: M = 1, 2, 4 members, greedy and beam 3, in ms per search and per decode step.  In the
same run the single-model ``TransformerModel`` decode of the same shapes (launch-chain greedy, beam 3) is the yardstick:
the figure to quote is the ensemble step time as a multiple of the single-model step time of THIS run.

Every number is the median of ``--reps`` (>= 5) timed searches after three warm-up searches of the same shape (the
second of which captures the HIP graph), each timed with device events on the stream around the whole call; the call ends
in the device-to-host copy of the token ids, so the events bracket finished work.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, TM, A_DIM, V, L = 64, 31, 512, 4981, 20


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": round(statistics.median(ms), 3), "ms_per_step": round(statistics.median(ms) / L, 4),
            "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ensemble_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    reps = max(5, args.reps)
    import audiocaption_amd as A
    from audiocaption_amd import build
    from audiocaption_amd import procedural as P
    from audiocaption_amd.ensemble import EnsembleModel
    build.build()
    members = []
    for n in range(4):
        st = P.decoder_state("", V, seed=500 + n)
        st["classifier.weight"][2] = 0.0      # an <end> logit of 0 against a maximum near 4 never wins: 20 steps are decoded
        dec = A.TransformerDecoder(emb_dim=256, vocab_size=V, fc_emb_dim=512, attn_emb_dim=A_DIM, dropout=0.2)
        dec.load_state_dict(P.to_torch(st), strict=True)
        members.append(A.TransformerModel(torch.nn.Identity(), dec).eval().cuda())
    g = torch.Generator().manual_seed(3)
    encs = [{"attn_emb": torch.randn(B, TM, A_DIM, generator=g).cuda(), "attn_emb_len": torch.full((B,), TM)} for _ in range(4)]
    res = {"shape": {"clips": B, "memory_frames": TM, "vocab": V, "max_length": L, "reps": reps},
           "device": torch.cuda.get_device_name(0), "single_model": {}, "ensemble": {}}

    m0, e0 = members[0], encs[0]
    req = {"mode": "inference", "max_length": L}
    single_g = m0.decoder.greedy(e0["attn_emb"], e0["attn_emb_len"], L, 1, 2, 0, mode="chain")
    assert int((single_g["seq"] == 2).sum()) == 0, "the bench decoder emitted <end>"
    res["single_model"]["greedy_chain"] = timed(
        lambda: m0.decoder.greedy(e0["attn_emb"], e0["attn_emb_len"], L, 1, 2, 0, mode="chain")["seq"].cpu(), reps)
    res["single_model"]["beam3"] = timed(
        lambda: m0.forward_decoder(dict(req, sample_method="beam", beam_size=3), e0)["seq"], reps)
    for M in (1, 2, 4):
        ens = EnsembleModel(members[:M])
        row = {}
        for method, kw in (("greedy", {}), ("beam3", {"beam_size": 3})):
            sm = "beam" if method == "beam3" else "greedy"
            out = ens.decode(encs[:M], sample_method=sm, max_length=L, **kw)
            assert int((out["seq"][:, :L - 1] == 2).sum()) == 0
            row[method] = timed(lambda: ens.decode(encs[:M], sample_method=sm, max_length=L, **kw), reps)
        res["ensemble"][f"M{M}"] = row
    sg, sb = res["single_model"]["greedy_chain"]["ms"], res["single_model"]["beam3"]["ms"]
    for name, row in res["ensemble"].items():
        for method, r in row.items():
            r["x_single"] = round(r["ms"] / (sg if method == "greedy" else sb), 2)
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
