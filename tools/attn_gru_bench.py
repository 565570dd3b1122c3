"""Timing of the attention-GRU caption decoder (csrc/attn_gru.hip, audiocaption_amd/attn_model.py) with encoder outputs
fed directly.

  python tools/attn_gru_bench.py [--out FILE] [--reps 7]        (default FILE: profiles/attn_gru_bench.json)

The published shape (E = d = attn_size = attn_emb_dim = fc_emb_dim = 512, V = 4981), 64 clips x 31 memory frames,
max_length 20, a decoder whose <end> row is zero so that every search runs its 20 steps: greedy (64 rows) and beam 3 (192
rows), in ms per search, ms per decode step and clips/s.  Every number is the median of ``--reps`` (>= 5) timed searches
after three warm-up searches of the same shape, each timed with device events around the whole call; the call ends in the
device-to-host copy of the token ids, so the events bracket finished work.

Also reported: the CPU restatement (tests/_attn_gru_ref.py, torch on the host's cores) on the same inputs, in clips/s, and
the fraction of the weight-read floor a step reaches - the 5.43 M weights one step reads (21.7 MB: W_h, ctx_proj,
W_ih[:, :2E], W_hh, the classifier) once per step at the 8.0 TB/s HBM peak, over the measured step time.  A whole-search
time over that floor is an end-to-end figure (launch gaps, attention and picks included), not a kernel's share of peak.
Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

B, TM, DIM, V, L = 64, 31, 512, 4981, 20
HBM_PEAK = 8.0e12


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
    med = statistics.median(ms)
    return {"ms": round(med, 3), "ms_per_step": round(med / L, 4), "clips_per_s": round(B / med * 1e3, 1),
            "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attn_gru_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    reps = max(5, args.reps)
    import audiocaption_amd as A
    from audiocaption_amd import build
    from audiocaption_amd import procedural as P
    import _attn_gru_ref as R
    build.build()
    st = P.bah_decoder_state(vocab_size=V, seed=700)
    st["classifier.weight"][2] = 0.0      # an <end> logit near 0 against a maximum of several units never wins
    st["classifier.bias"][2] = -1.0
    sd = P.to_torch(st)
    dec = A.TemporalBahAttnDecoder(emb_dim=DIM, vocab_size=V, fc_emb_dim=DIM, attn_emb_dim=DIM, dropout=0.5, d_model=DIM,
                                   attn_size=DIM)
    dec.load_state_dict(sd, strict=True)
    model = A.TemporalSeq2SeqAttnModel(torch.nn.Identity(), dec).eval().cuda()
    g = torch.Generator().manual_seed(3)
    mem = torch.randn(B, TM, DIM, generator=g) * 0.25
    lens, tags = torch.full((B,), TM), torch.arange(B) % 4
    req = {"mode": "inference", "max_length": L, "attn_emb": mem.cuda(), "fc_emb": mem.mean(1).cuda(), "attn_emb_len": lens,
           "temporal_tag": tags}
    weights = DIM * DIM * 2 + 3 * DIM * 2 * DIM + 3 * DIM * DIM + V * DIM
    floor_ms = weights * 4 / HBM_PEAK * 1e3
    res = {"shape": {"clips": B, "memory_frames": TM, "dim": DIM, "vocab": V, "max_length": L, "reps": reps},
           "device": torch.cuda.get_device_name(0), "weight_floats_per_step": weights,
           "weight_floor_ms_per_step": round(floor_ms, 5)}
    with torch.no_grad():
        for name, kw in (("greedy", {}), ("beam3", {"sample_method": "beam", "beam_size": 3})):
            out = model(dict(req, **kw))
            assert int((out["seq"][:, :L - 1] == 2).sum()) == 0, "the bench decoder emitted <end>"
            r = timed(lambda: model(dict(req, **kw))["seq"], reps)
            r["fraction_of_weight_floor"] = round(floor_ms / r["ms_per_step"], 4)
            res[name] = r
        torch.set_num_threads(min(16, torch.get_num_threads()))
        t0 = time.perf_counter()
        cpu = R.greedy(sd, mem, lens, mem.mean(1), tags, L)
        dt = time.perf_counter() - t0
        assert cpu["steps"] == L
        res["cpu_restatement_greedy"] = {"s": round(dt, 3), "clips_per_s": round(B / dt, 1), "threads": torch.get_num_threads()}
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
