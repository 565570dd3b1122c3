"""Timing of the constrained searches (repetition and word constraints: csrc/logit_rules.hip, ac_trm_search_rules,
ac_trm_beam_step_rules) next to the unconstrained launch chain of the same process.

  python tools/logit_rules_bench.py [--out FILE] [--rounds 9]      (default FILE: profiles/logit_rules_bench.json)

64 clips (31 memory frames of 512 features), V = 4981, max_length 20, a decoder whose <end> row is zero, so that every
search runs its 20 steps.  Greedy: the unconstrained launch chain (mode="chain") against the search with all four rules on;
beam 3: the same pair.  The variants of a pair alternate inside every round (one process, interleaved), after three warm-up
searches each (the second captures the HIP graph); every search is timed with device events around the whole call, which
ends in the device-to-host copy of the token ids.  The figure is the median over the rounds.  The kernel alone:
ac_logit_rules_apply over 64 rows at V = 4981 from a plane of stride 20 * V into an aligned plane, 200 back-to-back launches
between two events, per launch.  Prints one JSON object."""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

B, TM, A_DIM, V, L = 64, 31, 512, 4981, 20
RULES = {"repetition_penalty": 1.3, "no_repeat_ngram_size": 2, "bad_words": [17, 250, 4000], "min_length": 6}


def one(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(variants, rounds):
    """{name: fn} -> {name: stats}: three warm-ups each, then ``rounds`` rounds that run every variant once, in turn."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(one(fn))
    return {k: {"ms": round(statistics.median(v), 3), "ms_per_step": round(statistics.median(v) / L, 4),
                "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "logit_rules_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    rounds = max(5, args.rounds)
    import audiocaption_amd as A
    from audiocaption_amd import _lib, build
    from audiocaption_amd import procedural as P
    build.build()
    st = P.decoder_state("", V, seed=500)
    st["classifier.weight"][2] = 0.0      # an <end> logit of 0 against a maximum near 4 never wins: 20 steps are decoded
    dec = A.TransformerDecoder(emb_dim=256, vocab_size=V, fc_emb_dim=512, attn_emb_dim=A_DIM, dropout=0.2)
    dec.load_state_dict(P.to_torch(st), strict=True)
    model = A.TransformerModel(torch.nn.Identity(), dec).eval().cuda()
    g = torch.Generator().manual_seed(3)
    enc = {"attn_emb": torch.randn(B, TM, A_DIM, generator=g).cuda(), "attn_emb_len": torch.full((B,), TM)}
    req = {"mode": "inference", "max_length": L}
    res = {"shape": {"clips": B, "memory_frames": TM, "vocab": V, "max_length": L, "rounds": rounds, "rules": RULES},
           "device": torch.cuda.get_device_name(0)}

    os.environ["AUDIOCAPTION_GREEDY"] = "chain"      # the yardstick of the issue: the same commit's launch chain
    free = model.forward_decoder(dict(req, sample_method="greedy"), enc)["seq"]
    ruled = model.forward_decoder(dict(req, sample_method="greedy", **RULES), enc)["seq"]
    assert int((free == 2).sum()) == 0 and int((ruled == 2).sum()) == 0, "the bench decoder emitted <end>"
    assert not torch.equal(free, ruled)
    res["greedy"] = interleaved({
        "chain": lambda: model.forward_decoder(dict(req, sample_method="greedy"), enc)["seq"],
        "constrained": lambda: model.forward_decoder(dict(req, sample_method="greedy", **RULES), enc)["seq"]}, rounds)
    res["beam3"] = interleaved({
        "chain": lambda: model.forward_decoder(dict(req, sample_method="beam", beam_size=3), enc)["seq"],
        "constrained": lambda: model.forward_decoder(dict(req, sample_method="beam", beam_size=3, **RULES), enc)["seq"]},
        rounds)
    for k in ("greedy", "beam3"):
        res[k]["constrained"]["x_chain"] = round(res[k]["constrained"]["ms"] / res[k]["chain"]["ms"], 3)

    # the kernel alone
    lib = _lib.load()
    src = torch.randn(B, L, V, device="cuda:0")
    dst = torch.empty(B, (V + 3) // 4 * 4, device="cuda:0")
    tok = torch.randint(3, 40, (B, L + 1), device="cuda:0", dtype=torch.int32)
    bad = torch.tensor(RULES["bad_words"], device="cuda:0", dtype=torch.int32)
    rs = _lib.AcLogitRules(RULES["repetition_penalty"], RULES["no_repeat_ngram_size"], RULES["min_length"], 2, len(bad),
                           bad.data_ptr())
    n = 200

    def burst(t):
        for _ in range(n):
            _lib.check(lib.ac_logit_rules_apply(ctypes.c_void_p(src.data_ptr() + 4 * t * V), L * V, _lib.ptr(dst), dst.shape[1],
                                                B, V, _lib.ptr(tok), L + 1, t, ctypes.byref(rs), _lib.stream()),
                       "ac_logit_rules_apply")
    kern = interleaved({"t4_aligned": lambda: burst(4), "t19_scalar": lambda: burst(19)}, rounds)
    res["kernel_alone_us_per_launch"] = {k: round(v["ms"] * 1000 / n, 2) for k, v in kern.items()}
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
