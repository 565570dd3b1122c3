"""Timing of a group (diverse) beam search (TransformerModel.group_beam_search: csrc/group_beam.hip between
ac_trm_step_logits and ac_trm_beam_update_all) next to the plain beam search of the same total beam_size, same process.

  python tools/group_beam_bench.py [--out FILE] [--rounds 9]      (default FILE: profiles/group_beam_bench.json)

64 clips (31 memory frames of 512 features), V = 4981, max_length 20, beam_size 6, a decoder whose <end> row is zero, so that
no beam ever ends before the last step and the plain search runs its 20 steps (it has no clip to retire) - the group search
never exits early anyway.  Group search: group_size 3 (three groups of two beams), diversity_lambda 0.5.  Both searches
replayed from their HIP graphs (the default from the second use of a shape on) and eager (AUDIOCAPTION_DECODE_GRAPH=0, the
host launching every kernel); the variants of a pair alternate inside every round after three warm-up searches each, every
search timed with device events around the whole call, which ends in the device-to-host copies of the ranking.  The figure
is the median over the rounds; ``x_plain`` is group over plain.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

B, TM, A_DIM, V, L, BEAM, G, LAMBDA = 64, 31, 512, 4981, 20, 6, 3, 0.5


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
    return {k: {"ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "group_beam_bench.json"))
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    rounds = max(5, args.rounds)
    import audiocaption_amd as A
    from audiocaption_amd import build, search_state
    from audiocaption_amd import procedural as P
    build.build()
    st = P.decoder_state("", V, seed=500)
    st["classifier.weight"][2] = 0.0      # an <end> logit of 0 against a maximum near 4 never wins: 20 steps are decoded
    dec = A.TransformerDecoder(emb_dim=256, vocab_size=V, fc_emb_dim=512, attn_emb_dim=A_DIM, dropout=0.2)
    dec.load_state_dict(P.to_torch(st), strict=True)
    model = A.TransformerModel(torch.nn.Identity(), dec).eval().cuda()
    g = torch.Generator().manual_seed(3)
    enc = {"attn_emb": torch.randn(B, TM, A_DIM, generator=g).cuda(), "attn_emb_len": torch.full((B,), TM)}
    req = {"mode": "inference", "sample_method": "beam", "beam_size": BEAM, "max_length": L}
    variants = {"plain": lambda: model.forward_decoder(dict(req), enc)["seq"],
                "group": lambda: model.forward_decoder(dict(req, group_size=G, diversity_lambda=LAMBDA), enc)["seq"]}
    res = {"shape": {"clips": B, "memory_frames": TM, "vocab": V, "max_length": L, "beam_size": BEAM, "group_size": G,
                     "diversity_lambda": LAMBDA, "rounds": rounds,
                     "group_steps": len(search_state.group_steps(G, L)), "global_steps": L + G - 1},
           "device": torch.cuda.get_device_name(0)}
    plain, group = variants["plain"](), variants["group"]()
    assert int((plain == 2).sum()) == 0 and int((group == 2).sum()) == 0, "the bench decoder emitted <end>"
    assert tuple(group.shape) == (B, BEAM, L) and not torch.equal(group[:, 0], group[:, 2])
    for mode, flag in (("replayed", "1"), ("eager", "0")):
        os.environ["AUDIOCAPTION_DECODE_GRAPH"] = flag
        res[mode] = interleaved(variants, rounds)
        res[mode]["x_plain"] = round(res[mode]["group"]["ms"] / res[mode]["plain"]["ms"], 3)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
