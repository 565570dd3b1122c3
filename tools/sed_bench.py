"""Timing of the sound-event tagger (audiocaption_amd/sed_model.py, csrc/sed.hip) on one MI355X.

  python tools/sed_bench.py [--out FILE] [--reps 7] [--clips 64] [--seconds 10]     (default FILE: profiles/sed_bench.json)

64 clips x 10 s at 32 kHz (1001 frames, 250 segments, 447 classes), procedural weights.  Two kinds of figures:

  * ``forward_wav_ms``: the product call (log-mel -> tags on the device) plus the read-back of the B tags, device events
    around the whole call, median of ``--reps`` (>= 5) after three warm-up calls; next to it ``cnn14_encode_ms``,
    ``Cnn14Encoder.encode`` on the same batch, timed the same way (the tagger's cost relative to the captioner's encoder);
  * ``stages_ms``: the same call with a pair of device events around every launch of a stage, summed per stage - the log-mel,
    the eight conv launches, the four pool passes, fc1 + GRU projections + fc_audioset (``linear``), the GRU recurrence,
    the head, the tag kernels and the read-back (host clock around ``.tolist()`` after a synchronise).  The events sit in
    the stream between the launches, so the stages add up to a little more than the undisturbed call.

``conv_gflop`` counts the 3x3 products of the eight convs from the layer shapes (2 * 9 * Cin * Cout per output pixel over
the valid rows); ``conv_tflops`` is that over the conv stage's time - an end-to-end rate of the stage, launch gaps included,
not a kernel's share of peak.  ``vs_wino1d``: the timed batch once more on the F(2,3) tier - largest difference of the class
logits and whether the tags agree (the results of the route that is timed, checked at the size that is timed).  The pool
passes' share is what a fused avg + max conv epilogue could save.  Prints one JSON
object."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402


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
    return {"ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


class Stages:
    """Device events around every call of the wrapped functions, summed per stage after a synchronise."""

    def __init__(self):
        self.events = []

    def wrap(self, stage, fn):
        def wrapped(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.events.append((stage, e0, e1))
            return out
        return wrapped

    def totals(self):
        torch.cuda.synchronize()
        out, launches = {}, {}
        for stage, e0, e1 in self.events:
            out[stage] = out.get(stage, 0.0) + e0.elapsed_time(e1)
            launches[stage] = launches.get(stage, 0) + 1
        self.events = []
        return out, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sed_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    args = ap.parse_args()
    reps = max(5, args.reps)
    import audiocaption_amd as A
    from audiocaption_amd import build, kernels as K, procedural as P, sed_model as S
    build.build()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sed_bench.py measures on the GPU; there is none here")
    B, L = args.clips, int(args.seconds * 32000)
    tagger = A.Cnn8rnnSedModel(447)
    tagger.load_state_dict(P.to_torch(P.sed_state()), strict=True)
    tagger = tagger.cuda().eval()
    cnn14 = A.Cnn14Encoder()
    cnn14.load_state_dict(P.to_torch(P.cnn14_state()), strict=True)
    cnn14 = cnn14.cuda().eval()
    wav = torch.from_numpy(P.synthetic_wav(B, L, varied=True)).cuda()
    T = L // tagger.hop_length + 1
    H, Hp = tagger.geometry(T)
    gflop = sum(2 * 9 * cin * cout * B * H[lvl] * W for cin, cout, lvl, W in
                ((1, 64, 0, 64), (64, 64, 0, 64), (64, 128, 1, 32), (128, 128, 1, 32), (128, 256, 2, 16), (256, 256, 2, 16),
                 (256, 512, 2, 8), (512, 512, 2, 8))) / 1e9
    res = {"shape": {"clips": B, "samples": L, "frames": T, "segments": T // 4, "classes": 447, "rows_per_clip": Hp,
                     "reps": reps}, "device": torch.cuda.get_device_name(0), "conv_algo": tagger.effective_algo(),
           "conv_gflop": round(gflop, 1)}
    with torch.no_grad():
        res["forward_wav_ms"] = timed(lambda: tagger.forward_wav(wav).tolist(), reps)
        res["cnn14_encode_ms"] = timed(lambda: cnn14.encode(wav).sum().item(), reps)
        tags = tagger.forward_wav(wav).tolist()
        res["tags_histogram"] = [tags.count(t) for t in range(4)]
        # the timed route against the F(2,3) tier on the same batch: same tags, class logits within the tiers' error
        pre = tagger.last_preact.clone()
        tagger.conv_algo, timed_algo = "wino1d", tagger.conv_algo
        tags_f23 = tagger.forward_wav(wav).tolist()
        res["vs_wino1d"] = {"max_preact_diff": float((tagger.last_preact - pre).abs().max()), "max_abs_preact": float(pre.abs().max()),
                            "tags_equal": tags_f23 == tags}
        tagger.conv_algo = timed_algo

        # ---- per stage: events around every launch ----
        st = Stages()
        real = {n: getattr(K, n) for n in ("logmel", "conv3x3_first", "pool_avgmax", "linear", "gru_layer", "sed_head",
                                           "sed_temporal_tag")}
        real_tier = S.conv_tier
        stage_of = {"logmel": "logmel", "conv3x3_first": "conv", "pool_avgmax": "pool", "linear": "linear", "gru_layer": "gru",
                    "sed_head": "head", "sed_temporal_tag": "tag"}
        try:
            for n, fn in real.items():
                setattr(K, n, st.wrap(stage_of[n], fn))
            S.conv_tier = lambda algo: dataclasses.replace(real_tier(algo), launch=st.wrap("conv", real_tier(algo).launch))
            runs, back = [], []
            for i in range(3 + reps):
                dev_tags = tagger.forward_wav(wav)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                dev_tags.tolist()
                dt = (time.perf_counter() - t0) * 1e3
                tot, launches = st.totals()
                if i >= 3:
                    runs.append(tot)
                    back.append(dt)
        finally:
            for n, fn in real.items():
                setattr(K, n, fn)
            S.conv_tier = real_tier
        stages = {k: round(statistics.median(r[k] for r in runs), 3) for k in runs[0]}
        stages["read_back"] = round(statistics.median(back), 3)
        res["stages_ms"] = stages
        res["stage_launch_calls"] = launches
        total = sum(stages.values())
        res["stage_share"] = {k: round(v / total, 4) for k, v in stages.items()}
        res["conv_tflops"] = round(gflop / stages["conv"], 2)
        res["tagger_over_cnn14_encode"] = round(res["forward_wav_ms"]["ms"] / res["cnn14_encode_ms"]["ms"], 3)
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
