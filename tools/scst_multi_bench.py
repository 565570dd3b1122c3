"""Timing of multi-rollout self-critical sequence training against the single-rollout recipe, at the training shape bench.py
times: the Cnn14Rnn-Trm captioner (procedural weights, V 4981, model.train() with its configured dropout), 32 clips x 10 s
from the waveform, max_length 20, temp 1.0, the built-in device CIDEr-D over five references of 12 words per clip.

  python tools/scst_multi_bench.py [--out FILE] [--reps 9] [--rollouts 5]    (default FILE: profiles/scst_multi_bench.jsonl)

An iteration is ``ScstWrapper`` forward, ``loss.backward()``, ``clip_grad_norm_`` and ``FusedAdam.step()``.  Three
configurations, timed with device events (recorded on the stream before and after, read after a synchronise), three warm-up
rounds, then ``--reps`` (>= 5) rounds that alternate the three; the median is reported with the minimum and maximum.  One
JSON line per configuration, printed and appended to FILE:

  "scst_single"          one iteration of ScstWrapper(model): one sampled rollout, the greedy baseline decode, loss, backward;
  "scst_multi_mean"      one iteration of ScstWrapper(model, n_rollouts=K, baseline="mean"): K rollouts from one encoder pass;
  "scst_single_x_K"      K sequential "scst_single" iterations: the same number of sampled captions learnt from.

and the ratio of the last two."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, SECONDS, T, V, TEMP = 32, 10, 20, 4981, 1.0


class Vocabulary:
    class _Words:
        def __getitem__(self, i):
            return f"w{int(i)}"
    idx2word = _Words()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    return {"ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scst_multi_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--rollouts", type=int, default=5)
    args = ap.parse_args()
    reps, K = max(5, args.reps), args.rollouts
    import audiocaption_amd as A
    from audiocaption_amd import build
    from audiocaption_amd import procedural as P
    from audiocaption_amd.cider import Cider
    from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
    if not torch.cuda.is_available():
        raise SystemExit("scst_multi_bench: no ROCm device; nothing is measured without one")
    build.build()
    dev = "cuda"
    model = A.init_model_from_config(A.cnn14rnn_trm_config(V), print_fn=lambda s: None)
    model.load_state_dict(P.to_torch(P.cnn14rnn_trm_state(V)), strict=True)
    model = model.to(dev).train()
    single = A.ScstWrapper(model)
    multi = A.ScstWrapper(model, n_rollouts=K, baseline="mean")
    n = SECONDS * 32000
    wav = torch.from_numpy(P.synthetic_wav(B, n, seed=1)).to(dev)
    rng = np.random.default_rng(0)
    keys = [f"clip{i}" for i in range(B)]
    key2refs = {k: [" ".join(f"w{w}" for w in rng.integers(4, V, 12)) for _ in range(5)] for k in keys}
    batch = {"mode": "train", "wav": wav, "wav_len": [n] * B, "specaug": False, "max_length": T, "temp": TEMP, "keys": keys,
             "key2refs": key2refs, "vocabulary": Vocabulary(), "scorer": Cider()}
    params = [p for p in single.parameters() if p.requires_grad]
    opt = FusedAdam(params, lr=5e-5, weight_decay=1e-6)

    def iteration(wrapper):
        opt.zero_grad()
        out = wrapper(batch)
        out["loss"].backward()
        clip_grad_norm_(params, 1.0)
        opt.step()

    def k_singles():
        for _ in range(K):
            iteration(single)

    configs = (("scst_single", lambda: iteration(single)), ("scst_multi_mean", lambda: iteration(multi)),
               ("scst_single_x_K", k_singles))
    for _ in range(3):
        for _, fn in configs:
            fn()
    times = {name: [] for name, _ in configs}
    for _ in range(reps):
        for name, fn in configs:
            times[name].append(timed(fn))
    common = {"device": torch.cuda.get_device_name(0), "clips": B, "seconds": SECONDS, "max_length": T, "vocab": V,
              "temp": TEMP, "rollouts": K, "timer": "device events"}
    lines = [dict(common, config=name, **summary(times[name])) for name, _ in configs]
    lines[1]["ratio_multi_over_K_singles"] = round(lines[1]["ms"] / lines[2]["ms"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
