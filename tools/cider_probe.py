"""Development probe: what the SCST reward costs.  One ScstWrapper training forward (greedy baseline, sampled rollout,
reward, loss; no backward) on a synthetic AudioCaps-shape batch, timed under three scorers:

  constant  every sentence scores the same: the step without any scoring
  host      the float64 restatement of CIDEr-D (tests/_cider_ref.py) as a host scorer: two downloads, strings, two
            dictionary passes in the interpreter, one upload
  device    audiocaption_amd.Cider(): the reward computed on the device from the word ids (csrc/cider.hip)

Each forward ends in a device synchronisation; the figure is the median of --runs forwards after --warmup, the three
conditions taken in turn within every round.  ``--only device`` runs one condition alone (for a kernel trace:
rocprofv3 --kernel-trace --stats -- python tools/cider_probe.py --only device)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [_ROOT, os.path.join(_ROOT, "tests")]

import audiocaption_amd as A
from audiocaption_amd import procedural as Pr

import _cider_ref

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--max-length", type=int, default=20)
ap.add_argument("--refs", type=int, default=5)
ap.add_argument("--ref-words", type=int, default=12)
ap.add_argument("--vocab", type=int, default=4981)
ap.add_argument("--runs", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only", choices=("constant", "host", "device"))
args = ap.parse_args()


class Vocabulary:
    class _Words:
        def __getitem__(self, i):
            return f"w{int(i)}"
    idx2word = _Words()


class ConstantScorer:
    def compute_score(self, references, hypothesis):
        return 0.5, [0.5] * len(references)


B, L, T = args.batch, int(args.seconds * 32000), args.max_length
model = A.init_model_from_config(A.cnn14rnn_trm_config(args.vocab), print_fn=lambda s: None)
model.load_state_dict(Pr.to_torch(Pr.cnn14rnn_trm_state(args.vocab)), strict=True)
wrapper = A.ScstWrapper(model.to("cuda:0")).train()
rng = np.random.default_rng(0)
keys = [f"clip{i}" for i in range(B)]
key2refs = {k: [" ".join(f"w{w}" for w in rng.integers(4, args.vocab, args.ref_words)) for _ in range(args.refs)] for k in keys}
batch = {"mode": "train", "wav": torch.from_numpy(Pr.synthetic_wav(B, L, seed=1)).cuda(), "wav_len": [L] * B, "specaug": False,
         "max_length": T, "temp": 1.0, "keys": keys, "key2refs": key2refs, "vocabulary": Vocabulary(), "seed": 3,
         "dropout_seed": 3}
scorers = {"constant": ConstantScorer(), "host": _cider_ref.Scorer(), "device": A.Cider()}
if args.only:
    scorers = {args.only: scorers[args.only]}


def forward(scorer):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = wrapper(dict(batch, scorer=scorer))
    torch.cuda.synchronize()
    model._train_engine._saved = None
    return time.perf_counter() - t0, out


times = {name: [] for name in scorers}
for r in range(args.warmup + args.runs):
    for name, scorer in scorers.items():
        dt, out = forward(scorer)
        if r >= args.warmup:
            times[name].append(dt)
med = {name: statistics.median(v) for name, v in times.items()}
for name, v in times.items():
    print(f"{name:9s} median {1e3 * med[name]:8.3f} ms  (min {1e3 * min(v):.3f}, max {1e3 * max(v):.3f}, {len(v)} runs)")
if len(med) == 3:
    print(f"B={B} seconds={args.seconds:g} max_length={T} refs={args.refs}x{args.ref_words} words: host scorer adds "
          f"{1e3 * (med['host'] - med['constant']):.3f} ms, device scorer adds {1e3 * (med['device'] - med['constant']):.3f} ms")
