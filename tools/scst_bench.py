"""Development probe: time of one self-critical sequence training iteration (ScstWrapper, then loss.backward(), clip,
FusedAdam) on a synthetic AudioCaps-shape batch, and its split into greedy baseline, sampled rollout, host reward and
backward + update (each part timed with a device synchronisation after it).  The number to compare it with is the
cross-entropy iteration of the same commit (tools/train_bench.py).  The scorer is a unigram-overlap stand-in (a CIDEr scorer
is the caller's object; its host time comes on top)."""
import argparse
import time

import numpy as np
import torch

import audiocaption_amd as A
from audiocaption_amd import procedural as Pr
from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
from audiocaption_amd.rl_model import compute_batch_score, scst_loss
from audiocaption_amd.train import _TrainBridge

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--max-length", type=int, default=20)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--vocab", type=int, default=4981)
ap.add_argument("--temp", type=float, default=1.0)
ap.add_argument("--encoder", choices=("rnn", "trm"), default="rnn")
args = ap.parse_args()


class Vocabulary:
    class _Words:
        def __getitem__(self, i):
            return f"w{int(i)}"
    idx2word = _Words()


class OverlapScorer:
    def compute_score(self, references, hypothesis):
        scores = []
        for key, refs in references.items():
            words = hypothesis[key][0].split()
            known = set(w for r in refs for w in r.split())
            scores.append(sum(w in known for w in words) / len(words) if words else 0.0)
        return float(np.mean(scores)), scores


B, L, T = args.batch, int(args.seconds * 32000), args.max_length
if args.encoder == "trm":
    cfg, state = A.config.cnn14trm_trm_config(args.vocab), Pr.cnn14trm_trm_state(args.vocab)
else:
    cfg, state = A.cnn14rnn_trm_config(args.vocab), Pr.cnn14rnn_trm_state(args.vocab)
model = A.init_model_from_config(cfg, print_fn=lambda s: None)
model.load_state_dict(Pr.to_torch(state), strict=True)
wrapper = A.ScstWrapper(model.to("cuda:0")).train()
rng = np.random.default_rng(0)
keys = [f"clip{i}" for i in range(B)]
key2refs = {k: [" ".join(f"w{w}" for w in rng.integers(4, args.vocab, 12)) for _ in range(5)] for k in keys}
batch = {"mode": "train", "wav": torch.from_numpy(Pr.synthetic_wav(B, L, seed=1)).cuda(), "wav_len": [L] * B, "specaug": False,
         "max_length": T, "temp": args.temp, "keys": keys, "key2refs": key2refs, "vocabulary": Vocabulary(),
         "scorer": OverlapScorer()}
params = [p for p in wrapper.parameters() if p.requires_grad]
opt = FusedAdam(params, lr=5e-4, weight_decay=1e-6)


def iteration():
    opt.zero_grad()
    out = wrapper(batch)
    out["loss"].backward()
    clip = clip_grad_norm_(params, 1.0)
    opt.step()
    return out


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


for _ in range(3):
    out = iteration()
t0 = sync()
for _ in range(args.steps):
    out = iteration()
whole = (sync() - t0) / args.steps

# the same iteration piece by piece (ScstWrapper.scst's own sequence)
eng = model._train_engine
parts = {"baseline": 0.0, "rollout": 0.0, "reward": 0.0, "backward+update": 0.0}
for _ in range(args.steps):
    opt.zero_grad()
    t0 = sync()
    greedy = wrapper._baseline(batch, T)[0].cpu()
    t1 = sync()
    model.train()
    ro = eng.rollout(batch)
    sampled = ro["seq"].cpu()
    t2 = sync()
    score = [compute_batch_score(s.numpy(), key2refs, keys, model.start_idx, model.end_idx, batch["vocabulary"],
                                 batch["scorer"]) for s in (sampled, greedy)]
    reward = torch.from_numpy((score[0] - score[1]).astype(np.float32)).cuda()
    t3 = sync()
    logit = _TrainBridge.apply(eng, ro["logit"], *eng.flat.params)
    scst_loss(logit, ro["seq_i32"], reward, args.temp, model.end_idx).backward()
    clip_grad_norm_(params, 1.0)
    opt.step()
    t4 = sync()
    for k, dt in zip(parts, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
        parts[k] += dt / args.steps

print(f"encoder={args.encoder} B={B} seconds={args.seconds:g} max_length={T}: {1e3 * whole:.2f} ms/iteration "
      f"({B / whole:.0f} clips/s), loss {float(out['loss'].detach()):.4f}, mean reward {float(out['reward'].mean()):.4f}")
print("split: " + ", ".join(f"{k} {1e3 * v:.2f} ms" for k, v in parts.items()) + f" (sum {1e3 * sum(parts.values()):.2f} ms)")
