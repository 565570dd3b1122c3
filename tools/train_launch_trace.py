"""Development probe: the launch trace of eager training steps (TrainEngine.step, use_graph=False) on the synthetic
batch of tools/train_bench.py - every call into the HIP library in issue order, with its arguments, plus the side
stream's fork / join points.  Two versions of train.py that print the same SHA-256 issue the same launches, in the same
order, on the same streams, with the same arguments: the check for a restatement of the step that must change nothing.

Pointer arguments (device addresses, the stream handle) are written as the ordinal of their first appearance in the
trace, NULL as None; integers and floats are written exactly.  The frozen Cnn14 is launched through
audiocaption_amd.kernels, not through the engine's library handle, and is not part of the trace."""
import argparse
import hashlib
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import audiocaption_amd as A
from audiocaption_amd import procedural as Pr, train
from audiocaption_amd.optim import FusedAdam
from audiocaption_amd.train import TrainEngine
from launch_trace import TracingLib, ordinals, pointer, trace

ap = argparse.ArgumentParser()
ap.add_argument("--encoder", choices=("rnn", "trm"), default="rnn")
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--cap-len", type=int, default=22)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--vocab", type=int, default=4981)
ap.add_argument("--ss-ratio", type=float, nargs="+", default=[1.0, 0.85, 0.85],
                help="scheduled-sampling ratio of each traced step (1.0 = teacher forced)")
ap.add_argument("--out", default="train_launch_trace.txt")
args = ap.parse_args()

B, L = args.batch, int(args.seconds * 32000)
if args.encoder == "trm":
    cfg, state = A.config.cnn14trm_trm_config(args.vocab), Pr.cnn14trm_trm_state(args.vocab)
else:
    cfg, state = A.cnn14rnn_trm_config(args.vocab), Pr.cnn14rnn_trm_state(args.vocab)
model = A.init_model_from_config(cfg, print_fn=lambda s: None)
model.load_state_dict(Pr.to_torch(state), strict=True)
model = model.to("cuda:0").train()
wav = torch.from_numpy(Pr.synthetic_wav(B, L, seed=1)).cuda()
cap = torch.randint(4, args.vocab, (B, args.cap_len), generator=torch.Generator().manual_seed(0))
cap[:, 0], cap[:, -1] = 1, 2
batch = {"mode": "train", "wav": wav, "wav_len": [L] * B, "specaug": False, "cap": cap.cuda(),
         "cap_len": np.array([args.cap_len] * B)}

_fork, _join = train._SideStream.fork, train._SideStream.join


def fork(self):
    h = _fork(self)
    trace.append(f"fork -> {pointer(h)}")
    return h


def join(self):
    trace.append(f"join waits={bool(self.dirty)}")
    return _join(self)


train._SideStream.fork, train._SideStream.join = fork, join

eng = TrainEngine(model)
eng.lib = TracingLib(eng.lib)
opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=5e-4, weight_decay=1e-6)
random.seed(0)
for i, ss in enumerate(args.ss_ratio):
    trace.append(f"# step {i} ss_ratio={ss!r}")
    r = eng.step(dict(batch, ss_ratio=ss), opt, use_graph=False)
torch.cuda.synchronize()
text = "\n".join(trace) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(f"encoder={args.encoder} B={B} seconds={args.seconds:g} cap_len={args.cap_len} ss_ratio={args.ss_ratio}: "
      f"{len(trace)} records, {len(ordinals)} addresses, sha256 {hashlib.sha256(text.encode()).hexdigest()}, "
      f"loss {float(r['loss']):.4f} -> {args.out}")
