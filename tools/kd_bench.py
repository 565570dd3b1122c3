"""Development probe: what token-level distillation adds to a training iteration at the benchmark's training shape
(32 clips x 10 s, captions of 22 tokens, V 4981).  Three per-iteration figures, each over replayed graphs:
the plain label-smoothing step (``TrainEngine.step``), the same step with ``kd=`` (ac_kd_loss in the place of
ac_label_smoothing_loss, teacher logits copied into their static buffer), and the teacher's eval-mode forward
(``teacher(input_dict)`` with mode "train", as run_kd.py:42 calls it) that produces those logits."""
import argparse
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import audiocaption_amd as A
from audiocaption_amd import procedural as Pr
from audiocaption_amd.optim import FusedAdam
from audiocaption_amd.train import TrainEngine

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--cap-len", type=int, default=22)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--vocab", type=int, default=4981)
ap.add_argument("--temp", type=float, default=2.0)
ap.add_argument("--sup-weight", type=float, default=0.5)
args = ap.parse_args()

B, L = args.batch, int(args.seconds * 32000)


def make(state):
    model = A.init_model_from_config(A.cnn14rnn_trm_config(args.vocab), print_fn=lambda s: None)
    model.load_state_dict(Pr.to_torch(state), strict=True)
    return model.to("cuda:0")


state = Pr.cnn14rnn_trm_state(args.vocab)
student = make(state).train()
tstate = dict(state)
tstate.update(Pr.decoder_state_diverse("greedy", vocab_size=args.vocab))     # a teacher with other decoder weights
teacher = make(tstate).eval()
wav = torch.from_numpy(Pr.synthetic_wav(B, L, seed=1)).cuda()
g = torch.Generator().manual_seed(0)
cap = torch.randint(4, args.vocab, (B, args.cap_len), generator=g)
cap[:, 0], cap[:, -1] = 1, 2
batch = {"mode": "train", "wav": wav, "wav_len": [L] * B, "specaug": False, "cap": cap.cuda(),
         "cap_len": np.array([args.cap_len] * B), "ss_ratio": 0.85}
eng = TrainEngine(student)
opt = FusedAdam([p for p in student.parameters() if p.requires_grad], lr=5e-4, weight_decay=1e-6)
with torch.no_grad():
    tl = teacher(batch)["logit"]


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / args.steps


def teacher_forward():
    with torch.no_grad():
        return teacher(batch)["logit"]


random.seed(0)
kd = {"tchr_logit": tl, "temp": args.temp, "sup_weight": args.sup_weight}
plain = timed(lambda: eng.step(batch, opt))
with_kd = timed(lambda: eng.step(batch, opt, kd=kd))
fwd = timed(teacher_forward)
r = eng.step(batch, opt, kd=kd)
print(f"B={B} seconds={args.seconds:g} cap_len={args.cap_len} V={args.vocab} temp={args.temp:g} sup_weight={args.sup_weight:g}: "
      f"step {plain:.2f} ms, step with kd {with_kd:.2f} ms (+{with_kd - plain:.2f}), teacher forward {fwd:.2f} ms; "
      f"a distillation iteration {with_kd + fwd:.2f} ms ({B / (with_kd + fwd) * 1e3:.0f} clips/s); "
      f"loss {float(r['loss']):.4f} = {args.sup_weight:g} x {float(r['sup_loss']):.4f} + {1 - args.sup_weight:g} x "
      f"{float(r['kd_loss']):.4f}")
