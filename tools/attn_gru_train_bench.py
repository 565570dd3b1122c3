"""Timing of one training forward + backward of the attention-GRU captioner on the HIP path (Seq2SeqAttnModel.forward with
mode="train" through train_attn_gru.AttnGruTrainEngine, LabelSmoothingLoss, loss.backward()).

  python tools/attn_gru_train_bench.py [--out FILE] [--reps 9]     (default FILE: profiles/attn_gru_train_bench.jsonl)

The model of case 2 of tests/golden/make_golden_attn_gru_train.py (frozen Cnn14 + 3-layer bi-GRU + TemporalBahAttnDecoder
at E = d = S = A = F = 512, V 4981) with every dropout p = 0, 32 clips x 10 s (31 Cnn14 frames), captions of 21 tokens
(T = 20 steps), ss_ratio 0.7 with one fixed set of coins.  Three timed configurations, each with device events around the
whole forward + loss + backward (the forward ends in the device-to-host copy of ``seq``, the backward is followed by the
second event, so the events bracket finished work), three warm-up iterations of the same shape, ``--reps`` (>= 5) timed
iterations, the median reported with the minimum and maximum:

  "hip_from_wav"   the whole model from the waveform (the frozen Cnn14 included);
  "hip_from_cnn"   the same downstream of a preset Cnn14 output (the ``_cnn_attn`` hook): GRU encoder + decoder;
  "torch_from_cnn" the restatement of tests/_attn_gru_train_ref.py run with torch on the same device on the same preset
                   Cnn14 output - the only other implementation that exists on the machine.

"hip_from_cnn" and "torch_from_cnn" are timed alternately in one loop.  The logits and arg-max words of the two are compared
before anything is timed and the gap is reported.  Also printed: the launches one decoder step issues (counted from csrc/attn_gru_train.hip's chain:
8 forward, 6 backward) and the decoder chain's launches per iteration.  Prints one JSON line per configuration and
appends them to FILE."""
import argparse
import json
import os
import random
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

B, SECONDS, TC, V = 32, 10, 21, 4981
FWD_LAUNCHES_PER_STEP, BWD_LAUNCHES_PER_STEP = 8, 6


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    return {"ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attn_gru_train_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    reps = max(5, args.reps)
    import audiocaption_amd as A
    from audiocaption_amd import build
    from audiocaption_amd import procedural as P
    from audiocaption_amd.loss import LabelSmoothingLoss
    import _attn_gru_train_ref as R
    build.build()
    dev = "cuda"
    cfg = A.cnn14rnn_trm_config(V)
    cfg["encoder"]["rnn"]["args"]["dropout"] = 0.0
    cfg["decoder"] = {"type": "audiocaption_amd.rnn_decoder.TemporalBahAttnDecoder", "args": dict(R.PUB, dropout=0.0)}
    cfg["type"] = "audiocaption_amd.attn_model.TemporalSeq2SeqAttnModel"
    model = A.init_model_from_config(cfg, print_fn=lambda s: None)
    state = P.cnn14_state("encoder.cnn.")
    state = {k: v for k, v in P.to_torch(state).items() if k in model.state_dict()}
    own = R.pub_state(19, 3.0)
    state.update(own)
    model.load_state_dict(state, strict=False)
    model = model.to(dev).train()
    model.encoder.cnn.eval()           # the frozen Cnn14 without its dropout: the same work in every configuration
    n = SECONDS * 32000
    wav = torch.from_numpy(P.synthetic_wav(B, n, seed=1)).to(dev)
    cap, cap_len = R.caption(B, TC, [TC] * B, V, 5)
    tags = torch.arange(B) % 4
    random.seed(5)
    use_cap = [int(random.random() < 0.7) for _ in range(TC - 1)]
    batch = {"mode": "train", "wav": wav, "wav_len": [n] * B, "specaug": False, "cap": cap.to(dev), "cap_len": cap_len,
             "ss_ratio": 0.7, "_use_cap": use_cap, "temporal_tag": tags}
    loss_fn = LabelSmoothingLoss(smoothing=0.1)
    tgt, tgt_len = cap[:, 1:].to(dev), torch.as_tensor(cap_len - 1)

    def hip(b):
        out = model(b)
        loss_fn({"logit": out["logit"], "tgt": tgt, "tgt_len": tgt_len}).backward()
        return out

    # the preset Cnn14 output both "from_cnn" configurations start from: what the model's own Cnn14 gives for the batch
    hip(batch)
    cnn_attn = next(reversed(model._train_engine._states.values()))["cnn_attn"].clone()
    Tq = cnn_attn.shape[1]
    hooked = dict(batch, _cnn_attn=cnn_attn)
    own_dev = {k: v.to(dev) for k, v in own.items()}
    lens = torch.full((B,), Tq)

    def ref():
        return R.model_step_grads(own_dev, cnn_attn, lens, cap, cap_len, use_cap, tags)

    a, b = hip(hooked), ref()
    same_seq = bool(torch.equal(a["seq"], b["seq"].cpu()))      # a near-tie on a fed-back step may part the two
    gap = float((a["logit"].detach() - b["logit"]).abs().max()) / float(b["logit"].abs().max())
    for _ in range(3):
        hip(batch)
        hip(hooked)
        ref()
    torch.cuda.synchronize()
    t_wav = [event_ms(lambda: hip(batch)) for _ in range(reps)]
    t_hip, t_ref = [], []
    for _ in range(reps):
        t_hip.append(event_ms(lambda: hip(hooked)))
        t_ref.append(event_ms(ref))
    T = TC - 1
    common = {"device": torch.cuda.get_device_name(0), "clips": B, "seconds": SECONDS, "cnn14_frames": Tq, "steps": T,
              "vocab": V, "ss_ratio": 0.7, "fed_back_steps": T - sum(use_cap), "logit_gap_rel": round(gap, 9),
              "same_seq": same_seq}
    lines = [dict(common, config="hip_from_wav", **summary(t_wav)),
             dict(common, config="hip_from_cnn", **summary(t_hip), decoder_launches_per_step_forward=FWD_LAUNCHES_PER_STEP,
                  decoder_launches_per_step_backward=BWD_LAUNCHES_PER_STEP,
                  decoder_chain_launches=T * (FWD_LAUNCHES_PER_STEP + BWD_LAUNCHES_PER_STEP)),
             dict(common, config="torch_from_cnn", **summary(t_ref))]
    lines[2]["ratio_torch_over_hip"] = round(lines[2]["ms"] / lines[1]["ms"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
