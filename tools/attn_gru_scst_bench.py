"""Timing of one self-critical sequence training iteration of the attention-GRU captioner on the HIP path (ScstWrapper over
TemporalSeq2SeqAttnModel with the built-in device CIDEr-D, loss.backward(), clip_grad_norm_, FusedAdam), its parts, and the
two figures to hold it against.

  python tools/attn_gru_scst_bench.py [--out FILE] [--reps 9]     (default FILE: profiles/attn_gru_scst_bench.jsonl)

The model of tools/attn_gru_train_bench.py (frozen Cnn14 + 3-layer bi-GRU + TemporalBahAttnDecoder at E = d = S = A = F =
512, V 4981, every dropout p = 0), 32 clips x 10 s (31 Cnn14 frames), max_length T = 20, temp 1.0, five references of 12
words per clip.  Wall-clock times with a device synchronisation before and after each timed piece, three warm-up
iterations, ``--reps`` (>= 5) timed ones, the median reported with the minimum and maximum.  One JSON line per
configuration, printed and appended to FILE:

  "scst_hip_from_wav"    the whole iteration from the waveform;
  "scst_hip_parts"       the same iteration piece by piece (ScstWrapper.scst's own sequence): greedy baseline, sampled
                         rollout, reward (Cider.score_ids on the device), backward (loss, the engine's backward, clip, Adam);
  "ce_hip_from_wav"      the cross-entropy iteration of the same model in the same run (model(input_dict) with mode="train",
                         ss_ratio 0.7, captions of 21 tokens, LabelSmoothingLoss, backward, clip, FusedAdam);
  "scst_hip_from_cnn"    the SCST iteration downstream of a preset Cnn14 output (the ``_cnn_attn`` hook);
  "scst_torch_from_cnn"  the same iteration in plain torch on the same device on the same preset Cnn14 output: the bi-GRU and
                         decoder step of tests/_attn_gru_train_ref.py under autograd, a greedy pass without gradients, a
                         sampled pass (torch.multinomial), the same device CIDEr-D, torch's clip_grad_norm_ and Adam.

and the two ratios: SCST over cross-entropy (from the waveform) and torch over HIP (from the Cnn14 output)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

B, SECONDS, T, V, TEMP = 32, 10, 20, 4981, 1.0


class Vocabulary:
    class _Words:
        def __getitem__(self, i):
            return f"w{int(i)}"
    idx2word = _Words()


def sync():
    torch.cuda.synchronize()
    return time.perf_counter()


def timed(fn):
    t0 = sync()
    fn()
    return 1e3 * (sync() - t0)


def summary(ms):
    return {"ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attn_gru_scst_bench.jsonl"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    reps = max(5, args.reps)
    import audiocaption_amd as A
    from audiocaption_amd import build
    from audiocaption_amd import procedural as P
    from audiocaption_amd.cider import Cider
    from audiocaption_amd.loss import LabelSmoothingLoss
    from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
    from audiocaption_amd.rl_model import scst_loss
    from audiocaption_amd.train import _TrainBridge
    import _attn_gru_train_ref as R
    build.build()
    dev = "cuda"
    cfg = A.cnn14rnn_trm_config(V)
    cfg["encoder"]["rnn"]["args"]["dropout"] = 0.0
    cfg["decoder"] = {"type": "audiocaption_amd.rnn_decoder.TemporalBahAttnDecoder", "args": dict(R.PUB, dropout=0.0)}
    cfg["type"] = "audiocaption_amd.attn_model.TemporalSeq2SeqAttnModel"
    model = A.init_model_from_config(cfg, print_fn=lambda s: None)
    state = {k: v for k, v in P.to_torch(P.cnn14_state("encoder.cnn.")).items() if k in model.state_dict()}
    own = R.pub_state(19, 3.0)
    state.update(own)
    model.load_state_dict(state, strict=False)
    model = model.to(dev).train()
    model.encoder.cnn.eval()           # the frozen Cnn14 without its dropout: the same work in every configuration
    wrapper = A.ScstWrapper(model)
    n = SECONDS * 32000
    wav = torch.from_numpy(P.synthetic_wav(B, n, seed=1)).to(dev)
    tags = torch.arange(B) % 4
    rng = np.random.default_rng(0)
    keys = [f"clip{i}" for i in range(B)]
    key2refs = {k: [" ".join(f"w{w}" for w in rng.integers(4, V, 12)) for _ in range(5)] for k in keys}
    cider = Cider()
    batch = {"mode": "train", "wav": wav, "wav_len": [n] * B, "specaug": False, "temporal_tag": tags, "max_length": T,
             "temp": TEMP, "keys": keys, "key2refs": key2refs, "vocabulary": Vocabulary(), "scorer": cider}
    params = [p for p in wrapper.parameters() if p.requires_grad]
    opt = FusedAdam(params, lr=5e-4, weight_decay=1e-6)

    def scst(b):
        opt.zero_grad()
        out = wrapper(b)
        out["loss"].backward()
        clip_grad_norm_(params, 1.0)
        opt.step()
        return out

    cap, cap_len = R.caption(B, T + 1, [T + 1] * B, V, 5)
    ce_batch = {"mode": "train", "wav": wav, "wav_len": [n] * B, "specaug": False, "cap": cap.to(dev), "cap_len": cap_len,
                "ss_ratio": 0.7, "temporal_tag": tags}
    loss_fn = LabelSmoothingLoss(smoothing=0.1)
    tgt, tgt_len = cap[:, 1:].to(dev), torch.as_tensor(cap_len - 1)

    def ce():
        opt.zero_grad()
        out = model(ce_batch)
        loss_fn({"logit": out["logit"], "tgt": tgt, "tgt_len": tgt_len}).backward()
        clip_grad_norm_(params, 1.0)
        opt.step()

    scst(batch)
    eng = model._train_engine
    cnn_attn = next(v for v in reversed(list(eng._states.values())) if v.get("cnn_attn") is not None)["cnn_attn"].clone()
    Tq = cnn_attn.shape[1]
    hooked = dict(batch, _cnn_attn=cnn_attn)

    # ---- the same iteration in plain torch ----------------------------------------------------------------------------
    leaves = {k: torch.nn.Parameter(v.to(dev)) for k, v in own.items()}
    t_opt = torch.optim.Adam(list(leaves.values()), lr=5e-4, weight_decay=1e-6)
    lens = torch.full((B,), Tq, device=dev)
    tags_dev = tags.to(dev)
    end = model.end_idx

    def roll(dec, attn_emb, fc_emb, sample):
        h = torch.zeros(B, R.PUB["d_model"], device=dev)
        done = torch.zeros(B, dtype=torch.bool, device=dev)
        logits, words = [], []
        for t in range(T):
            emb = dec["temporal_embedding.weight"][tags_dev] if t == 0 else dec["word_embedding.weight"][words[-1]]
            h, logit, _ = R.step(dec, emb, h, attn_emb, lens, fc_emb)
            if sample:
                w = torch.multinomial(torch.softmax(torch.log_softmax(logit.detach(), -1) / TEMP, -1), 1).squeeze(1)
            else:
                w = logit.argmax(-1)
            w = torch.where(done, torch.full_like(w, end), w)
            done = done | (w == end)
            logits.append(logit)
            words.append(w)
        return torch.stack(logits, 1), torch.stack(words, 1)

    def torch_scst():
        t_opt.zero_grad()
        dec = {k[len("decoder."):]: v for k, v in leaves.items() if k.startswith("decoder.")}
        with torch.no_grad():
            attn_emb, fc_emb = R.encoder_forward(leaves, cnn_attn, lens)
            _, greedy = roll(dec, attn_emb, fc_emb, False)
        attn_emb, fc_emb = R.encoder_forward(leaves, cnn_attn, lens)
        logit, seq = roll(dec, attn_emb, fc_emb, True)
        reward = cider.score_ids(key2refs, batch["vocabulary"], V, keys, (seq.to(torch.int32), greedy.to(torch.int32)),
                                 model.start_idx, end)["reward"]
        lp = torch.log_softmax(logit, -1).gather(-1, seq.unsqueeze(-1)).squeeze(-1) / TEMP
        mask = torch.cat([torch.ones(B, 1, device=dev), (seq[:, :-1] != end).float()], 1)
        (-lp * reward[:, None] * mask).sum(1).mean().backward()
        torch.nn.utils.clip_grad_norm_(list(leaves.values()), 1.0)
        t_opt.step()

    for _ in range(3):
        scst(batch)
        ce()
        scst(hooked)
        torch_scst()
    t_scst = [timed(lambda: scst(batch)) for _ in range(reps)]
    t_ce = [timed(ce) for _ in range(reps)]
    t_hip, t_torch = [], []
    for _ in range(reps):
        t_hip.append(timed(lambda: scst(hooked)))
        t_torch.append(timed(torch_scst))

    # the iteration piece by piece (ScstWrapper.scst's own sequence)
    parts = {"baseline": [], "rollout": [], "reward": [], "backward": []}
    for _ in range(reps):
        opt.zero_grad()
        got = {}

        def baseline():
            got["greedy"] = wrapper._baseline(batch, T)[1]

        def rollout():
            model.train()
            got["ro"] = eng.rollout(batch)

        def reward():
            got["reward"] = cider.score_ids(key2refs, batch["vocabulary"], V, keys, (got["ro"]["seq_i32"], got["greedy"]),
                                            model.start_idx, end)["reward"]

        def backward():
            logit = _TrainBridge.apply(eng, got["ro"]["logit"], *eng.flat.params)
            scst_loss(logit, got["ro"]["seq_i32"], got["reward"], TEMP, end).backward()
            clip_grad_norm_(params, 1.0)
            opt.step()

        for name, fn in (("baseline", baseline), ("rollout", rollout), ("reward", reward), ("backward", backward)):
            parts[name].append(timed(fn))

    common = {"device": torch.cuda.get_device_name(0), "clips": B, "seconds": SECONDS, "cnn14_frames": Tq, "max_length": T,
              "vocab": V, "temp": TEMP}
    lines = [dict(common, config="scst_hip_from_wav", **summary(t_scst)),
             dict(common, config="scst_hip_parts", **{f"{k}_ms": round(statistics.median(v), 3) for k, v in parts.items()},
                  reps=reps),
             dict(common, config="ce_hip_from_wav", steps=T, ss_ratio=0.7, **summary(t_ce)),
             dict(common, config="scst_hip_from_cnn", **summary(t_hip)),
             dict(common, config="scst_torch_from_cnn", **summary(t_torch))]
    lines[0]["ratio_scst_over_ce"] = round(lines[0]["ms"] / lines[2]["ms"], 2)
    lines[4]["ratio_torch_over_hip"] = round(lines[4]["ms"] / lines[3]["ms"], 2)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
