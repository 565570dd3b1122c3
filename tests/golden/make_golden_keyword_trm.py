"""Generate g27_keyword_trm.npz: the keyword-conditioned Transformer captioner run by the REFERENCE on the CPU
(captioning/models/transformer_model.py:223-264 KeywordCondTransformerModel over transformer_decoder.py:177-214
KeywordProbTransformerDecoder; base.py for the searches and the training forward).

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_keyword_trm.py

The import stubs are those of make_golden_attn_gru.py.  Weights and inputs are seeded procedural draws
(tests/_keyword_trm_ref.py rebuilds them); the fixture stores outputs only.

Inference, both shapes of ``_keyword_trm_ref.SHAPES`` over ``nn.Identity()``, two keyword batches: greedy (seq, the top-8
logits of every live position), beam 2 and 3 with and without ``n_best``, and the decoder's eval-mode full-sequence forward.
Training (d256), every dropout p = 0, ``random.seed(COIN_SEED)`` before every forward: the whole model over the reference
``CrnnEncoder`` around a preset Cnn14 output under LabelSmoothingLoss(0.1) at ss_ratio 1 ("tf") and 0.5 ("ss"): coins, loss,
top-8 logits, seq, per trainable tensor the gradient's norm, sum and 64 samples, the total norm and the change of the samples
after one torch.optim.Adam step (lr 5e-4, weight_decay 1e-6) on the clipped gradients - make_golden_trm_train.py's recipe.

The draw rule is the project's: candidate draws are tried in order, one per shape; a draw is used only if on the reference's
own outputs every greedy top-1 / top-2 gap at a live position, every beam-search margin (between the candidates kept and the
first one dropped, traced by the restatement after its captions have been found equal to the reference's) and every top-1 /
top-2 gap of a fed-back training step is >= 1e-4, the greedy captions have varied tokens and at least one early <end>, and
zeroing the keywords moves the step-0 logits by more than 1e-3.  So no test skips an id comparison.  The draws tried and the
gaps of the restatement (float32 and float64) against the reference go to REPORT_keyword_trm.txt; the section from
REPORT_MARK on (a GPU run's figures) is kept.
"""
import os
import random
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

REPORT_MARK = "==== gates and measured figures"


def main():
    from make_golden_attn_gru import _install_stubs
    _install_stubs()
    torch.manual_seed(27)
    import captioning.models.transformer_decoder as ref_dec     # reference
    import captioning.models.transformer_model as ref_model
    from captioning.models.crnn_trm_encoder import CrnnEncoder
    from captioning.models.rnn_encoder import RnnEncoder
    from captioning.losses.loss import LabelSmoothingLoss
    from make_golden_trm_train import PresetCnn
    import _keyword_trm_ref as R

    GATE = R.GATE
    report, fixture, gaps = [], {}, {}
    idx_gen = np.random.default_rng(27)

    def ref_decoder(shape, state):
        dec = ref_dec.KeywordProbTransformerDecoder(dropout=0.0, **R.SHAPES[shape])
        dec.load_state_dict({k[len("decoder."):]: v for k, v in state.items() if k.startswith("decoder.")}, strict=True)
        return dec

    def note(key, a, b):
        gaps[key] = max(gaps.get(key, 0.0), float((a.double() - b.double()).abs().max()))
        return gaps[key]

    def try_infer(shape, state):
        out, msg = {}, []
        s64 = R.f64(state)
        model = ref_model.KeywordCondTransformerModel(nn.Identity(), ref_decoder(shape, state)).eval()
        F_ = R.SHAPES[shape]["fc_emb_dim"]
        with torch.no_grad():
            for which in (0, 1):
                attn, lens, kw = R.infer_inputs(shape, which)
                base = {"mode": "inference", "attn_emb": attn, "attn_emb_len": lens, "fc_emb": torch.zeros(R.B, F_),
                        "keyword": kw, "max_length": R.MAX_LENGTH}
                ref = model(dict(base, sample_method="greedy"))
                live = R.live_mask(ref["seq"])
                tv, ti = ref["logit"].topk(8, dim=2)
                gap = float((tv[..., 0] - tv[..., 1])[live].min())
                if gap < GATE:
                    return None, f"k{which}: greedy top-1 / top-2 gap {gap:.2e}"
                for tag, st in (("float32", state), ("float64", s64)):
                    mine = R.greedy(st, attn, lens, kw, shape)
                    assert torch.equal(mine["seq"], ref["seq"]), ("restatement differs from the reference (greedy)", shape, tag)
                    d = note(f"{shape} greedy logit, {tag}", mine["logit"][live], ref["logit"][live])
                    assert d < GATE, (shape, tag, d)
                lengths = [int((r != R.END).long().cumprod(0).sum()) for r in ref["seq"]]
                if which == 0:
                    if not (min(lengths) < R.MAX_LENGTH - 1 and max(lengths) > min(lengths)):
                        return None, f"k0: greedy lengths {lengths}: no early <end> beside a longer row"
                    if len(set(ref["seq"][live].tolist())) < 5:
                        return None, f"k0: greedy tokens {ref['seq'].tolist()} are not varied"
                    zero = model(dict(base, sample_method="greedy", keyword=torch.zeros_like(kw)))
                    moved = float((zero["logit"][:, 0] - ref["logit"][:, 0]).abs().max())
                    if moved <= 1e-3:
                        return None, f"k0: zeroing the keywords moves the step-0 logits by {moved:.1e}"
                keep = lambda x, m: torch.where(m, x, torch.zeros((), dtype=x.dtype)).numpy()   # noqa: E731
                out.update({f"k{which}_greedy_seq": ref["seq"].numpy(), f"k{which}_greedy_top_val": keep(tv, live[..., None]),
                            f"k{which}_greedy_top_idx": keep(ti, live[..., None]).astype(np.int32)})
                msg.append(f"k{which} greedy lengths {lengths} gap {gap:.2e}")
                for k in R.BEAMS:
                    ref_b = model(dict(base, sample_method="beam", beam_size=k))
                    ref_n = model(dict(base, sample_method="beam", beam_size=k, n_best=True, n_best_size=k))
                    trace = []
                    mine = R.beam_search(s64, attn, lens, kw, shape, k, trace=trace)
                    mine_n = R.beam_search(s64, attn, lens, kw, shape, k, n_best=True, n_best_size=k)
                    assert torch.equal(ref_b["seq"], mine["seq"]), ("restatement differs from the reference (beam)", shape, k)
                    assert torch.equal(ref_n["seq"], mine_n["seq"]), ("restatement differs (n_best)", shape, k)
                    margin = min(r["margin"] for r in trace)
                    if margin < GATE:
                        return None, f"k{which}: beam {k} margin {margin:.2e}"
                    out[f"k{which}_beam{k}_seq"] = ref_b["seq"].numpy()
                    out[f"k{which}_beam{k}_nbest_seq"] = ref_n["seq"].numpy()
                    msg.append(f"beam {k} margin {margin:.2e}")
            inp = R.forward_inputs(shape)
            ref = model.decoder(dict(inp))
            for tag, st in (("float32", state), ("float64", s64)):
                mine = R.forward(st, inp["word"], inp["attn_emb"], inp["attn_emb_len"], inp["keyword"], shape)
                assert note(f"{shape} forward logit, {tag}", mine["logit"], ref["logit"]) < GATE
                assert note(f"{shape} forward embed, {tag}", mine["embed"], ref["embed"]) < GATE
            out["forward_logit"], out["forward_embed"] = ref["logit"].numpy(), ref["embed"].numpy()
        return out, "; ".join(msg)

    def try_train(state):
        attn, lens, kw, cap, cap_len = R.train_inputs()
        T = cap.shape[1] - 1
        stored, msg, sample_idx = {}, [], None
        for tag, ss in (("tf", 1), ("ss", 0.5)):
            rnn = RnnEncoder(spec_dim=-1, fc_feat_dim=2048, attn_feat_dim=2048, bidirectional=True, hidden_size=256,
                             dropout=0.0, num_layers=3)
            enc = CrnnEncoder(PresetCnn(attn, list(R.TRAIN_LENS)), rnn, freeze_cnn=True, freeze_cnn_bn=True)
            model = ref_model.KeywordCondTransformerModel(enc, ref_dec.KeywordProbTransformerDecoder(dropout=0.0,
                                                                                                     **R.SHAPES["d256"]))
            assert set(model.state_dict()) == set(state), set(model.state_dict()) ^ set(state)
            model.load_state_dict(state, strict=True)
            model.train()
            trainable = [(k, p_) for k, p_ in model.named_parameters() if p_.requires_grad]
            assert sorted(k for k, _ in trainable) == sorted(R.trainable_keys(state)), "trainable key sets differ"
            if sample_idx is None:
                sample_idx = {k: idx_gen.integers(0, p_.numel(), size=min(64, p_.numel())) for k, p_ in trainable}
            random.seed(R.COIN_SEED)
            use_cap = [int(random.random() < ss) for _ in range(T)] if ss != 1 else [1] * T
            if ss != 1 and not (any(use_cap) and not all(use_cap[1:])):
                return None, None, f"{tag}: the coins {use_cap} leave no teacher-forced or no fed-back step"
            random.seed(R.COIN_SEED)
            out = model({"mode": "train", "wav": torch.zeros(R.TRAIN_N, 10), "wav_len": [10] * R.TRAIN_N, "specaug": False,
                         "cap": cap, "cap_len": cap_len, "ss_ratio": ss, "keyword": kw})
            out["tgt"], out["tgt_len"] = cap[:, 1:], torch.as_tensor(cap_len - 1)
            loss = LabelSmoothingLoss(smoothing=0.1)(out)
            loss.backward()
            total_norm = torch.nn.utils.clip_grad_norm_([p_ for _, p_ in trainable], 1.0)
            coef = min(1.0, float(1.0 / (total_norm + 1e-6)))
            raw = {k: p_.grad.detach().clone() / coef for k, p_ in trainable}
            opt = torch.optim.Adam([p_ for _, p_ in trainable], lr=5e-4, weight_decay=1e-6)
            before = {k: p_.detach().clone() for k, p_ in trainable}
            opt.step()
            logit = out["logit"].detach()
            if ss != 1:
                last = max([t for t in range(T) if not use_cap[t] and t > 0], default=0)
                top2 = logit[:, :last].topk(2, -1).values
                g = float((top2[..., 0] - top2[..., 1]).min()) if last else float("inf")
                if g < GATE:
                    return None, None, f"{tag}: fed-back top-1 / top-2 gap {g:.2e}"
                msg.append(f"{tag} fed-back gap {g:.2e} coins {''.join(map(str, use_cap))}")
            for name, dt in (("float32", torch.float32), ("float64", torch.float64)):
                o = R.train_step_grads(state, attn, lens, kw, cap, cap_len, use_cap, teacher_forcing=(ss == 1), dtype=dt)
                if ss != 1:
                    assert torch.equal(o["seq"], out["seq"]), f"{tag}: greedy tokens of the restatement differ"
                note(f"train {tag} logit, {name}", o["logit"], logit)
                gaps[f"train {tag} loss (relative), {name}"] = abs(float(o["loss"]) - float(loss)) / float(loss)
                gaps[f"train {tag} grads (rel. to max), {name}"] = max(
                    float((o["grads"][k].double() - raw[k].double()).abs().max()) / (float(raw[k].abs().max()) + 1e-12)
                    for k, _ in trainable)
                assert gaps[f"train {tag} logit, {name}"] < GATE and gaps[f"train {tag} grads (rel. to max), {name}"] < 1e-3
            top = logit.topk(8, dim=-1)
            st = {"use_cap": np.array(use_cap, dtype=np.int32), "loss": np.array(float(loss.detach())),
                  "total_norm": np.array(float(total_norm)), "logit_top_val": top.values.numpy(),
                  "logit_top_idx": top.indices.numpy().astype(np.int32)}
            if "seq" in out:
                st["seq"] = out["seq"].numpy()
            for k, p_ in trainable:
                st[f"gnorm/{k}"] = np.array(float(raw[k].double().norm()))
                st[f"gsum/{k}"] = np.array(float(raw[k].double().sum()))
                st[f"gsample/{k}"] = raw[k].reshape(-1)[sample_idx[k]].numpy()
                st[f"delta/{k}"] = (p_.detach() - before[k]).reshape(-1)[sample_idx[k]].numpy()
            stored.update({f"train_{tag}_{k}": v for k, v in st.items()})
        return stored, sample_idx, "; ".join(msg)

    for shape in R.SHAPES:
        used = None
        for seed, beta in R.CANDIDATES:
            state = R.decoder_state(shape, seed, beta)
            stored, msg = try_infer(shape, state)
            why, ok = [msg], stored is not None
            if ok and shape == "d256":
                tr, sample_idx, msg = try_train(R.model_state(seed, beta))
                why.append(msg)
                ok = tr is not None
                if ok:
                    stored.update(tr)
                    stored.update({f"sample_idx/{k}": v for k, v in sample_idx.items()})
            line = f"{shape} seed {seed} end_beta {beta}: " + ("USED: " if ok else "rejected: ") + "; ".join(why)
            print(line)
            report.append(line)
            if ok:
                used = (seed, beta)
                fixture.update({f"{shape}_{k}": v for k, v in stored.items()})
                break
        assert used is not None, f"{shape}: no candidate draw passes the gates"
        fixture[f"{shape}_recipe"] = np.array(used, dtype=np.float64)

    # the reference's own names: state-dict keys with shapes, and the parameter order
    dec = ref_dec.KeywordProbTransformerDecoder(dropout=0.2, **R.SHAPES["d256"])
    fixture["state_keys"] = np.array(list(dec.state_dict().keys()))
    fixture["state_shapes"] = np.array([",".join(map(str, v.shape)) for v in dec.state_dict().values()])
    fixture["param_names"] = np.array([k for k, _ in dec.named_parameters()])
    fixture["coin_seed"] = np.array(R.COIN_SEED)

    path = os.path.join(HERE, "g27_keyword_trm.npz")
    np.savez_compressed(path, **{k: fixture[k] for k in sorted(fixture)})
    size = os.path.getsize(path)
    assert size <= 1000000, size
    print(f"wrote {path}: {size} bytes")
    rpath, kept = os.path.join(HERE, "REPORT_keyword_trm.txt"), REPORT_MARK + " (tests/test_gpu_keyword_trm.py): not measured\n"
    if os.path.exists(rpath):
        with open(rpath) as f:
            old = f.read()
        if REPORT_MARK in old:
            kept = old[old.index(REPORT_MARK):]
    with open(rpath, "w") as f:
        f.write("g27_keyword_trm.npz: candidate draws tried by make_golden_keyword_trm.py (torch %s)\n" % torch.__version__)
        f.write("\n".join(report) + "\n")
        f.write("max |tests/_keyword_trm_ref.py - reference| on the CPU\n")
        for k, v in gaps.items():
            f.write(f"  {k:52s} {v:.3e}\n")
        f.write(kept)


if __name__ == "__main__":
    main()
