"""Generate g26_cond_attn_gru.npz: the condition-controlled attention-GRU captioners and the specificity loss run by the
REFERENCE on the CPU (captioning/models/rnn_decoder.py:276-336,519-575 ConditionalBahAttnDecoder / SpecificityBahAttnDecoder,
attn_model.py:191-223 ConditionalSeq2SeqAttnModel, base.py, losses/loss.py:195-219 SpecificityLossWrapper).

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_cond_attn_gru.py

The import stubs are those of make_golden_attn_gru.py plus ``captioning.models.style_model`` (attn_model.py:5 imports a
module the reference does not ship).  Weights and inputs are seeded procedural draws (tests/_cond_attn_gru_ref.py rebuilds
them); the fixture stores outputs only.

Inference (``_cond_attn_gru_ref.INFER``, both decoders): greedy and beam search of ``ConditionalSeq2SeqAttnModel`` over
``nn.Identity()`` - seq, the top-8 logits of every live position, attention weights (the small batches), beam captions.
Training, every dropout p = 0, ``random.seed(COIN_SEED)`` before every forward, make_golden_attn_gru_train.py's ``cloned_word``
hook: the decoder alone (``_cond_attn_gru_ref.TRAIN``) under LabelSmoothingLoss(0.1) at ss_ratio 1 ("tf") and 0.7 ("ss"), and
the whole model at the published widths over the reference ``CrnnEncoder`` around a preset Cnn14 output under
SpecificityLossWrapper(LabelSmoothingLoss(0.1), word_specificity, "sum", alpha 0.3): coins, the three losses, top-8 logits,
seq, per trainable tensor (and d attn_emb) the gradient's norm, sum and 64 samples, the total norm and the change of the
samples after one torch.optim.Adam step (lr 5e-4, weight_decay 1e-6) on the clipped gradients.
The loss alone (``LOSS_GRID``): the three losses and d logit (norm, 64 samples) of SpecificityLossWrapper over a plain
differentiable stand-in word loss, which lets tgt_len - 1 reach T.

The draw rule is make_golden_attn_gru.py's and make_golden_attn_gru_train.py's: weight draws are tried in order, one per
(shape, decoder); a draw is used only if on the reference's own outputs every greedy top-1 / top-2 gap at a live position,
every beam-search margin (between the candidates kept and the first one dropped, traced by the restatement after its
captions have been found equal to the reference's) and every top-1 / top-2 gap of a fed-back training step is >= 1e-4.  So no
test skips an id comparison.  The draws tried and the gaps of the restatement against the reference go to
REPORT_cond_attn_gru.txt; the section from REPORT_MARK on (a GPU run's figures) is kept.
"""
import os
import random
import sys
import types

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

GATE = 1e-4
LOSS_BAR, GRAD_BAR = 2e-5, 1e-4          # tests/test_gpu_attn_gru_train.py
CANDIDATES = [(seed, bias) for seed in (26, 27, 28, 29) for bias in (3.0, 2.5, 3.5)]
REPORT_MARK = "==== gates and measured figures"


def main():
    from make_golden_attn_gru import _install_stubs
    _install_stubs()
    style = types.ModuleType("captioning.models.style_model")
    style.StyleCaptionModel = type("StyleCaptionModel", (), {})
    sys.modules["captioning.models.style_model"] = style
    torch.manual_seed(26)
    import captioning.models.attn_model as ref_model     # reference
    import captioning.models.rnn_decoder as ref_dec
    from captioning.models.crnn_trm_encoder import CrnnEncoder
    from captioning.models.rnn_encoder import RnnEncoder
    from captioning.losses.loss import LabelSmoothingLoss, SpecificityLossWrapper
    from make_golden_trm_train import PresetCnn
    import _attn_gru_ref as AR
    import _attn_gru_train_ref as TR
    import _cond_attn_gru_ref as R

    DEC = {"cond": ref_dec.ConditionalBahAttnDecoder, "spec": ref_dec.SpecificityBahAttnDecoder}

    def zero_filled(cls):
        class Z(cls):
            def prepare_output(self, input_dict):
                out = super().prepare_output(input_dict)
                out["attn_weight"].zero_()
                return out

            def prepare_beamsearch_output(self, input_dict):
                out = super().prepare_beamsearch_output(input_dict)
                out["attn_weight"].zero_()
                return out
        return Z

    def cloned_word(cls):
        class C(cls):
            def prepare_decoder_input(self, input_dict, output):
                d = super().prepare_decoder_input(input_dict, output)
                d["word"] = d["word"].clone()
                return d
        return C

    def decoder(kind, shape, sd):
        dec = DEC[kind](dropout=0.0, **R.SHAPES[shape])
        dec.load_state_dict(sd, strict=True)
        return dec

    report, fixture, gaps = [], {}, {}
    idx_gen = np.random.default_rng(4)

    def caps(seq):
        return [tuple(r[:AR.first_end(r)]) for r in seq.tolist()]

    # ---- inference ---------------------------------------------------------------------------------------------------
    def try_infer(kind, name, sd):
        shape = R.INFER[name][0]
        mem, lens, cond, L, beams = R.infer_inputs(name)
        B, F = mem.shape[0], R.SHAPES[shape]["fc_emb_dim"]
        model = zero_filled(ref_model.ConditionalSeq2SeqAttnModel)(nn.Identity(), decoder(kind, shape, sd)).eval()
        base = {"mode": "inference", "attn_emb": mem, "attn_emb_len": lens, "fc_emb": torch.zeros(B, F), "condition": cond,
                "max_length": L}
        out, msg = {}, []
        with torch.no_grad():
            ref = model(dict(base, sample_method="greedy"))
            mine = R.greedy(kind, sd, mem, lens, cond, L)
            rc = caps(ref["seq"])
            assert rc == caps(mine["seq"]), ("restatement differs from the reference (greedy)", kind, name)
            live = torch.from_numpy(AR.live_mask(ref["seq"].numpy()))
            tv, ti = ref["logit"].topk(8, dim=2)
            gap = float((tv[..., 0] - tv[..., 1])[live].min())
            if gap < GATE:
                return None, f"{name}: greedy top-1 / top-2 gap {gap:.2e}"
            for k_, a, b in (("logit", ref["logit"], mine["logit"]),
                             ("attn_weight", ref["attn_weight"].transpose(1, 2), mine["attn_weight"].transpose(1, 2)),
                             ("embed", ref["embed"], mine["embed"])):
                dmax = float((a[live] - b[live]).abs().max())
                gaps[f"{kind} {name} greedy {k_}"] = dmax
                assert dmax < 1e-4, ("restatement differs from the reference (greedy)", kind, name, k_, dmax)
            keep = lambda x, m: torch.where(m, x, torch.zeros((), dtype=x.dtype)).numpy()   # noqa: E731
            out.update(greedy_seq=mine["seq"].numpy(), greedy_top_val=keep(tv, live[..., None]),
                       greedy_top_idx=keep(ti, live[..., None]).astype(np.int32), greedy_state=ref["state"].numpy())
            if B <= 5:
                out["greedy_attn_weight"] = keep(ref["attn_weight"], live[:, None, :])
            msg.append(f"{name} greedy lengths {[len(c) for c in rc]} gap {gap:.2e}")
            # the condition is read: other values, other logits
            other = model(dict(base, sample_method="greedy", condition=cond.roll(1) + 0.25))
            if float((other["logit"][:, 0] - ref["logit"][:, 0]).abs().max()) < 1e-3:
                return None, f"{name}: changing the condition changes no logit"
            for k in beams:
                ref_b = model(dict(base, sample_method="beam", beam_size=k))
                trace = []
                my_b = R.beam_search(kind, sd, mem, lens, cond, k, L, trace=trace)
                assert torch.equal(ref_b["seq"], my_b["seq"]), ("restatement differs from the reference (beam)", kind, name, k)
                dmax = float((ref_b["attn_weight"] - my_b["attn_weight"]).abs().max())
                gaps[f"{kind} {name} beam {k} attn_weight"] = dmax
                assert dmax < 1e-4, (kind, name, k, dmax)
                margin = min(r["margin"] for r in trace)
                if margin < GATE:
                    return None, f"{name}: beam {k} margin {margin:.2e}"
                out[f"beam{k}_seq"] = ref_b["seq"].numpy()
                if B <= 5:
                    out[f"beam{k}_attn_weight"] = ref_b["attn_weight"].numpy()
                msg.append(f"beam {k} margin {margin:.2e}")
        return out, "; ".join(msg)

    # ---- training ----------------------------------------------------------------------------------------------------
    def coins(ss_ratio, T):
        random.seed(TR.COIN_SEED)
        return [int(random.random() < ss_ratio) for _ in range(T)]

    def run_step(model, batch, extra_leaves, cap, cap_len, ss_ratio, sample_idx, loss_fn, wrapped):
        T = cap.shape[1] - 1
        use_cap = coins(ss_ratio, T)
        model.train()
        model.zero_grad(set_to_none=True)
        random.seed(TR.COIN_SEED)
        out = model(dict(batch, mode="train", cap=cap, cap_len=cap_len, ss_ratio=ss_ratio))
        out["tgt"], out["tgt_len"] = cap[:, 1:], torch.as_tensor(cap_len - 1)
        out["conditions"] = batch["condition"]
        if wrapped:
            loss, word, cl = loss_fn(out)
        else:
            loss = word = loss_fn(out)
            cl = torch.zeros(())
        loss.backward()
        trainable = [(k, p_) for k, p_ in model.named_parameters() if p_.requires_grad]
        total_norm = torch.nn.utils.clip_grad_norm_([p_ for _, p_ in trainable], 1.0)
        coef = min(1.0, float(1.0 / (total_norm + 1e-6)))
        raw = {k: p_.grad.detach().clone() / coef for k, p_ in trainable}
        opt = torch.optim.Adam([p_ for _, p_ in trainable], lr=5e-4, weight_decay=1e-6)
        before = {k: p_.detach().clone() for k, p_ in trainable}
        opt.step()
        top = out["logit"].detach().topk(8, dim=-1)
        st = {"use_cap": np.array(use_cap, dtype=np.int32), "loss": np.array(float(loss.detach())),
              "word_loss": np.array(float(word.detach())), "condition_loss": np.array(float(cl.detach())),
              "total_norm": np.array(float(total_norm)), "seq": out["seq"].numpy(),
              "logit_top_val": top.values.numpy(), "logit_top_idx": top.indices.numpy().astype(np.int32)}
        for k, p_ in trainable:
            st[f"gnorm/{k}"] = np.array(float(raw[k].double().norm()))
            st[f"gsum/{k}"] = np.array(float(raw[k].double().sum()))
            st[f"gsample/{k}"] = raw[k].reshape(-1)[sample_idx[k]].numpy()
            st[f"delta/{k}"] = (p_.detach() - before[k]).reshape(-1)[sample_idx[k]].numpy()
        for k, v in extra_leaves.items():
            st[f"gnorm/{k}"] = np.array(float(v.grad.double().norm()))
            st[f"gsum/{k}"] = np.array(float(v.grad.double().sum()))
            st[f"gsample/{k}"] = v.grad.reshape(-1)[sample_idx[k]].numpy()
        ref = {"logit": out["logit"].detach(), "seq": out["seq"], "loss": float(loss.detach()), "raw": raw,
               "attn_weight": out["attn_weight"].detach(), "use_cap": use_cap,
               "extra": {k: v.grad.detach().clone() for k, v in extra_leaves.items()}}
        return st, ref

    def fed_gap(ref):
        top2 = ref["logit"].topk(2, dim=-1).values
        fed = TR.fed_back_gaps(top2[..., 0] - top2[..., 1], ref["use_cap"], False)
        return float(fed.min()) if fed.numel() else float("inf")

    def compare(tag, ref, mine, strip=""):
        gaps[f"{tag} logit"] = float((mine["logit"].double() - ref["logit"].double()).abs().max())
        gaps[f"{tag} loss (relative)"] = abs(float(mine["loss"]) - ref["loss"]) / ref["loss"]
        gaps[f"{tag} grads (rel. to max)"] = max(
            float((mine["grads"][k[len(strip):]].double() - ref["raw"][k].double()).abs().max()) /
            (float(ref["raw"][k].abs().max()) + 1e-12) for k in ref["raw"])
        assert torch.equal(mine["seq"], ref["seq"]), f"{tag}: arg-max tokens of the restatement differ"
        assert gaps[f"{tag} logit"] < 1e-4 and gaps[f"{tag} grads (rel. to max)"] < 1e-3, tag

    def try_train(kind, name, sd):
        shape = R.TRAIN[name][0]
        mem, lens, cond, cap, cap_len = R.train_inputs(name)
        B, F = mem.shape[0], R.SHAPES[shape]["fc_emb_dim"]
        stored, msg, sample_idx = {}, [], None
        for tag, ss in (("tf", 1), ("ss", 0.7)):
            model = cloned_word(ref_model.ConditionalSeq2SeqAttnModel)(nn.Identity(), decoder(kind, shape, sd))
            a = mem.clone().requires_grad_(True)
            if sample_idx is None:
                sample_idx = {k: idx_gen.integers(0, p_.numel(), size=min(64, p_.numel()))
                              for k, p_ in list(model.named_parameters()) + [("attn_emb", a)]}
            batch = {"attn_emb": a, "fc_emb": torch.zeros(B, F), "attn_emb_len": lens, "condition": cond}
            st, ref = run_step(model, batch, {"attn_emb": a}, cap, cap_len, ss, sample_idx, LabelSmoothingLoss(smoothing=0.1),
                               False)
            if B <= 5:
                st["attn_weight"] = ref["attn_weight"].numpy()
            g = fed_gap(ref)
            if g < GATE:
                return None, None, f"{name} {tag}: fed-back top-1 / top-2 gap {g:.2e}"
            T = cap.shape[1] - 1
            if ss != 1 and T > 1 and not (any(ref["use_cap"]) and not all(ref["use_cap"])):
                return None, None, f"{name} {tag}: the coins {ref['use_cap']} leave no teacher-forced or no fed-back step"
            mine = R.decoder_step_grads(kind, sd, mem, lens, cond, cap, cap_len, ref["use_cap"])
            compare(f"{kind} {name}_{tag}", ref, mine, strip="decoder.")
            want = ref["extra"]["attn_emb"]
            gaps[f"{kind} {name}_{tag} d attn_emb (rel. to max)"] = \
                float((mine["d_attn_emb"] - want).abs().max()) / float(want.abs().max())
            stored.update({f"{name}_{tag}_{k}": v for k, v in st.items()})
            msg.append(f"{name} {tag} gap {g:.2e} coins {''.join(map(str, ref['use_cap']))}")
        return stored, sample_idx, "; ".join(msg)

    for kind in R.KINDS:
        for shape in ("tiny", "small"):
            tag = f"{kind}_{shape}"
            used = None
            for seed, bias in CANDIDATES:
                sd = R.state(kind, shape, seed, bias)
                stored, why, ok = {}, [], True
                for name in [n for n, c in R.INFER.items() if c[0] == shape]:
                    out, msg = try_infer(kind, name, sd)
                    why.append(msg)
                    if out is None:
                        ok = False
                        break
                    stored.update({f"{tag}_{name}_{k}" if name != shape else f"{tag}_{k}": v for k, v in out.items()})
                if ok:
                    for name in [n for n, c in R.TRAIN.items() if c[0] == shape]:
                        out, sample_idx, msg = try_train(kind, name, sd)
                        why.append(msg)
                        if out is None:
                            ok = False
                            break
                        stored.update({f"{kind}_train_{k}": v for k, v in out.items()})
                        stored.update({f"{kind}_train_{name}_sample_idx/{k}": v for k, v in sample_idx.items()})
                line = f"{tag} seed {seed} end_scale {bias}: " + ("USED: " if ok else "rejected: ") + "; ".join(why)
                print(line)
                report.append(line)
                if ok:
                    used = (seed, bias)
                    fixture.update(stored)
                    break
            assert used is not None, f"{tag}: no candidate draw passes the gates"
            fixture[f"{tag}_recipe"] = np.array(used, dtype=np.float64)

        # ---- the published widths: inference of the decoder alone, one training step of the whole model -----------------
        attn = TR.pub_cnn_attn()
        cap, cap_len = TR.pub_caption()
        cond = R.conditions(TR.PUB_N, 2)
        ws = R.word_specificity(TR.PUB["vocab_size"])
        used = None
        for seed, bias in CANDIDATES:
            state = R.pub_state(kind, seed, bias)
            sd = {k[len("decoder."):]: v for k, v in state.items() if k.startswith("decoder.")}
            out, msg = try_infer(kind, "pub", sd)
            why, ok = [msg], out is not None
            if ok:
                rnn = RnnEncoder(spec_dim=-1, fc_feat_dim=2048, attn_feat_dim=2048, bidirectional=True, hidden_size=256,
                                 dropout=0.0, num_layers=3)
                enc = CrnnEncoder(PresetCnn(attn, TR.PUB_LENS), rnn, freeze_cnn=True, freeze_cnn_bn=True)
                model = cloned_word(ref_model.ConditionalSeq2SeqAttnModel)(enc, DEC[kind](dropout=0.0, **TR.PUB))
                assert set(model.state_dict()) == set(state), set(model.state_dict()) ^ set(state)
                model.load_state_dict(state, strict=True)
                sample_idx = {k: idx_gen.integers(0, p_.numel(), size=min(64, p_.numel())) for k, p_ in model.named_parameters()}
                batch = {"wav": torch.zeros(TR.PUB_N, 10), "wav_len": [10] * TR.PUB_N, "specaug": False, "condition": cond}
                loss_fn = SpecificityLossWrapper(LabelSmoothingLoss(smoothing=0.1), ws, "sum", R.ALPHA)
                st, ref = run_step(model, batch, {}, cap, cap_len, 0.7, sample_idx, loss_fn, True)
                g = fed_gap(ref)
                why.append(f"whole model ss gap {g:.2e} coins {''.join(map(str, ref['use_cap']))}")
                ok = g >= GATE and any(ref["use_cap"]) and not all(ref["use_cap"])
                mine = R.model_step_grads(kind, state, attn, torch.tensor(TR.PUB_LENS), cond, cap, cap_len, ref["use_cap"],
                                          ws=ws, targets=cond, reduce="sum", alpha=R.ALPHA)
                compare(f"{kind} pub_ss", ref, mine)
            line = f"{kind}_pub seed {seed} end_scale {bias}: " + ("USED: " if ok else "rejected: ") + "; ".join(why)
            print(line)
            report.append(line)
            if ok:
                used = (seed, bias)
                fixture.update({f"{kind}_pub_{k}": v for k, v in out.items()})
                fixture.update({f"{kind}_train_pub_ss_{k}": v for k, v in st.items()})
                fixture.update({f"{kind}_train_pub_sample_idx/{k}": v for k, v in sample_idx.items()})
                break
        assert used is not None, f"{kind}_pub: no candidate draw passes the gates"
        fixture[f"{kind}_pub_recipe"] = np.array(used, dtype=np.float64)
        keys = list(DEC[kind](dropout=0.0, **TR.PUB).state_dict().keys())
        fixture[f"{kind}_state_keys"] = np.array(keys)

    # ---- the loss alone ----------------------------------------------------------------------------------------------
    dev32 = {"loss": 0.0, "grad": 0.0}
    for case in R.LOSS_GRID:
        logit, tgt_len, conds, ws, reduce, alpha = R.loss_inputs(case)
        leaf = logit.clone().requires_grad_(True)
        wrap = SpecificityLossWrapper(R.stand_in_word_loss, ws, reduce, alpha)
        loss, word, cl = wrap({"logit": leaf, "tgt_len": tgt_len, "conditions": conds})
        loss.backward()
        l64 = logit.double().requires_grad_(True)
        cl64 = R.specificity_loss(l64, ws.double(), tgt_len, conds.double(), reduce)
        tot64 = R.stand_in_word_loss({"logit": l64}) + alpha * cl64
        tot64.backward()
        dev32["loss"] = max(dev32["loss"], abs(float(cl) - float(cl64)) / (abs(float(cl64)) + 1e-30),
                            abs(float(loss) - float(tot64)) / abs(float(tot64)))
        dev32["grad"] = max(dev32["grad"], float((leaf.grad.double() - l64.grad).abs().max()) / float(l64.grad.abs().max()))
        idx = idx_gen.integers(0, logit.numel(), size=64)
        key = "loss_" + R.loss_case_name(case)
        fixture.update({f"{key}_losses": np.array([float(loss), float(word), float(cl)]),
                        f"{key}_gnorm": np.array(float(leaf.grad.double().norm())), f"{key}_sample_idx": idx,
                        f"{key}_gsample": leaf.grad.reshape(-1)[idx].numpy()})
    gate_loss = LOSS_BAR if dev32["loss"] <= LOSS_BAR / 4 else 4 * dev32["loss"]
    gate_grad = GRAD_BAR if dev32["grad"] <= GRAD_BAR / 4 else 4 * dev32["grad"]
    fixture["loss_gate"] = np.array([gate_loss, gate_grad])
    report.append(f"specificity loss, the reference in float32 on the CPU against float64 over {len(R.LOSS_GRID)} cases: losses "
                  f"{dev32['loss']:.3e} (a quarter of LOSS_BAR is {LOSS_BAR / 4:.1e}), d logit {dev32['grad']:.3e} (a quarter "
                  f"of GRAD_BAR is {GRAD_BAR / 4:.1e}) -> the GPU tests gate at {gate_loss:.3e} / {gate_grad:.3e}")
    print(report[-1])
    fixture["coin_seed"] = np.array(TR.COIN_SEED)

    path = os.path.join(HERE, "g26_cond_attn_gru.npz")
    np.savez_compressed(path, **{k: fixture[k] for k in sorted(fixture)})
    size = os.path.getsize(path)
    assert size <= 1000000, size
    print(f"wrote {path}: {size} bytes")
    rpath, kept = os.path.join(HERE, "REPORT_cond_attn_gru.txt"), ""
    if os.path.exists(rpath):
        with open(rpath) as f:
            old = f.read()
        if REPORT_MARK in old:
            kept = old[old.index(REPORT_MARK):]
    with open(rpath, "w") as f:
        f.write("g26_cond_attn_gru.npz: candidate draws tried by make_golden_cond_attn_gru.py (torch %s)\n" % torch.__version__)
        f.write("\n".join(report) + "\n")
        f.write("max |tests/_cond_attn_gru_ref.py - reference|, float32 on the CPU\n")
        for k, v in gaps.items():
            f.write(f"  {k:52s} {v:.3e}\n")
        f.write(kept)


if __name__ == "__main__":
    main()
