"""Generate g19_attn_gru.npz by running the REFERENCE's attention-GRU captioners on CPU: ``TemporalSeq2SeqAttnModel`` over
``TemporalBahAttnDecoder`` and ``Seq2SeqAttnModel`` over ``BahAttnCatFcDecoder`` (captioning/models/hf_wrapper.py:1377-1788,
the same code as captioning/models/rnn_decoder.py and attn_model.py), encoder ``nn.Identity()``, fed encoder outputs.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_attn_gru.py

``hf_wrapper.py`` imports under the inert stubs of make_golden.py once ``transformers`` has been imported first and an
inert ``efficientnet_pytorch`` stub is added.  The fixture stores the RECIPE, not the tensors:

  * weights: ``procedural.bah_decoder_state`` with the stored (seed, end_scale) per case;
  * "pub" (the published shape, E = d = attn_size = 512, V 4981): memory g3_decoder.npz's attn_emb (4 x 31 x 512, its own
    lengths), fc_emb its mean over the valid frames, temporal_tag [0, 1, 2, 3];
  * "small" (emb_dim 64, d_model 128, attn_size 96, attn_emb_dim 160, fc_emb_dim 96, V 517): 5 clips x 70 frames drawn
    from ``small_memory()``, lengths [70, 65, 64, 33, 1], fc_emb the first 96 features of the mean over the valid frames,
    temporal_tag [0, 1, 2, 3, 0];
  * each shape with the temporal model ("t") and the plain one ("p").

Weight draws are tried in order until the reference's own outputs make a test that can fail (asserted below): no caption
is <end> alone; greedy rows end at different steps and at least one ends early; one beam-3 clip exits early and one runs
to max_length; changing the clips' tags changes at least one caption; every greedy top-1 / top-2 gap on a live step and
every beam margin at the cut is >= 1e-4.  tests/_attn_gru_ref.py is compared with the reference here as well.

What is the reference's own: every id; the greedy values, top-8 logits, the two logit columns, attention weights and
the final state; the beam attention weights of the columns its search wrote (its buffers are zero-filled here instead of
``torch.empty``, by a subclass that changes nothing else); the sampling distributions and stored values.  The beam
margins are the restatement's (the reference does not expose its candidates).
"""
import os
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

import numpy as np
import torch
import torch.nn as nn

MAXLEN = 20
GATE = 1e-4
LOGIT_COLS = [2, 311]
SHAPES = {
    "pub": dict(emb_dim=512, d_model=512, attn_size=512, attn_emb_dim=512, fc_emb_dim=512, vocab_size=4981),
    "small": dict(emb_dim=64, d_model=128, attn_size=96, attn_emb_dim=160, fc_emb_dim=96, vocab_size=517),
}
SMALL_LENS, SMALL_SEED = [70, 65, 64, 33, 1], 19
CANDIDATES = [(seed, bias) for seed in (19, 20, 21, 22, 23, 24, 25, 26) for bias in (3.0, 2.5, 3.5, 2.0, 4.0)]
SAMPLE_CASES = [("sample", 0.7), ("top5", 0.7), ("top0.9", 1.0), ("gumbel", 1.0)]
SAMPLE_ROWS, SAMPLE_SEED = 3, 19
REPORT_MARK = "==== gates and measured figures"


def small_memory():
    """The audio memory of the small shape (5 x 70 x 160): a recipe the tests repeat."""
    return np.random.default_rng(SMALL_SEED).normal(0.0, 0.25, (5, 70, 160)).astype(np.float32)


def sample_logits(V=4981):
    return np.random.default_rng(SAMPLE_SEED).normal(0.0, 2.5, (SAMPLE_ROWS, V)).astype(np.float32)


def inputs_of(shape):
    """(attn_emb, lens, fc_emb, tags) of a shape, as torch CPU tensors."""
    if shape == "pub":
        g3 = np.load(os.path.join(HERE, "g3_decoder.npz"))
        mem, lens = g3["attn_emb"], g3["attn_emb_len"].astype(np.int64)
        tags = [0, 1, 2, 3]
    else:
        mem, lens, tags = small_memory(), np.array(SMALL_LENS, dtype=np.int64), [0, 1, 2, 3, 0]
    mem_t, lens_t = torch.from_numpy(mem), torch.from_numpy(lens)
    valid = (torch.arange(mem_t.shape[1])[None, :] < lens_t[:, None]).float()
    fc = (mem_t * valid[:, :, None]).sum(1) / lens_t[:, None].float()      # mean_with_lens
    fc = fc[:, :SHAPES[shape]["fc_emb_dim"]].contiguous()                  # small: the first fc_emb_dim features of it
    return mem_t, lens_t, fc, torch.tensor(tags, dtype=torch.long)


def _install_stubs():
    # before the stubs: transformers loads these lazily and looks the stubbed packages up while it does
    from transformers import PretrainedConfig, PreTrainedModel  # noqa: F401
    from make_golden import _install_stubs as base
    base()

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    eff = mod("efficientnet_pytorch", EfficientNet=object)
    eff.utils = mod("efficientnet_pytorch.utils", get_model_params=lambda *a, **k: None,
                    efficientnet_params=lambda *a, **k: None)


def main():
    _install_stubs()
    torch.manual_seed(19)
    torch.set_grad_enabled(False)
    import captioning.models.hf_wrapper as hf     # reference
    from audiocaption_amd import procedural as P
    import _attn_gru_ref as R
    import _sampling_ref as SR

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

    def build(shape, temporal, seed, bias):
        kw = SHAPES[shape]
        sd = P.to_torch(P.bah_decoder_state(temporal=temporal, seed=seed, end_scale=bias, **kw))
        dcls = hf.TemporalBahAttnDecoder if temporal else hf.BahAttnCatFcDecoder
        mcls = hf.TemporalSeq2SeqAttnModel if temporal else hf.Seq2SeqAttnModel
        dec = dcls(dropout=0.5, **kw)
        dec.load_state_dict(sd, strict=True)
        return zero_filled(mcls)(nn.Identity(), dec).eval(), sd, dec

    def run(model, shape, tags, **args):
        mem, lens, fc, _ = inputs_of(shape)
        d = {"mode": "inference", "attn_emb": mem, "attn_emb_len": lens, "fc_emb": fc, "max_length": MAXLEN}
        if tags is not None:
            d["temporal_tag"] = tags
        d.update(args)
        return model(d)

    def caps(seq):
        return [tuple(r[:R.first_end(r)]) for r in seq.tolist()]

    def try_case(shape, temporal, seed, bias):
        model, sd, _ = build(shape, temporal, seed, bias)
        mem, lens, fc, tags = inputs_of(shape)
        tags = tags if temporal else None
        B = mem.shape[0]
        out = {}
        # ---- greedy ----
        ref = run(model, shape, tags, sample_method="greedy")
        mine = R.greedy(sd, mem, lens, fc, tags, MAXLEN)
        rc = caps(ref["seq"])
        assert rc == caps(mine["seq"]), ("restatement differs from the reference (greedy)", rc, caps(mine["seq"]))
        if any(c == (2,) for c in rc):
            return None, "a greedy caption is <end> alone"
        ends = [len(c) for c in rc if c[-1] == 2]
        if not ends or len(set(len(c) for c in rc)) < 2 or min(ends) >= MAXLEN:
            return None, f"greedy: rows do not end at different steps with one early ({[len(c) for c in rc]})"
        live = torch.from_numpy(R.live_mask(ref["seq"].numpy()))
        tv, ti = ref["logit"].topk(8, dim=2)
        gap = float((tv[..., 0] - tv[..., 1])[live].min())
        if gap < GATE:
            return None, f"greedy top-1 / top-2 gap {gap:.2e}"
        for k_, a, b in (("logit", ref["logit"], mine["logit"]), ("attn_weight", ref["attn_weight"].transpose(1, 2),
                                                                 mine["attn_weight"].transpose(1, 2)),
                         ("embed", ref["embed"], mine["embed"]), ("value", ref["sampled_logprob"], mine["sampled_logprob"])):
            dmax = float((a[live] - b[live]).abs().max())
            assert dmax < 1e-4, ("restatement differs from the reference (greedy)", k_, dmax)
        assert float((ref["state"] - mine["state"]).abs().max()) < 1e-4
        assert int(ref["seq"].shape[1]) == MAXLEN and mine["steps"] == max(len(c) for c in rc)
        lv = live.numpy()
        def kept(x, m):   # the reference's columns of steps it never ran are torch.empty garbage (NaN included)
            return torch.where(m, x, torch.zeros((), dtype=x.dtype)).numpy()

        out.update(greedy_seq=mine["seq"].numpy(), greedy_value=kept(ref["sampled_logprob"], live),
                   greedy_top_val=kept(tv, live[..., None]), greedy_top_idx=kept(ti, live[..., None]).astype(np.int32),
                   greedy_logit_cols=kept(ref["logit"][:, :, LOGIT_COLS], live[..., None]),
                   greedy_attn_weight=kept(ref["attn_weight"], live[:, None, :]), greedy_state=ref["state"].numpy(),
                   greedy_gap=np.array(gap), greedy_live=lv)
        msg = [f"greedy lengths {[len(c) for c in rc]} min gap {gap:.2e}"]
        if temporal:
            other = caps(run(model, shape, tags.roll(1), sample_method="greedy")["seq"])
            if other == rc:
                return None, "changing the tags changes no caption"
        # ---- beam 3 / 4 ----
        for k in (3, 4):
            ref_b = run(model, shape, tags, sample_method="beam", beam_size=k)
            ref_nb = run(model, shape, tags, sample_method="beam", beam_size=k, n_best=True, n_best_size=k)
            trace = []
            my_b = R.beam_search(sd, mem, lens, fc, tags, k, MAXLEN, trace=trace)
            my_nb = R.beam_search(sd, mem, lens, fc, tags, k, MAXLEN, n_best=True, n_best_size=k)
            assert torch.equal(ref_b["seq"], my_b["seq"]), ("restatement differs from the reference (beam)", k)
            assert torch.equal(ref_nb["seq"], my_nb["seq"]), ("restatement differs from the reference (n-best)", k)
            dmax = float((ref_b["attn_weight"] - my_b["attn_weight"]).abs().max())
            assert dmax < 1e-4, ("restatement differs from the reference (beam attn_weight)", k, dmax)
            bc = caps(ref_b["seq"])
            if any(c == (2,) for c in bc):
                return None, f"a beam {k} caption is <end> alone"
            margin = min(r["margin"] for r in trace)
            if margin < GATE:
                return None, f"beam {k} margin {margin:.2e}"
            steps = [max(r["t"] for r in trace if r["clip"] == i) + 1 for i in range(B)]
            if k == 3 and not (min(steps) < MAXLEN and max(steps) == MAXLEN):
                return None, f"beam 3: no clip exits early or none runs to max_length (steps {steps})"
            if k == 3 and not any(r["prev_beam"] != list(range(k)) for r in trace if r["t"] > 0):
                return None, "beam 3: the parent beams never change"
            out[f"beam{k}_seq"] = ref_b["seq"].numpy()
            out[f"beam{k}_nbest"] = ref_nb["seq"].numpy()
            out[f"beam{k}_attn_weight"] = ref_b["attn_weight"].numpy()
            out[f"beam{k}_margin"] = np.array(margin)
            out[f"beam{k}_steps"] = np.array(steps)
            msg.append(f"beam {k} steps {steps} margin {margin:.2e}")
        return out, "; ".join(msg)

    fixture, report = {}, []
    for shape in SHAPES:
        for temporal in (True, False):
            tag = f"{shape}_{'t' if temporal else 'p'}"
            for seed, bias in CANDIDATES:
                out, why = try_case(shape, temporal, seed, bias)
                line = f"{tag} seed {seed} end_scale {bias}: " + ("USED: " if out is not None else "rejected: ") + why
                print(line)
                report.append(line)
                if out is not None:
                    break
            assert out is not None, f"{tag}: no candidate draw makes a fixture that can fail"
            fixture.update({f"{tag}_{k}": v for k, v in out.items()})
            fixture[f"{tag}_recipe"] = np.array([seed, bias], dtype=np.float64)

    # ---- the reference's key list and shapes (temporal decoder, published shape) ----
    _, _, dec = build("pub", True, *CANDIDATES[0])
    keys = list(dec.state_dict().keys())
    fixture["state_keys"] = np.array(keys)
    fixture["state_shapes"] = np.array([",".join(str(v) for v in dec.state_dict()[k].shape) for k in keys])

    # ---- sampling rules (base.py:214-252) on fixed logits, one case per method ----
    model, _, _ = build("small", True, *CANDIDATES[0])
    logits = torch.from_numpy(sample_logits())
    real = torch.distributions.Categorical
    captured = []

    class Recording(real):
        def __init__(self, probs=None, logits=None, validate_args=None):
            captured.append(logits.detach().clone())
            super().__init__(probs=probs, logits=logits, validate_args=validate_args)

    V = logits.shape[1]
    dist = np.zeros((len(SAMPLE_CASES), SAMPLE_ROWS, V), dtype=np.float32)
    word = np.zeros((len(SAMPLE_CASES), SAMPLE_ROWS), dtype=np.int64)
    value = np.zeros((len(SAMPLE_CASES), SAMPLE_ROWS), dtype=np.float32)
    torch.distributions.Categorical = Recording
    try:
        for ci, (method, temp) in enumerate(SAMPLE_CASES):
            for row in range(SAMPLE_ROWS):   # one row at a time: the gumbel branch gathers [N, 1]
                captured.clear()
                res = model.sample_next_word(logits[row:row + 1].clone(), method, temp)
                lp = torch.log_softmax(logits[row:row + 1], 1)
                d = lp if method == "gumbel" else captured[0]   # argmax(lp + Gumbel) draws from softmax(lp)
                w = int(res["word"][0])
                dist[ci, row], word[ci, row], value[ci, row] = d[0].numpy(), w, float(res["probs"].reshape(-1)[0])
                code, k, p = R.parse_method(method)
                wts, stored, _ = SR.distribution(logits[row].numpy(), code, k, p, temp)
                assert np.array_equal(wts > 0, np.isfinite(dist[ci, row])), (method, row)
                assert abs(stored[w] - value[ci, row]) < 1e-5, (method, row, stored[w], value[ci, row])
    finally:
        torch.distributions.Categorical = real
    fixture.update(sample_methods=np.array([m for m, _ in SAMPLE_CASES]), sample_temps=np.array([t for _, t in SAMPLE_CASES]),
                   sample_recipe=np.array([SAMPLE_ROWS, SAMPLE_SEED]), sample_dist=dist, sample_word=word, sample_value=value)
    fixture.update(max_length=np.array(MAXLEN), logit_cols=np.array(LOGIT_COLS), small_lens=np.array(SMALL_LENS),
                   small_seed=np.array(SMALL_SEED))

    path = os.path.join(HERE, "g19_attn_gru.npz")
    np.savez_compressed(path, **{k: fixture[k] for k in sorted(fixture)})
    size = os.path.getsize(path)
    assert size <= 1000000, size
    print(f"wrote {path}: {size} bytes")
    # the candidate list is rewritten; the section with the gates and a GPU run's figures (REPORT_MARK on) is kept
    rpath, kept = os.path.join(HERE, "REPORT_attn_gru.txt"), ""
    if os.path.exists(rpath):
        with open(rpath) as f:
            old = f.read()
        if REPORT_MARK in old:
            kept = old[old.index(REPORT_MARK):]
    with open(rpath, "w") as f:
        f.write("g19_attn_gru.npz: candidate draws tried by make_golden_attn_gru.py\n" + "\n".join(report) + "\n" + kept)


if __name__ == "__main__":
    main()
