"""Generate g20_attn_gru_edges.npz by running the REFERENCE's ``TemporalBahAttnDecoder.forward`` (captioning/models/
hf_wrapper.py:1513-1554, attention :1390-1414) on the CPU for single decoder steps at the length edges of the audio memory.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_attn_gru_edges.py

The stubs are those of make_golden_attn_gru.py.  The fixture stores the RECIPE, not the tensors (tests/_attn_gru_edges.py
repeats it: ``G20``, ``g20_inputs``, ``g20_step_inputs``):

  * shape: emb_dim 64, d_model 96, attn_size 160, attn_emb_dim 64, fc_emb_dim 32, V 516; weights
    ``procedural.bah_decoder_state(seed, end_scale=3.0)``;
  * memory: 5 clips x 301 frames and fc_emb from ``np.random.default_rng(seed).normal(0, 0.25, ...)``, lengths
    [301, 257, 1, 0, 306] - a full clip, one past the 256 boundary, a single frame, NO frame (the reference's softmax over
    a row of -1e10 is uniform) and a length above the frame count (the reference's mask is all-true, as for 301);
    clip 4's memory is a copy of clip 0's, so that the two rows can be compared;
  * step t = 0: the tags [0, 1, 2, 3, 0] and a zero state; step t = 3: word ids and a state in (-1, 1).

Recorded per step: ``attn_weight`` (5, 301), the new state (5, 96), the top-8 logit ids and values.  All of it is the
reference's own.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_attn_gru as G19   # noqa: E402  (its sys.path entries and stubs)

import numpy as np   # noqa: E402
import torch         # noqa: E402


def main():
    G19._install_stubs()
    torch.manual_seed(20)
    torch.set_grad_enabled(False)
    import captioning.models.hf_wrapper as hf     # reference
    import _attn_gru_edges as E
    import _attn_gru_ref as R

    sd, mem, lens, fc, tags = E.g20_inputs()
    dec = hf.TemporalBahAttnDecoder(dropout=0.5, **E.G20_SHAPE).eval()
    dec.load_state_dict(sd, strict=True)
    B = E.G20["B"]
    fixture = {"recipe_seed": np.array(E.G20["seed"]), "lens": lens.numpy(), "steps": np.array(E.G20["steps"]),
               "shape": np.array([E.G20_SHAPE[k] for k in E.KEYS])}
    for t in E.G20["steps"]:
        h, words = E.g20_step_inputs(sd, t)
        out = dec({"word": words.reshape(B, 1), "state": h.reshape(1, B, -1), "fc_emb": fc, "attn_emb": mem,
                   "attn_emb_len": lens, "temporal_tag": tags, "t": t})
        logit, state, w = out["logit"][:, 0], out["state"][0], out["attn_weight"]
        assert tuple(w.shape) == (B, E.G20["Tm"]) and torch.equal(out["embed"][:, 0], state)
        tv, ti = logit.topk(8, dim=1)
        gap = float((tv[:, 0] - tv[:, 1]).min())
        assert gap >= 1e-4, f"step {t}: top-1 / top-2 gap {gap:.2e}"
        assert float((tv[:, :-1] - tv[:, 1:]).min()) >= 1e-4, "top-8 order closer than the parity gate"
        # the restatement on the same step
        mine = R.step(sd, R.input_embed(sd, words, tags, t), h, mem, lens, fc)
        for name, a, b in (("state", state, mine[0]), ("logit", logit, mine[1]), ("attn_weight", w, mine[2])):
            d = float((a - b).abs().max())
            print(f"t={t} {name}: max |reference - restatement| {d:.3e}")
            assert d < 1e-4, (t, name, d)
        fixture.update({f"t{t}_attn_weight": w.numpy(), f"t{t}_state": state.numpy(), f"t{t}_top_val": tv.numpy(),
                        f"t{t}_top_idx": ti.numpy().astype(np.int32), f"t{t}_gap": np.array(gap)})
        print(f"t={t}: top-1 ids {ti[:, 0].tolist()} min gap {gap:.2e}; weight of the length-0 row "
              f"{float(w[3].min()):.9e}..{float(w[3].max()):.9e}")
    path = os.path.join(HERE, "g20_attn_gru_edges.npz")
    np.savez_compressed(path, **{k: fixture[k] for k in sorted(fixture)})
    size = os.path.getsize(path)
    assert size <= 60000, size
    print(f"wrote {path}: {size} bytes")


if __name__ == "__main__":
    main()
