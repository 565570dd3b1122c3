"""Generate g14_sampling.npz by running the REFERENCE's ``CaptionModel.sample_next_word`` (base.py:214-252) on CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_sampling.py

Eight logit rows at V = 4981 (near-ties at the top-k / top-p boundaries, a peaked row, flat and wide rows) are sampled with
"sample" at temp 0.7, "top5", "top50", "top0.5", "top0.9" and "gumbel", one row at a time (B = 1: the reference's gumbel
branch stores a [N, 1] gather and fails for larger batches).  ``torch.distributions.Categorical`` is wrapped to record the
logits the reference hands it, so the fixture holds the distribution each rule produced, the drawn word and the stored
``probs``.  Gumbel-max takes no Categorical: its distribution is softmax(log_softmax(logit)), recorded as such.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")

import numpy as np
import torch

from captioning.models.base import CaptionModel  # noqa: E402  (reference)

V = 4981
METHODS = [("sample", 0.7), ("top5", 1.0), ("top50", 1.0), ("top0.5", 1.0), ("top0.9", 1.0), ("gumbel", 1.0)]


def make_rows():
    g = np.random.default_rng(14)
    rows = []
    rows.append(g.normal(0, 3.0, V))                      # wide
    rows.append(g.normal(0, 1.0, V))                      # flat
    r = g.normal(0, 2.0, V)
    r[17] = r.max() + 12.0                                # peaked: one word holds ~all the mass
    rows.append(r)
    r = g.normal(0, 2.5, V)                               # exact ties at the 5th / 50th place
    order = np.argsort(-r, kind="stable")
    r[order[5]] = r[order[4]]
    r[order[50]] = r[order[49]]
    rows.append(r)
    r = g.normal(0, 2.5, V)                               # near-ties (1e-3) around the top-k boundaries
    order = np.argsort(-r, kind="stable")
    r[order[5]] = r[order[4]] - 1e-3
    r[order[50]] = r[order[49]] - 1e-3
    rows.append(r)
    r = np.full(V, -8.0) + g.normal(0, 0.01, V)           # a few strong words over a low floor: top-p cuts inside them
    r[[3, 900, 901, 4000]] = [3.0, 2.9, 2.9, 2.0]          # 900 / 901 tie exactly at the top0.5 cut
    rows.append(r)
    rows.append(g.normal(0, 4.0, V))                      # very wide
    r = g.normal(0, 3.0, V)
    r[[10, 11, 12]] = r.max() + 0.5                       # three equal maxima
    rows.append(r)
    return np.stack(rows).astype(np.float32)


def main():
    logits = make_rows()
    captured = []
    real = torch.distributions.Categorical

    class Recording(real):
        def __init__(self, probs=None, logits=None, validate_args=None):
            captured.append(logits.detach().clone())
            super().__init__(probs=probs, logits=logits, validate_args=validate_args)

    torch.distributions.Categorical = Recording
    torch.manual_seed(1414)
    out = {"logits": logits, "methods": np.array([m for m, _ in METHODS]), "temps": np.array([t for _, t in METHODS])}
    dist = np.zeros((len(METHODS), logits.shape[0], V), dtype=np.float32)
    word = np.zeros((len(METHODS), logits.shape[0]), dtype=np.int64)
    probs = np.zeros((len(METHODS), logits.shape[0]), dtype=np.float32)
    try:
        for mi, (method, temp) in enumerate(METHODS):
            for r in range(logits.shape[0]):
                captured.clear()
                res = CaptionModel.sample_next_word(None, torch.from_numpy(logits[r:r + 1]), method, temp)
                if method == "gumbel":
                    d = torch.log_softmax(torch.from_numpy(logits[r:r + 1]), 1)
                else:
                    assert len(captured) == 1
                    d = captured[0]
                dist[mi, r] = d[0].numpy()
                word[mi, r] = int(res["word"][0])
                probs[mi, r] = float(res["probs"].reshape(-1)[0])
    finally:
        torch.distributions.Categorical = real
    out.update(dist_logits=dist, word=word, probs=probs)
    path = os.path.join(HERE, "g14_sampling.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {logits.shape[0]} rows x {len(METHODS)} methods")


if __name__ == "__main__":
    main()
