"""Development probe: the launch trace of the caption searches (audiocaption_amd/search_state.py and its callers), the
sibling of tools/train_launch_trace.py and tools/encoder_launch_trace.py for the decode side.  Every call into the HIP
library that a search makes, in issue order, with its arguments, and the SHA-256 of every array it returns.  Each case runs
three times, so that the eager first use of a state, the capture of its graph and a replay are all crossed (a replay issues
no library call: its line of the trace holds the output hashes alone).  Two versions of the host code that write the same
file issue the same launches, in the same order, with the same arguments, and compute the same bits.

Procedural weights at the smallest shapes at which the paths differ: 3 clips of 7 memory frames with lengths (7, 4, 1),
max_length 6, beam 2, the decoder shape "S0" of tests/_decoder_shapes.py (the one the one-launch greedy search covers) with
a vocabulary of 300."""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import audiocaption_amd as A
from audiocaption_amd import _lib, procedural as Pr
from launch_trace import TracingLib, ordinals, trace

ap = argparse.ArgumentParser()
ap.add_argument("--out", default="decode_launch_trace.txt")
args = ap.parse_args()

DEV = "cuda:0"
B, TM, LENS, L, BEAM = 3, 7, [7, 4, 1], 6, 2
D, H, NL, FF, AE, V, KW = 256, 4, 2, 1024, 512, 300, 30
SEARCH = ("seq", "logit", "sampled_logprob", "embed", "unfinished_cnt", "cluster_error")


def normal(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def decoder(cls, state, **more):
    dec = cls(emb_dim=D, vocab_size=V, fc_emb_dim=AE, attn_emb_dim=AE, dropout=0.2, nhead=H, nlayers=NL, dim_feedforward=FF, **more)
    dec.load_state_dict(Pr.to_torch(state), strict=True)
    return dec.eval().to(DEV)


dec = decoder(A.TransformerDecoder, Pr.decoder_state("", V, D, AE, NL, FF, seed=5))
model = A.TransformerModel(torch.nn.Identity(), dec).eval()
other = A.TransformerModel(torch.nn.Identity(), decoder(A.TransformerDecoder, Pr.decoder_state("", V, D, AE, NL, FF, seed=8))).eval()
kdec = decoder(A.KeywordProbTransformerDecoder, Pr.keyword_decoder_state("", V, KW, D, AE, NL, FF, seed=5), keyword_classes_num=KW)
kmodel = A.KeywordCondTransformerModel(torch.nn.Identity(), kdec).eval()
ens = A.EnsembleModel([model, other])
GRU = dict(emb_dim=64, d_model=128, attn_size=96, attn_emb_dim=160, fc_emb_dim=96, vocab_size=517)
gdec = A.BahAttnCatFcDecoder(dropout=0.2, **GRU)
gdec.load_state_dict(Pr.to_torch(Pr.bah_decoder_state("", temporal=False, seed=5, **GRU)), strict=True)
gmodel = A.Seq2SeqAttnModel(torch.nn.Identity(), gdec.eval().to(DEV)).eval()

attn, attn2, attn_other = normal((B, TM, AE), 1), normal((B, TM, AE), 2), normal((B, 5, AE), 3)
keyword = (torch.rand(B, KW, generator=torch.Generator().manual_seed(4)) < 0.2).float()
word = torch.randint(3, V, (B, L), generator=torch.Generator().manual_seed(6))
word[:, 0], word[1, 4:] = 1, 0
tf = {"word": word, "cap_padding_mask": word == 0, "attn_emb": attn, "attn_emb_len": torch.tensor(LENS)}
req = {"mode": "inference", "attn_emb": attn, "attn_emb_len": LENS, "fc_emb": torch.zeros(B, 4, device=DEV), "max_length": L}
beam = {"sample_method": "beam", "beam_size": BEAM, "n_best": True, "n_best_size": BEAM}
encs = [{"attn_emb": attn, "attn_emb_len": LENS}, {"attn_emb": attn_other, "attn_emb_len": [5, 2, 1]}]
greq = {"mode": "inference", "attn_emb": normal((B, TM, GRU["attn_emb_dim"]), 7), "attn_emb_len": LENS,
        "fc_emb": normal((B, GRU["fc_emb_dim"]), 9), "max_length": L}

CASES = [
    ("greedy chain", SEARCH, lambda: dec.greedy(attn, LENS, L, 1, 2, 0, mode="chain")),
    ("greedy cluster", SEARCH, lambda: dec.greedy(attn, LENS, L, 1, 2, 0, mode="cluster")),
    ("greedy two batches, one chain", SEARCH, lambda: dec.greedy([attn, attn2], [LENS, [2, 7, 5]], L, 1, 2, 0, mode="chain")),
    ("sample top5", SEARCH, lambda: model(dict(req, sample_method="top5", temp=0.8, seed=11))),
    ("beam n_best", ("seq",), lambda: model(dict(req, **beam))),
    ("forward", ("embed", "logit"), lambda: dec(tf)),
    ("keyword greedy", SEARCH, lambda: kmodel(dict(req, keyword=keyword))),
    ("keyword sample top5", SEARCH, lambda: kmodel(dict(req, keyword=keyword, sample_method="top5", seed=11))),
    ("keyword beam n_best", ("seq",), lambda: kmodel(dict(req, keyword=keyword, **beam))),
    ("keyword forward", ("embed", "logit"), lambda: kdec(dict(tf, keyword=keyword))),
    ("ensemble greedy", ("seq", "sampled_logprob"), lambda: ens.decode(encs, sample_method="greedy", max_length=L)),
    ("ensemble beam n_best", ("seq", "score"), lambda: ens.decode(encs, max_length=L, **beam)),
    ("attention-GRU beam n_best", ("seq", "attn_weight"), lambda: gmodel(dict(greq, **beam))),
]

_lib._lib = TracingLib(_lib.load())   # what every later _lib.load() returns

# An ordinal stands for an address, so a buffer freed inside a call must not hand its address to the next one made there:
# every tensor of the factory functions the searches allocate with stays alive until the use is over.
alive = []
for _name in ("empty", "zeros", "full", "empty_like"):
    def _keep(*a, _make=getattr(torch, _name), **kw):
        alive.append(_make(*a, **kw))
        return alive[-1]
    setattr(torch, _name, _keep)

lines = []
for name, keys, run in CASES:
    for use in range(3):
        del trace[:], alive[:]
        ordinals.clear()              # one use's records do not depend on the uses and cases before it
        out = run()
        torch.cuda.synchronize()
        lines.append(f"# {name}, use {use + 1}")
        lines += trace
        for k in keys:
            if k in out:
                t = out[k].detach().cpu().contiguous()
                lines.append(f"{k} {t.dtype} {tuple(t.shape)} {hashlib.sha256(t.numpy().tobytes()).hexdigest()}")
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
print(f"{len(CASES)} cases x 3 uses: {len(lines)} lines, sha256 {hashlib.sha256(text.encode()).hexdigest()} -> {args.out}")
