"""Decoder shapes, procedural draws and float64 references shared by tests/test_decoder_shapes_cpu.py (the guards, no GPU)
and tests/test_gpu_decoder_shapes.py (the kernels of csrc/decoder.hip).  A helper module, not a conftest.

Every reference is ``oracle.cpu_path`` evaluated on the state cast to float64; each is computed once per process
(functools.lru_cache) and must be left unchanged by its readers.

The seeds of the searches below were found on the CPU (float64 oracle) so that no step has a near tie; the guards in
tests/test_decoder_shapes_cpu.py re-assert that, so an id comparison on the GPU is meaningful."""
import functools

import numpy as np
import torch

from oracle import cpu_path as O

END, PAD, START = O.END_IDX, O.PAD_IDX, O.START_IDX

# id -> (d_model, nhead, nlayers, dim_ff, attn_emb_dim, vocabulary) and what the shape reaches in csrc/decoder.hip
SHAPES = {
    "S0": (256, 4, 2, 1024, 512, 300),     # the fused per-row kernels; with AUDIOCAPTION_DEC_ROW=gemm the general sequence
    "S1": (64, 1, 1, 256, 32, 300),        # one head, one layer, KC = 64 / nsteps = 1, smallest attn_emb_dim
    "S2": (128, 4, 3, 512, 96, 300),       # hd = 32 branch, odd layer count (buffer ping-pong), attn_emb_dim % 64 != 0
    "S3": (192, 12, 2, 512, 64, 300),      # hd = 16, nsteps = 3, nf = 3
    "S4": (512, 8, 2, 2048, 256, 300),     # DEC_MAX_D, hd == 64 without fusion, dim_ff of four K chunks
    "S5": (384, 6, 8, 1536, 128, 300),     # AC_MAX_LAYERS
    "S6": (256, 8, 2, 1024, 512, 4981),    # d 256 but not 4 heads: leaves the fused route; vocabulary % 16 != 0
}
FUSED = {"S0"}                             # decoder_step: d_model 256 and 4 heads, unless AUDIOCAPTION_DEC_ROW=gemm

# teacher-forced forward (3a): memory frames per shape, lengths [Tm, Tm // 2, 1]
TF_TM = {"S0": 40, "S6": 40, "S2": 33, "S4": 33, "S1": 5, "S3": 9, "S5": 17}
TF_SEED = 1234                             # procedural.BASE_SEED: the plain draw of the g3 fixture, at each shape
LOGIT_BAR = 1e-4                           # tests/test_gpu_model.py test_g3_decoder_forward_vs_reference_golden
MARGIN = 1e-3                              # 10 x the logit bar: below it an id is not a meaningful comparison

# greedy past 32 positions (3c): case -> (shape, seed, AUDIOCAPTION_DEC_ROW or None); end_beta -3: no row ends
GREEDY_LEN, GREEDY_LENS, GREEDY_TM = 48, (20, 13, 6, 1), 20
GREEDY_CASES = {
    "S0": ("S0", 5, None),
    "S0-gemm": ("S0", 8, "gemm"),
    "S2": ("S2", 7, None),
    "S4": ("S4", 7, None),
    "S6": ("S6", 325, None),
}
# early stop among long rows (3d): case -> (shape, seed, end_beta)
STOP_CASES = {
    "S0": ("S0", 5, 1.0),
    "S2": ("S2", 3, 1.5),
}
# beam search (3e): case -> (shape, seed); beam 3, 40 steps, temperature 1, 2 clips
BEAM, BEAM_LEN, BEAM_LENS, BEAM_TM = 3, 40, (20, 9), 20
BEAM_CASES = {
    "S2": ("S2", 325),
    "S4": ("S4", 11),
}


def oracle_kw(sid):
    d, h, nl, ff, A_, V = SHAPES[sid]
    return {"nlayers": nl, "nhead": h}


def f64(state):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}


@functools.lru_cache(maxsize=None)
def plain_state(sid, seed=TF_SEED):
    """``procedural.decoder_state`` at the shape (float32 torch tensors under ``decoder.``)."""
    from audiocaption_amd import procedural as P
    d, h, nl, ff, A_, V = SHAPES[sid]
    return P.to_torch(P.decoder_state("decoder.", V, d, A_, nl, ff, seed=seed))


@functools.lru_cache(maxsize=None)
def diverse_state(sid, seed, end_beta=-3.0, emb_scale=3.0, pe_scale=4.0):
    """The high-entropy draw of ``procedural.decoder_state_diverse`` at the shape: embedding x 3, positional encoding x 4,
    the <end> row aligned with the last norm3.bias at ``end_beta`` (-3: <end> never wins; positive: rows end at different
    steps)."""
    from audiocaption_amd import procedural as P
    d, h, nl, ff, A_, V = SHAPES[sid]
    st = P.decoder_state("decoder.", V, d, A_, nl, ff, seed=seed)
    st["decoder.word_embedding.weight"] = st["decoder.word_embedding.weight"] * np.float32(emb_scale)
    st["decoder.pos_encoder.pe"] = st["decoder.pos_encoder.pe"] * np.float32(pe_scale)
    b3 = st[f"decoder.model.layers.{nl - 1}.norm3.bias"]
    cw = st["decoder.classifier.weight"].copy()
    cw[END] = ((end_beta / float(np.dot(b3, b3))) * b3).astype(np.float32)
    st["decoder.classifier.weight"] = cw
    return P.to_torch(st)


def memory(sid, rows, Tm, seed=0):
    """Audio features (rows, Tm, attn_emb_dim), float32 standard normal draws."""
    g = torch.Generator().manual_seed(1000 * seed + Tm)
    return torch.randn(rows, Tm, SHAPES[sid][4], generator=g)


def tf_inputs(sid, T, Tm, N=3, lens=None):
    """Teacher-forced inputs: random words in [3, V) behind <start>; row 1 padded from T // 2 on, row 2 (when there is one)
    with pads at positions 5-8 only, so masked keys sit inside and beyond the 32 prefetched keys of the self-attention."""
    V = SHAPES[sid][5]
    g = torch.Generator().manual_seed(T * 131 + Tm)
    word = torch.randint(3, V, (N, T), generator=g)
    word[:, 0] = START
    if N > 1 and T >= 4:
        word[1, T // 2:] = PAD
    if N > 2 and T >= 10:
        word[2, 5:9] = PAD
    lens = torch.tensor([Tm, max(1, Tm // 2), 1][:N] if lens is None else lens, dtype=torch.int64)
    return {"word": word, "cap_padding_mask": word == PAD, "attn_emb": memory(sid, N, Tm), "attn_emb_len": lens}


@functools.lru_cache(maxsize=None)
def tf_reference(sid, T, Tm, N=3, lens=None):
    """(inputs, float64 reference {"embed", "logit"}) of ``tf_inputs`` on ``plain_state``."""
    inp = tf_inputs(sid, T, Tm, N, lens)
    ref = O.decoder_forward(f64(plain_state(sid)), inp["word"], inp["attn_emb"].double(), inp["attn_emb_len"],
                            inp["cap_padding_mask"], **oracle_kw(sid))
    return inp, ref


def _search_memory(sid, lens, Tm, seed):
    return memory(sid, len(lens), Tm, seed), torch.tensor(lens, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def greedy_reference(sid, seed, end_beta=-3.0):
    """(attn_emb, lens, float64 ``O.greedy_decode`` over GREEDY_LEN steps) of the diverse draw."""
    emb, lens = _search_memory(sid, GREEDY_LENS, GREEDY_TM, seed)
    out = O.greedy_decode(f64(diverse_state(sid, seed, end_beta)), emb.double(), lens, GREEDY_LEN, **oracle_kw(sid))
    return emb, lens, out


def greedy_facts(out):
    """What the guards ask of a float64 greedy search: per-row steps before <end>, the oracle's unfinished count per step,
    distinct tokens per row, and the smallest top-1 margin over the steps of rows that had not ended."""
    seq, steps = out["seq"], out["steps"]
    L = seq.shape[1]
    ended = (seq == END).long().cumsum(1) > 0
    run_len = (~ended).sum(1)                                     # tokens before <end>
    live = torch.ones_like(ended)
    live[:, 1:] = ~ended[:, :-1]                                  # rows that had not ended before step t
    live[:, steps:] = False
    cnt = torch.zeros(L, dtype=torch.int64)
    cnt[:steps] = (~ended[:, :steps]).sum(0)
    top2 = out["logit"].topk(2, -1).values
    gap = (top2[..., 0] - top2[..., 1])[live]
    distinct = [len(set(seq[r, :int(run_len[r])].tolist())) for r in range(seq.shape[0])]
    return {"run_len": run_len.tolist(), "cnt": cnt, "distinct": distinct, "margin": float(gap.min()), "live": live}


@functools.lru_cache(maxsize=None)
def beam_reference(sid, seed):
    """(attn_emb, lens, float64 ``O.beam_search`` result, its trace) of the diverse draw with end_beta -3."""
    emb, lens = _search_memory(sid, BEAM_LENS, BEAM_TM, seed)
    trace = []
    out = O.beam_search(f64(diverse_state(sid, seed)), emb.double(), lens, BEAM, BEAM_LEN, 1.0, trace=trace,
                        **oracle_kw(sid))
    return emb, lens, out, trace


def product_decoder(sid, state=None, **over):
    """``audiocaption_amd.TransformerDecoder`` at the shape (CPU, eval), with ``state`` loaded when given."""
    import audiocaption_amd as A
    d, h, nl, ff, A_, V = SHAPES[sid]
    kw = dict(emb_dim=d, vocab_size=V, fc_emb_dim=A_, attn_emb_dim=A_, dropout=0.2, nhead=h, nlayers=nl, dim_feedforward=ff)
    kw.update(over)
    dec = A.TransformerDecoder(**kw)
    if state is not None:
        dec.load_state_dict({k[len("decoder."):]: v for k, v in state.items()}, strict=True)
    return dec.eval()


def product_model(sid, state):
    """Decoder-only product model on cuda:0, as tests/test_gpu_decode_select.py::_model builds it."""
    import audiocaption_amd as A
    from audiocaption_amd import build
    build.build()
    return A.TransformerModel(torch.nn.Identity(), product_decoder(sid, state)).eval().to("cuda:0")


# shapes the decode step does not run (3f): constructor arguments replacing S0's, and what the refusal must name
REFUSED = {
    "d768": (dict(emb_dim=768, nhead=12, dim_feedforward=3072), "exceeds 512"),
    "d96": (dict(emb_dim=96, nhead=None, dim_feedforward=None), "emb_dim 96 is not a multiple of 64"),
    "d192-ff768": (dict(emb_dim=192, nhead=3, dim_feedforward=None), "dim_feedforward 768"),
    "d320-ff1280": (dict(emb_dim=320, nhead=5, dim_feedforward=None), "dim_feedforward 1280"),
    "d256-h2": (dict(emb_dim=256, nhead=2), "head width"),
    "nlayers9": (dict(nlayers=9), "nlayers 9"),
}


def refused_decoder(name):
    """The product decoder of REFUSED[name] (CPU): S0 with the listed constructor arguments replaced; None leaves the
    constructor's default (nhead = emb_dim // 64, dim_feedforward = 4 x emb_dim)."""
    import audiocaption_amd as A
    over = dict(REFUSED[name][0])
    d, h, nl, ff, A_, V = SHAPES["S0"]
    kw = dict(emb_dim=d, vocab_size=50, fc_emb_dim=A_, attn_emb_dim=64, dropout=0.2, nhead=h, nlayers=nl, dim_feedforward=ff)
    kw.update(over)
    kw = {k: v for k, v in kw.items() if v is not None}
    return A.TransformerDecoder(**kw).eval()
