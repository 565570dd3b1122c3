"""Case table, input recipes and a mirror of the GEMM dispatch for the attention-GRU decoder's edge tests
(tests/test_gpu_attn_gru_edges.py, tests/test_attn_gru_edges_cpu.py, tests/golden/make_golden_attn_gru_edges.py).

A case is a decoder shape, a batch of audio memory and its lengths.  Weights come from ``procedural.bah_decoder_state``
with the case's seed and end_scale 3.0; memory, fc_emb (and random lengths) from ``np.random.default_rng(seed)`` in that
order; tags are ``arange(B) % 4``.  Seeds are the first, counted up from 31, at which the CPU restatement makes the test
one that can fail (tools: ``python tests/_attn_gru_edges.py`` prints the search):

  * ``seed``: the f32 and float64 restatements pick identical greedy ids at every max_length the tests decode, the
    smallest top-1 / top-2 gap on a live step is >= 1e-4 and no caption is <end> alone;
  * ``beam_seed[(beam, temp)]``: f32 and float64 beam ids agree and every margin at the cut is >= 1e-4.  ``beam_L`` is
    the max_length of the beam test where it is not ``L``: routes-1 searches 264 rows over a vocabulary of 8201, and the
    smallest of its 66 x 20 margins stayed under 1e-4 for every seed from 31 to 43; 9 steps still pass the host's first
    poll (t = 8).
"""
import numpy as np
import torch

import _attn_gru_ref as R
from audiocaption_amd import procedural as P

END_SCALE = 3.0
GATE = 1e-4
KEYS = ("emb_dim", "d_model", "attn_size", "attn_emb_dim", "fc_emb_dim", "vocab_size")


def _shape(E, d, S, A, F, V):
    return dict(zip(KEYS, (E, d, S, A, F, V)))


# dims (E, d, S, A, F, V), clips x frames, lengths (None: drawn in 1..Tm), max_length of the greedy test.
# The last clip of routes-1 and routes-2 is full: the last rows of the key projection (the ragged last row tile of routes-1)
# are then read by the attention kernel.
# routes-1: V is 8201, not 8200 - with V a multiple of 4 every logit + t * V is 16-byte aligned; with V odd the base of an
# odd step is 4-byte aligned only, which is the layout the case is there for (the tile counts are the same: 129 x 64).
CASES = {
    "narrow": dict(shape=_shape(32, 32, 32, 32, 32, 33), B=3, Tm=5, lens=[5, 1, 0], L=20, seed=35,
                   beam_seed={(1, 1.0): 31, (2, 1.0): 31, (8, 1.0): 31}),
    "long": dict(shape=_shape(64, 96, 160, 64, 32, 516), B=4, Tm=301, lens=[301, 257, 256, 0], L=20, seed=32,
                 beam_seed={(1, 1.0): 31, (2, 1.0): 31, (8, 1.0): 32, (3, 0.7): 31, (3, 1.0): 31}),
    "full": dict(shape=_shape(32, 64, 64, 32, 32, 130), B=2, Tm=2048, lens=[2048, 1025], L=20, seed=31, beam_seed={}),
    "wide": dict(shape=_shape(1024, 1024, 1024, 1024, 1024, 16384), B=2, Tm=9, lens=[9, 4], L=20, seed=31, beam_seed={}),
    "routes-1": dict(shape=_shape(64, 64, 128, 96, 64, 8201), B=66, Tm=130, lens=[None] * 65 + [130], L=20, seed=34,
                     beam_seed={(4, 1.0): 33}, beam_L=9),
    "routes-2": dict(shape=_shape(32, 32, 128, 32, 32, 130), B=32, Tm=2048,
                     lens=[2048, 0, 1, 2047, 1024, 1025, 255, 257] + [None] * 23 + [2048], L=4, seed=44, beam_seed={}),
}
MAX_LENGTHS = (1, 23)            # "long" at these lengths as well (greedy, beam 3, one sampling method at 23)

# the decoder step of tests/golden/g20_attn_gru_edges.npz: the "long" shape, its own memory and lengths
G20_SHAPE = CASES["long"]["shape"]
G20 = dict(B=5, Tm=301, lens=[301, 257, 1, 0, 306], seed=20, steps=(0, 3))


def load_g20():
    import os
    return dict(np.load(os.path.join(R.GOLDEN, "g20_attn_gru_edges.npz")))


def inputs(shape, B, Tm, lens, seed, temporal=True):
    """(state dict, attn_emb, lens, fc_emb, tags or None) from the recipe (CPU tensors)."""
    sd = P.to_torch(P.bah_decoder_state(temporal=temporal, seed=int(seed), end_scale=END_SCALE, **shape))
    rng = np.random.default_rng(int(seed))
    mem = rng.normal(0.0, 0.25, (B, Tm, shape["attn_emb_dim"])).astype(np.float32)
    fc = rng.normal(0.0, 0.25, (B, shape["fc_emb_dim"])).astype(np.float32)
    drawn = rng.integers(1, Tm + 1, B)
    if lens is None:
        lens = drawn
    lens = np.array([drawn[i] if v is None else v for i, v in enumerate(lens)], dtype=np.int64)
    tags = torch.arange(B) % 4 if temporal else None
    return sd, torch.from_numpy(mem), torch.from_numpy(lens), torch.from_numpy(fc), tags


def case_inputs(name, temporal=True, seed=None):
    c = CASES[name]
    return inputs(c["shape"], c["B"], c["Tm"], c["lens"], c["seed"] if seed is None else seed, temporal)


def build_model(shape, temporal, sd):
    """The product model over the case's decoder, on the GPU (encoder: identity)."""
    import audiocaption_amd as A
    dcls, mcls = ((A.TemporalBahAttnDecoder, A.TemporalSeq2SeqAttnModel) if temporal else
                  (A.BahAttnCatFcDecoder, A.Seq2SeqAttnModel))
    dec = dcls(dropout=0.5, **shape)
    dec.load_state_dict(sd, strict=True)
    return mcls(torch.nn.Identity(), dec).cuda().eval()


def g20_inputs():
    """The fixture's inputs.  Clip 4 (length 306 > Tm) repeats clip 0's memory (length 301 = Tm)."""
    sd, mem, lens, fc, tags = inputs(G20_SHAPE, G20["B"], G20["Tm"], G20["lens"], G20["seed"], True)
    mem[4] = mem[0]
    return sd, mem, lens, fc, tags


def g20_step_inputs(sd, t):
    """(h, words) of the fixture's step t: t = 0 takes the tags and a zero state, t = 3 word ids and a state in (-1, 1)
    drawn from torch.Generator().manual_seed(G20 seed + t); row 4 repeats row 0's state (its attention weights then
    depend on nothing row 0's do not)."""
    B, d, V = G20["B"], G20_SHAPE["d_model"], G20_SHAPE["vocab_size"]
    g = torch.Generator().manual_seed(G20["seed"] + t)
    h = torch.zeros(B, d) if t == 0 else torch.rand(B, d, generator=g) * 2 - 1
    h[4] = h[0]
    words = torch.randint(3, V, (B,), generator=g)
    return h, words


# ---- the dispatch of ac_gemm, mirrored (audiocaption_amd/csrc/train.hip:1420-1437) ---------------------------------------
def gemm_route(M, N, K, aligned=True, k_contiguous=True, pitches_mod4=True, splitk=1, a_scale=False):
    """The kernel ac_gemm launches for C[M][N] = A[M][K] B[N][K]^T.  ``aligned``: A and B bases on 16 bytes;
    ``pitches_mod4``: both row pitches multiples of 4 floats (train.hip:1423-1424); GT = 64 (train.hip:36)."""
    cdiv = lambda a, b: (a + b - 1) // b   # noqa: E731
    tiles64 = cdiv(M, 64) * cdiv(N, 64)
    small = splitk == 1 and tiles64 <= 256 and K >= 128                                   # train.hip:1422
    kk_ok = k_contiguous and K % 4 == 0 and pitches_mod4 and aligned                      # train.hip:1423-1424
    if small and not a_scale and k_contiguous and K % 32 == 0 and pitches_mod4 and aligned:   # train.hip:1427-1429
        return "kk"
    if kk_ok and N >= 96 and cdiv(M, 128) * cdiv(N, 128) * splitk >= 512:                # train.hip:1425,1430-1432
        return "nt<2>"
    if kk_ok and N >= 48 and tiles64 * splitk >= 128:                                     # train.hip:1426,1433-1435
        return "nt<1>"
    return "general"                                                                      # train.hip:1436-1437


def decoder_gemms(shape, B, Tm, R_):
    """(name, M, N, K) of every GEMM the decoder launches (csrc/attn_gru.hip: ac_bah_memory, bah_step) for B clips, R rows.
    Every base is 16-byte aligned and every pitch a multiple of 4 (dims are multiples of 32; the workspace is carved in
    units of 4 floats), so the route depends on (M, N, K) alone."""
    E, d, S, A, F, V = (shape[k] for k in KEYS)
    return [("ek", B * Tm, S, A), ("fc_proj", B, E, F), ("gf", B, 3 * d, E),
            ("hg_attn", R_, S, d), ("hg_hh", R_, 3 * d, d), ("ctx_proj", R_, E, A), ("gi", R_, 3 * d, 2 * E),
            ("classifier", R_, V, d)]


def case_routes(name, beam=1):
    c = CASES[name]
    return {nm: (M, N, K, gemm_route(M, N, K)) for nm, M, N, K in decoder_gemms(c["shape"], c["B"], c["Tm"], c["B"] * beam)}


def route_table():
    """Lines 'case (rows): gemm MxNxK -> route' for every case at the row counts its tests decode."""
    lines = []
    for name, c in CASES.items():
        for beam in sorted({1} | {k for k, _ in c["beam_seed"]}):
            r = case_routes(name, beam)
            lines.append(f"{name} beam {beam} ({c['B'] * beam} rows): " +
                         ", ".join(f"{nm} {M}x{N}x{K} {rt}" for nm, (M, N, K, rt) in r.items()))
    return lines


def assert_route_coverage():
    reached = {}
    for name, c in CASES.items():
        for beam in sorted({1} | {k for k, _ in c["beam_seed"]}):
            for nm, (M, N, K, rt) in case_routes(name, beam).items():
                reached.setdefault(rt, []).append((name, beam, nm))
    assert set(reached) == {"kk", "nt<2>", "nt<1>", "general"}, sorted(reached)
    ek = lambda name: case_routes(name)["ek"][3]   # noqa: E731
    assert ek("routes-1") == "nt<1>" and ek("routes-2") == "nt<2>"
    assert case_routes("routes-1")["classifier"][3] == "nt<1>" and case_routes("routes-1", 4)["classifier"][3] == "nt<1>"
    assert set(rt for _, _, _, rt in case_routes("narrow", 8).values()) == {"general"}
    assert CASES["routes-1"]["shape"]["vocab_size"] % 2 == 1       # logit + t * V is 4-byte aligned only at odd t
    return reached


# ---- CPU probes the tests share --------------------------------------------------------------------------------------------
def greedy_pair(sd, mem, lens, fc, tags, L):
    """f32 and float64 greedy runs of the restatement, the live mask and the error budget n."""
    with torch.no_grad():
        r32 = R.greedy(sd, mem, lens, fc, tags, L)
        r64 = R.greedy(sd, mem, lens, fc, tags, L, dtype=torch.float64)
    live = R.live_mask(r32["seq"].numpy())
    return r32, r64, live


def beam_pair(sd, mem, lens, fc, tags, k, L, temp=1.0):
    with torch.no_grad():
        trace = []
        r32 = R.beam_search(sd, mem, lens, fc, tags, k, L, temp=temp, trace=trace)
        r64 = R.beam_search(sd, mem, lens, fc, tags, k, L, temp=temp, dtype=torch.float64)
        nb = R.beam_search(sd, mem, lens, fc, tags, k, L, temp=temp, n_best=True, n_best_size=k)
        nb64 = R.beam_search(sd, mem, lens, fc, tags, k, L, temp=temp, n_best=True, n_best_size=k, dtype=torch.float64)
    margin = min(r["margin"] for r in trace)
    steps = [max(r["t"] for r in trace if r["clip"] == i) + 1 for i in range(mem.shape[0])]
    return r32, r64, nb, nb64, margin, steps


def _search_seeds():
    """Print, per case, the first seeds from 31 that satisfy the preconditions in the module docstring."""
    for name, c in CASES.items():
        lengths = (c["L"],) + {"long": MAX_LENGTHS, "narrow": (23, 7, 6)}.get(name, ())
        for seed in range(31, 60):
            ok, note = True, []
            for temporal in (True, False) if name in ("long", "narrow") else (True,):
                args = case_inputs(name, temporal, seed)
                for L in lengths:
                    r32, r64, live = greedy_pair(*args, L)
                    gap = float(r32["gap"][torch.from_numpy(live)].min())
                    note.append(f"L {L} {'t' if temporal else 'p'} ends {live.sum(1).tolist()[:8]} gap {gap:.2e}")
                    ok &= torch.equal(r32["seq"], r64["seq"]) and gap >= GATE and (L == 1 or int(live.sum(1).min()) > 1)
            print(f"{name} greedy seed {seed}: {'USED' if ok else 'rejected'}: " + "; ".join(note), flush=True)
            if ok:
                break
        for (k, temp) in c["beam_seed"]:
            lengths = (c.get("beam_L", c["L"]),) + (MAX_LENGTHS if (name, k, temp) == ("long", 3, 1.0) else ())
            for seed in range(31, 60):
                ok, note = True, []
                for temporal in (True,):
                    args = case_inputs(name, temporal, seed)
                    for L in lengths:
                        r32, r64, nb, nb64, margin, steps = beam_pair(*args, k, L, temp)
                        note.append(f"L {L} margin {margin:.2e} steps {steps[:8]}")
                        ok &= torch.equal(r32["seq"], r64["seq"]) and torch.equal(nb["seq"], nb64["seq"]) and margin >= GATE
                print(f"{name} beam {k} temp {temp} seed {seed}: {'USED' if ok else 'rejected'}: " + "; ".join(note), flush=True)
                if ok:
                    break


if __name__ == "__main__":
    print("\n".join(route_table()))
    _search_seeds()
