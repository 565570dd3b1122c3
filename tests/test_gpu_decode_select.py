"""Token selection of the decode searches across every branch of ``ac_trm_beam_step`` and ``ac_trm_greedy``
(csrc/decoder.hip), against plain references:

* beam search, one step at a time, against a float64 shadow of the step (oracle decoder, then
  log_softmax(log_softmax(x) / temp) + cum and the top `beam` in float64), and the bookkeeping of every step against a
  numpy restatement of base.py:317-335 (oracle/cpu_path.py beam_search);
* the final ids (plain and n-best) against ``oracle.cpu_path.beam_search``;
* ``ac_trm_beam_update`` on hand-made candidates against the same numpy restatement (exact equality);
* greedy at the vocabulary edges of ``greedy_pick_kernel`` in both forms (launch chain, one-launch cluster);
* the captured beam segments when AUDIOCAPTION_BEAM_SEGMENTS changes between calls.

Which selection kernels a configuration reaches (ac_trm_beam_step): beam <= 8 and V <= 5120 ``beam_row_topk_kernel<20>``,
beam <= 8 and 5120 < V <= 8192 ``beam_row_topk_kernel<32>`` (both + ``beam_merge_kernel``); otherwise
``beam_logprob_kernel`` + ``beam_topk_kernel``, with its register lists for beam <= 4 and a full rescan per winner above.

The models are decoder-only procedural draws (procedural.decoder_state_diverse) over the encoder memory of
tests/golden/g4_greedy.npz.  A clip is (k, length): golden clip k % 4 with its frames rolled by k // 4, memory length
`length`.  The clips of every configuration were chosen so that the searches have no near ties (the CPU guards below):
only there are ids a meaningful comparison."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import cpu_path as O

END, PAD, START = O.END_IDX, O.PAD_IDX, O.START_IDX
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (id, V, beam, temp, max_length, clips)
BEAM_CASES = [
    ("row20-V100-b8-t0.5", 100, 8, 0.5, 20, [(2, 1), (3, 1), (6, 15)]),
    ("row20-V5120-b5-t1.7", 5120, 5, 1.7, 20, [(6, 15), (5, 5), (5, 1)]),
    ("row20-V100-b2-L1", 100, 2, 1.0, 1, [(0, 31), (1, 27), (2, 15), (3, 29)]),
    ("row20-V5120-b1-L2", 5120, 1, 1.0, 2, [(2, 15), (3, 29), (0, 1)]),
    ("row32-V5121-b8", 5121, 8, 1.0, 20, [(7, 5), (2, 1), (7, 29)]),
    ("row32-V8192-b2-t0.5", 8192, 2, 0.5, 20, [(0, 31), (1, 27), (3, 1), (2, 15)]),
    ("row32-V5121-b1-t1.7", 5121, 1, 1.7, 20, [(2, 15), (3, 29)]),
    ("reg-V8193-b2-t1.7", 8193, 2, 1.7, 20, [(0, 5), (3, 5), (2, 15), (0, 1)]),
    ("reg-V12000-b4", 12000, 4, 1.0, 20, [(1, 27), (3, 29), (2, 1)]),
    ("reg-V8193-b1-t0.5-L1", 8193, 1, 0.5, 1, [(0, 31), (1, 27), (2, 15), (3, 29)]),
    ("scan-V8193-b5-t0.5", 8193, 5, 0.5, 20, [(0, 31), (6, 15), (5, 5), (2, 1)]),
    ("scan-V12000-b8-t1.7-L2", 12000, 8, 1.7, 2, [(1, 27), (2, 15), (3, 29), (1, 1)]),
    ("scan-V100-b9-t1.7", 100, 9, 1.7, 20, [(4, 1), (0, 5), (6, 15)]),
    ("scan-V5120-b16", 5120, 16, 1.0, 20, [(3, 5), (5, 5)]),
    ("scan-V100-b64-t0.5", 100, 64, 0.5, 20, [(5, 1)]),
    # 8 clips x 64 beams = 512 rows: the classifier takes the tiled ac_gemm (classifier_step) at a vocabulary of 5121
    ("scan-V5121-b64-gemm512-L2", 5121, 64, 1.0, 2, [(4, 1), (5, 1)] * 4),
]
BEAM_IDS = [c[0] for c in BEAM_CASES]

# V -> clips; greedy_pick_kernel holds up to PICK_MAXV = 16384 logits of a row in registers
GREEDY_CASES = {100: [(0, 31), (3, 29), (1, 1)], 5121: [(0, 31), (3, 29), (4, 5), (2, 15)],
                8193: [(2, 15), (3, 29), (4, 1), (0, 31)], 16384: [(0, 31), (4, 1), (3, 29), (7, 29)]}

MARGIN = 1e-3        # a gap in the scores below which the kept ids are not a meaningful comparison
SCORE_GAP = 2e-4     # finished-beam scores closer than this could sort either way in float32


def _tol(ref):
    """|kernel - float64| allowed for a score: the cumulative scores carry -1000 offsets, hence the relative term."""
    return 1e-4 + 1e-6 * np.abs(ref)


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(os.path.join(GOLDEN, "g4_greedy.npz"))
    return torch.from_numpy(g["attn_emb"]), g["attn_emb_len"]


def _clips(spec):
    emb, _ = _golden()
    e = torch.cat([torch.roll(emb[k % 4:k % 4 + 1], k // 4, dims=1) for k, _ in spec])
    return e.contiguous(), torch.tensor([ln for _, ln in spec], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _state(kind, V, tie=None):
    """Procedural decoder weights; tie = (src, dst): classifier row src copied into row dst (exact ties)."""
    from audiocaption_amd import procedural as P
    st = P.to_torch(P.decoder_state_diverse(kind, vocab_size=V))
    if tie is not None:
        w = st["decoder.classifier.weight"].clone()
        w[tie[1]] = w[tie[0]]
        st["decoder.classifier.weight"] = w
    return st


def _model(state):
    """Decoder-only product model on cuda:0 (the searches start from the encoder outputs)."""
    import audiocaption_amd as A
    from audiocaption_amd import build
    build.build()
    V = state["decoder.classifier.weight"].shape[0]
    dec = A.TransformerDecoder(emb_dim=256, vocab_size=V, fc_emb_dim=512, attn_emb_dim=512, dropout=0.2, nlayers=2)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in state.items()}, strict=True)
    return A.TransformerModel(torch.nn.Identity(), dec).eval().to("cuda:0")


@functools.lru_cache(maxsize=None)
def _oracle_beam(case_id, n_best=False):
    _, V, beam, temp, L, spec = next(c for c in BEAM_CASES if c[0] == case_id)
    emb, lens = _clips(spec)
    trace = []
    out = O.beam_search(_state("beam", V), emb, lens, beam, L, temp, n_best=n_best, trace=trace)
    return out, trace


def _enc(spec):
    emb, lens = _clips(spec)
    return {"attn_emb": emb.cuda(), "attn_emb_len": lens}


# ----------------------------------------------------------------------------------------------------------------------
# numpy restatement of the per-clip bookkeeping of base.py:290-335 (oracle/cpu_path.py beam_search) in the device layout
# of ac_trm_beam_update: token rows [B*beam][max_len+1], finished beams [B][cap][max_len]
# ----------------------------------------------------------------------------------------------------------------------
def _ref_update(s, top_val, top_idx, beam, V, L, t, end, pad, cap):
    """s: dict of numpy arrays tok, cum, active, done_cnt, done_seq, done_score, n_active (updated in place, tok replaced).
    Returns src_row."""
    B = len(s["active"])
    tok_in = s["tok"]
    tok = tok_in.copy()
    src_row = np.zeros(B * beam, np.int32)
    for c in range(B):
        act = s["active"][c] != 0
        for k in range(beam):
            flat = int(top_idx[c, k])
            src = c * beam + flat // V if act else c * beam + k   # prev_beam = topk_words // V (base.py:292)
            src_row[c * beam + k] = src
            tok[c * beam + k] = tok_in[src]
            if act:
                tok[c * beam + k, t + 1] = flat % V                # seq = cat(seq[prev_beam], next_word)
        if not act:                                                # a finished clip is left alone (the reference broke)
            continue
        cnt = int(s["done_cnt"][c])
        for k in range(beam):
            v = np.float32(top_val[c, k])
            is_end = int(top_idx[c, k]) % V == end or t == L - 1
            if is_end:
                if cnt < cap:
                    s["done_seq"][c, cnt] = [tok[c * beam + k, j + 1] if j <= t else end for j in range(L)]
                    s["done_score"][c, cnt] = v / np.float32(t + 1)
                cnt += 1
            s["cum"][c * beam + k] = v - np.float32(1000.0) if is_end else v   # topk_logprob[is_end] -= 1000
        s["done_cnt"][c] = cnt
        if cnt == beam:                                            # len(done) == beam_size
            s["active"][c] = 0
            s["n_active"][0] -= 1
    s["tok"] = tok
    s["mask"] = (tok == pad).astype(np.uint8)
    return src_row


# ----------------------------------------------------------------------------------------------------------------------
# CPU guards: the chosen clips have no near ties, so the id comparisons on the GPU cannot flake
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BEAM_CASES, ids=BEAM_IDS)
def test_beam_cases_have_no_near_ties(case):
    """Every step the oracle runs: the gaps among the kept candidates and to the first cut are >= 1e-3.  From beam 16 on
    (17+ ranks per step) only the cut is held to it: an order swap among kept candidates changes neither the kept set nor
    the result, and the step check compares those ranks only where their gaps allow.  The finished scores of a clip that
    decide the caption and its n-best order are >= 2e-4 apart."""
    case_id, V, beam = case[:3]
    _, trace = _oracle_beam(case_id)
    key = "margin" if beam < 16 else "cut"
    worst = min(r[key] for r in trace)
    print(f"{case_id}: steps {max(r['t'] for r in trace) + 1}, smallest {key} {worst:.4g}")
    assert worst >= MARGIN, (case_id, key, worst)
    for clip in sorted({r["clip"] for r in trace}):
        sc = sorted((s for r in trace if r["clip"] == clip for s in r["end_scores"]), reverse=True)[:beam + 1]
        gaps = [a - b for a, b in zip(sc[:-1], sc[1:])]
        assert not gaps or min(gaps) >= SCORE_GAP, (case_id, clip, gaps)


@pytest.mark.parametrize("V", sorted(GREEDY_CASES))
def test_greedy_cases_have_no_near_ties(V):
    """Every step the oracle's greedy search runs: the two largest logits of each still-unfinished clip are >= 1e-3 apart."""
    emb, lens = _clips(GREEDY_CASES[V])
    out = O.greedy_decode(_state("greedy", V), emb, lens, 20)
    steps = out["steps"]
    top2 = out["logit"][:, :steps].topk(2, -1).values
    gap = top2[..., 0] - top2[..., 1]
    seq = out["seq"][:, :steps]
    running = torch.ones_like(seq, dtype=torch.bool)
    running[:, 1:] = torch.cumprod((seq[:, :-1] != END).long(), 1).bool()   # clips that had not ended before step t
    worst = float(gap[running].min())
    print(f"V {V}: steps {steps}, smallest top-2 gap {worst:.4g}")
    assert worst >= MARGIN


def test_beam_cases_cover_every_selection_branch():
    """The configurations reach every branch of ac_trm_beam_step's selection and the boundaries on both sides."""
    def branch(V, beam):
        if beam <= 8 and V <= 8192:
            return "row20" if V <= 5120 else "row32"
        return "reg" if beam <= 4 else "scan"
    seen = {branch(V, beam) for _, V, beam, *_ in BEAM_CASES}
    assert seen == {"row20", "row32", "reg", "scan"}
    for cid, V, beam, *_ in BEAM_CASES:
        assert cid.startswith(branch(V, beam)), cid
    assert {V for _, V, *_ in BEAM_CASES} >= {100, 5120, 5121, 8192, 8193, 12000}
    assert {b for _, _, b, *_ in BEAM_CASES} >= {1, 2, 5, 8, 9, 16, 64}
    assert {c[3] for c in BEAM_CASES} >= {1.0, 0.5, 1.7}
    assert {c[4] for c in BEAM_CASES} >= {1, 2, 20}
    assert any(len(c[5]) * c[2] >= 512 for c in BEAM_CASES)
    assert any(ln == 1 for c in BEAM_CASES for _, ln in c[5])
    assert 8192 < max(GREEDY_CASES) <= 16384 and min(GREEDY_CASES) <= 5120


def test_ref_update_restates_the_oracle_bookkeeping():
    """The numpy restatement drives a beam search to the oracle's result: a step is a float64 top-k of the oracle's scores
    (no near ties in this case) + _ref_update, the captions come from its finished beams as _beam_finish reads them."""
    case_id, V, beam, temp, L, spec = BEAM_CASES[0]
    st = _state("beam", V)
    emb, lens = _clips(spec)
    B, R, cap = len(spec), len(spec) * beam, beam * L
    s = _fresh_shadow(B, beam, L, cap)
    for t in range(L):
        if s["n_active"][0] == 0:
            break
        lp = _shadow_scores(st, emb, lens, s, beam, t, temp)
        nrows = 1 if t == 0 else beam
        vals = np.zeros((B, beam), np.float32)
        idx = np.zeros((B, beam), np.int32)
        for c in range(B):
            v, i = lp[c * beam:c * beam + nrows].reshape(-1).topk(beam)
            vals[c], idx[c] = v.numpy(), i.numpy()
        _ref_update(s, vals, idx, beam, V, L, t, END, PAD, cap)
    want = _oracle_beam(case_id)[0]["seq"].numpy()
    for c in range(B):
        n = int(s["done_cnt"][c])
        best = max(range(n), key=lambda j: (s["done_score"][c, j], -j))
        np.testing.assert_array_equal(s["done_seq"][c, best], want[c])


# ----------------------------------------------------------------------------------------------------------------------
# the float64 shadow of one step
# ----------------------------------------------------------------------------------------------------------------------
def _fresh_shadow(B, beam, L, cap):
    R = B * beam
    tok = np.full((R, L + 1), END, np.int32)
    tok[:, 0] = START
    return {"tok": tok, "cum": np.zeros(R, np.float32), "active": np.ones(B, np.int32), "done_cnt": np.zeros(B, np.int32),
            "done_seq": np.zeros((B, cap, L), np.int32), "done_score": np.zeros((B, cap), np.float32),
            "n_active": np.array([B], np.int32), "mask": (tok == PAD).astype(np.uint8)}


def _shadow_scores(state, emb, lens, s, beam, t, temp):
    """float64 scores of step t for every row: the oracle decoder on the rows' prefixes (float32), then
    log_softmax(log_softmax(x) / temp) + cum in float64 (base.py:282-289).  Rows of finished clips are left at -inf."""
    R = s["tok"].shape[0]
    rows = [r for r in range(R) if s["active"][r // beam]]
    word = torch.from_numpy(s["tok"][rows, :t + 1].astype(np.int64))
    clip = torch.tensor([r // beam for r in rows])
    logit = O.decoder_forward(state, word, emb[clip], lens[clip], word == PAD)["logit"][:, -1].double()
    lp = torch.log_softmax(torch.log_softmax(logit, 1) / temp, 1) + torch.from_numpy(s["cum"][rows]).double()[:, None]
    out = torch.full((R, logit.shape[1]), float("-inf"), dtype=torch.float64)
    out[rows] = lp
    return out


def _check_step(lp, gv, gi, s_active, beam, t, where):
    """The kernel's top `beam` (values gv, flat ids gi: (B, beam)) against the float64 scores lp of the step."""
    compared = 0
    B = gv.shape[0]
    V = lp.shape[1]
    for c in range(B):
        if not s_active[c]:
            continue
        nrows = 1 if t == 0 else beam
        S = lp[c * beam:c * beam + nrows].reshape(-1).numpy()
        n = min(beam + 1, S.size)
        order = np.argsort(-S, kind="stable")[:n]
        ref = S[order]
        v = gv[c].astype(np.float64)
        i = gi[c].astype(np.int64)
        assert ((i >= 0) & (i < nrows * V)).all(), (where, c, i)
        assert len(set(i.tolist())) == beam, (where, c, "an id was chosen twice", i)
        assert (np.abs(v - ref[:beam]) <= _tol(ref[:beam])).all(), (where, c, "rank values", v - ref[:beam])
        assert (np.abs(v - S[i]) <= _tol(S[i])).all(), (where, c, "values of the chosen ids", v - S[i])
        for k in range(beam):
            lo = ref[k - 1] - ref[k] if k > 0 else np.inf
            hi = ref[k] - ref[k + 1] if k + 1 < n else np.inf
            if min(lo, hi) >= MARGIN:
                assert i[k] == order[k], (where, c, k, int(i[k]), int(order[k]))
                compared += 1
        if n > beam and ref[beam - 1] - ref[beam] >= MARGIN:
            assert set(i.tolist()) == set(order[:beam].tolist()), (where, c, "kept set")
    return compared


def _read(st, t):
    g = {k: st[k].cpu().numpy() for k in ("top_val", "top_idx", "cum", "active", "done_cnt", "done_seq", "done_score",
                                          "src_row", "n_active", "mask")}
    g["tok"] = st["tok"][(t + 1) & 1].cpu().numpy()
    return g


def _assert_bookkeeping(g, s, src_row, cap, where):
    for k in ("tok", "mask", "cum", "active", "done_cnt", "n_active"):
        np.testing.assert_array_equal(g[k], s[k], err_msg=f"{where}: {k}")
    np.testing.assert_array_equal(g["src_row"], src_row, err_msg=f"{where}: src_row")
    for c in range(len(s["active"])):
        n = min(int(s["done_cnt"][c]), cap)
        np.testing.assert_array_equal(g["done_seq"][c, :n], s["done_seq"][c, :n], err_msg=f"{where}: done_seq of clip {c}")
        np.testing.assert_array_equal(g["done_score"][c, :n], s["done_score"][c, :n], err_msg=f"{where}: done_score {c}")


def _run_steps(model, state, spec, beam, L, temp, monkeypatch, on_step=None):
    """A beam search launched one step per segment, eagerly; after every step the kernel's selection is checked against
    the float64 shadow and the device bookkeeping against _ref_update.  Returns the shadow and the steps run."""
    monkeypatch.setenv("AUDIOCAPTION_DECODE_GRAPH", "0")
    monkeypatch.setenv("AUDIOCAPTION_BEAM_SEGMENTS", ",".join(str(t) for t in range(L)))
    emb, lens = _clips(spec)
    V = state["decoder.classifier.weight"].shape[0]
    req = model._inference_dict({"mode": "inference", "sample_method": "beam", "beam_size": beam, "max_length": L,
                                 "temp": temp}, {"attn_emb": emb.cuda(), "attn_emb_len": lens})
    run = model._beam_begin(req)
    st, cap = run["st"], run["cap"]
    s = _fresh_shadow(len(spec), beam, L, cap)
    t = 0
    compared = 0
    while model._beam_advance(run):
        torch.cuda.synchronize()
        assert t < L
        g = _read(st, t)
        lp = _shadow_scores(state, emb, lens, s, beam, t, temp)
        where = f"step {t}"
        compared += _check_step(lp, g["top_val"], g["top_idx"], s["active"].copy(), beam, t, where)
        if on_step is not None:
            on_step(t, g, s)
        src_row = _ref_update(s, g["top_val"], g["top_idx"], beam, V, L, t, END, PAD, cap)
        _assert_bookkeeping(g, s, src_row, cap, where)
        t += 1
    model._beam_finish(run)
    return s, t, compared


# ----------------------------------------------------------------------------------------------------------------------
# part 1: beam selection
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", BEAM_CASES, ids=BEAM_IDS)
def test_beam_steps_match_float64_shadow(case, monkeypatch):
    """Each step's top `beam` values within 1e-4 + 1e-6 |x| of float64, the ids equal wherever float64 separates the
    ranks by >= 1e-3, the device bookkeeping equal to the numpy restatement; the finished beams equal the oracle's."""
    case_id, V, beam, temp, L, spec = case
    state = _state("beam", V)
    s, steps, compared = _run_steps(_model(state), state, spec, beam, L, temp, monkeypatch)
    _, trace = _oracle_beam(case_id)
    assert steps == max(r["t"] for r in trace) + 1            # the search stops where the reference's loop does
    assert compared > 0
    for c in range(len(spec)):
        want = sorted((x for r in trace if r["clip"] == c for x in r["end_scores"]), reverse=True)
        assert int(s["done_cnt"][c]) == len(want), c
        got = np.sort(s["done_score"][c, :len(want)].astype(np.float64))[::-1]
        assert (np.abs(got - want) <= _tol(np.array(want))).all(), (c, got, want)
    print(f"{case_id}: {steps} steps, {compared} ranks compared by id")


@pytest.mark.gpu
@pytest.mark.parametrize("case", BEAM_CASES, ids=BEAM_IDS)
def test_beam_search_ids_match_oracle(case):
    """Captions and n-best lists identical to oracle/cpu_path.py beam_search (default route: graphs and segments)."""
    case_id, V, beam, temp, L, spec = case
    model = _model(_state("beam", V))
    req = {"mode": "inference", "sample_method": "beam", "beam_size": beam, "max_length": L, "temp": temp}
    out = model.forward_decoder(dict(req), _enc(spec))
    np.testing.assert_array_equal(out["seq"].numpy(), _oracle_beam(case_id)[0]["seq"].numpy())
    outn = model.forward_decoder(dict(req, n_best=True), _enc(spec))
    np.testing.assert_array_equal(outn["seq"].numpy(), _oracle_beam(case_id, n_best=True)[0]["seq"].numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("V,beam", [(5120, 8), (8192, 3), (12000, 4), (100, 9), (8193, 16)],
                         ids=["row20", "row32", "reg", "scan-V100", "scan-V8193"])
def test_beam_exact_ties_take_the_lower_index(V, beam, monkeypatch):
    """A classifier row copied to a higher index gives bitwise-equal scores: the lower flattened index ranks first
    (cand_better / argmax_merge), on the row-kernel, register and rescan paths."""
    spec = [(0, 31), (1, 27)]
    emb, lens = _clips(spec)
    base = _state("beam", V)
    x0 = O.decoder_forward(base, torch.full((1, 1), START), emb[:1], lens[:1])["logit"][0, -1]
    x0[END] = -np.inf
    src = int(x0.argmax())                          # the strongest first word and its copy V / 2 away: both in the t = 0 top
    lo, hi = (src, src + V // 2) if src < V // 2 else (src - V // 2, src)
    assert END not in (lo, hi)
    state = _state("beam", V, tie=(src, hi if src == lo else lo))
    ties = []

    def on_step(t, g, s):
        for c in range(g["top_val"].shape[0]):
            v, i = g["top_val"][c], g["top_idx"][c]
            for k in range(beam - 1):
                if v[k] == v[k + 1]:
                    assert i[k] < i[k + 1], (t, c, k, i[k], i[k + 1])
                    ties.append((t, c, int(i[k]), int(i[k + 1])))

    _run_steps(_model(state), state, spec, beam, 3, 1.0, monkeypatch, on_step)
    print("ties", ties)
    assert (0, 0, lo, hi) in ties


# ----------------------------------------------------------------------------------------------------------------------
# part 2: ac_trm_beam_update on hand-made candidates
# ----------------------------------------------------------------------------------------------------------------------
def _update_case(B, beam, V, L, t, end=END, pad=PAD, cap=None, seed=0, ends=(), active=None, done_cnt=None):
    """Random parents and words (no end word unless listed in `ends` as (clip, slot)), descending scores per clip."""
    rng = np.random.default_rng(seed)
    cap = beam * L if cap is None else cap
    R = B * beam
    tok = rng.integers(3, V, size=(R, L + 1)).astype(np.int32)
    tok[:, 0] = START
    tok[:, t + 1:] = end
    nrows = 1 if t == 0 else beam
    idx = np.zeros((B, beam), np.int32)
    for c in range(B):
        prev = rng.integers(0, nrows, size=beam)
        words = rng.choice(np.arange(3, V), size=beam, replace=False)
        idx[c] = prev * V + words
    for c, k in ends:
        idx[c, k] = idx[c, k] - idx[c, k] % V + end
    val = -np.sort(rng.uniform(0.5, 30.0, size=(B, beam)).astype(np.float32), axis=1)
    s = {"tok": tok, "cum": rng.uniform(-30, 0, size=R).astype(np.float32),
         "active": np.ones(B, np.int32) if active is None else np.array(active, np.int32),
         "done_cnt": np.zeros(B, np.int32) if done_cnt is None else np.array(done_cnt, np.int32),
         "done_seq": np.full((B, cap, L), CANARY_SEQ, np.int32), "done_score": np.full((B, cap), CANARY_SCORE, np.float32),
         "n_active": None}
    s["n_active"] = np.array([int(s["active"].sum())], np.int32)
    s["mask"] = (tok == pad).astype(np.uint8)
    return s, val, idx, dict(beam=beam, V=V, L=L, t=t, end=end, pad=pad, cap=cap)


CANARY_SEQ, CANARY_SCORE, SPARE = -7, -12345.5, 4096


def _gpu_update(s, val, idx, p):
    """ac_trm_beam_update on copies of the shadow s.  The finished-beam buffers get SPARE canary elements past their end:
    a write beyond done_capacity entries of the last clip would land there."""
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in s.items()}
    spare = {}
    for k, fill in (("done_seq", CANARY_SEQ), ("done_score", CANARY_SCORE)):
        buf = torch.full((d[k].numel() + SPARE,), fill, dtype=d[k].dtype, device="cuda")
        buf[:d[k].numel()] = d[k].reshape(-1)
        spare[k] = buf
        d[k] = buf[:d[k].numel()].view(d[k].shape)
    tok_out = torch.full_like(d["tok"], -3)
    mask = torch.full_like(d["mask"], 9)
    src_row = torch.full((len(s["active"]) * p["beam"],), -3, dtype=torch.int32, device="cuda")
    tv, ti = torch.from_numpy(val).cuda(), torch.from_numpy(idx).cuda()
    P = _lib.ptr
    _lib.check(lib.ac_trm_beam_update(P(tv), P(ti), P(d["tok"]), P(tok_out), P(mask), P(d["cum"]), P(d["active"]),
                                      P(d["done_cnt"]), P(d["done_seq"]), P(d["done_score"]), P(src_row), P(d["n_active"]),
                                      len(s["active"]), p["beam"], p["V"], p["L"], p["t"], p["end"], p["pad"], p["cap"],
                                      _lib.stream()), "ac_trm_beam_update")
    torch.cuda.synchronize()
    for k, fill in (("done_seq", CANARY_SEQ), ("done_score", CANARY_SCORE)):
        assert (spare[k][-SPARE:] == fill).all(), f"{k} written past its end"
    g = {k: v.cpu().numpy() for k, v in d.items()}
    g["tok"], g["mask"], g["src_row"] = tok_out.cpu().numpy(), mask.cpu().numpy(), src_row.cpu().numpy()
    return g


def _check_update(s, val, idx, p):
    g = _gpu_update(s, val, idx, p)
    src_row = _ref_update(s, val, idx, p["beam"], p["V"], p["L"], p["t"], p["end"], p["pad"], p["cap"])
    _assert_bookkeeping(g, s, src_row, p["cap"], "update")
    # nothing past what the reference writes: the canaries stand everywhere else
    np.testing.assert_array_equal(g["done_seq"], s["done_seq"])
    np.testing.assert_array_equal(g["done_score"], s["done_score"])
    return g


UPDATE_CASES = {
    "end-in-slots": dict(B=3, beam=4, V=50, L=10, t=3, ends=[(0, 0), (1, 2), (2, 3), (2, 1)]),
    "first-step": dict(B=2, beam=3, V=40, L=6, t=0, ends=[(1, 1)]),
    "last-step-all-end": dict(B=3, beam=4, V=50, L=5, t=4, done_cnt=[0, 2, 3]),
    "cnt-jumps-past-beam": dict(B=2, beam=3, V=30, L=8, t=5, ends=[(0, 0), (0, 2), (1, 1)], done_cnt=[2, 1]),
    "cap-smaller-than-ends": dict(B=2, beam=4, V=30, L=6, t=2, cap=2, ends=[(0, 0), (0, 1), (0, 3), (1, 2)],
                                  done_cnt=[1, 2]),
    "inactive-clip": dict(B=3, beam=4, V=50, L=10, t=4, ends=[(0, 1), (1, 0), (1, 1)], active=[1, 0, 1], done_cnt=[0, 4, 1]),
    "pad-equals-end": dict(B=2, beam=3, V=30, L=8, t=3, pad=END, ends=[(0, 1), (1, 0)]),
    "clips-retire": dict(B=4, beam=3, V=40, L=8, t=2, ends=[(0, 0), (0, 1), (2, 2), (3, 0), (3, 1), (3, 2)],
                             done_cnt=[1, 0, 2, 0]),
    "beam64-B3": dict(B=3, beam=64, V=200, L=6, t=3, ends=[(0, 0), (0, 63), (1, 17), (2, 5), (2, 6)], done_cnt=[62, 0, 0]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(UPDATE_CASES))
def test_beam_update_matches_numpy_bookkeeping(name):
    s, val, idx, p = _update_case(**UPDATE_CASES[name])
    before = {k: v.copy() for k, v in s.items()}
    g = _check_update(s, val, idx, p)
    if name == "cnt-jumps-past-beam":            # 2 + 2 ends: done_cnt 4 > beam 3, and the clip goes on ('==')
        assert g["done_cnt"][0] == 4 and g["active"][0] == 1 and g["n_active"][0] == 2
    if name == "cap-smaller-than-ends":
        # clip 0 writes its slot 1 only (3 ends from count 1, capacity 2); clip 1 (count 2 = capacity) writes nothing
        assert g["done_cnt"].tolist() == [4, 3] and (g["done_seq"][0, 1] != CANARY_SEQ).all()
        assert (g["done_seq"][1] == CANARY_SEQ).all() and (g["done_score"][1] == CANARY_SCORE).all()
    if name == "inactive-clip":
        R = slice(4, 8)
        np.testing.assert_array_equal(g["tok"][R], before["tok"][R])
        np.testing.assert_array_equal(g["cum"][R], before["cum"][R])
        assert g["done_cnt"][1] == 4 and (g["done_seq"][1] == CANARY_SEQ).all() and (g["done_score"][1] == CANARY_SCORE).all()
    if name == "pad-equals-end":
        assert g["mask"][:, -1].all() and g["mask"][:, 0].sum() == 0
    if name == "clips-retire":                   # counts 2, 0, 3, 3 of beam 3: three clips retire, n_active 4 -> 1
        assert g["active"].tolist() == [0, 1, 0, 0] and g["n_active"][0] == 1
    if name == "last-step-all-end":
        assert (g["done_cnt"] == [4, 6, 7]).all() and g["active"].tolist() == [0, 1, 1] and g["n_active"][0] == 2
    if name == "beam64-B3":
        assert g["active"].tolist() == [0, 1, 1] and g["n_active"][0] == 2


@pytest.mark.gpu
def test_beam_abi_refuses_beams_wider_than_64():
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    x = torch.zeros(65 * 65, device="cuda")
    i = torch.zeros(65 * 65, dtype=torch.int32, device="cuda")
    P = _lib.ptr
    rc = lib.ac_trm_beam_update(P(x), P(i), P(i), P(i), P(i), P(x), P(i), P(i), P(i), P(x), P(i), P(i), 1, 65, 100, 4, 0,
                                END, PAD, 10, _lib.stream())
    assert rc != 0


# ----------------------------------------------------------------------------------------------------------------------
# part 3: greedy at the vocabulary edges
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["chain", "cluster"])
@pytest.mark.parametrize("V", sorted(GREEDY_CASES))
def test_greedy_ids_at_vocabulary_edges(V, mode, monkeypatch):
    """Ids identical to the oracle's greedy search and the oracle's top-8 logits within 1e-4, in both forms.  A vocabulary
    the cluster form does not cover: the form refuses it and the blocking call decodes with the launch chain."""
    state = _state("greedy", V)
    model = _model(state)
    spec = GREEDY_CASES[V]
    emb, lens = _clips(spec)
    want = O.greedy_decode(state, emb, lens, 20)
    req = {"mode": "inference", "sample_method": "greedy", "max_length": 20}
    dec = model.decoder
    if mode == "cluster" and not dec.cluster_covers(len(spec), emb.shape[1], 20):
        from audiocaption_amd import _lib
        monkeypatch.setenv("AUDIOCAPTION_GREEDY", "cluster")
        with pytest.raises(_lib.HipLibraryError):
            model.forward_decoder(dict(req), _enc(spec))
        monkeypatch.setenv("AUDIOCAPTION_GREEDY", "auto")
        out = model.forward_decoder(dict(req), _enc(spec))
        assert not any(k[7] for k in dec._greedy_state), "the blocking call did not fall back to the chain"
    else:
        monkeypatch.setenv("AUDIOCAPTION_GREEDY", mode)
        out = model.forward_decoder(dict(req), _enc(spec))
        assert any(k[7] == (mode == "cluster") for k in dec._greedy_state)
    np.testing.assert_array_equal(out["seq"].numpy(), want["seq"].numpy())
    steps = want["steps"]
    top = want["logit"][:, :steps].topk(8, -1)
    got = out["logit"][:, :steps].cpu().gather(-1, top.indices)
    d = float((got - top.values).abs().max())
    print(f"V {V} {mode}: {steps} steps, top-8 logits max|diff| {d:.3e}")
    assert d < 1e-4


# ----------------------------------------------------------------------------------------------------------------------
# part 4: the captured beam segments follow AUDIOCAPTION_BEAM_SEGMENTS
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_beam_graphs_follow_segment_changes(monkeypatch):
    """Captured and replayed under the default segments, then the same shape under "0" (one segment) and "0,5,17": every
    call returns the oracle's captions.  A graph cache keyed by the first step alone replays steps 0-7 for "0"."""
    monkeypatch.setenv("AUDIOCAPTION_DECODE_GRAPH", "1")
    monkeypatch.delenv("AUDIOCAPTION_BEAM_SEGMENTS", raising=False)
    V, beam, spec = 4981, 4, [(0, 31), (1, 27), (2, 15), (3, 29)]     # the g5b draw and clips
    state = _state("beam", V)
    emb, lens = _clips(spec)
    want = O.beam_search(state, emb, lens, beam, 20)["seq"].numpy()
    # a caption with a word at step 8 or later: a search cut off after steps 0-7 cannot return it
    assert (want[:, 8:] != END).any(), "every caption ends within steps 0-7: the test could not fail"
    model = _model(state)
    req = {"mode": "inference", "sample_method": "beam", "beam_size": beam, "max_length": 20}
    for _ in range(3):                                    # eager, capture, replay
        np.testing.assert_array_equal(model.forward_decoder(dict(req), _enc(spec))["seq"].numpy(), want)
    for seg in ("0", "0,5,17", "0,8,12,16"):
        monkeypatch.setenv("AUDIOCAPTION_BEAM_SEGMENTS", seg)
        for _ in range(2):
            np.testing.assert_array_equal(model.forward_decoder(dict(req), _enc(spec))["seq"].numpy(), want, err_msg=seg)
