"""No GPU: what tests/test_gpu_decoder_shapes.py relies on.

* the oracle (oracle/cpu_path.py decoder_forward with ``nlayers`` / ``nhead``) against ``torch.nn.TransformerDecoder`` in
  float64 at general shapes;
* the guards of the search cases of tests/_decoder_shapes.py: evaluated on the float64 oracle, asserted, not skipped;
* the oracle's own float32 evaluation against float64 on the teacher-forced inputs (the room the 1e-4 bar leaves);
* the shapes the HIP decoder refuses, from ``TransformerDecoder.weights()`` and from the C entry points, without a device."""
import ctypes
import math

import pytest
import torch

import _decoder_shapes as S
from oracle import cpu_path as O


# ----------------------------------------------------------------------------------------------------------------------
# the oracle at general shapes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", ["S2", "S3", "S6", "S1"])
def test_oracle_matches_torch_nn_in_float64(sid):
    """(128,4,3,512), (192,12,2,512), (256,8,2,1024) and (64,1,1,256): the same procedural state in the product class's
    nn modules (attn_proj, word_embedding, pos_encoder.pe, model, classifier) on the CPU, float64, masks as the reference
    passes them (transformer_decoder.py:86-101).  Measured < 1e-14; asserted < 1e-12."""
    d, h, nl, ff, A_, V = S.SHAPES[sid]
    T, Tm = 40, 9
    inp = S.tf_inputs(sid, T, Tm)
    state = S.f64(S.plain_state(sid))
    ref = O.decoder_forward(state, inp["word"], inp["attn_emb"].double(), inp["attn_emb_len"], inp["cap_padding_mask"],
                            **S.oracle_kw(sid))
    dec = S.product_decoder(sid, S.plain_state(sid)).double().eval()
    with torch.no_grad():
        mem = dec.attn_proj(inp["attn_emb"].double()).transpose(0, 1)
        x = dec.word_embedding(inp["word"]) * math.sqrt(d)
        x = x.transpose(0, 1) + dec.pos_encoder.pe[:T]
        causal = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
        mem_pad = ~(torch.arange(Tm)[None, :] < inp["attn_emb_len"][:, None])
        out = dec.model(x, mem, tgt_mask=causal, tgt_key_padding_mask=inp["cap_padding_mask"],
                        memory_key_padding_mask=mem_pad).transpose(0, 1)
        logit = dec.classifier(out)
    de, dl = float((out - ref["embed"]).abs().max()), float((logit - ref["logit"]).abs().max())
    print(f"{sid}: oracle vs torch.nn float64 max|embed| {de:.3e} max|logit| {dl:.3e}")
    assert torch.isfinite(ref["logit"]).all()
    assert de < 1e-12 and dl < 1e-12


def test_oracle_defaults_are_the_reference_shape():
    """``nlayers`` / ``nhead`` threaded through the searches leave the default calls as they were: 2 layers, 4 heads."""
    emb, lens = S.memory("S0", 2, 6), torch.tensor([6, 3])
    dec_state = S.plain_state("S0")
    a = O.greedy_decode(dec_state, emb, lens, 4)
    b = O.greedy_decode(dec_state, emb, lens, 4, nlayers=2, nhead=4)
    assert a["logit"].dtype == torch.float32 and torch.equal(a["logit"], b["logit"]) and torch.equal(a["seq"], b["seq"])
    a = O.beam_search(dec_state, emb, lens, 2, 4)
    b = O.beam_search(dec_state, emb, lens, 2, 4, nlayers=2, nhead=4)
    assert torch.equal(a["seq"], b["seq"]) and torch.equal(a["score"], b["score"])


def test_shape_table_reaches_what_it_claims():
    """The branches of csrc/decoder.hip the table is there for (dec_gemm_kernel: KC = min(K, 512), nsteps = KC / 64,
    nf = K / 64; attn_step_kernel: hd == 64 or not; decoder_step: fused for d 256 / 4 heads only)."""
    hd = {k: v[0] // v[1] for k, v in S.SHAPES.items()}
    assert hd["S2"] == 32 and hd["S3"] == 16 and hd["S1"] == 64 and hd["S4"] == 64 and hd["S6"] == 32
    assert {v[0] // 64 for v in S.SHAPES.values()} == {1, 2, 3, 4, 6, 8}            # nf, nsteps of the K = d projections
    assert S.SHAPES["S4"][3] == 4 * 512 and S.SHAPES["S5"][3] == 3 * 512 and S.SHAPES["S1"][3] < 512
    assert S.SHAPES["S2"][2] % 2 == 1 and S.SHAPES["S5"][2] == 8 and S.SHAPES["S1"][2] == 1
    assert S.SHAPES["S2"][4] % 64 and S.SHAPES["S1"][4] == 32 and S.SHAPES["S6"][5] % 16
    assert [k for k, v in S.SHAPES.items() if v[0] == 256 and v[1] == 4] == sorted(S.FUSED)
    assert max(S.TF_TM.values()) > 32 and 33 in S.TF_TM.values()


# ----------------------------------------------------------------------------------------------------------------------
# the room under the bar
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", sorted(S.SHAPES))
def test_float32_oracle_is_well_inside_the_logit_bar(sid):
    """The oracle itself in float32 against float64 on the teacher-forced inputs of 3a (T = 100): 2-5e-6 on the logits,
    which peak at 4-9.  The 1e-4 bar of test_g3_decoder_forward_vs_reference_golden therefore leaves a float32 kernel
    that sums in another order more than an order of magnitude."""
    inp, ref = S.tf_reference(sid, 100, S.TF_TM[sid])
    got = O.decoder_forward(S.plain_state(sid), inp["word"], inp["attn_emb"], inp["attn_emb_len"], inp["cap_padding_mask"],
                            **S.oracle_kw(sid))
    dl = float((got["logit"].double() - ref["logit"]).abs().max())
    de = float((got["embed"].double() - ref["embed"]).abs().max())
    print(f"{sid}: float32 oracle vs float64 max|logit| {dl:.3e} max|embed| {de:.3e}; |logit| peaks at "
          f"{float(ref['logit'].abs().max()):.2f}")
    assert torch.isfinite(ref["logit"]).all() and torch.isfinite(ref["embed"]).all()
    assert dl < S.LOGIT_BAR / 4 and de < S.LOGIT_BAR / 4


# ----------------------------------------------------------------------------------------------------------------------
# guards of the search cases
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(S.GREEDY_CASES))
def test_long_greedy_cases_are_meaningful(case):
    """Float64 oracle, 48 steps, <end> at beta -3: every row unfinished for at least 33 steps, the four rows differ, a row
    with >= 8 distinct tokens (a wrong key index shows), smallest top-1 margin over live rows >= 1e-3 (10 x the bar)."""
    sid, seed, _ = S.GREEDY_CASES[case]
    _, _, out = S.greedy_reference(sid, seed)
    f = S.greedy_facts(out)
    print(f"{case}: seed {seed}, steps {out['steps']}, tokens before <end> {f['run_len']}, distinct {f['distinct']}, "
          f"margin {f['margin']:.3g}")
    assert min(f["run_len"]) >= 33
    assert len({tuple(r) for r in out["seq"].tolist()}) == out["seq"].shape[0]
    assert max(f["distinct"]) >= 8
    assert f["margin"] >= S.MARGIN


@pytest.mark.parametrize("case", sorted(S.STOP_CASES))
def test_early_stop_cases_are_meaningful(case):
    """Rows that emit <end> within 5 steps beside rows that run past 32 positions; no near tie while a row is live."""
    sid, seed, beta = S.STOP_CASES[case]
    _, _, out = S.greedy_reference(sid, seed, beta)
    f = S.greedy_facts(out)
    print(f"{case}: seed {seed}, beta {beta}, steps {out['steps']}, tokens before <end> {f['run_len']}, margin {f['margin']:.3g}")
    assert min(f["run_len"]) < 5 and max(f["run_len"]) >= 33
    assert f["margin"] >= S.MARGIN
    assert int(f["cnt"][0]) < out["seq"].shape[0] or int(f["cnt"][4]) < out["seq"].shape[0]   # the count moves early


@pytest.mark.parametrize("case", sorted(S.BEAM_CASES))
def test_long_beam_cases_have_no_near_ties(case):
    """As tests/test_gpu_decode_select.py: the trace's ``margin`` and ``cut`` are >= 1e-3 at every step; the search runs all
    40 steps, re-gathers the KV cache past position 32, and the finished scores that decide a caption are >= 2e-4 apart."""
    sid, seed = S.BEAM_CASES[case]
    _, _, out, trace = S.beam_reference(sid, seed)
    worst, cut = min(r["margin"] for r in trace), min(r["cut"] for r in trace)
    print(f"{case}: seed {seed}, steps {max(r['t'] for r in trace) + 1}, smallest margin {worst:.4g}, cut {cut:.4g}")
    assert worst >= S.MARGIN and cut >= S.MARGIN
    ident = list(range(S.BEAM))
    for clip in range(len(S.BEAM_LENS)):
        assert max(r["t"] for r in trace if r["clip"] == clip) == S.BEAM_LEN - 1
        assert any(r["t"] >= 32 and r["prev_beam"] != ident for r in trace if r["clip"] == clip)
        sc = sorted((x for r in trace if r["clip"] == clip for x in r["end_scores"]), reverse=True)
        assert sc[0] - sc[1] >= 2e-4, (clip, sc)
    assert max(len(set(r)) for r in out["seq"].tolist()) >= 8


# ----------------------------------------------------------------------------------------------------------------------
# refusals that need no device
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.REFUSED))
def test_unsupported_shapes_are_refused_by_weights(name):
    """``weights()`` raises before a device pointer is taken (the decoder is on the CPU here: anything later would
    complain about that instead), names the limit and states the supported set."""
    from audiocaption_amd import _lib
    dec = S.refused_decoder(name)
    with pytest.raises(_lib.HipLibraryError, match=S.REFUSED[name][1]) as e:
        dec.weights()
    assert "Supported:" in str(e.value) and "multiple of 64" in str(e.value)
    assert dec._w is None and dec._ws == {}


def _c_struct(d, h, nl, ff, A_, V=50):
    from audiocaption_amd import _lib
    w = _lib.AcTrmWeights()
    w.d_model, w.nhead, w.nlayers, w.dim_ff, w.vocab, w.max_pos, w.attn_emb_dim = d, h, nl, ff, V, 100, A_
    return w


def test_c_entry_points_refuse_the_same_set():
    """csrc/decoder.hip check_weights is the step's real limits: the size queries and ac_trm_memory (asked with null
    buffers: nothing can be launched) refuse every shape ``check_supported`` refuses and accept every shape it accepts."""
    import audiocaption_amd as A
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    probe = A.TransformerDecoder(emb_dim=64, vocab_size=8, fc_emb_dim=32, attn_emb_dim=32, dropout=0.0, nhead=1, nlayers=1,
                                 dim_feedforward=64)
    seen = {True: 0, False: 0}
    for d in list(range(32, 640, 32)) + [768, 1024]:
        for h in (1, 2, 3, 4, 5, 6, 8, 12, 16):
            for ff in (32, 64, 192, 448, 512, 576, 768, 1024, 1280, 1536, 2048, 4 * d):
                for nl, A_ in ((1, 32), (8, 96), (9, 64), (2, 48), (0, 64)):
                    probe.d_model, probe.nhead, probe.dim_feedforward, probe.nlayers, probe.attn_emb_dim = d, h, ff, nl, A_
                    try:
                        probe.check_supported()
                        ok = True
                    except _lib.HipLibraryError:
                        ok = False
                    w = _c_struct(d, h, nl, ff, A_)
                    got = (lib.ac_trm_step_pack_floats(ctypes.byref(w)) > 0, lib.ac_trm_workspace_floats(ctypes.byref(w), 4, 20) > 0)
                    assert got == (ok, ok), (d, h, ff, nl, A_, ok, got)
                    if not ok:
                        assert lib.ac_trm_memory(ctypes.byref(w), None, 1, 4, None, None, None) == _lib.AC_ERR_ARG
                    seen[ok] += 1
    assert seen[True] > 100 and seen[False] > 100
    for sid, (d, h, nl, ff, A_, V) in S.SHAPES.items():
        assert lib.ac_trm_step_pack_floats(ctypes.byref(_c_struct(d, h, nl, ff, A_, V))) > 0, sid
    for name, (over, _) in S.REFUSED.items():
        dec = S.refused_decoder(name)
        w = _c_struct(dec.d_model, dec.nhead, dec.nlayers, dec.dim_feedforward, dec.attn_emb_dim)
        assert lib.ac_trm_step_pack_floats(ctypes.byref(w)) == -1, name
        assert lib.ac_trm_workspace_floats(ctypes.byref(w), 4, 20) == -1, name
