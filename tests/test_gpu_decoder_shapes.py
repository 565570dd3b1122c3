"""The caption decoder (csrc/decoder.hip) away from the one shape and length the other suites decode: every shape of
tests/_decoder_shapes.py, rows of 100 positions, searches past the 32 prefetched self-attention keys, memory edges, and
the shapes the step refuses.  The product classes are driven as tests/test_gpu_decode_select.py drives them; the reference
is always ``oracle.cpu_path`` on the state cast to float64.  The guards that make the id comparisons meaningful are
asserted on the CPU in tests/test_decoder_shapes_cpu.py.

Bars: 1e-4 absolute on ``embed`` / ``logit`` / ``sampled_logprob``, the project's own
(tests/test_gpu_model.py::test_g3_decoder_forward_vs_reference_golden) - inherited, not fitted to these runs: the teacher-
forced inputs are the same plain procedural draws (float64 logits peak at 4-9), on which the oracle's own float32
evaluation sits 2-6e-6 from float64 (test_float32_oracle_is_well_inside_the_logit_bar).  Ids must be equal."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _decoder_shapes as S

pytestmark = pytest.mark.gpu

END = S.END
BAR = S.LOGIT_BAR


@functools.lru_cache(maxsize=None)
def _tf_model(sid):
    return S.product_model(sid, S.plain_state(sid))


@functools.lru_cache(maxsize=None)
def _search_model(sid, seed, end_beta=-3.0):
    return S.product_model(sid, S.diverse_state(sid, seed, end_beta))


def _route(monkeypatch, dec_row):
    if dec_row is None:
        monkeypatch.delenv("AUDIOCAPTION_DEC_ROW", raising=False)
    else:
        monkeypatch.setenv("AUDIOCAPTION_DEC_ROW", dec_row)


def _forward(sid, inp):
    dec = _tf_model(sid).decoder
    out = dec({"word": inp["word"].cuda(), "attn_emb": inp["attn_emb"].cuda(), "attn_emb_len": inp["attn_emb_len"],
               "cap_padding_mask": inp["cap_padding_mask"].cuda()})
    torch.cuda.synchronize()
    return out["embed"].cpu().double(), out["logit"].cpu().double()


def _worst(got, ref):
    """(max |got - ref|, the (row, position, column) where it sits)."""
    diff = (got - ref).abs()
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, float("inf")), diff)
    i = int(diff.argmax())
    return float(diff.reshape(-1)[i]), tuple(int(v) for v in np.unravel_index(i, diff.shape))


# (shape, AUDIOCAPTION_DEC_ROW): S0 again on the general launch sequence
TF_CASES = [(sid, None) for sid in sorted(S.SHAPES)] + [("S0", "gemm")]
TF_IDS = [sid + ("-" + r if r else "") for sid, r in TF_CASES]


# ----------------------------------------------------------------------------------------------------------------------
# a. teacher-forced forward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid,dec_row", TF_CASES, ids=TF_IDS)
def test_forward_of_100_positions_matches_float64(sid, dec_row, monkeypatch):
    """N = 3, T = 100 = max_pos; one row padded from position 50 on, one with pads at positions 5-8 only; memory lengths
    [Tm, Tm // 2, 1].  ``embed`` and the whole ``logit`` tensor within 1e-4 of float64."""
    _route(monkeypatch, dec_row)
    inp, ref = S.tf_reference(sid, 100, S.TF_TM[sid])
    embed, logit = _forward(sid, inp)
    de, at_e = _worst(embed, ref["embed"])
    dl, at_l = _worst(logit, ref["logit"])
    late = float((logit[:, 33:] - ref["logit"][:, 33:]).abs().max())
    route = "fused" if sid in S.FUSED and dec_row is None else "general"
    print(f"{sid} ({route}): max|logit - f64| {dl:.3e} at (row, pos, col) {at_l}, positions >= 33 {late:.3e}; "
          f"max|embed - f64| {de:.3e} at {at_e}")
    assert embed.shape == ref["embed"].shape and logit.shape == ref["logit"].shape
    assert de < BAR, (sid, "embed", de, at_e)
    assert dl < BAR, (sid, "logit", dl, at_l)


@pytest.mark.parametrize("T", [31, 32, 33, 34, 64])
@pytest.mark.parametrize("sid,dec_row", [("S0", None), ("S0", "gemm"), ("S2", None)], ids=["S0", "S0-gemm", "S2"])
def test_forward_across_the_prefetch_seam(sid, dec_row, T, monkeypatch):
    """Rows that end just before, on and just after the 32 prefetched keys: only positions >= 30 count, so a fault of the
    tail loops (newest key from this step's projection, mask bytes per key) is not averaged away by the early positions."""
    _route(monkeypatch, dec_row)
    inp, ref = S.tf_reference(sid, T, S.TF_TM[sid])
    embed, logit = _forward(sid, inp)
    de, at_e = _worst(embed[:, 30:], ref["embed"][:, 30:])
    dl, at_l = _worst(logit[:, 30:], ref["logit"][:, 30:])
    print(f"{sid} T {T}: positions >= 30 max|logit - f64| {dl:.3e} max|embed - f64| {de:.3e}")
    assert de < BAR, (sid, T, "embed", de, at_e)
    assert dl < BAR, (sid, T, "logit", dl, at_l)


# ----------------------------------------------------------------------------------------------------------------------
# b. memory edges
# ----------------------------------------------------------------------------------------------------------------------
# (Tm, N, T, lengths or None = [Tm, Tm // 2, 1])
MEMORY_CASES = {
    "Tm1": (1, 3, 4, (1, 1, 1)),
    "Tm32": (32, 3, 4, None),
    "Tm33": (33, 3, 4, None),
    "len1-in-200": (200, 3, 4, (1, 200, 1)),
    "Tm1024": (1024, 2, 3, (1024, 1000)),
}


@pytest.mark.parametrize("case", sorted(MEMORY_CASES))
@pytest.mark.parametrize("sid", ["S0", "S2"])
def test_forward_at_memory_edges(sid, case):
    """One frame, the 32-key prefetch boundary on both sides, MAX_KEYS = 1024 frames, and a clip of one valid frame inside
    a long memory (every other key masked by its length)."""
    Tm, N, T, lens = MEMORY_CASES[case]
    inp, ref = S.tf_reference(sid, T, Tm, N, lens)
    embed, logit = _forward(sid, inp)
    de, at_e = _worst(embed, ref["embed"])
    dl, at_l = _worst(logit, ref["logit"])
    print(f"{sid} {case}: max|logit - f64| {dl:.3e} max|embed - f64| {de:.3e}")
    assert de < BAR, (sid, case, "embed", de, at_e)
    assert dl < BAR, (sid, case, "logit", dl, at_l)


@pytest.mark.parametrize("sid", ["S0", "S2"])
def test_memory_beyond_max_keys_is_refused(sid):
    """1025 frames: ``ac_trm_memory`` rejects its arguments (AC_ERR_ARG) before it launches anything."""
    from audiocaption_amd import _lib
    dec = _tf_model(sid).decoder
    inp = S.tf_inputs(sid, 3, 1025, 2, (1025, 1000))
    with pytest.raises(_lib.HipLibraryError, match="ac_trm_memory"):
        dec.memory(inp["attn_emb"].cuda())
    with pytest.raises(_lib.HipLibraryError, match="ac_trm_memory"):
        dec({"word": inp["word"].cuda(), "attn_emb": inp["attn_emb"].cuda(), "attn_emb_len": inp["attn_emb_len"],
             "cap_padding_mask": inp["cap_padding_mask"].cuda()})
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# c. / d. greedy search past 32 positions
# ----------------------------------------------------------------------------------------------------------------------
def _greedy(model, emb, lens):
    out = model.forward_decoder({"mode": "inference", "sample_method": "greedy", "max_length": S.GREEDY_LEN},
                                {"attn_emb": emb.cuda(), "attn_emb_len": lens})
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", sorted(S.GREEDY_CASES))
def test_greedy_of_48_steps_matches_float64(case, monkeypatch):
    """4 clips, max_length 48 (the launch chain: the one-launch form stops at 32), no row ends.  Ids equal to the float64
    oracle's, ``sampled_logprob`` within 1e-4; the first call launches eagerly, the second replays the captured graph."""
    sid, seed, dec_row = S.GREEDY_CASES[case]
    _route(monkeypatch, dec_row)
    monkeypatch.setenv("AUDIOCAPTION_DECODE_GRAPH", "1")
    emb, lens, want = S.greedy_reference(sid, seed)
    model = _search_model(sid, seed)
    for call in ("eager", "graph"):
        out = _greedy(model, emb, lens)
        seq = out["seq"].numpy()
        bad = np.argwhere(seq != want["seq"].numpy())
        assert bad.size == 0, (case, call, "first differing (row, step)", bad[0].tolist())
        dlp, at = _worst(out["sampled_logprob"].double(), want["sampled_logprob"])
        print(f"{case} {call}: {want['steps']} steps, max|sampled_logprob - f64| {dlp:.3e} at (row, step) {at}")
        assert dlp < BAR, (case, call, dlp, at)
    assert not any(k[7] for k in model.decoder._greedy_state), "max_length 48 went to the one-launch form"
    assert any(st["graph"] is not None for st in model.decoder._greedy_state.values())


@pytest.mark.parametrize("case", sorted(S.STOP_CASES))
def test_greedy_rows_that_end_early_beside_long_rows(case, monkeypatch):
    """Some rows emit <end> within 5 steps, others run past 32 positions: ids identical, ``unfinished_cnt`` the oracle's
    count per step, every column past a row's end holds end_idx, ``sampled_logprob`` of the live steps within 1e-4."""
    sid, seed, beta = S.STOP_CASES[case]
    _route(monkeypatch, None)
    emb, lens, want = S.greedy_reference(sid, seed, beta)
    facts = S.greedy_facts(want)
    model = _search_model(sid, seed, beta)
    for call in ("eager", "graph"):
        out = _greedy(model, emb, lens)
        seq = out["seq"].numpy()
        np.testing.assert_array_equal(seq, want["seq"].numpy(), err_msg=f"{case} {call}")
        np.testing.assert_array_equal(out["unfinished_cnt"].cpu().numpy().astype(np.int64), facts["cnt"].numpy(),
                                      err_msg=f"{case} {call}: unfinished_cnt")
        for r, n in enumerate(facts["run_len"]):
            assert (seq[r, n:] == END).all(), (case, call, r)
        live = facts["live"]
        dlp = float((out["sampled_logprob"].double() - want["sampled_logprob"])[live].abs().max())
        print(f"{case} {call}: tokens before <end> {facts['run_len']}, steps {want['steps']}, "
              f"max|sampled_logprob - f64| over live steps {dlp:.3e}")
        assert dlp < BAR


def _s0_greedy_child(tmp_path, dec_row):
    """The S0 12-step greedy of tools/decoder_route_digest.py in a process of its own (AUDIOCAPTION_DEC_ROW=split is latched
    by a process's first decode step): (its digest line, the arrays it hashed)."""
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "decoder_route_digest.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("AUDIOCAPTION_DEC_")}
    env["AUDIOCAPTION_DECODE_GRAPH"] = "0"
    if dec_row is not None:
        env["AUDIOCAPTION_DEC_ROW"] = dec_row
    dump = str(tmp_path / f"{dec_row or 'default'}.npz")
    r = subprocess.run([sys.executable, tool, "--case", "S0-greedy", "--dump", dump], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    return r.stdout.strip().splitlines()[-1], dict(np.load(dump))


def test_greedy_with_the_row_sublayers_as_two_launches_matches_float64(tmp_path):
    """AUDIOCAPTION_DEC_ROW=split: dec_row_kernel once per attention sub-layer instead of one dec_row2_kernel.  Rows 0-2 and
    steps 0-11 of the S0 greedy draw (a prefix of ``S.greedy_reference``: no row ends, rows are independent): ids equal to
    the float64 oracle's and logits within 1e-4, for the two-launch form and, beside it, the default.  Whether the two
    forms give the same bits is printed, not asserted (profiles/decoder_step_refactor.txt)."""
    sid, seed, _ = S.GREEDY_CASES["S0"]
    want = S.greedy_reference(sid, seed)[2]
    got = {}
    for dec_row in ("split", None):
        line, out = _s0_greedy_child(tmp_path, dec_row)
        got[dec_row] = out
        rows, steps = out["seq"].shape
        assert (rows, steps) == (3, 12)
        dl, at = _worst(torch.from_numpy(out["logit"]).double(), want["logit"][:rows, :steps])
        print(f"{line}\n  max|logit - f64| {dl:.3e} at (row, step, col) {at}")
        bad = np.argwhere(out["seq"] != want["seq"][:rows, :steps].numpy())
        assert bad.size == 0, (dec_row, "first differing (row, step)", bad[0].tolist())
        assert dl < BAR, (dec_row, dl, at)
    same = all(np.array_equal(got["split"][k], got[None][k]) for k in got[None])
    print(f"two launches and one launch give {'the same bits' if same else 'different bits'}")


# ----------------------------------------------------------------------------------------------------------------------
# e. beam search past 32 positions
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(S.BEAM_CASES))
def test_beam_of_40_steps_matches_float64(case, monkeypatch):
    """Beam 3, 40 steps, temperature 1, 2 clips: ``row_div = beam`` in the cross-attention and ``ac_trm_beam_reorder`` at
    d != 256, past 32 positions.  Captions equal to ``O.beam_search`` in float64; every finished beam's length-normalised
    score within 1e-4 + 1e-6 |x| (the cumulative scores carry the reference's -1000 offsets, as in
    tests/test_gpu_decode_select.py).  Eager launches first, captured segments second."""
    sid, seed = S.BEAM_CASES[case]
    _route(monkeypatch, None)
    monkeypatch.setenv("AUDIOCAPTION_DECODE_GRAPH", "1")
    monkeypatch.delenv("AUDIOCAPTION_BEAM_SEGMENTS", raising=False)
    emb, lens, want, trace = S.beam_reference(sid, seed)
    model = _search_model(sid, seed)
    for call in ("eager", "graph"):
        req = model._inference_dict({"mode": "inference", "sample_method": "beam", "beam_size": S.BEAM,
                                     "max_length": S.BEAM_LEN, "temp": 1.0}, {"attn_emb": emb.cuda(), "attn_emb_len": lens})
        run = model._beam_begin(req)
        while model._beam_advance(run):
            pass
        out = model._beam_finish(run)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out["seq"].numpy(), want["seq"].numpy(), err_msg=f"{case} {call}")
        cnt = run["st"]["done_cnt"].cpu().numpy()
        score = run["st"]["done_score"].cpu().numpy().astype(np.float64)
        for c in range(len(S.BEAM_LENS)):
            ref = np.array(sorted((x for r in trace if r["clip"] == c for x in r["end_scores"]), reverse=True))
            assert int(cnt[c]) == len(ref), (case, call, c)
            got = np.sort(score[c, :len(ref)])[::-1]
            assert (np.abs(got - ref) <= 1e-4 + 1e-6 * np.abs(ref)).all(), (case, call, c, got - ref)
            assert abs(got[0] - float(want["score"][c])) <= 1e-4 + 1e-6 * abs(float(want["score"][c]))
        print(f"{case} {call}: 40 steps, best scores {[round(float(np.max(score[c, :cnt[c]])), 4) for c in range(len(cnt))]}")


# ----------------------------------------------------------------------------------------------------------------------
# f. refusals
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(S.REFUSED))
def test_unsupported_shapes_are_refused_before_anything_exists(name):
    """On the device: ``weights()`` raises, naming the limit, and so does every entry that would build on it - before a
    packed copy, a workspace, a memory projection or a captured graph exists (no device memory is taken by the attempts)."""
    import audiocaption_amd as A
    from audiocaption_amd import _lib, build
    build.build()
    dec = S.refused_decoder(name).to("cuda:0")
    model = A.TransformerModel(torch.nn.Identity(), dec).eval()
    emb = torch.zeros(2, 4, dec.attn_emb_dim, device="cuda:0")
    lens = torch.tensor([4, 2])
    word = torch.full((2, 3), S.START, device="cuda:0")
    mask = word == S.PAD
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    calls = {
        "weights": dec.weights,
        "workspace": lambda: dec.workspace(2, 3, emb.device),
        "memory": lambda: dec.memory(emb),
        "forward": lambda: dec({"word": word, "attn_emb": emb, "attn_emb_len": lens, "cap_padding_mask": mask}),
        "greedy": lambda: model.forward_decoder({"mode": "inference", "sample_method": "greedy", "max_length": 5},
                                                {"attn_emb": emb, "attn_emb_len": lens}),
        "beam": lambda: model.forward_decoder({"mode": "inference", "sample_method": "beam", "beam_size": 2, "max_length": 5},
                                              {"attn_emb": emb, "attn_emb_len": lens}),
    }
    for what, call in calls.items():
        with pytest.raises(_lib.HipLibraryError, match=S.REFUSED[name][1]) as e:
            call()
        assert "Supported:" in str(e.value), what
        del e            # (the traceback would keep the refused call's frames alive)
    torch.cuda.synchronize()
    assert dec._w is None and dec._ws == {} and not dec._greedy_state and not getattr(model, "_beam_state", None)
    assert torch.cuda.memory_allocated() == before
