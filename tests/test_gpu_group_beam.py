"""Group (diverse) beam search on the GPU: ``ac_group_beam_select`` (csrc/group_beam.hip) on synthetic logits against float64
numpy, and ``TransformerModel.group_beam_search`` end to end against the reference's own results in
tests/golden/g_group_beam.npz (tests/test_group_beam_cpu.py holds the tie guards of those cases).

Which kernel a vocabulary reaches: V <= 5120 ``group_beam_row_kernel<20>``, 5120 < V <= 8192 ``<32>``; V = 100 leaves most
threads of the workgroup without a column."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _group_beam_ref as R

pytestmark = pytest.mark.gpu

END = R.END
MARGIN = R.MARGIN
B = 2


def _tol(ref):
    """|kernel - float64| allowed for a score (tests/test_gpu_decode_select.py): the cumulative scores carry -1000 offsets."""
    return 1e-4 + 1e-6 * np.abs(ref)


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


# ---- the selection kernel ------------------------------------------------------------------------------------------------------
def _log_softmax64(x):
    m = x.max(axis=1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True))


def _reference(z, cum, prev_words, bdash, V, lt, temp, lam):
    """float64: per clip the stable descending order of the candidates (flattened ids, values), bdash + 1 of them."""
    lp = _log_softmax64(_log_softmax64(z.astype(np.float64)) / temp)
    out = []
    for c in range(z.shape[0] // bdash):
        count = np.zeros(V)
        for w in prev_words[c]:
            count[w] += 1
        cand = cum[c * bdash:(c + 1) * bdash, None].astype(np.float64) + (lp[c * bdash:(c + 1) * bdash] - count[None] * lam)
        flat = cand[0] if lt == 0 else cand.reshape(-1)
        order = np.argsort(-flat, kind="stable")[:bdash + 1]
        out.append((order, flat[order]))
    return out


def _draw(V, bdash, n_prev, lt, temp, lam, seed):
    """Logits, cumulative scores (one finished beam at -1000 when the step has several rows) and the earlier groups' words:
    word 0, word V - 1, end_idx, and the clip's strongest words - one of them twice (count 2) - so that the penalty moves
    the selection; the rest random."""
    rng = np.random.default_rng(seed)
    R_ = B * bdash
    z = (rng.standard_normal((R_, V)) * 3.0).astype(np.float32)
    cum = rng.uniform(-12.0, 0.0, size=R_).astype(np.float32)
    if bdash > 1:
        cum[bdash - 1] -= 1000.0
    prev_words = []
    for c in range(B):
        strong = np.argsort(-z[c * bdash])[:3].tolist()
        words = ([strong[0], strong[0], 0, V - 1, END, strong[1], strong[2]] + rng.integers(0, V, size=64).tolist())[:n_prev * bdash]
        prev_words.append(words)
    return z, cum, prev_words


def _planes(prev_words, bdash, n_prev, lt, tok_ld, V, seed):
    """n_prev token planes [B * bdash][tok_ld]: column lt + 1 holds the words (group q, row j of clip c = word q * bdash + j),
    every other column other words - a kernel that read another column would count them."""
    rng = np.random.default_rng(seed + 1)
    planes = rng.integers(0, V, size=(n_prev, B * bdash, tok_ld)).astype(np.int32)
    for c in range(B):
        for q in range(n_prev):
            for j in range(bdash):
                planes[q, c * bdash + j, lt + 1] = prev_words[c][q * bdash + j]
    return [torch.from_numpy(p).cuda() for p in planes]


def _launch(lib, z, cum, planes, bdash, V, lt, temp, lam, ldl=None, n_prev=None):
    from audiocaption_amd import _lib
    P = _lib.ptr
    ldl = V if ldl is None else ldl
    n_prev = len(planes) if n_prev is None else n_prev
    R_ = z.shape[0]
    d_z = torch.full((R_, ldl), 1e30, dtype=torch.float32, device="cuda")       # beyond V: values that would win if read
    d_z[:, :V] = torch.from_numpy(z).cuda()
    d_cum = torch.from_numpy(cum).cuda()
    top_val = torch.full((R_ // bdash, bdash), -7.0, device="cuda")
    top_idx = torch.full((R_ // bdash, bdash), -7, dtype=torch.int32, device="cuda")
    scratch = torch.empty(2 * R_ * bdash, device="cuda")
    arr = (ctypes.c_void_p * max(n_prev, 1))(*[p.data_ptr() for p in planes[:n_prev]]) if n_prev else None
    tok_ld = planes[0].shape[1] if planes else lt + 2
    rc = lib.ac_group_beam_select(P(d_z), ldl, R_ // bdash, bdash, V, lt, temp, lam, P(d_cum), arr, n_prev, tok_ld,
                                  P(top_val), P(top_idx), P(scratch), _lib.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return top_val.cpu().numpy(), top_idx.cpu().numpy()


def _case(V, bdash, n_prev, lt, temp, lam):
    """The first draw whose float64 candidates are >= MARGIN apart among the kept and to the first cut."""
    for seed in range(40):
        z, cum, prev_words = _draw(V, bdash, n_prev, lt, temp, lam, seed)
        ref = _reference(z, cum, prev_words, bdash, V, lt, temp, lam)
        if min(float(np.min(v[:-1] - v[1:])) for _, v in ref) >= MARGIN:
            return z, cum, prev_words, ref, seed
    raise AssertionError(("no draw without near ties", V, bdash, n_prev, lt, temp, lam))


COMBOS = list(itertools.product((0, 1, 7), (0, 5), (0.5, 1.0, 1.7), (0.0, 0.5, 3.0)))   # n_prev, lt, temp, lambda


@pytest.mark.parametrize("bdash", [1, 3, 8])
@pytest.mark.parametrize("V", [100, 5120, 5121, 8192])
def test_select_matches_float64(lib, V, bdash):
    """Ids equal to the float64 reference's (its gaps are >= 1e-3, asserted), values within 1e-4 + 1e-6 |ref|, over n_prev
    x lt x temp x lambda; the penalty changes the kept set in some of them."""
    moved = 0
    for n_prev, lt, temp, lam in COMBOS:
        z, cum, prev_words, ref, seed = _case(V, bdash, n_prev, lt, temp, lam)
        planes = _planes(prev_words, bdash, n_prev, lt, lt + 4, V, seed)
        val, idx = _launch(lib, z, cum, planes, bdash, V, lt, temp, lam)
        plain = _reference(z, cum, [[]] * B, bdash, V, lt, temp, lam)
        for c, (order, want) in enumerate(ref):
            where = (V, bdash, n_prev, lt, temp, lam, c)
            assert float(np.min(want[:-1] - want[1:])) >= MARGIN, where
            np.testing.assert_array_equal(idx[c], order[:bdash], err_msg=str(where))
            assert (np.abs(val[c] - want[:bdash]) <= _tol(want[:bdash])).all(), (where, val[c] - want[:bdash])
            moved += int(not np.array_equal(order[:bdash], plain[c][0][:bdash]))
    assert moved > 0, "the penalty never changed a selection: the comparison could not tell it from none"


def test_select_with_a_row_stride_above_v(lib):
    V, bdash, n_prev, lt, temp, lam = 5121, 3, 1, 5, 1.7, 0.5
    z, cum, prev_words, ref, seed = _case(V, bdash, n_prev, lt, temp, lam)
    planes = _planes(prev_words, bdash, n_prev, lt, lt + 2, V, seed)
    val, idx = _launch(lib, z, cum, planes, bdash, V, lt, temp, lam, ldl=V + 7)
    for c, (order, want) in enumerate(ref):
        np.testing.assert_array_equal(idx[c], order[:bdash])
        assert (np.abs(val[c] - want[:bdash]) <= _tol(want[:bdash])).all()


@pytest.mark.parametrize("V", [100, 8192])
def test_lambda_zero_carries_the_bits_of_the_unpenalised_scores(lib, V):
    bdash, lt = 3, 5
    z, cum, _ = _draw(V, bdash, 3, lt, 1.0, 0.0, 5)
    v0, i0 = _launch(lib, z, cum, [], bdash, V, lt, 1.7, 0.0)
    prev_words = [[int(i0[c, 0]) % V] * (3 * bdash) for c in range(B)]   # every earlier row holds the clip's winning word
    planes = _planes(prev_words, bdash, 3, lt, lt + 2, V, 5)
    v3, i3 = _launch(lib, z, cum, planes, bdash, V, lt, 1.7, 0.0)
    np.testing.assert_array_equal(v0.view(np.int32), v3.view(np.int32))
    np.testing.assert_array_equal(i0, i3)
    vp, _ = _launch(lib, z, cum, planes, bdash, V, lt, 1.7, 0.5)        # and the planes ARE read: lambda 0.5 costs it 4.5
    assert (vp[:, 0] < v0[:, 0]).all()


@pytest.mark.parametrize("V", [100, 8192])
def test_penalty_is_one_product_and_one_subtraction_in_f32(lib, V):
    """With cum = 0 the kernel's value of a word is lp itself (lambda 0), so the penalised value must be
    fl(lp - fl(3 * lambda)) bit for bit.  lambda = 1000.1: the product (about 3000.3, ulp 2.4e-4) does round, by an amount
    of the order of the result's own ulp, so a fused multiply-add - one rounding - gives another float for many of the
    words.  Eight words in different registers of different threads carry the row; every other word sits 20000 below, so
    the eight stay the selection under the penalty."""
    bdash, lam, times = 8, 1000.1, 3
    words = [0, 1, 2, 50, 63, 64, 98, 99] if V == 100 else [0, 255, 256, 300, 5119, 5120, 7000, 8191]
    rng = np.random.default_rng(11)
    z = np.full((B * bdash, V), -20000.0, np.float32)
    z[:, words] = (rng.standard_normal((B * bdash, len(words))) * 3.0).astype(np.float32)
    cum = np.zeros(B * bdash, np.float32)
    v0, i0 = _launch(lib, z, cum, [], bdash, V, 0, 1.0, 0.0)
    assert all(sorted(i0[c].tolist()) == words for c in range(B))
    planes = _planes([sorted(words * times)] * B, bdash, times, 0, 2, V, 11)      # each of the eight three times
    vp, ip = _launch(lib, z, cum, planes, bdash, V, 0, 1.0, lam)
    pen = np.float32(times) * np.float32(lam)
    assert float(pen) != times * float(np.float32(lam))                           # the product does round
    fused = 0
    for c in range(B):
        assert sorted(ip[c].tolist()) == words
        lp = dict(zip(i0[c].tolist(), v0[c]))
        for w, v in zip(ip[c].tolist(), vp[c]):
            want = np.float32(lp[w] - pen)
            assert v.view(np.int32) == want.view(np.int32), (c, w, v, want)
            fused += int(np.float32(float(lp[w]) - times * float(np.float32(lam))) != want)
    assert fused > 0, "a fused multiply-add would give the same floats here: the comparison could not tell"


@pytest.mark.parametrize("V", [100, 5121])
def test_exact_ties(lib, V):
    """Two equal logits above all others: unpenalised the lower index is picked first with the same value; one earlier
    choice of the lower one and the higher index wins."""
    bdash, lo, hi = 2, 7, V - 1
    z = np.zeros((B * bdash, V), np.float32)
    z[:, lo] = z[:, hi] = 4.0
    z[:, 50] = 2.0
    cum = np.zeros(B * bdash, np.float32)
    words = [[lo, 50], [lo, 50]]                                       # group 0's two rows per clip
    planes = _planes(words, bdash, 1, 0, 3, V, 0)
    val, idx = _launch(lib, z, cum, planes, bdash, V, 0, 1.0, 0.5, n_prev=0)
    assert idx.tolist() == [[lo, hi]] * B and (val[:, 0] == val[:, 1]).all()
    val, idx = _launch(lib, z, cum, planes, bdash, V, 0, 1.0, 0.5)
    assert idx.tolist() == [[hi, lo]] * B
    np.testing.assert_array_equal(val[:, 1], val[:, 0] - np.float32(0.5))   # x - 1 * 0.5, rounded once
    # at lt > 0 the tie is between rows: the lower FLATTENED index (row 0) first
    planes = _planes(words, bdash, 1, 1, 3, V, 0)
    z[:, hi] = 0.0
    val, idx = _launch(lib, z, cum, planes, bdash, V, 1, 1.0, 0.5, n_prev=0)
    assert idx.tolist() == [[lo, V + lo]] * B and (val[:, 0] == val[:, 1]).all()


def test_select_refuses_bad_arguments(lib):
    from audiocaption_amd import _lib
    P = _lib.ptr
    V, bdash, lt = 100, 3, 1
    z = torch.zeros(B * bdash, V, device="cuda")
    cum = torch.zeros(B * bdash, device="cuda")
    planes = [torch.zeros(B * bdash, 21, dtype=torch.int32, device="cuda") for _ in range(8)]
    top_val = torch.full((B, bdash), -7.0, device="cuda")
    top_idx = torch.full((B, bdash), -7, dtype=torch.int32, device="cuda")
    scratch = torch.empty(2 * B * 9 * 9, device="cuda")
    arr = (ctypes.c_void_p * 8)(*[p.data_ptr() for p in planes])

    def call(**over):
        a = dict(logit=P(z), ldl=V, B=B, bdash=bdash, V=V, lt=lt, temp=1.0, lam=0.5, cum=P(cum), prev=arr, n_prev=2, tok_ld=21,
                 top_val=P(top_val), top_idx=P(top_idx), scratch=P(scratch))
        a.update(over)
        return lib.ac_group_beam_select(a["logit"], a["ldl"], a["B"], a["bdash"], a["V"], a["lt"], a["temp"], a["lam"],
                                        a["cum"], a["prev"], a["n_prev"], a["tok_ld"], a["top_val"], a["top_idx"], a["scratch"],
                                        _lib.stream())
    nul = (ctypes.c_void_p * 2)(planes[0].data_ptr(), None)
    for over in (dict(bdash=0), dict(bdash=9), dict(n_prev=-1), dict(n_prev=8), dict(V=0), dict(V=8193, ldl=8193),
                 dict(ldl=V - 1), dict(lt=-1), dict(temp=0.0), dict(temp=-1.0), dict(temp=float("nan")),
                 dict(temp=float("inf")), dict(lam=-0.1), dict(lam=float("nan")), dict(lam=float("inf")), dict(logit=None),
                 dict(cum=None), dict(top_val=None), dict(top_idx=None), dict(scratch=None), dict(prev=None), dict(prev=nul)):
        assert call(**over) == _lib.AC_ERR_ARG, over
    torch.cuda.synchronize()
    assert (top_val == -7.0).all() and (top_idx == -7).all()       # nothing was launched
    assert call() == 0 and call(n_prev=0, prev=None) == 0 and call(n_prev=7) == 0
    torch.cuda.synchronize()
    assert (top_idx >= 0).all()


# ---- TransformerModel end to end -----------------------------------------------------------------------------------------------
def _model(V):
    import audiocaption_amd as A
    from audiocaption_amd import build
    build.build()
    dec = A.TransformerDecoder(emb_dim=256, vocab_size=V, fc_emb_dim=512, attn_emb_dim=512, dropout=0.2, nlayers=2)
    dec.load_state_dict({k[len("decoder."):]: v for k, v in R.state(V).items()}, strict=True)
    return A.TransformerModel(torch.nn.Identity(), dec).eval().to("cuda:0")


def _enc(spec):
    emb, lens = R.clips(spec)
    return {"attn_emb": emb.cuda(), "attn_emb_len": lens}


def _req(case, **over):
    _, G, bdash, beam, lam, temp, L, V = case
    d = {"mode": "inference", "sample_method": "beam", "beam_size": beam, "group_size": G, "diversity_lambda": lam,
         "temp": temp, "max_length": L}
    d.update(over)
    return d


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_ids_match_the_reference(case, monkeypatch):
    """The reference's own captions, in both result shapes; the eager first call, the captured second and the replayed
    third agree, and so does a model that never captures.  Ragged memory lengths including 1."""
    monkeypatch.setenv("AUDIOCAPTION_DECODE_GRAPH", "1")
    cid, G, bdash, beam, _, _, L, V = case
    f = R.fixture()
    spec = R.case_clips(cid)
    assert any(ln == 1 for _, ln in spec) and len({ln for _, ln in spec}) > 1
    model = _model(V)
    want = f[f"{cid}/seq"]
    for call in range(3):
        out = model.forward_decoder(_req(case), _enc(spec))
        assert out["seq"].dtype == torch.int64 and out["seq"].device.type == "cpu" and tuple(out["seq"].shape) == (3, beam, L)
        np.testing.assert_array_equal(out["seq"].numpy(), want, err_msg=f"call {call}")
    (st,) = model._group_beam_state.values()
    assert st["uses"] == 3 and st["graph"] is not None and len(st["books"]) == G
    assert (out["seq"][:, G * bdash:] == END).all()
    assert tuple(out["logit"].shape) == (3, L, V) and tuple(out["sampled_logprob"].shape) == (3, L)
    assert tuple(out["embed"].shape) == (3, L, model.decoder.d_model) and "seq_dev" not in out
    best = model.forward_decoder(_req(case, group_nbest=False), _enc(spec))
    assert tuple(best["seq"].shape) == (3, G, L)
    np.testing.assert_array_equal(best["seq"].numpy(), f[f"{cid}/seq_best"])
    assert len(model._group_beam_state) == 2
    monkeypatch.setenv("AUDIOCAPTION_DECODE_GRAPH", "0")
    eager = _model(V)
    for _ in range(2):
        np.testing.assert_array_equal(eager.forward_decoder(_req(case), _enc(spec))["seq"].numpy(), want)
    assert all(st["graph"] is None for st in eager._group_beam_state.values())


def test_defaults_and_the_whole_model_call():
    """``model(input_dict)`` with ``group_size`` alone: beam_size 6, lambda 0.5, group_nbest - case 0's request."""
    case = R.CASES[0]
    model = _model(case[7])
    out = model(dict(_enc(R.case_clips(case[0])), mode="inference", sample_method="beam", group_size=3, max_length=case[6]))
    np.testing.assert_array_equal(out["seq"].numpy(), R.fixture()[f"{case[0]}/seq"])


def test_cached_states_are_reused_and_leave_plain_beam_search_alone():
    case = R.CASES[0]
    cid, V = case[0], case[7]
    spec = R.case_clips(cid)
    plain_req = {"mode": "inference", "sample_method": "beam", "beam_size": 3, "max_length": case[6]}
    fresh = _model(V).forward_decoder(dict(plain_req), _enc(spec))["seq"]
    with torch.no_grad():
        want_other = R.run_case(case, spec, diversity_lambda=R.OTHER_LAMBDA)["seq"].numpy()
    want = R.fixture()[f"{cid}/seq"]
    assert not np.array_equal(want_other, want)
    model = _model(V)
    np.testing.assert_array_equal(model.forward_decoder(_req(case), _enc(spec))["seq"].numpy(), want)
    np.testing.assert_array_equal(model.forward_decoder(_req(case, diversity_lambda=R.OTHER_LAMBDA), _enc(spec))["seq"].numpy(), want_other)
    assert len(model._group_beam_state) == 2
    assert torch.equal(model.forward_decoder(dict(plain_req), _enc(spec))["seq"], fresh)
    assert torch.equal(model.forward_decoder(dict(plain_req, group_size=None), _enc(spec))["seq"], fresh)
    assert len(model._group_beam_state) == 2 and len(model._beam_state) == 1      # group_size=None: the plain search's own state
    # back to the first state (captured now), with other clips in between the results stay those of the request
    np.testing.assert_array_equal(model.forward_decoder(_req(case), _enc(spec))["seq"].numpy(), want)
    np.testing.assert_array_equal(model.forward_decoder(_req(case, diversity_lambda=R.OTHER_LAMBDA), _enc(spec))["seq"].numpy(), want_other)
    assert [st["uses"] for st in model._group_beam_state.values()] == [2, 2]
    assert torch.equal(model.forward_decoder(dict(plain_req), _enc(spec))["seq"], fresh)


def test_seq_dev_goes_into_score_groups_as_it_lies():
    import _diversity_ref as D
    from audiocaption_amd import Diversity
    case = R.CASES[0]
    V = case[7]
    model = _model(V)
    out = model.forward_decoder(_req(case, _seq_on_device=True), _enc(R.case_clips(case[0])))
    seq_dev = out["seq_dev"]
    assert seq_dev.is_cuda and seq_dev.dtype == torch.int64 and torch.equal(seq_dev.cpu(), out["seq"])
    scorer = Diversity()
    got = scorer.score_groups(D.ListVocabulary(D.word_list(V)), V, seq_dev, R.START, END)
    assert tuple(got["group_mean"].shape) == (3, 5) and tuple(got["self_bleu"].shape) == (3 * case[3],)
    assert bool(torch.isfinite(got["summary"]).all())
