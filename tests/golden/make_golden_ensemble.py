"""Generate g16_ensemble.npz by running the REFERENCE's ``EnsembleRunner`` (python_scripts/train_eval/ensemble.py:
stepwise_forward :94-151, beam_search :154-276, sample_next_word_with_logprob :412-449) on CPU.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_ensemble.py

``ensemble.py`` is imported by file path under the inert stubs of make_golden.py plus stubs for what only its command
line needs (fire, tqdm, pandas, pycocoevalcap, the encoder / decoder registries, build_vocab, the base runner, datasets).
Members are reference ``TransformerModel``s at the real size (d 256, V 4981) whose encoder is ``nn.Identity()``, fed their
encoder outputs directly.  The fixture stores the RECIPE of the members, not their tensors:

  * weights: ``procedural.decoder_state_diverse`` draw 1 = "greedy", 2 = "beam" (``members``);
  * memory: g3_decoder.npz's attn_emb (4 x 31 x 512, its own lengths) with the feature axis rolled by the member's index;
    in the ``short`` variant member SHORT_MEMBER's memory is truncated to 24 frames (lengths clipped), so that members
    with different memory lengths decode together.

Member sets are tried in order until the reference's own outputs make a test that can fail (asserted below): no caption is
<end> alone; every clip's ensemble caption differs from what each member decodes alone under the same rule; greedy clips
finish at different steps; a beam clip finishes early while another runs to the end; the never-retiring search returns
something else than base.py's early stop would on at least one clip; every greedy top-1 / top-2 gap on a live step and
every beam margin at the cut is >= 1e-4 (the parity gate the GPU path is held to).  The CPU restatement
tests/_ensemble_ref.py is compared with the reference here as well.

What is the reference's own and what is not: every id (greedy, beam, n-best) is EnsembleRunner's output; the greedy values
(m[word], top-8 of m, gaps) come from the m the reference hands to its own sample_next_word_with_logprob, recorded by a
wrapper; the sampling distributions, words and stored values are the reference's.  The beam margins and the n-best SCORES
are the restatement's (the reference keeps its finished beams in a local variable): only the n-best ids and their order
are reference-pinned.
"""
import importlib.util
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

V = 4981
MAXLEN = 20
SHORT_MEMBER, SHORT_TM = 1, 24
# (decoder draw per member, roll step): member n's memory is rolled by n * step features
CANDIDATES = [(d, r) for r in (200, 1, 3, 7, 16, 64, 128, 5, 11, 32) for d in ([1, 2, 1], [2, 2], [2, 2, 1], [2, 1, 2])]
KIND = {1: "greedy", 2: "beam"}
SAMPLE_METHODS = ["sample", "top5", "top0.9", "gumbel"]
SAMPLE_TEMPS = [0.7, 1.0]
SAMPLE_ROWS, SAMPLE_MEMBERS, SAMPLE_SEED = 3, 3, 16
GATE = 1e-4


def _install_stubs():
    from make_golden import _install_stubs as base
    base()

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("fire", Fire=lambda *a, **k: None)
    mod("tqdm", tqdm=lambda *a, **k: None)
    mod("pandas")
    mod("pycocoevalcap")
    mod("pycocoevalcap.cider")
    mod("pycocoevalcap.cider.cider", Cider=object)
    import captioning.models  # noqa: F401  (reference)
    mod("captioning.models.encoder")
    mod("captioning.models.decoder")
    mod("captioning.utils.build_vocab", Vocabulary=object)
    mod("captioning.pytorch_runners")
    mod("captioning.pytorch_runners.base", BaseRunner=object)
    mod("captioning.datasets")


def sample_planes():
    """The member logit planes of the sampling cases (SAMPLE_MEMBERS x SAMPLE_ROWS x V): a recipe the tests repeat."""
    g = np.random.default_rng(SAMPLE_SEED)
    return (g.normal(0.0, 2.5, (SAMPLE_MEMBERS, SAMPLE_ROWS, V))).astype(np.float32)


def member_memory(attn_emb, lens, index, short):
    mem = np.roll(attn_emb, index, axis=2)   # index = member index * roll step
    ln = lens.copy()
    if short:
        mem, ln = mem[:, :SHORT_TM], np.minimum(ln, SHORT_TM)
    return np.ascontiguousarray(mem), ln


def main():
    _install_stubs()
    torch.manual_seed(16)
    torch.set_grad_enabled(False)
    from captioning.models.transformer_decoder import TransformerDecoder   # reference
    from captioning.models.transformer_model import TransformerModel       # reference
    from audiocaption_amd import procedural as P
    import _ensemble_ref as E

    spec = importlib.util.spec_from_file_location("ref_ensemble", os.path.join(REF, "python_scripts/train_eval/ensemble.py"))
    ens = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ens)

    g3 = np.load(os.path.join(HERE, "g3_decoder.npz"))
    attn_emb, lens = g3["attn_emb"], g3["attn_emb_len"].astype(np.int64)
    B = attn_emb.shape[0]
    states = {k: P.to_torch(P.decoder_state_diverse(KIND[k], prefix="decoder.", vocab_size=V)) for k in KIND}

    def ref_model(draw):
        dec = TransformerDecoder(emb_dim=256, vocab_size=V, fc_emb_dim=512, attn_emb_dim=512, dropout=0.2)
        dec.load_state_dict({k[len("decoder."):]: v for k, v in states[draw].items()}, strict=True)
        return TransformerModel(nn.Identity(), dec).eval()

    def members_of(cand, short=False, only=None):
        """(reference models, reference input dicts, restatement members) of a member set (``only``: one member alone,
        with the memory it has inside the set)."""
        models, inputs, mine = [], [], []
        draws, step = cand
        for n, d in enumerate(draws):
            if only is not None and n != only:
                continue
            mem, ln = member_memory(attn_emb, lens, n * step, short and n == SHORT_MEMBER)
            mem_t, ln_t = torch.from_numpy(mem), torch.from_numpy(ln)
            models.append(ref_model(d))
            # the tensor must be the FIRST value of the dict (ensemble.py:98)
            inputs.append({"attn_emb": mem_t, "attn_emb_len": ln_t, "fc_emb": mem_t.mean(1), "mode": "inference"})
            mine.append({"state": states[d], "attn_emb": mem_t, "attn_emb_len": ln_t})
        return models, inputs, mine

    def runner(**args):
        r = ens.EnsembleRunner()
        r.device = "cpu"
        r.vocabulary = range(V)
        r.start_idx, r.end_idx, r.pad_idx = 1, 2, 0
        base = {"max_length": MAXLEN, "method": "greedy", "sample_word_temp": 1.0, "beam_size": 3, "beam_temp": 1.0,
                "n_best": False, "n_best_size": 3}
        base.update(args)
        r.eval_config = {"inference_args": base}
        return r

    def ref_greedy(draws, short=False, only=None, record=None):
        """The reference's greedy ids; ``record`` (a list) receives the mean log-probabilities m (B, V) the reference hands
        to its own ``sample_next_word_with_logprob`` at every step."""
        models, inputs, _ = members_of(draws, short, only)
        r = runner(method="greedy")
        if record is not None:
            pick = r.sample_next_word_with_logprob

            def recording(logprob, method, temp):
                record.append(logprob.detach().clone())
                return pick(logprob, method=method, temp=temp)

            r.sample_next_word_with_logprob = recording
        return r.stepwise_forward(models, inputs)["seq"]

    def ref_greedy_values(seq, ms, mine):
        """m[word], the top-8 of m and its top-1 / top-2 gap on every live step (up to and including a row's first <end>),
        all from the REFERENCE's recorded m; the restatement ``mine`` must agree within 1e-5."""
        value, gap = torch.zeros(B, MAXLEN), torch.full((B, MAXLEN), float("inf"))
        top_val, top_idx = torch.zeros(B, MAXLEN, 8), torch.zeros(B, MAXLEN, 8, dtype=torch.long)
        for i, row in enumerate(seq.tolist()):
            for t in range(E.first_end(row)):
                tv, ti = ms[t][i].topk(8)
                assert int(ti[0]) == row[t]
                value[i, t], gap[i, t], top_val[i, t], top_idx[i, t] = ms[t][i, row[t]], tv[0] - tv[1], tv, ti
        assert torch.equal(top_idx, mine["top_idx"]) and torch.equal(torch.isinf(gap), torch.isinf(mine["gap"]))
        live = ~torch.isinf(gap)
        assert float((value - mine["sampled_logprob"]).abs().max()) < 1e-5 and float((top_val - mine["top_val"]).abs().max()) < 1e-5
        assert float((gap[live] - mine["gap"][live]).abs().max()) < 1e-5
        return value, gap, top_val, top_idx

    def ref_beam(draws, k, n_best=False, short=False, only=None):
        models, inputs, _ = members_of(draws, short, only)
        return runner(method="beam", beam_size=k, n_best=n_best, n_best_size=k).beam_search(models, inputs)["seq"]

    def caps(seq):
        return [tuple(r[:E.first_end(r)]) for r in seq.tolist()]

    report = []

    def try_set(draws):
        """The fixture entries of one member set, or the reason it is useless."""
        out = {}
        M = len(draws[0])
        _, _, mine = members_of(draws)
        # ---- greedy ----
        ref_ms = []
        ref_g = ref_greedy(draws, record=ref_ms)
        my_g = E.greedy(mine, MAXLEN)
        rc, mc = caps(ref_g), caps(my_g["seq"])
        assert rc == mc, ("restatement differs from the reference (greedy)", rc, mc)
        if any(c == (2,) for c in rc):
            return None, "a greedy caption is <end> alone"
        ends = [len(c) for c in rc if c[-1] == 2]
        if len(ends) < 2 or len(set(ends)) < 2:
            return None, f"greedy: fewer than two clips finish early at different steps ({[len(c) for c in rc]})"
        g_value, g_gap, g_top_val, g_top_idx = ref_greedy_values(ref_g, ref_ms, my_g)
        gap = float(g_gap.min())
        if gap < GATE:
            return None, f"greedy top-1 / top-2 gap {gap:.2e}"
        for n in range(M):
            alone = caps(ref_greedy(draws, only=n))
            same = [i for i in range(B) if alone[i] == rc[i]]
            if same:
                return None, f"greedy: member {n} alone gives the ensemble caption of clips {same}"
        # ids and values are the reference's (greedy_seq: its ids up to each row's first <end>, <end> afterwards)
        out.update(greedy_seq=my_g["seq"].numpy(), greedy_value=g_value.numpy(), greedy_gap=g_gap.numpy(),
                   greedy_top_val=g_top_val.numpy(), greedy_top_idx=g_top_idx.numpy().astype(np.int32))
        msg = [f"greedy lengths {[len(c) for c in rc]} min gap {gap:.2e}"]
        # ---- beam 3 / 4 ----
        differs_from_retiring = False
        for k in (3, 4):
            ref_b = ref_beam(draws, k)
            ref_nb = ref_beam(draws, k, n_best=True)
            trace = []
            my_b = E.beam_search(mine, k, MAXLEN, trace=trace)
            my_nb = E.beam_search(mine, k, MAXLEN, n_best=True, n_best_size=k)
            assert torch.equal(ref_b, my_b["seq"]), ("restatement differs from the reference (beam)", k)
            assert torch.equal(ref_nb, my_nb["seq"]), ("restatement differs from the reference (n-best)", k)
            bc = caps(ref_b)
            if any(c == (2,) for c in bc):
                return None, f"a beam {k} caption is <end> alone"
            margin = min(r["margin"] for r in trace)
            if margin < GATE:
                return None, f"beam {k} margin {margin:.2e}"
            sc = my_nb["nbest_score"]
            nb_gap = float((sc[:, :-1] - sc[:, 1:]).min())
            if nb_gap < GATE:
                return None, f"beam {k}: n-best scores {nb_gap:.2e} apart"
            lengths = [len(c) if c[-1] == 2 else MAXLEN + 1 for c in bc]
            if k == 3 and not (min(lengths) < MAXLEN and max(lengths) >= MAXLEN):
                return None, f"beam 3: no clip finishes early or none runs to the end ({lengths})"
            for n in range(M):
                alone = caps(ref_beam(draws, k, only=n))
                same = [i for i in range(B) if alone[i] == bc[i]]
                if same:
                    return None, f"beam {k}: member {n} alone gives the ensemble caption of clips {same}"
            retiring = caps(E.beam_search(mine, k, MAXLEN, retire=True)["seq"])
            diff = [i for i in range(B) if retiring[i] != bc[i]]
            differs_from_retiring |= bool(diff)
            out[f"beam{k}_seq"] = ref_b.numpy()
            out[f"beam{k}_nbest"] = ref_nb.numpy()
            out[f"beam{k}_nbest_score"] = sc.numpy()
            out[f"beam{k}_margin"] = np.array(margin)
            out[f"beam{k}_retiring_differs"] = np.array(diff, dtype=np.int64)
            msg.append(f"beam {k} lengths {lengths} margin {margin:.2e} n-best gap {nb_gap:.2e} retiring differs on {diff}")
        if not differs_from_retiring:
            return None, "the never-retiring search equals the retiring one on every clip"
        # ---- one member with a shorter memory ----
        _, _, mine_s = members_of(draws, short=True)
        ref_ms_s = []
        ref_gs, my_gs = ref_greedy(draws, short=True, record=ref_ms_s), E.greedy(mine_s, MAXLEN)
        assert caps(ref_gs) == caps(my_gs["seq"])
        s_value, s_gap, _, _ = ref_greedy_values(ref_gs, ref_ms_s, my_gs)
        ref_bs, tr = ref_beam(draws, 3, short=True), []
        my_bs = E.beam_search(mine_s, 3, MAXLEN, trace=tr)
        assert torch.equal(ref_bs, my_bs["seq"])
        sgap, smargin = float(s_gap.min()), min(r["margin"] for r in tr)
        if sgap < GATE or smargin < GATE:
            return None, f"short memory: greedy gap {sgap:.2e}, beam margin {smargin:.2e}"
        out.update(short_greedy_seq=my_gs["seq"].numpy(), short_greedy_value=s_value.numpy(),
                   short_beam3_seq=ref_bs.numpy())
        msg.append(f"short memory: greedy gap {sgap:.2e} beam 3 margin {smargin:.2e}")
        return out, "; ".join(msg)

    chosen = None
    for draws in CANDIDATES:
        out, why = try_set(draws)
        line = f"members {draws[0]} roll step {draws[1]}: " + ("USED: " if out is not None else "rejected: ") + why
        print(line)
        report.append(line)
        if out is not None:
            chosen = draws
            break
    assert chosen is not None, "no candidate member set makes a fixture that can fail"
    out.update(members=np.array(chosen[0], dtype=np.int64), roll_step=np.array(chosen[1]), short_member=np.array(SHORT_MEMBER), short_tm=np.array(SHORT_TM),
               max_length=np.array(MAXLEN))

    # ---- sampling rules on m (ensemble.py:412-449) ----
    planes = torch.from_numpy(sample_planes())
    m = torch.stack([torch.log_softmax(planes[n], -1) for n in range(SAMPLE_MEMBERS)]).mean(dim=0)
    real = torch.distributions.Categorical
    captured = []

    class Recording(real):
        def __init__(self, probs=None, logits=None, validate_args=None):
            captured.append(logits.detach().clone())
            super().__init__(probs=probs, logits=logits, validate_args=validate_args)

    torch.distributions.Categorical = Recording
    r = runner()
    nm, nt = len(SAMPLE_METHODS), len(SAMPLE_TEMPS)
    dist = np.zeros((nm, nt, SAMPLE_ROWS, V), dtype=np.float32)
    word = np.zeros((nm, nt, SAMPLE_ROWS), dtype=np.int64)
    value = np.zeros((nm, nt, SAMPLE_ROWS), dtype=np.float32)
    try:
        for mi, method in enumerate(SAMPLE_METHODS):
            for ti, temp in enumerate(SAMPLE_TEMPS):
                for row in range(SAMPLE_ROWS):   # one row at a time: the gumbel branch gathers [N, 1] (B = 1 only)
                    captured.clear()
                    res = r.sample_next_word_with_logprob(m[row:row + 1].clone(), method, temp)
                    if method == "gumbel":
                        d = m[row:row + 1]      # argmax(m + Gumbel) draws from softmax(m)
                    else:
                        assert len(captured) == 1
                        d = captured[0]
                    mine_d, mine_v = E.sample_distribution(m[row:row + 1], method, temp)
                    assert torch.equal(torch.isinf(mine_d), torch.isinf(d)) and \
                        float((mine_d - d)[~torch.isinf(d)].abs().max()) < 1e-6, (method, temp, row)
                    w = int(res["word"][0])
                    dist[mi, ti, row] = d[0].numpy()
                    word[mi, ti, row] = w
                    value[mi, ti, row] = float(res["probs"].reshape(-1)[0])
                    assert abs(float(mine_v[0, w]) - value[mi, ti, row]) < 1e-6
                    if method == "top0.9":     # the cut must not sit within f32 rounding of p (cumulative mass: ~1e-6)
                        q = torch.softmax(m[row].double() / temp, 0).sort(descending=True).values.cumsum(0)
                        assert float((q - 0.9).abs().min()) > 1e-5, (temp, row)
                    if method == "top5":       # nor the 5th and 6th value within rounding of each other
                        t6 = m[row].topk(6).values
                        assert float(t6[4] - t6[5]) > GATE
    finally:
        torch.distributions.Categorical = real
    out.update(sample_methods=np.array(SAMPLE_METHODS), sample_temps=np.array(SAMPLE_TEMPS),
               sample_recipe=np.array([SAMPLE_MEMBERS, SAMPLE_ROWS, SAMPLE_SEED]), sample_dist=dist, sample_word=word,
               sample_value=value)

    path = os.path.join(HERE, "g16_ensemble.npz")
    # a fixed archive: sorted keys, no timestamps (np.savez writes the zip entries with a constant date)
    np.savez_compressed(path, **{k: out[k] for k in sorted(out)})
    size = os.path.getsize(path)
    assert size <= 1000000, size
    print(f"wrote {path}: {size} bytes")


if __name__ == "__main__":
    main()
