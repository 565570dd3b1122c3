"""Generate g_group_beam.npz: group (diverse) beam search run by the REFERENCE on the CPU - its own
``CaptionModel.diverse_beam_search`` (captioning/models/base.py:363-471) over a ``TransformerDecoder``.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_group_beam.py

The import stubs are those of make_golden_attn_gru.py.  The reference's ``TransformerModel`` has no
``prepare_dbs_decoder_input`` (its ``sample_method="dbs"`` raises), so a generator-side subclass supplies it and
``dbs_process_step``, in the words of its ``prepare_beamsearch_decoder_input``: start token + the group's words so far, the
key-padding mask ``== pad_idx``, the clip's memory repeated ``bdash`` times.  The group's words are tracked in ``output_i``
(``seq_table`` is local to the reference's loop) from ``prev_words_beam`` / ``next_word``, which the loop leaves there.

Weights are the procedural draw ``procedural.decoder_state_diverse("beam", V)`` over the encoder memory of g4_greedy.npz; the
cases are ``_group_beam_ref.CASES``.  Per case the candidate clips of ``_group_beam_ref.CANDIDATE_CLIPS`` are tried in order,
one at a time; a clip is kept only if tests/_group_beam_ref.py returns the reference's ``seq`` for it (asserted: with and
without ``group_nbest``) and, on that run, every gap among the kept candidates and to the first cut is >= 1e-3 and the finished
scores that decide a group's top ``bdash`` differ by >= 2e-4 (test_gpu_decode_select.py's MARGIN and SCORE_GAP).  The first
``CLIPS_PER_CASE`` such clips are used, one of them of memory length 1.  The fixture stores the clips, the reference's ``seq``
in both shapes and the smallest gaps; the clips tried go to REPORT_group_beam.txt, whose section from REPORT_MARK on (a GPU
run's figures) is kept.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

REPORT_MARK = "==== gates and measured figures"


def main():
    from make_golden_attn_gru import _install_stubs
    _install_stubs()
    import captioning.models.transformer_decoder as ref_dec     # reference
    import captioning.models.transformer_model as ref_model
    from captioning.utils.model_util import repeat_tensor
    import _group_beam_ref as R

    class DbsTransformerModel(ref_model.TransformerModel):
        """What the reference would need to run its own diverse_beam_search over a TransformerDecoder."""

        def prepare_dbs_decoder_input(self, input_dict, output_i):
            i, divm, bdash = input_dict["sample_idx"], input_dict["divm"], input_dict["bdash"]
            words = output_i.setdefault("seq", [None] * input_dict["group_size"])[divm]
            start_word = torch.tensor([self.start_idx] * bdash).unsqueeze(1).long()
            word = start_word if words is None else torch.cat((start_word, words), dim=-1)
            return {"attn_emb": repeat_tensor(input_dict["attn_emb"][i], bdash),
                    "attn_emb_len": repeat_tensor(input_dict["attn_emb_len"][i], bdash),
                    "word": word, "cap_padding_mask": (word == self.pad_idx).to(input_dict["attn_emb"].device)}

        def dbs_process_step(self, output_i, output_t):
            divm = output_t["divm"]
            words, nxt = output_i["seq"][divm], output_i["next_word"][divm].unsqueeze(1)
            output_i["seq"][divm] = nxt if words is None else torch.cat([words[output_i["prev_words_beam"][divm]], nxt], dim=1)

    def ref_run(case, spec, group_nbest):
        _, G, bdash, beam, lam, temp, L, V = case
        dec = ref_dec.TransformerDecoder(emb_dim=256, vocab_size=V, fc_emb_dim=512, attn_emb_dim=512, dropout=0.2, nlayers=2)
        dec.load_state_dict({k[len("decoder."):]: v for k, v in R.state(V).items()}, strict=True)
        model = DbsTransformerModel(nn.Identity(), dec).eval()
        emb, lens = R.clips(spec)
        with torch.no_grad():
            out = model({"mode": "inference", "sample_method": "dbs", "attn_emb": emb, "attn_emb_len": lens,
                         "fc_emb": torch.zeros(len(spec), 512), "max_length": L, "temp": temp, "beam_size": beam,
                         "group_size": G, "diversity_lambda": lam, "group_nbest": group_nbest})
        return out["seq"]

    report, fixture = [], {}
    for case in R.CASES:
        cid, G, bdash = case[0], case[1], case[2]
        kept, worst = [], [float("inf"), float("inf")]
        for clip in R.CANDIDATE_CLIPS:
            if len(kept) == R.CLIPS_PER_CASE:
                break
            need_one = not any(ln == 1 for _, ln in kept) and len(kept) == R.CLIPS_PER_CASE - 1
            if need_one and clip[1] != 1:
                continue
            trace = []
            with torch.no_grad():
                mine = R.run_case(case, [clip], trace=trace)["seq"]
                mine_best = R.run_case(case, [clip], group_nbest=False)["seq"]
            ref, ref_best = ref_run(case, [clip], True), ref_run(case, [clip], False)
            assert torch.equal(mine, ref), ("restatement differs from the reference", cid, clip)
            assert torch.equal(mine_best, ref_best), ("restatement differs from the reference (group_nbest=False)", cid, clip)
            margin, gap = R.guards(trace, bdash)
            ok = margin >= R.MARGIN and gap >= R.SCORE_GAP
            line = f"{cid} clip {clip}: margin {margin:.3e} score gap {gap:.3e} " + ("USED" if ok else "rejected")
            print(line)
            report.append(line)
            if ok:
                kept.append(clip)
                worst = [min(worst[0], margin), min(worst[1], gap)]
        assert len(kept) == R.CLIPS_PER_CASE and any(ln == 1 for _, ln in kept), (cid, kept)
        # the batch as the tests run it: the reference loops over clips, so this is the per-clip results stacked
        ref, ref_best = ref_run(case, kept, True), ref_run(case, kept, False)
        with torch.no_grad():
            assert torch.equal(R.run_case(case, kept)["seq"], ref), cid
        assert ref.shape == (len(kept), case[3], case[6]) and ref_best.shape == (len(kept), G, case[6])
        fixture[f"{cid}/clips"] = np.array(kept, dtype=np.int32)
        fixture[f"{cid}/seq"] = ref.numpy()
        fixture[f"{cid}/seq_best"] = ref_best.numpy()
        fixture[f"{cid}/gaps"] = np.array(worst, dtype=np.float64)
    fixture["cases"] = np.array([c[0] for c in R.CASES])
    fixture["case_params"] = np.array([c[1:] for c in R.CASES], dtype=np.float64)

    path = R.FIXTURE
    np.savez_compressed(path, **{k: fixture[k] for k in sorted(fixture)})
    size = os.path.getsize(path)
    assert size <= 1000000, size
    print(f"wrote {path}: {size} bytes")
    rpath, kept_tail = os.path.join(HERE, "REPORT_group_beam.txt"), REPORT_MARK + " (tests/test_gpu_group_beam.py): not measured\n"
    if os.path.exists(rpath):
        with open(rpath) as f:
            old = f.read()
        if REPORT_MARK in old:
            kept_tail = old[old.index(REPORT_MARK):]
    with open(rpath, "w") as f:
        f.write("g_group_beam.npz: candidate clips tried by make_golden_group_beam.py (torch %s)\n" % torch.__version__)
        f.write("tests/_group_beam_ref.py returned the reference's seq for every clip listed, with and without group_nbest\n")
        f.write("\n".join(report) + "\n")
        f.write(kept_tail)


if __name__ == "__main__":
    main()
