"""Generate g28_cnn_small.npz: the REFERENCE's Cnn6Encoder / Cnn10Encoder (captioning/models/cnn_encoder.py:114-327) and its
captioners over them, run on the CPU in float64.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_cnn_small.py

Recipe of make_golden.py: the reference is imported from its checkout at generation time only, behind inert ``sys.modules``
stubs; the stand-in MelSpectrogram returns a preset log-mel, so every case starts at the log-mel
(``procedural.synthetic_logmel``, which the tests re-draw: it is not stored).  Weights are ``_cnn_small_ref.fixture_state``:
the procedural draw with one BN channel in five NEGATIVE.

Stored, for both encoders (cases of ``_cnn_small_ref.CASES``):
  keys / shapes   the reference's ``state_dict()`` key list and shapes
  (a) B = 3, 32 kHz, T = 60 / 33 / 16 frames padded to 60: attn_emb, fc_emb, attn_emb_len, the four block outputs
  (b) B = 2, 16 kHz, T = 60: attn_emb, fc_emb, attn_emb_len
  (c) B = 2 ten-second clips, ragged wav_len: attn_emb, fc_emb, attn_emb_len
  (d) CrnnEncoder + RnnEncoder + TransformerDecoder + TransformerModel on case (a): greedy and beam-3 ``seq``, max_length 8,
      vocabulary 64.
A block output is kept as ``_cnn_small_ref.block_digest``: every 16th channel in full and every channel's sum and absolute sum
(the four full maps of two encoders exceed the size limit of a committed file).

Case (d) is only kept for a seed at which the decisions are not close: along the greedy path the top-1 / top-2 logit gap is
>= 1e-3 at every step (ten times the 1e-4 logit bar of the f32-grade tiers), and in the beam search every gap between
neighbours among the kept candidates and to the first cut (the reference's own ``topk`` calls, observed) is >= 1e-3; the
float32 run of the reference must return the same ids.  The next seed is tried otherwise.  The smallest gaps go to
REPORT_cnn_small.txt, whose section from REPORT_MARK on (a GPU run's figures) is kept.
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

REPORT_MARK = "==== measured on the GPU"
GAP = 1e-3


def main():
    import make_golden as MG
    MG._install_stubs()
    torch.set_grad_enabled(False)
    import captioning.models.cnn_encoder as ref_cnn     # reference
    from captioning.utils import train_util
    from audiocaption_amd import config as C
    from audiocaption_amd import procedural as P
    import _cnn_small_ref as R

    fixture, report = {}, []
    classes = {"cnn6": ref_cnn.Cnn6Encoder, "cnn10": ref_cnn.Cnn10Encoder}
    configs = {"cnn6": C.cnn6rnn_trm_config, "cnn10": C.cnn10rnn_trm_config}

    def run_encoder(enc, case):
        sr, T, frames = R.CASES[case]
        lms = R.logmel(case).double()
        MG._PRESET["lms"] = lms
        L = R.hop(sr) * (T - 1)
        return lms, enc({"wav": torch.zeros(len(frames), L, dtype=torch.float64), "wav_len": R.wav_lens(case), "specaug": False})

    for kind, cls in classes.items():
        state = P.to_torch(R.fixture_state(kind))
        for case, (sr, T, frames) in R.CASES.items():
            enc = cls(sample_rate=sr)
            if case == "a":
                sd = enc.state_dict()
                fixture[f"{kind}/keys"] = np.array(list(sd.keys()))
                fixture[f"{kind}/shapes"] = np.array([",".join(str(n) for n in v.shape) for v in sd.values()])
            enc.load_state_dict(state, strict=True)
            enc = enc.double().eval()
            lms, out = run_encoder(enc, case)
            lens = out["attn_emb_len"].tolist()
            assert lens == R.feat_len(R.wav_lens(case), sr), (lens, case)
            mine = R.forward_f64(kind, R.fixture_state(kind), lms, lens)
            for k in ("attn_emb", "fc_emb"):
                d = float((mine[k] - out[k]).abs().max())
                report.append(f"{kind} ({case}) {k}: restatement vs reference max|diff| {d:.3e} (|ref| max {float(out[k].abs().max()):.3e})")
                assert d < 1e-9, report[-1]
            fixture[f"{kind}/{case}/attn_emb"] = out["attn_emb"].float().numpy()
            fixture[f"{kind}/{case}/fc_emb"] = out["fc_emb"].numpy()
            fixture[f"{kind}/{case}/attn_emb_len"] = np.array(lens, dtype=np.int64)
            if case == "a":
                x = lms.transpose(1, 2).unsqueeze(1)
                x = enc.bn0(x.transpose(1, 3)).transpose(1, 3)
                for b in range(1, 5):
                    x = getattr(enc, f"conv_block{b}")(x, pool_size=(2, 2), pool_type="avg")
                    assert float((x - mine["blocks"][b - 1]).abs().max()) < 1e-9
                    for k, v in R.block_digest(x).items():
                        fixture[f"{kind}/a/block{b}_{k}"] = v

        # ---- (d): the captioner over case (a) --------------------------------------------------------------------------
        sr, T, frames = R.CASES["a"]
        inp = {"mode": "inference", "wav_len": R.wav_lens("a"), "specaug": False, "max_length": R.MAX_LENGTH}
        for seed in range(P.BASE_SEED, P.BASE_SEED + 50):
            model = train_util.init_model_from_config(configs[kind](R.VOCAB), print_fn=lambda s: None)
            model.load_state_dict(P.to_torch(R.fixture_model_state(kind, seed)), strict=True)
            model.eval()
            res = {}
            for dt in (torch.float64, torch.float32):
                model = model.to(dt)
                MG._PRESET["lms"] = R.logmel("a").to(dt)
                wav = torch.zeros(len(frames), R.hop(sr) * (T - 1), dtype=dt)
                greedy = model(dict(inp, wav=wav, sample_method="greedy"))
                gaps = []
                real_topk = torch.Tensor.topk

                def spy(self, k, *a, **kw):
                    vals = real_topk(self, min(k + 1, self.numel()), *a, **kw)[0]
                    gaps.append(float((vals[:-1] - vals[1:]).min()))
                    return real_topk(self, k, *a, **kw)

                torch.Tensor.topk = spy
                try:
                    beam = model(dict(inp, wav=wav, sample_method="beam", beam_size=R.BEAM))
                finally:
                    torch.Tensor.topk = real_topk
                top2 = greedy["logit"].double().topk(2, dim=-1)[0]
                live = torch.ones_like(top2[..., 0], dtype=torch.bool)
                for i, row in enumerate(greedy["seq"].tolist()):   # steps after the end token decide nothing
                    if model.end_idx in row:
                        live[i, row.index(model.end_idx) + 1:] = False
                res[dt] = (greedy["seq"], beam["seq"], float((top2[..., 0] - top2[..., 1])[live].min()), min(gaps))
            g64, b64, ggap, bgap = res[torch.float64]
            same = torch.equal(g64, res[torch.float32][0]) and torch.equal(b64, res[torch.float32][1])
            ok = same and ggap >= GAP and bgap >= GAP
            report.append(f"{kind} (d) seed {seed}: greedy top-1/top-2 logit gap {ggap:.3e}, beam candidate gap {bgap:.3e}, "
                          f"float32 ids {'equal' if same else 'DIFFER'}: " + ("USED" if ok else "rejected"))
            if ok:
                break
        assert ok, report[-1]
        fixture[f"{kind}/d/seed"] = np.array(seed)
        fixture[f"{kind}/d/greedy_seq"] = g64.numpy()
        fixture[f"{kind}/d/beam_seq"] = b64.numpy()
        fixture[f"{kind}/d/gaps"] = np.array([ggap, bgap])

    np.savez_compressed(R.FIXTURE, **{k: fixture[k] for k in sorted(fixture)})
    size = os.path.getsize(R.FIXTURE)
    assert size <= 1000000, size
    print("\n".join(report))
    print(f"wrote {R.FIXTURE}: {size} bytes")
    tail = REPORT_MARK + " (tests/test_gpu_conv5x5.py, tests/test_gpu_cnn_small.py): not measured\n"
    if os.path.exists(R.REPORT):
        with open(R.REPORT) as f:
            old = f.read()
        if REPORT_MARK in old:
            tail = old[old.index(REPORT_MARK):]
    with open(R.REPORT, "w") as f:
        f.write("g28_cnn_small.npz: written by make_golden_cnn_small.py (torch %s), %d bytes\n" % (torch.__version__, size))
        f.write("\n".join(report) + "\n")
        f.write(tail)


if __name__ == "__main__":
    main()
