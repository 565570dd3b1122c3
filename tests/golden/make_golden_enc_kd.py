"""Generate g24_enc_kd.npz by running the REFERENCE's encoder-distillation wrappers unmodified on the CPU:
``ContraEncoderKdWrapper``, ``MseEncoderKdWrapper`` and ``ContraMseEncoderKdWrapper`` of captioning/models/kd_wrapper.py over
a stub captioner that returns a given ``fc_emb`` - loss value and autograd gradients.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_enc_kd.py

Shapes: fc_emb width 24, teacher width 12, shared width 16; batches ``b5`` (5 clips) and ``b1`` (one clip: the contrastive
term is 0).  Kinds: ``contra``, ``mse``, ``mse_l2``, ``contra_mse``, ``contra_mse_l2`` (``_l2`` = ``l2_norm=True``).  Inputs
and head weights are drawn in float32 and handed to the reference as float64; ``logit_scale`` is the reference's initial
log(1 / 0.07) (as float32).  The fixture holds data only: the inputs and weights once, and per case ``<batch>/<kind>/loss`` and
``<batch>/<kind>/d/<tensor>`` for fc_emb, stdnt_proj.weight / .bias, tchr_proj.weight / .bias and logit_scale, all float64
(67 KB).  The archive is written with fixed member dates and order, so that it regenerates byte for byte.
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

import numpy as np
import torch
import torch.nn as nn

FC, TCHR, SHARED = 24, 12, 16
BATCHES = {"b5": 5, "b1": 1}
GRADS = ["fc_emb", "stdnt_proj.weight", "stdnt_proj.bias", "tchr_proj.weight", "tchr_proj.bias", "logit_scale"]


class _Encoder(nn.Module):
    fc_emb_size = FC


class _Captioner(nn.Module):
    """A captioner whose ``fc_emb`` is whatever the input dict carries."""

    def __init__(self):
        super().__init__()
        self.encoder = _Encoder()

    def forward(self, input_dict):
        return {"fc_emb": input_dict["feat"]}


def main():
    from make_golden import _install_stubs
    from make_golden_kd import write_npz
    _install_stubs()
    from captioning.models import kd_wrapper as R     # reference
    import _enc_kd_ref as E

    g = torch.Generator().manual_seed(24)
    weights = {"stdnt_proj.weight": torch.randn(SHARED, FC, generator=g) * 0.3, "stdnt_proj.bias": torch.randn(SHARED, generator=g) * 0.1,
               "tchr_proj.weight": torch.randn(SHARED, TCHR, generator=g) * 0.3, "tchr_proj.bias": torch.randn(SHARED, generator=g) * 0.1}
    out = {k: v.numpy() for k, v in weights.items()}
    # the reference's initial value: log(1 / 0.07) rounded to float32 (a float32 parameter, kd_wrapper.py:133)
    out["logit_scale"] = np.array(float(torch.ones([]) * np.log(1 / 0.07)))
    build = {"contra": lambda m: R.ContraEncoderKdWrapper(m, SHARED, TCHR),
             "mse": lambda m: R.MseEncoderKdWrapper(m, SHARED, TCHR),
             "mse_l2": lambda m: R.MseEncoderKdWrapper(m, SHARED, TCHR, l2_norm=True),
             "contra_mse": lambda m: R.ContraMseEncoderKdWrapper(m, SHARED, TCHR),
             "contra_mse_l2": lambda m: R.ContraMseEncoderKdWrapper(m, SHARED, TCHR, l2_norm=True)}
    worst = 0.0
    for bname, B in BATCHES.items():
        fc, tchr = torch.randn(B, FC, generator=g), torch.randn(B, TCHR, generator=g)
        out[f"{bname}/fc_emb"], out[f"{bname}/tchr_emb"] = fc.numpy(), tchr.numpy()
        for kind, make in build.items():
            w = make(_Captioner()).double()
            with torch.no_grad():
                for k, v in weights.items():
                    dict(w.named_parameters())[k].copy_(v.double())
            assert "contra" not in kind or float(w.logit_scale) == float(out["logit_scale"])
            assert sorted(k for k, _ in w.named_parameters()) == sorted(
                list(weights) + (["logit_scale"] if "contra" in kind else [])), kind
            feat = fc.double().requires_grad_(True)
            loss = w({"feat": feat, "tchr_output": {"embedding": tchr.double()}})["enc_kd_loss"]
            loss.backward()
            got = {"fc_emb": feat.grad}
            got.update({k: p.grad for k, p in w.named_parameters()})
            out[f"{bname}/{kind}/loss"] = np.array(float(loss), dtype=np.float64)
            want = E.full(fc, tchr, *(weights[k] for k in ("stdnt_proj.weight", "stdnt_proj.bias", "tchr_proj.weight",
                                                           "tchr_proj.bias")), float(out["logit_scale"]), E.KINDS[kind])
            dv = abs(float(want["loss"]) - float(loss)) / max(abs(float(loss)), 1e-300) if float(loss) != 0 else abs(float(want["loss"]))
            line = f"{bname} {kind}: loss {float(loss):.12f}, restatement off by {dv:.2e} (value)"
            worst = max(worst, dv)
            for k in GRADS:
                if k == "logit_scale" and "contra" not in kind:
                    continue
                gr = got[k].detach()
                out[f"{bname}/{kind}/d/{k}"] = gr.numpy().astype(np.float64)
                top = float(gr.abs().max())
                dg = float((want[k] - gr).abs().max()) / top if top > 0 else float(want[k].abs().max())
                worst = max(worst, dg)
                line += f" {dg:.1e}"
            print(line + "  (gradients: " + ", ".join(GRADS) + ")")
    assert worst < 1e-12, worst
    path = os.path.join(HERE, "g24_enc_kd.npz")
    write_npz(path, out)
    print(f"worst {worst:.2e}; wrote g24_enc_kd.npz ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
