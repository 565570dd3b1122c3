"""Generate g18_kd.npz by running the REFERENCE's token-level distillation losses unmodified on the CPU:
``SupKdLoss(LabelSmoothingLoss(0.1), TokenLevelKdLoss(temp), sup_weight)`` of captioning/losses/kd_loss.py and
captioning/losses/loss.py, value and ``d loss / d logit`` (autograd).

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_kd.py

Inputs: (N, T, V) = (3, 5, 257), ``tgt_len`` = [5, 3, 1], student and teacher logits ``randn * 2.5`` drawn in float32 and
handed to the reference as float64 (its length mask stays float32), smoothing 0.1.  Cases: temp in {0.5, 1, 2} x
sup_weight in {0, 0.5, 1}.  The fixture holds data only: the inputs once, and per case ``loss/<temp>/<w>`` (float64) and
``dlogit/<temp>/<w>`` (rounded to float32: 6e-8 relative, the tests compare to 1e-6).  The archive is written with fixed
member dates and order, so that it regenerates byte for byte.
"""
import io
import os
import sys
import zipfile

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

N, T, V = 3, 5, 257
TGT_LEN = [5, 3, 1]
TEMPS = [0.5, 1.0, 2.0]
WEIGHTS = [0.0, 0.5, 1.0]
SMOOTHING = 0.1


def write_npz(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            a = np.asarray(a)
            np.lib.format.write_array(buf, np.ascontiguousarray(a) if a.ndim else a, allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    from make_golden import _install_stubs
    _install_stubs()
    from captioning.losses.kd_loss import SupKdLoss, TokenLevelKdLoss     # reference
    from captioning.losses.loss import LabelSmoothingLoss                 # reference
    import _kd_ref as K

    g = torch.Generator().manual_seed(18)
    logit = torch.randn(N, T, V, generator=g) * 2.5
    tchr = torch.randn(N, T, V, generator=g) * 2.5
    tgt = torch.randint(0, V, (N, T), generator=g)
    tgt_len = torch.tensor(TGT_LEN)
    out = {"logit": logit.numpy(), "tchr_logit": tchr.numpy(), "tgt": tgt.numpy(), "tgt_len": tgt_len.numpy(),
           "temps": np.array(TEMPS), "weights": np.array(WEIGHTS), "smoothing": np.array(SMOOTHING)}
    worst = 0.0
    for temp in TEMPS:
        for w in WEIGHTS:
            fn = SupKdLoss(LabelSmoothingLoss(SMOOTHING), TokenLevelKdLoss(temp), w)
            z = logit.double().requires_grad_(True)
            loss = fn({"logit": z, "tchr_logit": tchr.double(), "tgt": tgt, "tgt_len": tgt_len})
            loss.backward()
            out[f"loss/{temp:g}/{w:g}"] = np.array(float(loss), dtype=np.float64)
            out[f"dlogit/{temp:g}/{w:g}"] = z.grad.numpy().astype(np.float32)
            # the restatement against the reference, here as well
            want = K.kd_loss(logit, tchr, tgt, tgt_len, SMOOTHING, temp, w)[0]
            dwant = K.kd_dlogit(logit, tchr, tgt, tgt_len, SMOOTHING, temp, w)
            dv = abs(float(want) - float(loss)) / abs(float(loss))
            dg = float((dwant - z.grad).abs().max()) / float(z.grad.abs().max())
            worst = max(worst, dv, dg)
            print(f"temp {temp:g} w {w:g}: loss {float(loss):.9f}, restatement off by {dv:.2e} (value) {dg:.2e} (gradient)")
    assert worst < 1e-6, worst
    path = os.path.join(HERE, "g18_kd.npz")
    write_npz(path, out)
    print(f"wrote g18_kd.npz ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
