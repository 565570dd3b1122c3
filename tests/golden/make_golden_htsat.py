"""Generate g_htsat.npz by running the REFERENCE's ``captioning.models.transformer_encoder.Htsat`` unmodified on the CPU,
in eval mode and in FLOAT64 (``model.double()``, float64 input: torch's bicubic then forms its source positions in double
too), so the float64 restatement tests/_htsat_ref.py is held to 1e-9 of every stored array's maximum.

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_htsat.py

Weights: ``procedural.htsat_state`` (constructor defaults, depths 2-2-6-2).  Inputs: ``procedural.synthetic_logmel(2, 1001)``
(case ``t1001``: the stretch of a 10 s batch) and ``synthetic_logmel(1, 1024)`` (case ``t1024``: no resampling), fed through
the reference's own ``bn0``, ``reshape_wav2img`` and ``forward_features`` - the torchaudio front end is absent here and the
log-mel is pinned elsewhere.  Per case the fixture holds ``attn_emb``, ``fc_emb``, ``layer_0 .. layer_3``, two corners of the
folded image (the top-left one, and one across the boundary between the first two time chunks at the last columns), and
300 sampled token entries after the patch embedding and after every stage (``tok<k>_idx`` (300, 3) = clip, token, channel;
``tok<k>_val``).  ``state_keys`` / ``state_shapes``: the reference's ``state_dict()`` (the stubbed torchaudio transform
registers no buffers, so ``melspec_extractor.*`` is not among them).  Data only; fixed member dates and order.
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

CASES = {"t1001": (2, 1001), "t1024": (1, 1024)}
N_SAMPLED = 300


def main():
    from make_golden import _install_stubs
    from make_golden_kd import write_npz
    _install_stubs()
    from captioning.models.transformer_encoder import Htsat     # reference
    from audiocaption_amd import procedural as P
    import _htsat_ref as R

    model = Htsat().eval()
    own = model.state_dict()
    state = P.to_torch(P.htsat_state())
    missing = [k for k in own if k not in state and not k.endswith(("relative_position_index", "attn_mask"))]
    assert not missing and all(k in own for k in state), (missing, [k for k in state if k not in own])
    model.load_state_dict(dict(own, **state), strict=True)
    model = model.double()
    out = {"state_keys": np.array(list(own)), "state_shapes": np.array([",".join(map(str, v.shape)) for v in own.values()])}
    worst = 0.0
    for case, (B, T) in CASES.items():
        lms = torch.from_numpy(P.synthetic_logmel(B, T)).transpose(1, 2).contiguous()     # (B, T, 64)
        taps = []
        hooks = [model.patch_embed.register_forward_hook(lambda m, i, o: taps.append(o))]
        hooks += [layer.register_forward_hook(lambda m, i, o: taps.append(o[0])) for layer in model.layers]
        with torch.no_grad():
            x = lms.double().unsqueeze(1).transpose(1, 3)
            x = model.bn0(x).transpose(1, 3)
            img = model.reshape_wav2img(x)
            got = model.forward_features(img)
        for h in hooks:
            h.remove()
        want = R.forward({k: v for k, v in state.items()}, R.bn0(state, lms))
        rng = np.random.default_rng([7, B, T])
        arrays = {k: got[k] for k in ("attn_emb", "fc_emb", "layer_0", "layer_1", "layer_2", "layer_3")}
        arrays["corner"] = img[:, 0, :8, :8]
        arrays["corner_fold"] = img[:, 0, 62:66, 252:256]
        mine = {k: want[k] for k in ("attn_emb", "fc_emb", "layer_0", "layer_1", "layer_2", "layer_3")}
        folded = R.fold(R.bicubic_time(R.bn0(state, lms)))
        mine["corner"], mine["corner_fold"] = folded[:, :8, :8], folded[:, 62:66, 252:256]
        for k, tok in enumerate(taps):
            idx = np.stack([rng.integers(0, n, N_SAMPLED) for n in tok.shape], 1).astype(np.int32)
            out[f"{case}/tok{k}_idx"] = idx
            arrays[f"tok{k}_val"] = tok[idx[:, 0], idx[:, 1], idx[:, 2]]
            mine[f"tok{k}_val"] = want["tokens"][k][idx[:, 0], idx[:, 1], idx[:, 2]]
        for k, v in arrays.items():
            out[f"{case}/{k}"] = v.numpy().astype(np.float64)
            dv = float((mine[k] - v).abs().max() / v.abs().max())
            worst = max(worst, dv)
            print(f"{case} {k}: max |value| {float(v.abs().max()):.4f}, restatement off by {dv:.2e}")
    assert worst < 1e-9, worst
    path = os.path.join(HERE, "g_htsat.npz")
    write_npz(path, out)
    print(f"worst {worst:.2e}; wrote g_htsat.npz ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
