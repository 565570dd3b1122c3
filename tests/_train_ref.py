"""Plain restatements of the training step's kernels for the tests (tests/test_gpu_train_kernels.py,
tests/test_gpu_train.py): explicit loops over the same index spaces the HIP kernels use, in whatever dtype the inputs
come in (the kernel tests pass float64).  No GPU needed; tests/test_train_ref_cpu.py pins them against the oracle."""
import math

import numpy as np
import torch

from oracle import train_path as OT


def gru_bidir_reference(gx, whh, bhh, lens):
    """One bidirectional GRU layer under pack_padded_sequence semantics, as an explicit recurrence (autograd-friendly).
    gx [B][T][2][3H] plays x W_ih^T + b_ih (identity input projection), whh [2][3H][H], bhh [2][3H], lens [B].
    Returns out [B][T][2H]: zeros beyond a clip's length; the reverse direction starts at the clip's own last frame."""
    B, T = gx.shape[:2]
    H = whh.shape[2]
    lens_t = torch.as_tensor(lens)
    outs = []
    for d in range(2):
        out = torch.zeros(B, T, H, dtype=gx.dtype)
        h = torch.zeros(B, H, dtype=gx.dtype)
        for t in (range(T - 1, -1, -1) if d else range(T)):
            gh = torch.nn.functional.linear(h, whh[d], bhh[d])
            r = torch.sigmoid(gx[:, t, d, :H] + gh[:, :H])
            z = torch.sigmoid(gx[:, t, d, H:2 * H] + gh[:, H:2 * H])
            n = torch.tanh(gx[:, t, d, 2 * H:] + r * gh[:, 2 * H:])
            hn = (1 - z) * n + z * h
            valid = (t < lens_t).unsqueeze(1)
            h = torch.where(valid, hn, h)
            out[:, t] = torch.where(valid, hn, torch.zeros_like(hn))
        outs.append(out)
    return torch.cat(outs, -1)


def attention_reference(q, k, v, qrow0, qlen, krow0, klen, nhead, pl, ptk, p, seed, seqs, kvalid=None, word=None,
                        pad_idx=0, causal=False):
    """ac_attn_seq_fwd's contract (include/audiocaption_hip.h) over the sequences ``seqs``: sequence s has qlen[s] query
    rows at qrow0[s] and klen[s] key / value rows at krow0[s]; key j is visible to query i iff j < kvalid[s] (if given),
    j <= i (if causal) and word[krow0[s] + j] != pad_idx (if word is given).  The dropout on P uses the element index
    ((s * nhead + h) * pl + i) * ptk + j of the kernel's P layout.  Returns (o, P): o like q, zero on rows of sequences
    outside ``seqs``; P {s: [nhead][qlen][klen]} the softmax before dropout."""
    hd = q.shape[1] // nhead
    o = torch.zeros_like(q)
    probs = {}
    rows = []
    for s in seqs:
        L, Tk, q0, k0 = int(qlen[s]), int(klen[s]), int(qrow0[s]), int(krow0[s])
        qs = q[q0:q0 + L].reshape(L, nhead, hd).transpose(0, 1)
        ks = k[k0:k0 + Tk].reshape(Tk, nhead, hd).transpose(0, 1)
        vs = v[k0:k0 + Tk].reshape(Tk, nhead, hd).transpose(0, 1)
        sc = qs @ ks.transpose(1, 2) / math.sqrt(hd)
        ok = torch.ones(L, Tk, dtype=torch.bool)
        if kvalid is not None:
            ok &= (torch.arange(Tk) < int(kvalid[s]))[None, :]
        if causal:
            ok &= torch.ones(L, Tk, dtype=torch.bool).tril()
        if word is not None:
            ok &= (torch.as_tensor(word[k0:k0 + Tk]) != pad_idx)[None, :]
        a = torch.softmax(sc.masked_fill(~ok[None], float("-inf")), -1)
        probs[s] = a
        m = OT.drop_mask(seed, s * nhead * pl * ptk, nhead * pl * ptk, p).reshape(nhead, pl, ptk)[:, :L, :Tk]
        ctx = (a * torch.from_numpy(m).to(a.dtype)) @ vs
        rows.append((q0, L, ctx.transpose(0, 1).reshape(L, nhead * hd)))
    for q0, L, c in rows:
        o = o.index_copy(0, torch.arange(q0, q0 + L), c)
    return o, probs


def attn_lds_floats(lmax, tkmax, bwd):
    """Floats of dynamic LDS ac_attn_seq_fwd / _bwd carve up (csrc/train.hip attn_lds_bytes): Q, K, V tiles of pitch 65
    and a (tkmax + 1)-pitched score block; the backward adds dO and a second score block."""
    f = (lmax + 2 * tkmax) * 65 + lmax * (tkmax + 1)
    if bwd:
        f += lmax * 65 + lmax * (tkmax + 1)
    return f


ATT_LDS_MAX_FLOATS = 160 * 1024 // 4


def largest_tkmax(lmax, bwd):
    """The largest tkmax whose carve-up fits ATT_LDS_MAX at this lmax."""
    t = 1
    while attn_lds_floats(lmax, t + 1, bwd) <= ATT_LDS_MAX_FLOATS:
        t += 1
    return t


def _bf16_rne(u32):
    """uint32 bit patterns of float32 -> the bf16 (as the upper half of a uint32) nearest, ties to even."""
    return ((u32 + np.uint32(0x7FFF) + ((u32 >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)) << np.uint32(16)


def pw_pack_reference(w, s_n, s_k, N, K):
    """ac_pw_gemm_pack_strided restated: W(n, k) = w.flat[n * s_n + k * s_k] split into bf16 hi + lo (RNE, lo = bf16 of
    the exact remainder) in MFMA fragment order [K/16 k-steps][N/32 tiles][hi, lo][64 lanes][8 bf16], lane = (n % 32) +
    32 * ((k % 16) >= 8), zero padded.  Returns the packed bytes (uint8)."""
    flat = np.asarray(w, dtype=np.float32).reshape(-1)
    NT, KS = (N + 31) // 32, (K + 31) // 32 * 2
    Wm = np.zeros((NT * 32, KS * 16), dtype=np.float32)
    n = np.arange(N)[:, None]
    k = np.arange(K)[None, :]
    Wm[:N, :K] = flat[n * s_n + k * s_k]
    u = Wm.view(np.uint32)
    hi = _bf16_rne(u)
    lo = _bf16_rne((Wm - hi.view(np.float32)).view(np.uint32))
    out = np.zeros((KS, NT, 2, 64, 8), dtype=np.uint16)
    for plane, x in ((0, hi), (1, lo)):
        b = (x >> np.uint32(16)).astype(np.uint16).reshape(NT, 32, KS, 2, 8)   # [tile][n % 32][k-step][k half][8]
        out[:, :, plane] = b.transpose(2, 0, 3, 1, 4).reshape(KS, NT, 64, 8)
    return out.reshape(-1).view(np.uint8)


# ---------------------------------------------------------------------------------------------------------
# the whole step at the benchmark's shapes (bench.py bench_train): one batch both the HIP engine and the CPU oracle
# start from, downstream of the frozen Cnn14 (the engine's ``_cnn_attn`` hook)
# ---------------------------------------------------------------------------------------------------------
STEP_CASES = {
    # name: (clips, Cnn14 frames Tq, caption tokens Tc, dropout seed)
    "bench_10s": (32, 31, 22, 104),
    "clotho_30s": (8, 94, 30, 207),
}


def step_batch(name):
    """(cnn_attn [B][Tq][2048], attn_len [B], cap [B][Tc] int64, cap_len [B], use_cap [Tc - 1], seed) of a step case.
    Captions as bench.py draws them (lengths 8 .. Tc, the first clip full, pads after <eos>); clip lengths ragged from
    a single frame up to Tq; scheduled sampling 0.85 with fixed draws that leave free-running passes early, in the middle
    and at the end of the caption (the re-runs of ``TrainEngine._launch_forward`` with seq0 > 0)."""
    B, Tq, Tc, seed = STEP_CASES[name]
    g = torch.Generator().manual_seed(seed)
    cnn_attn = torch.randn(B, Tq, 2048, generator=g).abs() * 0.5       # a post-ReLU mean: non-negative
    attn_len = torch.randint(Tq // 2, Tq + 1, (B,), generator=g)
    attn_len[0], attn_len[1], attn_len[2] = Tq, 1, Tq - 1
    cap = torch.randint(4, 4981, (B, Tc), generator=g)
    cap_len = torch.randint(8, Tc + 1, (B,), generator=g)
    cap_len[0] = Tc
    cap[:, 0] = 1
    for i, n in enumerate(cap_len.tolist()):
        cap[i, n - 1] = 2
        cap[i, n:] = 0
    T = Tc - 1
    use_cap = [1] * T
    for t in (2, T // 2, T // 2 + 1, T - 1):
        use_cap[t] = 0
    return cnn_attn, attn_len, cap, cap_len.numpy(), use_cap, seed


def free_running_gaps(logit, use_cap):
    """Top-1 minus top-2 logit at every step whose greedy token a later free-running pass reads (pass t reads the
    tokens of steps 0 .. t-1), over all clips: [clips][steps]."""
    last = max([t for t in range(len(use_cap)) if not use_cap[t] and t > 0], default=0)
    top2 = logit[:, :last].topk(2, -1).values
    return top2[..., 0] - top2[..., 1]
