"""CPU checks of the float64 restatements in tests/_train_ref.py that tests/test_gpu_train_kernels.py holds the HIP
training kernels to, and the near-tie guard of its whole-step cases."""
import numpy as np
import torch

import _train_ref as R
from oracle import cpu_path as O
from oracle import train_path as OT


def test_attention_reference_is_the_oracles_attention():
    """attention_reference over the kernel's row space equals oracle._mha_train (identity projections) for one pass of
    N sequences: self-attention with causal and pad masks, cross-attention with ragged valid keys, dropout on P indexed
    from a first sequence seq0 > 0."""
    g = torch.Generator().manual_seed(0)
    N, L, Tk, nh, d, p, seq0 = 3, 5, 70, 4, 256, 0.2, 2
    pl, ptk = L + 2, Tk + 3
    eye = torch.eye(d, dtype=torch.float64)
    w, b = torch.cat([eye, eye, eye]), torch.zeros(3 * d, dtype=torch.float64)
    zero = torch.zeros(d, dtype=torch.float64)
    x = torch.randn(N, L, d, generator=g, dtype=torch.float64)
    mem = torch.randn(N, Tk, d, generator=g, dtype=torch.float64)
    word = torch.randint(3, 50, (N, L), generator=g)
    word[1, 2] = word[2, 4] = 0
    kvalid = [Tk, 1, 65]
    seed = OT.op_seed(9, 30)
    S = seq0 + N
    qrow0 = [0] * seq0 + [n * L for n in range(N)]
    qlen = [L] * S
    # self-attention
    neg = float("-inf")
    causal = torch.zeros(L, L, dtype=torch.float64).masked_fill(torch.ones(L, L, dtype=torch.bool).triu(1), neg)
    mask = causal[None, None] + torch.zeros(N, 1, 1, L, dtype=torch.float64).masked_fill((word == 0)[:, None, None], neg)
    pm = torch.from_numpy(OT.drop_mask(seed, seq0 * nh * pl * L, N * nh * pl * L, p)).view(N, nh, pl, L)[:, :, :L]
    want = OT._mha_train(x, x, x, w, b, eye, zero, nh, mask, pm.double())
    xr = x.reshape(N * L, d)
    got, _ = R.attention_reference(xr, xr, xr, qrow0, qlen, qrow0, qlen, nh, pl, L, p, seed, range(seq0, S),
                                   word=word.reshape(-1).tolist(), causal=True)
    assert float((got - want.reshape(N * L, d)).abs().max()) < 1e-12
    # cross-attention
    mask = torch.zeros(N, 1, 1, Tk, dtype=torch.float64)
    for n in range(N):
        mask[n, ..., kvalid[n]:] = neg
    pm = torch.from_numpy(OT.drop_mask(seed, seq0 * nh * pl * ptk, N * nh * pl * ptk, p)).view(N, nh, pl, ptk)[:, :, :L, :Tk]
    want = OT._mha_train(x, mem, mem, w, b, eye, zero, nh, mask, pm.double())
    mr = mem.reshape(N * Tk, d)
    krow0 = [0] * seq0 + [n * Tk for n in range(N)]
    got, _ = R.attention_reference(xr, mr, mr, qrow0, qlen, krow0, [Tk] * S, nh, pl, ptk, p, seed, range(seq0, S),
                                   kvalid=[0] * seq0 + kvalid)
    assert float((got - want.reshape(N * L, d)).abs().max()) < 1e-12


def test_gru_reference_is_the_oracles_recurrence():
    """gru_bidir_reference (identity input projection) equals oracle.cpu_path._gru_direction per direction."""
    g = torch.Generator().manual_seed(1)
    B, T, H = 4, 7, 8
    lens = [7, 1, 4, 6]
    gx = torch.randn(B, T, 2, 3 * H, generator=g)
    whh = torch.randn(2, 3 * H, H, generator=g) * 0.3
    bhh = torch.randn(2, 3 * H, generator=g) * 0.1
    got = R.gru_bidir_reference(gx, whh, bhh, lens)
    eye, zero = torch.eye(3 * H), torch.zeros(3 * H)
    for d in range(2):
        want = O._gru_direction(gx[:, :, d], torch.tensor(lens), eye, whh[d], zero, bhh[d], bool(d))
        assert torch.allclose(got[..., d * H:(d + 1) * H], want, atol=1e-6, rtol=0)


def test_pw_pack_reference_layout():
    """pw_pack_reference read back through the kernel's own item loop (csrc/pw_gemm.hip pw_pack_items: item t = k-step
    * NT32 + tile, lane -> column tile * 32 + lane % 32, k = 16 k-step + 8 (lane / 32) + e) gives hi + lo = W to within
    bf16 of the remainder, zeros in the padding, and a transposed stride pair packs W^T."""
    g = torch.Generator().manual_seed(2)
    N, K = 44, 70
    w = torch.randn(N, K, generator=g).numpy()
    for s_n, s_k, n_, k_, W in ((K, 1, N, K, w), (1, K, K, N, w.T)):
        b = R.pw_pack_reference(w, s_n, s_k, n_, k_).view(np.uint16)
        NT, KS = (n_ + 31) // 32, (k_ + 31) // 32 * 2
        assert b.size == KS * NT * 2 * 64 * 8
        back = np.zeros((NT * 32, KS * 16))
        for t in range(KS * NT):
            nt, kk = t % NT, t // NT
            for lane in range(64):
                n, k0 = nt * 32 + lane % 32, kk * 16 + 8 * (lane // 32)
                for pl in range(2):
                    v = b[((t * 2 + pl) * 64 + lane) * 8:((t * 2 + pl) * 64 + lane) * 8 + 8].astype(np.uint32) << 16
                    back[n, k0:k0 + 8] += v.view(np.float32)
        assert np.abs(back[:n_, :k_] - W).max() <= np.abs(W).max() * 2.0 ** -16
        assert not back[n_:].any() and not back[:, k_:].any()


def test_attention_lds_edge():
    for lmax in (1, 21, 29):
        for bwd in (False, True):
            t = R.largest_tkmax(lmax, bwd)
            assert R.attn_lds_floats(lmax, t, bwd) <= R.ATT_LDS_MAX_FLOATS < R.attn_lds_floats(lmax, t + 1, bwd)
            assert t >= 94      # the longest (30 s) audio memory fits


def test_whole_step_cases_have_no_free_running_near_ties(state4981):
    """The whole-step GPU cases compare greedy tokens with the oracle's: a free-running pass reads earlier greedy tokens,
    so a top-1 / top-2 gap below the forward's error (logits: 5e-5) would let both sides legitimately diverge.  The
    oracle's gaps at every step a free-running pass reads must be at least 1e-3 (the seeds of STEP_CASES were chosen so)."""
    for name in R.STEP_CASES:
        cnn_attn, lens, cap, cap_len, use_cap, seed = R.step_batch(name)
        assert any(not u for u in use_cap[1:])
        with torch.no_grad():
            emb = OT.gru_train_forward(state4981, cnn_attn, lens, seed, 0.5)
            out = OT.train_forward(state4981, emb, lens, cap, use_cap, seed, 0.2)
        gap = float(R.free_running_gaps(out["logit"], use_cap).min())
        print(f"{name}: smallest free-running top-1/top-2 gap {gap:.2e}")
        assert gap >= 1e-3, name
