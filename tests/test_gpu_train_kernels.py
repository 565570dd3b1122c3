"""GPU tests of the training step's kernels at the shapes, strides and flags the step really passes (bench.py's training
line: 32 clips x 10 s, 22-token captions, scheduled sampling 0.85, dropout on), each against a float64 restatement of
the same operation (tests/_train_ref.py), and the whole step at that configuration against the CPU oracle.

Tolerances: split-bf16 products (ac_pw_gemm_bf16x3_ex) carry 2^-16 relative operand error - 3e-5 of the largest output,
the bar of the other split-bf16 tests; exact-f32 kernels 1e-5 of the largest output (f32 rounding over reductions of at
most a few thousand terms); copies, integer kernels and single-rounding elementwise kernels must be bit-exact."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

import _train_ref as R
from oracle import train_path as OT
from test_gpu_train import _set_dropout, train_model  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SPLIT_BF16 = 3e-5
EXACT_F32 = 1e-5
NAN = float("nan")
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_KEEP = []   # P() only takes an address: temporaries such as ``x.cuda()`` are kept alive until the next test starts


@pytest.fixture(autouse=True)
def _drop_kept_tensors():
    _KEEP.clear()
    yield
    _KEEP.clear()


def P(t, offset_elems=0):
    if t is None:
        return None
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr() + offset_elems * t.element_size())


def rel(name, got, want, scale=None):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    sc = float(want.abs().max()) if scale is None else scale
    d = float((got - want).abs().max()) / (sc + 1e-30)
    print(f"[{name}] max|diff| / max|want| = {d:.3e} (max|want| {sc:.3e})")
    return d


def nan_like(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def i32(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int32)).to(DEV)


# =========================================================================================================
# 1. ac_pw_gemm_bf16x3_ex as the step calls it
# =========================================================================================================
def _pw_kernel(M, N, K):
    """Which kernel ac_pw_gemm_bf16x3_ex launches (csrc/pw_gemm.hip, no environment overrides, M < 16384)."""
    blocks = (M + 31) // 32 * (((N + 31) // 32 + 7) // 8)
    return "longk" if (K >= 512 and blocks <= 320) or (K >= 256 and blocks <= 200) else "tile32"


PW_CASES = [(M, N, K) for M in (7392, 3696) for N, K in ((768, 256), (256, 256), (1024, 256), (256, 1024), (512, 256))]


def test_pw_cases_reach_both_kernels():
    fwd = {_pw_kernel(M, N, K) for M, N, K in PW_CASES}
    dx = {_pw_kernel(M, K, N) for M, N, K in PW_CASES}
    assert fwd == dx == {"longk", "tile32"}


@pytest.mark.parametrize("M,N,K", PW_CASES)
def test_pw_gemm_ex_forward_and_input_gradient(lib, M, N, K):
    """Forward y = dropout(relu(x W^T + b)) with the mask index (row0 + m) * N + n, row0 > 0, on row-strided views
    (ldx > K, ldy > N); input gradient dx (+)= dy W through the transposed pack (s_n = 1, s_k = K), beta 0 and 1.
    Columns beyond the views must stay untouched."""
    print(f"forward on {_pw_kernel(M, N, K)}, input gradient on {_pw_kernel(M, K, N)}")
    g = torch.Generator().manual_seed(M + 7 * N + K)
    ldx, ldy = K + 12, N + 8
    x = torch.randn(M, ldx, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g) * 0.1
    wd = w.to(DEV)
    frag = torch.empty(lib.ac_pw_gemm_packed_bytes(N, K), dtype=torch.uint8, device=DEV)
    assert lib.ac_pw_gemm_pack_strided(P(wd), K, 1, P(frag), N, K, S()) == 0
    p, seed, row0 = 0.2, OT.op_seed(17, OT.OP_LAYER + 4), 4321
    y = nan_like(M + 1, ldy)             # beta = 0: the old contents are never read
    assert lib.ac_pw_gemm_bf16x3_ex(P(x.to(DEV)), ldx, P(frag), P(b.to(DEV)), P(y), ldy, M, N, K, 1, 0.0, None, 0, p, seed,
                                    None, row0, S()) == 0
    mask = torch.from_numpy(OT.drop_mask(seed, row0 * N, M * N, p)).view(M, N).double()
    want = torch.relu(x[:, :K].double() @ w.double().t() + b.double()) * mask
    yc = y.cpu()
    assert rel("x W^T + b, relu, dropout(row0)", yc[:M, :N], want) < SPLIT_BF16
    assert (yc[:M, :N][mask == 0] == 0).all()                     # dropped cells are exact zeros
    assert torch.isnan(yc[:M, N:]).all() and torch.isnan(yc[M]).all()
    # input gradient: W^T packed from the same row-major weights
    fragT = torch.empty(lib.ac_pw_gemm_packed_bytes(K, N), dtype=torch.uint8, device=DEV)
    assert lib.ac_pw_gemm_pack_strided(P(wd), 1, K, P(fragT), K, N, S()) == 0
    lddy, lddx = N + 4, K + 4
    dy = torch.randn(M, lddy, generator=g)
    dx0 = torch.randn(M, lddx, generator=g)
    dyd = dy.to(DEV)
    for beta in (0.0, 1.0):
        dx = dx0.to(DEV) if beta else nan_like(M, lddx)
        assert lib.ac_pw_gemm_bf16x3_ex(P(dyd), lddy, P(fragT), None, P(dx), lddx, M, K, N, 0, beta, None, 0, 0.0, 0, None,
                                        0, S()) == 0
        want = dy[:, :N].double() @ w.double() + beta * dx0[:, :K].double()
        dxc = dx.cpu()
        assert rel(f"dy W (beta {beta:g})", dxc[:, :K], want) < SPLIT_BF16
        if beta:
            assert torch.equal(dxc[:, K:], dx0[:, K:])
        else:
            assert torch.isnan(dxc[:, K:]).all()


def test_pw_pack_table_repacks_like_per_layer_packs(lib):
    """One ac_pw_gemm_pack_table launch over a device table of row-major and transposed records (N, K not multiples of
    32), after the weights changed in place, gives the bytes of per-layer ac_pw_gemm_pack_strided - and both are the
    fragment layout restated in tests/_train_ref.py (bf16 RNE hi + lo)."""
    g = torch.Generator().manual_seed(8)
    layers = [(100, 36, False), (100, 36, True), (260, 68, False), (44, 300, True), (52, 76, False), (76, 52, True)]
    recs, items = b"", []
    for N, K, tr in layers:
        w = (torch.randn(N, K, generator=g) * 0.3).to(DEV)
        n, k = (K, N) if tr else (N, K)
        s_n, s_k = (1, K) if tr else (K, 1)
        frag = torch.empty(lib.ac_pw_gemm_packed_bytes(n, k), dtype=torch.uint8, device=DEV)
        assert lib.ac_pw_gemm_pack_strided(P(w), s_n, s_k, P(frag), n, k, S()) == 0
        assert np.array_equal(frag.cpu().numpy(), R.pw_pack_reference(w.cpu().numpy(), s_n, s_k, n, k)), (N, K, tr)
        recs += struct.pack("<QQqqii", w.data_ptr(), frag.data_ptr(), s_n, s_k, n, k)
        items.append((w, frag, s_n, s_k, n, k))
    assert len(recs) == 40 * len(layers)
    table = torch.frombuffer(bytearray(recs), dtype=torch.uint8).to(DEV)
    for w, frag, *_ in items:
        w.mul_(-1.7).add_(0.25)              # the optimiser step moves the weights in place
        frag.fill_(0xAB)                     # every byte must be rewritten, padding included
    assert lib.ac_pw_gemm_pack_table(P(table), len(layers), S()) == 0
    for w, frag, s_n, s_k, n, k in items:
        fresh = torch.empty_like(frag)
        assert lib.ac_pw_gemm_pack_strided(P(w), s_n, s_k, P(fresh), n, k, S()) == 0
        assert torch.equal(frag, fresh), (n, k, s_n)
        assert np.array_equal(frag.cpu().numpy(), R.pw_pack_reference(w.cpu().numpy(), s_n, s_k, n, k))


# =========================================================================================================
# 2. attention forward / backward at training shapes
# =========================================================================================================
def _attn_case(lib, qlens, klens=None, kvalid=None, pads=(), seq0=0, nseq=None, pl=None, ptk=None, lmax=None, tkmax=None,
               p=0.2, gen=0):
    """Self-attention (klens None: causal, keys = the queries' rows of one qkv buffer of row pitch 3D, pad tokens at
    ``pads`` = (sequence, position)) or cross-attention (keys of sequence s at rows s * Tk of a kv buffer of pitch 2D,
    kvalid[s] valid).  Launches sequences seq0 .. seq0 + nseq of len(qlens); everything outside must stay NaN."""
    nh, hd, D = 4, 64, 256
    g = torch.Generator().manual_seed(100 + gen)
    Sn = len(qlens)
    nseq = Sn - seq0 if nseq is None else nseq
    run = range(seq0, seq0 + nseq)
    cross = klens is not None
    qrow0 = np.concatenate([[0], np.cumsum(qlens)[:-1]]).astype(np.int64)
    R_ = int(sum(qlens))
    if cross:
        krow0 = np.concatenate([[0], np.cumsum(klens)[:-1]]).astype(np.int64)
        Rk = int(sum(klens))
        word = None
    else:
        klens, krow0, Rk = qlens, qrow0, R_
        word = torch.randint(3, 4981, (R_,), generator=g).int()
        for s, j in pads:
            word[qrow0[s] + j] = 0
    lmax = max(qlens[s] for s in run) if lmax is None else lmax
    tkmax = max(klens[s] for s in run) if tkmax is None else tkmax
    pl = lmax + 3 if pl is None else pl
    ptk = tkmax + 5 if ptk is None else ptk
    seed = OT.op_seed(11, OT.OP_LAYER + (2 if cross else 0))
    if cross:
        qb = torch.randn(R_, D, generator=g)
        kvb = torch.randn(Rk, 2 * D, generator=g)
        q, k, v = qb, kvb[:, :D], kvb[:, D:]
        qd, kvd = qb.to(DEV), kvb.to(DEV)
        qp, ldq, kp, vp, ldk = P(qd), D, P(kvd), P(kvd, D), 2 * D
    else:
        qkv = torch.randn(R_, 3 * D, generator=g)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        qkvd = qkv.to(DEV)
        qp, ldq, kp, vp, ldk = P(qkvd), 3 * D, P(qkvd, D), P(qkvd, 2 * D), 3 * D
    # float64 reference
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    o_ref, probs = R.attention_reference(q64, k64, v64, qrow0, qlens, krow0, klens, nh, pl, ptk, p, seed, run,
                                         kvalid=kvalid, word=None if cross else word.tolist(), causal=not cross)
    dout = torch.randn(R_, D, generator=g)
    o_ref.backward(dout.double())
    # HIP forward
    o = nan_like(R_, D)
    Pb = nan_like(Sn * nh * pl * ptk)
    d_qrow0, d_qlen, d_krow0, d_klen = i32(qrow0), i32(qlens), i32(krow0), i32(klens)
    d_kvalid = i32(kvalid) if cross else None
    d_word = word.to(DEV) if word is not None else None
    assert lib.ac_attn_seq_fwd(qp, ldq, kp, ldk, vp, ldk, P(o), D, P(Pb), pl, ptk, P(d_qrow0), P(d_qlen), P(d_krow0),
                               P(d_klen), P(d_kvalid), P(d_word), 0, 0 if cross else 1, seq0, nseq, nh, hd, lmax, tkmax,
                               p, seed, None, S()) == 0
    qrows = torch.cat([torch.arange(qrow0[s], qrow0[s] + qlens[s]) for s in run])
    krows = torch.cat([torch.arange(krow0[s], krow0[s] + klens[s]) for s in run])
    qout = torch.ones(R_, dtype=torch.bool)
    qout[qrows] = False
    kout = torch.ones(Rk, dtype=torch.bool)
    kout[krows] = False
    oc = o.cpu()
    worst = {"o": rel("attention out", oc[qrows], o_ref.detach()[qrows])}
    assert worst["o"] < EXACT_F32
    assert torch.isnan(oc[qout]).all()
    Pc = Pb.cpu().view(Sn, nh, pl, ptk)
    for s in range(Sn):
        if s in run:
            L, Tk = qlens[s], klens[s]
            assert rel(f"P of sequence {s}", Pc[s, :, :L, :Tk], probs[s].detach(), scale=1.0) < EXACT_F32
            assert torch.isnan(Pc[s, :, L:]).all() and torch.isnan(Pc[s, :, :, Tk:]).all()
        else:
            assert torch.isnan(Pc[s]).all()
    # HIP backward (same launch)
    dq = nan_like(R_, D)
    if cross:
        dkv = nan_like(Rk, 2 * D)
        dkp, dvp, lddk, dk_of, dv_of = P(dkv), P(dkv, D), 2 * D, (lambda: dkv.cpu()[:, :D]), (lambda: dkv.cpu()[:, D:])
    else:
        dkv = nan_like(R_, 2 * D)
        dkp, dvp, lddk, dk_of, dv_of = P(dkv), P(dkv, D), 2 * D, (lambda: dkv.cpu()[:, :D]), (lambda: dkv.cpu()[:, D:])
    assert lib.ac_attn_seq_bwd(qp, ldq, kp, ldk, vp, ldk, P(Pb), pl, ptk, P(dout.to(DEV)), D, P(dq), D, dkp, lddk, dvp,
                               lddk, P(d_qrow0), P(d_qlen), P(d_krow0), P(d_klen), seq0, nseq, nh, hd, lmax, tkmax, p, seed,
                               None, S()) == 0
    dqc, dkc, dvc = dq.cpu(), dk_of(), dv_of()
    worst["dq"] = rel("attention dq", dqc[qrows], q64.grad[qrows])
    worst["dk"] = rel("attention dk", dkc[krows], k64.grad[krows])
    worst["dv"] = rel("attention dv", dvc[krows], v64.grad[krows])
    assert max(worst.values()) < EXACT_F32, worst
    assert torch.isnan(dqc[qout]).all() and torch.isnan(dkc[kout]).all() and torch.isnan(dvc[kout]).all()
    return worst


SELF_LENS = [1, 13, 21, 29, 21, 5]
SELF_PADS = [(1, 4), (2, 20), (3, 10), (3, 28), (4, 1)]


def test_self_attention_training_shapes(lib):
    """Causal self-attention over prefixes of 1 .. 29 tokens with pad keys, P strides beyond lmax / tkmax, dropout on P."""
    _attn_case(lib, SELF_LENS, pads=SELF_PADS)


def test_self_attention_free_running_relaunch(lib):
    """A launch over a subset (seq0 = 2, three sequences), as the free-running re-runs do: the other sequences' rows of o,
    dq, dk, dv and their P blocks stay untouched."""
    _attn_case(lib, SELF_LENS, pads=SELF_PADS, seq0=2, nseq=3, gen=1)


@pytest.mark.parametrize("Tk", [31, 94])
def test_cross_attention_training_shapes(lib, Tk):
    """Cross-attention onto Tk audio frames (94: the softmax takes a second lane pass), kvalid from 1 to Tk."""
    kvalid = [1, 2, Tk // 2, Tk - 1, Tk, 31, 64 if Tk > 64 else 7, 65 if Tk > 65 else 30][:8]
    qlens = [21, 1, 13, 21, 29, 5, 21, 21]
    _attn_case(lib, qlens, klens=[Tk] * 8, kvalid=kvalid, gen=2 + Tk)
    _attn_case(lib, qlens, klens=[Tk] * 8, kvalid=kvalid, seq0=3, nseq=4, gen=3 + Tk)


def test_attention_lds_limit(lib):
    """The largest (lmax, tkmax) whose LDS carve-up fits ATT_LDS_MAX runs correctly (keys in five lane passes); one key
    more is refused with AC_ERR_ARG before anything is launched (outputs untouched)."""
    L = 21
    for bwd in (False, True):
        tk = R.largest_tkmax(L, bwd)
        print(f"lmax {L}: largest tkmax {tk} ({'backward' if bwd else 'forward'})")
        if bwd:
            _attn_case(lib, [L, 7], klens=[tk, tk], kvalid=[tk, 100], gen=9)
        else:   # the forward alone at its own (larger) limit
            nh, D = 4, 256
            q = torch.randn(L, D, device=DEV)
            kv = torch.randn(tk, 2 * D, device=DEV)
            o = nan_like(L, D)
            Pb = nan_like(nh * L * tk)
            z, ln, kl = i32([0]), i32([L]), i32([tk])
            assert lib.ac_attn_seq_fwd(P(q), D, P(kv), 2 * D, P(kv, D), 2 * D, P(o), D, P(Pb), L, tk, P(z), P(ln), P(z), P(kl),
                                       None, None, 0, 0, 0, 1, nh, 64, L, tk, 0.0, 0, None, S()) == 0
            qh = q.double().cpu().view(L, nh, 64).transpose(0, 1)
            kh = kv[:, :D].double().cpu().view(tk, nh, 64).transpose(0, 1)
            vh = kv[:, D:].double().cpu().view(tk, nh, 64).transpose(0, 1)
            want = (torch.softmax(qh @ kh.transpose(1, 2) / 8.0, -1) @ vh).transpose(0, 1).reshape(L, D)
            assert rel("attention out at the forward's LDS limit", o, want) < EXACT_F32
        # one key beyond: refused, nothing written
        nh, D = 4, 256
        q = torch.randn(L, D, device=DEV)
        kv = torch.randn(tk + 1, 2 * D, device=DEV)
        o = nan_like(L, D)
        Pb = nan_like(nh * L * (tk + 1))
        z, ln, kl = i32([0]), i32([L]), i32([tk + 1])
        if bwd:
            dq, dkv = nan_like(L, D), nan_like(tk + 1, 2 * D)
            Pb.zero_()
            assert lib.ac_attn_seq_bwd(P(q), D, P(kv), 2 * D, P(kv, D), 2 * D, P(Pb), L, tk + 1, P(o.zero_()), D, P(dq), D,
                                       P(dkv), 2 * D, P(dkv, D), 2 * D, P(z), P(ln), P(z), P(kl), 0, 1, nh, 64, L, tk + 1,
                                       0.0, 0, None, S()) == -1
            torch.cuda.synchronize()
            assert torch.isnan(dq).all() and torch.isnan(dkv).all()
        else:
            assert lib.ac_attn_seq_fwd(P(q), D, P(kv), 2 * D, P(kv, D), 2 * D, P(o), D, P(Pb), L, tk + 1, P(z), P(ln), P(z),
                                       P(kl), None, None, 0, 0, 0, 1, nh, 64, L, tk + 1, 0.0, 0, None, S()) == -1
            torch.cuda.synchronize()
            assert torch.isnan(o).all() and torch.isnan(Pb).all()


# =========================================================================================================
# 3. dropout + residual + LayerNorm on the decoder-memory path
# =========================================================================================================
@pytest.mark.parametrize("R_", [7392, 7405])
def test_dropadd_layernorm_memory_path(lib, R_):
    """Forward with res = NULL over xmod-row replicas (row r reads x[r % xmod]) launched from row0 > 0 (rows below stay
    untouched) and then from 0; backward with accumulate = 1 onto a non-zero dres, and with dres = NULL and the ReLU gate
    relu_src[r % relu_mod] (train.py's memory backward); dgamma / dbeta accumulate onto non-zero values from
    ceil(R / 32) blocks.  7405 is not a multiple of the 32 rows per block."""
    g = torch.Generator().manual_seed(R_)
    D, xmod, p, eps = 256, 352, 0.2, 1e-5
    row0 = 3 * xmod
    seed = OT.op_seed(5, OT.OP_MEM)
    x = torch.relu(torch.randn(xmod, D, generator=g))          # the projected memory after its ReLU (exact zeros)
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    pre, y = nan_like(R_, D), nan_like(R_, D)
    assert lib.ac_dropadd_ln_fwd(P(xd), None, P(gd), P(bd), P(pre), P(y), row0, R_ - row0, xmod, D, p, seed, None, eps,
                                 S()) == 0
    torch.cuda.synchronize()
    assert torch.isnan(pre[:row0]).all() and torch.isnan(y[:row0]).all()
    assert lib.ac_dropadd_ln_fwd(P(xd), None, P(gd), P(bd), P(pre), P(y), 0, row0, xmod, D, p, seed, None, eps, S()) == 0
    mask = torch.from_numpy(OT.drop_mask(seed, 0, R_ * D, p)).view(R_, D)
    rep = torch.arange(R_) % xmod
    assert torch.equal(pre.cpu(), x[rep] * mask)                  # one f32 multiply per cell
    pre64 = (x[rep].double() * mask.double()).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y_ref = torch.nn.functional.layer_norm(pre64, (D,), g64, b64, eps)
    assert rel("ln forward (replicas, row0)", y, y_ref) < EXACT_F32
    dy = torch.randn(R_, D, generator=g)
    y_ref.backward(dy.double())
    dpre, dgam, dbet = pre64.grad, g64.grad, b64.grad
    # (a) dres accumulated, dx = dpre * mask
    dres0 = torch.randn(R_, D, generator=g)
    dg0, db0 = torch.randn(D, generator=g), torch.randn(D, generator=g)
    dx, dres, dg, db = nan_like(R_, D), dres0.to(DEV), dg0.to(DEV), db0.to(DEV)
    assert lib.ac_dropadd_ln_bwd(P(dy.to(DEV)), P(pre), P(gd), P(dx), P(dres), 1, None, 0, P(dg), P(db), R_, D, p, seed,
                                 None, eps, S()) == 0
    assert rel("ln dres (accumulate)", dres, dres0.double() + dpre) < EXACT_F32
    assert rel("ln dx (mask)", dx, dpre * mask.double()) < EXACT_F32
    assert rel("ln dgamma (+=)", dg, dg0.double() + dgam) < EXACT_F32
    assert rel("ln dbeta (+=)", db, db0.double() + dbet) < EXACT_F32
    # (b) dres = NULL, dx gated by the ReLU of the replicated source
    dx2, dg2, db2 = nan_like(R_, D), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    assert lib.ac_dropadd_ln_bwd(P(dy.to(DEV)), P(pre), P(gd), P(dx2), None, 0, P(xd), xmod, P(dg2), P(db2), R_, D, p, seed,
                                 None, eps, S()) == 0
    gate = (x[rep] > 0).double()
    assert rel("ln dx (mask, relu gate)", dx2, dpre * mask.double() * gate) < EXACT_F32
    assert (dx2.cpu()[gate == 0] == 0).all()
    assert rel("ln dgamma", dg2, dgam) < EXACT_F32 and rel("ln dbeta", db2, dbet) < EXACT_F32


# =========================================================================================================
# 4. embedding and row plumbing of the decoder passes
# =========================================================================================================
def _layout(N=32, T=21, Tm=31):
    from audiocaption_amd.train import TrainEngine
    return TrainEngine._layout(N, T, Tm, False, DEV)


def test_embedding_segments_and_backward_atomics(lib):
    """ac_embed_fwd over three row0 segments of the 32 x 21-pass row space, both dropouts on (seed from the device word),
    then one ac_embed_bwd over all rows onto a non-zero table; many rows share one token (atomics on the same row)."""
    lay = _layout()
    Rr, d, V = lay["R"], 256, 4981
    g = torch.Generator().manual_seed(4)
    word = torch.randint(4, 40, (Rr,), generator=g, dtype=torch.int32)
    word[::5] = 7
    emb = torch.randn(V, d, generator=g) * 0.1
    pe = torch.randn(40, d, generator=g) * 0.1
    pa = pb = 0.2
    base = torch.tensor([77], dtype=torch.int64, device=DEV)
    sa, sb = OT.op_seed(77, OT.OP_EMB_A), OT.op_seed(77, OT.OP_EMB_B)
    ed, wdv, posd = emb.to(DEV), word.to(DEV), lay["pos"]
    x = nan_like(Rr, d)
    for r0, r1 in ((0, 1000), (1000, 4000), (4000, Rr)):
        assert lib.ac_embed_fwd(P(ed), P(pe.to(DEV)), P(wdv), P(posd), P(x), r0, r1 - r0, d, pa, OT.OP_EMB_A, pb,
                                OT.OP_EMB_B, P(base), S()) == 0
    ma = torch.from_numpy(OT.drop_mask(sa, 0, Rr * d, pa)).view(Rr, d).double()
    mb = torch.from_numpy(OT.drop_mask(sb, 0, Rr * d, pb)).view(Rr, d).double()
    pos = posd.cpu().long()
    want = (emb.double()[word.long()] * ma * math.sqrt(d) + pe.double()[pos]) * mb
    assert rel("embedding forward", x, want) < EXACT_F32
    dx = torch.randn(Rr, d, generator=g)
    demb0 = torch.randn(V, d, generator=g)
    demb = demb0.to(DEV)
    assert lib.ac_embed_bwd(P(dx.to(DEV)), P(wdv), P(demb), Rr, d, pa, OT.OP_EMB_A, pb, OT.OP_EMB_B, P(base), S()) == 0
    want = demb0.double().index_add(0, word.long(), dx.double() * mb * math.sqrt(d) * ma)
    assert int((word == 7).sum()) > 1000
    assert rel("embedding backward", demb, want) < EXACT_F32


def test_prefix_gather_scatter_replicas_mask(lib):
    lay = _layout()
    N, T, Tc, D, Rr = 32, 21, 22, 256, lay["R"]
    g = torch.Generator().manual_seed(5)
    cap = torch.randint(0, 4981, (N, Tc), generator=g)
    seq = torch.randint(0, 4981, (N, T), generator=g, dtype=torch.int32)
    use_cap = torch.randint(0, 2, (T,), generator=g, dtype=torch.int32)
    use_cap[3], use_cap[4] = 0, 1
    capd, seqd = cap.to(DEV), seq.to(DEV)
    for ucap in (torch.ones(T, dtype=torch.int32), use_cap):
        word = torch.full((Rr,), -7, dtype=torch.int32, device=DEV)
        for t, (L, off) in enumerate(lay["passes"]):
            assert lib.ac_build_prefix(P(capd), Tc, P(seqd), T, P(ucap.to(DEV)), t, 1, P(word), off, N, L, S()) == 0
        want = np.full(Rr, -7, dtype=np.int32)
        for t, (L, off) in enumerate(lay["passes"]):
            for n in range(N):
                row = cap[n, :L].numpy() if ucap[t] else np.concatenate([[1], seq[n, :L - 1].numpy()])
                want[off + n * L:off + (n + 1) * L] = row
        assert np.array_equal(word.cpu().numpy(), want)
    # one pass alone touches only its rows
    L, off = lay["passes"][5]
    word = torch.full((Rr,), -7, dtype=torch.int32, device=DEV)
    assert lib.ac_build_prefix(P(capd), Tc, P(seqd), T, P(use_cap.to(DEV)), 5, 1, P(word), off, N, L, S()) == 0
    wc = word.cpu()
    assert (wc[:off] == -7).all() and (wc[off + N * L:] == -7).all() and (wc[off:off + N * L] != -7).all()
    # the classifier rows: gather / scatter-add through cls_rows (no duplicates), bit-exact
    cls = lay["cls_rows"]
    assert cls.unique().numel() == N * T
    src = torch.randn(Rr, D, generator=g)
    dst = nan_like(N * T, D)
    assert lib.ac_gather_rows(P(src.to(DEV)), P(cls), P(dst), N * T, D, S()) == 0
    assert torch.equal(dst.cpu(), src[cls.cpu().long()])
    add = torch.randn(N * T, D, generator=g)
    base = torch.randn(Rr, D, generator=g)
    out = base.to(DEV)
    assert lib.ac_scatter_add_rows(P(add.to(DEV)), P(cls), P(out), N * T, D, S()) == 0
    want = base.clone()
    want[cls.cpu().long()] += add
    assert torch.equal(out.cpu(), want)
    # the audio memory's gradient summed over 21 pass replicas
    n, reps = 352 * D, 21
    xr = torch.randn(reps * n, generator=g)
    out = nan_like(n)
    assert lib.ac_sum_replicas(P(xr.to(DEV)), P(out), n, reps, S()) == 0
    assert rel("sum of 21 replicas", out, xr.double().view(reps, n).sum(0)) < EXACT_F32
    # FFN hidden backward: g = h > 0 ? g * scale : 0 over R x 1024, one f32 multiply
    m = Rr * 1024
    h = torch.randn(m, generator=g)
    h[::5] = 0.0
    gg = torch.randn(m, generator=g)
    gd = gg.to(DEV)
    assert lib.ac_mask_pos_scale(P(gd), P(h.to(DEV)), m, 1.25, S()) == 0
    assert torch.equal(gd.cpu(), torch.where(h > 0, gg * 1.25, torch.zeros_like(gg)))


@pytest.mark.parametrize("M,N,ld", [(20000, 300, 308), (7392, 768, 768), (7392, 1024, 1028)])
def test_colsum(lib, M, N, ld):
    """Bias gradients: out[n] += sum_m x[m * ld + n]; 20000 rows exceed the 64 x 256 rows the grid's 64 row slices cover
    in one sweep; accumulated onto a non-zero out."""
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, ld, generator=g)
    out0 = torch.randn(N, generator=g) * 10
    out = out0.to(DEV)
    assert lib.ac_colsum(P(x.to(DEV)), ld, P(out), M, N, S()) == 0
    assert rel("colsum", out, out0.double() + x[:, :N].double().sum(0)) < EXACT_F32


# =========================================================================================================
# 5. label-smoothing loss
# =========================================================================================================
@pytest.mark.parametrize("V", [4981, 4368, 257])
def test_label_smoothing_loss_rows_and_gradient(lib, V):
    """Per-row loss, mean and dlogit against float64 log_softmax at T = 21, tgt_len 0 / T / beyond T; the count given
    on the host (inv_count, gscale > 0) and taken on the device (<= 0) with the upstream gradient in gscale_dev."""
    N, T, sm = 8, 21, 0.1
    g = torch.Generator().manual_seed(V)
    tgt_len = [0, T, T + 4, 1, 13, T, 40, 7]
    cap = torch.randint(0, V, (N, T + 1), generator=g)
    logit = torch.randn(N, T, V, generator=g) * 3
    lp = torch.log_softmax(logit.double(), -1)
    tgt = cap[:, 1:]
    q = torch.full_like(lp, sm / (V - 1)).scatter_(-1, tgt.unsqueeze(-1), 1.0 - sm)
    valid = (torch.arange(T)[None, :] < torch.tensor(tgt_len)[:, None]).double()
    row_ref = -(q * lp).sum(-1) * valid
    count = float(sum(min(n, T) for n in tgt_len))
    grad_ref = (lp.exp() - q) * valid[..., None]
    ld, capd, lend = logit.to(DEV), cap.to(DEV), i32(tgt_len)
    for mode in ("host", "device"):
        row_loss, loss, dlogit = nan_like(N * T), nan_like(1), nan_like(N, T, V)
        if mode == "host":
            inv, gsc, gdev, up = 1.0 / count, 0.7 / count, None, 0.7
        else:
            inv, gsc, gdev, up = 0.0, -1.0, torch.tensor([2.5], device=DEV), 2.5
        assert lib.ac_label_smoothing_loss(P(ld), P(capd, 1), T + 1, P(lend), N, T, V, sm, inv, P(row_loss), P(loss),
                                           P(dlogit), gsc, P(gdev), S()) == 0
        rl = row_loss.cpu().view(N, T)
        assert rel(f"row loss ({mode})", rl, row_ref) < EXACT_F32
        assert (rl[valid == 0] == 0).all()
        assert abs(float(loss) - float(row_ref.sum()) / count) < EXACT_F32 * float(row_ref.sum()) / count
        dl = dlogit.cpu()
        assert rel(f"dlogit ({mode})", dl, grad_ref * up / count) < EXACT_F32
        assert (dl[valid == 0] == 0).all()


# =========================================================================================================
# 6. optimiser kernels
# =========================================================================================================
NORM_TICKET = 4 + 1024      # csrc/train.hip AC_NORM_TICKET: the last-workgroup counter inside norm_state


def test_grad_sumsq_ticket_and_accumulation(lib):
    """Repeated calls into one norm_state - n above the 1024-workgroup cap (grid-stride) and n below one workgroup -
    must each find their last workgroup (the ticket is reset) and add to [0]."""
    g = torch.Generator().manual_seed(6)
    big = torch.randn(1024 * 256 * 3 + 77, generator=g)
    small = torch.randn(200, generator=g)
    st = torch.zeros(1032, device=DEV)
    acc = 0.0
    for t in (big, small, big, small, small):
        assert lib.ac_grad_sumsq(P(t.to(DEV)), t.numel(), P(st), S()) == 0
        acc += float((t.double() ** 2).sum())
        sc = st.cpu()
        assert int(sc.view(torch.int32)[NORM_TICKET]) == 0
        assert abs(float(sc[0]) - acc) < EXACT_F32 * acc, (float(sc[0]), acc)
        assert (sc[1:4] == 0).all()


@pytest.mark.parametrize("case", ["clip", "no_clip_needed", "max_norm_0", "nan", "inf"])
@pytest.mark.parametrize("grad_div", [1.0, 2.0])
def test_clip_coefficient_and_scale(lib, case, grad_div):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(50000, generator=g) * (1e-4 if case == "no_clip_needed" else 0.3)
    if case == "nan":
        x[123] = NAN
    if case == "inf":
        x[7] = 3e38                       # finite, but its square overflows
    max_norm = 0.0 if case == "max_norm_0" else 1.0
    st = torch.zeros(1032, device=DEV)
    xd = x.to(DEV)
    assert lib.ac_grad_sumsq(P(xd), x.numel(), P(st), S()) == 0
    assert lib.ac_clip_coef(P(st), max_norm, grad_div, S()) == 0
    sc = st.cpu()
    if case in ("nan", "inf"):
        assert float(sc[2]) == 0.0 and float(sc[3]) == 1.0
        return
    norm = math.sqrt(float((x.double() ** 2).sum())) / grad_div
    coef = (min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0) / grad_div
    assert abs(float(sc[1]) - norm) < EXACT_F32 * norm
    assert abs(float(sc[2]) - coef) < EXACT_F32 * coef and float(sc[3]) == 0.0
    assert lib.ac_scale_by_coef(P(xd), x.numel(), P(st), S()) == 0
    assert torch.equal(xd.cpu(), x * sc[2])


def test_adam_device_step_count_across_a_skipped_step(lib):
    """ac_adam_step with step_dev and ac_adam_commit over three optimiser steps, the second with a NaN gradient: it must
    leave parameters and moments bit-identical and not advance the count, so the third step's bias correction is t = 2."""
    g = torch.Generator().manual_seed(8)
    n, lr, b1, b2, eps, wd = 5003, 1e-3, 0.9, 0.999, 1e-8, 1e-2
    # the kernel takes the hyperparameters as f32: 1 - float32(0.999) is 1.3e-5 away from 1e-3, so the float64 restatement
    # uses the f32 values it is given (the reference's own Adam is pinned by test_gpu_train)
    rb1, rb2 = float(np.float32(b1)), float(np.float32(b2))
    p0 = torch.randn(n, generator=g) * 0.05
    pd, md, vd = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    rp, rm, rv, t = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), 0
    for k in range(3):
        gr = torch.randn(n, generator=g) * 0.05
        if k == 1:
            gr[17] = NAN
        st = torch.zeros(1032, device=DEV)
        grd = gr.to(DEV)
        assert lib.ac_grad_sumsq(P(grd), n, P(st), S()) == 0
        assert lib.ac_clip_coef(P(st), 1.0, 1.0, S()) == 0
        before = (pd.clone(), md.clone(), vd.clone())
        assert lib.ac_adam_step(P(pd), P(grd), P(md), P(vd), n, P(st), lr, b1, b2, eps, wd, 99, P(step), S()) == 0
        assert lib.ac_adam_commit(P(step), P(st), S()) == 0
        if k == 1:
            assert all(torch.equal(a, b) for a, b in zip(before, (pd, md, vd)))
            assert int(step) == 1
            continue
        t += 1
        assert int(step) == t
        norm = float(gr.double().norm())
        gg = gr.double() * min(1.0, 1.0 / (norm + 1e-6)) + float(np.float32(wd)) * rp
        rm = rb1 * rm + (1 - rb1) * gg
        rv = rb2 * rv + (1 - rb2) * gg * gg
        old = rp
        rp = rp - lr / (1 - rb1 ** t) * rm / (rv.sqrt() / math.sqrt(1 - rb2 ** t) + eps)
        assert rel(f"adam m (step {t})", md, rm) < EXACT_F32 and rel(f"adam v (step {t})", vd, rv) < EXACT_F32
        # the update itself: p is O(0.05), its rounding (ulp 3.7e-9) is < 1e-5 of an update of O(lr)
        assert rel(f"adam update (step {t})", pd.cpu().double() - before[0].cpu().double(), rp - old) < 3e-5
        rp = pd.cpu().double()             # continue from the device's f32 parameters


def test_swa_update_and_first_copy(lib):
    """n_averaged = 0 copies the parameters whatever the average held (AveragedModel's first update is a copy);
    n_averaged = 3 is avg + (p - avg) / 4."""
    g = torch.Generator().manual_seed(9)
    n = 70001
    p1, p2 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    junk = torch.randn(n, generator=g) * 1e8
    junk[::1000] = NAN
    avg = junk.to(DEV)
    assert lib.ac_swa_update(P(avg), P(p1.to(DEV)), n, 0, S()) == 0
    assert torch.equal(avg.cpu(), p1)
    assert lib.ac_swa_update(P(avg), P(p2.to(DEV)), n, 3, S()) == 0
    assert rel("swa (n_averaged 3)", avg, p1.double() + (p2.double() - p1.double()) / 4) < EXACT_F32


# =========================================================================================================
# 7. GRU training kernels at the step's shapes
# =========================================================================================================
@pytest.mark.parametrize("T", [31, 94])
def test_gru_training_kernels_at_step_shapes(lib, T):
    """ac_gru_layer_train, ac_gru_layer_split (the engine's forward) and ac_gru_layer_bwd at B = 32 clips of T frames
    (10 s / 30 s), ragged lengths from 1 to T, against the float64 recurrence.  Bars as test_gpu_train's T = 9 case:
    1e-5 on outputs, 2e-5 on gradients (f32 recurrences)."""
    g = torch.Generator().manual_seed(10 + T)
    B, H = 32, 256
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0], lens[1], lens[2] = T, 1, T - 1
    gx = torch.randn(B, T, 2, 3 * H, generator=g) * 0.5
    whh = torch.randn(2, 3 * H, H, generator=g) * 0.06
    bhh = torch.randn(2, 3 * H, generator=g) * 0.1
    dout = torch.randn(B, T, 2 * H, generator=g)
    gxr, whr, bhr = (t.double().requires_grad_(True) for t in (gx, whh, bhh))
    out_ref = R.gru_bidir_reference(gxr, whr, bhr, lens.tolist())
    out_ref.backward(dout.double())
    whh_d, bhh_d, gx_d, dout_d = whh.to(DEV), bhh.to(DEV), gx.to(DEV), dout.to(DEV)
    lens_d = lens.to(device=DEV, dtype=torch.int32)
    whhT = torch.empty(2, H, 3 * H, device=DEV)
    assert lib.ac_gru_pack_whh(P(whh_d), P(whhT), H, S()) == 0
    out, save = torch.empty(B, T, 2 * H, device=DEV), torch.empty(B, T, 2, 4 * H, device=DEV)
    assert lib.ac_gru_layer_train(P(gx_d), P(whhT), P(bhh_d), P(lens_d), P(out), P(save), B, T, H, S()) == 0
    worst = {"out": rel("gru out", out, out_ref)}
    out_s, save_s = nan_like(B, T, 2 * H), nan_like(B, T, 2, 4 * H)
    xch = torch.zeros((lib.ac_gru_split_workspace_bytes(B) + 7) // 8, device=DEV, dtype=torch.int64)
    assert lib.ac_gru_layer_split(P(gx_d), P(whh_d), P(bhh_d), P(lens_d), P(out_s), P(save_s), P(xch), B, T, H, S()) == 0
    assert int(xch.view(torch.int32)[0]) == 0
    worst["split out"] = rel("split gru out", out_s, out_ref)
    assert max(worst.values()) < 1e-5, worst
    for b, n in enumerate(lens.tolist()):
        assert float((save_s[b, :n] - save[b, :n]).abs().max()) < 1e-5
        assert torch.isnan(save_s[b, n:]).all()
    for tag, o_, s_ in (("", out, save), ("split ", out_s, save_s)):
        dgx, dgh, hprev = (torch.empty(B, T, 2, w, device=DEV) for w in (3 * H, 3 * H, H))
        assert lib.ac_gru_layer_bwd(P(dout_d), P(o_), P(s_), P(whh_d), P(lens_d), P(dgx), P(dgh), P(hprev), B, T, H,
                                    S()) == 0
        dwhh = torch.einsum("btdn,btdk->dnk", dgh.cpu().double(), hprev.cpu().double())
        d = {f"{tag}dgx": rel(f"{tag}gru dgx", dgx, gxr.grad), f"{tag}dW_hh": rel(f"{tag}gru dW_hh", dwhh, whr.grad),
             f"{tag}db_hh": rel(f"{tag}gru db_hh", dgh.cpu().double().sum((0, 1)), bhr.grad)}
        assert max(d.values()) < 2e-5, d


# =========================================================================================================
# 8. the whole step at the benchmark configuration against the CPU oracle
# =========================================================================================================
# ReLU kink width for the oracle comparison (oracle/train_path.py _relu_at_kinks): the step's forward products run on
# split-bf16 operands, whose pre-activation error is larger than the exact-f32 KINK; the test measures the audio
# memory's pre-activation error and requires it to stay below half this width.
STEP_KINK = 1e-4


@pytest.mark.parametrize("name", list(R.STEP_CASES))
def test_training_step_at_benchmark_shapes_vs_oracle(train_model, state4981, name):
    """TrainEngine.forward / backward on the default GEMM route at the benchmark's shapes (32 clips x 10 s, 22 tokens)
    and at 8 clips x 30 s (Tm = 94) with 30 tokens: p_dec 0.2, p_rnn 0.5, scheduled sampling with free-running passes.
    Both sides start from the same Cnn14 output (the engine's ``_cnn_attn`` hook) so that the oracle, and with it the
    near-tie guard of tests/test_train_ref_cpu.py, is reproducible on the CPU."""
    from audiocaption_amd.loss import _launch
    from audiocaption_amd.train import TrainEngine
    model = train_model
    _set_dropout(model, 0.2, 0.5, False)
    cnn_attn, lens, cap, cap_len, use_cap, seed = R.step_batch(name)
    B, Tq = cnn_attn.shape[:2]
    wav_len = [320 * (32 * int(n) - 1) for n in lens]          # cnn14_feat_len gives back `lens`
    eng = TrainEngine(model)
    out = eng.forward({"mode": "train", "wav": torch.zeros(B, 320 * 32 * Tq, device=DEV), "wav_len": wav_len,
                       "specaug": False, "cap": cap.to(DEV), "cap_len": cap_len, "ss_ratio": 0.85, "_use_cap": use_cap,
                       "dropout_seed": seed, "_cnn_attn": cnn_attn.to(DEV)})
    assert eng._pw, "the split-bf16 weight-product route (AUDIOCAPTION_TRAIN_GEMM=pw) was not taken"
    sv = eng._saved
    assert sv["free_ts"], "no free-running pass"
    ws_, R_ = sv["ws"], sv["lay"]["R"]
    rows_m = sv["N"] * sv["Tq"]
    gates = {"mem": ws_.tensor("mem_a")[:rows_m * 256].view(rows_m, 256).cpu(),
             "ffn": [ws_.tensor(f"hdn{l}")[:R_ * sv["F"]].view(R_, sv["F"]).cpu() for l in range(model.decoder.nlayers)]}
    o = OT.train_step_grads(state4981, cnn_attn, lens, cap, cap_len, use_cap, base_seed=seed, p_dec=0.2, p_rnn=0.5,
                            relu_gates=gates, kink=STEP_KINK)
    gap = float(R.free_running_gaps(o["logit"], use_cap).min())
    assert gap >= 1e-3, f"near-tie {gap:.1e} at a token a free-running pass reads: choose another seed"
    # the forward's error on a pre-activation (audio memory projection, split-bf16) against the kink width
    pre = torch.nn.functional.linear(o["attn_emb"].reshape(rows_m, -1), state4981["decoder.attn_proj.0.weight"],
                                     state4981["decoder.attn_proj.0.bias"])
    on = pre > STEP_KINK
    err = float((gates["mem"][on] - pre[on]).abs().max())
    print(f"{name}: memory pre-activation error {err:.2e} (kink width {STEP_KINK:.0e}), smallest free-running gap {gap:.2e}")
    assert err < STEP_KINK / 2
    worst = {"logit": rel("logit", out["logit"], o["logit"])}
    assert worst["logit"] < 5e-5
    assert torch.equal(out["seq"].cpu(), o["seq"])
    logit = out["logit"]
    tgt_len = torch.as_tensor(cap_len - 1)
    count = float(tgt_len.sum())
    dlogit = torch.empty_like(logit)
    loss, _ = _launch(logit, cap[:, 1:].to(DEV), tgt_len.to(device=DEV, dtype=torch.int32), 0.1, 1.0 / count, dlogit,
                      1.0 / count, None)
    worst["loss"] = abs(float(loss) - float(o["loss"])) / float(o["loss"])
    assert worst["loss"] < 2e-5
    eng.backward(dlogit)
    assert any(k[3] for k in eng._pw) and any(not k[3] for k in eng._pw)   # x W^T and dy W both on the pw route
    bad = []
    worst["grad"] = 0.0
    for key, view in zip(eng.flat.names, eng.flat.grad_views):
        d = rel(key, view, o["grads"][key])
        worst["grad"] = max(worst["grad"], d)
        if not d < 2e-4:
            bad.append((key, d))
    print(f"{name}: worst relative differences vs the oracle {worst}")
    assert not bad, bad
