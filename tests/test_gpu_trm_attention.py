"""GPU tests of ac_attn_self_bwd_tiled, the row-tiled attention backward of the Transformer encoder's self-attention
(N clips x T' + 1 rows, non-causal, key padding from attn_len + 1), against the float64 restatement of
tests/_train_ref.py at the exact-f32 bar, at sampled L from one row to the forward's limit of 126 - including
L = 92 .. 126, which the one-workgroup ac_attn_seq_bwd refuses - and on ragged sequences shorter than the launch bounds."""
import ctypes

import pytest
import torch

import _train_ref as R
from oracle import train_path as OT

pytestmark = pytest.mark.gpu

EXACT_F32 = 1e-5
D, NH, HD = 256, 4, 64
DEV = "cuda"
_KEEP = []


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


@pytest.fixture(autouse=True)
def _drop_kept_tensors():
    _KEEP.clear()
    yield
    _KEEP.clear()


def S():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t, offset_elems=0):
    if t is None:
        return None
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr() + 4 * offset_elems)


def i32(v):
    return torch.as_tensor(v, dtype=torch.int32).to(DEV)


def nan_like(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def same(a, b):
    """Bit-equal, NaN canaries included."""
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())


def rel(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)


def _case(lib, L, p, seed_case):
    """Five sequences of L rows (sequence 0 and 4 are outside the launch: NaN canaries), key padding 1 .. L."""
    g = torch.Generator().manual_seed(1000 + 7 * L + seed_case)
    Sn, seq0, nseq = 5, 1, 3
    qlens = [L] * Sn
    kvalid = [L, 1, max(1, (L + 1) // 2), L, max(1, L - 1)]
    qrow0 = [sum(qlens[:s]) for s in range(Sn)]
    R_ = sum(qlens)
    pl, ptk = L + 3, L + 5                          # P strides beyond lmax / tkmax
    run = list(range(seq0, seq0 + nseq))
    seed = OT.op_seed(17, 110)
    qkv = torch.randn(R_, 3 * D, generator=g)
    q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    o_ref, _ = R.attention_reference(q64, k64, v64, qrow0, qlens, qrow0, qlens, NH, pl, ptk, p, seed, run, kvalid=kvalid)
    dout = torch.randn(R_, D, generator=g)
    o_ref.backward(dout.double())
    qkvd = qkv.to(DEV)
    qp, kp, vp = P(qkvd), P(qkvd, D), P(qkvd, 2 * D)
    o = nan_like(R_, D)
    Pb = nan_like(Sn * NH * pl * ptk)
    d_row0, d_len, d_valid = i32(qrow0), i32(qlens), i32(kvalid)
    assert lib.ac_attn_seq_fwd(qp, 3 * D, kp, 3 * D, vp, 3 * D, P(o), D, P(Pb), pl, ptk, P(d_row0), P(d_len), P(d_row0),
                               P(d_len), P(d_valid), None, 0, 0, seq0, nseq, NH, HD, L, L, p, seed, None, S()) == 0
    rows = torch.cat([torch.arange(qrow0[s], qrow0[s] + L) for s in run])
    out = torch.ones(R_, dtype=torch.bool)
    out[rows] = False
    assert rel(o.cpu()[rows], o_ref[rows]) < EXACT_F32
    ddo = dout.to(DEV)

    def launch(fn, with_ws=True):
        """The tiled kernel with its D workspace (as the training step calls it) or without (D recomputed)."""
        dqkv = nan_like(R_, 3 * D)
        args = [qp, 3 * D, kp, 3 * D, vp, 3 * D, P(Pb), pl, ptk, P(ddo), D, P(dqkv), 3 * D, P(dqkv, D), 3 * D,
                P(dqkv, 2 * D), 3 * D, P(d_row0), P(d_len), P(d_row0), P(d_len), seq0, nseq, NH, HD, L, L, p, seed, None]
        if fn is lib.ac_attn_self_bwd_tiled:
            args.append(P(nan_like(nseq * NH * pl)) if with_ws else None)
        return fn(*args, S()), dqkv

    P_before = Pb.clone()
    rc, dqkv = launch(lib.ac_attn_self_bwd_tiled)
    assert rc == 0
    torch.cuda.synchronize()
    assert same(Pb, P_before)
    c = dqkv.cpu()
    worst = {n: rel(c[rows, i * D:(i + 1) * D], t.grad[rows]) for i, (n, t) in enumerate((("dq", q64), ("dk", k64),
                                                                                          ("dv", v64)))}
    print(f"L {L} p {p}: {worst}")
    assert max(worst.values()) < EXACT_F32, worst
    assert torch.isnan(c[out]).all()                 # rows of sequences outside the launch: untouched
    rc2, again = launch(lib.ac_attn_self_bwd_tiled)
    assert rc2 == 0 and same(again.cpu(), c)         # deterministic: bit-identical on a second launch
    rc3, no_ws = launch(lib.ac_attn_self_bwd_tiled, with_ws=False)
    assert rc3 == 0 and same(no_ws.cpu(), c)         # D from the workspace == D recomputed in the key pass
    return c, launch, rows


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("L", [1, 2, 32, 33, 91, 92, 94, 95, 126])
def test_tiled_self_attention_backward(lib, L, p):
    c, launch, rows = _case(lib, L, p, 0)
    rc_old, old = launch(lib.ac_attn_seq_bwd)
    if L <= 91:
        # where the one-workgroup kernel fits, both agree to the exact-f32 bar
        assert rc_old == 0
        assert rel(c[rows], old.cpu()[rows]) < EXACT_F32
    else:
        assert rc_old != 0                         # ac_attn_seq_bwd refuses (and this kernel exists for that reason)


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_tiled_backward_ragged_rows_and_cross_lengths(lib, p):
    """Sequences shorter than lmax / tkmax (partial last tiles, workgroups whose tile starts beyond the sequence) and
    qlen != klen (cross attention: query and key rows in separate buffers), key padding inside, NaN canaries around."""
    g = torch.Generator().manual_seed(77)
    qlens = [5, 17, 1, 95, 40, 33]
    klens = [9, 3, 94, 126, 1, 16]
    kvalid = [9, 2, 50, 126, 1, 7]
    Sn, seq0, nseq = len(qlens), 1, 4
    lmax, tkmax = 100, 126                          # launch-wide bounds above every launched sequence
    pl, ptk = lmax + 2, tkmax + 3
    qrow0 = [sum(qlens[:s]) for s in range(Sn)]
    krow0 = [sum(klens[:s]) for s in range(Sn)]
    Rq, Rk = sum(qlens), sum(klens)
    run = list(range(seq0, seq0 + nseq))
    seed = OT.op_seed(23, 112)
    qb = torch.randn(Rq, D, generator=g)
    kvb = torch.randn(Rk, 2 * D, generator=g)
    q, k, v = qb, kvb[:, :D], kvb[:, D:]
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    o_ref, _ = R.attention_reference(q64, k64, v64, qrow0, qlens, krow0, klens, NH, pl, ptk, p, seed, run, kvalid=kvalid)
    dout = torch.randn(Rq, D, generator=g)
    o_ref.backward(dout.double())
    qd, kvd, ddo = qb.to(DEV), kvb.to(DEV), dout.to(DEV)
    o = nan_like(Rq, D)
    Pb = nan_like(Sn * NH * pl * ptk)
    dq0, dql, dk0, dkl, dkv_ = i32(qrow0), i32(qlens), i32(krow0), i32(klens), i32(kvalid)
    assert lib.ac_attn_seq_fwd(P(qd), D, P(kvd), 2 * D, P(kvd, D), 2 * D, P(o), D, P(Pb), pl, ptk, P(dq0), P(dql), P(dk0),
                               P(dkl), P(dkv_), None, 0, 0, seq0, nseq, NH, HD, lmax, tkmax, p, seed, None, S()) == 0
    dq, dkv = nan_like(Rq, D), nan_like(Rk, 2 * D)
    assert lib.ac_attn_self_bwd_tiled(P(qd), D, P(kvd), 2 * D, P(kvd, D), 2 * D, P(Pb), pl, ptk, P(ddo), D, P(dq), D,
                                      P(dkv), 2 * D, P(dkv, D), 2 * D, P(dq0), P(dql), P(dk0), P(dkl), seq0, nseq, NH, HD,
                                      lmax, tkmax, p, seed, None, P(nan_like(nseq * NH * pl)), S()) == 0
    qrows = torch.cat([torch.arange(qrow0[s], qrow0[s] + qlens[s]) for s in run])
    krows = torch.cat([torch.arange(krow0[s], krow0[s] + klens[s]) for s in run])
    dqc, dkvc = dq.cpu(), dkv.cpu()
    worst = {"dq": rel(dqc[qrows], q64.grad[qrows]), "dk": rel(dkvc[krows, :D], k64.grad[krows]),
             "dv": rel(dkvc[krows, D:], v64.grad[krows])}
    print(f"ragged p {p}: {worst}")
    assert max(worst.values()) < EXACT_F32, worst
    qout = torch.ones(Rq, dtype=torch.bool)
    qout[qrows] = False
    kout = torch.ones(Rk, dtype=torch.bool)
    kout[krows] = False
    assert torch.isnan(dqc[qout]).all() and torch.isnan(dkvc[kout]).all()
    assert not torch.isnan(dqc[qrows]).any() and not torch.isnan(dkvc[krows]).any()


def test_tiled_backward_in_a_captured_graph_equals_eager(lib):
    _, launch, _ = _case(lib, 95, 0.2, 1)
    eager = launch(lib.ac_attn_self_bwd_tiled)[1]
    torch.cuda.synchronize()
    keep = []
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc, buf = launch(lib.ac_attn_self_bwd_tiled)
        keep.append(buf)
    assert rc == 0
    graph.replay()
    torch.cuda.synchronize()
    dqkv = keep[0]
    assert same(dqkv, eager)


def test_tiled_backward_refuses_bad_arguments(lib):
    z = ctypes.c_void_p(0)
    buf = torch.zeros(4, device=DEV)
    a = P(buf)
    # head_dim other than 64, and lmax beyond the P stride
    assert lib.ac_attn_self_bwd_tiled(a, 1, a, 1, a, 1, a, 4, 4, a, 1, a, 1, a, 1, a, 1, a, a, a, a, 0, 1, 1, 32, 4, 4, 0.0,
                                      0, None, None, S()) != 0
    assert lib.ac_attn_self_bwd_tiled(a, 1, a, 1, a, 1, a, 4, 4, a, 1, a, 1, a, 1, a, 1, a, a, a, a, 0, 1, 1, 64, 5, 4, 0.0,
                                      0, None, None, S()) != 0
    assert lib.ac_attn_self_bwd_tiled(a, 1, a, 1, a, 1, z, 4, 4, a, 1, a, 1, a, 1, a, 1, a, a, a, a, 0, 1, 1, 64, 4, 4, 0.0,
                                      0, None, None, S()) != 0
