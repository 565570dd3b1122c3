"""GPU parity tests of the training step through the C ABI:
kernel by kernel against torch-CPU autograd / the oracle (dropout ACTIVE, same counter-hash masks), and the whole
step against the gradients the reference itself produced (tests/golden/g8_train.npz, dropout 0)."""
import ctypes
import math
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


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


def P(t):
    if t is None:
        return None
    _KEEP.append(t)
    return ctypes.c_void_p(t.data_ptr())


def rel(name, got, want, scale=None):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    sc = float(want.abs().max()) if scale is None else scale
    d = float((got - want).abs().max()) / (sc + 1e-30)
    print(f"[{name}] max|diff| / max|want| = {d:.3e} (max|want| {sc:.3e})")
    return d


# ---------------------------------------------------------------------------------------------------------
def test_general_gemm_all_layouts(lib):
    g = torch.Generator().manual_seed(0)
    M, N, K = 150, 200, 330
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    # y = relu(x w^T + b)
    y = torch.empty(M, N, device="cuda")
    assert lib.ac_gemm(P(xd), K, 1, P(wd), 1, K, P(y), N, M, N, K, P(bd), 1, 0.0, 1, 0.0, 0, None, 0, None, 0, S()) == 0
    assert rel("x w^T + b, relu", y, torch.relu(x.double() @ w.double().t() + b.double())) < 1e-5
    # dx = dy w, accumulated on top of an existing tensor (beta = 1)
    dy = torch.randn(M, N, generator=g)
    dx0 = torch.randn(M, K, generator=g)
    dx = dx0.cuda()
    assert lib.ac_gemm(P(dy.cuda()), N, 1, P(wd), K, 1, P(dx), K, M, K, N, None, 0, 1.0, 1, 0.0, 0, None, 0, None, 0, S()) == 0
    assert rel("dy w + dx0", dx, dy.double() @ w.double() + dx0.double()) < 1e-5
    # dw += dy^T x, split-K with atomics, strided views (ld > width)
    dyp = torch.randn(M, N + 24, generator=g)
    xp = torch.randn(M, K + 8, generator=g)
    for splitk in (1, 3, 8):
        dw0 = torch.randn(N, K, generator=g)
        dw = dw0.cuda()
        dyd, xdp = dyp.cuda(), xp.cuda()
        assert lib.ac_gemm(P(dyd), 1, N + 24, P(xdp), K + 8, 1, P(dw), K, N, K, M, None, 0, 1.0, splitk, 0.0, 0, None, 0,
                           None, 0, S()) == 0
        want = dyp[:, :N].double().t() @ xp[:, :K].double() + dw0.double()
        assert rel(f"dy^T x split-K {splitk}", dw, want) < 1e-5
    # rejected combinations
    assert lib.ac_gemm(P(xd), K, 1, P(wd), 1, K, P(y), N, M, N, K, P(bd), 0, 1.0, 4, 0.0, 0, None, 0, None, 0, S()) == -1


@pytest.mark.parametrize("M,N,K", [(1344, 768, 256), (7392, 256, 1024), (520, 1024, 512), (4100, 260, 776)])
def test_split_bf16_gemm_all_layouts(lib, M, N, K):
    """ac_gemm_bf16x3 (three bf16 MFMAs per product on operands split into hi + lo at staging) in the three layouts the
    training step uses - x w^T (+ bias, ReLU), dy w (+ beta), dy^T x (split-K atomics, strided views) - against float64:
    2^-16 relative operand error, so 3e-5 of the largest output instead of the exact-f32 kernels' 1e-5; tile tails
    (M, N, K not multiples of the 128 / 64 / 32 tile) included."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g)
    b = torch.randn(N, generator=g)
    xd, wd, bd = x.cuda(), w.cuda(), b.cuda()
    y = torch.empty(M, N, device="cuda")
    assert lib.ac_gemm_bf16x3(P(xd), K, 1, P(wd), 1, K, P(y), N, M, N, K, P(bd), 1, 0.0, 1, 0.0, 0, None, 0, None, 0, S()) == 0
    assert rel("bf16x3: x w^T + b, relu", y, torch.relu(x.double() @ w.double().t() + b.double())) < 3e-5
    dy = torch.randn(M, N, generator=g)
    dx0 = torch.randn(M, K, generator=g)
    dx = dx0.cuda()
    assert lib.ac_gemm_bf16x3(P(dy.cuda()), N, 1, P(wd), K, 1, P(dx), K, M, K, N, None, 0, 1.0, 1, 0.0, 0, None, 0, None, 0,
                              S()) == 0
    assert rel("bf16x3: dy w + dx0", dx, dy.double() @ w.double() + dx0.double()) < 3e-5
    dyp = torch.randn(M, N + 24, generator=g)
    xp = torch.randn(M, K + 8, generator=g)
    for splitk in (1, 7):
        dw0 = torch.randn(N, K, generator=g)
        dw = dw0.cuda()
        assert lib.ac_gemm_bf16x3(P(dyp.cuda()), 1, N + 24, P(xp.cuda()), K + 8, 1, P(dw), K, N, K, M, None, 0, 1.0, splitk,
                                  0.0, 0, None, 0, None, 0, S()) == 0
        want = dyp[:, :N].double().t() @ xp[:, :K].double() + dw0.double()
        assert rel(f"bf16x3: dy^T x split-K {splitk}", dw, want) < 3e-5
    # a layout it cannot take (rows of 4981 floats are not 16-byte aligned) is forwarded to the exact-f32 kernels
    V = 4981
    dl = torch.randn(672, V, generator=g)
    wc = torch.randn(V, 256, generator=g)
    dxl = torch.empty(672, 256, device="cuda")
    assert lib.ac_gemm_bf16x3(P(dl.cuda()), V, 1, P(wc.cuda()), 256, 1, P(dxl), 256, 672, 256, V, None, 0, 0.0, 1, 0.0, 0,
                              None, 0, None, 0, S()) == 0
    assert rel("forwarded: dl w_cls", dxl, dl.double() @ wc.double()) < 1e-5
    # the squeeze-excite form of EfficientNet's projection convs: y = res + swish?(x .* gate[row group]) w^T + b
    rows_per = 64
    G = (M + rows_per - 1) // rows_per
    gate = torch.rand(G, K, generator=g)
    res = torch.randn(M, N, generator=g)
    yg = res.clone().cuda()
    assert lib.ac_gemm_bf16x3(P(xd), K, 1, P(wd), 1, K, P(yg), N, M, N, K, P(bd), 0, 1.0, 1, 0.0, 0, None, 0, P(gate.cuda()),
                              rows_per, S()) == 0
    xg = x.double() * gate.double().repeat_interleave(rows_per, 0)[:M]
    assert rel("bf16x3: gated x w^T + b + res", yg, res.double() + xg @ w.double().t() + b.double()) < 3e-5


def test_dropout_hash_is_the_oracles(lib):
    from oracle import train_path as OT
    n = 100003
    x = torch.ones(n, device="cuda")
    y = torch.empty_like(x)
    for p, seed, idx0 in ((0.2, OT.op_seed(7, 3), 0), (0.5, OT.op_seed(123456789, 35), 4096), (0.9, 1, 77)):
        assert lib.ac_dropout(P(x), P(y), n, p, seed, None, idx0, S()) == 0
        want = OT.drop_mask(seed, idx0, n, p)
        assert np.array_equal(y.cpu().numpy(), want), f"mask differs for p={p}"
        keep = float((want > 0).mean())
        assert abs(keep - (1 - p)) < 0.01
    # device-side base seed: effective seed = op + (base << 16)
    base = torch.tensor([99], dtype=torch.int64, device="cuda")
    assert lib.ac_dropout(P(x), P(y), n, 0.2, 5, P(base), 0, S()) == 0
    assert np.array_equal(y.cpu().numpy(), OT.drop_mask(OT.op_seed(99, 5), 0, n, 0.2))


def test_dropadd_layernorm_forward_backward(lib):
    from oracle import train_path as OT
    g = torch.Generator().manual_seed(1)
    R, p, seed, row0 = 77, 0.2, OT.op_seed(3, 31), 5
    x = torch.randn(row0 + R, 256, generator=g)
    res = torch.randn(row0 + R, 256, generator=g)
    gamma, beta = torch.randn(256, generator=g), torch.randn(256, generator=g)
    mask = torch.from_numpy(OT.drop_mask(seed, 0, (row0 + R) * 256, p)).view(-1, 256)
    xr, rr, gr, br = (t.clone().requires_grad_(True) for t in (x, res, gamma, beta))
    y_ref = torch.nn.functional.layer_norm(rr + xr * mask, (256,), gr, br)
    dy = torch.randn(row0 + R, 256, generator=g)
    dy[:row0] = 0  # rows outside the forward range of this test
    y_ref.backward(dy)
    pre = torch.zeros(row0 + R, 256, device="cuda")
    y = torch.zeros(row0 + R, 256, device="cuda")
    assert lib.ac_dropadd_ln_fwd(P(x.cuda()), P(res.cuda()), P(gamma.cuda()), P(beta.cuda()), P(pre), P(y), row0, R, 0, 256,
                                 p, seed, None, 1e-5, S()) == 0
    assert rel("ln fwd", y[row0:], y_ref[row0:]) < 1e-5
    # backward over rows 0..: fill the untouched head of `pre` so that the kernel sees valid numbers
    pre[:row0] = (res + x * mask)[:row0].cuda()
    dx = torch.empty_like(pre)
    dres = torch.empty_like(pre)
    dgam = torch.zeros(256, device="cuda")
    dbet = torch.zeros(256, device="cuda")
    assert lib.ac_dropadd_ln_bwd(P(dy.cuda()), P(pre), P(gamma.cuda()), P(dx), P(dres), 0, None, 0, P(dgam), P(dbet),
                                 row0 + R, 256, p, seed, None, 1e-5, S()) == 0
    assert rel("ln dx", dx, xr.grad) < 1e-5
    assert rel("ln dres", dres, rr.grad) < 1e-5
    assert rel("ln dgamma", dgam, gr.grad) < 1e-5
    assert rel("ln dbeta", dbet, br.grad) < 1e-5


def _attention_case(lib, cross):
    from oracle import train_path as OT
    g = torch.Generator().manual_seed(2 + cross)
    nh, hd, T, Tk_max = 4, 64, 6, 9
    lens = [1, 4, 6, 3]
    S_ = len(lens)
    qrow0 = np.cumsum([0] + lens[:-1]).astype(np.int32)
    R = int(sum(lens))
    p, seed = 0.2, OT.op_seed(11, 30 + 2 * cross)
    q = torch.randn(R, nh * hd, generator=g)
    if cross:
        klen = [Tk_max] * S_
        kvalid = [9, 5, 1, 7]
        krow0 = (np.arange(S_) * Tk_max).astype(np.int32)
        Rk = S_ * Tk_max
        word = None
    else:
        klen, kvalid, krow0, Rk = lens, None, qrow0, R
        word = torch.randint(1, 50, (R,), generator=g).int()
        word[qrow0[2] + 2] = 0  # a pad token inside sequence 2 (masked as a key)
    k = torch.randn(Rk, nh * hd, generator=g)
    v = torch.randn(Rk, nh * hd, generator=g)
    ptk = Tk_max if cross else T
    dout = torch.randn(R, nh * hd, generator=g)
    # torch reference
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    outs = []
    for s in range(S_):
        L, Tk = lens[s], klen[s]
        qs = qr[qrow0[s]:qrow0[s] + L].view(L, nh, hd).transpose(0, 1)
        ks = kr[krow0[s]:krow0[s] + Tk].view(Tk, nh, hd).transpose(0, 1)
        vs = vr[krow0[s]:krow0[s] + Tk].view(Tk, nh, hd).transpose(0, 1)
        sc = qs @ ks.transpose(1, 2) / math.sqrt(hd)
        ok = torch.ones(L, Tk, dtype=torch.bool)
        if cross:
            ok &= (torch.arange(Tk) < kvalid[s])[None, :]
        else:
            ok &= torch.tril(torch.ones(L, Tk, dtype=torch.bool))
            ok &= (word[qrow0[s]:qrow0[s] + Tk] != 0)[None, :]
        sc = sc.masked_fill(~ok[None], float("-inf"))
        m = torch.from_numpy(OT.drop_mask(seed, s * nh * T * ptk, nh * T * ptk, p)).view(nh, T, ptk)[:, :L, :Tk]
        a = torch.softmax(sc, -1) * m
        outs.append((a @ vs).transpose(0, 1).reshape(L, nh * hd))
    o_ref = torch.cat(outs)
    o_ref.backward(dout)
    # HIP
    dev = "cuda"
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    o = torch.zeros(R, nh * hd, device=dev)
    Pb = torch.zeros(S_ * nh * T * ptk, device=dev)
    i32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int32)).to(dev)
    qrow0_d, qlen_d, krow0_d, klen_d = i32(qrow0), i32(lens), i32(krow0), i32(klen)
    kvalid_d = i32(kvalid) if cross else None
    word_d = word.to(dev) if word is not None else None
    lmax, tkmax = max(lens), max(klen)
    assert lib.ac_attn_seq_fwd(P(qd), 256, P(kd), 256, P(vd), 256, P(o), 256, P(Pb), T, ptk, P(qrow0_d), P(qlen_d),
                               P(krow0_d), P(klen_d), P(kvalid_d) if cross else None,
                               P(word_d) if word is not None else None, 0, 0 if cross else 1, 0, S_, nh, hd, lmax, tkmax,
                               p, seed, None, S()) == 0
    assert rel("attention out", o, o_ref) < 1e-5
    dq, dk, dv = (torch.zeros_like(t, device=dev) for t in (q, k, v))
    assert lib.ac_attn_seq_bwd(P(qd), 256, P(kd), 256, P(vd), 256, P(Pb), T, ptk, P(dout.to(dev)), 256, P(dq), 256, P(dk),
                               256, P(dv), 256, P(qrow0_d), P(qlen_d), P(krow0_d), P(klen_d), 0, S_, nh, hd, lmax, tkmax,
                               p, seed, None, S()) == 0
    assert rel("attention dq", dq, qr.grad) < 1e-5
    assert rel("attention dk", dk, kr.grad) < 1e-5
    assert rel("attention dv", dv, vr.grad) < 1e-5


def test_self_attention_forward_backward(lib):
    _attention_case(lib, 0)


def test_cross_attention_forward_backward(lib):
    _attention_case(lib, 1)


def test_gru_layer_train_forward_backward(lib):
    from oracle import cpu_path as O
    g = torch.Generator().manual_seed(4)
    B, T, H = 3, 9, 256
    lens = [9, 4, 1]
    gx = torch.randn(B, T, 2, 3 * H, generator=g) * 0.5
    whh = torch.randn(2, 3 * H, H, generator=g) * 0.06
    bhh = torch.randn(2, 3 * H, generator=g) * 0.1
    dout = torch.randn(B, T, 2 * H, generator=g)
    # reference: explicit recurrence with autograd (gx plays x W_ih^T + b_ih: identity input projection)
    from _train_ref import gru_bidir_reference
    gxr, whr, bhr = (t.clone().requires_grad_(True) for t in (gx, whh, bhh))
    out_ref = gru_bidir_reference(gxr, whr, bhr, lens)
    out_ref.backward(dout)
    dev = "cuda"
    whhT = torch.empty(2, H, 3 * H, device=dev)
    whh_d = whh.to(dev)
    assert lib.ac_transpose(P(whh_d), P(whhT), 2, 3 * H, H, S()) == 0
    assert torch.equal(whhT.cpu(), whh.transpose(1, 2).contiguous())
    assert lib.ac_gru_pack_whh(P(whh_d), P(whhT), H, S()) == 0          # [2][H/4][3H][4]
    assert torch.equal(whhT.cpu().view(2, H // 4, 3 * H, 4), whh.view(2, 3 * H, H // 4, 4).permute(0, 2, 1, 3))
    out = torch.empty(B, T, 2 * H, device=dev)
    save = torch.empty(B, T, 2, 4 * H, device=dev)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    gx_d, bhh_d = gx.to(dev), bhh.to(dev)
    assert lib.ac_gru_layer_train(P(gx_d), P(whhT), P(bhh_d), P(lens_d), P(out), P(save), B, T, H, S()) == 0
    assert rel("gru out", out, out_ref) < 1e-5
    # same numbers as the inference kernel
    out_inf = torch.empty_like(out)
    assert lib.ac_gru_layer(P(gx_d), P(whhT), P(bhh_d), P(lens_d), P(out_inf), B, T, H, S()) == 0
    assert torch.equal(out_inf, out)
    dgx = torch.empty(B, T, 2, 3 * H, device=dev)
    dgh = torch.empty(B, T, 2, 3 * H, device=dev)
    hprev = torch.empty(B, T, 2, H, device=dev)
    assert lib.ac_gru_layer_bwd(P(dout.to(dev)), P(out), P(save), P(whh_d), P(lens_d), P(dgx), P(dgh), P(hprev), B, T, H,
                                S()) == 0
    assert rel("gru dgx", dgx, gxr.grad) < 2e-5
    dwhh = torch.einsum("btdn,btdk->dnk", dgh.cpu().double(), hprev.cpu().double())
    assert rel("gru dW_hh", dwhh, whr.grad) < 2e-5
    assert rel("gru db_hh", dgh.cpu().double().sum((0, 1)), bhr.grad) < 2e-5
    # the 4-way split forward (what the engine runs) leaves the same gates for the same backward: the cells of valid
    # steps agree with the single-workgroup kernel's, the cells of padded steps are never written by either
    out_s = torch.full_like(out, float("nan"))
    save_s = torch.full_like(save, float("nan"))
    xch = torch.zeros((lib.ac_gru_split_workspace_bytes(B) + 7) // 8, device=dev, dtype=torch.int64)
    assert lib.ac_gru_layer_split(P(gx_d), P(whh_d), P(bhh_d), P(lens_d), P(out_s), P(save_s), P(xch), B, T, H, S()) == 0
    assert int(xch.view(torch.int32)[0]) == 0
    assert rel("split gru out", out_s, out_ref) < 1e-5
    for b, n in enumerate(lens):
        assert float((save_s[b, :n] - save[b, :n]).abs().max()) < 1e-5
        assert torch.isnan(save_s[b, n:]).all()
    dgx_s, dgh_s, hprev_s = torch.empty_like(dgx), torch.empty_like(dgh), torch.empty_like(hprev)
    assert lib.ac_gru_layer_bwd(P(dout.to(dev)), P(out_s), P(save_s), P(whh_d), P(lens_d), P(dgx_s), P(dgh_s), P(hprev_s),
                                B, T, H, S()) == 0
    assert rel("split gru dgx", dgx_s, gxr.grad) < 2e-5
    dwhh = torch.einsum("btdn,btdk->dnk", dgh_s.cpu().double(), hprev_s.cpu().double())
    assert rel("split gru dW_hh", dwhh, whr.grad) < 2e-5


def test_label_smoothing_loss_vs_reference_value_and_autograd(lib, golden_dir, state4981):
    from audiocaption_amd.loss import LabelSmoothingLoss
    from oracle import train_path as OT
    g7 = dict(np.load(os.path.join(golden_dir, "g7_loss.npz")))
    g3 = dict(np.load(os.path.join(golden_dir, "g3_decoder.npz")))
    # the reference value was computed on the reference decoder's logits; rebuild them with the oracle (CPU)
    from oracle import cpu_path as O
    word = torch.from_numpy(g3["word"])
    logit = O.decoder_forward(state4981, word, torch.from_numpy(g3["attn_emb"]), torch.from_numpy(g3["attn_emb_len"]),
                              word == 0)["logit"][:, :11].contiguous()
    tgt, tgt_len = torch.from_numpy(g7["tgt"]), torch.from_numpy(g7["tgt_len"])
    lg = logit.cuda().requires_grad_(True)
    loss = LabelSmoothingLoss(smoothing=0.1)({"logit": lg, "tgt": tgt, "tgt_len": tgt_len})
    assert abs(float(loss) - float(g7["loss"])) < 2e-5 * float(g7["loss"])
    (loss * 3.0).backward()
    lr = logit.clone().requires_grad_(True)
    (OT.label_smoothing_loss(lr, tgt, tgt_len, 0.1) * 3.0).backward()
    assert rel("dlogit", lg.grad, lr.grad) < 1e-5
    # sum / none reductions
    s = LabelSmoothingLoss(smoothing=0.1, reduction="sum")({"logit": lg.detach(), "tgt": tgt, "tgt_len": tgt_len})
    assert abs(float(s) / float(tgt_len.sum()) - float(g7["loss"])) < 2e-5 * float(g7["loss"])
    n = LabelSmoothingLoss(smoothing=0.1, reduction="none")({"logit": lg.detach(), "tgt": tgt, "tgt_len": tgt_len})
    assert n.shape == (4, 11) and float(n[1, 9:].abs().max()) == 0.0


def test_clip_and_fused_adam_match_torch_semantics(lib):
    from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
    from oracle import train_path as OT
    g = torch.Generator().manual_seed(5)
    shapes = [(300, 70), (513,), (64, 64)]
    params = {f"p{i}": torch.randn(*s, generator=g) for i, s in enumerate(shapes)}
    ref_p = {k: v.clone() for k, v in params.items()}
    m1 = {k: torch.zeros_like(v) for k, v in params.items()}
    m2 = {k: torch.zeros_like(v) for k, v in params.items()}
    for flat in (False, True):
        if flat:  # parameters and gradients as views of two flat buffers -> one launch
            tot = sum(v.numel() for v in params.values())
            fp, fg = torch.zeros(tot, device="cuda"), torch.zeros(tot, device="cuda")
            dev_p, o = [], 0
            for k, v in params.items():
                t = torch.nn.Parameter(fp[o:o + v.numel()].view(v.shape))
                t.data.copy_(v)
                t.grad = fg[o:o + v.numel()].view(v.shape)
                dev_p.append(t)
                o += v.numel()
        else:
            dev_p = [torch.nn.Parameter(v.clone().cuda()) for v in params.values()]
        opt = FusedAdam(dev_p, lr=5e-4, weight_decay=1e-6)
        rp = {k: v.clone() for k, v in ref_p.items()}
        r1 = {k: v.clone() for k, v in m1.items()}
        r2 = {k: v.clone() for k, v in m2.items()}
        for step in (1, 2, 3):
            grads = {k: torch.randn(*v.shape, generator=g) * (10.0 if step == 2 else 0.01) for k, v in params.items()}
            for t, gr in zip(dev_p, grads.values()):
                if t.grad is None:
                    t.grad = gr.cuda()
                else:
                    t.grad.copy_(gr)
            clip = clip_grad_norm_(dev_p, 1.0, scale_now=(step == 3))
            opt.step(clip=None if step == 3 else clip)
            norm = OT.clip_and_adam(rp, grads, r1, r2, step)
            assert abs(float(clip.total_norm) - float(norm)) < 1e-5 * float(norm)
            for t, k in zip(dev_p, rp):
                assert rel(f"flat={flat} step {step} {k}", t.data, rp[k]) < 2e-6
        sd = opt.state_dict()
        assert sd["state"][0]["step"] == 3 and sd["state"][0]["exp_avg"].shape == shapes[0]


def test_argmax_rows(lib):
    g = torch.Generator().manual_seed(6)
    x = torch.randn(7, 3, 4981, generator=g)
    x[2, 1, 100] = x[2, 1, 4000] = 50.0  # tie -> first index
    xd = x.cuda()
    out = torch.full((7, 3), -1, dtype=torch.int32, device="cuda")
    assert lib.ac_argmax_rows(ctypes.c_void_p(xd.data_ptr() + 4 * 4981), 3 * 4981, 7, 4981,
                              ctypes.c_void_p(out.data_ptr() + 4), 3, S()) == 0
    assert torch.equal(out[:, 1].cpu().long(), x[:, 1].argmax(-1)) and int(out[2, 1]) == 100
    assert int(out[0, 0]) == -1


# ---------------------------------------------------------------------------------------------------------
# the assembled training step
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture()
def train_model(state4981):
    import audiocaption_amd as A
    model = A.init_model_from_config(A.cnn14rnn_trm_config(4981), print_fn=lambda s: None)
    model.load_state_dict(state4981, strict=True)
    model = model.to("cuda:0")
    model.train()
    return model


def _set_dropout(model, p_dec, p_rnn, cnn_train):
    for m in model.decoder.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = p_dec
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = p_dec
    model.encoder.rnn.network.dropout = p_rnn
    model.encoder.cnn.train(cnn_train)


def _cnn_attn_f32(model, lms):
    """Cnn14 output from a given log-mel with the exact-f32 conv kernels (the goldens start at the log-mel)."""
    from test_gpu_model import _cnn_from_logmel
    cnn = model.encoder.cnn
    algo = cnn.conv_algo
    cnn.conv_algo = "winograd"
    try:
        attn, _ = _cnn_from_logmel(cnn, lms)
    finally:
        cnn.conv_algo = algo
    return attn


@pytest.mark.parametrize("tag", ["ss", "tf"])
def test_training_step_vs_reference_gradients(train_model, golden_dir, tag):
    """Forward logits / greedy tokens / loss, every parameter's gradient and the first Adam update against what the
    REFERENCE produced (dropout 0): scheduled sampling (ss) and pure teacher forcing (tf)."""
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.loss import LabelSmoothingLoss
    from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
    g8 = dict(np.load(os.path.join(golden_dir, "g8_train.npz")))
    model = train_model
    _set_dropout(model, 0.0, 0.0, False)
    lms = torch.from_numpy(Pr.synthetic_logmel(4, 1001)).cuda()
    cnn_attn = _cnn_attn_f32(model, lms)
    cap = torch.from_numpy(g8["cap"]).cuda()
    cap_len = g8["cap_len"]
    ss_ratio = 1 if tag == "tf" else 0.7
    random.seed(5)  # the reference drew its scheduled-sampling choices from this stream
    out = model({"mode": "train", "wav": torch.zeros(4, 320000, device="cuda"), "wav_len": g8["wav_len"].tolist(),
                 "specaug": False, "cap": cap, "cap_len": cap_len, "ss_ratio": ss_ratio, "_cnn_attn": cnn_attn})
    logit = out["logit"]
    top_val, top_idx = logit.detach().topk(8, dim=-1)
    assert rel("logit top-8", top_val, g8[f"{tag}_logit_top_val"]) < 2e-5
    assert np.array_equal(top_idx.cpu().numpy()[..., 0], g8[f"{tag}_logit_top_idx"][..., 0])
    if tag == "ss":
        assert np.array_equal(out["seq"].cpu().numpy(), g8["ss_seq"])
    loss = LabelSmoothingLoss(smoothing=0.1)({"logit": logit, "tgt": cap[:, 1:], "tgt_len": torch.as_tensor(cap_len - 1)})
    assert abs(float(loss) - float(g8[f"{tag}_loss"])) < 2e-5 * float(g8[f"{tag}_loss"])
    loss.backward()
    named = dict(model.named_parameters())
    worst, bad = 0.0, []
    for key in [k[len("sample_idx/"):] for k in g8 if k.startswith("sample_idx/")]:
        grad = named[key].grad
        assert grad is not None, key
        gn = float(g8[f"{tag}_gnorm/{key}"])
        d_norm = abs(float(grad.double().norm()) - gn) / (gn + 1e-12)
        sample = grad.reshape(-1)[torch.from_numpy(g8[f"sample_idx/{key}"]).cuda()].cpu().numpy()
        want = g8[f"{tag}_gsample/{key}"]
        d_s = float(np.abs(sample - want).max()) / (float(np.abs(grad.cpu().numpy()).max()) + 1e-12)
        worst = max(worst, d_norm, d_s)
        print(f"  {key:60s} grad norm rel diff {d_norm:.2e}, sample diff {d_s:.2e}")
        if not (d_norm < 1e-4 and d_s < 1e-4):
            bad.append(key)
    print(f"[{tag}] worst relative gradient difference vs the reference: {worst:.3e}")
    assert not bad, f"gradients differ from the reference's: {bad}"
    params = [p for p in model.parameters() if p.requires_grad]
    before = {k: named[k].detach().clone() for k in named if named[k].requires_grad}
    clip = clip_grad_norm_(params, 1.0)
    assert abs(float(clip.total_norm) - float(g8[f"{tag}_total_norm"])) < 1e-4 * float(g8[f"{tag}_total_norm"])
    FusedAdam(params, lr=5e-4, weight_decay=1e-6).step()
    for key in before:
        idx = torch.from_numpy(g8[f"sample_idx/{key}"]).cuda()
        delta = (named[key].detach() - before[key]).reshape(-1)[idx].cpu().numpy()
        want = g8[f"{tag}_delta/{key}"]
        gs = np.abs(g8[f"{tag}_gsample/{key}"])
        # Adam's first step is lr * g / (|g| + 1e-8), i.e. lr * sign(g) unless |g| is near eps: entries whose gradient is
        # within the GEMMs' error of zero are skipped (split-bf16 GEMMs: 7e-6 of the tensor's max; exact f32: 1e-6)
        solid = gs > 1e-4 * (gs.max() + 1e-30) + 1e-6
        assert np.abs(delta - want)[solid].max(initial=0.0) < 5e-6, key


def test_training_step_with_dropout_vs_oracle(train_model, state4981):
    """Dropout ACTIVE everywhere (Cnn14 0.2, GRU 0.5, decoder 0.2) and SpecAugment on: the HIP step and the CPU oracle
    regenerate the same counter-hash masks and stripe draws, so logits, tokens, loss and gradients must agree."""
    from audiocaption_amd import kernels as K
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.train import TrainEngine
    from audiocaption_amd.loss import _launch
    from oracle import train_path as OT
    model = train_model
    _set_dropout(model, 0.2, 0.5, True)
    B, L = 3, 192000
    wav = torch.from_numpy(Pr.synthetic_wav(B, L, seed=3)).cuda()
    wav_len = [192000, 150000, 100000]
    g = torch.Generator().manual_seed(21)
    cap = torch.randint(4, 4981, (B, 9), generator=g)
    cap_len = np.array([9, 6, 8])
    cap[:, 0] = 1
    for i, n in enumerate(cap_len):
        cap[i, n - 1] = 2
        cap[i, n:] = 0
    use_cap = [1, 0, 1, 1, 0, 0, 1, 0]
    seed = 1234
    eng = TrainEngine(model)
    cnn = model.encoder.cnn
    cnn.conv_algo = "winograd"
    out = eng.forward({"mode": "train", "wav": wav, "wav_len": wav_len, "specaug": True, "cap": cap.cuda(),
                       "cap_len": cap_len, "ss_ratio": 0.5, "_use_cap": use_cap, "dropout_seed": seed})
    sv = eng._saved
    cnn_attn = sv["cnn_attn"].cpu()
    # (1) Cnn14 with dropout: oracle from the HIP log-mel
    T, Hs, Hp = cnn.geometry(L)
    pk = cnn._pack(wav.device)
    lms = K.logmel(wav, cnn._tables, rows_per_clip=Hp[0], channels_last=True).view(B, Hp[0], 64)[:, :T].transpose(1, 2)
    stripes = OT.specaug_stripes(OT.op_seed(seed, OT.OP_SPECAUG), B, T)
    assert stripes[:, :2, 1].max() < 64 and stripes[:, 2:, 1].max() < 8 and (stripes[:, :2].sum(-1) <= T).all()
    o_cnn = OT.cnn14_train_from_logmel(state4981, lms.cpu(), seed, 0.2, rows_per_clip=Hp[1:] + [Hp[5]], specaug=True)
    o_plain = OT.cnn14_train_from_logmel(state4981, lms.cpu(), seed, 0.2, rows_per_clip=Hp[1:] + [Hp[5]])
    assert float((o_cnn - o_plain).abs().max()) > 1e-3       # the stripes did change the features
    assert rel("cnn attn (dropout)", cnn_attn, o_cnn) < 1e-4
    # (2) the rest from the HIP Cnn14 output
    lens = OT.O.cnn14_feat_len(wav_len)
    # ReLU kinks: a pre-activation within 1e-5 of zero lies on either side depending on the last bits of the forward (the
    # 4-way split GRU kernel and the single-workgroup one differ by 1e-6 there), and its side switches a whole gradient
    # path.  The oracle takes the side the HIP forward took for exactly those cells (oracle/train_path.py _relu_at_kinks).
    ws_, R_ = sv["ws"], sv["lay"]["R"]
    rows_m = sv["N"] * sv["Tq"]
    gates = {"mem": ws_.tensor("mem_a")[:rows_m * 256].view(rows_m, 256).cpu(),
             "ffn": [ws_.tensor(f"hdn{l}")[:R_ * sv["F"]].view(R_, sv["F"]).cpu() for l in range(model.decoder.nlayers)]}
    o = OT.train_step_grads(state4981, cnn_attn, lens, cap, cap_len, use_cap, base_seed=seed, p_dec=0.2, p_rnn=0.5,
                            relu_gates=gates)
    assert rel("logit", out["logit"], o["logit"]) < 5e-5
    assert torch.equal(out["seq"].cpu(), o["seq"])
    logit = out["logit"]
    tgt_len = torch.as_tensor(cap_len - 1)
    count = float(tgt_len.sum())
    dlogit = torch.empty_like(logit)
    loss, _ = _launch(logit, cap[:, 1:].cuda(), tgt_len.to(device="cuda", dtype=torch.int32), 0.1, 1.0 / count, dlogit,
                      1.0 / count, None)
    assert abs(float(loss) - float(o["loss"])) < 2e-5 * float(o["loss"])
    eng.backward(dlogit)
    worst, bad = 0.0, []
    for key, view in zip(eng.flat.names, eng.flat.grad_views):
        d = rel(key, view, o["grads"][key])
        worst = max(worst, d)
        if not d < 2e-4:
            bad.append((key, d))
    assert not bad, bad
    print(f"worst relative gradient difference vs the oracle (dropout on): {worst:.3e}")


def test_engine_step_trains_and_refreshes_inference_weights(train_model):
    """TrainEngine.step (fused loss/backward/clip/Adam): the loss of a fixed batch goes down, dropout masks change
    from step to step, and eval-mode decoding afterwards uses the UPDATED weights."""
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.optim import FusedAdam
    from audiocaption_amd.train import TrainEngine
    model = train_model
    B, L = 4, 160000
    wav = torch.from_numpy(Pr.synthetic_wav(B, L, seed=9)).cuda()
    g = torch.Generator().manual_seed(2)
    cap = torch.randint(4, 4981, (B, 10), generator=g)
    cap[:, 0], cap[:, -1] = 1, 2
    batch = {"mode": "train", "wav": wav, "wav_len": [L] * B, "specaug": False, "cap": cap.cuda(),
             "cap_len": np.array([10] * B), "ss_ratio": 0.8}
    model.eval()
    with torch.no_grad():
        logit0 = model({"mode": "inference", "wav": wav, "wav_len": [L] * B, "specaug": False,
                        "sample_method": "greedy", "max_length": 10})["logit"][:, 0].clone()
    model.train()
    eng = TrainEngine(model, seed=100)
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=5e-4, weight_decay=1e-6)
    random.seed(0)
    losses = []
    for it in range(12):
        r = eng.step(batch, opt, smoothing=0.1, max_grad_norm=1.0)
        losses.append(float(r["loss"]))
    print("losses:", [f"{v:.3f}" for v in losses])
    assert all(np.isfinite(losses)) and losses[-1] < losses[0] - 0.5
    assert eng.seed == 112
    model.eval()
    with torch.no_grad():
        out = model({"mode": "inference", "wav": wav, "wav_len": [L] * B, "specaug": False,
                     "sample_method": "greedy", "max_length": 10})
    # 12 updates towards `cap` must have moved the first-step logit of the target word up
    first = cap[:, 1].cuda()
    gain = out["logit"][:, 0].gather(1, first[:, None]) - logit0.gather(1, first[:, None])
    print("first-word logit gain:", gain.flatten().tolist())
    assert float(gain.min()) > 0.0


def test_swa_and_nan_skip_on_device(train_model):
    """SWA over the flat parameter buffer (one launch) equals the running mean of the snapshots; a non-finite gradient
    makes clip + Adam skip the update on the device (run.py:123) instead of poisoning the parameters."""
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
    from audiocaption_amd.train import TrainEngine
    from audiocaption_amd.trainer import SwaAverager
    model = train_model
    B, L = 2, 96000
    wav = torch.from_numpy(Pr.synthetic_wav(B, L, seed=4)).cuda()
    cap = torch.tensor([[1, 9, 30, 2, 0], [1, 7, 7, 12, 2]])
    batch = {"mode": "train", "wav": wav, "wav_len": [L] * B, "specaug": False, "cap": cap.cuda(),
             "cap_len": np.array([4, 5]), "ss_ratio": 0.9}
    eng = TrainEngine(model)
    model._train_engine = eng
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    swa = SwaAverager(model)
    key = "decoder.classifier.weight"
    snaps = []
    for _ in range(3):
        eng.step(batch, opt)
        snaps.append(dict(model.named_parameters())[key].detach().clone())
        swa.update_parameters(model)
    want = sum(snaps) / 3
    assert rel("swa average", swa.state_dict()[key], want) < 1e-6
    assert swa.n_averaged == 3 and set(swa.state_dict()) == set(model.state_dict())
    # poison one gradient entry: the norm is NaN -> flag set, coefficient 0, parameters and moments unchanged
    before = eng.flat.flat.clone()
    m_before = opt._flat_state[0]["m"].clone()
    eng.flat.attach_grads()
    eng.flat.grad[5] = float("nan")
    clip = clip_grad_norm_(eng.flat.params, 1.0, scale_now=False)
    opt.step(clip=clip)
    assert float(clip.state[3]) == 1.0 and float(clip.state[2]) == 0.0
    assert torch.equal(eng.flat.flat, before) and torch.equal(opt._flat_state[0]["m"], m_before)
    # the skipped update does not advance Adam's step count either (the reference never calls optimizer.step() then)
    sd = opt.state_dict()
    assert all(int(v["step"]) == 3 for v in sd["state"].values())
    # a loaded state replaces the flat moment buffers and the device-side step count
    sd["state"][0]["exp_avg"] = torch.full_like(sd["state"][0]["exp_avg"], 0.25)
    for v in sd["state"].values():
        v["step"] = 7
    opt.load_state_dict(sd)
    assert opt._flat_state == {} and opt._step_dev == {}
    eng.flat.grad.zero_()
    opt.step()                                                 # zero gradient: m <- 0.9 m
    p0 = opt.param_groups[0]["params"][0]
    assert rel("adopted first moment", opt.state[p0]["exp_avg"], torch.full_like(p0, 0.225)) < 1e-6
    assert all(int(v["step"]) == 8 for v in opt.state_dict()["state"].values())


def test_generic_optimizer_skips_a_non_finite_step(train_model):
    """``engine.step`` with a plain torch optimiser: a NaN loss (here: a NaN smoothing constant) must leave the parameters
    untouched - scaling NaN gradients by a zero clip coefficient would still hand NaNs to the optimiser (run.py:123)."""
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.train import TrainEngine
    model = train_model
    B, L = 2, 96000
    wav = torch.from_numpy(Pr.synthetic_wav(B, L, seed=4)).cuda()
    cap = torch.tensor([[1, 9, 30, 2, 0], [1, 7, 7, 12, 2]])
    batch = {"mode": "train", "wav": wav, "wav_len": [L] * B, "specaug": False, "cap": cap.cuda(),
             "cap_len": np.array([4, 5]), "ss_ratio": 0.9}
    eng = TrainEngine(model)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-2, momentum=0.9)
    r = eng.step(batch, opt, use_graph=False)
    assert np.isfinite(float(r["loss"]))
    before = eng.flat.flat.clone()
    r = eng.step(batch, opt, smoothing=float("nan"), use_graph=False)
    assert not np.isfinite(float(r["loss"]))
    assert torch.equal(eng.flat.flat, before) and torch.isfinite(eng.flat.flat).all()
    r = eng.step(batch, opt, use_graph=False)                  # and training goes on
    assert np.isfinite(float(r["loss"])) and not torch.equal(eng.flat.flat, before)


def test_replayed_graph_after_a_buffer_regrow_equals_the_eager_step(train_model):
    """Captured step graphs hold raw addresses of the frozen Cnn14's packed weights and of its shared activation buffers.
    Optimiser steps must not repack the frozen network, and a larger batch shape re-allocating the shared buffers must
    make the older shape's graph re-capture: with lr = 0 (parameters fixed) and a fixed dropout seed, a step of the
    small shape gives the SAME loss eagerly, captured, replayed, and replayed again after the larger shape ran."""
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.optim import FusedAdam
    from audiocaption_amd.train import TrainEngine
    model = train_model
    eng = TrainEngine(model, seed=3)
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=0.0)
    base = torch.from_numpy(Pr.synthetic_wav(4, 256000, seed=12, varied=True)).cuda()
    g = torch.Generator().manual_seed(3)

    def batch(L, Tc, n):
        cap = torch.randint(4, 4981, (n, Tc), generator=g)
        cap[:, 0], cap[:, -1] = 1, 2
        return {"mode": "train", "wav": base[:n, :L].contiguous(), "wav_len": [L] * n, "specaug": False, "cap": cap.cuda(),
                "cap_len": np.array([Tc] * n), "ss_ratio": 0.8, "dropout_seed": 11, "_use_cap": [1, 0, 1, 1, 0, 1, 1][:Tc - 1]}

    small, big = batch(96000, 6, 2), batch(256000, 8, 4)

    def run(b, **kw):   # (loss, gradient norm): the norm pins the BACKWARD of the replayed graphs as well - a replay that
        r = eng.step(b, opt, **kw)   # accumulates onto a buffer the capture zeroed only once shows up here, not in the loss
        return float(r["loss"]), float(r["total_norm"])

    eager = run(small, use_graph=False)
    cnn = model.encoder.cnn
    tier = cnn.effective_algo(None, True)                               # the conv tier of the train-mode forward
    pack_id = id(cnn._packed[tier][1])
    ptr_small = cnn._bufs[("full", torch.float32)].data_ptr()
    vals = [run(small) for _ in range(4)]                              # eager (first of the shape), capture, replay, replay
    st_small = eng._states[next(k for k in eng._states if k[1] == 2)]
    assert "fwd0" in st_small["graphs"] and "tail" in st_small["graphs"]
    assert id(cnn._packed[tier][1]) == pack_id                      # optimiser steps do not repack the frozen Cnn14
    big_eager = run(big, use_graph=False)                               # larger shape: shared buffers re-allocated
    assert cnn._bufs[("full", torch.float32)].data_ptr() != ptr_small or cnn._bufs[("full", torch.float32)].numel() > 0
    filler = torch.full((int(1e8),), 3.0, device="cuda")                # recycle the freed blocks
    big_vals = [run(big) for _ in range(4)]
    after = [run(small) for _ in range(2)]                             # must re-capture, not replay stale addresses
    del filler
    print("small:", eager, vals, after, "big:", big_eager, big_vals)
    for v in vals + after:
        assert abs(v[0] - eager[0]) < 1e-5 * abs(eager[0])
        assert abs(v[1] - eager[1]) < 1e-3 * abs(eager[1])             # split-K slices accumulate atomically: order-dependent rounding
    for v in big_vals:
        assert abs(v[0] - big_eager[0]) < 1e-5 * abs(big_eager[0])
        assert abs(v[1] - big_eager[1]) < 1e-3 * abs(big_eager[1])


def test_changing_batch_shapes_share_one_workspace(train_model):
    """Real batches are padded to their longest clip / caption, so shapes change all the time: the activation workspace is
    shared (grows to the largest shape only), per-shape states are an LRU, and a graph captured for a shape is
    re-captured when a later, larger shape re-allocated the buffers it points into."""
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.optim import FusedAdam
    from audiocaption_amd.train import TrainEngine
    model = train_model
    eng = TrainEngine(model, seed=7)
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    rng = np.random.default_rng(0)
    base = torch.from_numpy(Pr.synthetic_wav(4, 224000, seed=12)).cuda()
    g = torch.Generator().manual_seed(3)

    def batch(L, Tc, n=4):
        cap = torch.randint(4, 4981, (n, Tc), generator=g)
        cap[:, 0], cap[:, -1] = 1, 2
        return {"mode": "train", "wav": base[:n, :L].contiguous(), "wav_len": [L] * n, "specaug": False, "cap": cap.cuda(),
                "cap_len": np.array([Tc] * n), "ss_ratio": 0.8}

    random.seed(2)
    small = batch(96000, 6)
    for _ in range(3):                       # eager, capture, replay
        r = eng.step(small, opt)
    st_small = next(iter(eng._states.values()))
    assert "fwd0" in st_small["graphs"] and "tail" in st_small["graphs"]
    gen0 = eng._wsg.gen
    losses = [float(r["loss"])]
    torch.cuda.synchronize()
    mem0 = torch.cuda.memory_allocated()
    for i in range(24):                      # 24 different shapes: lengths and caption lengths keep changing
        L = int(rng.integers(30, 70)) * 3200
        losses.append(float(eng.step(batch(L, int(rng.integers(5, 12))), opt)["loss"]))
    assert len(eng._states) <= 16 and all(np.isfinite(losses))
    assert eng._wsg.gen > gen0               # larger shapes re-allocated shared buffers ...
    r = eng.step(small, opt)                 # ... so the small shape (if still cached) must re-capture, not replay stale addresses
    assert np.isfinite(float(r["loss"]))
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - mem0
    print(f"memory growth over 24 shapes: {grown / 2**20:.0f} MiB, states {len(eng._states)}, workspace generation {eng._wsg.gen}")
    assert grown < 3 * 2**30


def test_split_gru_timeout_skips_the_update_on_the_device(train_model):
    """A partner timeout of the split GRU kernel (sticky error word of its exchange area) must not reach the parameters:
    the word is folded into the clip state's non-finite flag on the device, the update is skipped like a NaN loss
    (run.py:123) and counted, the word is cleared in stream order so that the NEXT iteration updates again (a sticky word
    used to skip every later update silently), ``gru_timeout()`` reports the hit once, and training goes on."""
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.optim import FusedAdam
    from audiocaption_amd.train import TrainEngine
    model = train_model
    B, L = 2, 96000
    wav = torch.from_numpy(Pr.synthetic_wav(B, L, seed=4)).cuda()
    cap = torch.tensor([[1, 9, 30, 2, 0], [1, 7, 7, 12, 2]])
    batch = {"mode": "train", "wav": wav, "wav_len": [L] * B, "specaug": False, "cap": cap.cuda(),
             "cap_len": np.array([4, 5]), "ss_ratio": 0.9}
    eng = TrainEngine(model)
    if eng.gru_algo != "split":
        pytest.skip("single-workgroup GRU: no partner protocol")
    opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3)
    for _ in range(3):                                   # eager, capture, replay
        eng.step(batch, opt)
    assert eng.gru_timeout() is False
    st = next(iter(eng._states.values()))
    before = eng.flat.flat.clone()
    eng._gru_error_word(st).fill_(1)                    # what a timed-out workgroup leaves behind
    r = eng.step(batch, opt)
    assert np.isfinite(float(r["loss"]))
    assert torch.equal(eng.flat.flat, before)
    assert all(int(v["step"]) == 3 for v in opt.state_dict()["state"].values())
    assert int(r["skipped_updates"]) == 1 and eng.skipped_updates() == 1
    # the word judged ONE iteration: the next one updates again without anybody having called gru_timeout() in between
    r2 = eng.step(batch, opt)
    assert not torch.equal(eng.flat.flat, before) and int(r2["skipped_updates"]) == 1
    assert eng.gru_timeout() is True and eng.gru_timeout() is False


# Adam's epsilon in the tests that compare two SCHEDULES of the same training run step by step.  With the default 1e-8 the
# first updates are lr * sign(gradient) whatever the gradient's size: a parameter whose gradient is zero up to the step's own
# summation noise (atomics: ~1e-12) moves by +-lr at random, and after three steps the loss of ONE run comes out in two
# variants 1e-4 apart (tools/train_bimodal.py: 333 parameters flipped together in 4 of 24 identical runs, the frozen Cnn14's
# output bit-identical in all of them).  1e-5 keeps the update proportional to such gradients: the trajectories are then a
# continuous function of the arithmetic and two schedules can be held to the step's noise.
TRAJ_EPS = 1e-5


def test_cnn_look_ahead_is_the_same_training_trajectory(train_model, state4981):
    """``step(..., next_batch=...)`` launches the frozen Cnn14 forward of the NEXT iteration on a side stream under this
    iteration's GRU / decoder work.  The masks are the ones the in-line forward draws (same counter hash, same seed word),
    so losses and parameters after five iterations over two alternating batches (with SpecAugment and dropout on) are
    those of the plain loop up to the step's own run-to-run noise - eager, capture and replay included."""
    import random
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.optim import FusedAdam
    from audiocaption_amd.train import TrainEngine
    model = train_model
    B, L = 2, 96000
    batches = []
    for k in range(2):
        wav = torch.from_numpy(Pr.synthetic_wav(B, L, seed=4 + k, varied=True)).cuda()
        cap = torch.tensor([[1, 9 + k, 30, 2, 0], [1, 7, 7 + k, 12, 2]])
        batches.append({"mode": "train", "wav": wav, "wav_len": [L, L - 16000 * k], "specaug": True, "cap": cap.cuda(),
                        "cap_len": np.array([4, 5]), "ss_ratio": 1.0})   # teacher forced: a free-running pass would turn a
        #                                       last-bit difference of a logit into another token now and then - chaos, not schedule

    def run(look_ahead):
        model.load_state_dict(state4981, strict=True)
        model.train()
        random.seed(3)
        eng = TrainEngine(model, seed=77)
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3, eps=TRAJ_EPS)
        losses = []
        for it in range(5):
            nxt = batches[(it + 1) % 2] if look_ahead and it < 4 else None
            losses.append(float(eng.step(batches[it % 2], opt, next_batch=nxt)["loss"]))
        torch.cuda.synchronize()
        assert eng.skipped_updates() == 0 and not eng.gru_timeout()
        return losses, eng.flat.flat.clone()

    plain, p0 = run(False)
    ahead, p1 = run(True)
    print("losses plain", plain, "look-ahead", ahead)
    # the step itself is reproducible to a few ulp only (split-K products and the loss sum accumulate with device atomics: two
    # PLAIN runs differ by ~3e-7 in the loss), so the two schedules are held to that noise, not to bit equality
    assert all(abs(a - b) <= 5e-6 * abs(a) for a, b in zip(plain, ahead))
    # (Adam turns a last-bit difference of a near-zero gradient into a full +-lr step of that one parameter: the mean
    # over the 10.7 M parameters is what shows that the trajectories coincide)
    # ... and a single parameter can be off by at most 2 * lr per iteration (both runs stepping it in opposite directions)
    assert float((p0 - p1).abs().mean()) <= 1e-7 and float((p0 - p1).abs().max()) <= 2 * 1e-3 * 5 * 1.01


def test_cnn_look_ahead_keeps_the_callers_seed_and_notices_a_refilled_batch(train_model, state4981):
    """The look-ahead must not change WHAT is computed: (a) an explicit ``dropout_seed`` (resume, reproducibility) wins over
    the seed the look-ahead guessed a step earlier; (b) a loader that refills ONE static ``wav`` tensor in place gets the
    features of the new contents, not those computed from the old ones (the look-ahead is keyed on storage, version counter,
    shape, SpecAugment flag, mode and seed - ``TrainEngine._pf_key``); (c) a train-mode ``forward`` between two steps, which
    advances the engine's seed, does not make the next step reuse masks that forward already drew."""
    import random
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.optim import FusedAdam
    from audiocaption_amd.train import TrainEngine
    model = train_model
    B, L = 2, 96000
    wavs = [torch.from_numpy(Pr.synthetic_wav(B, L, seed=14 + k, varied=True)).cuda() for k in range(3)]
    cap = torch.tensor([[1, 9, 30, 2, 0], [1, 7, 8, 12, 2]]).cuda()

    def batch(wav, **kw):
        return dict({"mode": "train", "wav": wav, "wav_len": [L, L - 16000], "specaug": True, "cap": cap,
                     "cap_len": np.array([4, 5]), "ss_ratio": 1.0}, **kw)

    def run(schedule):
        model.load_state_dict(state4981, strict=True)
        model.train()
        random.seed(3)
        eng = TrainEngine(model, seed=77)
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3, eps=TRAJ_EPS)
        losses = schedule(eng, opt)
        torch.cuda.synchronize()
        assert eng.skipped_updates() == 0 and not eng.gru_timeout()
        return losses

    seeds = [501, 77, 9000]   # explicit seeds, unrelated to the engine's own sequence

    def plain(eng, opt):
        return [float(eng.step(batch(wavs[i], dropout_seed=seeds[i]), opt)["loss"]) for i in range(3)]

    def ahead_explicit(eng, opt):   # (a): next_batch carries its own seed
        out = []
        for i in range(3):
            nxt = batch(wavs[i + 1], dropout_seed=seeds[i + 1]) if i < 2 else None
            out.append(float(eng.step(batch(wavs[i], dropout_seed=seeds[i]), opt, next_batch=nxt)["loss"]))
        return out

    def ahead_guessed_wrong(eng, opt):   # (a'): the look-ahead guessed the default seed, the step then names another one
        out = []
        for i in range(3):
            nxt = batch(wavs[i + 1]) if i < 2 else None     # no seed: prefetched with the engine's default
            out.append(float(eng.step(batch(wavs[i], dropout_seed=seeds[i]), opt, next_batch=nxt)["loss"]))
        return out

    def ahead_refilled(eng, opt):   # (b): one static tensor, refilled in place between the look-ahead and its step
        static = wavs[0].clone()
        out = []
        for i in range(3):
            cur = batch(static, dropout_seed=seeds[i])
            out.append(float(eng.step(cur, opt, next_batch=batch(static, dropout_seed=seeds[min(i + 1, 2)]))["loss"]))
            if i < 2:
                torch.cuda.synchronize()
                static.copy_(wavs[i + 1])    # the look-ahead already ran on the OLD contents
        return out

    ref = run(plain)
    for name, sched in (("explicit", ahead_explicit), ("guessed", ahead_guessed_wrong), ("refilled", ahead_refilled)):
        got = run(sched)
        print(name, ref, got)
        assert all(abs(a - b) <= 5e-6 * abs(a) for a, b in zip(ref, got)), (name, ref, got)

    # (c) default seeds with a train-mode forward between two steps
    def plain_fwd(eng, opt):
        a = float(eng.step(batch(wavs[0]), opt)["loss"])
        eng.forward(batch(wavs[2]))
        return [a, float(eng.step(batch(wavs[1]), opt)["loss"])]

    def ahead_fwd(eng, opt):
        a = float(eng.step(batch(wavs[0]), opt, next_batch=batch(wavs[1]))["loss"])
        eng.forward(batch(wavs[2]))                     # advances the seed: the look-ahead's guess is stale now
        return [a, float(eng.step(batch(wavs[1]), opt)["loss"])]

    ref, got = run(plain_fwd), run(ahead_fwd)
    print("forward between", ref, got)
    assert all(abs(a - b) <= 5e-6 * abs(a) for a, b in zip(ref, got))


def test_graph_replay_after_host_sync_equals_eager(train_model, state4981):
    """Replayed iterations must not depend on what the host did between them.  The split GRU kernel's ticket / granule
    clearing used to be a hipMemsetAsync: as a memset node it was not reliably ordered before the kernel node in replays,
    and with the host synchronised before a replay every workgroup took itself for a surplus one and returned (a stale layer
    output: losses 6.70 / 5.92 instead of 6.73 / 5.81 from the third iteration on).  Eager and graph, each with a device
    synchronisation before every step, give the same trajectory."""
    from audiocaption_amd import procedural as Pr
    from audiocaption_amd.optim import FusedAdam
    from audiocaption_amd.train import TrainEngine
    model = train_model
    B, L = 2, 96000
    batches = []
    for k in range(2):
        wav = torch.from_numpy(Pr.synthetic_wav(B, L, seed=4 + k, varied=True)).cuda()
        cap = torch.tensor([[1, 9 + k, 30, 2, 0], [1, 7, 7 + k, 12, 2]])
        batches.append({"mode": "train", "wav": wav, "wav_len": [L, L - 16000 * k], "specaug": True, "cap": cap.cuda(),
                        "cap_len": np.array([4, 5]), "ss_ratio": 1.0})

    def run(use_graph):
        model.load_state_dict(state4981, strict=True)
        model.train()
        eng = TrainEngine(model, seed=77)
        opt = FusedAdam([p for p in model.parameters() if p.requires_grad], lr=1e-3, eps=TRAJ_EPS)
        losses = []
        for it in range(5):
            torch.cuda.synchronize()
            losses.append(float(eng.step(batches[it % 2], opt, use_graph=use_graph)["loss"]))
        assert eng.skipped_updates() == 0 and not eng.gru_timeout()
        return losses

    eager, graph = run(False), run(True)
    print("losses eager", eager, "graph", graph)
    assert all(abs(a - b) <= 5e-6 * abs(a) for a, b in zip(eager, graph))
