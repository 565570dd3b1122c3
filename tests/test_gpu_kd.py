"""GPU tests of token-level knowledge distillation on the HIP path: the kernel of csrc/kd.hip against the float64
restatement (tests/_kd_ref.py) and against what the reference's own losses computed (tests/golden/g18_kd.npz), the loss
modules under autograd, the eval-mode (teacher) forward of TrainEngine, and ``TrainEngine.step(kd=...)`` against the
bridge path and under graph replay.

Bounds.  Kernel and modules: the project's own from test_gpu_scst.py (loss 2e-5 of its scale, row terms 2e-5 of their
maximum, dlogit 1e-5 of its maximum).  Step against step (tests 5 and 6), per tensor and relative to its maximum:
the loss 1e-5 and the gradient norm 1e-3 are the bounds test_gpu_train.py already holds graph replay to against the eager
step; the parameters after the update get ten times the measured run-to-run spread of the plain label-smoothing step at
this shape, and not below 1e-5 - the largest spread measured is 4.58e-6 (tests/golden/REPORT_kd.txt), so 4.6e-5.
"""
import os

import numpy as np
import pytest
import torch

import _kd_ref as K

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V = 4981
SMOOTHING = 0.1
TEMPS = [0.5, 1.0, 2.0]
WEIGHTS = [0.0, 0.5, 1.0]
TOL_LOSS, TOL_NORM, TOL_PARAM = 1e-5, 1e-3, 4.6e-5   # see the module docstring
TRAJ_EPS = 1e-5                                      # Adam's eps of the trajectory tests (test_gpu_train.py TRAJ_EPS)


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def g18(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g18_kd.npz")))


def rel(name, got, want):
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    d = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)
    print(f"[{name}] {d:.3e}")
    return d


# ---- 1. ac_kd_loss ---------------------------------------------------------------------------------------------------
def _tgt_lens(N, T):
    """A full row, a short row, a row beyond T (clamped) and, for N > 1, a row of length 1.  The four kinds do not all fit
    into one or two clips: N = 1 has the clamped (= full) row only and no masked position, N = 2 the clamped row and the
    row of length 1 (which is its short row); N = 3 and N = 5 hold every kind as a row of its own."""
    return {1: [T + 2], 2: [T + 2, 1], 3: [T + 2, max(T - 2, 1), 1], 5: [T, max(T - 3, 1), T + 2, 1, T - 1]}[N]


def _kernel_case(N, T, Vc, seed):
    g = torch.Generator().manual_seed(seed)
    logit = torch.randn(N, T, Vc, generator=g) * 2.5
    tchr = torch.randn(N, T, Vc, generator=g) * 2.5
    logit[0, 0] += 90.0                      # without the maximum subtraction exp overflows at temp 0.5
    tchr[0, min(1, T - 1)] += 90.0
    tgt = torch.randint(0, Vc, (N, T), generator=g)
    tgt_len = torch.tensor(_tgt_lens(N, T))
    mask = K.valid_mask(tgt_len, T)
    tchr_dev = tchr.clone()
    tchr_dev[~mask] = float("nan")           # a teacher's values at padded positions must not reach the loss
    return logit, tchr, tchr_dev, tgt, tgt_len, mask


def _check_kernel(logit, tchr, tchr_dev, tgt, tgt_len, mask, temp, w, want_loss=None, want_dlogit=None):
    from audiocaption_amd.kd_loss import _launch
    N, T, Vc = logit.shape
    lg, tc = logit.to(DEV), tchr_dev.to(DEV)
    tg, tl = tgt.to(DEV), tgt_len.to(device=DEV, dtype=torch.int32)
    loss64, sup64, kd64, scale = K.kd_loss(logit, tchr, tgt, tgt_len, SMOOTHING, temp, w)
    rs64, rk64 = K.row_sup(logit, tchr, tgt, tgt_len, SMOOTHING, temp), K.row_kd(logit, tchr, tgt, tgt_len, SMOOTHING, temp)
    d64 = K.kd_dlogit(logit, tchr, tgt, tgt_len, SMOOTHING, temp, w, g=1.7)
    count = float(mask.sum())
    got = {}
    # inv_count / gscale given, and "<= 0": the count taken from tgt_len on the device
    for tag, inv in (("host count", 1.0 / count), ("device count", 0.0)):
        dlogit = torch.full_like(lg, float("nan"))
        gdev = torch.tensor([1.7], device=DEV)
        loss, row_sup, row_kd = _launch(lg, tc, tg, tl, SMOOTHING, temp, w, inv, dlogit, inv, gdev)
        loss, row_sup, row_kd = loss.cpu().double(), row_sup.cpu().double().view(N, T), row_kd.cpu().double().view(N, T)
        print(f"N {N} T {T} V {Vc} temp {temp} w {w} ({tag}): loss {float(loss[0]):.6f} vs {float(loss64):.6f} "
              f"(|d| {abs(float(loss[0]) - float(loss64)):.2e}, scale {float(scale):.3e}), sup {float(loss[1]):.6f} vs "
              f"{float(sup64):.6f}, kd {float(loss[2]):.6f} vs {float(kd64):.6f}, rows sup "
              f"{float((row_sup - rs64).abs().max()):.2e} kd {float((row_kd - rk64).abs().max()):.2e}")
        assert not torch.isnan(loss).any() and not torch.isnan(row_sup).any() and not torch.isnan(row_kd).any()
        assert abs(float(loss[0]) - float(loss64)) <= 2e-5 * float(scale)
        assert abs(float(loss[1]) - float(sup64)) <= 2e-5 * float(rs64.abs().sum() / count)
        assert abs(float(loss[2]) - float(kd64)) <= 2e-5 * float(rk64.abs().sum() / count)
        assert float((row_sup - rs64).abs().max()) <= 2e-5 * float(rs64.abs().max())
        assert float((row_kd - rk64).abs().max()) <= 2e-5 * float(rk64.abs().max())
        assert float(row_sup[~mask].abs().sum()) == 0.0
        assert float(row_kd[~mask].abs().sum()) == 0.0
        assert rel("dlogit", dlogit, d64) < 1e-5
        dl = dlogit.cpu()
        assert not torch.isnan(dl).any()
        assert float(dl[~mask].abs().sum()) == 0.0                           # exactly 0 on masked rows
        got[tag] = (loss, row_sup, dl)
    if want_loss is not None:                # the reference's own numbers
        loss, _, dl = got["host count"]
        assert abs(float(loss[0]) - want_loss) <= 2e-5 * float(scale)
        assert rel("dlogit vs the reference", dl / 1.7, want_dlogit) < 1e-5
    return got["host count"]


@pytest.mark.parametrize("N,T,Vc", [(1, 1, 2), (2, 3, 255), (2, 3, 256), (2, 3, 257), (3, 4, 1025), (5, 7, 4981),
                                    (3, 4, 16384)])
def test_kd_loss_kernel_vs_float64(lib, N, T, Vc):
    from audiocaption_amd.loss import _launch as xent_launch
    logit, tchr, tchr_dev, tgt, tgt_len, mask = _kernel_case(N, T, Vc, 1000 * N + 10 * T + Vc % 7)
    lens = tgt_len.tolist()
    assert max(lens) > T and (N == 1 or 1 in lens)
    count = float(mask.sum())
    for temp in TEMPS:
        for w in WEIGHTS:
            loss, row_sup, dl = _check_kernel(logit, tchr, tchr_dev, tgt, tgt_len, mask, temp, w)
            if w == 1.0:
                # sup_weight 1 is the label-smoothing loss of csrc/train.hip on the same inputs
                lg = logit.to(DEV)
                xd = torch.empty_like(lg)
                xl, xrow = xent_launch(lg, tgt.to(DEV), tgt_len.to(device=DEV, dtype=torch.int32), SMOOTHING, 1.0 / count, xd,
                                       1.0 / count, torch.tensor([1.7], device=DEV))
                xrow = xrow.cpu().double().view(N, T)
                assert abs(float(loss[0]) - float(xl)) <= 2e-5 * float(xrow.abs().sum() / count)
                assert float((row_sup - xrow).abs().max()) <= 2e-5 * float(xrow.abs().max())
                assert rel("dlogit vs ac_label_smoothing_loss", dl, xd) < 1e-5


def test_kd_loss_kernel_on_unaligned_views(lib):
    """Base pointers that are only 4-byte aligned take the word-by-word route: same numbers."""
    logit, tchr, tchr_dev, tgt, tgt_len, mask = _kernel_case(2, 3, 257, 5)
    from audiocaption_amd.kd_loss import _launch
    N, T, Vc = logit.shape
    pad = lambda x: torch.cat([torch.zeros(1), x.reshape(-1)]).to(DEV)[1:].view(N, T, Vc)
    lg, tc = pad(logit), pad(tchr_dev)
    assert lg.data_ptr() % 16 == 4 and lg.is_contiguous()
    dbuf = torch.full((N * T * Vc + 1,), float("nan"), device=DEV)
    dlogit = dbuf[1:].view(N, T, Vc)
    loss, _, _ = _launch(lg, tc, tgt.to(DEV), tgt_len.to(device=DEV, dtype=torch.int32), SMOOTHING, 2.0, 0.5, 0.0, dlogit, 0.0,
                         None)
    want, _, _, scale = K.kd_loss(logit, tchr, tgt, tgt_len, SMOOTHING, 2.0, 0.5)
    assert abs(float(loss[0]) - float(want)) <= 2e-5 * float(scale)
    assert rel("dlogit (unaligned)", dlogit, K.kd_dlogit(logit, tchr, tgt, tgt_len, SMOOTHING, 2.0, 0.5)) < 1e-5
    assert bool(torch.isnan(dbuf[:1]).all())                  # the word before the view is untouched


def test_kd_loss_kernel_vs_reference_fixture(lib, g18):
    logit, tchr = torch.from_numpy(g18["logit"]), torch.from_numpy(g18["tchr_logit"])
    tgt, tgt_len = torch.from_numpy(g18["tgt"]), torch.from_numpy(g18["tgt_len"])
    mask = K.valid_mask(tgt_len, logit.shape[1])
    for temp in g18["temps"].tolist():
        for w in g18["weights"].tolist():
            _check_kernel(logit, tchr, tchr, tgt, tgt_len, mask, temp, w, want_loss=float(g18[f"loss/{temp:g}/{w:g}"]),
                          want_dlogit=g18[f"dlogit/{temp:g}/{w:g}"])


# ---- 2. refusals -------------------------------------------------------------------------------------------------------
def test_kd_loss_kernel_refuses_bad_arguments(lib):
    from audiocaption_amd import _lib
    x = torch.zeros(2, 3, 10, device=DEV)
    tg = torch.zeros(2, 3, device=DEV, dtype=torch.int64)
    tl = torch.tensor([3, 2], device=DEV, dtype=torch.int32)
    rs, rk, ls = torch.zeros(6, device=DEV), torch.zeros(6, device=DEV), torch.zeros(3, device=DEV)
    P = _lib.ptr

    def call(temp=1.0, w=0.5, Vc=10, logit=x, tchr=x):
        return lib.ac_kd_loss(P(logit), P(tchr), P(tg), 3, P(tl), 2, 3, Vc, 0.1, temp, w, 0.0, P(rs), P(rk), P(ls), None, 0.0,
                              None, _lib.stream())

    assert call() == 0
    assert call(w=0.0) == 0 and call(w=1.0) == 0
    for bad in (dict(Vc=1), dict(Vc=16385), dict(temp=0.0), dict(temp=float("nan")), dict(temp=float("inf")),
                dict(temp=-1.0), dict(w=-0.1), dict(w=1.1), dict(w=float("nan")), dict(tchr=None), dict(logit=None)):
        assert call(**bad) == _lib.AC_ERR_ARG, bad
    torch.cuda.synchronize()


# ---- 3. the loss modules ---------------------------------------------------------------------------------------------
def test_loss_modules_under_autograd(lib):
    from audiocaption_amd.kd_loss import SupKdLoss, TokenLevelKdLoss
    from audiocaption_amd.loss import LabelSmoothingLoss
    logit, tchr, tchr_dev, tgt, tgt_len, mask = _kernel_case(3, 4, 1025, 77)
    count = float(mask.sum())
    temp, w = 2.0, 0.3

    def run(fn):
        la = logit.to(DEV).requires_grad_(True)
        ta = tchr_dev.to(DEV).requires_grad_(True)
        loss = fn({"logit": la, "tchr_logit": ta, "tgt": tgt.to(DEV), "tgt_len": tgt_len})
        (loss * 3.0).backward()
        assert ta.grad is None                                            # the teacher gets no gradient
        return float(loss), la.grad

    # the fused pair: one launch each way
    fused = SupKdLoss(LabelSmoothingLoss(SMOOTHING), TokenLevelKdLoss(temp), w)
    assert fused.fused()
    want, _, _, scale = K.kd_loss(logit, tchr, tgt, tgt_len, SMOOTHING, temp, w)
    got, grad = run(fused)
    assert abs(got - float(want)) <= 2e-5 * float(scale)
    assert rel("fused dlogit x3", grad, K.kd_dlogit(logit, tchr, tgt, tgt_len, SMOOTHING, temp, w, g=3.0)) < 1e-5
    # TokenLevelKdLoss alone
    want, _, _, scale = K.kd_loss(logit, tchr, tgt, tgt_len, 0.0, temp, 0.0)
    got, grad = run(TokenLevelKdLoss(temp))
    assert abs(got - float(want)) <= 2e-5 * float(scale)
    assert rel("kd dlogit x3", grad, K.kd_dlogit(logit, tchr, tgt, tgt_len, 0.0, temp, 0.0, g=3.0)) < 1e-5
    # any other pair is composed through autograd: a summed supervised loss
    composed = SupKdLoss(LabelSmoothingLoss(SMOOTHING, reduction="sum"), TokenLevelKdLoss(temp), w)
    assert not composed.fused()
    _, sup, kd, _ = K.kd_loss(logit, tchr, tgt, tgt_len, SMOOTHING, temp, w)
    rs = K.row_sup(logit, tchr, tgt, tgt_len, SMOOTHING, temp)
    rk = K.row_kd(logit, tchr, tgt, tgt_len, SMOOTHING, temp)
    want = w * count * float(sup) + (1 - w) * float(kd)
    scale = w * float(rs.abs().sum()) + (1 - w) * float(rk.abs().sum()) / count
    dwant = (K.kd_dlogit(logit, tchr, tgt, tgt_len, SMOOTHING, temp, 1.0, g=3.0) * (w * count) +
             K.kd_dlogit(logit, tchr, tgt, tgt_len, SMOOTHING, temp, 0.0, g=3.0) * (1 - w))
    got, grad = run(composed)
    print(f"composed: {got:.6f} vs {want:.6f}")
    assert abs(got - want) <= 2e-5 * scale
    assert rel("composed dlogit x3", grad, dwant) < 1e-5
    # half-precision / strided logits are converted like LabelSmoothingLoss converts its own
    out = {"logit": logit.to(DEV).half(), "tchr_logit": tchr_dev.to(DEV).transpose(0, 1).contiguous().transpose(0, 1),
           "tgt": tgt.to(DEV), "tgt_len": tgt_len}
    assert np.isfinite(float(fused(out)))


# ---- 4. the eval-mode (teacher) forward ------------------------------------------------------------------------------
def _set_dropout(model, p):
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = p
        if isinstance(m, torch.nn.MultiheadAttention):
            m.dropout = p
    if hasattr(model.encoder, "rnn"):
        model.encoder.rnn.network.dropout = p
    else:
        for ly in model.encoder.trm.model.layers:
            ly.self_attn.dropout = p


def _rnn_model(state):
    import audiocaption_amd as A
    model = A.init_model_from_config(A.cnn14rnn_trm_config(V), print_fn=lambda s: None)
    model.load_state_dict(state, strict=True)
    return model.to(DEV)


def _trm_model(state):
    import audiocaption_amd as A
    model = A.init_model_from_config(A.config.cnn14trm_trm_config(V), print_fn=lambda s: None)
    model.load_state_dict(state, strict=True)
    return model.to(DEV)


def _small_batch(seed=5, **extra):
    g = torch.Generator().manual_seed(41)
    hook = torch.rand(3, 8, 2048, generator=g)
    lens = [8, 5, 3]
    cap = torch.randint(4, V, (3, 6), generator=g)
    cap_len = np.array([6, 4, 2])
    cap[:, 0] = 1
    for i, n in enumerate(cap_len.tolist()):
        cap[i, n - 1] = 2
        cap[i, n:] = 0
    d = {"mode": "train", "wav": torch.zeros(3, 320 * 32 * 8, device=DEV), "wav_len": [320 * (32 * n - 1) for n in lens],
         "specaug": False, "cap": cap.to(DEV), "cap_len": cap_len, "ss_ratio": 1, "dropout_seed": seed,
         "_cnn_attn": hook.to(DEV)}
    d.update(extra)
    return d


def _check_eval_forward(make, state, batch):
    from audiocaption_amd.optim import FusedAdam
    teacher = make(state).eval()               # dropout modules keep their p = 0.2: eval mode alone must switch them off
    out = teacher(batch)                       # grad mode on, as a careless caller would
    assert not teacher.training and not teacher.encoder.cnn.training and not teacher.decoder.training
    assert out["logit"].requires_grad is False and out["logit"].grad_fn is None
    eng = teacher._train_engine
    assert eng._saved is None
    with pytest.raises(RuntimeError):
        eng.backward(torch.zeros_like(out["logit"]))
    with pytest.raises(RuntimeError):
        eng.step(batch, FusedAdam([p for p in teacher.parameters() if p.requires_grad], lr=0.0))
    assert all(k[-1] == "eval" for k in eng._states)
    by_hand = make(state).train()
    _set_dropout(by_hand, 0.0)
    by_hand.encoder.cnn.train(False)
    want = by_hand(batch)
    assert all(k[-1] != "eval" for k in by_hand._train_engine._states)
    assert torch.equal(out["logit"], want["logit"].detach())                 # bit-equal
    if "seq" in want:
        assert torch.equal(out["seq"], want["seq"])
    assert want["logit"].requires_grad
    # with dropout left on, the train-mode logits differ: the comparison above can fail
    _set_dropout(by_hand, 0.2)
    assert not torch.equal(out["logit"], by_hand(batch)["logit"].detach())
    return out["logit"]


def test_eval_mode_forward_is_the_dropout_free_train_forward(lib, state4981):
    batch = _small_batch()
    logit = _check_eval_forward(_rnn_model, state4981, batch)
    assert tuple(logit.shape) == (3, 5, V)


def test_eval_mode_forward_of_the_cnn14_trm_captioner(lib):
    import _trm_train_ref as TR
    from audiocaption_amd import procedural as P
    cnn_attn, lens, cap, cap_len, use_cap, seed = TR.step_batch("bench_10s")
    B, Tq = cnn_attn.shape[:2]
    batch = {"mode": "train", "wav": torch.zeros(B, 320 * 32 * Tq, device=DEV),
             "wav_len": [320 * (32 * int(n) - 1) for n in lens], "specaug": False, "cap": cap.to(DEV), "cap_len": cap_len,
             "ss_ratio": 0.85, "_use_cap": use_cap, "dropout_seed": seed, "_cnn_attn": cnn_attn.to(DEV)}
    _check_eval_forward(_trm_model, P.to_torch(P.cnn14trm_trm_state(V)), batch)


# ---- 5. / 6. TrainEngine.step(kd=...) --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def teacher_logits(lib, state4981):
    """The logits of a second model (other decoder weights) in eval mode on the small batch, and a fixed perturbation."""
    from audiocaption_amd import procedural as P
    st = dict(state4981)
    st.update(P.to_torch(P.decoder_state_diverse("greedy", vocab_size=V)))
    teacher = _rnn_model(st).eval()
    with torch.no_grad():
        tl = teacher(_small_batch())["logit"].clone()
    noise = torch.randn(tl.shape, generator=torch.Generator().manual_seed(8)).to(DEV)
    return tl, noise


def _params(model):
    return [p for p in model.parameters() if p.requires_grad]


def _close(name, a, b, tol):
    d = rel(name, a, b)
    assert d <= tol, (name, d, tol)


def _compare_params(ma, mb):
    worst = 0.0
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        if pa.requires_grad:
            d = float((pa.detach() - pb.detach()).abs().max()) / (float(pb.detach().abs().max()) + 1e-30)
            worst = max(worst, d)
            assert d <= TOL_PARAM, (k, d)
    print(f"[parameters after the update] worst {worst:.3e}")


def test_step_with_kd_vs_the_bridge_path(lib, state4981, teacher_logits):
    from audiocaption_amd.kd_loss import SupKdLoss, TokenLevelKdLoss, _launch
    from audiocaption_amd.loss import LabelSmoothingLoss
    from audiocaption_amd.optim import FusedAdam, clip_grad_norm_
    from audiocaption_amd.train import TrainEngine
    tl, _ = teacher_logits
    temp, w = 2.0, 0.4
    batch = _small_batch()
    tgt, tgt_len = batch["cap"][:, 1:], torch.as_tensor(batch["cap_len"]) - 1
    # (a) the reference runner's surface
    ma = _rnn_model(state4981).train()
    opt_a = FusedAdam(_params(ma), lr=1e-3, eps=TRAJ_EPS)
    out = ma(batch)
    loss_a = SupKdLoss(LabelSmoothingLoss(SMOOTHING), TokenLevelKdLoss(temp), w)(
        {"logit": out["logit"], "tchr_logit": tl, "tgt": tgt, "tgt_len": tgt_len})
    parts_a, _, _ = _launch(out["logit"].detach(), tl, tgt.contiguous(), tgt_len.to(device=DEV, dtype=torch.int32), SMOOTHING,
                            temp, w, 0.0, None, 0.0, None)
    loss_a.backward()
    clip = clip_grad_norm_(_params(ma), 1.0, scale_now=False)
    opt_a.step(clip=clip)
    # (b) the fast path on a fresh copy of the same state
    mb = _rnn_model(state4981).train()
    eng = TrainEngine(mb)
    r = eng.step(batch, FusedAdam(_params(mb), lr=1e-3, eps=TRAJ_EPS), smoothing=SMOOTHING,
                 kd={"tchr_logit": tl, "temp": temp, "sup_weight": w}, use_graph=False)
    assert float(r["skipped_updates"]) == 0
    _close("loss", r["loss"], loss_a, TOL_LOSS)
    _close("loss (kernel total)", r["loss"], parts_a[0], TOL_LOSS)
    _close("sup_loss", r["sup_loss"], parts_a[1], TOL_LOSS)
    _close("kd_loss", r["kd_loss"], parts_a[2], TOL_LOSS)
    _close("total_norm", r["total_norm"], clip.total_norm, TOL_NORM)
    _compare_params(mb, ma)
    # and the teacher matters: the label-smoothing step from the same start gives another loss
    mc = _rnn_model(state4981).train()
    r0 = TrainEngine(mc).step(batch, FusedAdam(_params(mc), lr=1e-3, eps=TRAJ_EPS), smoothing=SMOOTHING, use_graph=False)
    assert "kd_loss" not in r0 and abs(float(r0["loss"]) - float(r["loss"])) > 1e-3 * abs(float(r0["loss"]))
    _close("sup_loss vs the label-smoothing step", r["sup_loss"], r0["loss"], TOL_LOSS)


def test_step_with_kd_graph_replay_vs_eager(lib, state4981, teacher_logits):
    from audiocaption_amd.optim import FusedAdam
    from audiocaption_amd.train import TrainEngine
    tl, noise = teacher_logits
    # iteration: 1 eager (first of the shape), 2 capture, 3 temp changes, 4 sup_weight changes, 5 a pure replay of 4's graph
    # on other teacher logits; then a step without kd
    sched = [(2.0, 0.5), (2.0, 0.5), (1.0, 0.5), (1.0, 0.25), (1.0, 0.25)]
    tls = [tl + 0.5 * k * noise for k in range(len(sched))]

    def run(use_graph):
        model = _rnn_model(state4981).train()
        eng = TrainEngine(model, seed=77)
        opt = FusedAdam(_params(model), lr=1e-3, eps=TRAJ_EPS)
        res = []
        for it, (temp, w) in enumerate(sched):
            r = eng.step(_small_batch(seed=100 + it), opt, smoothing=SMOOTHING,
                         kd={"tchr_logit": tls[it], "temp": temp, "sup_weight": w}, use_graph=use_graph)
            res.append([float(r[k]) for k in ("loss", "sup_loss", "kd_loss", "total_norm")])
        # a following step without kd is the plain label-smoothing step again (eagerly: today's launches, untouched)
        r = eng.step(_small_batch(seed=200), opt, smoothing=SMOOTHING, use_graph=use_graph)
        assert "kd_loss" not in r and "sup_loss" not in r
        res.append([float(r["loss"]), float(r["total_norm"])])
        r = eng.step(_small_batch(seed=201), opt, smoothing=SMOOTHING, use_graph=use_graph)      # (replayed: no kd)
        res.append([float(r["loss"]), float(r["total_norm"])])
        assert eng.skipped_updates() == 0 and not eng.gru_timeout()
        if use_graph:
            st = next(iter(eng._states.values()))
            assert st["graphs"]["tail"][1][-1] is None and "fwd0" in st["graphs"]
        return res, model

    eager, me = run(False)
    graph, mg = run(True)
    print("eager", eager, "\ngraph", graph)
    for it, (a, b) in enumerate(zip(eager, graph)):
        for x, y, tol in zip(a, b, (TOL_LOSS, TOL_LOSS, TOL_LOSS, TOL_NORM) if len(a) == 4 else (TOL_LOSS, TOL_NORM)):
            assert abs(x - y) <= tol * abs(x), (it, a, b)
    # the schedule can tell a stale buffer or scalar: every iteration's kd term differs from its neighbours'
    assert all(abs(eager[i][2] - eager[i + 1][2]) > 1e-3 * abs(eager[i][2]) for i in range(len(sched) - 1))
    _compare_params(mg, me)
