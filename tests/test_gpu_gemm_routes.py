"""Every kernel ``ac_gemm`` and ``ac_gemm_bf16x3`` (csrc/train.hip) can dispatch to, called through the C ABI at the
smallest shapes that reach it (tests/_gemm_routes.py: the dispatch restated, the case list, and one case for every
(route, N, K, bias, beta) the HTS-AT encoder reaches at 1, 2, 3, 8 and 64 clips) against float64.

Per case:
* guards: the output is a view with ldc = N + 8 of a buffer with three extra rows, pre-filled with 7.0; the pad columns and
  the extra rows keep their bits;
* exact-f32 routes (general, kk, nt<1>, nt<2>): within 1e-5 of the largest float64 output, the bar of
  tests/test_gpu_train.py::test_general_gemm_all_layouts;
* split-bf16 routes (bf16x3 64 x 64 and 128 x 128 tiles): within 3e-5 of the largest float64 output, and the predicted-error
  criterion of tests/_split_ref.py (``S.verdict``: the kernel's error against the CPU emulation of hi/lo-split operands with
  hi*hi + hi*lo + lo*hi products) on both of its input families.  A residual (beta = 1) is added to the exact and to the
  emulated output alike.

Which kernel ran is not visible from the result; tests/test_gemm_routes_cpu.py pins the restated dispatch and
tests/golden/REPORT_gemm_routes.txt records the kernel names a kernel trace of this file observed, with the measured
ratios."""
import ctypes

import pytest
import torch

import _gemm_routes as G
import _split_ref as S

pytestmark = pytest.mark.gpu

EXACT_BAR, SPLIT_BAR = 1e-5, 3e-5


@pytest.fixture(scope="module")
def lib():
    from audiocaption_amd import _lib, build
    build.build()
    return _lib.load()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def reference(c):
    """(x, w, b, res, exact, split case or None) of a case, on the CPU."""
    seed = 11 + (c.M * 7 + c.N * 5 + c.K * 3 + int(c.has_bias) + 2 * int(c.beta)) % 100003
    x, w, b = S.draw_linear(c.family, c.M, c.N, c.K, seed)
    if not c.has_bias:
        b = None
    res = torch.randn(c.M, c.N, generator=torch.Generator().manual_seed(seed + 1)) if c.beta else None
    if c.route in G.EXACT:
        exact = x.double() @ w.double().t()
        if b is not None:
            exact += b.double()
        if res is not None:
            exact += res.double()
        return x, w, b, res, exact, None
    case = S.linear(x, w, b)
    if res is not None:
        case.exact = case.exact + res.double()
        case.emul = (case.emul.double() + res.double()).float()     # one f32 rounding, as ``v += beta * *c``
    return x, w, b, res, case.exact, case


@pytest.mark.parametrize("c", G.CASES, ids=[G.case_id(c) for c in G.CASES])
def test_gemm_route(lib, c):
    assert G.route(c.entry, c.M, c.N, c.K) == c.route
    x, w, b, res, exact, case = reference(c)
    M, N, K = c.M, c.N, c.K
    ldc = N + 8
    buf = torch.full((M + 3, ldc), 7.0)
    if res is not None:
        buf[:M, :N] = res
    xd, wd, bd, out = x.cuda(), w.cuda(), (b.cuda() if b is not None else None), buf.cuda()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = getattr(lib, c.entry)(_ptr(xd), K, 1, _ptr(wd), 1, K, _ptr(out), ldc, M, N, K, _ptr(bd), 0, c.beta, 1, 0.0, 0, None, 0,
                               None, 0, stream)
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu()
    seven = torch.full((), 7.0)
    assert torch.equal(got[:, N:], seven.expand(M + 3, 8)), "the pad columns keep their bits"
    assert torch.equal(got[M:], seven.expand(3, ldc)), "the rows beyond M keep their bits"
    got = got[:M, :N]
    assert bool(torch.isfinite(got).all())
    name = f"{G.case_id(c)} [{c.family}]"
    d = float((got.double() - exact).abs().max()) / float(exact.abs().max())
    if case is None:
        S.report(f"gpu {name}: max|diff| / max|want| {d:.3e}")
        assert d < EXACT_BAR, name
        return
    fig = S.figures(got, case)
    S.report(S.fmt_figures(f"gpu {name}: max|diff| / max|want| {d:.3e}", fig))
    assert d < SPLIT_BAR, name
    assert S.verdict(fig) == [], (name, S.verdict(fig))
