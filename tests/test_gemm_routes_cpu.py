"""tests/_gemm_routes.py on the CPU: the restated dispatch of ``ac_gemm`` / ``ac_gemm_bf16x3`` at the shapes whose routes
are known from the sources, the route of every linear layer of the HTS-AT encoder at 1, 2, 3, 8 and 64 clips, and the
coverage of the GPU case list (tests/test_gpu_gemm_routes.py) over those routes."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gemm_routes as G  # noqa: E402

KK, NT1, B64, B128 = "kk", "nt1", "bf16x3_64", "bf16x3_128"


def _stage(qkv, proj, fc1, fc2, red=None):
    return dict(qkv=qkv, proj=proj, fc1=fc1, fc2=fc2, **({} if red is None else {"red": red}))


ALL_KK, ALL_KK3 = _stage(KK, KK, KK, KK, KK), _stage(KK, KK, KK, KK)
# batch -> per stage, the route of qkv (3C, C), proj (C, C), fc1 (4C, C), fc2 (C, 4C) and the merge reduction (2C, 4C)
TABLE = {
    1: [_stage(B64, NT1, B64, KK, KK), ALL_KK, ALL_KK, ALL_KK3],
    2: [_stage(B64, B64, B64, B64, KK), _stage(B64, KK, B64, KK, KK), ALL_KK, ALL_KK3],
    3: [_stage(B64, B64, B64, B64, KK), _stage(B64, KK, B64, KK, KK), _stage(B64, KK, B64, KK, KK), ALL_KK3],
    8: [_stage(B128, B64, B128, B64, B64), _stage(B64, B64, B64, B64, KK), _stage(B64, KK, B64, KK, KK), _stage(B64, KK, B64, KK)],
    64: [_stage(B128, B128, B128, B128, B128), _stage(B128, B128, B128, B128, B64), _stage(B128, B64, B128, B64, B64),
         _stage(B128, B64, B128, B64)],
}


@pytest.mark.parametrize("B", sorted(TABLE))
def test_htsat_route_table(B):
    calls = G.htsat_linear_calls(B)
    assert len(calls) == 4 * 12 + 3
    seen = [{} for _ in range(4)]
    for name, M, N, K, has_bias, beta in calls:
        s, layer = int(name[1]), name.rsplit(".", 1)[1]
        C, H = 96 << s, 64 >> s
        assert (N, K) == {"qkv": (3 * C, C), "proj": (C, C), "fc1": (4 * C, C), "fc2": (C, 4 * C), "red": (2 * C, 4 * C)}[layer]
        assert M == (B * H * H // 4 if layer == "red" else B * H * H)
        assert has_bias == (layer != "red") and beta == (1.0 if layer in ("proj", "fc2") else 0.0)
        rt = G.route("ac_gemm_bf16x3", M, N, K)
        assert seen[s].setdefault(layer, rt) == rt          # every block of a stage takes the same routes
    assert seen == TABLE[B]


def test_call_order_of_one_block_and_merge():
    calls = G.htsat_linear_calls(2, depths=(1, 1, 1, 1))
    assert [c[0] for c in calls[:6]] == ["s0.b0.qkv", "s0.b0.proj", "s0.b0.fc1", "s0.b0.fc2", "s0.red", "s1.b0.qkv"]
    assert calls[0][1:] == (8192, 288, 96, True, 0.0) and calls[1][1:] == (8192, 96, 96, True, 1.0)
    assert calls[3][1:] == (8192, 96, 384, True, 1.0) and calls[4][1:] == (2048, 192, 384, False, 0.0)
    assert calls[-1][0] == "s3.b0.fc2" and len(calls) == 19


def test_gpu_cases_reach_their_routes_and_cover_the_table():
    for c in G.CASES:
        assert G.route(c.entry, c.M, c.N, c.K) == c.route, c
    assert len({G.case_id(c) for c in G.CASES}) == len(G.CASES)
    have = {(c.route, c.N, c.K, c.has_bias, c.beta) for c in G.CASES}
    missing = G.htsat_route_keys((1, 2, 3, 8, 64)) - have
    assert not missing, sorted(missing)
    assert {c.route for c in G.CASES} == set(G.ROUTES) - {"general"}      # general: test_general_gemm_all_layouts
    for rt in ("bf16x3_64", "bf16x3_128"):                                 # both input families on both split-bf16 tiles
        assert {c.family for c in G.CASES if c.route == rt} == {"randn", "checkpoint-like"}
    # the shapes the first list names
    named = {("kk", 50, 768, 3072), ("nt1", 4096, 96, 96), ("nt1", 4069, 96, 96), ("nt2", 16389, 512, 100),
             ("nt1", 32768, 96, 16), ("nt2", 32768, 144, 24), ("bf16x3_64", 8165, 96, 96), ("bf16x3_128", 19109, 288, 96),
             ("bf16x3_128", 57253, 96, 96), ("bf16x3_128", 57253, 96, 384), ("bf16x3_128", 28581, 192, 384)}
    assert named <= {(c.route, c.M, c.N, c.K) for c in G.CASES}


def test_route_on_layouts_the_existing_tests_use():
    r = G.route
    assert r("ac_gemm", 150, 200, 330) == "general"                                   # K % 32 != 0, 12 tiles
    for M, N, K in [(1344, 768, 256), (7392, 256, 1024), (4100, 260, 776)]:
        assert r("ac_gemm_bf16x3", M, N, K) == "bf16x3_64"
    assert r("ac_gemm_bf16x3", 520, 1024, 512) == "kk"                                # 144 tiles of 64 x 64: forwarded
    # dy w: A (M, N) k-fast, B = w (N, K) read as (k = n, n = k): contiguous along its rows
    assert r("ac_gemm_bf16x3", 7392, 256, 1024, sam=1024, sak=1, sbk=256, sbn=1) == "bf16x3_64"
    assert r("ac_gemm", 7392, 256, 1024, sam=1024, sak=1, sbk=256, sbn=1) == "general"
    # rows of 4981 floats are not 16-byte aligned: forwarded, and not an x w^T kernel either
    assert r("ac_gemm_bf16x3", 672, 256, 4981, sam=4981, sak=1, sbk=256, sbn=1) == "general"
    assert r("ac_gemm_bf16x3", 8192, 288, 96, a_aligned=False) == "general"
    assert r("ac_gemm_bf16x3", 8192, 288, 96, b_aligned=False) == "general"
    # split-K counts as tiles and never takes the K-quarter kernel; a gate keeps the K-quarter kernel out as well
    assert r("ac_gemm", 256, 256, 4096) == "kk" and r("ac_gemm", 256, 256, 4096, splitk=8) == "nt1"
    assert r("ac_gemm", 256, 256, 4096, a_scale=True) == "general"
    assert r("ac_gemm_bf16x3", 8192, 288, 96, a_scale=True) == "bf16x3_64"
    assert r("ac_gemm_bf16x3", 8192, 288, 96, a_scale=True, a_scale_aligned=False) == "general"
    # thresholds: 3e7 products, 200 64 x 64 tiles, 448 128 x 128 tiles
    assert r("ac_gemm_bf16x3", 6400, 128, 96) == "bf16x3_64" and r("ac_gemm_bf16x3", 6336, 128, 96) == "nt1"
    assert r("ac_gemm_bf16x3", 57344, 96, 96) == "bf16x3_128" and r("ac_gemm_bf16x3", 57345, 96, 96) == "bf16x3_128"
    assert r("ac_gemm_bf16x3", 57216, 96, 96) == "bf16x3_64"
    assert r("ac_gemm", 16384, 512, 96) == "nt2" and r("ac_gemm", 16256, 512, 96) == "nt1"
