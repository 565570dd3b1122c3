"""The attention-GRU restatement (tests/_attn_gru_ref.py) at the length edges of the audio memory, against the reference's
recorded decoder steps (tests/golden/g20_attn_gru_edges.npz: lengths [301, 257, 1, 0, 306] over 301 frames) - ids
identical, values within 1e-4 - and the route coverage of the edge-case table."""
import numpy as np
import pytest
import torch

import _attn_gru_edges as E
import _attn_gru_ref as R


@pytest.fixture(scope="module")
def g20():
    return E.load_g20()


def test_fixture_is_the_recipe(g20):
    assert g20["lens"].tolist() == E.G20["lens"] and int(g20["recipe_seed"]) == E.G20["seed"]
    assert g20["steps"].tolist() == list(E.G20["steps"])
    assert g20["shape"].tolist() == [E.G20_SHAPE[k] for k in E.KEYS]


@torch.no_grad()
@pytest.mark.parametrize("t", E.G20["steps"])
def test_step_at_the_length_edges(g20, t):
    sd, mem, lens, fc, tags = E.g20_inputs()
    h, words = E.g20_step_inputs(sd, t)
    assert t == 0 or float(h.abs().max()) > 0.5
    state, logit, w = R.step(sd, R.input_embed(sd, words, tags, t), h, mem, lens, fc)
    tv, ti = logit.topk(8, dim=1)
    np.testing.assert_array_equal(ti.numpy(), g20[f"t{t}_top_idx"])
    for name, got, want in (("top-8 logits", tv, g20[f"t{t}_top_val"]), ("state", state, g20[f"t{t}_state"]),
                            ("attn_weight", w, g20[f"t{t}_attn_weight"])):
        d = float(np.abs(got.numpy() - want).max())
        print(f"t={t} {name}: max |restatement - fixture| {d:.3e}")
        assert d < 1e-4, name
    assert float(g20[f"t{t}_gap"]) >= 1e-4
    # the reference's own weights, in float64
    ref = g20[f"t{t}_attn_weight"].astype(np.float64)
    Tm = E.G20["Tm"]
    # length 0: every score is -1e10, the softmax is uniform - each weight the same f32, one rounding from 1 / Tm
    assert (ref[3] == ref[3, 0]).all(), "the length-0 row is not uniform"
    assert abs(ref[3, 0] - 1.0 / Tm) <= np.spacing(np.float32(1.0 / Tm)), ref[3, 0]
    # length 306 > Tm masks nothing: the row equals the length-301 row of the same memory and state
    np.testing.assert_array_equal(ref[4], ref[0])
    assert not ref[1, 257:].any() and not ref[2, 1:].any() and ref[2, 0] == 1.0 and ref[0].min() > 0
    for i in range(5):
        assert abs(ref[i].sum() - 1.0) <= 2 * Tm * 2.0 ** -24


def test_case_table_reaches_every_gemm_route():
    """At least one decoder GEMM of the edge cases goes down each of ac_gemm's four kernels; the key projection reaches
    both nt kernels (the mirror of the dispatch, _attn_gru_edges.gemm_route, produces no expected values)."""
    print("\n".join(E.route_table()))
    E.assert_route_coverage()
