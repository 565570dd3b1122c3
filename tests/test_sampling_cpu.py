"""CPU tests of caption sampling: the Philox generator, the numpy restatement of the sampler's rules against the reference's
sample_next_word (g14_sampling.npz), method-string parsing, the refusals that stay, and the two new C symbols."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _sampling_ref as S
from audiocaption_amd import _lib
from audiocaption_amd import sampling as SM

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ctr,key,want", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    got = S.philox4x32_10(np.array(ctr), np.array(key))
    assert " ".join(f"{int(v):08x}" for v in got) == want


def test_uniform_range_and_layout():
    u = S.uniform(0x0123456789abcdef, 7, np.arange(4096))
    assert u.min() > 0 and u.max() <= 1 and len(np.unique(u)) > 4000
    assert np.all(u * 2 ** 24 == np.round(u * 2 ** 24))                  # 24-bit grid
    assert S.uniform(5, 3, np.array([9]))[0] == S.uniform(5, 3, np.arange(12))[9]   # a row's draw ignores its batch
    assert S.uniform(5, 3, np.array([9]))[0] != S.uniform(6, 3, np.array([9]))[0]


def _g14():
    return np.load(os.path.join(REPO, "tests", "golden", "g14_sampling.npz"))


def _rule(method, temp, V):
    code, k, p, t = SM.parse_sample_method(str(method), V, float(temp))
    return code, k, p, t


def test_restated_rules_match_the_reference_distribution():
    """The kept set, the distribution and the stored value of the restatement equal what the reference computed."""
    g = _g14()
    logits = g["logits"]
    V = logits.shape[1]
    for mi, (method, temp) in enumerate(zip(g["methods"], g["temps"])):
        code, k, p, t = _rule(method, temp, V)
        for r in range(logits.shape[0]):
            w, stored, amb = S.distribution(logits[r], code, k, p, t, set_tol=1e-6)
            assert not amb, f"{method} row {r}: fixture row too close to the top-p boundary"
            want = torch.softmax(torch.from_numpy(g["dist_logits"][mi, r]).double(), 0).numpy()
            got = w / w.sum()
            assert np.abs(got - want).max() < 1e-6, f"{method} row {r}"
            assert np.array_equal(got > 0, want > 0), f"{method} row {r}: kept set differs"
            wd = int(g["word"][mi, r])
            assert got[wd] > 0, f"{method} row {r}: the reference drew a word outside the kept set"
            assert abs(stored[wd] - float(g["probs"][mi, r])) < 1e-5, f"{method} row {r}"


def test_fixture_covers_ties_and_peaks():
    g = _g14()
    x = g["logits"]
    V = x.shape[1]
    # exact ties at the 5th / 50th place keep the lower index (torch leaves it open: the fixture rows are built so
    # that its choice and the rule agree, checked through the kept sets above)
    o = S.rank_order(x[3].astype(np.float64))
    assert x[3][o[4]] == x[3][o[5]] and o[4] < o[5]
    w, _, _ = S.distribution(x[2], S.TOPP, p=0.9)
    assert np.count_nonzero(w) == 1                                     # peaked: the nucleus is one word
    w, _, _ = S.distribution(x[7], S.TOPK, k=1)
    assert np.flatnonzero(w).tolist() == [10]                           # three equal maxima: the lowest index
    assert V == 4981


def test_draw_is_inverse_cdf_in_index_order():
    w = np.array([0.0, 1.0, 0.0, 2.0, 1.0])
    assert S.draw(w, 0.25, 0)[0] == 1
    assert S.draw(w, 0.2500001, 0)[0] == 3
    assert S.draw(w, 0.75, 0)[0] == 3
    assert S.draw(w, 1.0, 0)[0] == 4
    assert S.draw(w, 0.25, 1e-3)[1] == {1, 3}


@pytest.mark.parametrize("name,want", [
    ("sample", (SM.PLAIN, 0, 0.0, 0.7)), ("anything", (SM.PLAIN, 0, 0.0, 0.7)),
    ("top5", (SM.TOPK, 5, 0.0, 0.7)), ("top1.7", (SM.TOPK, 1, 0.0, 0.7)), ("top1", (SM.TOPK, 1, 0.0, 0.7)),
    ("top4981", (SM.TOPK, 4981, 0.0, 0.7)), ("top0.9", (SM.TOPP, 0, 0.9, 1.0)), ("top.5", (SM.TOPP, 0, 0.5, 1.0)),
    ("gumbel", (SM.GUMBEL, 0, 0.0, 1.0)),
])
def test_method_parsing(name, want):
    assert SM.parse_sample_method(name, 4981, 0.7) == want


@pytest.mark.parametrize("name,temp", [
    ("top0", 1.0), ("top-3", 1.0), ("top4982", 1.0), ("topx", 1.0), ("top", 1.0), ("topnan", 1.0), ("topinf", 1.0),
    ("sample", 0.0), ("sample", -1.0), ("top5", 0.0), ("sample", float("inf")),
])
def test_method_parsing_rejects(name, temp):
    with pytest.raises(ValueError):
        SM.parse_sample_method(name, 4981, temp)


def test_top_p_and_gumbel_ignore_temp():
    assert SM.parse_sample_method("top0.9", 100, -5.0)[3] == 1.0
    assert SM.parse_sample_method("gumbel", 100, 0.0)[3] == 1.0
    assert SM.parse_sample_method("top0.99999999999", 100)[2] < 1.0   # kept below 1 in f32


def test_seed_word_and_draw():
    assert SM.seed_word(0) == 0 and SM.seed_word(2 ** 63) == -2 ** 63 and SM.seed_word(2 ** 64 - 1) == -1
    with pytest.raises(ValueError):
        SM.seed_word(2 ** 64)
    torch.manual_seed(3)
    a = SM.draw_seed()
    torch.manual_seed(3)
    assert SM.draw_seed() == a and 0 <= a < 2 ** 64


def _tiny_model():
    import audiocaption_amd as A
    return A.init_model_from_config(A.cnn14rnn_trm_config(100), print_fn=lambda s: None)


def test_dbs_and_forward_async_still_refuse():
    m = _tiny_model()
    with pytest.raises(NotImplementedError):
        m.inference_forward({"sample_method": "dbs"})
    with pytest.raises(NotImplementedError):
        m.forward_async({"mode": "inference", "sample_method": "top5", "wav": torch.zeros(1, 32000)})


def test_sampling_reaches_the_sampler_and_validates_first():
    """A sampling method is no longer refused: invalid names raise ValueError before any device work."""
    m = _tiny_model()
    with pytest.raises(ValueError):
        m.inference_forward({"sample_method": "top0", "temp": 1.0, "max_length": 5})
    with pytest.raises(ValueError):
        m.inference_forward({"sample_method": "sample", "temp": 0.0, "max_length": 5})


def test_sampling_symbols_in_header_and_ctypes_table():
    header = open(os.path.join(REPO, "include", "audiocaption_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("ac_sample_rows", "ac_trm_sample"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["ac_sample_rows"][1][8] is ctypes.c_void_p           # seed_dev: a device pointer
    greedy = _lib.SIGNATURES["ac_trm_greedy"][1]
    samp = _lib.SIGNATURES["ac_trm_sample"][1]
    assert samp[:15] == greedy[:15] and samp[-1] == greedy[-1]                     # ac_trm_greedy's arguments ...
    assert samp[15:20] == [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_void_p]   # ... plus these
    for code, name in ((SM.PLAIN, "PLAIN"), (SM.TOPK, "TOPK"), (SM.TOPP, "TOPP"), (SM.GUMBEL, "GUMBEL")):
        assert re.search(rf"#define AC_SAMPLE_{name} {code}\b", header)


def test_sampling_symbols_exported_and_validate_arguments():
    if not os.path.exists(_lib.LIB_PATH):
        from audiocaption_amd import build
        build.build()
    lib = _lib.load()
    for name in ("ac_sample_rows", "ac_trm_sample"):
        assert getattr(lib, name) is not None
    # rejected before any HIP call
    assert lib.ac_sample_rows(None, 4981, 4, 4981, 0, 0, 0.0, 1.0, None, 0, None, None, None) == -1
    dummy = ctypes.c_void_p(16)
    assert lib.ac_sample_rows(dummy, 4981, 4, 4981, 1, 0, 0.0, 1.0, dummy, 0, dummy, dummy, None) == -1      # k = 0
    assert lib.ac_sample_rows(dummy, 4981, 4, 4981, 1, 4982, 0.0, 1.0, dummy, 0, dummy, dummy, None) == -1   # k > V
    assert lib.ac_sample_rows(dummy, 4981, 4, 4981, 2, 0, 1.0, 1.0, dummy, 0, dummy, dummy, None) == -1      # p = 1
    assert lib.ac_sample_rows(dummy, 4981, 4, 4981, 0, 0, 0.0, 0.0, dummy, 0, dummy, dummy, None) == -1      # temp 0
    assert lib.ac_sample_rows(dummy, 4981, 4, 4981, 7, 0, 0.0, 1.0, dummy, 0, dummy, dummy, None) == -1      # method
    assert lib.ac_sample_rows(dummy, 20000, 4, 20000, 0, 0, 0.0, 1.0, dummy, 0, dummy, dummy, None) == -1    # V > 16384
    w = _lib.AcTrmWeights()
    assert lib.ac_trm_sample(ctypes.byref(w), None, None, 1, 1, 1, 1, 2, 0, None, None, None, None, None, None,
                             0, 0, 0.0, 1.0, None, None) == -1
