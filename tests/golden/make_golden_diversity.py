"""Generate g25_diversity.npz by running the REFERENCE's n-gram richness (python_scripts/eval/old_diversity.py:
calc_richness :10-42, diversity_evaluate :45-60) on the corpora of the diversity tests (tests/_diversity_ref.py CASES).

Run in the build container only (the reference never travels to the GPU box):

    python tests/golden/make_golden_diversity.py

``old_diversity.py`` is imported by file path under inert stubs for ``fire`` and ``pandas``; it reads its captions through
``iterrows()``, ``["tokens"].values`` and ``shape`` only, so a small duck-typed frame whose tokens are word lists stands in
for the DataFrame.  Stored, per corpus: the reference's ``calc_richness`` for n = 1 .. 4 and its ``diversity_evaluate``
(NaN where the reference divides by zero because no sentence has an n-gram of that order).  The fixture holds these
numbers and the corpus names, nothing else.  The CPU restatement tests/_diversity_ref.py is compared with the reference
here as well, to 1e-12 relative: it repeats the reference's operations, and the order of a sum over a set is not fixed.

What is the reference's own and what is not: only the richness is reference-pinned.  Self-BLEU needs nltk, which is not
available; it rests on the restatement of nltk's published algorithm and on the closed forms of
tests/test_diversity_cpu.py.  The distinct n-gram counts are integers restated from diversity.py:49-96.
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np


class Frame:
    """What old_diversity.py reads of a DataFrame with a ``tokens`` column."""

    class _Column:
        def __init__(self, values):
            self.values = values

    def __init__(self, tokens):
        self._tokens = list(tokens)
        self.shape = (len(self._tokens), 1)

    def iterrows(self):
        return ((i, {"tokens": t}) for i, t in enumerate(self._tokens))

    def __getitem__(self, name):
        assert name == "tokens"
        return Frame._Column(self._tokens)


def _install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m

    mod("fire", Fire=lambda *a, **k: None)
    mod("pandas", DataFrame=Frame)


def close(got, want):
    """NaN where the reference has none, else within 1e-12 relative: both sum a sentence's terms in the iteration order
    of a set of word tuples, which differs between the two and from run to run."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.array_equal(np.isnan(got), np.isnan(want)) and bool(np.all(np.isnan(want) | (np.abs(got - want) <= 1e-12 * np.abs(want))))


def main():
    _install_stubs()
    import _diversity_ref as D
    spec = importlib.util.spec_from_file_location("ref_old_diversity", os.path.join(REF, "python_scripts/eval/old_diversity.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    per_order = np.full((len(D.CASES), D.ORDER), np.nan, dtype=np.float64)
    overall = np.full(len(D.CASES), np.nan, dtype=np.float64)
    for c, name in enumerate(D.CASES):
        sentences = D.make_case(name)["sentences"]
        frame = Frame(sentences)
        for n in range(D.ORDER):
            try:
                per_order[c, n] = ref.calc_richness(frame, n + 1)
            except ZeroDivisionError:       # no sentence has an n-gram of this order
                pass
        try:
            overall[c] = ref.diversity_evaluate(frame, N=D.ORDER)
        except ZeroDivisionError:
            pass
        mine_each, mine = D.richness(sentences)
        assert close(mine_each, per_order[c]), (name, mine_each, per_order[c])
        assert close(mine, overall[c]), (name, mine, overall[c])
        print(f"{name}: {len(sentences)} sentences, richness {per_order[c].tolist()} overall {overall[c]}")
    closed = D.CASES.index("captions")
    assert np.allclose(per_order[closed], D.CLOSED_CAPTIONS["richness"], rtol=1e-12, atol=0)
    assert abs(overall[closed] - D.CLOSED_CAPTIONS["overall"]) < 1e-12

    path = os.path.join(HERE, "g25_diversity.npz")
    np.savez_compressed(path, cases=np.array(D.CASES), richness_per_order=per_order, richness=overall)
    size = os.path.getsize(path)
    assert size <= 100000, size
    print(f"wrote {path}: {size} bytes")


if __name__ == "__main__":
    main()
