"""How varied a set of captions is, on the device (csrc/diversity.hip): the numbers of the reference's diversity
evaluation - ``eval/diversity.py`` (vocabulary size, % novel sentences, Distinct-1, Distinct-2, Self-BLEU),
``eval/diversity_instance.py`` (Distinct-n per sentence) and ``eval/old_diversity.py`` (the n-gram richness) - built in.
Unlike ``Cider``, ``Bleu`` and ``Rouge`` it takes no references: every caption of the set is scored against all the others.

``Diversity()`` offers two routes onto the same kernels:

* ``score_ids(vocabulary, vocab_size, words, start_idx, end_idx)`` on decoded word ids, one (N, T) tensor or a list of
  them (the samples of several decodes) pooled into one corpus; the results stay on the device and nothing is synchronised.
* ``compute_score(hypothesis, train_captions=None)`` on strings, ``{key: [sentence, ...]}`` or a list of sentences, all
  pooled as diversity.py pools a prediction with several captions; a plain dict of Python numbers comes back.

Self-BLEU is nltk's ``sentence_bleu(all other sentences, sentence, weights=(.25, .25, .25, .25),
smoothing_function=SmoothingFunction().method1)`` averaged over the sentences; the arithmetic is stated with the prototype
in include/audiocaption_hip.h.  Distinct-2 divides by the number of WORDS, as diversity.py does.  The instance means divide
by a sentence's own unigrams and bigrams; where the reference divides by zero (a sentence without a bigram) they raise
ValueError.  The sentence rule and the canonical-id table are those of cider.py.

Not built: Self-BLEU within groups (the samples of one clip), mBLEU, clap_score.py and specificity.py.
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .cider import MAX_HYP_WORDS, PackedScorer

MAX_TOTAL_WORDS = 1 << 26     # N * T, the bound of ac_diversity_scores


def _refuse_without_bigram(length, sentences=None):
    short = np.flatnonzero(length < 2)
    if short.size:
        i = int(short[0])
        text = f" ({sentences[i]!r})" if sentences is not None else ""
        raise ValueError(f"Diversity: sentence {i}{text} has {int(length[i])} word(s) and so no bigram: Distinct-n per "
                         f"sentence divides by a sentence's bigrams")


def instance_means(stats, sent_distinct, sentences=None):
    """diversity_instance.py:80-92 from the integers of a call: ``(mean of distinct unigrams / unigrams, mean of distinct
    bigrams / bigrams)`` over the sentences.  A sentence with fewer than two words has no bigram (the reference divides
    by zero there): ValueError naming the first such sentence."""
    length = np.asarray(stats, dtype=np.int64)[:, 0]
    distinct = np.asarray(sent_distinct, dtype=np.int64)
    _refuse_without_bigram(length, sentences)
    return float(np.mean(distinct[:, 0] / length)), float(np.mean(distinct[:, 1] / (length - 1)))


def novel_share(sentences, train_captions):
    """The share of ``sentences`` that are not among ``train_captions`` (diversity.py:73-74, 91): a set lookup of the whole
    string on the host."""
    train = train_captions if isinstance(train_captions, (set, frozenset)) else set(train_captions)
    return sum(s not in train for s in sentences) / len(sentences)


class Diversity(PackedScorer):
    """``score_ids`` returns ``{"self_bleu": (N,) f64, "stats": (N, 10) int32 = L, ref_len, den[4], num[4] per sentence,
    "sent_distinct": (N, 4) int32, "totals": (5,) int32 = total words, distinct n-grams for n = 1 .. 4, "summary": (6,) f64 =
    mean Self-BLEU, richness per order, richness}``.  A word id outside the vocabulary before a row's ``end_idx`` makes every
    float NaN and every integer -1 (ids held on the host are refused instead)."""
    _who = "Diversity"

    def __init__(self):
        self._workspace = None
        self.clear_cache()

    # ---- the kernels ---------------------------------------------------------------------------------------------
    @staticmethod
    def _check_sizes(N, T):
        if N < 2:
            raise ValueError(f"Diversity: {N} sentence(s): Self-BLEU scores a sentence against all the others, and with "
                             f"fewer than two there is no other length for nltk's closest_ref_length to choose from")
        if T > MAX_HYP_WORDS:
            raise ValueError(f"Diversity: sentences of {T} words; the kernels take {MAX_HYP_WORDS}")
        if N * max(T, 1) > MAX_TOTAL_WORDS:
            raise ValueError(f"Diversity: {N} rows of {T} words; the kernels take {MAX_TOTAL_WORDS} words in all")

    def score_rows(self, rows, start_idx, end_idx, canon, vocab_size):
        """The dict of ``score_ids`` for one int32 plane ``rows`` (N, T) on the device of ``canon``."""
        lib = _lib.load()
        dev = canon.device
        N, T = rows.shape
        self._check_sizes(N, T)
        if T == 0:
            rows = rows.new_full((N, 1), int(end_idx))
            T = 1
        if rows.stride(1) != 1:
            rows = rows.contiguous()
        need = lib.ac_diversity_workspace_bytes(N, T)
        if need < 0:
            raise _lib.HipLibraryError(f"ac_diversity_workspace_bytes refused ({N} rows of {T} words)")
        workspace = self._workspace_of(need, dev)
        out = {"self_bleu": torch.empty(N, device=dev, dtype=torch.float64),
               "stats": torch.empty(N, 10, device=dev, dtype=torch.int32),
               "sent_distinct": torch.empty(N, 4, device=dev, dtype=torch.int32),
               "totals": torch.empty(5, device=dev, dtype=torch.int32),
               "summary": torch.empty(6, device=dev, dtype=torch.float64)}
        check(lib.ac_diversity_scores(ptr(rows), rows.stride(0), N, T, int(start_idx), int(end_idx), ptr(canon),
                                      int(vocab_size), ptr(workspace), workspace.numel(), ptr(out["stats"]),
                                      ptr(out["sent_distinct"]), ptr(out["totals"]), ptr(out["self_bleu"]),
                                      ptr(out["summary"]), stream()), "ac_diversity_scores")
        return out

    # ---- word ids ------------------------------------------------------------------------------------------------
    def score_ids(self, vocabulary, vocab_size, words, start_idx, end_idx):
        vocab_size = int(vocab_size)
        self._canon(vocabulary, vocab_size)   # (a vocabulary that cannot be used is refused first)
        planes = [torch.as_tensor(w) for w in (words if isinstance(words, (list, tuple)) else [words])]
        if not planes or any(w.dim() != 2 for w in planes):
            raise ValueError(f"Diversity: words must be (N, T) tensors of word ids, got "
                             f"{[tuple(w.shape) for w in planes]}")
        T = max(w.shape[1] for w in planes)
        self._check_sizes(sum(w.shape[0] for w in planes), T)
        for w in planes:
            self._refuse_foreign_ids(w, vocab_size, start_idx, end_idx)
        dev = self._device_of(planes)
        canon_dev = self._canon(vocabulary, vocab_size, dev)
        planes = [w.to(device=dev, dtype=torch.int32) for w in planes]
        # rows of a shorter plane end where they end: filled up with end_idx
        planes = [w if w.shape[1] == T else torch.nn.functional.pad(w, (0, T - w.shape[1]), value=int(end_idx))
                  for w in planes]
        rows = planes[0] if len(planes) == 1 else torch.cat(planes, dim=0)
        return self.score_rows(rows, start_idx, end_idx, canon_dev, vocab_size)

    # ---- strings -------------------------------------------------------------------------------------------------
    @staticmethod
    def _sentences(hypothesis):
        if isinstance(hypothesis, dict):
            groups = hypothesis.values()
            if any(isinstance(g, str) for g in groups):
                raise ValueError("Diversity.compute_score: {key: [sentence, ...]} or a list of sentences")
            return [s for g in groups for s in g]
        return list(hypothesis)

    def _pack_sentences(self, sentences):
        """``(rows int32 (N, T) padded with end_idx, start_idx, end_idx, vocab_size)``: the words numbered through a
        table private to the call."""
        end_idx, start_idx, first_word = 0, 1, 2
        table = {}
        ids = [[table.setdefault(w, first_word + len(table)) for w in s.split()] for s in sentences]
        T = max(1, max((len(s) for s in ids), default=0))
        self._check_sizes(len(ids), T)
        rows = np.full((len(ids), T), end_idx, dtype=np.int32)
        for row, s in zip(rows, ids):
            row[:len(s)] = s
        return rows, start_idx, end_idx, first_word + len(table)

    def _score_strings(self, sentences):
        rows, start_idx, end_idx, vocab_size = self._pack_sentences(sentences)
        canon = torch.arange(vocab_size, device="cuda", dtype=torch.int32)
        return self.score_rows(torch.from_numpy(rows).to(canon.device), start_idx, end_idx, canon, vocab_size)

    def compute_score(self, hypothesis, train_captions=None, instance=True):
        """``{"vocabulary", "distinct_1", "distinct_2", "self_bleu", "richness", "distinct_1_instance",
        "distinct_2_instance"[, "novel"]}`` for all sentences of ``hypothesis`` pooled.  ``novel`` (the share of sentences
        not in ``train_captions``, any container of strings) only when ``train_captions`` is given.  The instance means
        raise ValueError for a set with a sentence of fewer than two words; ``instance=False`` leaves them out."""
        sentences = self._sentences(hypothesis)
        if any(not isinstance(s, str) for s in sentences):
            raise ValueError("Diversity.compute_score: sentences must be strings")
        if instance:          # (before any launch)
            _refuse_without_bigram(np.array([len(t.split()) for t in sentences], dtype=np.int64), sentences)
        out = self._score_strings(sentences)
        totals = out["totals"].cpu().tolist()
        summary = out["summary"].cpu().tolist()
        words = totals[0]
        result = {"vocabulary": totals[1],
                  "distinct_1": totals[1] / words if words else float("nan"),
                  "distinct_2": totals[2] / words if words else float("nan"),
                  "self_bleu": summary[0], "richness": summary[5]}
        if instance:
            d1, d2 = instance_means(out["stats"].cpu().numpy(), out["sent_distinct"].cpu().numpy(), sentences)
            result["distinct_1_instance"], result["distinct_2_instance"] = d1, d2
        if train_captions is not None:
            result["novel"] = novel_share(sentences, train_captions)
        return result
