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

Within groups - the evaluation of SEVERAL captions per clip, each clip's captions scored against each other only:

* ``score_groups(vocabulary, vocab_size, words, start_idx, end_idx, group_off=None)`` on word ids, ``(B, S, T)`` (the groups
  are the clips: ``TransformerModel``'s ``seq_dev`` under ``n_samples``, taken where it lies) or ``(N, T)`` with explicit
  row offsets ``group_off`` (ragged groups); the results stay on the device.
* ``compute_group_score({key: [sentence, ...]})`` on strings: mBLEU-1..4 (nltk's ``sentence_bleu`` of a caption against its
  clip's other captions with uniform weights over the orders 1..n, method1), Self-BLEU (= mBLEU-4) and div-1 / div-2
  (distinct n-grams of a clip's captions / their words) as means over the clips, plus the per-key values.

Not built: richness within groups, clap_score.py and specificity.py.
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

    def score_group_rows(self, rows, group_off, start_idx, end_idx, canon, vocab_size):
        """The dict of ``score_groups`` for one int32 plane ``rows`` (N, T) and int32 offsets ``group_off`` (G + 1,), both on
        the device of ``canon`` (the offsets have been checked on the host: ``_group_offsets``)."""
        lib = _lib.load()
        dev = canon.device
        N, T = rows.shape
        G = group_off.numel() - 1
        self._check_sizes(N, T)
        if T == 0:
            rows = rows.new_full((N, 1), int(end_idx))
            T = 1
        if rows.stride(1) != 1:
            rows = rows.contiguous()
        need = lib.ac_diversity_group_workspace_bytes(N, T, G)
        if need < 0:
            raise _lib.HipLibraryError(f"ac_diversity_group_workspace_bytes refused ({N} rows of {T} words in {G} groups)")
        workspace = self._workspace_of(need, dev)
        i32, f64 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float64)
        out = {"self_bleu": torch.empty(N, **f64), "mbleu": torch.empty(N, 4, **f64),
               "stats": torch.empty(N, 10, **i32), "sent_distinct": torch.empty(N, 4, **i32),
               "group_totals": torch.empty(G, 5, **i32), "group_mean": torch.empty(G, 5, **f64),
               "summary": torch.empty(5, **f64)}
        check(lib.ac_diversity_group_scores(ptr(rows), rows.stride(0), N, T, int(start_idx), int(end_idx), ptr(canon),
                                            int(vocab_size), ptr(group_off), G, ptr(workspace), workspace.numel(),
                                            ptr(out["stats"]), ptr(out["sent_distinct"]), ptr(out["self_bleu"]),
                                            ptr(out["mbleu"]), ptr(out["group_totals"]), ptr(out["group_mean"]),
                                            ptr(out["summary"]), stream()), "ac_diversity_group_scores")
        return out

    @staticmethod
    def _group_offsets(sizes):
        """Row offsets (G + 1,) int32 on the host of groups of ``sizes`` rows.  ValueError for no group and for a group of
        fewer than two rows: a caption alone in its group has no other caption to be scored against."""
        sizes = [int(n) for n in sizes]
        if not sizes:
            raise ValueError("Diversity: no groups")
        for g, n in enumerate(sizes):
            if n < 2:
                raise ValueError(f"Diversity: group {g} has {n} sentence(s): within a group a sentence is scored against "
                                 f"the group's others, so every group needs two or more")
        return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)

    def score_groups(self, vocabulary, vocab_size, words, start_idx, end_idx, group_off=None):
        """Diversity within groups: ``words`` (B, S, T) - B groups of S rows, e.g. the S sampled captions of each of B clips -
        or (N, T) with ``group_off``, G + 1 ascending row offsets from 0 to N held on the host (a list, an array or a CPU
        tensor; ragged groups).  A device tensor is scored where it lies; nothing is synchronised.  Returns device tensors
        ``{"stats" (N, 10), "sent_distinct" (N, 4), "self_bleu" (N,), "mbleu" (N, 4), "group_totals" (G, 5) = words and
        distinct n-grams of the group, "group_mean" (G, 5) = mean mBLEU-1..4 and mean Self-BLEU of the group, "summary" (5,)
        = their means over the groups}`` with "the others" of a sentence being the other rows of its group.  ValueError
        before any launch for a group of fewer than two rows and for the limits of ``score_ids``; a word id outside the
        vocabulary on the device makes every float NaN and every integer -1."""
        vocab_size = int(vocab_size)
        self._canon(vocabulary, vocab_size)   # (a vocabulary that cannot be used is refused first)
        w = torch.as_tensor(words)
        if w.dim() == 3:
            if group_off is not None:
                raise ValueError("Diversity.score_groups: (B, S, T) words imply the groups; group_off goes with (N, T) words")
            B, S, T = w.shape
            offsets = self._group_offsets([S] * B)
            w = w.reshape(B * S, T)
        elif w.dim() == 2:
            if group_off is None:
                raise ValueError("Diversity.score_groups: (N, T) words need group_off, the G + 1 row offsets of the groups")
            offsets = np.asarray(torch.as_tensor(group_off).cpu(), dtype=np.int64).reshape(-1)
            if offsets.size < 2 or offsets[0] != 0 or offsets[-1] != w.shape[0]:
                raise ValueError(f"Diversity.score_groups: group_off must run from 0 to {w.shape[0]} rows, got "
                                 f"{offsets.tolist()[:8]}")
            offsets = self._group_offsets(np.diff(offsets))
        else:
            raise ValueError(f"Diversity.score_groups: words must be (B, S, T) or (N, T) word ids, got {tuple(w.shape)}")
        self._check_sizes(w.shape[0], w.shape[1])
        self._refuse_foreign_ids(w, vocab_size, start_idx, end_idx)
        dev = self._device_of([w])
        canon_dev = self._canon(vocabulary, vocab_size, dev)
        return self.score_group_rows(w.to(device=dev, dtype=torch.int32), torch.from_numpy(offsets).to(dev), start_idx,
                                     end_idx, canon_dev, vocab_size)

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

    # ---- strings, within groups ------------------------------------------------------------------------------------
    def _pack_groups(self, hypothesis):
        """``{key: [sentence, ...]}`` as ``(keys, rows, group_off, start_idx, end_idx, vocab_size)``: the sentences of a key
        are consecutive rows, the keys in the dict's order.  Every refusal of ``compute_group_score`` is raised here."""
        if not isinstance(hypothesis, dict) or any(isinstance(g, str) for g in hypothesis.values()):
            raise ValueError("Diversity.compute_group_score: {key: [sentence, ...]}")
        keys = list(hypothesis)
        groups = [list(hypothesis[k]) for k in keys]
        for k, g in zip(keys, groups):
            if len(g) < 2:
                raise ValueError(f"Diversity.compute_group_score: key {k!r} has {len(g)} sentence(s): a caption is scored "
                                 f"against the other captions of its key, so every key needs two or more")
            if any(not isinstance(t, str) for t in g):
                raise ValueError("Diversity.compute_group_score: sentences must be strings")
        group_off = self._group_offsets([len(g) for g in groups])
        rows, start_idx, end_idx, vocab_size = self._pack_sentences([t for g in groups for t in g])
        return keys, rows, group_off, start_idx, end_idx, vocab_size

    def compute_group_score(self, hypothesis):
        """``{"mbleu_1" .. "mbleu_4", "self_bleu", "div_1", "div_2"}`` as means over the keys of ``hypothesis`` =
        ``{key: [sentence, ...]}`` - each key's sentences scored against each other only - and ``"per_key"``: the same seven
        numbers for every key.  div-n of a key: the distinct n-grams of its sentences over their words (NaN for a key
        without a word).  ValueError for a key with fewer than two sentences, a sentence of more than ``MAX_HYP_WORDS``
        words and the other limits of ``compute_score``."""
        keys, rows, group_off, start_idx, end_idx, vocab_size = self._pack_groups(hypothesis)
        canon = torch.arange(vocab_size, device="cuda", dtype=torch.int32)
        out = self.score_group_rows(torch.from_numpy(rows).to(canon.device), torch.from_numpy(group_off).to(canon.device),
                                    start_idx, end_idx, canon, vocab_size)
        summary = out["summary"].cpu().tolist()
        means = out["group_mean"].cpu().tolist()
        totals = out["group_totals"].cpu().tolist()
        names = ("mbleu_1", "mbleu_2", "mbleu_3", "mbleu_4", "self_bleu")
        per_key = {}
        for key, m, t in zip(keys, means, totals):
            per_key[key] = dict(zip(names, m))
            per_key[key]["div_1"] = t[1] / t[0] if t[0] else float("nan")
            per_key[key]["div_2"] = t[2] / t[0] if t[0] else float("nan")
        result = dict(zip(names, summary))
        for name in ("div_1", "div_2"):
            total = 0.0
            for key in keys:          # added in the order of the keys
                total += per_key[key][name]
            result[name] = total / len(keys)
        result["per_key"] = per_key
        return result
