"""CIDEr-D on the device (csrc/cider.hip): the scorer that the reference's second training stage passes to ``ScstWrapper``
(run.py:39, ``pycocoevalcap.cider.cider.Cider()``) and to its validation (run.py:152), built in.

``Cider(n=4, sigma=6.0)`` offers two routes onto the same kernels:

* ``compute_score(references, hypothesis)`` - pycocoevalcap's contract on strings: ``{key: [sentence, ...]}`` and
  ``{key: [sentence]}`` -> ``(mean, per-key array)`` in the order of ``references.keys()``.  Sentences are split on
  whitespace on the host and numbered through a word table private to the call.
* ``score_ids(key2refs, vocabulary, vocab_size, keys, words, start_idx, end_idx)`` - the route of self-critical sequence
  training: ``words`` are the decoded word ids of S hypothesis sets (N x T each, on the device or not), the result stays on
  the device: ``scores`` (S, N) and, for S >= 2, ``reward = scores[0] - scores[1]``.

Both score what ``compute_batch_score`` (rl_model.py, model_util.py:117-164) hands a string scorer: ``start_idx`` skipped,
the sentence cut at the first ``end_idx``, rows that share a key scored once on the first such row.  The document
frequencies are those of the call's own references, as pycocoevalcap's ``Cider`` computes them.

Ids and strings agree only if distinct ids are distinct words, so two vocabulary ids with the same string are mapped to
the first of them (the canonical-id table), reference words outside the vocabulary get fresh ids from ``vocab_size`` on,
and a vocabulary word that is empty or contains whitespace - which ``" ".join`` and ``split`` would not bring back - is
refused.  Packed references are kept per key for as long as the same ``key2refs`` object and vocabulary are passed; call
``clear_cache()`` after changing a ``key2refs`` in place.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

MAX_SETS = 4            # include/audiocaption_hip.h AC_CIDER_MAX_SETS
MAX_HYP_WORDS = 1024    # AC_CIDER_MAX_HYP_WORDS
MAX_REF_WORDS = 1024    # AC_CIDER_MAX_REF_WORDS


def canonical_ids(vocabulary, vocab_size):
    """``(word -> first id that spells it, canon int32 [vocab_size])`` from ``vocabulary.idx2word[i]``, i < vocab_size."""
    word2id = {}
    canon = np.empty(int(vocab_size), dtype=np.int32)
    for i in range(int(vocab_size)):
        word = vocabulary.idx2word[i]
        if not isinstance(word, str) or word.split() != [word]:
            raise ValueError(f"Cider: vocabulary word {i} is {word!r}: an empty word or one with whitespace does not survive "
                             f"' '.join and split(), so sentences of ids and of strings would differ")
        canon[i] = word2id.setdefault(word, i)
    return word2id, canon


def pack_sentence(sentence, word2id, oov, vocab_size):
    """The canonical ids of ``sentence.split()``; a word outside ``word2id`` gets (or reuses) an id >= vocab_size in ``oov``."""
    ids = []
    for word in sentence.split():
        i = word2id.get(word)
        if i is None:
            i = oov.setdefault(word, vocab_size + len(oov))
        ids.append(i)
    return np.asarray(ids, dtype=np.int32)


class PackedBatch:
    """The references of one call as the kernels read them (host arrays, int32): ``words`` of all sentences back to back,
    ``sent_off`` (M + 1), ``key_off`` (K + 1, first sentence of each distinct key, keys in order of first appearance),
    ``row_key`` (N, the distinct-key index of each row), ``first_row`` (K), and ``n_words``: ids are below it."""

    def __init__(self, keys, refs_of_key, n_words, who="Cider"):
        index, order, first_row = {}, [], []
        row_key = np.empty(len(keys), dtype=np.int32)
        for row, key in enumerate(keys):
            k = index.get(key)
            if k is None:
                k = index[key] = len(order)
                order.append(key)
                first_row.append(row)
            row_key[row] = k
        sentences, key_off = [], [0]
        for key in order:
            refs = refs_of_key(key)
            if len(refs) == 0:
                raise ValueError(f"{who}: key {key!r} has no reference sentence")
            sentences.extend(refs)
            key_off.append(len(sentences))
        lens = np.fromiter((len(s) for s in sentences), dtype=np.int64, count=len(sentences))
        self.keys = order
        self.words = np.concatenate(sentences).astype(np.int32, copy=False) if sentences else np.zeros(0, np.int32)
        self.sent_off = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
        self.key_off = np.asarray(key_off, dtype=np.int32)
        self.row_key = row_key
        self.first_row = np.asarray(first_row, dtype=np.int32)
        self.n_words = int(n_words)

    @property
    def max_ref_words(self):
        return int(np.diff(self.sent_off).max(initial=0))


class PackedScorer:
    """What the built-in scorers share (``Cider`` here, ``Bleu`` and ``Rouge`` of caption_metrics.py): the canonical-id
    table and the per-key cache of packed references behind ``pack_ids``, the checks and the one upload in front of a
    kernel call, and the numbering of the string route.  ``_who`` names the scorer in its refusals."""
    _who = "Cider"

    def clear_cache(self):
        self._vocab = None        # (vocabulary, vocab_size, word2id, canon, {device: canon on it})
        self._oov = {}
        self._refs = (None, {})   # (key2refs, {key: [ids of each reference]})
        self.packed_keys = 0      # keys packed since the last clear (a key is packed once per key2refs)

    def _canon(self, vocabulary, vocab_size, dev=None):
        """The canonical-id table of ``vocabulary``, built once per vocabulary (another vocabulary clears every cache):
        the host array, or with ``dev`` its copy on that device, uploaded once per device."""
        vocab_size = int(vocab_size)
        if self._vocab is None or self._vocab[0] is not vocabulary or self._vocab[1] != vocab_size:
            self.clear_cache()
            self._vocab = (vocabulary, vocab_size) + canonical_ids(vocabulary, vocab_size) + ({},)
        if dev is not None and dev not in self._vocab[4]:
            self._vocab[4][dev] = torch.from_numpy(self._vocab[3]).to(dev)
        return self._vocab[3] if dev is None else self._vocab[4][dev]

    @staticmethod
    def _device_of(tensors):
        """The device of the first of ``tensors`` that lives on one, else the current one."""
        on_dev = [w.device for w in tensors if w.is_cuda]
        return on_dev[0] if on_dev else torch.device("cuda", torch.cuda.current_device())

    def _refuse_foreign_ids(self, w, vocab_size, start_idx, end_idx, what="word id"):
        """ValueError for an id in ``w`` that is neither in the vocabulary nor start / end, if ``w`` is held on the host: a
        host copy can be checked; on the device the kernel answers a bad id with NaN."""
        if not w.is_cuda and not bool((((w >= 0) & (w < vocab_size)) | (w == start_idx) | (w == end_idx)).all()):
            raise ValueError(f"{self._who}: a {what} outside [0, {vocab_size})")

    def pack_ids(self, key2refs, vocabulary, vocab_size, keys):
        """The PackedBatch of ``keys`` (one per row) under ``vocabulary`` and the canonical-id table (host)."""
        vocab_size = int(vocab_size)
        canon = self._canon(vocabulary, vocab_size)
        if self._refs[0] is not key2refs:
            self._refs = (key2refs, {})
        word2id, cache = self._vocab[2], self._refs[1]

        def refs_of_key(key):
            hit = cache.get(key)
            if hit is None:
                hit = cache[key] = [pack_sentence(s, word2id, self._oov, vocab_size) for s in key2refs[key]]
                self.packed_keys += 1
            return hit

        batch = PackedBatch(list(keys), refs_of_key, 0, self._who)
        batch.n_words = vocab_size + len(self._oov)
        return batch, canon

    def _pack_for_ids(self, key2refs, vocabulary, vocab_size, keys, words):
        """``(batch, hypothesis tensors, canon on the device)`` for ``score_ids``."""
        words = [torch.as_tensor(w) for w in words]
        dev = self._device_of(words)
        keys = list(keys)
        if words[0].dim() != 2 or words[0].shape[0] != len(keys):
            raise ValueError(f"{self._who}: {len(keys)} keys for hypothesis words of shape {tuple(words[0].shape)}")
        batch, _ = self.pack_ids(key2refs, vocabulary, vocab_size, keys)
        return batch, words, self._canon(vocabulary, vocab_size, dev)

    def _pack_strings(self, references, hypothesis):
        """pycocoevalcap's arguments as ``(batch, rows, start_idx, end_idx, vocab_size)``: one row per key in the order of
        ``references.keys()``, the words numbered through a table private to the call."""
        who = f"{self._who}.compute_score"
        keys = list(references.keys())
        if not keys:
            raise ValueError(f"{who}: no references")
        if set(keys) != set(hypothesis.keys()):
            raise ValueError(f"{who}: references and hypothesis must have the same keys")
        end_idx, start_idx, first_word = 0, 1, 2
        table = {}

        def ids(sentence):
            return np.asarray([table.setdefault(w, first_word + len(table)) for w in sentence.split()], dtype=np.int32)

        hyps = []
        for key in keys:
            if len(hypothesis[key]) != 1:
                raise ValueError(f"{who}: one hypothesis per key, {key!r} has {len(hypothesis[key])}")
            hyps.append(ids(hypothesis[key][0]))
        batch = PackedBatch(keys, lambda key: [ids(s) for s in references[key]], 0, self._who)
        batch.n_words = vocab_size = first_word + len(table)
        rows = np.full((len(keys), max(1, max(len(h) for h in hyps))), end_idx, dtype=np.int32)
        for row, h in zip(rows, hyps):
            row[:len(h)] = h
        return batch, rows, start_idx, end_idx, vocab_size

    def _device_inputs(self, batch, words, start_idx, end_idx, canon, vocab_size):
        """Everything the host can check, raised as ValueError before the first launch, then the hypothesis sets as int32
        planes of one length and stride on the device of ``canon`` and the references in one upload.  Returns
        ``(S, keep, planes, refs)``: the leading arguments every scorer's entry point takes, in two runs (``planes``: the
        hypothesis sets up to ``vocab_size``; ``refs``: the packed references; ``ac_cider_scores`` takes ``n_words``
        between them), and ``keep``, which owns the memory they point to."""
        who = self._who
        dev = canon.device
        N = batch.row_key.shape[0]
        if not 1 <= len(words) <= MAX_SETS:
            raise ValueError(f"{who}: 1 to {MAX_SETS} hypothesis sets, got {len(words)}")
        if batch.max_ref_words > MAX_REF_WORDS:
            raise ValueError(f"{who}: a reference sentence of {batch.max_ref_words} words; the kernels take {MAX_REF_WORDS}")
        if batch.words.size and (int(batch.words.min()) < 0 or int(batch.words.max()) >= batch.n_words):
            raise ValueError(f"{who}: a reference word id outside [0, {batch.n_words}) (vocabulary {vocab_size} + "
                             f"{batch.n_words - vocab_size} words outside it)")
        sets = []
        for w in words:
            w = torch.as_tensor(w)
            if w.dim() != 2 or w.shape[0] != N:
                raise ValueError(f"{who}: hypothesis words must be ({N} rows, length), got {tuple(w.shape)}")
            if w.shape[1] > MAX_HYP_WORDS:
                raise ValueError(f"{who}: hypotheses of {w.shape[1]} words; the kernels take {MAX_HYP_WORDS}")
            self._refuse_foreign_ids(w, vocab_size, start_idx, end_idx, "hypothesis word id")
            sets.append(w.to(device=dev, dtype=torch.int32))
        T = sets[0].shape[1]
        if any(w.shape[1] != T for w in sets):
            raise ValueError(f"{who}: the hypothesis sets must have one length")
        if any(w.stride(1) != 1 or w.stride(0) != sets[0].stride(0) for w in sets) or T == 0:
            sets = [w.contiguous() for w in sets]
        K, M, W = batch.first_row.shape[0], batch.sent_off.shape[0] - 1, batch.words.shape[0]
        host = np.concatenate((batch.words, batch.sent_off, batch.key_off, batch.row_key, batch.first_row))
        ints = torch.from_numpy(host).to(dev)          # the one upload
        base = ints.data_ptr()
        p_words, p_sent, p_key, p_row, p_first = (ctypes.c_void_p(base + 4 * int(o)) for o in np.cumsum([0, W, M + 1, K + 1, N]))
        S = len(sets)
        hyp = (ctypes.c_void_p * S)(*[w.data_ptr() for w in sets])
        planes = (ctypes.cast(hyp, ctypes.c_void_p), S, sets[0].stride(0), N, T, int(start_idx), int(end_idx), ptr(canon),
                  int(vocab_size))
        refs = (p_words, W, p_sent, M, batch.max_ref_words, p_key, K, p_row, p_first)
        return S, (sets, ints, hyp), planes, refs

    def _workspace_of(self, need, dev):
        if self._workspace is None or self._workspace.device != dev or self._workspace.numel() < need:
            self._workspace = torch.empty(need, device=dev, dtype=torch.uint8)
        return self._workspace


class Cider(PackedScorer):

    def __init__(self, n=4, sigma=6.0):
        if not 1 <= int(n) <= 4:
            raise ValueError("Cider: n-grams of 1 to 4 words are built in")
        if not sigma > 0:
            raise ValueError("Cider: sigma must be > 0")
        self._n, self._sigma = int(n), float(sigma)
        self._workspace = None
        self.clear_cache()

    def method(self):
        return "CIDEr"

    # ---- the kernels ---------------------------------------------------------------------------------------------
    def score_packed(self, batch, words, start_idx, end_idx, canon, vocab_size):
        """Scores (S, N) f32 and reward (N,) f32 (None for S == 1) on the device of ``canon`` for the hypothesis sets
        ``words`` (S tensors N x T of word ids) against the references of ``batch``.  Everything is checked before the
        first launch: what the host can see raises ValueError here, and the entry point checks its limits again."""
        lib = _lib.load()
        dev = canon.device
        S, keep, planes, refs = self._device_inputs(batch, words, start_idx, end_idx, canon, vocab_size)
        N, K, M, W = batch.row_key.shape[0], batch.first_row.shape[0], batch.sent_off.shape[0] - 1, batch.words.shape[0]
        need = lib.ac_cider_workspace_bytes(W, M, K, S)
        if need < 0:
            raise _lib.HipLibraryError(f"ac_cider_workspace_bytes refused ({W} words, {M} sentences, {K} keys, {S} sets)")
        workspace = self._workspace_of(need, dev)
        scores = torch.empty(S, N, device=dev, dtype=torch.float32)
        reward = torch.empty(N, device=dev, dtype=torch.float32) if S >= 2 else None
        check(lib.ac_cider_scores(*planes, batch.n_words, *refs, self._n, self._sigma, ptr(workspace), workspace.numel(),
                                  ptr(scores), ptr(reward), stream()), "ac_cider_scores")
        return scores, reward

    # ---- strings (pycocoevalcap's contract) ------------------------------------------------------------------------
    def compute_score(self, references, hypothesis):
        batch, rows, start_idx, end_idx, vocab_size = self._pack_strings(references, hypothesis)
        canon = torch.arange(vocab_size, device="cuda", dtype=torch.int32)
        scores, _ = self.score_packed(batch, [torch.from_numpy(rows)], start_idx, end_idx, canon, vocab_size)
        scores = scores[0].cpu().numpy().astype(np.float64)
        return float(scores.mean()), scores

    # ---- word ids (self-critical sequence training) ------------------------------------------------------------------
    def score_ids(self, key2refs, vocabulary, vocab_size, keys, words, start_idx, end_idx):
        """``{"scores": (S, N) f32, "reward": (N,) f32 = scores[0] - scores[1] (None for S == 1)}`` on the device, for the
        S hypothesis sets ``words`` (N x T word ids each; N = len(keys))."""
        batch, words, canon_dev = self._pack_for_ids(key2refs, vocabulary, vocab_size, keys, words)
        scores, reward = self.score_packed(batch, words, start_idx, end_idx, canon_dev, int(vocab_size))
        return {"scores": scores, "reward": reward}
