"""BLEU-1..4 and ROUGE-L on the device (csrc/capmetrics.hip): beside ``Cider`` the two scorers of the reference's
``evaluate`` / ``evaluate_prediction`` (train_eval/base.py:154-165, 330-340, ``[Bleu(n=4), Rouge(), Cider()]`` from
pycocoevalcap) that need neither Java nor a language model, built in, and ``eval_prediction``, the loop that runs them.

``Bleu(n=4)`` and ``Rouge()`` keep pycocoevalcap's contracts and offer the two routes of ``Cider`` onto their kernels:

* ``compute_score(references, hypothesis)`` on strings, ``{key: [sentence, ...]}`` and ``{key: [sentence]}``, results in
  the order of ``references.keys()``: ``Bleu`` returns ``([n corpus scores], [n lists of per-key scores])`` and ``Rouge``
  ``(mean over the keys, float64 array per key)``.
* ``score_ids(key2refs, vocabulary, vocab_size, keys, words, start_idx, end_idx)`` on the decoded word ids of S hypothesis
  sets (N x T each, on the device or not); the results stay on the device, the integers the scores were computed from are
  part of them, and totals and means run over the distinct keys.

The arithmetic is that of bleu_scorer.py with ``option="closest"`` and of rouge.py with ``beta = 1.2``, stated with the
prototypes in include/audiocaption_hip.h; the counts are exact integers and the formulas run in float64.  Sentences are
split on whitespace, as ``Cider`` splits them.  pycocoevalcap's Rouge splits on single spaces instead; the one visible
difference is the empty hypothesis, which scores 0 here (there it is a sentence of one empty word).  A key without
references is refused, as by ``Cider``, and so is a reference without words (a recall over a length of zero).  The
sentence rule, the canonical-id table and the cache of packed references are those of cider.py.

Not built, and not part of ``eval_prediction``: the PTB tokenizer (input is taken as tokenized, the reference's
``pretokenized=True``), METEOR and SPICE (Java), SPIDEr (needs SPICE) and FENSE (a language model).
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream
from .cider import PackedScorer


class _StringMetric(PackedScorer):
    """The calling side that ``Bleu`` and ``Rouge`` share; ``_launch`` is the one call that differs."""

    def _init(self):
        self._workspace = None
        self.clear_cache()

    def _check_references(self, batch):
        if int(np.diff(batch.sent_off).min(initial=1)) == 0:
            raise ValueError(f"{self._who}: a reference sentence without words")

    def pack_ids(self, key2refs, vocabulary, vocab_size, keys):
        batch, canon = super().pack_ids(key2refs, vocabulary, vocab_size, keys)
        self._check_references(batch)
        return batch, canon

    def score_packed(self, batch, words, start_idx, end_idx, canon, vocab_size):
        """The scorer's dict of device tensors (see ``score_ids``) on the device of ``canon`` for the hypothesis sets
        ``words`` (S tensors N x T of word ids) against the references of ``batch``.  Everything is checked before the
        first launch: what the host can see raises ValueError here, and the entry point checks its limits again."""
        lib = _lib.load()
        dev = canon.device
        self._check_references(batch)
        S, keep, planes, refs = self._device_inputs(batch, words, start_idx, end_idx, canon, vocab_size)
        K = batch.first_row.shape[0]
        need = lib.ac_capmetrics_workspace_bytes(K, S)
        if need < 0:
            raise _lib.HipLibraryError(f"ac_capmetrics_workspace_bytes refused ({K} keys, {S} sets)")
        workspace = self._workspace_of(need, dev)
        out = self._launch(lib, batch, S, dev, planes + refs, (ptr(workspace), workspace.numel()))
        out["keys"] = batch.keys
        return out

    def score_ids(self, key2refs, vocabulary, vocab_size, keys, words, start_idx, end_idx):
        batch, words, canon_dev = self._pack_for_ids(key2refs, vocabulary, vocab_size, keys, words)
        return self.score_packed(batch, words, start_idx, end_idx, canon_dev, int(vocab_size))

    def _score_strings(self, references, hypothesis):
        batch, rows, start_idx, end_idx, vocab_size = self._pack_strings(references, hypothesis)
        self._check_references(batch)
        canon = torch.arange(vocab_size, device="cuda", dtype=torch.int32)
        return self.score_packed(batch, [torch.from_numpy(rows)], start_idx, end_idx, canon, vocab_size)


class Bleu(_StringMetric):
    """``score_ids`` returns ``{"scores": (S, n, N) f64, "corpus": (S, n) f64, "stats": (S, K, 2 + 2 n) int32 =
    testlen, reflen, guess[n], correct[n] per distinct key, "keys": the K distinct keys in that order}``."""
    _who = "Bleu"

    def __init__(self, n=4):
        if not 1 <= int(n) <= 4:
            raise ValueError("Bleu: n-grams of 1 to 4 words are built in")
        self._n = int(n)
        self._init()

    def method(self):
        return "Bleu"

    def _launch(self, lib, batch, S, dev, shared, workspace):
        N, K, n = batch.row_key.shape[0], batch.first_row.shape[0], self._n
        stats = torch.empty(S, K, 2 + 2 * n, device=dev, dtype=torch.int32)
        scores = torch.empty(S, n, N, device=dev, dtype=torch.float64)
        corpus = torch.empty(S, n, device=dev, dtype=torch.float64)
        check(lib.ac_bleu_scores(*shared, n, *workspace, ptr(stats), ptr(scores), ptr(corpus), stream()), "ac_bleu_scores")
        return {"scores": scores, "corpus": corpus, "stats": stats}

    def compute_score(self, references, hypothesis):
        out = self._score_strings(references, hypothesis)
        return out["corpus"][0].cpu().tolist(), out["scores"][0].cpu().tolist()


class Rouge(_StringMetric):
    """``score_ids`` returns ``{"scores": (S, N) f64, "mean": (S,) f64 over the distinct keys, "lcs": (S, M) int32, the
    longest common subsequence of each of the M packed reference sentences (the references of the K distinct keys back to
    back) with the hypothesis of its key, "keys": the K distinct keys in that order}``."""
    _who = "Rouge"

    def __init__(self):
        self._init()

    def method(self):
        return "Rouge"

    def _launch(self, lib, batch, S, dev, shared, workspace):
        N, M = batch.row_key.shape[0], batch.sent_off.shape[0] - 1
        lcs = torch.empty(S, M, device=dev, dtype=torch.int32)
        scores = torch.empty(S, N, device=dev, dtype=torch.float64)
        mean = torch.empty(S, device=dev, dtype=torch.float64)
        check(lib.ac_rouge_l_scores(*shared, *workspace, ptr(lcs), ptr(scores), ptr(mean), stream()), "ac_rouge_l_scores")
        return {"scores": scores, "mean": mean, "lcs": lcs}

    def compute_score(self, references, hypothesis):
        out = self._score_strings(references, hypothesis)
        return float(out["mean"][0]), out["scores"][0].cpu().numpy()


def eval_prediction(key2refs, key2pred, scorers, per_audio=False):
    """The reference's ``_eval_prediction`` (train_eval/base.py:112-127) for tokenized input: ``{method: score}`` over
    ``scorers`` (any objects with ``method()`` and ``compute_score(key2refs, key2pred)``), and with ``per_audio`` also
    ``{"per_audio": {method: {key: score}}}`` in the order of ``key2refs``; for ``"Bleu"`` the overall score is the list
    of the n corpus scores and the per-audio one is BLEU-4's (the highest order of a scorer built with n < 4)."""
    output = {}
    if per_audio:
        output["per_audio"] = {}
    for scorer in scorers:
        name = scorer.method()
        score, scores = scorer.compute_score(key2refs, key2pred)
        output[name] = score
        if per_audio:
            if name == "Bleu":
                scores = scores[min(3, len(scores) - 1)]
            output["per_audio"][name] = dict(zip(key2refs.keys(), scores))
    return output


def specificity(predictions, word_to_specificity):
    """The reference's specificity score (python_scripts/eval/specificity.py:13-22), on the host: the mean over
    ``predictions`` of the summed specificities of a caption's whitespace-separated words.  ``predictions``: captions as
    strings, or the ``{"tokens": caption}`` records of the reference's prediction files.  A word that is not in
    ``word_to_specificity`` raises KeyError, as there."""
    totals = []
    for prediction in predictions:
        caption = prediction["tokens"] if isinstance(prediction, dict) else prediction
        totals.append(sum(word_to_specificity[word] for word in caption.split()))
    return sum(totals) / len(totals)
