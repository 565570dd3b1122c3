"""Repetition and word constraints of a search: the four ``input_dict`` keys every generation stack offers against
captions that repeat themselves or emit unwanted words, parsed and validated on the host.

    repetition_penalty     rho, finite and > 0 (1.0 = off): the logit of every word the row has generated is divided by rho
                           when positive, multiplied by it otherwise - once per word, from the raw logit
    no_repeat_ngram_size   n, int, 0 = off, up to max_length: no n-gram occurs twice in a caption
    bad_words              flat list of at most 256 word ids in [0, vocab): never emitted (no multi-word phrases)
    min_length             m, int, 0 .. max_length: <end> is not emitted before step m

They act on the raw logits of a step, in this order, before the search's own selection rule (csrc/logit_rules.hip; a banned
word's logit is -inf and the log-softmax renormalises over the others, so ``sampled_logprob`` is the constrained
distribution's value).  The rules are a pure function of (prefix, logits) and apply to every row alike.

``LogitRules.parse`` raises ValueError before anything is launched; a parsed object is hashable (it is part of a search
state's key: a graph captured under one rule set is never replayed under another) and knows whether it is ``neutral`` -
a neutral request takes exactly the code path of a request without the keys."""
import math

import torch

from . import _lib

KEYS = ("repetition_penalty", "no_repeat_ngram_size", "bad_words", "min_length")
MAX_BAD_WORDS = 256     # csrc/logit_rules.hip


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _bad_list(v):
    """``bad_words`` as a tuple of ints (None / empty: ()).  ValueError for anything but a flat sequence of ints."""
    if v is None:
        return ()
    if isinstance(v, torch.Tensor):
        if v.dim() != 1 or v.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"bad_words must be a flat list of word ids, got a {tuple(v.shape)} {v.dtype} tensor")
        v = v.tolist()
    if isinstance(v, (str, bytes)) or not hasattr(v, "__iter__"):
        raise ValueError(f"bad_words must be a flat list of word ids, got {v!r}")
    out = []
    for w in v:
        if hasattr(w, "item") and not isinstance(w, torch.Tensor):    # numpy integers
            w = w.item()
        if not _is_int(w):
            raise ValueError(f"bad_words must be a flat list of word ids (multi-word phrases are not built), got {w!r}")
        out.append(w)
    return tuple(out)


class LogitRules:
    __slots__ = ("repetition_penalty", "no_repeat_ngram_size", "bad_words", "min_length")

    def __init__(self, repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words=(), min_length=0):
        self.repetition_penalty = float(repetition_penalty)
        self.no_repeat_ngram_size = int(no_repeat_ngram_size)
        self.bad_words = tuple(int(w) for w in bad_words)
        self.min_length = int(min_length)

    @classmethod
    def parse(cls, input_dict, vocab_size, max_length, start_idx, end_idx):
        """The rules of a request (keys absent or None: off), checked against the search they are for."""
        rho = input_dict.get("repetition_penalty")
        rho = 1.0 if rho is None else rho
        if isinstance(rho, bool) or not isinstance(rho, (int, float)) or not math.isfinite(rho) or not rho > 0:
            raise ValueError(f"repetition_penalty must be a finite number > 0 (1.0 = off), got {rho!r}")
        n = input_dict.get("no_repeat_ngram_size")
        n = 0 if n is None else n
        if not _is_int(n) or not 0 <= n <= max_length:
            raise ValueError(f"no_repeat_ngram_size must be an int in 0..max_length = {max_length} (0 = off), got {n!r}")
        m = input_dict.get("min_length")
        m = 0 if m is None else m
        if not _is_int(m) or not 0 <= m <= max_length:
            raise ValueError(f"min_length must be an int in 0..max_length = {max_length}, got {m!r}")
        bad = _bad_list(input_dict.get("bad_words"))
        if len(bad) > MAX_BAD_WORDS:
            raise ValueError(f"bad_words takes at most {MAX_BAD_WORDS} word ids, got {len(bad)}")
        for w in bad:
            if not 0 <= w < vocab_size:
                raise ValueError(f"bad_words: word id {w} is outside the vocabulary [0, {vocab_size})")
            if w == end_idx or w == start_idx:
                raise ValueError(f"bad_words: {w} is the {'end' if w == end_idx else 'start'} token")
        rules = cls(rho, n, bad, m)
        # the words of a prefix, <end> and the banned words together must leave a row one word it can emit
        if not rules.neutral and len(bad) + max_length + 1 >= vocab_size:
            raise ValueError(f"{len(bad)} bad_words and a caption of {max_length} words could ban a whole row of a "
                             f"vocabulary of {vocab_size}")
        return rules

    @property
    def neutral(self):
        return (self.repetition_penalty == 1.0 and self.no_repeat_ngram_size == 0 and not self.bad_words
                and self.min_length == 0)

    def key(self):
        return (self.no_repeat_ngram_size, self.repetition_penalty, self.min_length, self.bad_words)

    def __hash__(self):
        return hash(self.key())

    def __eq__(self, other):
        return isinstance(other, LogitRules) and self.key() == other.key()

    def __repr__(self):
        return (f"LogitRules(repetition_penalty={self.repetition_penalty}, no_repeat_ngram_size={self.no_repeat_ngram_size}, "
                f"bad_words={list(self.bad_words)}, min_length={self.min_length})")

    # ---- the device side ------------------------------------------------------------------------------------------------
    def buffers(self, dev, rows, vocab_size, end_idx):
        """What a search state holds for these rules: the banned words on the device, the plane of constrained rows (``rows``
        rows of ``ld_plane`` floats, rows 16-byte aligned) and the ``ac_logit_rules`` struct over them."""
        bad = torch.tensor(self.bad_words or (0,), device=dev, dtype=torch.int32)
        ld = (vocab_size + 3) // 4 * 4
        rules = _lib.AcLogitRules(self.repetition_penalty, self.no_repeat_ngram_size, self.min_length, int(end_idx),
                                  len(self.bad_words), bad.data_ptr() if self.bad_words else None)
        return {"rules_bad": bad, "rules_plane": torch.empty(rows, ld, device=dev, dtype=torch.float32), "ld_plane": ld,
                "rules": rules}


def first_active_key(input_dict):
    """The first of the four keys whose value in ``input_dict`` switches a rule on (None: the request is neutral).  For the
    surfaces that do not build the rules: they name the key they refuse, and accept neutral values."""
    rho = input_dict.get("repetition_penalty")
    if rho is not None and rho != 1.0:
        return "repetition_penalty"
    for k in ("no_repeat_ngram_size", "min_length"):
        if input_dict.get(k) not in (None, 0):
            return k
    bad = input_dict.get("bad_words")
    if bad is not None and len(bad) > 0:
        return "bad_words"
    return None


def refuse(input_dict, who, instead="TransformerModel's blocking model(input_dict)"):
    """NotImplementedError naming the key when ``input_dict`` asks ``who`` for a non-neutral rule."""
    k = first_active_key(input_dict)
    if k is not None:
        raise NotImplementedError(f"{who}: {k} (repetition and word constraints) is not built here; it is built for {instead}")

