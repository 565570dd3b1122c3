"""``sample_method`` names of the reference's ``CaptionModel.sample_next_word`` (base.py:214-252) other than "greedy" /
"beam" / "dbs", mapped to the sampler of csrc/sample.hip (``AC_SAMPLE_*`` in include/audiocaption_hip.h)."""
import math

import numpy as np
import torch

PLAIN, TOPK, TOPP, GUMBEL = 0, 1, 2, 3
_TOPP_MAX = float(np.nextafter(np.float32(1.0), np.float32(0.0)))   # largest f32 below 1


def parse_sample_method(method, vocab_size, temp=1.0):
    """(method code, k, top_p, temp) as base.py:217-233 reads the name: "gumbel"; "top<x>" with 0 < x < 1 top-p, else top-k
    with k = int(x); any other name plain temperature sampling.  Raises ValueError where the reference fails or returns NaN:
    a malformed "top" suffix, k < 1 or k > vocab_size, temp <= 0 for plain and top-k sampling."""
    temp = float(temp)
    if method == "gumbel":
        return GUMBEL, 0, 0.0, 1.0          # argmax(lp + G) / temp: temp does not move the argmax
    if method.startswith("top"):
        try:
            top_num = float(method[3:])
        except ValueError:
            raise ValueError(f"sample_method={method!r}: 'top' must be followed by a number (top-k: 'top5', top-p: 'top0.9')")
        if 0 < top_num < 1:
            return TOPP, 0, min(top_num, _TOPP_MAX), 1.0   # top-p draws from softmax(logit): temp is not used
        try:
            k = int(top_num)
        except (ValueError, OverflowError):
            raise ValueError(f"sample_method={method!r}: not a valid top-k / top-p value")
        if not 1 <= k <= vocab_size:
            raise ValueError(f"sample_method={method!r}: top-k needs 1 <= k <= vocab size ({vocab_size})")
        _check_temp(method, temp)
        return TOPK, k, 0.0, temp
    _check_temp(method, temp)
    return PLAIN, 0, 0.0, temp


def _check_temp(method, temp):
    if not (temp > 0 and math.isfinite(temp)):
        raise ValueError(f"sample_method={method!r} needs a finite temp > 0 (got {temp})")


def draw_seed():
    """A 64-bit seed from torch's default CPU generator: ``torch.manual_seed(s)`` makes a sampled run reproducible."""
    lo, hi = (int(v) for v in torch.randint(0, 2 ** 32, (2,), dtype=torch.int64))
    return lo | (hi << 32)


def seed_word(seed):
    """The seed as the int64 whose bits the kernels read as their uint64 Philox key."""
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed {seed} is not a 64-bit unsigned integer")
    return seed - 2 ** 64 if seed >= 2 ** 63 else seed
