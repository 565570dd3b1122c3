"""CPU restatement of the sound-event tagger ``Cnn8rnnSedModel`` (reference hf_wrapper.py:1791-1859) and of its host
post-processing (hf_wrapper.py:89-216), written from the reference's arithmetic with plain torch / NumPy ops.
tests/golden/make_golden_sed.py asserts that it equals the reference (values within 1e-4, tags identical); the tests use it
where the fixture cannot hold the reference's own arrays.

``stack(state, lms, double=False)``: the conv stack, fc1, the bi-GRU and fc_audioset -> the pre-activation (B, T // 4, C).
``double=True`` evaluates everything in float64 (what a tolerance is measured against).
"""
import numpy as np
import torch
import torch.nn.functional as F

RATIO = 4
HIGH, LOW, N_CONNECT, TIME_RES, THRE = 0.75, 0.25, 1, 0.01, 0.5
POOLS = [(2, 2), (2, 2), (1, 2), (1, 2)]


def _bn(x, st, p, eps=1e-5):
    shape = (1, -1, 1, 1)
    scale = st[p + ".weight"] / torch.sqrt(st[p + ".running_var"] + eps)
    return (x - st[p + ".running_mean"].view(shape)) * scale.view(shape) + st[p + ".bias"].view(shape)


def _gru_dir(x, w_ih, w_hh, b_ih, b_hh, reverse):
    B, S, _ = x.shape
    Hd = w_hh.shape[1]
    gx = x @ w_ih.t() + b_ih
    h = x.new_zeros(B, Hd)
    out = [None] * S
    for t in (range(S - 1, -1, -1) if reverse else range(S)):
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gx[:, t, :Hd] + gh[:, :Hd])
        z = torch.sigmoid(gx[:, t, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
        n = torch.tanh(gx[:, t, 2 * Hd:] + r * gh[:, 2 * Hd:])
        h = (1 - z) * n + z * h
        out[t] = h
    return torch.stack(out, 1)


def features(state, lms, prefix="", double=False, blocks=None):
    """lms (B, 64, T) -> the bi-GRU's output (B, T // 4, 512) (hf_wrapper.py:1824-1847)."""
    dt = torch.float64 if double else torch.float32
    st = {k[len(prefix):]: v.to(dt) for k, v in state.items() if k.startswith(prefix) and v.dtype.is_floating_point}
    x = lms.to(dt).transpose(1, 2).unsqueeze(1)                    # (B, 1, T, 64)
    x = _bn(x.transpose(1, 3), st, "bn0").transpose(1, 3)
    for b, pool in enumerate(POOLS):
        p = f"conv_block{b + 1}."
        x = F.relu(_bn(F.conv2d(x, st[p + "conv1.weight"], padding=1), st, p + "bn1"))
        x = F.relu(_bn(F.conv2d(x, st[p + "conv2.weight"], padding=1), st, p + "bn2"))
        x = F.avg_pool2d(x, pool) + F.max_pool2d(x, pool)
        if blocks is not None:
            blocks.append(x.clone())
    return _after_conv(st, x.mean(dim=3).transpose(1, 2))          # (B, T // 4, 512)


def after_conv(state, x, prefix="", double=False):
    """The mean over mel of block 4 (B, T // 4, 512) -> the bi-GRU's output: fc1 + ReLU and the GRU (hf_wrapper.py:1846-1847)."""
    dt = torch.float64 if double else torch.float32
    st = {k[len(prefix):]: v.to(dt) for k, v in state.items() if k.startswith(prefix) and v.dtype.is_floating_point}
    return _after_conv(st, x.to(dt))


def _after_conv(st, x):
    x = F.relu(x @ st["fc1.weight"].t() + st["fc1.bias"])
    fwd = _gru_dir(x, st["rnn.weight_ih_l0"], st["rnn.weight_hh_l0"], st["rnn.bias_ih_l0"], st["rnn.bias_hh_l0"], False)
    bwd = _gru_dir(x, st["rnn.weight_ih_l0_reverse"], st["rnn.weight_hh_l0_reverse"], st["rnn.bias_ih_l0_reverse"],
                   st["rnn.bias_hh_l0_reverse"], True)
    return torch.cat([fwd, bwd], dim=2)


def head_preact(state, feat, prefix=""):
    w, b = state[prefix + "fc_audioset.weight"].to(feat.dtype), state[prefix + "fc_audioset.bias"].to(feat.dtype)
    return feat @ w.t() + b


def stack(state, lms, prefix="", double=False):
    return head_preact(state, features(state, lms, prefix, double), prefix)


def probs(pre):
    """clamp(sigmoid(pre), 1e-7, 1) (hf_wrapper.py:1848)."""
    return torch.sigmoid(pre).clamp(1e-7, 1.0)


def framewise(seg, frames_num, ratio=RATIO):
    """interpolate + pad_framewise_output (hf_wrapper.py:54-87) on a NumPy / torch array (B, S, C)."""
    seg = np.asarray(seg)
    fr = np.repeat(seg, ratio, axis=1)
    if fr.shape[1] < frames_num:
        fr = np.concatenate([fr, np.repeat(seg[:, -1:], frames_num - fr.shape[1], axis=1)], axis=1)
    return fr


# ---- post-processing: double_threshold(., 0.75, 0.25, n_connect=1) + decode_with_timestamps(., 0.01) -----------------
def segments(seg_prob, frames_num, ratio=RATIO, high=HIGH, low=LOW, n_connect=N_CONNECT):
    """One clip's segment-wise probabilities (S, C) float32 -> [(class, onset frame, offset frame)] in the reference's
    order (class by class, by onset): runs of p > low with a p > high inside, merged across gaps of <= n_connect frames,
    the last segment stretched to frames_num."""
    x = np.asarray(seg_prob, dtype=np.float32)
    S, C = x.shape
    lo, hi = x > np.float32(low), x > np.float32(high)
    out = []
    for c in np.nonzero(hi.any(axis=0))[0]:
        col = lo[:, c]
        edges = np.flatnonzero(np.diff(np.concatenate([[False], col, [False]]).astype(np.int8)))
        cur = None
        for s0, s1 in edges.reshape(-1, 2):
            if not hi[s0:s1, c].any():
                continue
            on, off = int(s0) * ratio, (frames_num if s1 == S else int(s1) * ratio)
            if cur is not None and on - cur[1] <= n_connect:
                cur[1] = off
            else:
                if cur is not None:
                    out.append((int(c), cur[0], cur[1]))
                cur = [on, off]
        if cur is not None:
            out.append((int(c), cur[0], cur[1]))
    return out


def _contracted_durations(a, res):
    """e * res - s * res as a compiler that contracts computes it: fma(-res, s, round(e * res)), ONE rounding of the exact
    value (rational arithmetic, then the nearest double)."""
    from fractions import Fraction
    r = Fraction(res)
    return np.array([float(Fraction(float(e) * res) - r * int(s)) for s, e in zip(a[:, 1], a[:, 2])], dtype=np.float64)


def tag_of_segments(segs, res=TIME_RES, thre=THRE, integer_form=False, contracted=False):
    """segments_to_temporal_tag (hf_wrapper.py:191-203) on [(class, onset frame, offset frame)], vectorised over all
    ordered pairs in float64 exactly as the reference computes them: t = frame * res first, then the differences.
    Two WRONG variants the tests must reject, because they miss ties that the float64 rounding of frame * 0.01 breaks:
    ``integer_form``, the reformulation 2 * (e_j - s_k) < min(...) on frame counts, and ``contracted``, the durations with
    the product fused into the subtraction (what -ffp-contract=fast makes of them on the device)."""
    if not segs:
        return 0
    a = np.asarray(segs, dtype=np.int64)
    cls = a[:, 0]
    if integer_form:
        s, e = a[:, 1], a[:, 2]
        d = e - s
        ov2, mind = 2 * (e[:, None] - s[None, :]), np.minimum(d[:, None], d[None, :])
        after, while_ = ov2 < mind, (s[:, None] < s[None, :]) & (ov2 > mind)
    else:
        s, e = a[:, 1] * res, a[:, 2] * res          # int64 * Python float -> float64, as row[0] * time_resolution
        d = _contracted_durations(a, res) if contracted else e - s
        lim = thre * np.minimum(d[:, None], d[None, :])
        ov = e[:, None] - s[None, :]
        after, while_ = ov < lim, (s[:, None] < s[None, :]) & (ov > lim)
    diff = cls[:, None] != cls[None, :]
    return 2 * int((after & diff).any()) + int((while_ & diff).any())


def temporal_tags(seg_prob, frames_num, ratio=RATIO, integer_form=False, n_connect=N_CONNECT):
    """(B, S, C) segment-wise probabilities -> list of B tags."""
    return [tag_of_segments(segments(x, frames_num, ratio, n_connect=n_connect), integer_form=integer_form)
            for x in np.asarray(seg_prob)]


# ---- the tie sweep: thousands of segment pairs on the 4-frame grid ------------------------------------------------------
SWEEP_S = 250
NAMED_PAIRS = [((760, 936), (892, 980)), ((460, 888), (832, 944)),     # the issue's: the reference sets after / while
               ((808, 840), (232, 824)), ((428, 564), (176, 496))]     # contracted durations set while / after, the reference neither


def tie_sweep(n_ties=3072, n_random=1020, seed=21):
    """[((s_j, e_j), (s_k, e_k))] in frames, multiples of 4 below 4 * SWEEP_S: the named pairs, ``n_ties`` random pairs whose
    overlap is EXACTLY half the shorter duration in integer frames (the rule then hangs on the float64 rounding of
    frame * 0.01) and ``n_random`` unconstrained ones."""
    rng = np.random.default_rng(seed)
    pairs, ties = list(NAMED_PAIRS), 0
    while ties < n_ties:
        sj, sk = (int(v) for v in rng.integers(0, SWEEP_S - 2, 2))
        dk = int(rng.integers(1, SWEEP_S - sk)) // 2 * 2
        if dk < 2:
            continue
        ej = sk + dk // 2                      # 2 * (e_j - s_k) == d_k
        if ej <= sj or ej > SWEEP_S or ej - sj < dk:
            continue                           # d_k must be the shorter (or equal) duration
        pairs.append(((4 * sj, 4 * ej), (4 * sk, 4 * (sk + dk))))
        ties += 1
    for _ in range(n_random):
        (sj, ej), (sk, ek) = (sorted(int(v) for v in rng.choice(SWEEP_S + 1, 2, replace=False)) for _ in range(2))
        pairs.append(((4 * sj, 4 * ej), (4 * sk, 4 * ek)))
    return pairs


def sweep_tags(pairs, **variant):
    return [tag_of_segments([(0,) + j, (1,) + k], **variant) for j, k in pairs]


def sweep_probabilities(pairs):
    """(len(pairs), SWEEP_S, 2) float32: clip i holds pair i, segment j in class 0 and segment k in class 1; frames_num is
    4 * SWEEP_S."""
    x = np.full((len(pairs), SWEEP_S, 2), 0.05, dtype=np.float32)
    for i, segs in enumerate(pairs):
        for c, (on, off) in enumerate(segs):
            x[i, on // 4:off // 4, c] = 0.5
            x[i, on // 4, c] = 0.9
    return x


# ---- the hand-built post-processing set ---------------------------------------------------------------------------------
def _clip(S, C, runs, base=0.05):
    """(S, C) probabilities: ``runs`` = [(class, first segment, end segment, level, peak)] - the run sits at ``level`` with
    one point at ``peak`` (peak None: no point above the run's level)."""
    x = np.full((S, C), base, dtype=np.float32)
    for c, s0, s1, level, peak in runs:
        x[s0:s1, c] = level
        if peak is not None:
            x[(s0 + s1 - 1) // 2, c] = peak
    return x


def handbuilt_cases():
    """[(name, probabilities (B, S, C) float32, frames_num)]: the situations the tag kernel can get wrong.  Frame numbers
    are segment numbers times 4; the two tie pairs are (760, 936) / (892, 980) and (460, 888) / (832, 944) in frames."""
    S, C = 250, 5
    ok = (0.5, 0.9)
    cases = []
    clips = [
        _clip(S, C, [(0, 190, 234) + ok, (1, 223, 245) + ok]),                  # tie: the reference sets "after" -> 2
        _clip(S, C, [(0, 115, 222) + ok, (1, 208, 236) + ok]),                  # tie: the reference sets "while" -> 1
        _clip(S, C, [(2, 10, 20) + ok, (2, 40, 90) + ok, (2, 100, 250) + ok]),  # every segment in one class -> 0
        _clip(S, C, [(0, 0, 30) + ok, (3, 10, 40) + ok, (4, 200, 250) + ok]),   # touches frame 0 and the last segment -> 3
        _clip(S, C, [(0, 20, 60) + ok, (1, 30, 50, 0.5, None)]),                # a low run without a high point: one segment -> 0
        _clip(S, C, []),                                                         # nothing above the low threshold -> 0
        _clip(S, C, [(1, 10, 100) + ok, (3, 20, 90) + ok]),                     # nested, the later one inside -> 1
        _clip(S, C, [(1, 10, 20) + ok, (3, 100, 120) + ok]),                    # one after the other -> 2
    ]
    cases.append(("mixed_1001", np.stack(clips), 4 * S + 1))
    cases.append(("mixed_1000", np.stack(clips), 4 * S))
    # a run that ends in the last segment against one that starts late: the stretch to frames_num decides its duration
    tail = [_clip(S, C, [(0, 240, 250) + ok, (1, 236, 246) + ok])]
    cases.append(("tail_1003", np.stack(tail), 4 * S + 3))
    cases.append(("tail_1000", np.stack(tail), 4 * S))
    # several hundred segments over 3 classes: every other segment on, the classes shifted against one another (B = 1)
    many = np.full((S, C), 0.05, dtype=np.float32)
    for c, off in ((0, 0), (2, 1), (4, 0)):
        many[off::2, c] = 0.9
    cases.append(("many_1001", many[None], 4 * S + 1))
    return cases


def handbuilt_ratio1():
    """Ratio 1 (frames = segments), where connect_ matters: in clip 0 the two class-0 runs are ONE frame apart and merge into
    (2, 12), which holds class 1's (6, 8) -> "while" alone; in clip 1 they are TWO frames apart and stay (2, 6) and (8, 12),
    which class 1's (6, 8) only follows and precedes -> "after" alone.  Never merging turns clip 0 into clip 1's tag, merging
    at a gap of 2 the other way round."""
    S, C = 40, 3
    ok = (0.5, 0.9)
    clips = [_clip(S, C, [(0, 2, 6) + ok, (0, 7, 12) + ok, (1, 6, 8) + ok]),
             _clip(S, C, [(0, 2, 6) + ok, (0, 8, 12) + ok, (1, 6, 8) + ok])]
    return ("ratio1_40", np.stack(clips), S, 1)
