"""Timing of the HTS-AT encoder (audiocaption_amd/htsat.py, csrc/htsat.hip) next to Cnn14 + bi-GRU on the same batch.

  python tools/htsat_bench.py [--out FILE] [--reps 9] [--clips 64] [--profile]     (default FILE: profiles/htsat_bench.json)

64 clips x 10 s at 32 kHz (1001 frames: the bicubic stretch runs).  Timed, in one process and on the same waveforms:
the Htsat encoder alone (``model.encoder(input_dict)``), the Htsat captioner through the blocking call (encoder + greedy
decode, max_length 20), and the same two figures for the Cnn14 + bi-GRU captioner (``cnn14rnn_trm_config``), the
reference point of THIS run.  Also counted: the library launches of one encoder call (the entry points of the C ABI it goes
through; torch's own launches - the output allocations - are not kernels).

Every number is the median of ``--reps`` (>= 5) timed calls after three warm-up calls of the same shape, each timed with
device events around the whole call on the current stream; a greedy call ends in the device-to-host copy of the token
ids, an encoder call in an event synchronise, so the events bracket finished work.  ``--profile``: warm up and run three
encoder calls only, no timing - the run to put under ``rocprofv3 --kernel-trace --stats`` on its own.
Prints one JSON object."""
import argparse
import collections
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

V, L, SECONDS = 4368, 20, 10


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


class CountCalls:
    """Wraps the loaded library: counts the calls of every entry point while active."""

    def __init__(self, lib):
        self.lib, self.counts = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("ac_"):
            return fn

        def call(*a):
            self.counts[name] += 1
            return fn(*a)
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "htsat_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    reps, B = max(5, args.reps), args.clips
    if not torch.cuda.is_available():
        raise SystemExit("tools/htsat_bench.py measures on the GPU; there is none here")
    import audiocaption_amd as A
    from audiocaption_amd import _lib, build
    from audiocaption_amd import procedural as P
    build.build()
    n = SECONDS * 32000
    wav = torch.from_numpy(P.synthetic_wav(B, n)).cuda()
    inp = {"wav": wav, "wav_len": [n] * B, "specaug": False}
    req = dict(inp, mode="inference", sample_method="greedy", max_length=L)

    htsat = A.init_model_from_config(A.htsat_trm_config(V), print_fn=lambda s: None)
    htsat.load_state_dict(dict(htsat.state_dict(), **P.to_torch(P.htsat_trm_state(V))), strict=True)
    htsat = htsat.eval().cuda()
    if args.profile:
        for _ in range(6):
            htsat.encoder(inp)
        torch.cuda.synchronize()
        print(json.dumps({"profile_run": True, "encoder_calls": 6, "clips": B}))
        return

    res = {"shape": {"clips": B, "seconds": SECONDS, "frames": n // 320 + 1, "vocab": V, "max_length": L, "reps": reps},
           "device": torch.cuda.get_device_name(0), "htsat": {}, "cnn14_bigru": {}}
    res["htsat"]["encoder"] = timed(lambda: htsat.encoder(inp), reps)
    res["htsat"]["encoder_greedy"] = timed(lambda: htsat(req)["seq"], reps)
    counter = CountCalls(_lib.load())
    real = _lib._lib
    _lib._lib = counter
    try:
        htsat.encoder(inp)
    finally:
        _lib._lib = real
    res["htsat"]["library_launches_per_encoder_call"] = sum(counter.counts.values())
    res["htsat"]["launches_by_entry_point"] = dict(counter.counts)

    cnn = A.init_model_from_config(A.cnn14rnn_trm_config(V), print_fn=lambda s: None)
    cnn.load_state_dict(P.to_torch(P.cnn14rnn_trm_state(V)), strict=True)
    cnn = cnn.eval().cuda()
    res["cnn14_bigru"]["encoder"] = timed(lambda: cnn.encoder(inp), reps)
    res["cnn14_bigru"]["encoder_greedy"] = timed(lambda: cnn(req)["seq"], reps)
    res["htsat_encoder_over_cnn14_bigru_encoder"] = round(res["htsat"]["encoder"]["ms"] / res["cnn14_bigru"]["encoder"]["ms"], 3)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
