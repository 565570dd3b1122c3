"""Development probe: the launch trace of the Cnn14 encoder (audiocaption_amd/cnn_encoder.py), the sibling of
tools/train_launch_trace.py for the frozen network that tool leaves out.  Every call into the HIP library that a set of
eager encoder calls makes, in issue order, with its arguments, plus the ``CONV_LAUNCH_HOOK`` events, over every conv tier
and every routing switch.  Two versions of cnn_encoder.py / kernels.py that print the same SHA-256 per case issue the same
launches, in the same order, with the same arguments; the second hash of a case (the returned bytes) says that they also
computed the same bits.

The cases run ``--passes`` times (default 2): the launch hashes are those of the first pass; a case whose OUTPUT hash is
not the same in every pass is marked "NOT run-to-run stable" (its bits cannot be compared between two versions either).
Pointer ordinals restart with every case, so that one case's hash does not depend on the cases before it."""
import argparse
import contextlib
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import audiocaption_amd as A
from audiocaption_amd import _lib, cnn_encoder as CE, kernels as K, procedural as Pr
from launch_trace import TracingLib, ordinals, trace

ap = argparse.ArgumentParser()
ap.add_argument("--vocab", type=int, default=4368)
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--out", default="encoder_launch_trace.txt")
ap.add_argument("--records", default=None, help="also write every record of the first pass to this file")
args = ap.parse_args()

TIERS = ("wino43", "wino1d", "bf16x3", "bf16x3_lds", "f16x2", "winograd", "direct")
SR = 32000
L10 = 10 * SR

model = A.init_model_from_config(A.cnn14rnn_trm_config(args.vocab), print_fn=lambda s: None)
model.load_state_dict(Pr.to_torch(Pr.cnn14rnn_trm_state(args.vocab)), strict=True)
model = model.to("cuda:0").eval()
cnn = model.encoder.cnn
_lib._lib = TracingLib(_lib.load())   # what every later _lib.load() returns
K.CONV_LAUNCH_HOOK = lambda phase, info: trace.append(f"hook {phase} {sorted(info.items())}")
seed_dev = torch.full((1,), 12345, device="cuda:0", dtype=torch.int64)


_noise = {}


def wavs(B, seconds=(10.0,)):
    """(wav (B, 10 s) on the device, wav_len): clip i lasts seconds[i % len(seconds)], zero-padded."""
    if B not in _noise:
        _noise[B] = Pr.synthetic_wav(B, L10, seed=1)
    wav = _noise[B].copy()
    lens = [int(seconds[i % len(seconds)] * SR) for i in range(B)]
    for i, n in enumerate(lens):
        wav[i, n:] = 0.0
    return torch.from_numpy(wav).cuda(), lens


@contextlib.contextmanager
def switched(env=None, module=None, attrs=None):
    """Environment variables, module globals of cnn_encoder and attributes of the encoder, restored afterwards."""
    env, module, attrs = env or {}, module or {}, attrs or {}
    saved = ({k: os.environ.get(k) for k in env}, {k: getattr(CE, k) for k in module}, {k: getattr(cnn, k) for k in attrs})
    os.environ.update(env)
    for k, v in module.items():
        setattr(CE, k, v)
    for k, v in attrs.items():
        setattr(cnn, k, v)
    try:
        yield
    finally:
        for k, v in saved[0].items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        for k, v in saved[1].items():
            setattr(CE, k, v)
        for k, v in saved[2].items():
            setattr(cnn, k, v)


def forward(algo, B, seconds=(10.0,), skip_fc=True, env=None, module=None, attrs=None):
    def run():
        wav, lens = wavs(B, seconds)
        with switched(env, module, dict(attrs or {}, conv_algo=algo)):
            out = cnn({"wav": wav, "wav_len": lens}, skip_fc=skip_fc)
        return [out["attn_emb"]] + ([out["fc_emb"]] if "fc_emb" in out else [])
    return run


def train(algo, B, dropout=True):
    def run():
        wav, _ = wavs(B)
        with switched(attrs={"conv_algo": algo}):
            return [cnn.encode(wav, dropout=(0.2, 40, seed_dev.data_ptr()) if dropout else None, train=True)]
    return run


RAGGED = (10.0, 7.3, 5.0, 3.5)
CASES = []
for t in TIERS:
    CASES.append((f"{t} forward 64x10s skip_fc", forward(t, 64)))
    CASES.append((f"{t} forward 1x10s fc_emb", forward(t, 1, skip_fc=False)))
for t in ("wino43", "wino1d"):
    for exact in "01":
        for skip in "10":
            CASES.append((f"{t} ragged 4 clips RAGGED_EXACT={exact} SKIP_DEAD_ROWS={skip}",
                          forward(t, 4, RAGGED, env={"AUDIOCAPTION_RAGGED_EXACT": exact, "AUDIOCAPTION_SKIP_DEAD_ROWS": skip})))
    CASES.append((f"{t} ragged 4 clips W43_MIN_WORKGROUPS=1", forward(t, 4, RAGGED, module={"W43_MIN_WORKGROUPS": 1})))
CASES.append(("f16x2 4 clips, one of 2 s", forward("f16x2", 4, (10.0, 10.0, 2.0, 10.0))))
CASES.append(("f16x2 64x10s f16x2_block6=f16x2", forward("f16x2", 64, attrs={"f16x2_block6": "f16x2"})))
for name, sw in (("FUSE_BLOCK1=0", {"env": {"AUDIOCAPTION_FUSE_BLOCK1": "0"}}), ("W1_SPLITK=0", {"env": {"AUDIOCAPTION_W1_SPLITK": "0"}}),
                 ("W1_C64=0", {"env": {"AUDIOCAPTION_W1_C64": "0"}}), ("BLOCK1_CONV1=valu", {"module": {"BLOCK1_CONV1": "valu"}}),
                 ("SKINNY=False", {"module": {"SKINNY": False}})):
    for B in (1, 64):
        CASES.append((f"wino43 {name} {B}x10s", forward("wino43", B, **sw)))
for t in ("wino43", "wino1d", "bf16x3", "winograd", "f16x2"):
    for B in (4, 32):
        CASES.append((f"{t} train dropout {B}x10s", train(t, B)))
CASES.append(("wino43 train no dropout 4x10s", train("wino43", 4, dropout=False)))


def sha(data):
    return hashlib.sha256(data).hexdigest()


launch, bits, records = {}, {}, []
for p in range(args.passes):
    for name, run in CASES:
        del trace[:]
        ordinals.clear()
        outs = run()
        torch.cuda.synchronize()
        text = "\n".join(trace) + "\n"
        out_hash = sha(b"".join(o.float().cpu().numpy().tobytes() for o in outs))
        if p == 0:
            launch[name] = (len(trace), sha(text.encode()))
            records.append(f"# {name}\n{text}")
        bits.setdefault(name, []).append(out_hash)
        del outs

lines = []
for name, _ in CASES:
    stable = len(set(bits[name])) == 1
    lines.append(f"{name}: {launch[name][0]} records, launches {launch[name][1]}, output "
                 f"{bits[name][0] if stable else 'NOT run-to-run stable: ' + ' / '.join(bits[name])}")
lines.append(f"total: {len(CASES)} cases x {args.passes} passes, launches {sha(''.join(records).encode())}, outputs "
             f"{sha(''.join(b[0] for b in bits.values()).encode())}")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
if args.records:
    with open(args.records, "w") as f:
        f.write("".join(records))
print("\n".join(lines))
