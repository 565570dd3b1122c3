#!/usr/bin/env python
"""SHA-256 of what the decode step (csrc/decoder.hip decoder_step / classifier_step) computes on each of its routes: one
line per case, to be compared between two builds of the library on the same machine (profiles/decoder_route_digest_*.txt).
A refactor of the host code that issues the step's launches must leave every line as it was.

usage: decoder_route_digest.py                      every case, one after another, each in a child process of its own
       decoder_route_digest.py --case NAME [--dump FILE.npz]     one case in this process (the switches come from the
                                                                 environment); --dump also saves the hashed arrays

The weights are procedural (audiocaption_amd.procedural through the draws of tests/_decoder_shapes.py), the shapes the
smallest that reach each branch.  A case is a fresh process because four of the switches are latched on first use
(csrc/decoder.hip resolve_route).  Greedy and teacher-forced cases hash seq / logit / sampled_logprob / embed, beam cases
top_val / top_idx of every step."""
import argparse
import ctypes
import hashlib
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

# A case's own work is a few seconds; the limit also covers a first import of torch and the load of the code objects.
CHILD_SECONDS = 20
SWITCHES = ("AUDIOCAPTION_DEC_ROW", "AUDIOCAPTION_DEC_WIDE_MIN", "AUDIOCAPTION_DEC_HYBRID", "AUDIOCAPTION_DEC_CLS_GEMM",
            "AUDIOCAPTION_DEC_NTB", "AUDIOCAPTION_DEC_CLS_NTB", "AUDIOCAPTION_DEC_WIDE_CLS_NTB", "AUDIOCAPTION_BEAM_TOPK")

# (case, switches): the order of the output lines
RUNS = [
    ("S0-greedy", {}),                                        # fused per-row route, dec_row2_kernel
    ("S0-greedy", {"AUDIOCAPTION_DEC_ROW": "split"}),         # fused per-row route, two dec_row_kernel launches
    ("S0-greedy", {"AUDIOCAPTION_DEC_ROW": "gemm"}),          # general route at the fused shape
    ("S2-greedy", {}),                                        # general route, 3 layers (odd number of swaps), hd 32
    ("S4-forward", {}),                                       # teacher forcing, dim_ff of four K chunks
    ("S0-beam", {}),                                          # row_div 3, both cache sets, ac_trm_beam_reorder
    ("S0-528", {}),                                           # ntb 2, LayerNorm + ac_gemm classifier, scratch classifier
    ("S0-528", {"AUDIOCAPTION_DEC_CLS_GEMM": "0"}),
    ("S0-528", {"AUDIOCAPTION_DEC_WIDE_MIN": "128"}),
    ("S0-528", {"AUDIOCAPTION_DEC_HYBRID": "1"}),
    ("S0-130", {"AUDIOCAPTION_DEC_WIDE_MIN": "128"}),         # wide route, rows no multiple of 32
    ("S0-segments", {}),                                      # struct Live: one of two segments ends early
]


def _greedy(S, state_args, emb, lens, max_length):
    import torch
    dec = S.product_model(state_args[0], S.diverse_state(*state_args)).decoder
    dev = torch.device("cuda:0")
    if isinstance(emb, list):
        emb = [e.to(dev) for e in emb]
    else:
        emb = emb.to(dev)
    out = dec.greedy(emb, lens, max_length, S.START, S.END, S.PAD, mode="chain")
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in ("seq", "logit", "sampled_logprob", "embed")}


def _beam_chain(S, state_args, emb, lens, beam, steps):
    """The launches of TransformerModel._beam_begin's ``segment`` for steps 0 .. steps - 1, keeping every step's picks."""
    import torch
    from audiocaption_amd import _lib
    from audiocaption_amd.kernels import check, ptr, stream, upload
    dec = S.product_model(state_args[0], S.diverse_state(*state_args)).decoder
    lib = _lib.load()
    dev = torch.device("cuda:0")
    emb = emb.to(dev)
    B, Tm, _ = emb.shape
    R, V, ld, cap = B * beam, dec.vocab_size, steps + 1, beam * steps
    i32, f32 = dict(device=dev, dtype=torch.int32), dict(device=dev, dtype=torch.float32)
    w = ctypes.byref(dec.weights())
    memkv = dec.memory(emb)
    mem_len = upload(lens, dev, torch.int32)
    ws = dec.workspace(R, steps, dev)
    tok = [torch.full((R, ld), S.END, **i32) for _ in range(2)]
    tok[0][:, 0] = S.START
    mask = torch.zeros(R, ld, device=dev, dtype=torch.uint8)
    cum, active, done_cnt = torch.zeros(R, **f32), torch.ones(B, **i32), torch.zeros(B, **i32)
    done_seq, done_score = torch.zeros(B, cap, steps, **i32), torch.zeros(B, cap, **f32)
    src_row, n_active = torch.zeros(R, **i32), torch.full((1,), B, **i32)
    top_val, top_idx = torch.empty(B, beam, **f32), torch.empty(B, beam, **i32)
    out = {}
    for t in range(steps):
        check(lib.ac_trm_beam_step(w, ptr(memkv), ptr(mem_len), B, beam, Tm, steps, t, 1.0, ptr(tok[t & 1]), ptr(mask),
                                   ptr(cum), ptr(top_val), ptr(top_idx), ptr(ws), stream()), "ac_trm_beam_step")
        check(lib.ac_trm_beam_update(ptr(top_val), ptr(top_idx), ptr(tok[t & 1]), ptr(tok[(t + 1) & 1]), ptr(mask), ptr(cum),
                                     ptr(active), ptr(done_cnt), ptr(done_seq), ptr(done_score), ptr(src_row), ptr(n_active),
                                     B, beam, V, steps, t, S.END, S.PAD, cap, stream()), "ac_trm_beam_update")
        if t + 1 < steps:
            check(lib.ac_trm_beam_reorder(w, R, steps, t, ptr(src_row), ptr(ws), stream()), "ac_trm_beam_reorder")
        torch.cuda.synchronize()
        out[f"top_val{t}"], out[f"top_idx{t}"] = top_val.cpu().numpy(), top_idx.cpu().numpy()
    return out


def s0_greedy_inputs(S):
    """Rows 0-2 of the 48-step greedy draw of S0 (tests/_decoder_shapes.py GREEDY_CASES), 12 steps: a prefix, row by row
    and step by step, of ``S.greedy_reference("S0", 5)``."""
    emb, lens = S._search_memory("S0", S.GREEDY_LENS, S.GREEDY_TM, 5)
    return ("S0", 5), emb[:3], lens[:3], 12


def run_case(name):
    """{array name: numpy array} of one case, in the order they are hashed."""
    import torch
    import _decoder_shapes as S
    if name == "S0-greedy":
        return _greedy(S, *s0_greedy_inputs(S))
    if name == "S2-greedy":
        emb, lens = S._search_memory("S2", S.GREEDY_LENS, S.GREEDY_TM, 7)
        return _greedy(S, ("S2", 7), emb[:3], lens[:3], 12)
    if name == "S4-forward":
        inp = S.tf_inputs("S4", 8, S.TF_TM["S4"])
        dec = S.product_model("S4", S.plain_state("S4")).decoder
        out = dec({"word": inp["word"].cuda(), "attn_emb": inp["attn_emb"].cuda(), "attn_emb_len": inp["attn_emb_len"],
                   "cap_padding_mask": inp["cap_padding_mask"].cuda()})
        torch.cuda.synchronize()
        return {k: out[k].cpu().numpy() for k in ("logit", "embed")}
    if name == "S0-beam":
        emb, lens = S._search_memory("S0", S.BEAM_LENS, S.BEAM_TM, 5)
        return _beam_chain(S, ("S0", 5), emb, lens, 3, 6)
    if name == "S0-528":
        # 528 rows twice: a greedy chain (the classifier writes `embed`) and 176 clips x beam 3 (it has only scratch)
        lens = torch.arange(528) % 20 + 1
        out = _greedy(S, ("S0", 5), S.memory("S0", 528, 20, 5), lens, 2)
        out.update(_beam_chain(S, ("S0", 5), S.memory("S0", 176, 20, 6), lens[:176], 3, 2))
        return out
    if name == "S0-130":
        return _greedy(S, ("S0", 5), S.memory("S0", 130, 20, 5), torch.arange(130) % 20 + 1, 3)
    if name == "S0-segments":
        # the early-stop draw of S0 (STOP_CASES): rows 0 and 1 emit <end> at steps 9 and 3, rows 2 and 3 never - as two
        # segments of two rows the first ends after step 9 and the chain's later launches skip its rows
        sid, seed, beta = S.STOP_CASES["S0"]
        emb, lens = S._search_memory(sid, S.GREEDY_LENS, S.GREEDY_TM, seed)
        return _greedy(S, (sid, seed, beta), [emb[:2], emb[2:]], [lens[:2], lens[2:]], 16)
    raise SystemExit(f"unknown case {name!r}")


def label(name, env):
    return name + "".join(f" {k[len('AUDIOCAPTION_'):]}={v}" for k, v in env.items())


def child(name, dump):
    import numpy as np
    arrays = run_case(name)
    h = hashlib.sha256()
    for k, v in arrays.items():
        h.update(np.ascontiguousarray(v).tobytes())
    if dump:
        np.savez(dump, **arrays)
    env = {k: os.environ[k] for k in SWITCHES if k in os.environ}
    print(f"{label(name, env):44s} {h.hexdigest()}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case")
    ap.add_argument("--dump", metavar="FILE.npz")
    args = ap.parse_args()
    if args.case:
        return child(args.case, args.dump)
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    base["AUDIOCAPTION_DECODE_GRAPH"] = "0"
    for name, env in RUNS:
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_SECONDS), sys.executable, os.path.abspath(__file__), "--case", name],
                           env={**base, **env}, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            raise SystemExit(f"{label(name, env)}: exit status {r.returncode}; stopping")


if __name__ == "__main__":
    main()
