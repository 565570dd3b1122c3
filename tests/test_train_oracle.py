"""CPU tests of the training-step oracle and host logic: the oracle against the gradients the REFERENCE produced
(tests/golden/g8_train.npz), the LR schedule, the dropout hash, and the flat-gradient all-reduce on gloo (world 2)."""
import os
import random

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


@pytest.mark.parametrize("tag", ["ss", "tf"])
def test_oracle_training_step_matches_reference_gradients(golden_dir, state4981, tag):
    from audiocaption_amd import procedural as P
    from oracle import cpu_path as O
    from oracle import train_path as OT
    g8 = dict(np.load(os.path.join(golden_dir, "g8_train.npz")))
    lms = torch.from_numpy(P.synthetic_logmel(4, 1001))
    cnn_attn = O.cnn14_from_logmel(state4981, lms)
    cap, cap_len = torch.from_numpy(g8["cap"]), g8["cap_len"]
    use_cap = g8[f"{tag}_use_cap"].tolist()
    o = OT.train_step_grads(state4981, cnn_attn, O.cnn14_feat_len(g8["wav_len"].tolist()), cap, cap_len, use_cap,
                            p_dec=0.0, p_rnn=0.0, teacher_forcing=(tag == "tf"))
    assert abs(float(o["loss"]) - float(g8[f"{tag}_loss"])) < 2e-5 * float(g8[f"{tag}_loss"])
    top = o["logit"].topk(8, dim=-1)
    assert np.abs(top.values.numpy() - g8[f"{tag}_logit_top_val"]).max() < 5e-5
    if tag == "ss":
        assert np.array_equal(o["seq"].numpy(), g8["ss_seq"])
    for key, grad in o["grads"].items():
        gn = float(g8[f"{tag}_gnorm/{key}"])
        assert abs(float(grad.double().norm()) - gn) < 1e-4 * gn + 1e-12, key
        sample = grad.reshape(-1)[torch.from_numpy(g8[f"sample_idx/{key}"])].numpy()
        assert np.abs(sample - g8[f"{tag}_gsample/{key}"]).max() < 1e-4 * float(grad.abs().max()) + 1e-12, key
    # clip + Adam: the total norm and the update on solid gradients
    keys = list(o["grads"])
    params = {k: state4981[k].clone() for k in keys}
    m1 = {k: torch.zeros_like(v) for k, v in params.items()}
    m2 = {k: torch.zeros_like(v) for k, v in params.items()}
    norm = OT.clip_and_adam(params, o["grads"], m1, m2, 1)
    assert abs(float(norm) - float(g8[f"{tag}_total_norm"])) < 1e-4 * float(norm)
    for k in keys:
        idx = torch.from_numpy(g8[f"sample_idx/{k}"])
        delta = (params[k] - state4981[k]).reshape(-1)[idx].numpy()
        gs = np.abs(g8[f"{tag}_gsample/{k}"])
        solid = gs > 1e-5 * (gs.max() + 1e-30) + 1e-7
        assert np.abs(delta - g8[f"{tag}_delta/{k}"])[solid].max(initial=0.0) < 5e-6, k


def test_dropout_hash_properties():
    from oracle import train_path as OT
    a = OT.drop_mask(OT.op_seed(5, 31), 0, 200000, 0.2)
    b = OT.drop_mask(OT.op_seed(5, 31), 1000, 1000, 0.2)
    assert np.array_equal(a[1000:2000], b)                       # pure function of (seed, index)
    assert set(np.unique(a)) == {np.float32(0.0), np.float32(1.25)}
    assert abs((a > 0).mean() - 0.8) < 0.005
    c = OT.drop_mask(OT.op_seed(6, 31), 0, 200000, 0.2)
    assert 0.6 < (a == c).mean() < 0.76                          # independent streams agree on 0.8^2 + 0.2^2 = 0.68
    assert np.all(OT.drop_mask(1, 0, 100, 0.0) == 1.0)


def test_exponential_decay_scheduler_matches_the_reference_formula():
    from audiocaption_amd.lr_scheduler import ExponentialDecayScheduler
    from oracle import train_path as OT
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=5e-4)
    total, warm = 200, 40          # run.py:249-251: warm-up = iterations // 5
    sched = ExponentialDecayScheduler(opt, total_iters=total, final_lrs=5e-7, warmup_iters=warm)
    lrs = []
    for it in range(total):
        sched.step()               # stepped before the optimiser, once per iteration (run.py:104-105)
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
    # closed form of lr_scheduler.py:22-42 (the constructor's implicit first step makes _step_count start at 1)
    want = [OT.exponential_decay_lr(it + 2, 5e-4, 5e-7, total, warm) for it in range(total)]
    np.testing.assert_allclose(lrs, want, rtol=1e-12)
    assert lrs[warm - 2] == pytest.approx(5e-4) and lrs[0] == pytest.approx(5e-4 * 2 / warm)
    assert lrs[-1] < 6e-7 * 1.2


def _allreduce_worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from audiocaption_amd.train import allreduce_flat_gradients
        flat = torch.arange(1000, dtype=torch.float32) * (rank + 1)
        w = allreduce_flat_gradients(flat)
        # the division by the world size is folded into the clip coefficient (csrc/train.hip clip_coef_kernel)
        norm = float((flat / w).norm())
        coef = min(1.0, 1.0 / (norm + 1e-6)) / w
        # reduce-scatter + all-gather spelling of the same sum: odd lengths (a tail that does not divide), blocking and
        # asynchronous, on random data - bit-equal to the all-reduce
        same = True
        for n in (1001, 7, 1, 4096):
            g = torch.Generator().manual_seed(100 * rank + n)
            x = torch.randn(n, generator=g)
            a, b, c = x.clone(), x.clone(), x.clone()
            allreduce_flat_gradients(a, algo="all_reduce")
            assert allreduce_flat_gradients(b, algo="rs_ag") == world
            allreduce_flat_gradients(c, async_op=True, algo="rs_ag").wait()
            same = same and torch.equal(a, b) and torch.equal(a, c)
        # a numpy copy travels by value: a torch tensor would be shared through a descriptor that this process must stay
        # alive to hand over, and it exits right after the put
        out.put((rank, w, flat.numpy().copy(), coef, same))
    finally:
        dist.destroy_process_group()


def test_flat_gradient_allreduce_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + random.randint(0, 400)
    procs = [ctx.Process(target=_allreduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = torch.arange(1000, dtype=torch.float32) * 3
    for rank, w, flat, coef, same in res:
        assert w == 2 and torch.equal(torch.from_numpy(flat), want)
        avg = want / 2
        assert coef * 2 == pytest.approx(min(1.0, 1.0 / (float(avg.norm()) + 1e-6)))
        assert same, "reduce_scatter + all_gather differs from all_reduce"


def test_scheduled_sampling_ratio_follows_run_py():
    from audiocaption_amd.trainer import ScheduledSampling
    lin = ScheduledSampling(True, "linear", 0.7, 1000)
    r = [lin.step() for _ in range(1000)]
    assert r[0] == pytest.approx(1 - 0.3 / 1000) and r[-1] == pytest.approx(0.7)
    ex = ScheduledSampling(True, "exponential", 0.7, 500)
    r = [ex.step() for _ in range(500)]
    assert r[-1] == pytest.approx(0.01) and r[0] == pytest.approx(0.01 ** (1 / 500))
    off = ScheduledSampling(False)
    assert off.step() == 1.0
    with pytest.raises(Exception):
        ScheduledSampling(True, "cosine")


def test_dict_tokenizer_roundtrip_and_prediction_file(tmp_path):
    import json
    import pickle
    from audiocaption_amd.text import DictTokenizer, write_predictions
    words = {"<pad>": 0, "<start>": 1, "<end>": 2, "<unk>": 3, "a": 4, "dog": 5, "barks": 6}
    p = tmp_path / "vocab.pkl"
    p.write_bytes(pickle.dumps(words))
    tok = DictTokenizer(str(p), max_length=3)
    assert tok.loaded and len(tok) == 7 and (tok.bos, tok.eos, tok.pad) == (1, 2, 0)
    enc = tok(["a dog barks loudly today", "a cat"])
    assert enc["cap"].tolist() == [[1, 4, 5, 6, 2], [1, 4, 3, 2, 0]] and enc["cap_len"].tolist() == [5, 4]
    seqs = np.array([[4, 5, 6, 2, 2, 2], [1, 4, 5, 2, 6, 6], [4, 4, 4, 4, 4, 4]])
    assert tok.decode(seqs) == ["a dog barks", "a dog", "a a a a a a"]
    out = tmp_path / "sub" / "pred.json"
    write_predictions({"x.wav": ["a dog barks"], "y.wav": ["a dog"]}, str(out))
    assert json.loads(out.read_text()) == {"predictions": [{"filename": "x.wav", "tokens": "a dog barks"},
                                                           {"filename": "y.wav", "tokens": "a dog"}]}


def test_dict_tokenizer_vs_reference_fixture(golden_dir, tmp_path):
    """audiocaption_amd.text.DictTokenizer against what the reference's tokenizer returned on the same seeded vocabulary,
    captions (unknown words, truncation to max_length, ragged lengths) and id matrices (rows with / without <start>, an
    <end> in the middle, <pad> / <unk> ids): tests/golden/make_tokenizer_golden.py."""
    import json
    import pickle
    from audiocaption_amd.text import DictTokenizer
    g = json.load(open(os.path.join(golden_dir, "g12_tokenizer.json")))
    p = tmp_path / "vocab.pkl"
    p.write_bytes(pickle.dumps(g["vocab"]))
    tok = DictTokenizer(str(p), max_length=g["max_length"])
    assert len(tok) == g["len"] and tok.state_dict() == g["vocab"]
    enc = tok(g["texts"])
    assert enc["cap"].tolist() == g["cap"] and np.asarray(enc["cap_len"]).tolist() == g["cap_len"]
    assert tok.decode(np.array(g["seqs"])) == g["decoded"]
    grown = DictTokenizer(max_length=g["max_length"])             # built word by word like the reference's vocabulary builder
    for w, i in sorted(g["vocab"].items(), key=lambda kv: kv[1]):
        grown.add_word(w)
    assert grown.state_dict() == g["vocab"] and grown.decode(np.array(g["seqs"])) == g["decoded"]


def test_dict_tokenizer_keeps_the_references_costs_and_errors():
    """text_tokenizer.py:30-34 / :56-68: ``add_word`` is O(1) (a vocabulary of 20 k words builds in well under a second),
    ``idx2word`` is a plain dict kept in step with ``word2idx``, an id outside the vocabulary that ``decode`` has to look up
    raises KeyError like ``idx2word[token_id]`` does (ids behind the first <end> are never looked up), an empty list encodes
    to empty arrays."""
    import time
    from audiocaption_amd.text import DictTokenizer
    tok = DictTokenizer()
    t0 = time.perf_counter()
    for i in range(20000):
        tok.add_word(f"w{i}")
    assert time.perf_counter() - t0 < 1.0 and len(tok) == 20004
    assert tok.idx2word is tok.idx2word and tok.idx2word[4] == "w0" and tok.idx2word[20003] == "w19999"
    assert tok.decode([[1, 4, 5, 2, 999999]]) == ["w0 w1"]
    with pytest.raises(KeyError):
        tok.decode([[1, 4, 999999, 2]])
    with pytest.raises(KeyError):
        tok.decode([[1, -7, 2]])
    tok.add_word("late")                                  # the decode table follows later additions
    assert tok.decode([[20004, 2]]) == ["late"]
    empty = tok([])
    assert empty["cap"].shape == (0, 0) and empty["cap_len"].shape == (0,)


def test_swa_averager_on_cpu_tensors():
    from audiocaption_amd.trainer import SwaAverager
    m = torch.nn.Sequential(torch.nn.Linear(4, 3), torch.nn.BatchNorm1d(3))
    swa = SwaAverager(m)
    snaps = []
    for k in range(4):
        with torch.no_grad():
            for p in m.parameters():
                p.add_(k + 1.0)
        snaps.append({n: t.detach().clone() for n, t in m.state_dict().items()})
        swa.update_parameters(m)
    sd = swa.state_dict()
    assert set(sd) == set(m.state_dict())
    for n in ("0.weight", "0.bias", "1.weight"):
        want = sum(s[n] for s in snaps) / 4
        assert torch.allclose(sd[n], want, atol=1e-6)


def test_with_next_pairs_every_batch_with_its_successor():
    from audiocaption_amd.trainer import with_next
    assert list(with_next([])) == [] and list(with_next(["a"])) == [("a", None)]
    assert list(with_next(iter("abc"))) == [("a", "b"), ("b", "c"), ("c", None)]
