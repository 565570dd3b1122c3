"""CPU tests of the attention-GRU training path: the restatement of tests/_attn_gru_train_ref.py against the steps the
REFERENCE ran (tests/golden/g22_attn_gru_train.npz), the dropout site code, the C ABI's new rows and the refusals the
entry points make before any launch (nothing here needs a GPU)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _attn_gru_train_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGIT_BAR, LOSS_BAR, GRAD_BAR = 2e-5, 2e-5, 1e-4


@pytest.fixture(scope="module")
def g22():
    return R.load_g22()


def _check(g22, case, idx_prefix, res, grads):
    top = res["logit"].topk(8, dim=-1)
    want = g22[f"{case}_logit_top_val"]
    assert float(np.abs(top.values.numpy() - want).max()) < LOGIT_BAR * float(np.abs(want).max())
    assert np.array_equal(top.indices.numpy()[..., 0], g22[f"{case}_logit_top_idx"][..., 0])
    assert np.array_equal(res["seq"].numpy(), g22[f"{case}_seq"])
    assert abs(float(res["loss"]) - float(g22[f"{case}_loss"])) < LOSS_BAR * float(g22[f"{case}_loss"])
    assert set(grads) == {k.split("/", 1)[1] for k in g22 if k.startswith(f"{case}_gnorm/")}
    for key, grad in grads.items():
        gn = float(g22[f"{case}_gnorm/{key}"])
        assert abs(float(grad.double().norm()) - gn) < GRAD_BAR * gn, key
        assert abs(float(grad.double().sum()) - float(g22[f"{case}_gsum/{key}"])) < GRAD_BAR * gn * np.sqrt(grad.numel()), key
        sample = grad.reshape(-1)[torch.from_numpy(g22[f"{idx_prefix}_sample_idx/{key}"])].numpy()
        assert float(np.abs(sample - g22[f"{case}_gsample/{key}"]).max()) < GRAD_BAR * float(grad.abs().max()), key
    total = np.sqrt(sum(float(g.double().norm()) ** 2 for k, g in grads.items() if k not in ("attn_emb", "fc_emb")))
    assert abs(total - float(g22[f"{case}_total_norm"])) < GRAD_BAR * float(g22[f"{case}_total_norm"])


@pytest.mark.parametrize("kind,tag", [("t", "tf"), ("t", "ss"), ("p", "tf"), ("p", "ss")])
def test_decoder_restatement_vs_reference(g22, kind, tag):
    temporal = kind == "t"
    case = f"small_{kind}_{tag}"
    sd = R.small_state(temporal, *g22[f"small_{kind}_recipe"])
    mem, lens, fc, tags = R.small_inputs()
    cap, cap_len = R.small_caption()
    use_cap = g22[f"{case}_use_cap"].tolist()
    res = R.decoder_step_grads(sd, mem, lens, fc, cap, cap_len, use_cap, tags if temporal else None)
    assert float((res["attn_weight"] - torch.from_numpy(g22[f"{case}_attn_weight"])).abs().max()) < LOGIT_BAR
    grads = {"decoder." + k: v for k, v in res["grads"].items()}
    grads.update(attn_emb=res["d_attn_emb"], fc_emb=res["d_fc_emb"])
    _check(g22, case, f"small_{kind}", res, grads)
    for b, n in enumerate(R.SMALL_LENS):
        assert not res["d_attn_emb"][b, n:].any()
    if tag == "ss":     # the fixture's gates: a teacher-forced and a fed-back step, no near-tie on a fed-back one
        steps = use_cap[1:] if temporal else use_cap
        assert any(steps) and not all(steps)
        assert float(R.fed_back_gaps(res["gap"], use_cap, temporal).min()) >= 1e-4


def test_model_restatement_vs_reference(g22):
    state = R.pub_state(*g22["pub_recipe"])
    attn = R.pub_cnn_attn()
    assert abs(float(attn.double().sum()) - float(g22["pub_attn_sum"])) < 1e-6 * float(g22["pub_attn_sum"])
    cap, cap_len = R.pub_caption()
    use_cap = g22["pub_ss_use_cap"].tolist()
    res = R.model_step_grads(state, attn, torch.tensor(R.PUB_LENS), cap, cap_len, use_cap, torch.tensor(R.PUB_TAGS))
    _check(g22, "pub_ss", "pub", res, res["grads"])
    assert float(R.fed_back_gaps(res["gap"], use_cap, True).min()) >= 1e-4


def test_dropout_masks_are_the_projects(g22):
    """The site code is train.OP_BAH_IN; the mask of step t is the counter hash at (t * B + clip) * E + feature."""
    from audiocaption_amd import train
    from oracle import train_path as OT
    assert R.OP_BAH_IN == train.OP_BAH_IN
    codes = [v for k, v in vars(train).items() if k.startswith("OP_") and isinstance(v, int)]
    assert len(codes) == len(set(codes))
    B, E, p = 5, 64, 0.2
    m = R.in_dropout_mask(9, 3, B, E, p)
    flat = OT.drop_mask(OT.op_seed(9, train.OP_BAH_IN), 0, 4 * B * E, p).reshape(4, B, E)
    assert np.array_equal(m.numpy(), flat[3]) and set(np.unique(flat)) == {np.float32(0.0), np.float32(1.0) / np.float32(0.8)}
    sd = R.small_state(True, *g22["small_t_recipe"])
    mem, lens, fc, tags = R.small_inputs()
    cap, _ = R.small_caption()
    use_cap = g22["small_t_ss_use_cap"].tolist()
    a = R.decoder_forward(sd, mem, lens, fc, cap, use_cap, tags, p=0.2, base_seed=1)["logit"]
    b = R.decoder_forward(sd, mem, lens, fc, cap, use_cap, tags, p=0.2, base_seed=2)["logit"]
    assert not torch.equal(a, b)


def test_abi_rows_and_build_list():
    from audiocaption_amd import _lib, build
    assert "attn_gru_train.hip" in build.SOURCES and _lib.ABI_VERSION == 2
    header = open(os.path.join(REPO, "include", "audiocaption_hip.h")).read()
    assert "#define AC_ABI_VERSION 2" in header
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("ac_bah_train_workspace_floats", "ac_bah_train_forward", "ac_bah_train_backward", "ac_bah_mean_lens_bwd"):
        proto = re.search(r"\b(int|long)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert proto, name
        res, args = _lib.SIGNATURES[name]
        assert res is (ctypes.c_long if proto.group(1) == "long" else ctypes.c_int)
        assert len([a for a in proto.group(2).split(",")]) == len(args), name
    fields = re.search(r"typedef struct \{([^}]*)\} ac_bah_grads;", header).group(1)
    assert [f.strip(" *\n") for f in fields.replace("float", "").replace(";", "").split(",")] == \
        [n for n, _ in _lib.AcBahGrads._fields_]
    # the gradient struct names the weight struct's tensors, in its order
    assert [n for n, _ in _lib.AcBahGrads._fields_] == [n for n, t in _lib.AcBahWeights._fields_ if t is ctypes.c_void_p]


def test_entry_points_refuse_before_touching_the_device():
    """AC_ERR_ARG / -1 for a bad width, Tm 4096 and null pointers (nothing is launched on a machine without a GPU)."""
    from audiocaption_amd import _lib, build
    build.build()
    lib = _lib.load()
    keep = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(keep))      # a non-null address no accepted call ever reaches
    w = _lib.AcBahWeights()
    w.emb_dim, w.d_model, w.attn_size, w.attn_emb_dim, w.fc_emb_dim, w.vocab, w.n_tags = 64, 128, 96, 160, 96, 517, 4
    for name, t in _lib.AcBahWeights._fields_:
        if t is ctypes.c_void_p:
            setattr(w, name, p)
    assert lib.ac_bah_train_workspace_floats(ctypes.byref(w), 5, 70, 8) > 0
    assert lib.ac_bah_train_workspace_floats(ctypes.byref(w), 5, 2048, 8) > 0
    assert lib.ac_bah_train_workspace_floats(ctypes.byref(w), 5, 4096, 8) == -1
    assert lib.ac_bah_train_workspace_floats(ctypes.byref(w), 5, 70, 0) == -1
    bad = _lib.AcBahWeights.from_buffer_copy(w)
    bad.attn_size = 100
    assert lib.ac_bah_train_workspace_floats(ctypes.byref(bad), 5, 70, 8) == -1
    big = _lib.AcBahWeights.from_buffer_copy(w)
    big.vocab = 16385
    assert lib.ac_bah_train_workspace_floats(ctypes.byref(big), 5, 70, 8) == -1
    coins = (ctypes.c_int * 8)(*([1] * 8))
    fwd = [ctypes.byref(w), p, p, p, p, 9, coins, p, 5, 70, 8, 1, 0.0, 0, None, p, p, p, p, p, p, p, None]
    for i, v in ((0, ctypes.byref(bad)), (1, None), (2, None), (3, None), (4, None), (5, 7), (6, None), (7, None), (9, 4096),
                 (12, -0.1), (12, 1.0), (15, None), (16, None), (19, None), (21, None)):
        args = list(fwd)
        args[i] = v
        assert lib.ac_bah_train_forward(*args) == _lib.AC_ERR_ARG, i
    g = _lib.AcBahGrads()
    for name, _ in _lib.AcBahGrads._fields_:
        setattr(g, name, p)
    no_temb = _lib.AcBahGrads.from_buffer_copy(g)
    no_temb.temb = None
    bwd = [ctypes.byref(w), ctypes.byref(g), p, p, p, p, 5, 70, 8, 0.0, 0, None, p, p, p, None]
    for i, v in ((0, ctypes.byref(bad)), (1, None), (1, ctypes.byref(no_temb)), (2, None), (5, None), (7, 4096), (8, 0),
                 (12, None), (13, None), (14, None)):
        args = list(bwd)
        args[i] = v
        assert lib.ac_bah_train_backward(*args) == _lib.AC_ERR_ARG, i
    assert lib.ac_bah_mean_lens_bwd(None, p, p, 2, 3, 64, 64, None) == _lib.AC_ERR_ARG
    assert lib.ac_bah_mean_lens_bwd(p, p, p, 2, 3, 32, 64, None) == _lib.AC_ERR_ARG


def test_train_mode_over_another_encoder_still_raises():
    import audiocaption_amd as A
    dec = A.rnn_decoder.TemporalBahAttnDecoder(dropout=0.5, **R.SMALL)
    model = A.TemporalSeq2SeqAttnModel(torch.nn.Identity(), dec)
    with pytest.raises(NotImplementedError, match="train"):
        model({"mode": "train"})
    from audiocaption_amd.train_attn_gru import AttnGruTrainEngine
    with pytest.raises(NotImplementedError):
        AttnGruTrainEngine(model)
