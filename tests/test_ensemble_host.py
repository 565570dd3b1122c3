"""EnsembleModel without a GPU: what the constructor refuses, that it only decodes, and the attributes
``hf_wrapper.CaptioningModel`` reads from the model it wraps."""
import pytest
import torch
import torch.nn as nn

import audiocaption_amd as A
from audiocaption_amd import _lib
from audiocaption_amd.ensemble import EnsembleModel


def _member(vocab=50, **kw):
    dec = A.TransformerDecoder(emb_dim=64, vocab_size=vocab, fc_emb_dim=32, attn_emb_dim=32, dropout=0.2, nhead=2, nlayers=1,
                               dim_feedforward=64)
    return A.TransformerModel(nn.Identity(), dec, **kw)


def test_exported_from_the_package():
    assert A.EnsembleModel is EnsembleModel and "EnsembleModel" in A.__all__


def test_constructor_refuses_what_cannot_be_decoded_together():
    with pytest.raises(ValueError, match="at least one"):
        EnsembleModel([])
    with pytest.raises(ValueError, match="vocab_size"):
        EnsembleModel([_member(50), _member(51)])
    with pytest.raises(ValueError, match="AC_ENS_MAX"):
        EnsembleModel([_member() for _ in range(_lib.AC_ENS_MAX + 1)])
    longer = _member()
    longer.max_length = 30   # only one max_length can be the ensemble's default
    with pytest.raises(ValueError, match="max_length"):
        EnsembleModel([_member(), longer])
    odd = _member()
    odd.end_idx = 3          # an instance whose <end> differs from the class default of the others
    with pytest.raises(ValueError, match="start_idx / end_idx / pad_idx"):
        EnsembleModel([_member(), odd])

    class OtherDecoder(nn.Module):
        vocab_size = 50

    class OtherModel(nn.Module):
        vocab_size, start_idx, end_idx, pad_idx, max_length = 50, 1, 2, 0, 20

        def __init__(self):
            super().__init__()
            self.decoder = OtherDecoder()

    with pytest.raises(NotImplementedError, match="TransformerDecoder"):
        EnsembleModel([_member(), OtherModel()])


def test_attributes_and_members():
    members = [_member(), _member(), _member()]
    ens = EnsembleModel(members)
    assert (ens.vocab_size, ens.start_idx, ens.end_idx, ens.pad_idx, ens.max_length) == (50, 1, 2, 0, 20)
    assert isinstance(ens.models, nn.ModuleList) and list(ens.models) == members
    assert sum(p.numel() for p in ens.parameters()) == 3 * sum(p.numel() for p in members[0].parameters())
    EnsembleModel([_member() for _ in range(_lib.AC_ENS_MAX)])   # the limit itself is accepted


def test_training_mode_raises():
    ens = EnsembleModel([_member()])
    with pytest.raises(NotImplementedError, match="inference"):
        ens({"mode": "train", "wav": torch.zeros(1, 100), "wav_len": [100]})


def test_decode_checks_its_arguments_before_touching_the_device():
    ens = EnsembleModel([_member(), _member()])
    enc = {"attn_emb": torch.zeros(2, 5, 32), "attn_emb_len": torch.tensor([5, 5])}
    with pytest.raises(ValueError, match="encoder outputs"):
        ens.decode([enc])
    with pytest.raises(ValueError, match="batch size"):
        ens.decode([enc, {"attn_emb": torch.zeros(3, 5, 32), "attn_emb_len": torch.tensor([5, 5, 5])}])
    with pytest.raises(NotImplementedError, match="dbs"):
        ens.decode([enc, enc], sample_method="dbs")
    with pytest.raises(ValueError, match="beam sizes"):
        ens.decode([enc, enc], sample_method="beam", beam_size=9)


def test_hf_wrapper_takes_an_ensemble():
    from audiocaption_amd.hf_wrapper import CaptioningModel
    wrapped = CaptioningModel(EnsembleModel([_member(), _member()]))
    assert wrapped.config.vocab_size == 50
    assert next(wrapped.model.parameters()).device.type == "cpu"


class _FlaggingEncoder(nn.Module):
    """An encoder that raises ``f16_overflow`` unless it is asked for the split-bf16 tier (as the conv stack does when an
    activation leaves the fp16 range), and says which tier produced its memory through the memory's value."""

    def __init__(self, raises):
        super().__init__()
        self.raises, self.calls = raises, []

    def forward(self, input_dict):
        algo = input_dict.get("conv_algo")
        self.calls.append(algo)
        wide = algo == "bf16x3"
        out = {"attn_emb": torch.full((2, 5, 32), 2.0 if wide else 1.0), "attn_emb_len": torch.tensor([5, 4])}
        if self.raises:
            out["f16_overflow"] = torch.tensor(0 if wide else 1, dtype=torch.int32)
        return out


def test_a_raised_encoder_status_word_reruns_that_encoder_and_decodes_again(monkeypatch):
    """The re-run path of ``forward`` on the CPU: the decode is replaced by a recorder (it needs the device), the encoders
    are stubs.  Only the member whose encoder raised the word is run again, on the tier that cannot raise it, without a
    decode of its own; the ensemble is then decoded a second time from the new memory and that result is returned."""
    dec = lambda: A.TransformerDecoder(emb_dim=64, vocab_size=50, fc_emb_dim=32, attn_emb_dim=32, dropout=0.2, nhead=2,  # noqa: E731
                                       nlayers=1, dim_feedforward=64)
    quiet, loud = _FlaggingEncoder(False), _FlaggingEncoder(True)
    members = [A.TransformerModel(quiet, dec()), A.TransformerModel(loud, dec())]
    for m in members:
        monkeypatch.setattr(m, "forward_decoder", lambda *a, **k: pytest.fail("a member decoded on its own"))
    ens = EnsembleModel(members)
    seen = []

    def fake_decode(encs, **args):
        seen.append(([float(e["attn_emb"][0, 0, 0]) for e in encs], args))
        return {"seq": torch.full((2, 4), len(seen)), "encoder_outputs": list(encs)}

    monkeypatch.setattr(ens, "decode", fake_decode)
    out = ens({"mode": "inference", "wav": torch.zeros(2, 100), "wav_len": [100, 80], "sample_method": "beam", "beam_size": 4,
               "max_length": 4})
    assert quiet.calls == [None] and loud.calls == [None, "bf16x3"]
    assert [s[0] for s in seen] == [[1.0, 1.0], [1.0, 2.0]]
    assert seen[0][1] == seen[1][1] == {"sample_method": "beam", "beam_size": 4, "max_length": 4}
    assert int(out["seq"][0, 0]) == 2 and float(out["encoder_outputs"][1]["attn_emb"][0, 0, 0]) == 2.0
    # nothing raised: one pass, one decode
    seen.clear()
    loud.raises = False
    ens({"mode": "inference", "wav": torch.zeros(2, 100), "wav_len": [100, 80]})
    assert len(seen) == 1 and loud.calls[-1] is None
