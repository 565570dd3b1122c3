"""The reference's Hugging Face call surface on the MI355X path.

``Effb2TrmConfig`` / ``Effb2TrmCaptioningModel`` mirror ``captioning.models.hf_wrapper`` (hf_wrapper.py:1115-1181): the same
config keys and defaults, the same module tree -

    Effb2TrmCaptioningModel.model        ContraEncoderKdWrapper   (hf_wrapper.py:1071-1112; kd_wrapper.py here)
        .model                           TransformerModel(EfficientNetB2(), TransformerDecoder(tie_weights=True))
        .stdnt_proj / .tchr_proj / .logit_scale     knowledge-distillation heads: in the checkpoint, unused at inference

- hence the same ``state_dict()`` keys as the published ``wsntxxn/effb2-trm-audio-captioning`` weights
(``model.model.encoder.backbone.eff_net._conv_stem.weight`` ..., ``model.stdnt_proj.weight``, ``model.logit_scale``), and
the same call: ``model(audio, audio_length, sample_method="beam", beam_size=3, max_length=20, temp=1.0)`` returning a CPU
LongTensor (B, max_length); ``model.config.sample_rate`` is what callers resample to (README.md:35).

With ``transformers`` importable the two classes ARE a ``PretrainedConfig`` / ``PreTrainedModel`` (``from_pretrained`` /
``save_pretrained`` work on a local directory); without it they fall back to plain classes with ``load_checkpoint``.

``Cnn14RnnTempAttnGruConfig`` / ``Cnn14RnnTempAttnGruModel`` mirror hf_wrapper.py:1862-1974 the same way: ``cap_model`` =
``TemporalSeq2SeqAttnModel(Cnn14RnnEncoder, TemporalBahAttnDecoder)`` and ``sed_model`` = ``Cnn8rnnSedModel(447)``, whose
temporal tag (0..3 per clip) the decoder embeds at step 0; the tagger runs first, on the device, then the captioner.

``CaptioningModel`` is the same call surface around ANY model of this package (the reference ships it only for its EffB2
model), so ``demo.py``-style callers can use the Cnn14Rnn-Trm captioner without the input_dict plumbing.
"""
import numpy as np
import torch
import torch.nn as nn

from . import kernels as K
from . import logit_rules
from .attn_model import TemporalSeq2SeqAttnModel
from .cnn_encoder import Cnn14Encoder
from .config import merge_load_state_dict
from .crnn_trm_encoder import Cnn14RnnEncoder
from .effnet_encoder import EfficientNetB2
from .kd_wrapper import ContraEncoderKdWrapper   # noqa: F401 - hf_wrapper.py:1071-1112 defines it here; kd_wrapper.py holds all three
from .mel import MelSpectrogramBuffers, MelTables
from .rnn_decoder import TemporalBahAttnDecoder, check_temporal_tag
from .rnn_encoder import RnnEncoder
from .sed_model import Cnn8rnnSedModel
from .transformer_decoder import TransformerDecoder
from .transformer_model import TransformerModel

try:   # the real base classes when the package is there (it is an optional dependency of the reference as well)
    from transformers import PretrainedConfig, PreTrainedModel
    HAVE_TRANSFORMERS = True
except Exception:   # noqa: BLE001
    HAVE_TRANSFORMERS = False

    class PretrainedConfig:   # minimal stand-ins: attribute bag + nn.Module
        def __init__(self, **kwargs):
            self.__dict__.update(kwargs)

    class PreTrainedModel(nn.Module):
        config_class = None

        def __init__(self, config):
            super().__init__()
            self.config = config

        @property
        def device(self):
            return next(self.parameters()).device

        def post_init(self):
            pass


def _input_dict(device, audio, audio_length, sample_method, beam_size, max_length, temp, rules=None):
    """``rules``: the repetition and word constraints of the call (``logit_rules.KEYS``), passed on when they are set."""
    if not isinstance(audio, torch.Tensor):
        audio = torch.as_tensor(np.asarray(audio))
    d = {"wav": audio.to(device), "wav_len": audio_length, "specaug": False, "mode": "inference",
         "sample_method": sample_method, "max_length": max_length, "temp": temp}
    if sample_method == "beam":
        d["beam_size"] = beam_size
    d.update(rules or {})
    return d


def _rules(repetition_penalty, no_repeat_ngram_size, bad_words, min_length):
    """The four controls of a call as ``input_dict`` keys; the defaults (off) add none."""
    given = {"repetition_penalty": repetition_penalty, "no_repeat_ngram_size": no_repeat_ngram_size, "bad_words": bad_words,
             "min_length": min_length}
    return {k: v for k, v in given.items() if logit_rules.first_active_key({k: v}) is not None}


class Effb2TrmConfig(PretrainedConfig):
    """hf_wrapper.py:1115-1141: same keys, same defaults."""
    model_type = "effb2_trm_captioning"

    def __init__(self, sample_rate=16000, tchr_dim=768, shared_dim=1024, fc_emb_dim=1408, attn_emb_dim=1408,
                 decoder_n_layers=2, decoder_we_tie_weights=True, decoder_emb_dim=256, decoder_dropout=0.2,
                 vocab_size=4981, **kwargs):
        self.sample_rate = sample_rate
        self.tchr_dim = tchr_dim
        self.shared_dim = shared_dim
        self.fc_emb_dim = fc_emb_dim
        self.attn_emb_dim = attn_emb_dim
        self.decoder_n_layers = decoder_n_layers
        self.decoder_we_tie_weights = decoder_we_tie_weights
        self.decoder_emb_dim = decoder_emb_dim
        self.decoder_dropout = decoder_dropout
        self.vocab_size = vocab_size
        super().__init__(**kwargs)


class Effb2TrmCaptioningModel(PreTrainedModel):
    """hf_wrapper.py:1144-1181."""
    config_class = Effb2TrmConfig
    base_model_prefix = "model"
    main_input_name = "audio"
    # decoder.classifier.weight IS decoder.word_embedding.weight when decoder_we_tie_weights (transformer_decoder.py:36-37)
    _tied_weights_keys = {"model.model.decoder.classifier.weight": "model.model.decoder.word_embedding.weight"}
    _keys_to_ignore_on_load_missing = [r"melspec_extractor\."]

    def __init__(self, config):
        super().__init__(config)
        encoder = EfficientNetB2()
        decoder = TransformerDecoder(emb_dim=config.decoder_emb_dim, vocab_size=config.vocab_size,
                                     fc_emb_dim=config.fc_emb_dim, attn_emb_dim=config.attn_emb_dim,
                                     dropout=config.decoder_dropout, nlayers=config.decoder_n_layers,
                                     tie_weights=config.decoder_we_tie_weights)
        model = TransformerModel(encoder, decoder)
        self.model = ContraEncoderKdWrapper(model, config.shared_dim, config.tchr_dim)
        if not config.decoder_we_tie_weights:
            self._tied_weights_keys = {}
        self.post_init()

    def tie_weights(self, *args, **kwargs):
        """Called by the HF loaders after the weights are in place (models are built on the meta device there, which
        drops the tie made at construction): the classifier shares the word-embedding matrix again."""
        try:
            super().tie_weights(*args, **kwargs)
        except Exception:   # noqa: BLE001 - the stand-in base class has none; the HF one may reject our key style
            pass
        if getattr(self.config, "decoder_we_tie_weights", False) and hasattr(self, "model"):
            dec = self.model.model.decoder
            dec.classifier.weight = dec.word_embedding.weight

    def _init_weights(self, module):
        """The sub-modules initialise themselves at construction (as the reference's do); nothing is re-drawn here."""

    def load_checkpoint(self, state_dict, strict=True, output_fn=lambda s: None):
        """Load a state dict in the PUBLISHED layout (keys ``model.model.encoder...``, ``model.model.decoder...``,
        ``model.stdnt_proj...``, ``model.tchr_proj...``, ``model.logit_scale``; hf_wrapper.py:1071-1160) or in the layout of
        a bare captioner (``encoder...`` / ``decoder...``: what the reference's trainer saves, run.py:209-216).  ``strict``:
        every key of the module must be present with the right shape (the two torchaudio mel buffers may be absent);
        otherwise the tolerant shape-filtered merge of train_util.py:188-202."""
        if isinstance(state_dict, str):
            state_dict = torch.load(state_dict, map_location="cpu")
        if "model" in state_dict and isinstance(state_dict["model"], dict):
            state_dict = state_dict["model"]
        if not any(k.startswith("model.") for k in state_dict):      # bare captioner -> wrapped names
            state_dict = {"model.model." + k: v for k, v in state_dict.items()}
            own = self.state_dict()
            for k in ("model.stdnt_proj.weight", "model.stdnt_proj.bias", "model.tchr_proj.weight", "model.tchr_proj.bias",
                      "model.logit_scale"):
                state_dict.setdefault(k, own[k])     # the distillation heads are not part of a bare captioner
        if strict:
            return self.load_state_dict(state_dict, strict=True)
        return merge_load_state_dict(state_dict, self, output_fn)

    @torch.no_grad()
    def forward(self, audio, audio_length, sample_method="beam", beam_size=3, max_length=20, temp=1.0,
                repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words=(), min_length=0):
        """The last four: the repetition and word constraints of ``logit_rules`` (default off)."""
        rules = _rules(repetition_penalty, no_repeat_ngram_size, bad_words, min_length)
        return self.model(_input_dict(self.device, audio, audio_length, sample_method, beam_size, max_length, temp,
                                      rules))["seq"].cpu()


class Cnn14RnnTempAttnGruConfig(PretrainedConfig):
    """hf_wrapper.py:1862-1894: same keys, same defaults."""
    model_type = "cnn14rnn_tempattn_gru_captioning"

    def __init__(self, sample_rate=32000, encoder_rnn_bidirectional=True, encoder_rnn_hidden_size=256,
                 encoder_rnn_dropout=0.5, encoder_rnn_num_layers=3, decoder_emb_dim=512, vocab_size=4981, fc_emb_dim=512,
                 attn_emb_dim=512, decoder_rnn_type="GRU", decoder_num_layers=1, decoder_d_model=512, decoder_dropout=0.5,
                 **kwargs):
        self.sample_rate = sample_rate
        self.encoder_rnn_bidirectional = encoder_rnn_bidirectional
        self.encoder_rnn_hidden_size = encoder_rnn_hidden_size
        self.encoder_rnn_dropout = encoder_rnn_dropout
        self.encoder_rnn_num_layers = encoder_rnn_num_layers
        self.decoder_emb_dim = decoder_emb_dim
        self.vocab_size = vocab_size
        self.fc_emb_dim = fc_emb_dim
        self.attn_emb_dim = attn_emb_dim
        self.decoder_rnn_type = decoder_rnn_type
        self.decoder_num_layers = decoder_num_layers
        self.decoder_d_model = decoder_d_model
        self.decoder_dropout = decoder_dropout
        super().__init__(**kwargs)


class Cnn14RnnTempAttnGruModel(PreTrainedModel):
    """hf_wrapper.py:1897-1974.  The state dict has the reference's keys (``cap_model.encoder.cnn...``,
    ``cap_model.encoder.rnn.network...``, ``cap_model.decoder...``, ``sed_model...``) and the two buffers of the top-level
    ``melspec_extractor``, which a checkpoint may or may not carry; the tagger's log-mel is computed from them."""
    config_class = Cnn14RnnTempAttnGruConfig
    main_input_name = "audio"
    _keys_to_ignore_on_load_missing = [r"melspec_extractor\."]

    def __init__(self, config):
        super().__init__(config)
        sr = config.sample_rate
        self.melspec_extractor = MelSpectrogramBuffers(sr, 32 * sr // 1000, 50.0, float({32000: 14000, 16000: 8000}[sr]), 64,
                                                       "slaney", "slaney")
        encoder = Cnn14RnnEncoder(
            Cnn14Encoder(sample_rate=sr),
            RnnEncoder(-1, 2048, 2048, bidirectional=config.encoder_rnn_bidirectional,
                       hidden_size=config.encoder_rnn_hidden_size, dropout=config.encoder_rnn_dropout,
                       num_layers=config.encoder_rnn_num_layers))
        decoder = TemporalBahAttnDecoder(emb_dim=config.decoder_emb_dim, vocab_size=config.vocab_size,
                                         fc_emb_dim=config.fc_emb_dim, attn_emb_dim=config.attn_emb_dim,
                                         rnn_type=config.decoder_rnn_type, num_layers=config.decoder_num_layers,
                                         d_model=config.decoder_d_model, dropout=config.decoder_dropout)
        self.cap_model = TemporalSeq2SeqAttnModel(encoder, decoder)
        self.sed_model = Cnn8rnnSedModel(classes_num=447, sample_rate=sr)
        self._sed_tables = None
        self._sed_tables_key = None
        self.post_init()

    def _init_weights(self, module):
        """The sub-modules initialise themselves at construction (as the reference's do); nothing is re-drawn here."""

    def load_checkpoint(self, state_dict, strict=True, output_fn=lambda s: None):
        """Load a state dict in the published layout (a path, or a dict, possibly under ``"model"``).  ``strict``: every key
        of the module must be present with the right shape (the mel buffers may be absent); otherwise the tolerant
        shape-filtered merge of train_util.py:188-202."""
        if isinstance(state_dict, str):
            state_dict = torch.load(state_dict, map_location="cpu")
        if "model" in state_dict and isinstance(state_dict["model"], dict):
            state_dict = state_dict["model"]
        if strict:
            return self.load_state_dict(state_dict, strict=True)
        return merge_load_state_dict(state_dict, self, output_fn)

    def _tables(self, dev):
        mkey = self.melspec_extractor.key()
        if self._sed_tables is None or self._sed_tables.window.device != dev or self._sed_tables_key != mkey:
            sr = self.config.sample_rate
            cnn = self.cap_model.encoder.cnn
            self._sed_tables = MelTables(sr, cnn.n_fft, cnn.hop_length, cnn.f_min, cnn.f_max, 64, "slaney", "slaney", dev,
                                         window=self.melspec_extractor.spectrogram.window, fb=self.melspec_extractor.mel_scale.fb)
            self._sed_tables_key = mkey
        return self._sed_tables

    def temporal_tags(self, audio, temporal_tag=None):
        """The clips' temporal tags as the reference forms them (hf_wrapper.py:1954-1961): the tagger's, combined with a
        caller's ``temporal_tag`` by element-wise minimum.  int64 on the host - one copy of B integers, which
        ``check_temporal_tag`` wants there anyway."""
        sed_tag = self.sed_model.forward_wav(audio, tables=self._tables(audio.device))
        if temporal_tag is not None:
            mine = K.upload(check_temporal_tag(temporal_tag, audio.shape[0]), audio.device, torch.int32)
            sed_tag = torch.minimum(sed_tag, mine)
        return sed_tag.cpu().long()

    @torch.no_grad()
    def forward(self, audio, audio_length, temporal_tag=None, sample_method="beam", beam_size=3, max_length=20, temp=1.0,
                repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words=(), min_length=0):
        rules = _rules(repetition_penalty, no_repeat_ngram_size, bad_words, min_length)
        logit_rules.refuse(rules, type(self).__name__)     # before the tagger runs: the attention-GRU search has no rules
        d = _input_dict(self.device, audio, audio_length, sample_method, beam_size, max_length, temp)
        d["temporal_tag"] = self.temporal_tags(d["wav"], temporal_tag)
        return self.cap_model(d)["seq"].cpu()


class CaptioningConfig:
    """Minimal stand-in for the HF config object: callers read ``model.config.sample_rate`` (README.md:35)."""

    def __init__(self, sample_rate=32000, vocab_size=4368, **kwargs):
        self.sample_rate = sample_rate
        self.vocab_size = vocab_size
        self.__dict__.update(kwargs)


class CaptioningModel(nn.Module):
    """``model(audio, audio_length)`` around any captioner of this package."""

    def __init__(self, model, config=None):
        super().__init__()
        self.model = model
        self.config = config or CaptioningConfig(vocab_size=model.vocab_size)

    @torch.no_grad()
    def forward(self, audio, audio_length, sample_method="beam", beam_size=3, max_length=20, temp=1.0,
                repetition_penalty=1.0, no_repeat_ngram_size=0, bad_words=(), min_length=0):
        """The last four: the repetition and word constraints of ``logit_rules`` (default off; a model that does not build
        them raises NotImplementedError naming the key)."""
        device = next(self.model.parameters()).device
        rules = _rules(repetition_penalty, no_repeat_ngram_size, bad_words, min_length)
        return self.model(_input_dict(device, audio, audio_length, sample_method, beam_size, max_length, temp,
                                      rules))["seq"].cpu()
