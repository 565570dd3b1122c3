"""MI355X-native audio-captioning forward/decode path (Cnn14Rnn-Trm), behind the plugin API of
wsntxxn/AudioCaption.  See DESIGN.md / INTEGRATION.md."""
from .cnn_encoder import Cnn6Encoder, Cnn10Encoder, Cnn14Encoder
from .config import (cnn6rnn_trm_config, cnn10rnn_trm_config, cnn14rnn_keyword_trm_config, cnn14rnn_trm_config, effb2_trm_config,
                     htsat_trm_config, init_model_from_config)
from .effnet_encoder import EfficientNetB2
from .htsat import Htsat
from .crnn_trm_encoder import Cnn14RnnEncoder, CrnnEncoder
from .rnn_encoder import RnnEncoder
from .transformer_decoder import KeywordProbTransformerDecoder, TransformerDecoder
from .transformer_model import CaptionModel, KeywordCondTransformerModel, TransformerModel
from .rnn_decoder import (BahAttnCatFcDecoder, ConditionalBahAttnDecoder, RnnDecoder, Seq2SeqAttention,
                          SpecificityBahAttnDecoder, TemporalBahAttnDecoder)
from .attn_model import ConditionalSeq2SeqAttnModel, Seq2SeqAttnModel, TemporalSeq2SeqAttnModel
from .loss import SpecificityLossWrapper
from .sed_model import Cnn8rnnSedModel
from .ensemble import EnsembleModel
from .logit_rules import LogitRules
from .rl_model import ScstWrapper
from .cider import Cider
from .caption_metrics import Bleu, Rouge
from .diversity import Diversity
from .kd_loss import SupKdLoss, TokenLevelKdLoss
from .kd_wrapper import ContraEncoderKdWrapper, ContraMseEncoderKdWrapper, MseEncoderKdWrapper

__all__ = ["Cnn14Encoder", "RnnEncoder", "CrnnEncoder", "Cnn14RnnEncoder", "TransformerDecoder",
           "CaptionModel", "TransformerModel", "RnnDecoder", "Seq2SeqAttention", "BahAttnCatFcDecoder", "TemporalBahAttnDecoder",
           "Seq2SeqAttnModel", "TemporalSeq2SeqAttnModel", "ConditionalBahAttnDecoder", "SpecificityBahAttnDecoder",
           "ConditionalSeq2SeqAttnModel", "SpecificityLossWrapper", "Cnn8rnnSedModel", "EnsembleModel", "ScstWrapper", "Cider", "Bleu", "Rouge", "Diversity", "TokenLevelKdLoss", "SupKdLoss",
           "MseEncoderKdWrapper", "ContraEncoderKdWrapper", "ContraMseEncoderKdWrapper", "init_model_from_config", "cnn14rnn_trm_config",
           "KeywordProbTransformerDecoder", "KeywordCondTransformerModel", "cnn14rnn_keyword_trm_config", "LogitRules", "Htsat", "htsat_trm_config",
           "Cnn6Encoder", "Cnn10Encoder", "cnn6rnn_trm_config", "cnn10rnn_trm_config"]
