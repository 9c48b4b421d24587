from t2ms_amd.model.pretrained.tsae import (PositionalEncoding, AdaLN, TimeSeriesEncoder, AdaptiveLinear,  # noqa: F401
                                            ConditionFusionModule, TimeSeriesDecoder, AttentionSeq2SeqAutoencoder)
