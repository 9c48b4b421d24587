from t2ms_amd.model.pretrained.myvqvae import Residual, ResidualStack, Encoder, Decoder, vqvae  # noqa: F401
