from t2ms_amd.model.denoiser.mytransformer import *  # noqa: F401,F403
